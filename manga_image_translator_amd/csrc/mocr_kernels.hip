// mocr_kernels.hip — the pre-processing kernels of the manga-ocr recogniser, which stand between the rectified line crop and the patch
// projection (manga_ocr's img.convert("L").convert("RGB"), ViTImageProcessor's rescale + normalize, the patch
// convolution's im2col).  Memory-bound, one value per thread.  (mit_layernorm_wide is the decoder's LayerNorm kernel, mocr_decoder.hip.)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

__global__ void mocr_gray_kernel(const uint8_t *__restrict__ rgb, int64_t npix, uint8_t *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < npix; i += stride) {
        const uint32_t r = rgb[3 * i], g = rgb[3 * i + 1], bl = rgb[3 * i + 2];
        const uint8_t l = (uint8_t)((19595u * r + 38470u * g + 7471u * bl + 0x8000u) >> 16);   // Pillow Convert.c, L24 >> 16
        out[3 * i] = l;
        out[3 * i + 1] = l;
        out[3 * i + 2] = l;
    }
}

// out[n][py_blk * G + px_blk][(c * ps + py) * ps + px] = (img[n][py_blk * ps + py][px_blk * ps + px][c] * (1 / 255) - 0.5) / 0.5
__global__ void mocr_patches_kernel(const uint8_t *__restrict__ img, int N, int S, int ps, float *__restrict__ out) {
    const int G = S / ps, cols = 3 * ps * ps;
    const int64_t total = (int64_t)N * G * G * cols;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int col = (int)(i % cols);
        const int64_t p = i / cols;
        const int px = col % ps, py = (col / ps) % ps, c = col / (ps * ps);
        const int gx = (int)(p % G), gy = (int)((p / G) % G);
        const int64_t n = p / ((int64_t)G * G);
        const uint8_t v = img[((n * S + (int64_t)gy * ps + py) * S + (int64_t)gx * ps + px) * 3 + c];
        out[i] = ((float)v * (1.0f / 255.0f) - 0.5f) / 0.5f;
    }
}

int grid1d(int64_t total) { return (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

}  // namespace

extern "C" int mit_mocr_gray(const uint8_t *rgb_dev, int64_t npix, uint8_t *out_dev, void *stream) {
    if (!rgb_dev || !out_dev) return mit_set_error("mit_mocr_gray: null argument");
    if (npix <= 0) return mit_set_error("mit_mocr_gray: npix must be positive");
    hipStream_t s = (hipStream_t)stream;
    MitProbeScope probe("mocr_gray_kernel", s, 6.0 * (double)npix);
    hipLaunchKernelGGL(mocr_gray_kernel, dim3(grid1d(npix)), dim3(256), 0, s, rgb_dev, npix, out_dev);
    MIT_CHECK_LAUNCH("mit_mocr_gray");
    return 0;
}

extern "C" int mit_mocr_patches(const uint8_t *img_dev, int N, int S, int ps, float *out_dev, void *stream) {
    if (!img_dev || !out_dev) return mit_set_error("mit_mocr_patches: null argument");
    if (N <= 0 || S <= 0 || ps <= 0 || S % ps != 0) return mit_set_error("mit_mocr_patches: image size %d is no multiple of the patch size %d", S, ps);
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)N * S * S * 3;
    MitProbeScope probe("mocr_patches_kernel", s, 5.0 * (double)total);
    hipLaunchKernelGGL(mocr_patches_kernel, dim3(grid1d(total)), dim3(256), 0, s, img_dev, N, S, ps, out_dev);
    MIT_CHECK_LAUNCH("mit_mocr_patches");
    return 0;
}
