// pil_resample.hip — Pillow's 8-bit ImagingResample for one axis of a u8 [B,H,W,C] tensor, on the GPU, so the 4x page of the ESRGAN
// upscaler is brought to its final size on the device and only the smaller page crosses PCIe
// (upscaling/esrgan_pytorch.py:546 BILINEAR by ratio / 4; upscaling/common.py:32 and manga_translator.py:629 BICUBIC).
//
// Pillow resamples separably: first horizontally into an 8-bit image, then vertically on that, and skips a pass whose size does
// not change.  One launch of mit_resample_pil_u8 is one such pass; the 8-bit intermediate between the two launches is Pillow's own
// intermediate rounding, so the result is byte-identical to the library (tests/test_pil_resample_gpu.py checks that against the
// real Pillow).  Per output index of the axis the host (imgproc.pil_coeffs) supplies the window {xmin, cnt} and `ksize` 22-bit
// integer coefficients; the output byte is clamp((2^21 + sum src[xmin + x] * k[x]) >> 22, 0, 255) in 32-bit signed arithmetic.
//
// Both passes are HBM-bound byte kernels (every source byte is needed about once, every destination byte written once):
//   vertical    a block owns one output row; its window and coefficients are the same for every lane (scalar loads), lanes run
//               along x * C, four bytes per lane as one 32-bit load / store where W * C is a multiple of 4, single bytes otherwise
//   horizontal  one lane per output pixel, consecutive lanes consecutive pixels of a row: their source windows are neighbouring or
//               overlapping byte ranges of the same cache lines
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;  // Pillow's Resample.c

__device__ __forceinline__ uint32_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// rows of RC = W * C bytes: dst[b, yy, :] = sum_k src[b, ymin + k, :] * coef[yy, k].  VEC = 4: RC % 4 == 0 and both bases 4-byte aligned.
template <int VEC>
__global__ __launch_bounds__(256) void pil_vert_kernel(const uint8_t *__restrict__ src, int H, int64_t RC, uint8_t *__restrict__ dst, int n_out,
                                                       const int *__restrict__ bounds, const int *__restrict__ coef, int ksize) {
    const int64_t row = blockIdx.x;            // b * n_out + yy
    const int yy = (int)(row % n_out);
    const int64_t b = row / n_out;
    int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    ymin = min(max(ymin, 0), H);
    cnt = max(min(min(cnt, ksize), H - ymin), 0);
    const int *k = coef + (int64_t)yy * ksize;
    const uint8_t *s = src + (b * H + ymin) * RC;
    uint8_t *d = dst + row * RC;
    const int64_t n = RC / VEC;
    for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.y * blockDim.x) {
        if (VEC == 4) {
            int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int t = 0; t < cnt; ++t) {
                const uint32_t v = *reinterpret_cast<const uint32_t *>(s + (int64_t)t * RC + 4 * i);
                const int c = k[t];
                a0 += (int)(v & 255u) * c;
                a1 += (int)((v >> 8) & 255u) * c;
                a2 += (int)((v >> 16) & 255u) * c;
                a3 += (int)(v >> 24) * c;
            }
            *reinterpret_cast<uint32_t *>(d + 4 * i) = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
        } else {
            int a = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t) a += (int)s[(int64_t)t * RC + i] * k[t];
            d[i] = (uint8_t)clip8(a);
        }
    }
}

// dst[r, xx, c] = sum_k src[r, xmin + k, c] * coef[xx, k] over R = B * H rows
template <int C>
__global__ __launch_bounds__(256) void pil_horiz_kernel(const uint8_t *__restrict__ src, int64_t R, int W, uint8_t *__restrict__ dst, int n_out,
                                                        const int *__restrict__ bounds, const int *__restrict__ coef, int ksize) {
    const int64_t total = R * n_out;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int xx = (int)(i % n_out);
        const int64_t r = i / n_out;
        int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        xmin = min(max(xmin, 0), W);
        cnt = max(min(min(cnt, ksize), W - xmin), 0);
        const int *k = coef + (int64_t)xx * ksize;
        const uint8_t *s = src + (r * W + xmin) * C;
        int a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const int kc = k[t];
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] += (int)s[(int64_t)t * C + c] * kc;
        }
        uint8_t *d = dst + i * C;
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = (uint8_t)clip8(a[c]);
    }
}

}  // namespace

extern "C" int mit_resample_pil_u8(const uint8_t *src_dev, int B, int H, int W, int C, uint8_t *dst_dev, int n_out, int axis,
                                   const int *bounds_dev, const int *coef_dev, int ksize, void *stream) {
    if (!src_dev || !dst_dev || !bounds_dev || !coef_dev) return mit_set_error("mit_resample_pil_u8: null pointer");
    if (src_dev == dst_dev) return mit_set_error("mit_resample_pil_u8: src and dst must not alias");
    if (B <= 0 || H <= 0 || W <= 0 || n_out <= 0 || ksize <= 0 || (C != 1 && C != 3))
        return mit_set_error("mit_resample_pil_u8: bad shape (C is 1 or 3)");
    if (axis != 0 && axis != 1) return mit_set_error("mit_resample_pil_u8: axis must be 0 (horizontal) or 1 (vertical)");
    hipStream_t st = (hipStream_t)stream;
    if (axis == 0) {
        const int64_t R = (int64_t)B * H, total = R * n_out;
        MitProbeScope probe("pil_horiz_kernel", st, (double)R * C * ((double)W + n_out));
        int64_t g = (total + 255) / 256;
        g = g > 1048576 ? 1048576 : g;
        if (C == 3)
            hipLaunchKernelGGL(pil_horiz_kernel<3>, dim3((unsigned)g), dim3(256), 0, st, src_dev, R, W, dst_dev, n_out, bounds_dev, coef_dev, ksize);
        else
            hipLaunchKernelGGL(pil_horiz_kernel<1>, dim3((unsigned)g), dim3(256), 0, st, src_dev, R, W, dst_dev, n_out, bounds_dev, coef_dev, ksize);
    } else {
        const int64_t RC = (int64_t)W * C, rows = (int64_t)B * n_out;
        if (rows > 2147483647LL) return mit_set_error("mit_resample_pil_u8: B * n_out exceeds the grid");
        MitProbeScope probe("pil_vert_kernel", st, (double)B * RC * ((double)H + n_out));
        const bool vec = RC % 4 == 0 && ((uintptr_t)src_dev & 3) == 0 && ((uintptr_t)dst_dev & 3) == 0;
        int64_t gy = (RC / (vec ? 4 : 1) + 255) / 256;
        gy = gy > 65535 ? 65535 : (gy < 1 ? 1 : gy);
        if (vec)
            hipLaunchKernelGGL(pil_vert_kernel<4>, dim3((unsigned)rows, (unsigned)gy), dim3(256), 0, st, src_dev, H, RC, dst_dev, n_out, bounds_dev,
                               coef_dev, ksize);
        else
            hipLaunchKernelGGL(pil_vert_kernel<1>, dim3((unsigned)rows, (unsigned)gy), dim3(256), 0, st, src_dev, H, RC, dst_dev, n_out, bounds_dev,
                               coef_dev, ksize);
    }
    MIT_CHECK_LAUNCH("mit_resample_pil_u8");
    return 0;
}
