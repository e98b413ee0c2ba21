// det_filters.hip — the page filters CommonDetector.detect puts around every detector, on the device.
//
// Reference: manga_translator/detection/common.py:12-64 (detect: rotate, border, invert, gamma before the network; border and rotation
// removed from the masks after it), :71-79 (_add_border: zeros, page at the top left), :101-102 (_add_rotation: np.rot90(image, k=-1)),
// :104-107 (_remove_rotation: np.rot90 of both masks), :115-116 (_add_inversion: cv2.bitwise_not), :118-124 (_add_gamma_correction).
// The host statements are det_filters.apply_host / undo_host; these kernels give their bytes.
//
// Order (common.py:24-35): rotation, border, inversion, gamma.  The border is therefore part of what is inverted (it becomes 255), of the
// gray mean the gamma exponent is computed from, and of what goes through the gamma table.  Everything here is bytes and integers: the
// gamma table itself (256 bytes a page) is made on the host by the reference's own numpy statement from the exact integer gray sum
// (det_filters.gamma_lut), so nothing of np.power is restated.
//
// A rotation is a transpose: it goes through an LDS tile of 32 x 32 pixels, one pixel per 32-bit word, rows padded to 33 words.  A wave
// writes the tile along a row (consecutive words) and reads it along a column (stride 33 words: 33 is odd, so the 32 lanes of a half wave
// fall on 32 different banks) — both the global reads and the global writes run along image rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

constexpr int TILE = 32;          // pixels per tile side
constexpr int TILE_LD = TILE + 1; // words per tile row in LDS
constexpr int MAX_SIDE = 32768;   // side^2 * 3 stays far inside 63 bits, and a grid dimension inside 65535 tiles

// cv2.COLOR_BGR2GRAY in the project's fixed-point form (hostglue.py, csrc/ctd_refine.hip)
__device__ __forceinline__ unsigned gray_of(unsigned c0, unsigned c1, unsigned c2) {
    return (c0 * 1868u + c1 * 9617u + c2 * 4899u + 8192u) >> 14;
}

// sums[b] += gray of every (inverted) pixel of page b; block (0, b) adds the border's share, 255 a pixel under inversion.
__global__ __launch_bounds__(256) void gray_sum_kernel(const uint8_t *__restrict__ src, int64_t P, int invert, unsigned long long border,
                                                       unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long part[4];
    const uint8_t *page = src + (int64_t)blockIdx.y * P * 3;
    const unsigned x = invert ? 255u : 0u;
    unsigned long long acc = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *q = page + p * 3;
        acc += gray_of(q[0] ^ x, q[1] ^ x, q[2] ^ x);   // 255 - v == v ^ 255 on a byte
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = part[0] + part[1] + part[2] + part[3];
        if (blockIdx.x == 0) s += border;
        atomicAdd(&sums[blockIdx.y], s);
    }
}

__device__ __forceinline__ uint8_t filter_byte(unsigned v, unsigned x, const uint8_t *__restrict__ lut) {
    v ^= x;
    return lut ? lut[v] : (uint8_t)v;
}

// The un-rotated form: dst [B,dh,dw,3] from src [B,H,W,3] at its top left, zero elsewhere, every byte through inversion and the table.
// One thread per four consecutive bytes of a destination page.
__global__ __launch_bounds__(256) void apply_plain_kernel(const uint8_t *__restrict__ src, int H, int W, int dw, int64_t dst_bytes,
                                                          int invert, const uint8_t *__restrict__ lut, uint8_t *__restrict__ dst) {
    const int b = blockIdx.y;
    int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q >= dst_bytes) return;
    const uint8_t *s = src + (int64_t)b * H * W * 3;
    uint8_t *d = dst + (int64_t)b * dst_bytes;
    const uint8_t *t = lut ? lut + b * 256 : nullptr;
    const unsigned x = invert ? 255u : 0u;
    const int row_bytes = dw * 3, src_row_bytes = W * 3;
    int64_t row = q / row_bytes;
    int cb = (int)(q - row * row_bytes);
    const int n = dst_bytes - q < 4 ? (int)(dst_bytes - q) : 4;
    for (int k = 0; k < n; ++k) {
        const unsigned v = (row < H && cb < src_row_bytes) ? s[row * src_row_bytes + cb] : 0u;
        d[q + k] = filter_byte(v, x, t);
        if (++cb == row_bytes) {
            cb = 0;
            ++row;
        }
    }
}

// A quarter turn of the top-left sh x sw window of src (rows of src_ld pixels, C bytes a pixel) into dst [dh,dw] (dense), whose turned
// window is sw x sh at the top left; the rest of dst is the filtered zero.
//   CCW == false (np.rot90(k=-1)): out[i, j] = src[sh - 1 - j, i]
//   CCW == true  (np.rot90(k=1)):  out[i, j] = src[j, sw - 1 - i]
// Block 32 x 8; tile[ty][tx] holds out(i0 + tx, j0 + ty), loaded along source rows, written back along destination rows.
template <int C, bool CCW>
__global__ __launch_bounds__(256) void turn_kernel(const uint8_t *__restrict__ src, int sh, int sw, int64_t src_ld, int64_t src_page,
                                                   int dh, int dw, int invert, const uint8_t *__restrict__ lut,
                                                   uint8_t *__restrict__ dst) {
    __shared__ uint32_t tile[TILE][TILE_LD];
    const int b = blockIdx.z;
    const uint8_t *s = src + (int64_t)b * src_page * C;
    uint8_t *d = dst + (int64_t)b * dh * dw * C;
    const uint8_t *t = lut ? lut + b * 256 : nullptr;
    const unsigned x = invert ? 255u : 0u;
    const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    const int tx = threadIdx.x, ty0 = threadIdx.y;
    for (int ty = ty0; ty < TILE; ty += 8) {
        const int i = i0 + tx, j = j0 + ty;   // the output pixel this word is for
        uint32_t v = 0;
        if (i < sw && j < sh) {
            const int r = CCW ? j : sh - 1 - j, c = CCW ? sw - 1 - i : i;
            const uint8_t *q = s + ((int64_t)r * src_ld + c) * C;
            v = q[0];
            if (C == 3) v |= ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
        tile[ty][tx] = v;
    }
    __syncthreads();
    for (int ty = ty0; ty < TILE; ty += 8) {
        const int i = i0 + ty, j = j0 + tx;
        if (i >= dh || j >= dw) continue;
        const uint32_t v = tile[tx][ty];
        uint8_t *q = d + ((int64_t)i * dw + j) * C;
        q[0] = filter_byte(v & 255u, x, t);
        if (C == 3) {
            q[1] = filter_byte((v >> 8) & 255u, x, t);
            q[2] = filter_byte((v >> 16) & 255u, x, t);
        }
    }
}

// 0 when (B, H, W, side) describe pages this unit takes, else the error already set.
int check_pages(const char *who, int B, int H, int W, int side) {
    if (B <= 0 || H <= 0 || W <= 0) return mit_set_error("%s: sizes must be positive (B %d H %d W %d)", who, B, H, W);
    if (B > 65535) return mit_set_error("%s: at most 65535 pages a call (B %d)", who, B);
    if (H > MAX_SIDE || W > MAX_SIDE || side > MAX_SIDE) return mit_set_error("%s: sides up to %d (H %d W %d side %d)", who, MAX_SIDE, H, W, side);
    if (side < 0 || (side > 0 && side < (H > W ? H : W)))
        return mit_set_error("%s: side %d is smaller than the frame (H %d W %d); 0 means no border", who, side, H, W);
    return 0;
}

}  // namespace

extern "C" int mit_det_filter_gray_sum(const uint8_t *pages_dev, int B, int H, int W, int side, int invert, uint64_t *sums_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!pages_dev || !sums_dev) return mit_set_error("mit_det_filter_gray_sum: null pointer");
    if (int e = check_pages("mit_det_filter_gray_sum", B, H, W, side)) return e;
    if (reinterpret_cast<uintptr_t>(sums_dev) % 8) return mit_set_error("mit_det_filter_gray_sum: the sums must be 8-byte aligned");
    const int64_t P = (int64_t)H * W;
    const unsigned long long border = (side > 0 && invert) ? 255ull * (unsigned long long)((int64_t)side * side - P) : 0ull;
    const int blocks = (int)(mit_div_up(P, 256 * 8) < 1024 ? mit_div_up(P, 256 * 8) : 1024);
    MitProbeScope probe("det_filter_gray_sum", stream, (double)B * P * 3);
    MIT_CHECK_HIP(hipMemsetAsync(sums_dev, 0, (size_t)B * sizeof(uint64_t), stream));
    hipLaunchKernelGGL(gray_sum_kernel, dim3(blocks, B), dim3(256), 0, stream, pages_dev, P, invert, border,
                       reinterpret_cast<unsigned long long *>(sums_dev));
    MIT_CHECK_LAUNCH("mit_det_filter_gray_sum");
    return 0;
}

extern "C" int mit_det_filter_apply(const uint8_t *src_dev, int B, int H, int W, int rotate, int side, int invert, const uint8_t *lut_dev,
                                    uint8_t *dst_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!src_dev || !dst_dev) return mit_set_error("mit_det_filter_apply: null pointer");
    if (int e = check_pages("mit_det_filter_apply", B, H, W, side)) return e;
    if (src_dev == dst_dev) return mit_set_error("mit_det_filter_apply: the filtered page cannot be written over its source");
    const int dh = side > 0 ? side : (rotate ? W : H), dw = side > 0 ? side : (rotate ? H : W);
    MitProbeScope probe("det_filter_apply", stream, (double)B * ((double)H * W + (double)dh * dw) * 3);
    if (rotate) {
        hipLaunchKernelGGL((turn_kernel<3, false>), dim3(mit_div_up(dw, TILE), mit_div_up(dh, TILE), B), dim3(TILE, 8), 0, stream, src_dev, H, W,
                           (int64_t)W, (int64_t)H * W, dh, dw, invert, lut_dev, dst_dev);
    } else {
        const int64_t dst_bytes = (int64_t)dh * dw * 3;
        hipLaunchKernelGGL(apply_plain_kernel, dim3(mit_div_up(dst_bytes, 1024), B), dim3(256), 0, stream, src_dev, H, W, dw, dst_bytes, invert,
                           lut_dev, dst_dev);
    }
    MIT_CHECK_LAUNCH("mit_det_filter_apply");
    return 0;
}

extern "C" int mit_det_unrotate_u8(const uint8_t *maps_dev, int B, int h, int w, int ch, int cw, uint8_t *out_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!maps_dev || !out_dev) return mit_set_error("mit_det_unrotate_u8: null pointer");
    if (B <= 0 || h <= 0 || w <= 0 || ch <= 0 || cw <= 0)
        return mit_set_error("mit_det_unrotate_u8: sizes must be positive (B %d h %d w %d crop %d x %d)", B, h, w, ch, cw);
    if (B > 65535) return mit_set_error("mit_det_unrotate_u8: at most 65535 maps a call (B %d)", B);
    if (h > MAX_SIDE || w > MAX_SIDE) return mit_set_error("mit_det_unrotate_u8: sides up to %d (h %d w %d)", MAX_SIDE, h, w);
    if (ch > h || cw > w) return mit_set_error("mit_det_unrotate_u8: the crop %d x %d lies outside the map %d x %d", ch, cw, h, w);
    if (maps_dev == out_dev) return mit_set_error("mit_det_unrotate_u8: the turned map cannot be written over its source");
    MitProbeScope probe("det_unrotate_u8", stream, (double)B * ch * cw * 2);
    // out [B,cw,ch]: out[i, j] = m[j, cw - 1 - i]
    hipLaunchKernelGGL((turn_kernel<1, true>), dim3(mit_div_up(ch, TILE), mit_div_up(cw, TILE), B), dim3(TILE, 8), 0, stream, maps_dev, ch, cw,
                       (int64_t)w, (int64_t)h * w, cw, ch, 0, static_cast<const uint8_t *>(nullptr), out_dev);
    MIT_CHECK_LAUNCH("mit_det_unrotate_u8");
    return 0;
}
