// dbnet_tail.hip — the tail of DefaultDetector._infer (detection/default.py:89-95) after the network: the float text mask goes through
// cv2.resize(mask, (2w, 2h), INTER_LINEAR), the padding is cropped off and the result becomes bytes, np.clip(m * 255, 0, 255).astype(uint8).
// One pass on the device, so that a DBNet raw mask never visits the host: 4 bytes read per source element, 1 byte written per output.
//
// Arithmetic (plugins._resize2x_f32 is the numpy statement of it; this kernel gives its bytes): float data takes OpenCV's unquantised
// bilinear path.  The tap of output index i sits at (i + 0.5) * 0.5 - 0.5, so
//   i == 0                 -> source 0 with weights 1 / 0            (the tap is left of the first centre: clamped)
//   i == 2k     (k >= 1)   -> sources k-1, k with weights 0.25 / 0.75
//   i == 2k + 1 (k < n-1)  -> sources k, k+1 with weights 0.75 / 0.25
//   i == 2n - 1            -> source n-1 with weights 1 / 0          (right of the last centre: clamped)
// HORIZONTAL pass first, r = m[x0] * wx0 + m[x1] * wx1 as two rounded fp32 products and one rounded sum (the unit is built with
// -ffp-contract=off: no FMA), then the vertical pass the same way on those sums, then v * 255.0f, clamp to [0, 255], truncate.
//
// Layout: one lane owns one 4-byte-ALIGNED word of an output row and writes it with one 32-bit store; the lanes of a wave own
// consecutive words of one row.  A row of `ow` bytes starts wherever (b * oh + y) * ow puts it, so the first and the last word of a row
// may belong to it only in part: those lanes write their bytes one by one and touch nothing outside the row.  With `mis` = the row's
// start address & 3, lane t covers columns 4t - mis .. 4t - mis + 3; their sources are the columns kb .. kb + 3 with
// kb = floor((4t - mis - 1) / 2) (three of them when mis is odd), from two source rows, clamped into the map.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

// Weights of output index i along an axis of n source elements: (w_lo, w_hi) for the sources floor((i - 1) / 2) and that + 1, both
// clamped into [0, n - 1] by the caller.  At a border both clamp to the same element and the weights are 1 / 0.
__device__ __forceinline__ void tap_weights(int i, int n, float &w_lo, float &w_hi) {
    const bool odd = i & 1;
    const bool edge = odd ? (i >> 1) >= n - 1 : i == 0;
    w_lo = edge ? 1.0f : (odd ? 0.75f : 0.25f);
    w_hi = edge ? 0.0f : (odd ? 0.25f : 0.75f);
}

// MIS_ODD: the row starts at an odd address, i.e. the word's first column 4t - mis is odd.  Column c0 + p then reads the registers
// (p + 1) / 2 and (p + 1) / 2 + 1 of the loaded run when c0 is even (run starts at c0 / 2 - 1), p / 2 and p / 2 + 1 when it is odd.
// INTERIOR: none of the four columns is the first or the last of the 2x map, so the horizontal weights follow from the parity alone.
template <bool MIS_ODD, bool INTERIOR>
__device__ __forceinline__ void tail_word(const float *__restrict__ r0, const float *__restrict__ r1, int w, int ow, float wy0, float wy1,
                                          int c0, uint8_t *__restrict__ dst_word) {
    const int kb = MIS_ODD ? (c0 - 1) >> 1 : (c0 >> 1) - 1;   // floor((c0 - 1) / 2) for either parity (c0 may be as low as -3)
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = min(max(kb + j, 0), w - 1);
        a[j] = r0[x];
        b[j] = r1[x];
    }
    uint32_t word = 0;
    uint8_t byte[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int lo = MIS_ODD ? p / 2 : (p + 1) / 2;
        float wx0, wx1;
        if (INTERIOR) {
            const bool odd = MIS_ODD != bool(p & 1);              // the parity of column c0 + p
            wx0 = odd ? 0.75f : 0.25f;
            wx1 = odd ? 0.25f : 0.75f;
        } else {
            tap_weights(c0 + p, w, wx0, wx1);
        }
        const float h0 = a[lo] * wx0 + a[lo + 1] * wx1;
        const float h1 = b[lo] * wx0 + b[lo + 1] * wx1;
        float v = (h0 * wy0 + h1 * wy1) * 255.0f;
        v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        byte[p] = (uint8_t)(int)v;
        word |= (uint32_t)byte[p] << (8 * p);
    }
    if (c0 >= 0 && c0 + 3 < ow) {
        *reinterpret_cast<uint32_t *>(dst_word) = word;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (c0 + p >= 0 && c0 + p < ow) dst_word[p] = byte[p];
    }
}

constexpr int TAIL_BLOCK = 128;   // lanes per block: a 1536-byte row is three full blocks

// grid = (word blocks of a row, oh, B); the lanes of a block own consecutive words of one row.
__global__ __launch_bounds__(TAIL_BLOCK) void dbnet_mask_tail_kernel(const float *__restrict__ src, int64_t src_batch_stride,
                                                                     int64_t src_row_stride, int h, int w, uint8_t *__restrict__ out, int oh,
                                                                     int ow) {
    const int t = (int)blockIdx.x * TAIL_BLOCK + threadIdx.x;
    const int y = (int)blockIdx.y;
    const int64_t b = blockIdx.z;
    uint8_t *row_out = out + (b * oh + y) * ow;
    const int mis = (int)(reinterpret_cast<uintptr_t>(row_out) & 3);
    const int c0 = 4 * t - mis;
    if (c0 >= ow) return;
    const int ky = (y - 1) >> 1;                                  // floor((y - 1) / 2): -1 for y == 0
    const int y0 = min(max(ky, 0), h - 1), y1 = min(max(ky + 1, 0), h - 1);
    float wy0, wy1;
    tap_weights(y, h, wy0, wy1);
    const float *r0 = src + b * src_batch_stride + (int64_t)y0 * src_row_stride;
    const float *r1 = src + b * src_batch_stride + (int64_t)y1 * src_row_stride;
    const bool interior = c0 >= 1 && c0 + 3 <= 2 * w - 2;
    if (mis & 1) {
        if (interior) tail_word<true, true>(r0, r1, w, ow, wy0, wy1, c0, row_out + c0);
        else tail_word<true, false>(r0, r1, w, ow, wy0, wy1, c0, row_out + c0);
    } else {
        if (interior) tail_word<false, true>(r0, r1, w, ow, wy0, wy1, c0, row_out + c0);
        else tail_word<false, false>(r0, r1, w, ow, wy0, wy1, c0, row_out + c0);
    }
}

}  // namespace

extern "C" int mit_dbnet_mask_tail(const float *src_dev, int64_t src_batch_stride, int64_t src_row_stride, int B, int h, int w,
                                   uint8_t *out_dev, int oh, int ow, void *stream) {
    if (!src_dev || !out_dev) return mit_set_error("mit_dbnet_mask_tail: null pointer");
    if (B <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return mit_set_error("mit_dbnet_mask_tail: sizes must be positive");
    if (oh > 2 * (int64_t)h || ow > 2 * (int64_t)w)
        return mit_set_error("mit_dbnet_mask_tail: the output (%d x %d) must lie inside the 2x map (%lld x %lld)", oh, ow, 2 * (long long)h,
                             2 * (long long)w);
    if (src_row_stride < w || (B > 1 && src_batch_stride < 0)) return mit_set_error("mit_dbnet_mask_tail: bad source strides");
    // aligned words a row touches: ow / 4 when every row starts on a word boundary, else up to (ow + 6) / 4 (3 bytes of lead, then ow)
    const bool rows_aligned = ow % 4 == 0 && reinterpret_cast<uintptr_t>(out_dev) % 4 == 0;
    const int word_blocks = mit_div_up(rows_aligned ? ow / 4 : ((int64_t)ow + 6) / 4, TAIL_BLOCK);
    if (oh > 65535 || B > 65535) return mit_set_error("mit_dbnet_mask_tail: at most 65535 output rows and 65535 maps a launch (grid y / z)");
    MitProbeScope probe("dbnet_mask_tail_kernel", (hipStream_t)stream, (double)B * (4.0 * h * w + (double)oh * ow));
    hipLaunchKernelGGL(dbnet_mask_tail_kernel, dim3((unsigned)word_blocks, (unsigned)oh, (unsigned)B), dim3(TAIL_BLOCK), 0, (hipStream_t)stream,
                       src_dev, src_batch_stride, src_row_stride, h, w, out_dev, oh, ow);
    MIT_CHECK_LAUNCH("mit_dbnet_mask_tail");
    return 0;
}
