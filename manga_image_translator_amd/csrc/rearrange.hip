// rearrange.hip — the tiling of a webtoon strip around the detector network, on the device: det_rearrange_forward
// (utils/generic.py:876-997) cuts the strip into overlapping bands, lays pw_num bands side by side into squares, and after the
// network stitches the squares' maps back, averaging where consecutive bands overlap.  Geometry (the plan, the band starts) comes
// from the host (rearrange.py), exactly as the host path computes it.  Both kernels move a few bytes per element and are HBM-bound:
// no LDS, no MFMA; the work is keeping the global accesses coalesced.
//
// squares: both plans copy contiguous page-row segments.  Plain plan: row r of square s is, for j < pw_num, the whole page row
// (s*pw_num + j)*ph_step + r.  Transposed plan (wide strip): row j*w + a of square s is page row a, columns [b*ph_step, b*ph_step + patch).
// A thread writes one 16-byte aligned piece of the output; when the piece lies inside one segment it is one 16-byte load (aligned or
// not: w*3 bytes per band row is rarely a multiple of 16) and one aligned 16-byte store, else a byte loop.
//
// stitch: the reference accumulates band after band into the strip's map and, from the second band on, halves the rows a band shares with
// its predecessor right after adding it (generic.py:898-914).  Per output element that is a short recurrence over the bands that cover
// its row, in ascending band order — v += src; v *= 0.5 — which one thread replays in registers: one pass, no atomics, no dependence
// between elements, and bit-identical to the reference's float32 arithmetic (x / 2 == x * 0.5f exactly; no contraction: the add and the
// multiply are separate roundings by __fadd_rn / __fmul_rn).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));   // a 16-byte load from any byte address

struct SquaresGeom {
    int transpose, w, pw_num, ph_num, ph_step, patch;
    int64_t page_row;   // bytes per page row
    int64_t total;      // bytes of the output
};

// Source byte of output byte (row `row` of square `s`, byte `cb` of that row): -1 for the empty bands of the last square.
// *seg_end = the end (byte in the row) of the contiguous segment cb lies in.
__device__ __forceinline__ int64_t squares_src(const SquaresGeom &g, int s, int row, int cb, int *seg_end) {
    if (g.transpose) {
        const int j = row / g.w, a = row - j * g.w;
        const int b = s * g.pw_num + j;
        *seg_end = g.patch * 3;
        return b < g.ph_num ? (int64_t)a * g.page_row + (int64_t)b * g.ph_step * 3 + cb : -1;
    }
    const int wb = g.w * 3;
    const int j = cb / wb;
    const int b = s * g.pw_num + j;
    *seg_end = (j + 1) * wb;
    return b < g.ph_num ? ((int64_t)b * g.ph_step + row) * g.page_row + (cb - j * wb) : -1;
}

__global__ __launch_bounds__(256) void rearrange_squares_kernel(const uint8_t *__restrict__ page, uint8_t *__restrict__ sq, SquaresGeom g) {
    const int64_t o = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (o >= g.total) return;
    const int rowbytes = g.patch * 3;
    int64_t rowidx;   // s * patch + row
    int cb;
    if (g.total < ((int64_t)1 << 32)) {   // uniform: 32-bit division where the output allows it
        const uint32_t r = (uint32_t)o / (uint32_t)rowbytes;
        rowidx = r;
        cb = (int)((uint32_t)o - r * (uint32_t)rowbytes);
    } else {
        rowidx = o / rowbytes;
        cb = (int)(o - rowidx * rowbytes);
    }
    int s = (int)(rowidx / g.patch), row = (int)(rowidx - (int64_t)s * g.patch);
    int seg_end;
    int64_t src = squares_src(g, s, row, cb, &seg_end);
    if (cb + 16 <= seg_end && o + 16 <= g.total) {   // the whole piece inside one segment (a segment never crosses a row)
        u32x4 v = {0u, 0u, 0u, 0u};
        if (src >= 0) {
            const uint8_t *p = page + src;
            v = ((reinterpret_cast<uintptr_t>(p) & 15) == 0) ? *reinterpret_cast<const u32x4 *>(p) : *reinterpret_cast<const u32x4_unaligned *>(p);
        }
        *reinterpret_cast<u32x4 *>(sq + o) = v;
        return;
    }
    const int n = (int)(g.total - o < 16 ? g.total - o : 16);
    for (int k = 0; k < n; ++k) {
        if (cb >= seg_end) {           // next segment, or the next row (of the next square)
            if (cb >= rowbytes) {
                cb = 0;
                if (++row == g.patch) {
                    row = 0;
                    ++s;
                }
            }
            src = squares_src(g, s, row, cb, &seg_end);
        }
        sq[o + k] = src >= 0 ? page[src] : (uint8_t)0;
        if (src >= 0) ++src;
        ++cb;
    }
}

struct StitchGeom {
    int C, m, transpose, pw_num, ph_num, step, pw, hh, ops;
    int64_t sn, sc, sy, sx;
};

// One element of the strip's map: y along the strip (< hh), x across it (< pw).  `starts` is non-decreasing (band p starts at
// round(p * ph_step / h * hh)), so the first band that starts below y ends the walk.
__device__ __forceinline__ float stitch_one(const float *__restrict__ src, const int *__restrict__ starts, const StitchGeom &g, int c, int y,
                                            int x) {
    float v = 0.0f;
    const int psize = g.m;
    for (int p = 0; p < g.ph_num; ++p) {
        const int t = starts[p];
        if (t > y) break;
        const int r = y - t;
        if (r >= psize) continue;
        const int sqi = p / g.pw_num, col = (p - sqi * g.pw_num) * g.pw + x;
        const float *q = src + (int64_t)sqi * g.sn + (int64_t)c * g.sc;
        v = __fadd_rn(v, g.transpose ? q[(int64_t)col * g.sy + (int64_t)r * g.sx] : q[(int64_t)r * g.sy + (int64_t)col * g.sx]);
        if (p > 0 && r < psize - g.step) v = __fmul_rn(v, 0.5f);
    }
    return v;
}

__device__ __forceinline__ uint8_t mask_u8(float v) { return (uint8_t)(int)(v * 255.0f); }   // postprocess_mask (ctd.py:41-44): truncating

// Scalar form, both plans: consecutive threads walk the output's contiguous axis (x for the plain plan, y for the transposed one),
// which is the source's contiguous axis as well.
__global__ __launch_bounds__(256) void rearrange_stitch_kernel(const float *__restrict__ src, const int *__restrict__ starts, float *__restrict__ dst,
                                                               uint8_t *__restrict__ dst_u8, StitchGeom g) {
    const int64_t plane = (int64_t)g.hh * g.pw;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane * g.C) return;
    const int c = (int)(i / plane);
    const int e = (int)(i - (int64_t)c * plane);
    int y, x;
    if (g.transpose) {   // dst [C, pw, hh]
        x = e / g.hh;
        y = e - x * g.hh;
    } else {             // dst [C, hh, pw]
        y = e / g.pw;
        x = e - y * g.pw;
    }
    const float v = stitch_one(src, starts, g, c, y, x);
    dst[i] = v;
    if (g.ops & 1) dst_u8[i] = mask_u8(v);
}

// Plain plan with pw % 4 == 0, unit column stride and 16-byte aligned rows: four consecutive x per thread, 128-bit loads and stores.
__global__ __launch_bounds__(256) void rearrange_stitch_x4_kernel(const float *__restrict__ src, const int *__restrict__ starts,
                                                                  float *__restrict__ dst, uint8_t *__restrict__ dst_u8, StitchGeom g) {
    const int pw4 = g.pw >> 2;
    const int64_t plane4 = (int64_t)g.hh * pw4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane4 * g.C) return;
    const int c = (int)(i / plane4);
    const int e = (int)(i - (int64_t)c * plane4);
    const int y = e / pw4, x = (e - y * pw4) * 4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int psize = g.m;
    for (int p = 0; p < g.ph_num; ++p) {
        const int t = starts[p];
        if (t > y) break;
        const int r = y - t;
        if (r >= psize) continue;
        const int sqi = p / g.pw_num, col = (p - sqi * g.pw_num) * g.pw + x;
        const float4 a = *reinterpret_cast<const float4 *>(src + (int64_t)sqi * g.sn + (int64_t)c * g.sc + (int64_t)r * g.sy + col);
        v.x = __fadd_rn(v.x, a.x);
        v.y = __fadd_rn(v.y, a.y);
        v.z = __fadd_rn(v.z, a.z);
        v.w = __fadd_rn(v.w, a.w);
        if (p > 0 && r < psize - g.step) {
            v.x = __fmul_rn(v.x, 0.5f);
            v.y = __fmul_rn(v.y, 0.5f);
            v.z = __fmul_rn(v.z, 0.5f);
            v.w = __fmul_rn(v.w, 0.5f);
        }
    }
    const int64_t o = ((int64_t)c * g.hh + y) * g.pw + x;
    *reinterpret_cast<float4 *>(dst + o) = v;
    if (g.ops & 1) *reinterpret_cast<uchar4 *>(dst_u8 + o) = make_uchar4(mask_u8(v.x), mask_u8(v.y), mask_u8(v.z), mask_u8(v.w));
}

}  // namespace

extern "C" int mit_rearrange_squares(const uint8_t *page_dev, int H, int W, int transpose, int w, int pw_num, int ph_num, int ph_step, int p_num,
                                     uint8_t *sq_dev, void *stream) {
    if (!page_dev || !sq_dev) return mit_set_error("mit_rearrange_squares: null pointer");
    if (H <= 0 || W <= 0 || w <= 0 || pw_num < 1 || ph_num < 1 || ph_step < 0 || p_num < 1)
        return mit_set_error("mit_rearrange_squares: bad plan");
    const int h = transpose ? W : H;
    if (w != (transpose ? H : W)) return mit_set_error("mit_rearrange_squares: the strip width of the plan is not the page's");
    const int64_t patch = (int64_t)pw_num * w;
    if (patch > h || (int64_t)(ph_num - 1) * ph_step + patch > h) return mit_set_error("mit_rearrange_squares: a band ends beyond the strip");
    if ((int64_t)p_num * pw_num < ph_num || (int64_t)(p_num - 1) * pw_num >= ph_num)
        return mit_set_error("mit_rearrange_squares: p_num squares of pw_num bands do not hold ph_num bands");
    if (patch * p_num >= ((int64_t)1 << 31) || patch * 3 >= ((int64_t)1 << 31)) return mit_set_error("mit_rearrange_squares: plan too large");
    SquaresGeom g;
    g.transpose = transpose ? 1 : 0;
    g.w = w, g.pw_num = pw_num, g.ph_num = ph_num, g.ph_step = ph_step, g.patch = (int)patch;
    g.page_row = (int64_t)W * 3;
    g.total = (int64_t)p_num * patch * patch * 3;
    const int64_t pieces = (g.total + 15) / 16;
    if ((pieces + 255) / 256 >= ((int64_t)1 << 31)) return mit_set_error("mit_rearrange_squares: plan too large");
    MitProbeScope probe("rearrange_squares_kernel", (hipStream_t)stream, 2.0 * (double)g.total);
    hipLaunchKernelGGL(rearrange_squares_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, page_dev, sq_dev, g);
    MIT_CHECK_LAUNCH("mit_rearrange_squares");
    return 0;
}

extern "C" int mit_rearrange_stitch(const float *src_dev, int n, int C, int m, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int transpose,
                                    int pw_num, int ph_num, int step, int pw, int hh, const int *starts_dev, float *dst_dev, uint8_t *dst_u8_dev,
                                    int ops, void *stream) {
    if (!src_dev || !dst_dev || !starts_dev) return mit_set_error("mit_rearrange_stitch: null pointer");
    if ((ops & ~1) != 0 || ((ops & 1) && !dst_u8_dev)) return mit_set_error("mit_rearrange_stitch: ops is 0 or 1 (1 needs dst_u8_dev)");
    if (n < 1 || C < 1 || m < 1 || pw_num < 1 || ph_num < 1 || pw < 1 || hh < 1 || step < 0 || step > m)
        return mit_set_error("mit_rearrange_stitch: bad geometry");
    if ((int64_t)pw * pw_num > m) return mit_set_error("mit_rearrange_stitch: pw_num bands of pw columns do not fit a square of side m");
    if ((int64_t)n * pw_num < ph_num) return mit_set_error("mit_rearrange_stitch: n squares hold fewer than ph_num bands");
    if (sn < 0 || sc < 0 || sy < 0 || sx < 0) return mit_set_error("mit_rearrange_stitch: negative stride");
    const int64_t plane = (int64_t)hh * pw;
    if (plane >= ((int64_t)1 << 31)) return mit_set_error("mit_rearrange_stitch: map too large");
    StitchGeom g;
    g.C = C, g.m = m, g.transpose = transpose ? 1 : 0, g.pw_num = pw_num, g.ph_num = ph_num, g.step = step, g.pw = pw, g.hh = hh, g.ops = ops;
    g.sn = sn, g.sc = sc, g.sy = sy, g.sx = sx;
    const bool x4 = !transpose && pw % 4 == 0 && sx == 1 && sn % 4 == 0 && sc % 4 == 0 && sy % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(src_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst_dev) & 15) == 0 &&
                    (!(ops & 1) || (reinterpret_cast<uintptr_t>(dst_u8_dev) & 3) == 0);
    const int64_t threads = x4 ? plane / 4 * C : plane * C;
    if ((threads + 255) / 256 >= ((int64_t)1 << 31)) return mit_set_error("mit_rearrange_stitch: map too large");
    // bytes: every output element is written once and read from at most the bands that cover it (two where bands overlap)
    MitProbeScope probe("rearrange_stitch_kernel", (hipStream_t)stream, (double)plane * C * (8.0 + (ops & 1)));
    if (x4)
        hipLaunchKernelGGL(rearrange_stitch_x4_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_dev, starts_dev,
                           dst_dev, dst_u8_dev, g);
    else
        hipLaunchKernelGGL(rearrange_stitch_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_dev, starts_dev,
                           dst_dev, dst_u8_dev, g);
    MIT_CHECK_LAUNCH("mit_rearrange_stitch");
    return 0;
}
