// dbconvnext_kernels.hip — the two elementwise kernels the dbconvnext detector (DBNet on ConvNeXt) adds to the library:
// LayerNorm over rows up to 1024 wide, and the ConvNeXt block's depthwise 7x7 convolution with its channel LayerNorm in one pass.
// Everything else of that network runs on mit_conv_gemm.
#include "common.h"
#include "../../include/mit_hip.h"

namespace {

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float sum4(const float4 v) { return (v.x + v.y) + (v.z + v.w); }

// Sum over the L lanes of a lane group (L a power of two <= 64, groups aligned to L): xor butterfly, so every lane of the group
// ends with the same value, built in the same order whatever the launch looks like.
template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- LayerNorm over the last dimension of [rows, D], D % 4 == 0, D <= 1024 ------------------------------------------------------
// L lanes own a row (D <= 256: 16, D <= 512: 32, else 64), each lane up to four float4 of it in registers; two passes over the
// registers (mean, then the centred second moment), as torch's CPU kernel does; 256 / L rows per workgroup.
template <int L>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float *__restrict__ in, int64_t in_rs, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ out, int64_t out_rs,
                                                             int64_t rows, int D4, float inv_d, float eps) {
    const int lane = threadIdx.x % L;
    const int64_t row = (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L;
    if (row >= rows) return;  // whole lane groups leave together: the shuffles below stay inside a group
    const float *src = in + row * in_rs;
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c4 = lane + i * L;
        v[i] = c4 < D4 ? ld4(src + c4 * 4) : float4{0.f, 0.f, 0.f, 0.f};
        s += sum4(v[i]);
    }
    const float mean = group_sum<L>(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c4 = lane + i * L;
        v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
        if (c4 < D4) q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float rstd = 1.0f / sqrtf(group_sum<L>(q) * inv_d + eps);
    float *dst = out + row * out_rs;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c4 = lane + i * L;
        if (c4 >= D4) continue;
        const float4 g = ld4(w + c4 * 4), bb = ld4(b + c4 * 4);
        float4 o;
        o.x = v[i].x * rstd * g.x + bb.x; o.y = v[i].y * rstd * g.y + bb.y;
        o.z = v[i].z * rstd * g.z + bb.z; o.w = v[i].w * rstd * g.w + bb.w;
        *reinterpret_cast<float4 *>(dst + c4 * 4) = o;
    }
}

// ---- depthwise 7x7 (zero padding 3) + bias, then LayerNorm over the C channels of each pixel ------------------------------------
// A work item is XT = 4 consecutive output pixels of one image row; C / 4 threads own it, four channels each, so a pixel's channels
// never leave the workgroup and the norm is finished in the same pass.  Per kernel row a thread loads 10 input float4 and 7 weight
// float4 for 28 float4 FMAs; the input halo and the weights come through the caches (49 C floats of weights do not fit LDS beside
// anything else from C = 256 on, and every workgroup reads the same ones).  C / 4 <= 64 lanes reduce by shuffles alone; wider
// pixels take one LDS exchange between their 2 or 4 waves, summed in wave order by every thread.
constexpr int DW_XT = 4;

template <int C>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const float *__restrict__ x, int64_t xs, const float *__restrict__ w,
                                                         const float *__restrict__ bdw, const float *__restrict__ g,
                                                         const float *__restrict__ b, float eps, float *__restrict__ out, int64_t os,
                                                         int H, int W, int WG, int64_t items) {
    constexpr int C4 = C / 4;                       // threads per work item
    constexpr int L = C4 < 64 ? C4 : 64;            // lanes of one wave that belong to the same item
    constexpr int NW = C4 / L;                      // waves per item
    constexpr int IPB = 256 / C4;                   // items per workgroup
    __shared__ float red[2][IPB][NW > 1 ? NW : 1][DW_XT];
    const int c4 = threadIdx.x % C4, it = threadIdx.x / C4;
    const int64_t item = (int64_t)blockIdx.x * IPB + it;
    const bool live = item < items;                 // a dead item still walks through the barriers below
    int x0 = 0, y = 0;
    int64_t img = 0;
    if (live) {
        x0 = (int)(item % WG) * DW_XT;
        const int64_t r = item / WG;
        y = (int)(r % H);
        img = r / H;
    }
    float4 acc[DW_XT];
#pragma unroll
    for (int t = 0; t < DW_XT; ++t) acc[t] = float4{0.f, 0.f, 0.f, 0.f};
    if (live) {
        for (int ky = 0; ky < 7; ++ky) {
            const int yy = y + ky - 3;
            if (yy < 0 || yy >= H) continue;
            const float *row = x + ((img * H + yy) * (int64_t)W) * xs + c4 * 4;
            float4 v[DW_XT + 6];
#pragma unroll
            for (int j = 0; j < DW_XT + 6; ++j) {
                const int xx = x0 + j - 3;
                v[j] = (xx >= 0 && xx < W) ? ld4(row + (int64_t)xx * xs) : float4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float4 ww = ld4(w + (ky * 7 + kx) * C + c4 * 4);
#pragma unroll
                for (int t = 0; t < DW_XT; ++t) {
                    acc[t].x = fmaf(v[t + kx].x, ww.x, acc[t].x); acc[t].y = fmaf(v[t + kx].y, ww.y, acc[t].y);
                    acc[t].z = fmaf(v[t + kx].z, ww.z, acc[t].z); acc[t].w = fmaf(v[t + kx].w, ww.w, acc[t].w);
                }
            }
        }
        const float4 bb = ld4(bdw + c4 * 4);
#pragma unroll
        for (int t = 0; t < DW_XT; ++t) { acc[t].x += bb.x; acc[t].y += bb.y; acc[t].z += bb.z; acc[t].w += bb.w; }
    }
    const int wv = c4 / 64;                         // this thread's wave within the item (NW > 1 only)
    float mean[DW_XT], rstd[DW_XT];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float s[DW_XT];
#pragma unroll
        for (int t = 0; t < DW_XT; ++t) {
            if (pass == 0) {
                s[t] = sum4(acc[t]);
            } else {
                acc[t].x -= mean[t]; acc[t].y -= mean[t]; acc[t].z -= mean[t]; acc[t].w -= mean[t];
                s[t] = (acc[t].x * acc[t].x + acc[t].y * acc[t].y) + (acc[t].z * acc[t].z + acc[t].w * acc[t].w);
            }
            s[t] = group_sum<L>(s[t]);
        }
        if (NW > 1) {
            if (c4 % 64 == 0) {
#pragma unroll
                for (int t = 0; t < DW_XT; ++t) red[pass][it][wv][t] = s[t];
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < DW_XT; ++t) {
                float a = red[pass][it][0][t];
#pragma unroll
                for (int k = 1; k < NW; ++k) a += red[pass][it][k][t];
                s[t] = a;
            }
        }
#pragma unroll
        for (int t = 0; t < DW_XT; ++t) {
            if (pass == 0) mean[t] = s[t] * (1.0f / C);
            else rstd[t] = 1.0f / sqrtf(s[t] * (1.0f / C) + eps);
        }
    }
    if (!live) return;
    const float4 gg = ld4(g + c4 * 4), be = ld4(b + c4 * 4);
    float *dst = out + ((img * H + y) * (int64_t)W + x0) * os + c4 * 4;
#pragma unroll
    for (int t = 0; t < DW_XT; ++t) {
        if (x0 + t >= W) break;
        float4 o;
        o.x = acc[t].x * rstd[t] * gg.x + be.x; o.y = acc[t].y * rstd[t] * gg.y + be.y;
        o.z = acc[t].z * rstd[t] * gg.z + be.z; o.w = acc[t].w * rstd[t] * gg.w + be.w;
        *reinterpret_cast<float4 *>(dst + (int64_t)t * os) = o;
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Widths at which the one-pass form is the faster one on gfx950 (scripts/bench_dbconvnext.py, profiles/r23a_dbconvnext.json).
inline bool dwconv7_ln_fused(int C) { return C == 128 || C == 256 || C == 512 || C == 1024; }

}  // namespace

extern "C" int mit_layernorm_rows(const float *in_dev, int64_t in_rowstride, const float *w_dev, const float *b_dev, float *out_dev,
                                  int64_t out_rowstride, int64_t rows, int D, float eps, void *stream) {
    if (!in_dev || !w_dev || !b_dev || !out_dev) return mit_set_error("mit_layernorm_rows: null pointer");
    if (D <= 0 || D > 1024 || (D & 3)) return mit_set_error("mit_layernorm_rows: D %% 4 == 0 and D <= 1024 required (got %d)", D);
    if ((in_rowstride & 3) || (out_rowstride & 3) || in_rowstride < D || out_rowstride < D)
        return mit_set_error("mit_layernorm_rows: row strides must be multiples of 4 and at least D");
    if (!aligned16(in_dev) || !aligned16(out_dev) || !aligned16(w_dev) || !aligned16(b_dev))
        return mit_set_error("mit_layernorm_rows: pointers must be 16-byte aligned");
    if (rows <= 0) return 0;
    const int L = D <= 256 ? 16 : D <= 512 ? 32 : 64;
    const int64_t blocks = (rows + 256 / L - 1) / (256 / L);
    if (blocks > 0x7fffffff) return mit_set_error("mit_layernorm_rows: too many rows");
    hipStream_t s = (hipStream_t)stream;
    MitProbeScope probe("layernorm_rows_kernel", s, 8.0 * (double)rows * D);
    const dim3 grid((unsigned)blocks), block(256);
    const float inv_d = 1.0f / (float)D;
    switch (L) {
        case 16: hipLaunchKernelGGL(layernorm_rows_kernel<16>, grid, block, 0, s, in_dev, in_rowstride, w_dev, b_dev, out_dev, out_rowstride, rows, D / 4, inv_d, eps); break;
        case 32: hipLaunchKernelGGL(layernorm_rows_kernel<32>, grid, block, 0, s, in_dev, in_rowstride, w_dev, b_dev, out_dev, out_rowstride, rows, D / 4, inv_d, eps); break;
        default: hipLaunchKernelGGL(layernorm_rows_kernel<64>, grid, block, 0, s, in_dev, in_rowstride, w_dev, b_dev, out_dev, out_rowstride, rows, D / 4, inv_d, eps); break;
    }
    MIT_CHECK_LAUNCH("mit_layernorm_rows");
    return 0;
}

extern "C" int mit_dwconv7_ln_supported(int C) { return dwconv7_ln_fused(C) ? 1 : 0; }

extern "C" int mit_dwconv7_ln_nhwc(const float *x_dev, int64_t x_pixstride, const float *w_dev, const float *bdw_dev, const float *g_dev,
                                   const float *b_dev, float eps, float *out_dev, int64_t out_pixstride, int B, int H, int W, int C,
                                   void *stream) {
    if (!x_dev || !w_dev || !bdw_dev || !g_dev || !b_dev || !out_dev) return mit_set_error("mit_dwconv7_ln_nhwc: null pointer");
    if (C != 128 && C != 256 && C != 512 && C != 1024) return mit_set_error("mit_dwconv7_ln_nhwc: C must be 128, 256, 512 or 1024 (got %d)", C);
    if (B <= 0 || H <= 0 || W <= 0) return mit_set_error("mit_dwconv7_ln_nhwc: empty image");
    if ((x_pixstride & 3) || (out_pixstride & 3) || x_pixstride < C || out_pixstride < C)
        return mit_set_error("mit_dwconv7_ln_nhwc: pixel strides must be multiples of 4 and at least C");
    if (!aligned16(x_dev) || !aligned16(out_dev) || !aligned16(w_dev) || !aligned16(bdw_dev) || !aligned16(g_dev) || !aligned16(b_dev))
        return mit_set_error("mit_dwconv7_ln_nhwc: pointers must be 16-byte aligned");
    const int WG = (W + DW_XT - 1) / DW_XT;
    const int64_t items = (int64_t)B * H * WG;
    const int ipb = 256 / (C / 4);
    const int64_t blocks = (items + ipb - 1) / ipb;
    if (blocks > 0x7fffffff) return mit_set_error("mit_dwconv7_ln_nhwc: image too large");
    hipStream_t s = (hipStream_t)stream;
    const double elems = (double)B * H * W * C;
    MitProbeScope probe("dwconv7_ln_kernel", s, 8.0 * elems, 2.0 * 49.0 * elems);
    const dim3 grid((unsigned)blocks), block(256);
#define MIT_DWLN(CC) hipLaunchKernelGGL(dwconv7_ln_kernel<CC>, grid, block, 0, s, x_dev, x_pixstride, w_dev, bdw_dev, g_dev, b_dev, eps, out_dev, out_pixstride, H, W, WG, items)
    switch (C) {
        case 128: MIT_DWLN(128); break;
        case 256: MIT_DWLN(256); break;
        case 512: MIT_DWLN(512); break;
        default: MIT_DWLN(1024); break;
    }
#undef MIT_DWLN
    MIT_CHECK_LAUNCH("mit_dwconv7_ln_nhwc");
    return 0;
}
