// aot_kernels.hip — the memory-bound pieces of the AOT inpainter (the reference's ``Inpainter.default``): the u8 page / mask
// -> [-1, 1] network input, the gate of every gated layer, the per-plane statistics of my_layer_norm, the AOT blend and the
// last gated layer fused with clip, the u8 conversion and the composite.  The convolutions themselves run on mit_conv_gemm.
//
// Reference: manga_translator/inpainting/inpainting_aot.py
//   GatedWSConvPadded.forward :128-133, GatedWSTransposeConvPadded.forward :142-146, relu_nf :35-36,
//   my_layer_norm :163-168, AOTBlock.forward :187-193, AOTGenerator.forward :266-274;
// and the plugin path it inherits, inpainting_lama_mpe.py:_infer :82-117.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

constexpr float RELU_NF = 1.7139588594436646f;  // relu_nf :35-36
constexpr int STATS_THREADS = 256;
constexpr int STATS_CHUNK = 512;                // pixels per partial: the partition depends on h * w only, never on B

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

inline int grid_for(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    return (int)(g > 256 * 16 ? 256 * 16 : (g < 1 ? 1 : g));
}

// ---- (1) u8 page + u8 mask -> fp32 [B,H,W,4] = (m, (rgb / 127.5 - 1) * (1 - m)),  m = (mask / 255 >= 0.5) ----
__global__ void aot_prep_kernel(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask, float4 *__restrict__ out,
                                int64_t npix) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < npix; i += stride) {
        const float m = ((float)mask[i] / 255.0f >= 0.5f) ? 1.f : 0.f;  // inpainting_lama_mpe.py:85-87
        const float k = 1.f - m;
        float4 v;
        v.x = m;                                                        // torch.cat([mask, img]) :266
        v.y = ((float)img[3 * i + 0] / 127.5f - 1.0f) * k;              // :84, img_torch *= (1 - mask) :92
        v.z = ((float)img[3 * i + 1] / 127.5f - 1.0f) * k;
        v.w = ((float)img[3 * i + 2] / 127.5f - 1.0f) * k;
        out[i] = v;
    }
}

// ---- (2) [.., 2C] (signal | gate) -> [.., C]: signal * sigmoid(gate) * 1.8 (+ relu_nf) ----
__global__ void aot_gate_kernel(const float *__restrict__ in, int64_t in_ps, float *__restrict__ out, int64_t out_ps, int64_t npix,
                                int C, int relu_nf) {
    const int q4 = C >> 2;
    const int64_t total = npix * q4;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int64_t p = i / q4;
        const int c = (int)(i - p * q4) * 4;
        const float4 s = *reinterpret_cast<const float4 *>(in + p * in_ps + c);
        const float4 g = *reinterpret_cast<const float4 *>(in + p * in_ps + C + c);
        float4 v;
        v.x = s.x * sigmoid_f(g.x) * 1.8f;   // signal * gate * 1.8 :133
        v.y = s.y * sigmoid_f(g.y) * 1.8f;
        v.z = s.z * sigmoid_f(g.z) * 1.8f;
        v.w = s.w * sigmoid_f(g.w) * 1.8f;
        if (relu_nf) {
            v.x = fmaxf(v.x, 0.f) * RELU_NF;
            v.y = fmaxf(v.y, 0.f) * RELU_NF;
            v.z = fmaxf(v.z, 0.f) * RELU_NF;
            v.w = fmaxf(v.w, 0.f) * RELU_NF;
        }
        *reinterpret_cast<float4 *>(out + p * out_ps + c) = v;
    }
}

// ---- (3) plane statistics: partial sums of (x - shift) and (x - shift)^2 per (b, chunk, c), in double, fixed-order tree ----
// grid (nchunks, B), STATS_THREADS threads: C / 4 channel quads x (STATS_THREADS / (C / 4)) pixel lanes.
__global__ void __launch_bounds__(STATS_THREADS) aot_stats_partial_kernel(const float *__restrict__ x, int64_t bs, int64_t ps, int hw, int C,
                                                                        const float *__restrict__ shift, double *__restrict__ part) {
    __shared__ double red[2][STATS_THREADS][4];
    const int q4 = C >> 2, lanes = STATS_THREADS / q4;
    const int t = threadIdx.x, q = t % q4, lane = t / q4;
    const int b = blockIdx.y, k = blockIdx.x, nchunks = gridDim.x;
    const int p0 = k * STATS_CHUNK, p1 = min(hw, p0 + STATS_CHUNK);
    float4 sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (shift) sh = *reinterpret_cast<const float4 *>(shift + (int64_t)b * C + 4 * q);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    const float *xb = x + (int64_t)b * bs + 4 * q;
    for (int p = p0 + lane; p < p1; p += lanes) {
        const float4 v = *reinterpret_cast<const float4 *>(xb + (int64_t)p * ps);
        const double d0 = (double)v.x - sh.x, d1 = (double)v.y - sh.y, d2 = (double)v.z - sh.z, d3 = (double)v.w - sh.w;
        s0 += d0; s1 += d1; s2 += d2; s3 += d3;
        t0 += d0 * d0; t1 += d1 * d1; t2 += d2 * d2; t3 += d3 * d3;
    }
    red[0][t][0] = s0; red[0][t][1] = s1; red[0][t][2] = s2; red[0][t][3] = s3;
    red[1][t][0] = t0; red[1][t][1] = t1; red[1][t][2] = t2; red[1][t][3] = t3;
    __syncthreads();
    for (int off = lanes >> 1; off > 0; off >>= 1) {   // pairwise over the lanes, always in the same order
        if (lane < off) {
            const int o = t + off * q4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                red[0][t][j] += red[0][o][j];
                red[1][t][j] += red[1][o][j];
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        double *dst = part + (((int64_t)b * nchunks + k) * C + 4 * q) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dst[2 * j] = red[0][t][j];
            dst[2 * j + 1] = red[1][t][j];
        }
    }
}

// grid B, C threads: the chunks in index order.  final == 0: mean = S / n.  final == 1 (shift = that mean): the mean corrected by
// the residual sum, the unbiased std of the plane and 1 / (std + 1e-9) (my_layer_norm :164-165).
__global__ void aot_stats_final_kernel(const double *__restrict__ part, int nchunks, int C, int hw, const float *__restrict__ shift,
                                       float *__restrict__ mean, float *__restrict__ istd) {
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    double S = 0, SS = 0;
    for (int k = 0; k < nchunks; ++k) {
        const double *src = part + (((int64_t)b * nchunks + k) * C + c) * 2;
        S += src[0];
        SS += src[1];
    }
    const double n = (double)hw;
    if (!shift) {
        mean[(int64_t)b * C + c] = (float)(S / n);
        return;
    }
    const double dm = S / n;
    const double var = fmax((SS - S * dm) / (n - 1.0), 0.0);
    const float sd = (float)sqrt(var);
    mean[(int64_t)b * C + c] = (float)((double)shift[(int64_t)b * C + c] + dm);
    istd[(int64_t)b * C + c] = 1.f / (sd + 1e-9f);
}

// ---- (4) AOT blend, in place over x: m = sigmoid(5 * (2 * (g - mean) * istd - 1)); x = x * (1 - m) + fuse * m ----
__global__ void aot_blend_kernel(float *__restrict__ x, int64_t x_bs, int64_t x_ps, const float *__restrict__ f, int64_t f_bs, int64_t f_ps,
                                 const float *__restrict__ g, int64_t g_bs, int64_t g_ps, const float *__restrict__ mean,
                                 const float *__restrict__ istd, int B, int hw, int C) {
    const int q4 = C >> 2;
    const int64_t per_b = (int64_t)hw * q4, total = per_b * B;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int b = (int)(i / per_b);
        const int64_t r = i - b * per_b;
        const int64_t p = r / q4;
        const int c = (int)(r - p * q4) * 4;
        float4 *xp = reinterpret_cast<float4 *>(x + b * x_bs + p * x_ps + c);
        const float4 xv = *xp;
        const float4 fv = *reinterpret_cast<const float4 *>(f + b * f_bs + p * f_ps + c);
        const float4 gv = *reinterpret_cast<const float4 *>(g + b * g_bs + p * g_ps + c);
        const float4 mu = *reinterpret_cast<const float4 *>(mean + (int64_t)b * C + c);
        const float4 is = *reinterpret_cast<const float4 *>(istd + (int64_t)b * C + c);
        const float m0 = sigmoid_f(5.f * (2.f * (gv.x - mu.x) * is.x - 1.f));   // my_layer_norm :166-167, sigmoid :191
        const float m1 = sigmoid_f(5.f * (2.f * (gv.y - mu.y) * is.y - 1.f));
        const float m2 = sigmoid_f(5.f * (2.f * (gv.z - mu.z) * is.z - 1.f));
        const float m3 = sigmoid_f(5.f * (2.f * (gv.w - mu.w) * is.w - 1.f));
        float4 o;
        o.x = xv.x * (1.f - m0) + fv.x * m0;                                     // x * (1 - mask) + out * mask :192
        o.y = xv.y * (1.f - m1) + fv.y * m1;
        o.z = xv.z * (1.f - m2) + fv.z * m2;
        o.w = xv.w * (1.f - m3) + fv.w * m3;
        *xp = o;
    }
}

// ---- (5) last gated layer (3 signal | 3 gate columns) -> clip -> (x + 1) * 127.5 truncated to u8 -> composite ----
__global__ void aot_post_kernel(const float *__restrict__ pre, int64_t pre_ps, const uint8_t *__restrict__ img,
                                const uint8_t *__restrict__ mask, uint8_t *__restrict__ out, float *__restrict__ preclip, int64_t npix,
                                int composite) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < npix; i += stride) {
        const uint8_t mk = mask[i];
        const bool keep_inpainted = !composite || mk >= 127;  // mask_original :57-61 (composite == 0: img_inpainted itself, :114)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = pre[i * pre_ps + c], g = pre[i * pre_ps + 3 + c];
            float v = s * sigmoid_f(g) * 1.8f;                    // tail[8] :133
            if (preclip) preclip[3 * i + c] = v;
            v = fminf(fmaxf(v, -1.f), 1.f);                       // torch.clip(x, -1, 1) :274
            const uint8_t q = (uint8_t)(int)((v + 1.0f) * 127.5f); // astype(np.uint8): truncation :114
            out[3 * i + c] = keep_inpainted ? q : img[3 * i + c]; // :117
        }
    }
}

}  // namespace

extern "C" int mit_aot_prep(const uint8_t *img_dev, const uint8_t *mask_dev, float *out_dev, int B, int H, int W, void *stream) {
    if (!img_dev || !mask_dev || !out_dev) return mit_set_error("mit_aot_prep: null pointer");
    if (B <= 0 || H <= 0 || W <= 0) return mit_set_error("mit_aot_prep: empty page");
    if (reinterpret_cast<uintptr_t>(out_dev) & 15) return mit_set_error("mit_aot_prep: output must be 16-byte aligned");
    const int64_t npix = (int64_t)B * H * W;
    MitProbeScope probe("aot_prep_kernel", (hipStream_t)stream, (double)npix * (3 + 1 + 16));
    hipLaunchKernelGGL(aot_prep_kernel, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, img_dev, mask_dev,
                       reinterpret_cast<float4 *>(out_dev), npix);
    MIT_CHECK_LAUNCH("mit_aot_prep");
    return 0;
}

extern "C" int mit_aot_gate(const float *in_dev, int64_t in_pixstride, float *out_dev, int64_t out_pixstride, int64_t npix, int C,
                            int relu_nf, void *stream) {
    if (!in_dev || !out_dev) return mit_set_error("mit_aot_gate: null pointer");
    if (npix <= 0 || C <= 0 || (C & 3)) return mit_set_error("mit_aot_gate: C must be a positive multiple of 4 (got %d)", C);
    if (in_pixstride < 2 * C || out_pixstride < C || (in_pixstride & 3) || (out_pixstride & 3))
        return mit_set_error("mit_aot_gate: pixel strides must be multiples of 4 and hold 2C (in) / C (out) channels");
    if ((reinterpret_cast<uintptr_t>(in_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return mit_set_error("mit_aot_gate: operands must be 16-byte aligned");
    MitProbeScope probe("aot_gate_kernel", (hipStream_t)stream, (double)npix * C * 12);
    hipLaunchKernelGGL(aot_gate_kernel, dim3(grid_for(npix * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_pixstride,
                       out_dev, out_pixstride, npix, C, relu_nf);
    MIT_CHECK_LAUNCH("mit_aot_gate");
    return 0;
}

extern "C" int64_t mit_aot_plane_stats_ws(int B, int hw, int C) {
    if (B <= 0 || hw <= 0 || C <= 0) return 0;
    return (int64_t)B * ((hw + STATS_CHUNK - 1) / STATS_CHUNK) * C * 2 * (int64_t)sizeof(double);
}

extern "C" int mit_aot_plane_stats(const float *x_dev, int64_t batch_stride, int64_t pixstride, int B, int hw, int C, void *ws_dev,
                                   int64_t ws_bytes, float *mean_dev, float *istd_dev, void *stream) {
    if (!x_dev || !ws_dev || !mean_dev || !istd_dev) return mit_set_error("mit_aot_plane_stats: null pointer");
    if (B <= 0 || hw < 2) return mit_set_error("mit_aot_plane_stats: need B >= 1 and at least 2 pixels per plane");
    if (C < 4 || C > 4 * STATS_THREADS || (C & (C - 1))) return mit_set_error("mit_aot_plane_stats: C must be a power of two in [4, 1024] (got %d)", C);
    if (pixstride < C || (pixstride & 3) || (batch_stride & 3) || batch_stride < (int64_t)hw * pixstride)
        return mit_set_error("mit_aot_plane_stats: bad strides");
    if ((reinterpret_cast<uintptr_t>(x_dev) & 15) || (reinterpret_cast<uintptr_t>(mean_dev) & 15) || (reinterpret_cast<uintptr_t>(ws_dev) & 7))
        return mit_set_error("mit_aot_plane_stats: misaligned operand");
    if (ws_bytes < mit_aot_plane_stats_ws(B, hw, C)) return mit_set_error("mit_aot_plane_stats: workspace too small");
    const int nchunks = (hw + STATS_CHUNK - 1) / STATS_CHUNK;
    if (B > 65535) return mit_set_error("mit_aot_plane_stats: B too large");
    hipStream_t s = (hipStream_t)stream;
    double *part = reinterpret_cast<double *>(ws_dev);
    MitProbeScope probe("aot_plane_stats", s, 2.0 * B * hw * C * 4);
    for (int pass = 0; pass < 2; ++pass) {   // pass 0: the mean; pass 1: sums around it (accurate when |mean| >> std)
        const float *sh = pass ? mean_dev : nullptr;
        hipLaunchKernelGGL(aot_stats_partial_kernel, dim3(nchunks, B), dim3(STATS_THREADS), 0, s, x_dev, batch_stride, pixstride, hw, C, sh, part);
        MIT_CHECK_LAUNCH("mit_aot_plane_stats(partial)");
        hipLaunchKernelGGL(aot_stats_final_kernel, dim3(B), dim3(C), 0, s, part, nchunks, C, hw, sh, mean_dev, istd_dev);
        MIT_CHECK_LAUNCH("mit_aot_plane_stats(final)");
    }
    return 0;
}

extern "C" int mit_aot_blend(float *x_dev, int64_t x_bs, int64_t x_ps, const float *fuse_dev, int64_t f_bs, int64_t f_ps,
                             const float *gate_dev, int64_t g_bs, int64_t g_ps, const float *mean_dev, const float *istd_dev, int B, int hw,
                             int C, void *stream) {
    if (!x_dev || !fuse_dev || !gate_dev || !mean_dev || !istd_dev) return mit_set_error("mit_aot_blend: null pointer");
    if (B <= 0 || hw <= 0 || C <= 0 || (C & 3)) return mit_set_error("mit_aot_blend: C must be a positive multiple of 4");
    if ((x_bs | x_ps | f_bs | f_ps | g_bs | g_ps) & 3) return mit_set_error("mit_aot_blend: strides must be multiples of 4");
    if (x_ps < C || f_ps < C || g_ps < C) return mit_set_error("mit_aot_blend: pixel strides must hold C channels");
    if ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(fuse_dev) | reinterpret_cast<uintptr_t>(gate_dev) |
         reinterpret_cast<uintptr_t>(mean_dev) | reinterpret_cast<uintptr_t>(istd_dev)) & 15)
        return mit_set_error("mit_aot_blend: operands must be 16-byte aligned");
    const int64_t total = (int64_t)B * hw * (C / 4);
    MitProbeScope probe("aot_blend_kernel", (hipStream_t)stream, (double)B * hw * C * 16);
    hipLaunchKernelGGL(aot_blend_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x_dev, x_bs, x_ps, fuse_dev, f_bs, f_ps,
                       gate_dev, g_bs, g_ps, mean_dev, istd_dev, B, hw, C);
    MIT_CHECK_LAUNCH("mit_aot_blend");
    return 0;
}

extern "C" int mit_aot_post(const float *pre_dev, int64_t pre_pixstride, const uint8_t *img_dev, const uint8_t *mask_dev, uint8_t *out_dev,
                            float *preclip_dev, int B, int H, int W, int composite, void *stream) {
    if (!pre_dev || !img_dev || !mask_dev || !out_dev) return mit_set_error("mit_aot_post: null pointer");
    if (B <= 0 || H <= 0 || W <= 0) return mit_set_error("mit_aot_post: empty page");
    if (pre_pixstride < 6) return mit_set_error("mit_aot_post: the input holds 3 signal + 3 gate channels per pixel");
    const int64_t npix = (int64_t)B * H * W;
    MitProbeScope probe("aot_post_kernel", (hipStream_t)stream, (double)npix * (24 + 3 + 1 + 3));
    hipLaunchKernelGGL(aot_post_kernel, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, pre_dev, pre_pixstride, img_dev, mask_dev,
                       out_dev, preclip_dev, npix, composite);
    MIT_CHECK_LAUNCH("mit_aot_post");
    return 0;
}
