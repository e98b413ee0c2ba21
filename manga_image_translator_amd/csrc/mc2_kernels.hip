// mc2_kernels.hip — the manga-colorization-v2 colorizer (the reference's ``Colorizer.mc2``): the grouped 3x3 convolution of the
// ResNeXt blocks, squeeze-and-excitation, and the u8 glue around FFDNet and the generator.  Dense convolutions run on mit_conv_gemm.
//
// Reference: manga_translator/colorization/manga_colorization_v2.py:_infer :42-74 and manga_colorization_v2_utils/
//   networks/extractor.py (Selayer :8-26, BottleneckX_Origin :29-72), networks/models.py (Selayer :88-106, ResNeXtBottleneck :125-151),
//   denoising/denoiser.py:get_denoised_image :51-118, denoising/functions.py (concatenate_input_noise_map :16-56,
//   UpSampleFeaturesFunction :58-102), denoising/utils.py:variable_to_cv2_image :17-33, utils/utils.py:resize_pad :4-44.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_TY = 8, GC_TX = 32;   // output pixels of a workgroup: 8 rows x 32 columns, one per thread
constexpr int GC_CS = 16;              // channels of a workgroup's slab: whole groups for every width 2..16
constexpr int GC_PSTR = 20;            // LDS floats per staged pixel: 16 + 4 pad keeps each 16-lane ds_read_b128 group conflict-free
constexpr int SE_THREADS = 256;
constexpr int SE_CHUNK = 256;          // pixels per squeeze partial: the partition depends on h * w only, never on B

inline unsigned grid_for(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    return (unsigned)(g > 256 * 16 ? 256 * 16 : (g < 1 ? 1 : g));
}

__device__ __forceinline__ float act_f(float v, int act, float alpha) {
    if (act == MIT_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == MIT_ACT_LEAKY) return v > 0.f ? v : v * alpha;
    return v;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// ---- (1) grouped 3x3 convolution, NHWC fp32, groups of CPG channels (Cin == Cout == C), stride s, dilation = padding = d ----
// grid (tiles_x * tiles_y, C / 16, B).  The workgroup stages its input tile with the halo (at most 4 each side at stride 1) for one
// 16-channel slab in LDS, plus the slab's weights; each thread computes 16 output channels of one pixel as fmaf chains over
// (tap, input channel of the group) in that fixed order.
template <int CPG>
__global__ void __launch_bounds__(GC_THREADS) grouped_conv3x3_kernel(const float *__restrict__ in, int64_t in_bs, int64_t in_ps, int H, int W,
                                                                   int C, const float *__restrict__ w, const float *__restrict__ scale,
                                                                   const float *__restrict__ bias, float *__restrict__ out, int64_t out_bs,
                                                                   int64_t out_ps, int Ho, int Wo, int s, int d, int act, float alpha,
                                                                   int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int rows = (GC_TY - 1) * s + 2 * d + 1, cols = (GC_TX - 1) * s + 2 * d + 1;
    float *tile = smem;                                   // [rows][cols][GC_PSTR]
    float *wl = smem + rows * cols * GC_PSTR;             // [9][16][CPG]
    const int t = threadIdx.x;
    const int tyo = (blockIdx.x / tiles_x) * GC_TY, txo = (blockIdx.x % tiles_x) * GC_TX;
    const int c0 = blockIdx.y * GC_CS, b = blockIdx.z;
    const int iy0 = tyo * s - d, ix0 = txo * s - d;
    const float *inb = in + (int64_t)b * in_bs + c0;
    const int nq = rows * cols * 4;
    for (int i = t; i < nq; i += GC_THREADS) {
        const int pix = i >> 2, q = i & 3;
        const int r = pix / cols, c = pix - r * cols;
        const int iy = iy0 + r, ix = ix0 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const float4 *>(inb + ((int64_t)iy * W + ix) * in_ps + 4 * q);
        *reinterpret_cast<float4 *>(tile + pix * GC_PSTR + 4 * q) = v;
    }
    for (int i = t; i < 9 * GC_CS * CPG; i += GC_THREADS) {   // torch layout w[co][ci][ky][kx] -> wl[tap][co - c0][ci]
        const int ci = i % CPG, co = (i / CPG) % GC_CS, tap = i / (CPG * GC_CS);
        wl[i] = w[((int64_t)(c0 + co) * CPG + ci) * 9 + tap];
    }
    __syncthreads();
    const int ty = t / GC_TX, tx = t % GC_TX;
    const int oy = tyo + ty, ox = txo + tx;
    float acc[GC_CS];
#pragma unroll
    for (int k = 0; k < GC_CS; ++k) acc[k] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {   // rolled: an unrolled tap loop hoists every weight read and spills
        const int ky = tap / 3, kx = tap % 3;
        const float *xp = tile + ((ty * s + ky * d) * cols + tx * s + kx * d) * GC_PSTR;
        float xin[GC_CS];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(xp + 4 * q);
            xin[4 * q] = v.x; xin[4 * q + 1] = v.y; xin[4 * q + 2] = v.z; xin[4 * q + 3] = v.w;
        }
        const float *wt = wl + tap * GC_CS * CPG;
#pragma unroll
        for (int co = 0; co < GC_CS; ++co) {
            const int g0 = (co / CPG) * CPG;
#pragma unroll
            for (int ci = 0; ci < CPG; ++ci) acc[co] = fmaf(xin[g0 + ci], wt[co * CPG + ci], acc[co]);
        }
    }
    if (oy >= Ho || ox >= Wo) return;
    float *op = out + (int64_t)b * out_bs + ((int64_t)oy * Wo + ox) * out_ps + c0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 4 * q + j;
            float v = acc[4 * q + j];
            if (scale) v = v * scale[c];
            if (bias) v = v + bias[c];
            r[j] = act_f(v, act, alpha);
        }
        *reinterpret_cast<float4 *>(op + 4 * q) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---- (2) SE squeeze: per (b, chunk) double partial sums of every channel; grid (nchunks, B) ----
__global__ void __launch_bounds__(SE_THREADS) se_partial_kernel(const float *__restrict__ x, int64_t bs, int64_t ps, int hw, int C,
                                                              double *__restrict__ part) {
    __shared__ double red[SE_THREADS][4];
    const int q4 = C >> 2, lanes = SE_THREADS / q4;
    const int t = threadIdx.x, q = t % q4, lane = t / q4;
    const int b = blockIdx.y, k = blockIdx.x, nchunks = gridDim.x;
    const int p0 = k * SE_CHUNK, p1 = min(hw, p0 + SE_CHUNK);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (lane < lanes) {
        const float *xb = x + (int64_t)b * bs + 4 * q;
        for (int p = p0 + lane; p < p1; p += lanes) {
            const float4 v = *reinterpret_cast<const float4 *>(xb + (int64_t)p * ps);
            s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
        }
    }
    red[t][0] = s0; red[t][1] = s1; red[t][2] = s2; red[t][3] = s3;
    __syncthreads();
    for (int off = lanes >> 1; off > 0; off >>= 1) {   // pairwise over the pixel lanes, always in the same order
        if (lane < off) {
            const int o = t + off * q4;
#pragma unroll
            for (int j = 0; j < 4; ++j) red[t][j] += red[o][j];
        }
        __syncthreads();
    }
    if (lane == 0) {
        double *dst = part + ((int64_t)b * nchunks + k) * C + 4 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = red[t][j];
    }
}

// ---- (3) SE excite: one workgroup per sample.  mean over the chunks in index order, then conv1 (C -> C/16) + ReLU, conv2 + sigmoid ----
__global__ void __launch_bounds__(SE_THREADS) se_excite_kernel(const double *__restrict__ part, int nchunks, int hw, int C,
                                                             const float *__restrict__ w1, const float *__restrict__ b1,
                                                             const float *__restrict__ w2, const float *__restrict__ b2,
                                                             float *__restrict__ s_out) {
    __shared__ float m[1024];
    __shared__ float h[64];
    const int b = blockIdx.x, Ch = C / 16;
    for (int c = threadIdx.x; c < C; c += SE_THREADS) {
        double S = 0;
        for (int k = 0; k < nchunks; ++k) S += part[((int64_t)b * nchunks + k) * C + c];
        m[c] = (float)(S / (double)hw);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Ch; j += SE_THREADS) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(w1[(int64_t)j * C + c], m[c], acc);
        acc = acc + b1[j];
        h[j] = acc > 0.f ? acc : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += SE_THREADS) {
        float acc = 0.f;
        for (int j = 0; j < Ch; ++j) acc = fmaf(w2[(int64_t)c * Ch + j], h[j], acc);
        s_out[(int64_t)b * C + c] = sigmoid_f(acc + b2[c]);
    }
}

// ---- (4) SE apply: out = act(x * s[b, c] + residual), float4 along C; out may alias x or residual ----
__global__ void se_apply_kernel(const float *x, int64_t x_bs, int64_t x_ps, const float *__restrict__ sc, const float *res, int64_t r_bs,
                                int64_t r_ps, float *out, int64_t o_bs, int64_t o_ps, int B, int hw, int C, int act) {
    const int q4 = C >> 2;
    const int64_t per_b = (int64_t)hw * q4, total = per_b * B;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int b = (int)(i / per_b);
        const int64_t r = i - b * per_b;
        const int64_t p = r / q4;
        const int c = (int)(r - p * q4) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(x + b * x_bs + p * x_ps + c);
        const float4 g = *reinterpret_cast<const float4 *>(sc + (int64_t)b * C + c);
        const float4 e = *reinterpret_cast<const float4 *>(res + b * r_bs + p * r_ps + c);
        float4 o;
        o.x = act_f(v.x * g.x + e.x, act, 0.f);
        o.y = act_f(v.y * g.y + e.y, act, 0.f);
        o.z = act_f(v.z * g.z + e.z, act, 0.f);
        o.w = act_f(v.w * g.w + e.w, act, 0.f);
        *reinterpret_cast<float4 *>(out + b * o_bs + p * o_ps + c) = o;
    }
}

// ---- (5) FFDNet input ----
// per-page max of the u8 RGB(A) page (alpha excluded): atomicMax on one word per page (order-independent)
__global__ void page_max_kernel(const uint8_t *__restrict__ img, int64_t npix, int Cin, unsigned *__restrict__ pmax) {
    const int b = blockIdx.y;
    const uint8_t *p = img + (int64_t)b * npix * Cin;
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *q = p + i * Cin;
        m = max(m, (unsigned)max(q[0], max(q[1], q[2])));
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_down((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(pmax + b, m);
}

// the page value FFDNet sees: /255 (np.float32(data / 255.)) only when the page's max exceeds 1.2 (denoiser.py:86-87)
__device__ __forceinline__ float ffd_value(uint8_t v, bool norm) { return norm ? (float)((double)v / 255.0) : (float)v; }

// u8 [B,H,W,Cin] -> [B,h2,w2,16]: (sigma x3, space-to-depth channel 3 + c*4 + (i*2 + j), 0); odd sides repeat their last row / column
__global__ void ffd_pack_kernel(const uint8_t *__restrict__ img, int H, int W, int Cin, const unsigned *__restrict__ pmax, float sigma,
                                float *__restrict__ out, int B, int h2, int w2) {
    const int64_t total = (int64_t)B * h2 * w2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % w2);
        const int64_t r = i / w2;
        const int y = (int)(r % h2), b = (int)(r / h2);
        const bool norm = pmax[b] > 1u;   // u8 max > 1.2
        float v[16];
        v[0] = v[1] = v[2] = sigma;
        v[15] = 0.f;
#pragma unroll
        for (int idx = 0; idx < 4; ++idx) {
            const int yy = min(2 * y + (idx >> 1), H - 1), xx = min(2 * x + (idx & 1), W - 1);
            const uint8_t *q = img + (((int64_t)b * H + yy) * W + xx) * Cin;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 + c * 4 + idx] = ffd_value(q[c], norm);
        }
        float4 *o = reinterpret_cast<float4 *>(out + i * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
}

// ---- (6) FFDNet output: depth-to-space of the 12-channel noise, clamp(x - noise, 0, 1), crop, RGB -> BGR, (v * 255) truncated ----
__global__ void ffd_unpack_kernel(const uint8_t *__restrict__ img, int H, int W, int Cin, const unsigned *__restrict__ pmax,
                                  const float *__restrict__ noise, int64_t n_ps, int h2, int w2, uint8_t *__restrict__ plane_b,
                                  uint8_t *__restrict__ bgr, int B) {
    const int64_t total = (int64_t)B * H * W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % W);
        const int64_t r = i / W;
        const int y = (int)(r % H), b = (int)(r / H);
        const bool norm = pmax[b] > 1u;
        const int idx = (y & 1) * 2 + (x & 1);
        const float *n = noise + (((int64_t)b * h2 + (y >> 1)) * w2 + (x >> 1)) * n_ps;
        const uint8_t *q = img + i * Cin;
        uint8_t o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf(ffd_value(q[c], norm) - n[c * 4 + idx], 0.f), 1.f);
            const float s = v * 255.f;
            o[2 - c] = (uint8_t)(s > 255.f ? 255.f : s);   // BGR; astype(uint8) truncates
        }
        if (plane_b) plane_b[i] = o[0];
        if (bgr) { bgr[3 * i] = o[0]; bgr[3 * i + 1] = o[1]; bgr[3 * i + 2] = o[2]; }
    }
}

// ---- (7) generator input: u8 plane [B,h,w] -> fp32 [B,Hp,Wp,4] = (ToTensor of np.pad(.., 'maximum'), 0, 0, 0) ----
__global__ void gen_in_kernel(const uint8_t *__restrict__ plane, int h, int w, float *__restrict__ out, int Hp, int Wp, int B) {
    const int64_t total = (int64_t)B * Hp * Wp;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % Wp);
        const int64_t r = i / Wp;
        const int y = (int)(r % Hp), b = (int)(r / Hp);
        const uint8_t *p = plane + (int64_t)b * h * w;
        unsigned v = 0;
        if (y < h && x < w) v = p[(int64_t)y * w + x];
        else if (y >= h) for (int yy = 0; yy < h; ++yy) v = max(v, (unsigned)p[(int64_t)yy * w + x]);   // rows padded: column max
        else for (int xx = 0; xx < w; ++xx) v = max(v, (unsigned)p[(int64_t)y * w + xx]);              // columns padded: row max
        *reinterpret_cast<float4 *>(out + i * 4) = make_float4((float)v / 255.f, 0.f, 0.f, 0.f);
    }
}

// ---- (8) exit: tanh, * 0.5 + 0.5, crop, * 255 truncated to u8 RGB ----
// Evaluated in double: the byte is the floor of the exact value wherever float64 resolves it.  In float32 the sum tanh * 0.5 + 0.5
// rounds up to 1.0 from tanh = 1 - 2^-24 on (x = 9 gives 255 where the exact value is 254.999996); the reference's own float32 bytes
// differ from these only within float32 rounding (1.5e-5 of a byte) of a truncation boundary.  Three double tanh per pixel are far
// below what the 12-byte load and 3-byte store of that pixel cost.
__global__ void post_kernel(const float *__restrict__ pre, int64_t pre_ps, int Hp, int Wp, uint8_t *__restrict__ out, int h, int w, int B) {
    const int64_t total = (int64_t)B * h * w;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % w);
        const int64_t r = i / w;
        const int y = (int)(r % h), b = (int)(r / h);
        const float *p = pre + (((int64_t)b * Hp + y) * Wp + x) * pre_ps;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = tanh((double)p[c]) * 0.5 + 0.5;
            out[3 * i + c] = (uint8_t)fmin(fmax(v * 255.0, 0.0), 255.0);
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t mit_grouped_conv3x3_lds_bytes(int stride, int dilation, int cpg) {
    const int rows = (GC_TY - 1) * stride + 2 * dilation + 1, cols = (GC_TX - 1) * stride + 2 * dilation + 1;
    return (int64_t)(rows * cols * GC_PSTR + 9 * GC_CS * cpg) * 4;
}

extern "C" int mit_grouped_conv3x3(const float *in_dev, int64_t in_bs, int64_t in_ps, int B, int H, int W, int C, int cpg, int stride,
                                   int dilation, const float *w_dev, const float *scale_dev, const float *bias_dev, int act, float alpha,
                                   float *out_dev, int64_t out_bs, int64_t out_ps, void *stream) {
    if (!in_dev || !w_dev || !out_dev) return mit_set_error("mit_grouped_conv3x3: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % GC_CS) return mit_set_error("mit_grouped_conv3x3: bad shape (C a multiple of 16)");
    if (cpg != 2 && cpg != 4 && cpg != 8 && cpg != 16) return mit_set_error("mit_grouped_conv3x3: channels per group must be 2, 4, 8 or 16");
    if ((stride != 1 && stride != 2) || (dilation != 1 && dilation != 2 && dilation != 4))
        return mit_set_error("mit_grouped_conv3x3: stride 1 | 2 and dilation 1 | 2 | 4");
    if (in_ps < C || out_ps < C || in_ps % 4 || out_ps % 4 || in_bs % 4 || out_bs % 4 || !aligned16(in_dev) || !aligned16(out_dev))
        return mit_set_error("mit_grouped_conv3x3: pixel / batch strides must be multiples of 4 floats (>= C), operands 16-byte aligned");
    if (act != MIT_ACT_NONE && act != MIT_ACT_RELU && act != MIT_ACT_LEAKY) return mit_set_error("mit_grouped_conv3x3: act none | relu | leaky");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int tiles_x = (Wo + GC_TX - 1) / GC_TX, tiles_y = (Ho + GC_TY - 1) / GC_TY;
    const size_t lds = (size_t)mit_grouped_conv3x3_lds_bytes(stride, dilation, cpg);
    dim3 grid(tiles_x * tiles_y, C / GC_CS, B);
    MitProbeScope probe("grouped_conv3x3_kernel", (hipStream_t)stream, 4.0 * B * C * ((double)H * W + (double)Ho * Wo),
                        2.0 * B * C * (double)Ho * Wo * 9 * cpg);
    static DynSmemOptIn optin[4];   // stride 2 stages about 96 KB (four input pixels per output pixel)
#define GC_LAUNCH(N, I)                                                                                                               \
    optin[I].ensure(reinterpret_cast<const void *>(grouped_conv3x3_kernel<N>), lds);                                                 \
    hipLaunchKernelGGL(grouped_conv3x3_kernel<N>, grid, dim3(GC_THREADS), lds, (hipStream_t)stream, in_dev, in_bs, in_ps, H, W, C, w_dev, \
                       scale_dev, bias_dev, out_dev, out_bs, out_ps, Ho, Wo, stride, dilation, act, alpha, tiles_x)
    switch (cpg) {
        case 2: GC_LAUNCH(2, 0); break;
        case 4: GC_LAUNCH(4, 1); break;
        case 8: GC_LAUNCH(8, 2); break;
        default: GC_LAUNCH(16, 3); break;
    }
#undef GC_LAUNCH
    MIT_CHECK_LAUNCH("mit_grouped_conv3x3");
    return 0;
}

extern "C" int64_t mit_se_squeeze_ws(int B, int hw, int C) {
    const int64_t nchunks = ((int64_t)hw + SE_CHUNK - 1) / SE_CHUNK;
    return (int64_t)B * nchunks * C * (int64_t)sizeof(double);
}

extern "C" int mit_se_squeeze(const float *x_dev, int64_t bs, int64_t ps, int B, int hw, int C, void *ws_dev, int64_t ws_bytes, void *stream) {
    if (!x_dev || !ws_dev) return mit_set_error("mit_se_squeeze: null pointer");
    if (B <= 0 || hw <= 0 || C < 4 || C > 1024 || (C & (C - 1))) return mit_set_error("mit_se_squeeze: C must be a power of two in [4, 1024]");
    if (ps % 4 || bs % 4 || !aligned16(x_dev)) return mit_set_error("mit_se_squeeze: strides must be multiples of 4 floats, x 16-byte aligned");
    if (ws_bytes < mit_se_squeeze_ws(B, hw, C)) return mit_set_error("mit_se_squeeze: workspace too small");
    const int nchunks = (hw + SE_CHUNK - 1) / SE_CHUNK;
    MitProbeScope probe("se_partial_kernel", (hipStream_t)stream, 4.0 * B * (double)hw * C);
    hipLaunchKernelGGL(se_partial_kernel, dim3(nchunks, B), dim3(SE_THREADS), 0, (hipStream_t)stream, x_dev, bs, ps, hw, C, (double *)ws_dev);
    MIT_CHECK_LAUNCH("mit_se_squeeze");
    return 0;
}

extern "C" int mit_se_excite(const void *ws_dev, int B, int hw, int C, const float *w1_dev, const float *b1_dev, const float *w2_dev,
                             const float *b2_dev, float *s_dev, void *stream) {
    if (!ws_dev || !w1_dev || !b1_dev || !w2_dev || !b2_dev || !s_dev) return mit_set_error("mit_se_excite: null pointer");
    if (B <= 0 || hw <= 0 || C < 16 || C > 1024 || C % 16) return mit_set_error("mit_se_excite: C must be a multiple of 16 in [16, 1024]");
    const int nchunks = (hw + SE_CHUNK - 1) / SE_CHUNK;
    MitProbeScope probe("se_excite_kernel", (hipStream_t)stream, 8.0 * B * (double)nchunks * C + 8.0 * C * (C / 16));
    hipLaunchKernelGGL(se_excite_kernel, dim3(B), dim3(SE_THREADS), 0, (hipStream_t)stream, (const double *)ws_dev, nchunks, hw, C, w1_dev,
                       b1_dev, w2_dev, b2_dev, s_dev);
    MIT_CHECK_LAUNCH("mit_se_excite");
    return 0;
}

extern "C" int mit_se_apply(const float *x_dev, int64_t x_bs, int64_t x_ps, const float *s_dev, const float *res_dev, int64_t r_bs,
                            int64_t r_ps, float *out_dev, int64_t o_bs, int64_t o_ps, int B, int hw, int C, int act, void *stream) {
    if (!x_dev || !s_dev || !res_dev || !out_dev) return mit_set_error("mit_se_apply: null pointer");
    if (B <= 0 || hw <= 0 || C <= 0 || C % 4) return mit_set_error("mit_se_apply: C must be a multiple of 4");
    if (x_ps % 4 || r_ps % 4 || o_ps % 4 || x_bs % 4 || r_bs % 4 || o_bs % 4 || !aligned16(x_dev) || !aligned16(res_dev) || !aligned16(out_dev))
        return mit_set_error("mit_se_apply: strides must be multiples of 4 floats, operands 16-byte aligned");
    if (act != MIT_ACT_NONE && act != MIT_ACT_RELU) return mit_set_error("mit_se_apply: act none | relu");
    const int64_t total = (int64_t)B * hw * (C / 4);
    MitProbeScope probe("se_apply_kernel", (hipStream_t)stream, 12.0 * B * (double)hw * C);
    hipLaunchKernelGGL(se_apply_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x_dev, x_bs, x_ps, s_dev, res_dev, r_bs,
                       r_ps, out_dev, o_bs, o_ps, B, hw, C, act);
    MIT_CHECK_LAUNCH("mit_se_apply");
    return 0;
}

extern "C" int mit_mc2_ffd_pack(const uint8_t *img_dev, int B, int H, int W, int Cin, float sigma, unsigned *pmax_dev, float *out_dev,
                                void *stream) {
    if (!img_dev || !pmax_dev || !out_dev) return mit_set_error("mit_mc2_ffd_pack: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || (Cin != 3 && Cin != 4)) return mit_set_error("mit_mc2_ffd_pack: bad shape (Cin 3 | 4)");
    if (!aligned16(out_dev)) return mit_set_error("mit_mc2_ffd_pack: output must be 16-byte aligned");
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    MIT_CHECK_HIP(hipMemsetAsync(pmax_dev, 0, sizeof(unsigned) * B, (hipStream_t)stream));
    const int64_t npix = (int64_t)H * W;
    {
        MitProbeScope probe("page_max_kernel", (hipStream_t)stream, (double)B * npix * Cin);
        const int64_t gx0 = (npix + 255) / 256;
        const unsigned gx = (unsigned)(gx0 < 512 ? gx0 : 512);
        hipLaunchKernelGGL(page_max_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, img_dev, npix, Cin, pmax_dev);
        MIT_CHECK_LAUNCH("mit_mc2_ffd_pack (max)");
    }
    const int64_t total = (int64_t)B * h2 * w2;
    MitProbeScope probe("ffd_pack_kernel", (hipStream_t)stream, (double)B * npix * Cin + 64.0 * total);
    hipLaunchKernelGGL(ffd_pack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, img_dev, H, W, Cin, pmax_dev, sigma,
                       out_dev, B, h2, w2);
    MIT_CHECK_LAUNCH("mit_mc2_ffd_pack");
    return 0;
}

extern "C" int mit_mc2_ffd_unpack(const uint8_t *img_dev, int B, int H, int W, int Cin, const unsigned *pmax_dev, const float *noise_dev,
                                  int64_t noise_pixstride, uint8_t *plane_dev, uint8_t *bgr_dev, void *stream) {
    if (!img_dev || !pmax_dev || !noise_dev || (!plane_dev && !bgr_dev)) return mit_set_error("mit_mc2_ffd_unpack: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || (Cin != 3 && Cin != 4) || noise_pixstride < 12) return mit_set_error("mit_mc2_ffd_unpack: bad shape");
    const int64_t total = (int64_t)B * H * W;
    MitProbeScope probe("ffd_unpack_kernel", (hipStream_t)stream, (double)total * (Cin + 12 + 4));
    hipLaunchKernelGGL(ffd_unpack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, img_dev, H, W, Cin, pmax_dev, noise_dev,
                       noise_pixstride, (H + 1) / 2, (W + 1) / 2, plane_dev, bgr_dev, B);
    MIT_CHECK_LAUNCH("mit_mc2_ffd_unpack");
    return 0;
}

extern "C" int mit_mc2_gen_in(const uint8_t *plane_dev, int B, int h, int w, float *out_dev, int Hp, int Wp, void *stream) {
    if (!plane_dev || !out_dev) return mit_set_error("mit_mc2_gen_in: null pointer");
    if (B <= 0 || h <= 0 || w <= 0 || Hp < h || Wp < w || (Hp > h && Wp > w)) return mit_set_error("mit_mc2_gen_in: bad shape (one side padded)");
    if (!aligned16(out_dev)) return mit_set_error("mit_mc2_gen_in: output must be 16-byte aligned");
    const int64_t total = (int64_t)B * Hp * Wp;
    MitProbeScope probe("gen_in_kernel", (hipStream_t)stream, (double)B * h * w + 16.0 * total);
    hipLaunchKernelGGL(gen_in_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, plane_dev, h, w, out_dev, Hp, Wp, B);
    MIT_CHECK_LAUNCH("mit_mc2_gen_in");
    return 0;
}

extern "C" int mit_mc2_post(const float *pre_dev, int64_t pre_pixstride, int B, int Hp, int Wp, uint8_t *out_dev, int h, int w, void *stream) {
    if (!pre_dev || !out_dev) return mit_set_error("mit_mc2_post: null pointer");
    if (B <= 0 || h <= 0 || w <= 0 || h > Hp || w > Wp || pre_pixstride < 3) return mit_set_error("mit_mc2_post: bad shape");
    const int64_t total = (int64_t)B * h * w;
    MitProbeScope probe("mc2_post_kernel", (hipStream_t)stream, total * (12.0 + 3.0));
    hipLaunchKernelGGL(post_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, pre_dev, pre_pixstride, Hp, Wp, out_dev, h, w,
                       B);
    MIT_CHECK_LAUNCH("mit_mc2_post");
    return 0;
}
