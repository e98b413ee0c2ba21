// ocr32_decoder.hip — native beam-search decoder of the 32px OCR (OCR.infer_beam_batch + next_token_batch,
// manga_translator/ocr/model_32px.py:415-465, :518-595).
//
// Two POST-norm nn.TransformerDecoderLayer (320, 4 heads x 80, FFN 2048, ReLU), sinusoidal positions, weights of `pred` tied to the
// embedding.  The whole loop after the encoder is one C call, as mit_ocr48_decode is for the 48px model; what differs from that loop:
//   * the layer order is norm(x + sublayer(x)) (:451-460), so the LayerNorms cannot ride inside the consuming Linear;
//   * a hypothesis CARRIES its per-layer activation history when the beam is re-ordered (Hypothesis.extend clones
//     cached_activations, :404-410; the 48px model leaves its caches in place).  Here a K / V / output row is written once, at
//     (beam row, position), and never moved: each beam row keeps a table `src[t]` = the row that holds position t of its
//     history, which the bookkeeping kernel copies from the parent (T + 1 ints instead of 2 layers x 2 x T x 320 floats);
//   * the beam rules (:542-580): candidates ranked by the MEAN log-probability over len + 1 entries (the start token's 0.0
//     counts), stable order, the best beams_k + 1 = 6 are looked at, a line with max_finished ended hypotheses drops out, and the
//     final pick prefers ANY finished hypothesis over live ones.
// Lines stay in place (five rows each) after they are done: row r always belongs to line r / 5, so the cross-attention needs no
// table; a done line's rows keep running on stale values and are never read again.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/mit_hip.h"
#include "common.h"
#include "ocr_kernels.h"
#include "pgemm_rows.h"
#include "ocr_linear.h"
#include "bf16_split.h"

namespace {

using namespace ocrlin;

constexpr int E = 320;
constexpr int FF = 2048;
constexpr int HEADS = 4;
constexpr int HD = 80;
constexpr int BEAMS = 5;
constexpr int ROWS_MAX = 2560;            // rows (lines x beams) up to which a step runs in the few-row form (16 pages of 32 lines, as the 48px loop)
constexpr int FF2_SPLITK_MAX_ROWS = 640;  // rows up to which the few-row FFN output Linear cuts K across four waves (as the 48px loop)

struct Ws {
    float *x, *y, *qkv, *att, *q2, *ffh, *decoded, *p1, *logits, *vals, *sel_dec, *cfeat;
    double *lsum, *fin_mean;
    int *idx, *hist, *src, *fin_tok, *fin_src, *fin_len, *fin_cnt, *done, *done_count, *sel_src;
    // the few-row form: activations that feed a Linear also live as bf16 planes [3][K / 8][Rp][8] (pgemm_rows.h)
    uint16_t *x_p, *att_p, *ffh_p, *p1_p;
    int64_t Rp;
};

int64_t carve(Ws *w, char *base, int N, int T, int D) {
    const int64_t R = (int64_t)N * BEAMS;
    const int64_t Dp = (D + 3) / 4 * 4;
    const int64_t P = T + 1;   // positions a hypothesis can hold (network evaluations 0 .. T)
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    Ws o;
    o.x = (float *)take(R * E * 4);
    o.y = (float *)take(R * E * 4);
    o.qkv = (float *)take(2 * 3 * R * P * E * 4);
    o.att = (float *)take(R * E * 4);
    o.q2 = (float *)take(R * E * 4);
    o.ffh = (float *)take(R * FF * 4);
    o.decoded = (float *)take(R * P * E * 4);
    o.p1 = (float *)take(R * E * 4);
    o.logits = (float *)take(R * Dp * 4);
    o.vals = (float *)take(R * 5 * 4);
    o.sel_dec = (float *)take((int64_t)N * P * E * 4);
    o.cfeat = (float *)take((int64_t)N * P * 64 * 4);
    o.lsum = (double *)take(2 * R * 8);
    o.fin_mean = (double *)take((int64_t)N * 2 * 8);
    o.idx = (int *)take(R * 5 * 4);
    o.hist = (int *)take(2 * R * (T + 2) * 4);
    o.src = (int *)take(2 * R * P * 4);
    o.fin_tok = (int *)take((int64_t)N * 2 * (T + 2) * 4);
    o.fin_src = (int *)take((int64_t)N * 2 * P * 4);
    o.fin_len = (int *)take((int64_t)N * 2 * 4);
    o.fin_cnt = (int *)take((int64_t)N * 4);
    o.done = (int *)take((int64_t)N * 4);
    o.done_count = (int *)take(256);
    o.sel_src = (int *)take((int64_t)N * P * 4);
    o.Rp = (R + 31) / 32 * 32;
    o.x_p = (uint16_t *)take(3 * E * o.Rp * 2);
    o.att_p = (uint16_t *)take(3 * E * o.Rp * 2);
    o.ffh_p = (uint16_t *)take(3 * FF * o.Rp * 2);
    o.p1_p = (uint16_t *)take(3 * E * o.Rp * 2);
    if (w) *w = o;
    return off;
}

// eight consecutive fp32 values -> their cell in each of the three planes (the split a GEMM tile applies to the value itself)
__device__ __forceinline__ void store_cells(const OcrPlanes &o, const int k8, const int64_t row, const float *v8) {
    mitcg::u32x4 h, m, l;
    mitcg::split8(*reinterpret_cast<const f32x4 *>(v8), *reinterpret_cast<const f32x4 *>(v8 + 4), h, m, l);
    mitcg::u32x4 *dst = reinterpret_cast<mitcg::u32x4 *>(o.p) + (int64_t)k8 * o.ld + row;
    const int64_t plane = (int64_t)o.K8 * o.ld;
    dst[0] = h;
    dst[plane] = m;
    dst[2 * plane] = l;
}
__device__ __forceinline__ void wave_lds_fence() {  // a wave's own LDS accesses complete in order: wait for them, keep the compiler from reordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- LayerNorm of the post-norm order: out = LN(in) as fp32 (the residual of the next sub-layer) and, for the few-row form, as the
// bf16 planes the next Linear consumes.  `in` already holds x + sublayer(x): the producing Linear adds the residual in its epilogue.
// One wave per row, D == 320 (five values per lane); the arithmetic of layernorm_kernel (ocr_kernels.hip), value for value.
__global__ __launch_bounds__(256) void ocr32_layernorm_kernel(const float *__restrict__ in, int64_t in_rs, const float *__restrict__ w,
                                                              const float *__restrict__ b, float *__restrict__ out, int64_t out_rs, int rows,
                                                              float eps, OcrPlanes pl) {
    __shared__ __attribute__((aligned(16))) float ybuf[4][E];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = in + (int64_t)row * in_rs;
    float v[E / 64];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < E / 64; ++j) {
        v[j] = x[lane + 64 * j];
        sum += v[j];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)E;
    float var = 0.f;
#pragma unroll
    for (int j = 0; j < E / 64; ++j) {
        const float t = v[j] - mean;
        var += t * t;
    }
    for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
    const float rstd = 1.0f / sqrtf(var / (float)E + eps);
    float *y = out + (int64_t)row * out_rs;
    float *yb = ybuf[threadIdx.x >> 6];
#pragma unroll
    for (int j = 0; j < E / 64; ++j) {
        const int d = lane + 64 * j;
        const float r = (v[j] - mean) * rstd * w[d] + b[d];
        y[d] = r;
        yb[d] = r;
    }
    if (!pl.p) return;
    wave_lds_fence();
    if (lane < E / 8) store_cells(pl, lane, row, yb + lane * 8);
}

int layernorm(const float *in, const float *w, const float *b, float *out, int64_t out_rs, int rows, const OcrPlanes &pl, hipStream_t s) {
    MitProbeScope probe("ocr32_layernorm_kernel", s, 10.0 * (double)rows * E);
    hipLaunchKernelGGL(ocr32_layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, (int64_t)E, w, b, out, out_rs, rows, 1e-5f, pl);
    return 0;
}

// ---- attention of ONE query per beam row: 4 heads x 80, one workgroup per row, one wave per head ----
// Keys / values of position t come from row (src ? src[r * src_ld + t] : r / kv_div) of K / V (row stride kv_rs floats, position stride
// E).  Valid keys: min(klen ? klen[r / kv_div] : Tk, Tk).  Scores: lane-strided over t, each a sequential 80-term dot product; the
// softmax sums by the wave's butterfly; the weighted sum has the channel on the lane (coalesced rows of V) and sums t in four interleaved partial sums, sixteen rows of V in flight.
// The query is already scaled (the projection's epilogue carries head_dim ** -0.5).
__global__ __launch_bounds__(256) void ocr32_attention_kernel(const float *__restrict__ Q, int64_t q_rs, const float *__restrict__ K,
                                                              const float *__restrict__ V, int64_t kv_rs, const int *__restrict__ src,
                                                              int src_ld, int kv_div, const int *__restrict__ klen, int Tk,
                                                              float *__restrict__ O, int R, OcrPlanes opl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // q [E] | p [HEADS][Tk] | row [Tk] ints
    const int r = blockIdx.x;
    if (r >= R) return;
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    float *qs = smem;
    float *ps = smem + E + h * Tk;
    int *rows = reinterpret_cast<int *>(smem + E + HEADS * Tk);
    const int line = r / kv_div;
    int n = Tk;
    if (klen) n = min(klen[line], Tk);
    for (int i = tid; i < E; i += 256) qs[i] = Q[(int64_t)r * q_rs + i];
    for (int t = tid; t < n; t += 256) rows[t] = src ? src[(int64_t)r * src_ld + t] : line;
    __syncthreads();
    float mx = -INFINITY;
    for (int t = lane; t < n; t += 64) {
        const float4 *k4 = reinterpret_cast<const float4 *>(K + (int64_t)rows[t] * kv_rs + (int64_t)t * E + h * HD);
        const float4 *q4 = reinterpret_cast<const float4 *>(qs + h * HD);
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < HD / 4; ++d) {
            const float4 kv = k4[d], qv = q4[d];
            acc += qv.x * kv.x;
            acc += qv.y * kv.y;
            acc += qv.z * kv.z;
            acc += qv.w * kv.w;
        }
        ps[t] = acc;
        mx = fmaxf(mx, acc);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int t = lane; t < n; t += 64) {
        const float e = expf(ps[t] - mx);
        ps[t] = e;
        sum += e;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();   // every lane's p[t] is visible to the wave (and the wave's own LDS writes are complete)
    const float inv = 1.f / sum;
    float *oh = qs + h * HD;   // the head's query slice is dead (only this wave read it): its 80 outputs are staged there for the planes
    // lane d sums channel d (and lanes 0 .. 15 channel 64 + d beside it); four partial sums over t mod 4 keep four loads and adds in flight
    const bool two = lane < HD - 64;
    const float *vb = V + h * HD + lane;
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    int t = 0;
    for (; t + 16 <= n; t += 16) {   // sixteen rows of V requested before the first is used: the loop is bound by the round trips
        float v0[16], v1[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float *vr = vb + (int64_t)rows[t + j] * kv_rs + (int64_t)(t + j) * E;
            v0[j] = vr[0];
            v1[j] = two ? vr[64] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float pj = ps[t + j];
            a0[j & 3] += pj * v0[j];
            a1[j & 3] += pj * v1[j];
        }
    }
    for (; t + 4 <= n; t += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *vr = vb + (int64_t)rows[t + j] * kv_rs + (int64_t)(t + j) * E;
            const float pj = ps[t + j];
            a0[j] += pj * vr[0];
            if (two) a1[j] += pj * vr[64];
        }
    }
    for (int j = 0; t < n; ++t, ++j) {
        const float *vr = vb + (int64_t)rows[t] * kv_rs + (int64_t)t * E;
        a0[j] += ps[t] * vr[0];
        if (two) a1[j] += ps[t] * vr[64];
    }
    const float o0 = ((a0[0] + a0[1]) + (a0[2] + a0[3])) * inv, o1 = ((a1[0] + a1[1]) + (a1[2] + a1[3])) * inv;
    if (opl.p) {
        oh[lane] = o0;
        if (two) oh[64 + lane] = o1;
    } else {
        O[(int64_t)r * E + h * HD + lane] = o0;
        if (two) O[(int64_t)r * E + h * HD + 64 + lane] = o1;
    }
    if (opl.p) {   // the output feeds a few-row Linear only: bf16 planes instead of fp32
        wave_lds_fence();
        if (lane < HD / 8) store_cells(opl, h * (HD / 8) + lane, r, oh + lane * 8);
    }
}

int attention(const float *Q, int64_t q_rs, const float *K, const float *V, int64_t kv_rs, const int *src, int src_ld, int kv_div,
              const int *klen, int Tk, float *O, int R, hipStream_t s, const OcrPlanes &opl) {
    const size_t smem = ((size_t)E + (size_t)(HEADS + 1) * Tk) * 4;
    if (Tk <= 0 || smem > 64 * 1024) return mit_set_error("mit_ocr32_decode: attention over %d keys does not fit the LDS form", Tk);
    MitProbeScope probe("ocr32_attention_kernel", s, 8.0 * (double)R * Tk * E);
    hipLaunchKernelGGL(ocr32_attention_kernel, dim3(R), dim3(256), smem, s, Q, q_rs, K, V, kv_rs, src, src_ld, kv_div, klen, Tk, O, R, opl);
    return 0;
}

// ---- bookkeeping ----
__global__ void ocr32_fill_rows_kernel(int *__restrict__ hist, int64_t n_hist, int start_tok, int *__restrict__ src, int src_ld, int64_t n_src,
                                       int R) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = i; j < n_hist; j += stride) hist[j] = start_tok;
    for (int64_t j = i; j < n_src; j += stride) src[j] = (int)((j / src_ld) % R);   // a row's own slot until a parent's table is copied in
}

// One cell of eight values of embd[tok] + pe[pos] (next_token_batch :427-429: the last token of a hypothesis at offset len) as fp32 and,
// for the few-row form, as planes.
__device__ __forceinline__ void embed_cell(const float *__restrict__ embd, const float *__restrict__ pe, int tok, int pos, int c, int row,
                                           float *__restrict__ out, const OcrPlanes &pl) {
    const float4 *a = reinterpret_cast<const float4 *>(embd + (int64_t)tok * E) + 2 * c;
    const float4 *b = reinterpret_cast<const float4 *>(pe + (int64_t)pos * E) + 2 * c;
    const float4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    __attribute__((aligned(16))) float v[8] = {a0.x + b0.x, a0.y + b0.y, a0.z + b0.z, a0.w + b0.w, a1.x + b1.x, a1.y + b1.y, a1.z + b1.z, a1.w + b1.w};
    float4 *o = reinterpret_cast<float4 *>(out + (int64_t)row * E) + 2 * c;
    o[0] = make_float4(v[0], v[1], v[2], v[3]);
    o[1] = make_float4(v[4], v[5], v[6], v[7]);
    if (pl.p) store_cells(pl, c, row, v);
}

__global__ void ocr32_embed_kernel(const int *__restrict__ tok, int64_t tok_stride, const float *__restrict__ embd, const float *__restrict__ pe,
                                   int pos, float *__restrict__ out, int R, OcrPlanes pl) {
    const int64_t total = (int64_t)R * (E / 8);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int c = (int)(i % (E / 8)), r = (int)(i / (E / 8));
        embed_cell(embd, pe, tok[(int64_t)r * tok_stride], pos, c, r, out, pl);
    }
}

struct BeamBufs {
    const int *hist_in;
    int *hist_out;
    int hist_ld;          // T + 2
    const int *src_in;
    int *src_out;
    int src_ld;           // T + 1
    const double *lsum_in;
    double *lsum_out;
    int *fin_tok, *fin_src, *fin_len, *fin_cnt;
    double *fin_mean;
    int *done, *done_count;
    const float *embd, *pe;   // next step's residual stream: embd[token] + pe[step + 1]
    float *x_next;
    OcrPlanes x_planes;       // ... and its planes (few-row form; p == NULL: none)
};

// One wave per line.  step == 0 (:531-541): the five best tokens of the line's first row become its hypotheses; nothing is tested for
// </S>.  step >= 1 (:544-572): lane c < 25 holds candidate (hypothesis c / 5, rank c % 5); its key is the mean of out_logprobs, which
// has step + 2 entries (the start token's 0.0 included); rank = number of candidates that sort before it in Python's stable order.
__global__ __launch_bounds__(64) void ocr32_beam_kernel(const float *__restrict__ vals, const int *__restrict__ idx, BeamBufs b, int N, int step,
                                                        int T, int end_tok, int max_finished) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N) return;
    __shared__ int s_order[32];     // rank -> candidate
    __shared__ int s_keep[BEAMS];   // kept hypothesis -> candidate
    __shared__ int s_fin[2];        // finished slot written this step -> candidate (-1: none)
    __shared__ int s_flags[2];      // kept count, done
    const int row0 = n * BEAMS;
    int tokk[BEAMS];
    if (step == 0) {
        if (lane < BEAMS) {
            const int row = row0 + lane;
            b.hist_out[(int64_t)row * b.hist_ld + 1] = idx[row0 * 5 + lane];   // [0] holds the start token (filled)
            b.lsum_out[row] = (double)vals[row0 * 5 + lane];
            if (1 < b.src_ld) b.src_out[(int64_t)row * b.src_ld + 1] = row;
        }
#pragma unroll
        for (int k = 0; k < BEAMS; ++k) tokk[k] = idx[row0 * 5 + k];
    } else {
        if (b.done[n]) return;   // (uniform over the wave; only this wave writes done[n])
        double key = 0.0;
        if (lane < 25) {
            const int hb = lane / 5, j = lane - hb * 5, row = row0 + hb;
            key = (b.lsum_in[row] + (double)vals[row * 5 + j]) / (double)(step + 2);
        }
        int rank = 0;
        for (int c = 0; c < 25; ++c) {
            const double ok = __shfl(key, c);
            if (ok > key || (ok == key && c < lane)) ++rank;
        }
        if (lane < 25) s_order[rank] = lane;
        __syncthreads();
        if (lane == 0) {
            int kept = 0, fin = b.fin_cnt[n], isdone = 0;
            s_fin[0] = s_fin[1] = -1;
            for (int q = 0; q < BEAMS + 1; ++q) {
                const int c = s_order[q];
                const int hb = c / 5, j = c - hb * 5;
                if (idx[(row0 + hb) * 5 + j] == end_tok) {
                    if (fin < 2) s_fin[fin] = c;
                    ++fin;
                    if (fin >= max_finished) {
                        isdone = 1;
                        break;
                    }
                } else if (kept < BEAMS) {
                    s_keep[kept++] = c;
                }
            }
            s_flags[0] = kept;
            s_flags[1] = isdone;
        }
        __syncthreads();
        // finished hypotheses of this step: tokens 0 .. step of the parent + </S>, the parent's output history 0 .. step
        for (int f = 0; f < 2; ++f) {
            const int c = s_fin[f];
            if (c < 0) continue;
            const int prow = row0 + c / 5;
            int *ft = b.fin_tok + ((int64_t)n * 2 + f) * b.hist_ld;
            int *fs = b.fin_src + ((int64_t)n * 2 + f) * b.src_ld;
            for (int t = lane; t <= step; t += 64) {
                ft[t] = b.hist_in[(int64_t)prow * b.hist_ld + t];
                fs[t] = b.src_in[(int64_t)prow * b.src_ld + t];
            }
            const double k = __shfl(key, c);
            if (lane == 0) {
                ft[step + 1] = end_tok;
                b.fin_len[n * 2 + f] = step + 2;
                b.fin_mean[n * 2 + f] = k;
            }
        }
        if (lane == 0) {
            int fin = b.fin_cnt[n];
            fin += (s_fin[0] >= 0) + (s_fin[1] >= 0);
            b.fin_cnt[n] = fin;
            if (s_flags[1]) {
                b.done[n] = 1;
                atomicAdd(b.done_count, 1);
            }
        }
        if (s_flags[1]) return;   // the line drops out (:565-572): its rows are never read again
        // a live line always keeps exactly five (six candidates looked at, at most one of them finished)
#pragma unroll
        for (int k = 0; k < BEAMS; ++k) {
            const int c = s_keep[k];
            const int hb = c / 5, j = c - hb * 5;
            const int prow = row0 + hb, row = row0 + k;
            for (int t = lane; t <= step; t += 64) {
                b.hist_out[(int64_t)row * b.hist_ld + t] = b.hist_in[(int64_t)prow * b.hist_ld + t];
                b.src_out[(int64_t)row * b.src_ld + t] = b.src_in[(int64_t)prow * b.src_ld + t];
            }
            tokk[k] = idx[prow * 5 + j];
            if (lane == 0) {
                b.hist_out[(int64_t)row * b.hist_ld + step + 1] = tokk[k];
                if (step + 1 < b.src_ld) b.src_out[(int64_t)row * b.src_ld + step + 1] = row;
                b.lsum_out[row] = b.lsum_in[prow] + (double)vals[prow * 5 + j];
            }
        }
    }
    if (step + 1 > T) return;   // no further evaluation
    for (int i = lane; i < BEAMS * (E / 8); i += 64) {
        const int k = i / (E / 8), c = i - k * (E / 8);
        const int t = k == 0 ? tokk[0] : k == 1 ? tokk[1] : k == 2 ? tokk[2] : k == 3 ? tokk[3] : tokk[4];
        embed_cell(b.embd, b.pe, t, step + 1, c, row0 + k, b.x_next, b.x_planes);
    }
}

// The final pick (:576-594): no finished hypothesis -> the best of the last step's candidates, which is the first kept one (had it ended
// in </S> it would be in the finished list); else the better finished one (stable: the earlier on a tie) even if a live one scores
// higher.  Writes the tokens, their count, exp(mean) and the table of the rows that hold the chosen hypothesis's output history.
__global__ __launch_bounds__(64) void ocr32_finalize_kernel(const int *__restrict__ hist, int hist_ld, const int *__restrict__ src, int src_ld,
                                                            const double *__restrict__ lsum, const int *__restrict__ fin_tok,
                                                            const int *__restrict__ fin_src, const int *__restrict__ fin_len,
                                                            const double *__restrict__ fin_mean, const int *__restrict__ fin_cnt, int N,
                                                            int evals, int *__restrict__ res_tok, int *__restrict__ res_len,
                                                            float *__restrict__ res_prob, int *__restrict__ sel_src) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N) return;
    const int *tk, *sr;
    int len;
    double mean;
    const int fc = fin_cnt[n];
    if (fc == 0) {
        const int row = n * BEAMS;
        tk = hist + (int64_t)row * hist_ld;
        sr = src + (int64_t)row * src_ld;
        len = evals + 1;
        mean = lsum[row] / (double)len;
    } else {
        const int f = (fc >= 2 && fin_mean[n * 2 + 1] > fin_mean[n * 2 + 0]) ? 1 : 0;
        tk = fin_tok + ((int64_t)n * 2 + f) * hist_ld;
        sr = fin_src + ((int64_t)n * 2 + f) * src_ld;
        len = fin_len[n * 2 + f];
        mean = fin_mean[n * 2 + f];
    }
    for (int t = lane; t < hist_ld; t += 64) res_tok[(int64_t)n * hist_ld + t] = t < len ? tk[t] : 0;
    for (int t = lane; t < src_ld; t += 64) sel_src[(int64_t)n * src_ld + t] = t < len - 1 ? sr[t] : -1;
    if (lane == 0) {
        res_len[n] = len;
        res_prob[n] = (float)exp(mean);
    }
}

// out[n][t] = decoded[sel_src[n][t]][t] (zero where the hypothesis has no position t): the output history of the chosen hypothesis
__global__ void ocr32_gather_kernel(const float *__restrict__ decoded, int64_t row_stride, const int *__restrict__ sel_src, int64_t n_pos,
                                    int P, float *__restrict__ out) {
    const int64_t total = n_pos * (E / 4);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int d4 = (int)(i % (E / 4));
        const int64_t p = i / (E / 4);
        const int t = (int)(p % P), r = sel_src[p];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r >= 0) v = reinterpret_cast<const float4 *>(decoded + (int64_t)r * row_stride + (int64_t)t * E)[d4];
        reinterpret_cast<float4 *>(out)[i] = v;
    }
}

int grid1d(int64_t total) { return (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024); }

// One bookkeeping launch: reads buffer `cur`, returns the buffer it wrote (step 0 fills buffer 0 in place).  embd == NULL: no next-step rows.
int launch_beam(const Ws &w, const float *vals, const int *idx, const float *embd, const float *pe, const OcrPlanes &x_planes,
                const MitOcr32DecodeArgs *a, int step, int cur, hipStream_t s) {
    const int N = a->N, T = a->max_seq_length, R = N * BEAMS;
    const int hist_ld = T + 2, src_ld = T + 1;
    BeamBufs b;
    const int in = cur, out = step == 0 ? cur : cur ^ 1;
    b.hist_in = w.hist + (int64_t)in * R * hist_ld;
    b.hist_out = w.hist + (int64_t)out * R * hist_ld;
    b.hist_ld = hist_ld;
    b.src_in = w.src + (int64_t)in * R * src_ld;
    b.src_out = w.src + (int64_t)out * R * src_ld;
    b.src_ld = src_ld;
    b.lsum_in = w.lsum + (int64_t)in * R;
    b.lsum_out = w.lsum + (int64_t)out * R;
    b.fin_tok = w.fin_tok; b.fin_src = w.fin_src; b.fin_len = w.fin_len; b.fin_cnt = w.fin_cnt; b.fin_mean = w.fin_mean;
    b.done = w.done; b.done_count = w.done_count;
    b.embd = embd; b.pe = pe; b.x_next = w.x; b.x_planes = x_planes;
    MitProbeScope probe("ocr32_beam_kernel", s, 8.0 * (double)R * (step + 2));
    hipLaunchKernelGGL(ocr32_beam_kernel, dim3(N), dim3(64), 0, s, vals, idx, b, N, step, embd ? T : -1, a->end_tok, a->max_finished);
    return out;
}

}  // namespace

extern "C" int64_t mit_ocr32_decode_workspace_bytes(int N, int T, int dict_size) {
    if (N <= 0 || T <= 0 || dict_size <= 0) return 0;
    return carve(nullptr, nullptr, N, T, dict_size);
}

// The bookkeeping of one step alone, on caller-provided (vals, idx) tables [steps][5 N][5]: what the loop below runs after every
// log-softmax / top-5.  For tests of the beam rules without a network; the same kernels, the same buffers.
extern "C" int mit_ocr32_beam_replay(const float *vals_dev, const int32_t *idx_dev, int steps, MitOcr32DecodeArgs *a, void *stream) {
    if (!a || !vals_dev || !idx_dev) return mit_set_error("mit_ocr32_beam_replay: null argument");
    const int N = a->N, T = a->max_seq_length;
    if (N <= 0 || T <= 0 || steps <= 0 || steps > T + 1) return mit_set_error("mit_ocr32_beam_replay: steps must be in 1 .. max_seq_length + 1");
    if (a->max_finished < 1 || a->max_finished > 2) return mit_set_error("mit_ocr32_beam_replay: max_finished must be 1 or 2");
    if (!a->workspace || !a->res_tok || !a->res_len || !a->res_prob) return mit_set_error("mit_ocr32_beam_replay: null buffer");
    if (a->workspace_bytes < carve(nullptr, nullptr, N, T, 8)) return mit_set_error("mit_ocr32_beam_replay: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    carve(&w, (char *)a->workspace, N, T, 8);
    const int R = N * BEAMS, hist_ld = T + 2, src_ld = T + 1;
    hipLaunchKernelGGL(ocr32_fill_rows_kernel, dim3(64), dim3(256), 0, s, w.hist, (int64_t)2 * R * hist_ld, a->start_tok, w.src, src_ld,
                       (int64_t)2 * R * src_ld, R);
    MIT_CHECK_HIP(hipMemsetAsync(w.done, 0, (size_t)N * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.fin_cnt, 0, (size_t)N * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.done_count, 0, 4, s));
    int cur = 0, evals = 0;
    for (int step = 0; step < steps; ++step) {
        cur = launch_beam(w, vals_dev + (int64_t)step * R * 5, idx_dev + (int64_t)step * R * 5, nullptr, nullptr, OcrPlanes{nullptr, 0, 0}, a, step, cur, s);
        evals = step + 1;
        if (a->trace_hist)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_hist + (int64_t)step * R * hist_ld, w.hist + (int64_t)cur * R * hist_ld, (size_t)R * hist_ld * 4,
                                         hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(ocr32_finalize_kernel, dim3(N), dim3(64), 0, s, w.hist + (int64_t)cur * R * hist_ld, hist_ld,
                       w.src + (int64_t)cur * R * src_ld, src_ld, w.lsum + (int64_t)cur * R, w.fin_tok, w.fin_src, w.fin_len, w.fin_mean,
                       w.fin_cnt, N, evals, a->res_tok, a->res_len, a->res_prob, w.sel_src);
    if (a->res_src) MIT_CHECK_HIP(hipMemcpyAsync(a->res_src, w.sel_src, (size_t)N * src_ld * 4, hipMemcpyDeviceToDevice, s));
    MIT_CHECK_LAUNCH("mit_ocr32_beam_replay");
    a->steps_run = evals;
    return 0;
}

extern "C" int mit_ocr32_decode(const MitOcr32Decoder *dec, MitOcr32DecodeArgs *a, void *stream) {
    if (!dec || !a) return mit_set_error("mit_ocr32_decode: null argument");
    const int N = a->N, L = a->L, T = a->max_seq_length, D = dec->dict_size;
    if (N <= 0 || L <= 0 || T <= 0 || D <= 0) return mit_set_error("mit_ocr32_decode: empty problem");
    if (!a->mem_k || !a->mem_v || !a->mem_len || !a->workspace || !a->res_tok || !a->res_len || !a->res_prob || !a->colors || !dec->embd ||
        !dec->pe)
        return mit_set_error("mit_ocr32_decode: null buffer");
    if (a->workspace_bytes < carve(nullptr, nullptr, N, T, D)) return mit_set_error("mit_ocr32_decode: workspace too small");
    if (T + 2 > dec->pe_len) return mit_set_error("mit_ocr32_decode: positional table (%d rows) too short for %d steps", dec->pe_len, T);
    if (a->max_finished < 1 || a->max_finished > 2) return mit_set_error("mit_ocr32_decode: max_finished must be 1 or 2 (got %d)", a->max_finished);
    if (a->start_tok < 0 || a->start_tok >= D || a->end_tok < 0 || a->end_tok >= D) return mit_set_error("mit_ocr32_decode: token out of range");
    if (dec->color_heads.N > 8 || dec->color1.N != 64) return mit_set_error("mit_ocr32_decode: unexpected colour head shapes");
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    carve(&w, (char *)a->workspace, N, T, D);
    const int R = N * BEAMS;
    const int P = T + 1;
    const int64_t Dp = (D + 3) / 4 * 4;
    const int64_t PE_ = (int64_t)P * E;   // floats between beam rows of the K / V / output histories
    const int hist_ld = T + 2, src_ld = P;

    hipLaunchKernelGGL(ocr32_fill_rows_kernel, dim3(64), dim3(256), 0, s, w.hist, (int64_t)2 * R * hist_ld, a->start_tok, w.src, src_ld,
                       (int64_t)2 * R * src_ld, R);
    MIT_CHECK_HIP(hipMemsetAsync(w.done, 0, (size_t)N * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.fin_cnt, 0, (size_t)N * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.done_count, 0, 4, s));
    // The few-row form of a step (as in mit_ocr48_decode): every Linear as one wave per 32 x 32 output block on bf16-plane activations
    // (pgemm_rows.h) — the embedding, LayerNorm and attention kernels hand the planes over, the residual stream and the histories stay
    // fp32.  Needs a split GEMM mode and plane-packed weights; else (and with args->form == 1) the tiled GEMM on fp32 activations.
    const int gmode = mit_gemm_mode_get();
    bool rows_path = a->form != 1 && (gmode == 6 || gmode == 9) && R <= ROWS_MAX && rows_ok(dec->pred1);
    for (int l = 0; l < 2 && rows_path; ++l) {
        const MitOcrDecoderLayer &ly = dec->layers[l];
        rows_path = rows_ok(ly.qkv) && rows_ok(ly.out) && rows_ok(ly.q2) && rows_ok(ly.out2) && rows_ok(ly.ff1) && rows_ok(ly.ff2);
    }
    // `pred` (N = the dictionary) takes the planar form when its width allows, else the tile on pred1's fp32 output
    const bool pred_rows = rows_path && dec->pred.w_split && dec->pred.Kp == dec->pred.K && (dec->pred.K % 16) == 0 && (dec->pred.N % 4) == 0;
    const int ff2_splitk = R <= FF2_SPLITK_MAX_ROWS ? 1 : 0;
    const int64_t Rp = w.Rp;
    const OcrPlanes none{nullptr, 0, 0};
    const OcrPlanes x_pl = rows_path ? OcrPlanes{w.x_p, Rp, E / 8} : none;
    const OcrPlanes att_pl = rows_path ? OcrPlanes{w.att_p, Rp, E / 8} : none;
    // evaluation 0 (:529-531): one hypothesis per line = <S>; run on all five rows of the line (identical), the bookkeeping reads the first
    hipLaunchKernelGGL(ocr32_embed_kernel, dim3(grid1d((int64_t)R * (E / 8))), dim3(256), 0, s, w.hist, (int64_t)hist_ld, dec->embd, dec->pe, 0,
                       w.x, R, x_pl);

    int cur = 0, evals = 0;
    for (int step = 0; step <= T; ++step) {
        const int64_t so = (int64_t)step * E;
        const int *src = w.src + (int64_t)cur * R * src_ld;
        for (int l = 0; l < 2; ++l) {
            const MitOcrDecoderLayer &ly = dec->layers[l];
            float *qc = w.qkv + (int64_t)(l * 3 + 0) * R * PE_;
            float *kc = w.qkv + (int64_t)(l * 3 + 1) * R * PE_;
            float *vc = w.qkv + (int64_t)(l * 3 + 2) * R * PE_;
            const float *mk = a->mem_k + (int64_t)l * N * L * E;
            const float *mv = a->mem_v + (int64_t)l * N * L * E;
            // the last layer's output row goes straight to position `step` of the row's output history (:462-463)
            float *out3 = l == 0 ? w.x : w.decoded + so;
            const int64_t out3_rs = l == 0 ? E : PE_;
            if (rows_path) {
                // self-attention over the layer's input history (:444-453); q | k | v of the new row land at position `step` of the row's slot
                if (pgemm(ly.qkv, w.x_p, Rp, R, qc + so, PE_, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s, E, (int64_t)R * PE_)) return 1;
                if (attention(qc + so, PE_, kc, vc, PE_, src, src_ld, 1, nullptr, step + 1, nullptr, R, s, att_pl)) return 1;
                if (pgemm(ly.out, w.att_p, Rp, R, w.y, E, MIT_ACT_NONE, w.x, E, nullptr, 0, s)) return 1;
                if (layernorm(w.y, ly.ln1_w, ly.ln1_b, w.x, E, R, x_pl, s)) return 1;
                // cross-attention over the line's memory with its key mask (:454-456)
                if (pgemm(ly.q2, w.x_p, Rp, R, w.q2, E, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s)) return 1;
                if (attention(w.q2, E, mk, mv, (int64_t)L * E, nullptr, 0, BEAMS, a->mem_len, L, nullptr, R, s, att_pl)) return 1;
                if (pgemm(ly.out2, w.att_p, Rp, R, w.y, E, MIT_ACT_NONE, w.x, E, nullptr, 0, s)) return 1;
                if (layernorm(w.y, ly.ln2_w, ly.ln2_b, w.x, E, R, x_pl, s)) return 1;
                // feed forward (:457-460): the hidden activations exist as planes only
                if (pgemm(ly.ff1, w.x_p, Rp, R, nullptr, 0, MIT_ACT_RELU, nullptr, 0, w.ffh_p, Rp, s)) return 1;
                if (pgemm(ly.ff2, w.ffh_p, Rp, R, w.y, E, MIT_ACT_NONE, w.x, E, nullptr, 0, s, 0, 0, ff2_splitk)) return 1;
                if (layernorm(w.y, ly.ln3_w, ly.ln3_b, out3, out3_rs, R, x_pl, s)) return 1;
            } else {
                if (gemm(ly.qkv, w.x, E, qc + so, PE_, R, MIT_ACT_NONE, nullptr, 0, s, E, (int64_t)R * PE_)) return 1;
                if (attention(qc + so, PE_, kc, vc, PE_, src, src_ld, 1, nullptr, step + 1, w.att, R, s, none)) return 1;
                if (gemm(ly.out, w.att, E, w.y, E, R, MIT_ACT_NONE, w.x, E, s)) return 1;
                if (layernorm(w.y, ly.ln1_w, ly.ln1_b, w.x, E, R, none, s)) return 1;
                if (gemm(ly.q2, w.x, E, w.q2, E, R, MIT_ACT_NONE, nullptr, 0, s)) return 1;
                if (attention(w.q2, E, mk, mv, (int64_t)L * E, nullptr, 0, BEAMS, a->mem_len, L, w.att, R, s, none)) return 1;
                if (gemm(ly.out2, w.att, E, w.y, E, R, MIT_ACT_NONE, w.x, E, s)) return 1;
                if (layernorm(w.y, ly.ln2_w, ly.ln2_b, w.x, E, R, none, s)) return 1;
                if (gemm(ly.ff1, w.x, E, w.ffh, FF, R, MIT_ACT_RELU, nullptr, 0, s)) return 1;
                if (gemm(ly.ff2, w.ffh, FF, w.y, E, R, MIT_ACT_NONE, w.x, E, s)) return 1;
                if (layernorm(w.y, ly.ln3_w, ly.ln3_b, out3, out3_rs, R, none, s)) return 1;
            }
        }
        if (rows_path && pred_rows) {
            if (pgemm(dec->pred1, w.x_p, Rp, R, nullptr, 0, MIT_ACT_RELU, nullptr, 0, w.p1_p, Rp, s)) return 1;
            if (pgemm(dec->pred, w.p1_p, Rp, R, w.logits, Dp, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s)) return 1;
        } else {
            if (rows_path) {
                if (pgemm(dec->pred1, w.x_p, Rp, R, w.p1, E, MIT_ACT_RELU, nullptr, 0, nullptr, 0, s)) return 1;
            } else {
                if (gemm(dec->pred1, w.decoded + so, PE_, w.p1, E, R, MIT_ACT_RELU, nullptr, 0, s)) return 1;
            }
            if (gemm(dec->pred, w.p1, E, w.logits, Dp, R, MIT_ACT_NONE, nullptr, 0, s)) return 1;
        }
        if (a->trace_logits)
            MIT_CHECK_HIP(hipMemcpy2DAsync(a->trace_logits + (int64_t)step * R * D, (size_t)D * 4, w.logits, (size_t)Dp * 4, (size_t)D * 4, R,
                                           hipMemcpyDeviceToDevice, s));
        ocrk_logsoftmax_top5(w.logits, Dp, R, D, -1, w.vals, w.idx, nullptr, s);
        cur = launch_beam(w, w.vals, w.idx, dec->embd, dec->pe, x_pl, a, step, cur, s);
        evals = step + 1;
        if (a->trace_hist)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_hist + (int64_t)step * R * hist_ld, w.hist + (int64_t)cur * R * hist_ld, (size_t)R * hist_ld * 4,
                                         hipMemcpyDeviceToDevice, s));
        MIT_CHECK_LAUNCH("mit_ocr32_decode");
        if (step >= 1 && (step % 4 == 3) && step < T) {   // early exit (:573-574) without a per-step sync
            int dc = 0;
            MIT_CHECK_HIP(hipMemcpyAsync(&dc, w.done_count, 4, hipMemcpyDeviceToHost, s));
            MIT_CHECK_HIP(hipStreamSynchronize(s));
            if (dc >= N) break;
        }
    }
    hipLaunchKernelGGL(ocr32_finalize_kernel, dim3(N), dim3(64), 0, s, w.hist + (int64_t)cur * R * hist_ld, hist_ld,
                       w.src + (int64_t)cur * R * src_ld, src_ld, w.lsum + (int64_t)cur * R, w.fin_tok, w.fin_src, w.fin_len, w.fin_mean,
                       w.fin_cnt, N, evals, a->res_tok, a->res_len, a->res_prob, w.sel_src);
    // colour heads over the chosen hypothesis's whole output history (:586-593)
    hipLaunchKernelGGL(ocr32_gather_kernel, dim3(grid1d((int64_t)N * P * (E / 4))), dim3(256), 0, s, w.decoded, PE_, w.sel_src, (int64_t)N * P, P,
                       w.sel_dec);
    if (gemm(dec->color1, w.sel_dec, E, w.cfeat, 64, N * P, MIT_ACT_RELU, nullptr, 0, s)) return 1;
    if (gemm(dec->color_heads, w.cfeat, 64, a->colors, 8, N * P, MIT_ACT_NONE, nullptr, 0, s)) return 1;
    if (a->res_src) MIT_CHECK_HIP(hipMemcpyAsync(a->res_src, w.sel_src, (size_t)N * src_ld * 4, hipMemcpyDeviceToDevice, s));
    MIT_CHECK_LAUNCH("mit_ocr32_decode");
    a->steps_run = evals;
    return 0;
}
