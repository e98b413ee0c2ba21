// mocr_decoder.hip — HuggingFace ``generate`` of the manga-ocr recogniser after its encoder, as one native call (mit_mocr_decode):
// BertLMHeadModel with cross-attention under VisionEncoderDecoderModel (reference: manga_translator/ocr/model_manga_ocr.py:132-295, whose
// text comes from manga_ocr's ``model.generate(x[None], max_length=300)``), beam search as transformers' generation/utils.py::_beam_search.
//
// What differs from the 32px loop (ocr32_decoder.hip), whose layout this follows:
//   * every size is a run-time value read from the model's config (hidden, heads, FFN, vocabulary, layers, beams): one wave per row or
//     per head with lane-strided loops instead of compile-time widths;
//   * the embedding is word + token-type 0 + position -> LayerNorm, the activation the erf GELU, the LM head dense + GELU + LayerNorm
//     -> vocabulary Linear with bias;
//   * the candidates of a step are the top 2 * num_beams over beams x vocabulary of (running score + log-probability), after the
//     no-repeat-n-gram ban; a candidate that ends in EOS (or reaches max_length) inside the first num_beams enters the line's list of
//     finished hypotheses with score sum / generated_length ** length_penalty, the first num_beams others run on;
//   * a line is done when its finished list is full (early_stopping) or when the best running score, divided by the current length
//     ** length_penalty, can no longer beat the worst finished one (the early-stop heuristic, sticky).  HuggingFace keeps running such
//     a line while others live but can no longer change it (the -1e9 penalties of _update_finished_beams); here its rows stay in place
//     and are not touched again.
// The K / V row of (beam row, position) is written once (the query of a step is used by that step alone and not kept); each beam row keeps a table src[t] = the row that holds position t of its
// history, copied from the parent by the bookkeeping kernel (as in the 32px loop) — the history is never re-projected or moved.
// Scores are summed in double from fp32 log-probabilities (HuggingFace sums in fp32; tests compare within 1e-3 relative).

#include <hip/hip_runtime.h>
#include <math.h>
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

constexpr int BEAMS_MAX = 8;
constexpr int KEEP_MAX = 2 * BEAMS_MAX;   // candidates looked at per line and step
constexpr int ROWS_MAX = 2560;            // rows up to which a step runs in the few-row form (as the 32px and 48px loops)
constexpr int HEADS_MAX = 16;             // one wave per head, one workgroup per row

struct Ws {
    float *x, *y, *q, *kv, *att, *q2, *ffh, *t1, *t2, *logits, *logp, *vals;
    double *run, *fin_score;
    int *idx, *hist, *src, *fin_tok, *fin_len, *fin_order, *fin_cnt, *heur, *done, *done_count;
    uint16_t *x_p, *att_p, *ffh_p, *t1_p, *t2_p;
    int64_t Rp;
};

int64_t carve(Ws *w, char *base, int N, int nb, int T, int H, int I, int V, int Ln) {
    const int64_t R = (int64_t)N * nb;
    const int64_t Vp = (V + 3) / 4 * 4;
    const int K = 2 * nb;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    Ws o;
    o.x = (float *)take(R * H * 4);
    o.y = (float *)take(R * H * 4);
    o.q = (float *)take(R * H * 4);
    o.kv = (float *)take((int64_t)Ln * 2 * R * T * H * 4);
    o.att = (float *)take(R * H * 4);
    o.q2 = (float *)take(R * H * 4);
    o.ffh = (float *)take(R * I * 4);
    o.t1 = (float *)take(R * H * 4);
    o.t2 = (float *)take(R * H * 4);
    o.logits = (float *)take(R * Vp * 4);
    o.logp = (float *)take(R * (int64_t)V * 4);
    o.vals = (float *)take(R * K * 4);
    o.run = (double *)take(2 * R * 8);
    o.fin_score = (double *)take(R * 8);
    o.idx = (int *)take(R * K * 4);
    o.hist = (int *)take(2 * R * T * 4);
    o.src = (int *)take(2 * R * T * 4);
    o.fin_tok = (int *)take(R * T * 4);
    o.fin_len = (int *)take(R * 4);
    o.fin_order = (int *)take(R * 4);
    o.fin_cnt = (int *)take((int64_t)N * 4);
    o.heur = (int *)take((int64_t)N * 4);
    o.done = (int *)take((int64_t)N * 4);
    o.done_count = (int *)take(256);
    o.Rp = (R + 31) / 32 * 32;
    o.x_p = (uint16_t *)take(3 * H * o.Rp * 2);
    o.att_p = (uint16_t *)take(3 * H * o.Rp * 2);
    o.ffh_p = (uint16_t *)take(3 * I * o.Rp * 2);
    o.t1_p = (uint16_t *)take(3 * H * o.Rp * 2);
    o.t2_p = (uint16_t *)take(3 * H * o.Rp * 2);
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

// LayerNorm of one row by one wave: val(d) is the row's value at d (recomputed in every pass: the operands stay in L1), the result goes
// to y as fp32 and, for the few-row form, to the planes the next Linear reads (the same expression again, eight values per lane).
template <class F>
__device__ __forceinline__ void ln_row(F val, int D, const float *__restrict__ w, const float *__restrict__ b, float eps, float *__restrict__ y,
                                       const OcrPlanes &pl, int row, int lane) {
    float sum = 0.f;
    for (int d = lane; d < D; d += 64) sum += val(d);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)D;
    float var = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float t = val(d) - mean;
        var += t * t;
    }
    for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
    const float rstd = 1.0f / sqrtf(var / (float)D + eps);
    for (int d = lane; d < D; d += 64) y[d] = (val(d) - mean) * rstd * w[d] + b[d];
    if (!pl.p) return;
    for (int c = lane; c < D / 8; c += 64) {
        __attribute__((aligned(16))) float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (val(c * 8 + j) - mean) * rstd * w[c * 8 + j] + b[c * 8 + j];
        store_cells(pl, c, row, v);
    }
}

__global__ __launch_bounds__(256) void mocr_layernorm_kernel(const float *__restrict__ in, int64_t in_rs, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ out, int64_t out_rs, int rows,
                                                             int D, float eps, OcrPlanes pl) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = in + (int64_t)row * in_rs;
    ln_row([&](int d) { return x[d]; }, D, w, b, eps, out + (int64_t)row * out_rs, pl, row, lane);
}

// BertEmbeddings: LayerNorm((word[tok] + token_type[0]) + position[pos]) for the last token of every beam row
__global__ __launch_bounds__(256) void mocr_embed_ln_kernel(const int *__restrict__ hist, int hist_ld, int pos, const float *__restrict__ we,
                                                            const float *__restrict__ pe, const float *__restrict__ te,
                                                            const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ out,
                                                            int rows, int D, float eps, OcrPlanes pl) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *a = we + (int64_t)hist[(int64_t)row * hist_ld + pos] * D;
    const float *p = pe + (int64_t)pos * D;
    ln_row([&](int d) { return (a[d] + te[d]) + p[d]; }, D, w, b, eps, out + (int64_t)row * D, pl, row, lane);
}

// ---- attention of ONE query per beam row: one workgroup per row, one wave per head (heads <= 16, head_dim % 8 == 0) ----
// Keys / values of position t come from row (src ? src[r * src_ld + t] : r / kv_div) of K / V (row stride kv_rs floats, position stride
// E = heads * hd).  The query is already scaled (the projection's epilogue carries head_dim ** -0.5).
__global__ __launch_bounds__(1024) void mocr_attention_kernel(const float *__restrict__ Q, int64_t q_rs, const float *__restrict__ K,
                                                              const float *__restrict__ V, int64_t kv_rs, const int *__restrict__ src,
                                                              int src_ld, int kv_div, int Tk, float *__restrict__ O, int R, int heads, int hd,
                                                              OcrPlanes opl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // q [E] | p [heads][Tk] | row [Tk] ints
    const int r = blockIdx.x;
    if (r >= R) return;
    const int E = heads * hd, nthr = heads * 64;
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    float *qs = smem;
    float *ps = smem + E + h * Tk;
    int *rows = reinterpret_cast<int *>(smem + E + heads * Tk);
    const int line = r / kv_div;
    const int n = Tk;
    for (int i = tid; i < E; i += nthr) qs[i] = Q[(int64_t)r * q_rs + i];
    for (int t = tid; t < n; t += nthr) rows[t] = src ? src[(int64_t)r * src_ld + t] : line;
    __syncthreads();
    float mx = -INFINITY;
    for (int t = lane; t < n; t += 64) {
        const float4 *k4 = reinterpret_cast<const float4 *>(K + (int64_t)rows[t] * kv_rs + (int64_t)t * E + h * hd);
        const float4 *q4 = reinterpret_cast<const float4 *>(qs + h * hd);
        float acc = 0.f;
        for (int d = 0; d < hd / 4; ++d) {
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
    __syncthreads();   // every lane's p[t] is visible to the wave; every wave is past its reads of q
    const float inv = 1.f / sum;
    float *oh = qs + h * hd;   // the head's query slice is dead (only this wave read it): its outputs are staged there for the planes
    for (int d = lane; d < hd; d += 64) {   // lane d sums channel d over t in four interleaved partial sums
        const float *vb = V + h * hd + d;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        int t = 0;
        for (; t + 4 <= n; t += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += ps[t + j] * vb[(int64_t)rows[t + j] * kv_rs + (int64_t)(t + j) * E];
        }
        for (; t < n; ++t) a[0] += ps[t] * vb[(int64_t)rows[t] * kv_rs + (int64_t)t * E];
        const float o0 = ((a[0] + a[1]) + (a[2] + a[3])) * inv;
        if (opl.p) oh[d] = o0;
        else O[(int64_t)r * E + h * hd + d] = o0;
    }
    if (opl.p) {   // the output feeds a few-row Linear only: bf16 planes instead of fp32
        wave_lds_fence();
        for (int c = lane; c < hd / 8; c += 64) store_cells(opl, h * (hd / 8) + c, r, oh + c * 8);
    }
}

// ---- log-softmax, the no-repeat-n-gram ban and the row's K best (value, token), ties to the lower token ----
// One workgroup per beam row.  is_logp: the input already holds log-probabilities (beam replay).  logp_out [R][V] receives the
// processed log-probabilities (banned tokens -inf), which the K selection passes then read back.
__global__ __launch_bounds__(256) void mocr_logprob_topk_kernel(const float *__restrict__ in, int64_t ld, int V, int is_logp,
                                                                const int *__restrict__ hist, int hist_ld, int cur_len, int ngram, int K,
                                                                float *__restrict__ logp_out, float *__restrict__ vals, int *__restrict__ idx) {
    __shared__ float s_f[4];
    __shared__ int s_i[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *x = in + (int64_t)r * ld;
    float *lp = logp_out + (int64_t)r * V;
    if (!is_logp) {
        float mx = -INFINITY;
        for (int d = tid; d < V; d += 256) mx = fmaxf(mx, x[d]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) s_f[wv] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
        __syncthreads();
        float sum = 0.f;
        for (int d = tid; d < V; d += 256) sum += expf(x[d] - mx);
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) s_f[wv] = sum;
        __syncthreads();
        sum = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
        __syncthreads();
        const float lse = logf(sum);
        for (int d = tid; d < V; d += 256) lp[d] = (x[d] - mx) - lse;
    } else {
        for (int d = tid; d < V; d += 256) lp[d] = x[d];
    }
    __syncthreads();
    // NoRepeatNGramLogitsProcessor: token hist[i + n - 1] is banned when hist[i .. i + n - 2] equals the last n - 1 tokens
    if (ngram > 0 && cur_len + 1 >= ngram) {
        const int *hrow = hist + (int64_t)r * hist_ld;
        for (int i = tid; i + ngram <= cur_len; i += 256) {
            bool same = true;
            for (int j = 0; j < ngram - 1; ++j) same = same && hrow[i + j] == hrow[cur_len - (ngram - 1) + j];
            const int tok = hrow[i + ngram - 1];
            if (same && tok >= 0 && tok < V) lp[tok] = -INFINITY;
        }
        __syncthreads();
    }
    float last_v = INFINITY;
    int last_i = -1;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int d = tid; d < V; d += 256) {
            const float v = lp[d];
            const bool after = v < last_v || (v == last_v && d > last_i);      // not yet selected
            const bool better = v > bv || (v == bv && d < bi);
            if (after && better) bv = v, bi = d;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
        if (lane == 0) s_f[wv] = bv, s_i[wv] = bi;
        __syncthreads();
        bv = s_f[0], bi = s_i[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (s_f[j] > bv || (s_f[j] == bv && s_i[j] < bi)) bv = s_f[j], bi = s_i[j];
        __syncthreads();
        if (tid == 0) vals[(int64_t)r * K + k] = bv, idx[(int64_t)r * K + k] = bi;
        last_v = bv, last_i = bi;
    }
}

// ---- bookkeeping ----
__global__ void mocr_fill_kernel(int *__restrict__ hist, int T, int64_t n_hist, int start_tok, int pad_tok, int *__restrict__ src, int R,
                                 double *__restrict__ run, int *__restrict__ fin_tok, int64_t n_fin, int *__restrict__ fin_order, int nb,
                                 int *__restrict__ heur, int *__restrict__ done, int *__restrict__ fin_cnt, int N, int *__restrict__ done_count) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = i; j < n_hist; j += stride) {
        hist[j] = (j % T) == 0 ? start_tok : pad_tok;
        src[j] = (int)((j / T) % R);   // a row's own slot until a parent's table is copied in
    }
    for (int64_t j = i; j < n_fin; j += stride) fin_tok[j] = pad_tok;
    for (int64_t j = i; j < 2 * (int64_t)R; j += stride) run[j] = 0.0;
    for (int64_t j = i; j < R; j += stride) fin_order[j] = (int)(j % nb);
    for (int64_t j = i; j < N; j += stride) heur[j] = 1, done[j] = 0, fin_cnt[j] = 0;
    if (i == 0) *done_count = 0;
}

struct BeamBufs {
    const int *hist_in;
    int *hist_out;
    const int *src_in;
    int *src_out;
    const double *run_in;
    double *run_out;
    int *fin_tok, *fin_len, *fin_order, *fin_cnt, *heur, *done, *done_count;
    double *fin_score;
};

// One wave per line.  Candidate c = (beam c / K, rank c % K inside the beam's own top K); key = running score + log-probability (at step 0
// only beam 0 counts: HuggingFace starts the others at -1e9).  The K best keys overall, in order, are what torch.topk over beams x vocab
// returns (a token outside its beam's top K cannot be inside the overall top K).
__global__ __launch_bounds__(64) void mocr_beam_kernel(const float *__restrict__ vals, const int *__restrict__ idx, BeamBufs b, int N, int nb,
                                                       int step, int T, int eos_tok, int early_stopping, double length_penalty) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N) return;
    __shared__ double s_key[BEAMS_MAX * KEEP_MAX];
    __shared__ int s_sorted[KEEP_MAX];   // rank -> candidate
    __shared__ int s_hit[KEEP_MAX];      // rank -> ends here (EOS or max_length)
    __shared__ int s_keep[BEAMS_MAX];    // running beam -> rank
    __shared__ int s_slot[BEAMS_MAX];    // rank < nb -> finished slot written this step (-1: none)
    const int K = 2 * nb, C = nb * K, row0 = n * nb;
    if (b.done[n]) {   // (uniform over the wave) the line's rows stay as they are, in both buffers
        for (int i = lane; i < nb * T; i += 64) {
            b.hist_out[(int64_t)row0 * T + i] = b.hist_in[(int64_t)row0 * T + i];
            b.src_out[(int64_t)row0 * T + i] = b.src_in[(int64_t)row0 * T + i];
        }
        if (lane < nb) b.run_out[row0 + lane] = b.run_in[row0 + lane];
        return;
    }
    for (int c = lane; c < C; c += 64) {
        const int beam = c / K;
        const double run = (step == 0 && beam > 0) ? -1.0e9 : b.run_in[row0 + beam];
        s_key[c] = run + (double)vals[(int64_t)(row0 + beam) * K + (c - beam * K)];
    }
    __syncthreads();
    for (int c = lane; c < C; c += 64) {
        const double key = s_key[c];
        int rank = 0;
        for (int o = 0; o < C; ++o) {
            const double ok = s_key[o];
            if (ok > key || (ok == key && o < c)) ++rank;
        }
        if (rank < K) s_sorted[rank] = c;
    }
    __syncthreads();
    const int hit_all = step + 2 >= T;   // the sequence reaches max_length with this token
    const double len_pow = pow((double)(step + 1), length_penalty);
    if (lane == 0) {
        int kept = 0;
        for (int q = 0; q < K; ++q) {
            const int c = s_sorted[q], beam = c / K;
            const int tok = idx[(int64_t)(row0 + beam) * K + (c - beam * K)];
            s_hit[q] = hit_all || tok == eos_tok;
            if (!s_hit[q] && kept < nb) s_keep[kept++] = q;
        }
        for (int q = 0; q < K && kept < nb; ++q)   // fewer than nb candidates run on (max_length): the ended ones fill up, as top-k over -1e9 does
            if (s_hit[q]) s_keep[kept++] = q;
        int cnt = b.fin_cnt[n];
        int *order = b.fin_order + row0;
        double *fscore = b.fin_score + row0;
        for (int q = 0; q < nb; ++q) {
            s_slot[q] = -1;
            if (!s_hit[q]) continue;
            const double sc = s_key[s_sorted[q]] / len_pow;
            int slot, m;
            if (cnt < nb) {
                slot = order[cnt];
                m = cnt++;
            } else {
                slot = order[nb - 1];
                if (!(sc > fscore[slot])) continue;
                m = nb - 1;
            }
            while (m > 0 && sc > fscore[order[m - 1]]) {   // sorted insert, descending; an equal score stays behind the earlier one
                order[m] = order[m - 1];
                --m;
            }
            order[m] = slot;
            fscore[slot] = sc;
            b.fin_len[row0 + slot] = step + 2;
            s_slot[q] = slot;
        }
        b.fin_cnt[n] = cnt;
    }
    __syncthreads();
    for (int q = 0; q < nb; ++q) {   // finished hypotheses of this step: the parent's tokens 0 .. step + the new one, pad beyond
        const int slot = s_slot[q];
        if (slot < 0) continue;
        const int c = s_sorted[q], beam = c / K;
        const int *hp = b.hist_in + (int64_t)(row0 + beam) * T;
        int *ft = b.fin_tok + (int64_t)(row0 + slot) * T;
        const int tok = idx[(int64_t)(row0 + beam) * K + (c - beam * K)];
        for (int t = lane; t < T; t += 64) ft[t] = t == step + 1 ? tok : hp[t];   // (positions past step hold the pad token)
    }
    for (int k = 0; k < nb; ++k) {
        const int q = s_keep[k], c = s_sorted[q], beam = c / K;
        const int prow = row0 + beam, row = row0 + k;
        const int tok = idx[(int64_t)prow * K + (c - beam * K)];
        for (int t = lane; t < T; t += 64) {
            b.hist_out[(int64_t)row * T + t] = t == step + 1 ? tok : b.hist_in[(int64_t)prow * T + t];
            b.src_out[(int64_t)row * T + t] = t <= step ? b.src_in[(int64_t)prow * T + t] : row;
        }
        if (lane == 0) b.run_out[row] = s_key[c] + (s_hit[q] ? -1.0e9 : 0.0);
    }
    __syncthreads();
    if (lane == 0) {
        const int cnt = b.fin_cnt[n];
        int heur = b.heur[n];
        if (cnt == nb) {   // _check_early_stop_heuristic: can the best running beam still beat the worst finished one?
            const double worst = b.fin_score[row0 + b.fin_order[row0 + nb - 1]];
            const double best = (s_key[s_sorted[s_keep[0]]] + (s_hit[s_keep[0]] ? -1.0e9 : 0.0)) / len_pow;
            if (!(best > worst)) heur = 0;
        }
        b.heur[n] = heur;
        const int isdone = (early_stopping ? cnt == nb : !heur) || hit_all;
        if (isdone) {
            b.done[n] = 1;
            atomicAdd(b.done_count, 1);
        }
    }
}

__global__ __launch_bounds__(64) void mocr_finalize_kernel(const int *__restrict__ fin_tok, const int *__restrict__ fin_len,
                                                           const double *__restrict__ fin_score, const int *__restrict__ fin_order,
                                                           const int *__restrict__ fin_cnt, int N, int nb, int T, int pad_tok,
                                                           int *__restrict__ res_tok, int *__restrict__ res_len, float *__restrict__ res_score) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N) return;
    const int have = fin_cnt[n] > 0;
    const int slot = n * nb + fin_order[n * nb];
    for (int t = lane; t < T; t += 64) res_tok[(int64_t)n * T + t] = have ? fin_tok[(int64_t)slot * T + t] : pad_tok;
    if (lane == 0) {
        res_len[n] = have ? fin_len[slot] : 0;
        res_score[n] = have ? (float)fin_score[slot] : -1.0e9f;
    }
}

int layernorm(const float *in, int64_t in_rs, const float *w, const float *b, float *out, int64_t out_rs, int rows, int D, float eps,
              const OcrPlanes &pl, hipStream_t s) {
    MitProbeScope probe("mocr_layernorm_kernel", s, 10.0 * (double)rows * D);
    hipLaunchKernelGGL(mocr_layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, in_rs, w, b, out, out_rs, rows, D, eps, pl);
    return 0;
}

int attention(const float *Q, int64_t q_rs, const float *K, const float *V, int64_t kv_rs, const int *src, int src_ld, int kv_div, int Tk,
              float *O, int R, int heads, int hd, hipStream_t s, const OcrPlanes &opl) {
    const size_t smem = ((size_t)heads * hd + (size_t)(heads + 1) * Tk) * 4;
    if (Tk <= 0 || smem > 64 * 1024) return mit_set_error("mit_mocr_decode: attention over %d keys does not fit the LDS form", Tk);
    MitProbeScope probe("mocr_attention_kernel", s, 8.0 * (double)R * Tk * heads * hd);
    hipLaunchKernelGGL(mocr_attention_kernel, dim3(R), dim3(heads * 64), smem, s, Q, q_rs, K, V, kv_rs, src, src_ld, kv_div, Tk, O, R, heads,
                       hd, opl);
    return 0;
}

int grid1d(int64_t total) { return (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024); }

int check_search(const char *who, const MitMocrDecodeArgs *a, int V) {
    if (a->N <= 0) return mit_set_error("%s: N must be positive", who);
    if (a->num_beams < 1 || a->num_beams > BEAMS_MAX) return mit_set_error("%s: num_beams must be in 1 .. %d (got %d)", who, BEAMS_MAX, a->num_beams);
    if (a->max_length < 2) return mit_set_error("%s: max_length must be at least 2 (got %d)", who, a->max_length);
    if (a->no_repeat_ngram_size < 0) return mit_set_error("%s: no_repeat_ngram_size must not be negative", who);
    if (a->early_stopping != 0 && a->early_stopping != 1) return mit_set_error("%s: early_stopping must be 0 or 1 (\"never\" is not implemented)", who);
    if (V < 2 * a->num_beams) return mit_set_error("%s: the vocabulary (%d) is smaller than 2 * num_beams", who, V);
    if (a->eos_token_id < 0 || a->eos_token_id >= V || a->pad_token_id < 0 || a->pad_token_id >= V || a->decoder_start_token_id < 0 ||
        a->decoder_start_token_id >= V)
        return mit_set_error("%s: eos / pad / decoder_start token out of range", who);
    if (!(a->length_penalty == a->length_penalty)) return mit_set_error("%s: length_penalty is not a number", who);
    if (!a->workspace || !a->res_tok || !a->res_len || !a->res_score) return mit_set_error("%s: null buffer", who);
    return 0;
}

void init_state(const Ws &w, const MitMocrDecodeArgs *a, hipStream_t s) {
    const int N = a->N, nb = a->num_beams, T = a->max_length, R = N * nb;
    hipLaunchKernelGGL(mocr_fill_kernel, dim3(64), dim3(256), 0, s, w.hist, T, (int64_t)2 * R * T, a->decoder_start_token_id, a->pad_token_id,
                       w.src, R, w.run, w.fin_tok, (int64_t)R * T, w.fin_order, nb, w.heur, w.done, w.fin_cnt, N, w.done_count);
}

// log-probabilities -> ban -> per-row top K -> bookkeeping.  Reads buffer `cur`, returns the buffer it wrote.
int launch_step(const Ws &w, const float *in, int64_t ld, int V, int is_logp, const MitMocrDecodeArgs *a, int step, int cur, hipStream_t s) {
    const int N = a->N, nb = a->num_beams, T = a->max_length, R = N * nb, K = 2 * nb;
    const int out = cur ^ 1;
    // greedy search ends a line at its first EOS whatever early_stopping says
    const int es = nb == 1 ? 1 : a->early_stopping;
    {
        MitProbeScope probe("mocr_logprob_topk_kernel", s, 4.0 * (double)R * V * (K + 3));
        hipLaunchKernelGGL(mocr_logprob_topk_kernel, dim3(R), dim3(256), 0, s, in, ld, V, is_logp, w.hist + (int64_t)cur * R * T, T, step + 1,
                           a->no_repeat_ngram_size, K, w.logp, w.vals, w.idx);
    }
    BeamBufs b;
    b.hist_in = w.hist + (int64_t)cur * R * T;
    b.hist_out = w.hist + (int64_t)out * R * T;
    b.src_in = w.src + (int64_t)cur * R * T;
    b.src_out = w.src + (int64_t)out * R * T;
    b.run_in = w.run + (int64_t)cur * R;
    b.run_out = w.run + (int64_t)out * R;
    b.fin_tok = w.fin_tok; b.fin_len = w.fin_len; b.fin_order = w.fin_order; b.fin_cnt = w.fin_cnt; b.heur = w.heur; b.done = w.done;
    b.done_count = w.done_count; b.fin_score = w.fin_score;
    MitProbeScope probe("mocr_beam_kernel", s, 8.0 * (double)R * T);
    hipLaunchKernelGGL(mocr_beam_kernel, dim3(N), dim3(64), 0, s, w.vals, w.idx, b, N, nb, step, T, a->eos_token_id, es, a->length_penalty);
    return out;
}

int finish(const Ws &w, MitMocrDecodeArgs *a, int steps_run, hipStream_t s) {
    hipLaunchKernelGGL(mocr_finalize_kernel, dim3(a->N), dim3(64), 0, s, w.fin_tok, w.fin_len, w.fin_score, w.fin_order, w.fin_cnt, a->N,
                       a->num_beams, a->max_length, a->pad_token_id, a->res_tok, a->res_len, a->res_score);
    a->steps_run = steps_run;
    return 0;
}

}  // namespace

// nn.LayerNorm of any width for the encoder: the decoder's own kernel without planes
extern "C" int mit_layernorm_wide(const float *in_dev, int64_t in_rowstride, const float *w_dev, const float *b_dev, float *out_dev,
                                  int64_t out_rowstride, int rows, int D, float eps, void *stream) {
    if (!in_dev || !w_dev || !b_dev || !out_dev) return mit_set_error("mit_layernorm_wide: null argument");
    if (rows <= 0) return mit_set_error("mit_layernorm_wide: rows must be positive");
    if (D < 1 || D > 8192) return mit_set_error("mit_layernorm_wide: D out of range (1 .. 8192, got %d)", D);
    if (in_rowstride < D || out_rowstride < D) return mit_set_error("mit_layernorm_wide: a row stride is shorter than D");
    if (layernorm(in_dev, in_rowstride, w_dev, b_dev, out_dev, out_rowstride, rows, D, eps, OcrPlanes{nullptr, 0, 0}, (hipStream_t)stream)) return 1;
    MIT_CHECK_LAUNCH("mit_layernorm_wide");
    return 0;
}

extern "C" int64_t mit_mocr_decode_workspace_bytes(int N, int num_beams, int max_length, int hidden, int inter, int vocab, int n_layers) {
    if (N <= 0 || num_beams <= 0 || max_length <= 0 || hidden < 0 || inter < 0 || vocab <= 0 || n_layers < 0) return 0;
    return carve(nullptr, nullptr, N, num_beams, max_length, hidden, inter, vocab, n_layers);
}

extern "C" int mit_mocr_beam_replay(const float *logp_dev, int steps, int vocab, MitMocrDecodeArgs *a, void *stream) {
    if (!a || !logp_dev) return mit_set_error("mit_mocr_beam_replay: null argument");
    if (vocab <= 0) return mit_set_error("mit_mocr_beam_replay: empty vocabulary");
    if (check_search("mit_mocr_beam_replay", a, vocab)) return 1;
    const int N = a->N, nb = a->num_beams, T = a->max_length, R = N * nb;
    if (steps <= 0 || steps > T - 1) return mit_set_error("mit_mocr_beam_replay: steps must be in 1 .. max_length - 1");
    if (a->workspace_bytes < carve(nullptr, nullptr, N, nb, T, 0, 0, vocab, 0)) return mit_set_error("mit_mocr_beam_replay: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    carve(&w, (char *)a->workspace, N, nb, T, 0, 0, vocab, 0);
    init_state(w, a, s);
    int cur = 0;
    for (int step = 0; step < steps; ++step) {
        cur = launch_step(w, logp_dev + (int64_t)step * R * vocab, vocab, vocab, 1, a, step, cur, s);
        if (a->trace_hist)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_hist + (int64_t)step * R * T, w.hist + (int64_t)cur * R * T, (size_t)R * T * 4,
                                         hipMemcpyDeviceToDevice, s));
    }
    a->form_run = 0;
    finish(w, a, steps, s);
    MIT_CHECK_LAUNCH("mit_mocr_beam_replay");
    return 0;
}

extern "C" int mit_mocr_decode(const MitMocrDecoder *dec, MitMocrDecodeArgs *a, void *stream) {
    if (!dec || !a) return mit_set_error("mit_mocr_decode: null argument");
    const int Ln = dec->n_layers, H = dec->hidden, heads = dec->heads, I = dec->inter, V = dec->vocab;
    if (Ln <= 0 || H <= 0 || heads <= 0 || I <= 0 || V <= 0 || !dec->layers) return mit_set_error("mit_mocr_decode: empty model");
    if (check_search("mit_mocr_decode", a, V)) return 1;
    const int N = a->N, L = a->L, nb = a->num_beams, T = a->max_length;
    if (heads > HEADS_MAX || H % heads != 0 || (H / heads) % 8 != 0 || H % 16 != 0 || I % 16 != 0)
        return mit_set_error("mit_mocr_decode: hidden %d / heads %d / intermediate %d not supported (heads <= %d, head_dim %% 8 == 0, sizes %% 16 == 0)",
                             H, heads, I, HEADS_MAX);
    if (L <= 0 || !a->mem_k || !a->mem_v) return mit_set_error("mit_mocr_decode: no encoder memory");
    if (!dec->word_emb || !dec->pos_emb || !dec->type_emb || !dec->emb_ln_w || !dec->emb_ln_b || !dec->head_ln_w || !dec->head_ln_b)
        return mit_set_error("mit_mocr_decode: null weight");
    if (T > dec->max_pos) return mit_set_error("mit_mocr_decode: max_length %d exceeds the position table (%d rows)", T, dec->max_pos);
    if (dec->head_out.N != V || dec->head_dense.N != H) return mit_set_error("mit_mocr_decode: unexpected LM head shapes");
    if (a->workspace_bytes < carve(nullptr, nullptr, N, nb, T, H, I, V, Ln)) return mit_set_error("mit_mocr_decode: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    carve(&w, (char *)a->workspace, N, nb, T, H, I, V, Ln);
    const int R = N * nb, hd = H / heads;
    const int64_t Vp = (V + 3) / 4 * 4;
    const int64_t PE_ = (int64_t)T * H;   // floats between beam rows of the K / V histories
    const float eps = dec->ln_eps;

    init_state(w, a, s);
    // The few-row form of a step (as in mit_ocr32_decode): every Linear as one wave per 32 x 32 output block on bf16-plane activations
    // (pgemm_rows.h); needs a split GEMM mode and plane-packed weights, else (and with args->form == 1) the tiled GEMM on fp32.
    const int gmode = mit_gemm_mode_get();
    bool rows_path = a->form != 1 && (gmode == 6 || gmode == 9) && R <= ROWS_MAX && rows_ok(dec->head_dense);
    for (int l = 0; l < Ln && rows_path; ++l) {
        const MitMocrLayer &ly = dec->layers[l];
        rows_path = rows_ok(ly.q) && rows_ok(ly.kv) && rows_ok(ly.out) && rows_ok(ly.q2) && rows_ok(ly.out2) && rows_ok(ly.ff1) && rows_ok(ly.ff2);
    }
    const bool out_rows = rows_path && rows_ok(dec->head_out);   // the vocabulary Linear: planar when its width allows, else the tile
    const int64_t Rp = w.Rp;
    const OcrPlanes none{nullptr, 0, 0};
    const OcrPlanes x_pl = rows_path ? OcrPlanes{w.x_p, Rp, H / 8} : none;
    const OcrPlanes att_pl = rows_path ? OcrPlanes{w.att_p, Rp, H / 8} : none;
    const OcrPlanes t2_pl = out_rows ? OcrPlanes{w.t2_p, Rp, H / 8} : none;
    a->form_run = rows_path ? (out_rows ? 2 : 1) : 0;

    int cur = 0, steps_run = 0;
    for (int step = 0; step + 1 < T; ++step) {
        const int64_t so = (int64_t)step * H;
        const int *src = w.src + (int64_t)cur * R * T;
        {
            MitProbeScope probe("mocr_embed_ln_kernel", s, 12.0 * (double)R * H);
            hipLaunchKernelGGL(mocr_embed_ln_kernel, dim3((R + 3) / 4), dim3(256), 0, s, w.hist + (int64_t)cur * R * T, T, step, dec->word_emb,
                               dec->pos_emb, dec->type_emb, dec->emb_ln_w, dec->emb_ln_b, w.x, R, H, eps, x_pl);
        }
        for (int l = 0; l < Ln; ++l) {
            const MitMocrLayer &ly = dec->layers[l];
            float *kc = w.kv + (int64_t)(l * 2 + 0) * R * PE_;
            float *vc = w.kv + (int64_t)(l * 2 + 1) * R * PE_;
            const float *mk = a->mem_k + (int64_t)l * N * L * H;
            const float *mv = a->mem_v + (int64_t)l * N * L * H;
            if (rows_path) {
                // self-attention: k | v of the new token land at position `step` of the row's own slot; q is read once and not kept
                if (pgemm(ly.q, w.x_p, Rp, R, w.q, H, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s)) return 1;
                if (pgemm(ly.kv, w.x_p, Rp, R, kc + so, PE_, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s, H, (int64_t)R * PE_)) return 1;
                if (attention(w.q, H, kc, vc, PE_, src, T, 1, step + 1, nullptr, R, heads, hd, s, att_pl)) return 1;
                if (pgemm(ly.out, w.att_p, Rp, R, w.y, H, MIT_ACT_NONE, w.x, H, nullptr, 0, s)) return 1;
                if (layernorm(w.y, H, ly.ln1_w, ly.ln1_b, w.x, H, R, H, eps, x_pl, s)) return 1;
                // cross-attention over the line's encoder memory
                if (pgemm(ly.q2, w.x_p, Rp, R, w.q2, H, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s)) return 1;
                if (attention(w.q2, H, mk, mv, (int64_t)L * H, nullptr, 0, nb, L, nullptr, R, heads, hd, s, att_pl)) return 1;
                if (pgemm(ly.out2, w.att_p, Rp, R, w.y, H, MIT_ACT_NONE, w.x, H, nullptr, 0, s)) return 1;
                if (layernorm(w.y, H, ly.ln2_w, ly.ln2_b, w.x, H, R, H, eps, x_pl, s)) return 1;
                // feed forward: the hidden activations exist as planes only
                if (pgemm(ly.ff1, w.x_p, Rp, R, nullptr, 0, MIT_ACT_GELU, nullptr, 0, w.ffh_p, Rp, s)) return 1;
                if (pgemm(ly.ff2, w.ffh_p, Rp, R, w.y, H, MIT_ACT_NONE, w.x, H, nullptr, 0, s)) return 1;
                if (layernorm(w.y, H, ly.ln3_w, ly.ln3_b, w.x, H, R, H, eps, x_pl, s)) return 1;
            } else {
                if (gemm(ly.q, w.x, H, w.q, H, R, MIT_ACT_NONE, nullptr, 0, s)) return 1;
                if (gemm(ly.kv, w.x, H, kc + so, PE_, R, MIT_ACT_NONE, nullptr, 0, s, H, (int64_t)R * PE_)) return 1;
                if (attention(w.q, H, kc, vc, PE_, src, T, 1, step + 1, w.att, R, heads, hd, s, none)) return 1;
                if (gemm(ly.out, w.att, H, w.y, H, R, MIT_ACT_NONE, w.x, H, s)) return 1;
                if (layernorm(w.y, H, ly.ln1_w, ly.ln1_b, w.x, H, R, H, eps, none, s)) return 1;
                if (gemm(ly.q2, w.x, H, w.q2, H, R, MIT_ACT_NONE, nullptr, 0, s)) return 1;
                if (attention(w.q2, H, mk, mv, (int64_t)L * H, nullptr, 0, nb, L, w.att, R, heads, hd, s, none)) return 1;
                if (gemm(ly.out2, w.att, H, w.y, H, R, MIT_ACT_NONE, w.x, H, s)) return 1;
                if (layernorm(w.y, H, ly.ln2_w, ly.ln2_b, w.x, H, R, H, eps, none, s)) return 1;
                if (gemm(ly.ff1, w.x, H, w.ffh, I, R, MIT_ACT_GELU, nullptr, 0, s)) return 1;
                if (gemm(ly.ff2, w.ffh, I, w.y, H, R, MIT_ACT_NONE, w.x, H, s)) return 1;
                if (layernorm(w.y, H, ly.ln3_w, ly.ln3_b, w.x, H, R, H, eps, none, s)) return 1;
            }
        }
        // BertLMPredictionHead: dense + GELU -> LayerNorm -> decoder (+ bias)
        if (rows_path) {
            if (pgemm(dec->head_dense, w.x_p, Rp, R, w.t1, H, MIT_ACT_GELU, nullptr, 0, nullptr, 0, s)) return 1;
        } else {
            if (gemm(dec->head_dense, w.x, H, w.t1, H, R, MIT_ACT_GELU, nullptr, 0, s)) return 1;
        }
        if (layernorm(w.t1, H, dec->head_ln_w, dec->head_ln_b, w.t2, H, R, H, eps, t2_pl, s)) return 1;
        if (out_rows) {
            if (pgemm(dec->head_out, w.t2_p, Rp, R, w.logits, Vp, MIT_ACT_NONE, nullptr, 0, nullptr, 0, s)) return 1;
        } else {
            if (gemm(dec->head_out, w.t2, H, w.logits, Vp, R, MIT_ACT_NONE, nullptr, 0, s)) return 1;
        }
        cur = launch_step(w, w.logits, Vp, V, 0, a, step, cur, s);
        steps_run = step + 1;
        if (a->trace_logits)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_logits + (int64_t)step * R * V, w.logp, (size_t)R * V * 4, hipMemcpyDeviceToDevice, s));
        if (a->trace_hist)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_hist + (int64_t)step * R * T, w.hist + (int64_t)cur * R * T, (size_t)R * T * 4,
                                         hipMemcpyDeviceToDevice, s));
        MIT_CHECK_LAUNCH("mit_mocr_decode");
        if ((step % 4 == 3) && step + 2 < T) {   // early exit without a per-step sync
            int dc = 0;
            MIT_CHECK_HIP(hipMemcpyAsync(&dc, w.done_count, 4, hipMemcpyDeviceToHost, s));
            MIT_CHECK_HIP(hipStreamSynchronize(s));
            if (dc >= N) break;
        }
    }
    finish(w, a, steps_run, s);
    MIT_CHECK_LAUNCH("mit_mocr_decode");
    return 0;
}
