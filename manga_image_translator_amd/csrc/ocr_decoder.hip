// ocr_decoder.hip — native beam-search decoder loop of the 48px OCR (OCR.infer_beam_batch_tensor,
// manga_translator/ocr/model_48px.py:691-784).
//
// The reference runs ~75 tiny torch ops per step from Python and syncs to the host several times per
// step (:741-772).  Here the whole loop is one C call: every step enqueues its kernels on the stream
// from C++ (no Python, no per-step host sync), keeps a real K/V cache per layer (the reference
// re-projects the whole history each step, :561-566 — identical values, since row r's history never
// changes: the reference re-orders hypotheses but not caches, :730-735), and does the top-k / beam
// bookkeeping on the device.  Finished samples stay in place (frozen results) instead of being
// compacted away; the host polls a device counter every few steps for the early exit.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"
#include "ocr_kernels.h"
#include "pgemm_rows.h"
#include "ocr_linear.h"

namespace {

using namespace ocrlin;

constexpr int E = 320;
constexpr int FF = 2048;

constexpr int FF2_SPLITK_MAX_ROWS = 640;   // rows (lines x beams) up to which the few-row FFN output Linear cuts K across four waves

struct Ws {
    float *tgt, *nrm, *qkv, *att, *q2, *ffh, *decoded, *p1, *logits, *vals, *logp, *cfeat;
    int *idx, *hist, *done, *done_count;
    // the few-row form (rows_path): activations that only feed a Linear live as bf16 planes [3][K / 8][Rp][8] (pgemm_rows.h)
    uint16_t *nrm_p, *att_p, *ffh_p, *dec_p, *p1_p;
    int64_t Rp;
};

int64_t carve(Ws *w, char *base, int N, int T, int D) {
    const int64_t R = (int64_t)N * 5;
    const int64_t Dp = (D + 3) / 4 * 4;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    float *tgt = (float *)take(R * E * 4);
    float *nrm = (float *)take(R * E * 4);
    float *qkv = (float *)take(5 * 3 * R * T * E * 4);
    float *att = (float *)take(R * E * 4);
    float *q2 = (float *)take(R * E * 4);
    float *ffh = (float *)take(R * FF * 4);
    float *decoded = (float *)take(R * T * E * 4);
    float *p1 = (float *)take(R * E * 4);
    float *logits = (float *)take(R * Dp * 4);
    float *vals = (float *)take(R * 5 * 4);
    float *logp = (float *)take(2 * R * 4);
    float *cfeat = (float *)take(R * T * 64 * 4);
    int *idx = (int *)take(R * 5 * 4);
    int *hist = (int *)take(2 * R * (T + 1) * 4);
    int *done = (int *)take((int64_t)N * 4);
    int *done_count = (int *)take(256);
    const int64_t Rp = (R + 31) / 32 * 32;
    uint16_t *nrm_p = (uint16_t *)take(3 * E * Rp * 2);
    uint16_t *att_p = (uint16_t *)take(3 * E * Rp * 2);
    uint16_t *ffh_p = (uint16_t *)take(3 * FF * Rp * 2);
    uint16_t *dec_p = (uint16_t *)take(3 * E * Rp * 2);
    uint16_t *p1_p = (uint16_t *)take(3 * E * Rp * 2);
    if (w) *w = Ws{tgt, nrm, qkv, att, q2, ffh, decoded, p1, logits, vals, logp, cfeat, idx, hist, done, done_count,
                   nrm_p, att_p, ffh_p, dec_p, p1_p, Rp};
    return off;
}


__global__ void fill_int_kernel(int *p, int64_t n, int v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

constexpr int FORMS_ALL = MIT_OCR48_FORM_ROWS | MIT_OCR48_FORM_LN_FUSED | MIT_OCR48_FORM_Q2_FUSED | MIT_OCR48_FORM_FF2_SPLITK | MIT_OCR48_FORM_SELF_ROWS;
}  // namespace

extern "C" int64_t mit_ocr48_decode_workspace_bytes(int N, int T, int dict_size) {
    if (N <= 0 || T <= 0 || dict_size <= 0) return 0;
    return carve(nullptr, nullptr, N, T, dict_size);
}

extern "C" int mit_ocr48_decode(const MitOcr48Decoder *dec, MitOcr48DecodeArgs *a, void *stream) {
    if (!dec || !a) return mit_set_error("mit_ocr48_decode: null argument");
    const int forms_off = a->forms_off;
    if (forms_off & ~FORMS_ALL) return mit_set_error("mit_ocr48_decode: unknown bits in forms_off");
    const int N = a->N, L = a->L, T = a->max_seq_length, D = dec->dict_size;
    if (N <= 0 || L <= 0 || T <= 0) return mit_set_error("mit_ocr48_decode: empty problem");
    if (!a->mem_k || !a->mem_v || !a->mem_len || !a->workspace || !a->res_tok || !a->res_len || !a->res_prob || !a->res_row || !a->colors)
        return mit_set_error("mit_ocr48_decode: null buffer");
    if (a->workspace_bytes < carve(nullptr, nullptr, N, T, D)) return mit_set_error("mit_ocr48_decode: workspace too small");
    if (T + 1 > dec->xpos.imax || (T + 1) / 2 + 1 >= dec->xpos.pmax) return mit_set_error("mit_ocr48_decode: XPOS tables too small for T");
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    carve(&w, (char *)a->workspace, N, T, D);
    const int R = N * 5;
    const int64_t Dp = (D + 3) / 4 * 4;
    const int64_t TE = (int64_t)T * E;
    const int hist_ld = T + 1;
    int *hist[2] = {w.hist, w.hist + (int64_t)R * hist_ld};
    float *logp[2] = {w.logp, w.logp + R};

    hipLaunchKernelGGL(fill_int_kernel, dim3(64), dim3(256), 0, s, hist[0], (int64_t)2 * R * hist_ld, a->start_tok);
    MIT_CHECK_HIP(hipMemsetAsync(w.done, 0, (size_t)N * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.done_count, 0, 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(w.decoded, 0, (size_t)R * TE * 4, s));
    MIT_CHECK_HIP(hipMemsetAsync(a->res_len, 0, (size_t)N * 4, s));
    ocrk_embed(hist[0], hist_ld, dec->embd, w.tgt, R, E, s);   // step 0: the start tokens; every later step's rows come from the beam kernel

    int cur = 0, steps = 0;
    // One beam-search step is a launch sequence on the stream (body below); its step-dependent arguments are host values.
    // rows_path: the few-row form of a step (see body).  MIT_OCR48_ROWS_MAX: largest R = 5 N it is used for; measured equal to
    // the 64 x 64 split tiles at R = 2560 (16 pages) and 2-3.5x faster per Linear at R = 160 .. 640 (profiles/r04u_pgemm_rows.log).
    // Which forms a call takes: the conditions below and a->forms_off (mit_hip.h, MIT_OCR48_FORM_*) — per call, no process-wide switch.
    const int gmode = mit_gemm_mode_get();
    bool rows_path = (gmode == 6 || gmode == 9) && R <= MIT_OCR48_ROWS_MAX && !(forms_off & MIT_OCR48_FORM_ROWS) && rows_ok(dec->pred1) && dec->pred.w_split &&
                     dec->pred.Kp == dec->pred.K && (dec->pred.K % 16) == 0 && (dec->pred.N % 4) == 0;
    for (int l = 0; l < 5 && rows_path; ++l) {
        const MitOcrDecoderLayer &ly = dec->layers[l];
        rows_path = rows_ok(ly.qkv) && rows_ok(ly.out) && rows_ok(ly.q2) && rows_ok(ly.out2) && rows_ok(ly.ff1) && rows_ok(ly.ff2);
    }
    // LayerNorm inside the Linear that consumes it (else the two-launch form)
    const bool ln_fused = rows_path && !(forms_off & MIT_OCR48_FORM_LN_FUSED);
    // The FFN's second Linear (K = 2048) with K cut across four waves: for FEW rows only (a page or two, where its 10 us accumulator chain
    // is a sixth of the step) — its sums round differently from the k-sequential chain every other form uses, so a page decoded alone
    // differs from the same page inside a large group in the last bits of the log-probabilities (tests: tokens equal, 1e-5 on the
    // probabilities).  Without it: the one-chain kernel (bit for bit the tiled form).
    const int ff2_splitk = (rows_path && R <= FF2_SPLITK_MAX_ROWS && !(forms_off & MIT_OCR48_FORM_FF2_SPLITK)) ? 1 : 0;
    // norm2 + q projection inside the cross-attention kernel (else separate launches; bit-identical either way; gemm mode 6 only)
    const bool q2_fused = ln_fused && gmode == 6 && !(forms_off & MIT_OCR48_FORM_Q2_FUSED);
    const bool per_head_self = forms_off & MIT_OCR48_FORM_SELF_ROWS;
    int forms_run = (rows_path ? MIT_OCR48_FORM_ROWS : 0) | (ln_fused ? MIT_OCR48_FORM_LN_FUSED : 0) | (ff2_splitk ? MIT_OCR48_FORM_FF2_SPLITK : 0);
    auto body = [&](const int step, hipStream_t st) -> int {
        const int64_t so = (int64_t)step * E;  // the step's column block of the q / k / v and activation caches
        // (w.tgt holds the embedded tokens of this step: the start tokens before the loop, then written by the previous step's beam kernel)
        const int Tk = step + 1;  // the self-attention's key history 0 .. step
        if (rows_path) {
            // few rows (one page .. a group of pages): every Linear on the one-wave-per-block planar GEMM (pgemm_rows.h) — the LayerNorms,
            // the attention kernels and the ReLU / GELU epilogues hand over bf16 planes, the residual stream and the K / V caches stay
            // fp32.  Same kernels' arithmetic, same plane split, same MFMA order as the tiles of the other form: identical results.
            const int64_t Rp = w.Rp;
            const OcrPlanes nrm_pl{w.nrm_p, Rp, E / 8}, att_pl{w.att_p, Rp, E / 8};
            for (int l = 0; l < 5; ++l) {
                const MitOcrDecoderLayer &ly = dec->layers[l];
                float *qc = w.qkv + (int64_t)(l * 3 + 0) * R * TE;
                float *kc = w.qkv + (int64_t)(l * 3 + 1) * R * TE;
                float *vc = w.qkv + (int64_t)(l * 3 + 2) * R * TE;
                if (ln_fused) {
                    if (pgemm_ln(ly.qkv, w.tgt, E, ly.ln1_w, ly.ln1_b, R, qc + so, TE, MIT_ACT_NONE, nullptr, 0, st, E, (int64_t)R * TE)) return 1;
                } else {
                    if (ocrk_layernorm(w.tgt, E, ly.ln1_w, ly.ln1_b, nullptr, 0, R, E, 1e-5f, st, &nrm_pl)) return 1;
                    if (pgemm(ly.qkv, w.nrm_p, Rp, R, qc + so, TE, MIT_ACT_NONE, nullptr, 0, nullptr, 0, st, E, (int64_t)R * TE)) return 1;
                }
                OcrAttXpos xs{dec->xpos.cos_t, dec->xpos.sin_t, dec->xpos.scale_t, dec->xpos.iscale_t, dec->xpos.pmax, step, 1};
                if (ocrk_attention(qc + so, TE, E, kc, TE, E, vc, TE, E, nullptr, 0, 0, nullptr, R, 1, Tk, 1, st, 4, 80, &xs, &att_pl, per_head_self) == OcrAttKernel::SelfRows)
                    forms_run |= MIT_OCR48_FORM_SELF_ROWS;
                if (pgemm(ly.out, w.att_p, Rp, R, w.tgt, E, MIT_ACT_NONE, w.tgt, E, nullptr, 0, st)) return 1;
                const float *mk = a->mem_k + (int64_t)l * N * L * E;
                const float *mv = a->mem_v + (int64_t)l * N * L * E;
                OcrAttXpos xc{dec->xpos.cos_t, dec->xpos.sin_t, dec->xpos.scale_t, dec->xpos.iscale_t, dec->xpos.pmax, step, 0};
                // norm2 + the q projection inside the cross-attention kernel where that form exists (a page or a few; else two launches)
                bool q_inside = false;
                if (q2_fused && ly.q2.bias && ly.q2.N == E) {
                    const OcrAttQProj qp{w.tgt, E, ly.ln2_w, ly.ln2_b, 1e-5f, ly.q2.w_split, ly.q2.ldw, ly.q2.scale, ly.q2.bias};
                    q_inside = ocrk_cross_attention_qproj(qp, mk, (int64_t)L * E, E, mv, (int64_t)L * E, E, a->mem_len, R, L, st, &xc, &att_pl);
                    if (q_inside) forms_run |= MIT_OCR48_FORM_Q2_FUSED;
                }
                if (!q_inside) {
                    if (ln_fused) {
                        if (pgemm_ln(ly.q2, w.tgt, E, ly.ln2_w, ly.ln2_b, R, w.q2, E, MIT_ACT_NONE, nullptr, 0, st)) return 1;
                    } else {
                        if (ocrk_layernorm(w.tgt, E, ly.ln2_w, ly.ln2_b, nullptr, 0, R, E, 1e-5f, st, &nrm_pl)) return 1;
                        if (pgemm(ly.q2, w.nrm_p, Rp, R, w.q2, E, MIT_ACT_NONE, nullptr, 0, nullptr, 0, st)) return 1;
                    }
                    ocrk_attention(w.q2, E, E, mk, (int64_t)L * E, E, mv, (int64_t)L * E, E, nullptr, 0, 0, a->mem_len, R, 1, L, 5, st, 4, 80, &xc, &att_pl);
                }
                if (pgemm(ly.out2, w.att_p, Rp, R, w.tgt, E, MIT_ACT_NONE, w.tgt, E, nullptr, 0, st)) return 1;
                if (ln_fused) {
                    if (pgemm_ln(ly.ff1, w.tgt, E, ly.ln3_w, ly.ln3_b, R, nullptr, 0, MIT_ACT_RELU, w.ffh_p, Rp, st)) return 1;
                } else {
                    if (ocrk_layernorm(w.tgt, E, ly.ln3_w, ly.ln3_b, nullptr, 0, R, E, 1e-5f, st, &nrm_pl)) return 1;
                    if (pgemm(ly.ff1, w.nrm_p, Rp, R, nullptr, 0, MIT_ACT_RELU, nullptr, 0, w.ffh_p, Rp, st)) return 1;
                }
                if (l < 4) {
                    if (pgemm(ly.ff2, w.ffh_p, Rp, R, w.tgt, E, MIT_ACT_NONE, w.tgt, E, nullptr, 0, st, 0, 0, ff2_splitk)) return 1;
                } else {  // last layer: the step's output into the activation cache (:570), and as planes for the prediction head
                    if (pgemm(ly.ff2, w.ffh_p, Rp, R, w.decoded + so, TE, MIT_ACT_NONE, w.tgt, E, w.dec_p, Rp, st, 0, 0, ff2_splitk)) return 1;
                }
            }
            if (pgemm(dec->pred1, w.dec_p, Rp, R, nullptr, 0, MIT_ACT_GELU, nullptr, 0, w.p1_p, Rp, st)) return 1;
            if (pgemm(dec->pred, w.p1_p, Rp, R, w.logits, Dp, MIT_ACT_NONE, nullptr, 0, nullptr, 0, st)) return 1;
        } else {
            for (int l = 0; l < 5; ++l) {
                const MitOcrDecoderLayer &ly = dec->layers[l];
                float *qc = w.qkv + (int64_t)(l * 3 + 0) * R * TE;
                float *kc = w.qkv + (int64_t)(l * 3 + 1) * R * TE;
                float *vc = w.qkv + (int64_t)(l * 3 + 2) * R * TE;
                // self attention (:565)
                if (ocrk_layernorm(w.tgt, E, ly.ln1_w, ly.ln1_b, w.nrm, E, R, E, 1e-5f, st)) return 1;
                if (gemm(ly.qkv, w.nrm, E, qc + so, TE, R, MIT_ACT_NONE, nullptr, 0, st, E, (int64_t)R * TE)) return 1;
                // (the XPOS rotation of the step's query and of the key history 0 .. step happens inside the attention kernel)
                OcrAttXpos xs{dec->xpos.cos_t, dec->xpos.sin_t, dec->xpos.scale_t, dec->xpos.iscale_t, dec->xpos.pmax, step, 1};
                if (ocrk_attention(qc + so, TE, E, kc, TE, E, vc, TE, E, w.att, E, E, nullptr, R, 1, Tk, 1, st, 4, 80, &xs, nullptr, per_head_self) == OcrAttKernel::SelfRows)
                    forms_run |= MIT_OCR48_FORM_SELF_ROWS;
                if (gemm(ly.out, w.att, E, w.tgt, E, R, MIT_ACT_NONE, w.tgt, E, st)) return 1;
                // cross attention (:567)
                if (ocrk_layernorm(w.tgt, E, ly.ln2_w, ly.ln2_b, w.nrm, E, R, E, 1e-5f, st)) return 1;
                if (gemm(ly.q2, w.nrm, E, w.q2, E, R, MIT_ACT_NONE, nullptr, 0, st)) return 1;
                const float *mk = a->mem_k + (int64_t)l * N * L * E;
                const float *mv = a->mem_v + (int64_t)l * N * L * E;
                OcrAttXpos xc{dec->xpos.cos_t, dec->xpos.sin_t, dec->xpos.scale_t, dec->xpos.iscale_t, dec->xpos.pmax, step, 0};
                ocrk_attention(w.q2, E, E, mk, (int64_t)L * E, E, mv, (int64_t)L * E, E, w.att, E, E, a->mem_len, R, 1, L, 5, st, 4, 80, &xc);
                if (gemm(ly.out2, w.att, E, w.tgt, E, R, MIT_ACT_NONE, w.tgt, E, st)) return 1;
                // feed forward (:568)
                if (ocrk_layernorm(w.tgt, E, ly.ln3_w, ly.ln3_b, w.nrm, E, R, E, 1e-5f, st)) return 1;
                if (gemm(ly.ff1, w.nrm, E, w.ffh, FF, R, MIT_ACT_RELU, nullptr, 0, st)) return 1;
                if (l < 4) {
                    if (gemm(ly.ff2, w.ffh, FF, w.tgt, E, R, MIT_ACT_NONE, w.tgt, E, st)) return 1;
                } else {  // last layer writes the step's output straight into the activation cache (:570)
                    if (gemm(ly.ff2, w.ffh, FF, w.decoded + so, TE, R, MIT_ACT_NONE, w.tgt, E, st)) return 1;
                }
            }
            if (gemm(dec->pred1, w.decoded + so, TE, w.p1, E, R, MIT_ACT_GELU, nullptr, 0, st)) return 1;
            if (gemm(dec->pred, w.p1, E, w.logits, Dp, R, MIT_ACT_NONE, nullptr, 0, st)) return 1;
        }
        if (a->trace_logits)
            MIT_CHECK_HIP(hipMemcpy2DAsync(a->trace_logits + (int64_t)step * R * D, (size_t)D * 4, w.logits, (size_t)Dp * 4,
                                           (size_t)D * 4, R, hipMemcpyDeviceToDevice, st));
        ocrk_logsoftmax_top5(w.logits, Dp, R, D, a->suppress_eos ? a->end_tok : -1, w.vals, w.idx, nullptr, st);
        if (step == 0) {
            ocrk_beam_init(w.vals, w.idx, hist[cur], hist_ld, logp[cur], N, a->start_tok, st, dec->embd, w.tgt, E);
        } else {
            ocrk_beam_step(w.vals, w.idx, hist[cur], hist[cur ^ 1], hist_ld, logp[cur], logp[cur ^ 1], w.done, a->res_row,
                           a->res_len, a->res_prob, a->res_tok, w.done_count, N, step, a->end_tok, a->max_finished, st, dec->embd, w.tgt, E);
            cur ^= 1;
        }
        if (a->trace_hist)
            MIT_CHECK_HIP(hipMemcpyAsync(a->trace_hist + (int64_t)step * R * hist_ld, hist[cur], (size_t)R * hist_ld * 4,
                                         hipMemcpyDeviceToDevice, st));
        MIT_CHECK_LAUNCH("mit_ocr48_decode");
        return 0;
    };

    for (int step = 0; step < T; ++step) {
        if (body(step, s)) return 1;
        steps = step + 1;
        if (!a->suppress_eos && step >= 1 && (step % 4 == 3) && step + 1 < T) {  // early exit (:765-766) without a per-step sync;
            // with EOS suppressed no hypothesis can finish, so the loop stays fully asynchronous
            int dc = 0;
            MIT_CHECK_HIP(hipMemcpyAsync(&dc, w.done_count, 4, hipMemcpyDeviceToHost, s));
            MIT_CHECK_HIP(hipStreamSynchronize(s));
            if (dc >= N) break;
        }
    }
    ocrk_beam_finalize(hist[cur], hist_ld, logp[cur], w.done, a->res_row, a->res_len, a->res_prob, a->res_tok, N, steps + 1, s);
    // colour heads over every beam row's activation cache (:789-799); the caller gathers rows res_row[n]
    if (gemm(dec->color1, w.decoded, E, w.cfeat, 64, R * T, MIT_ACT_RELU, nullptr, 0, s)) return 1;
    if (gemm(dec->color_heads, w.cfeat, 64, a->colors, 12, R * T, MIT_ACT_NONE, nullptr, 0, s)) return 1;
    MIT_CHECK_LAUNCH("mit_ocr48_decode");
    a->steps_run = steps;
    a->forms_run = forms_run;
    return 0;
}
