// ocr_linear.h — the Linear launches of the native OCR decoder loops (ocr_decoder.hip, ocr32_decoder.hip): host-side helpers that fill
// a GEMM descriptor from a MitLinear and launch it on the tiled GEMM (mit_conv_gemm) or on the few-row planar GEMM (pgemm_rows.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/mit_hip.h"
#include "pgemm_rows.h"

namespace ocrlin {

inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// C[M x N] = act((A[M x K] @ W) * scale + bias) + post, rows of A / C / post strided.
inline int gemm(const MitLinear &lin, const float *A, int64_t lda, float *Cp, int64_t ldc, int M, int act, const float *post,
                int64_t ldpost, hipStream_t s, int nsplit = 0, int64_t nhi = 0) {
    MitConvGemm d;
    memset(&d, 0, sizeof(d));
    d.a = A;
    d.a_xs = lda;
    d.NB = 1; d.Hi = 1; d.Wi = M; d.Ho = 1; d.Wo = M; d.sy = 1; d.sx = 1;
    d.ntaps = 1; d.pad_mode = MIT_PAD_ZERO;
    d.w = lin.w; d.ldw = lin.ldw; d.Nw = lin.Np;
    d.N = lin.N;
    d.Cin = lin.K; d.Kw = lin.Kp;
    d.Z = 1; d.zdiv = 1;
    d.w_split = lin.w_split;  // planes attached by the packer in a split GEMM mode (NULL otherwise); the launcher decides by the mode of the moment
    d.c.base = Cp; d.c.xs = ldc; d.c.nsplit = nsplit; d.c.nhi = nhi;
    if (post) {
        d.post.base = const_cast<float *>(post);
        d.post.xs = ldpost;
    }
    d.scale = lin.scale; d.bias = lin.bias; d.act = act;
    return mit_conv_gemm(&d, s);
}

// The same Linear on planar activations (pgemm_rows.h), one wave per 32 x 32 output block: C fp32 (optional, with the column split
// of gemm()) and / or planes.  splitk: the K = 2048 Linear with K cut across four waves.
inline int pgemm(const MitLinear &lin, const uint16_t *a_planes, int64_t lda, int M, float *Cp, int64_t ldc, int act, const float *post,
                 int64_t ldpost, uint16_t *c_planes, int64_t ld_cp, hipStream_t s, int nsplit = 0, int64_t nhi = 0, int splitk = 0) {
    MitPGemm d;
    memset(&d, 0, sizeof(d));
    d.a_planes = a_planes; d.lda = lda;
    d.w_planes = lin.w_split; d.ldw = lin.ldw;
    d.M = M; d.N = lin.N; d.K = lin.K; d.Z = 1;
    d.c = Cp; d.ldc = ldc;
    d.post = post; d.ld_post = ldpost;
    d.scale = lin.scale; d.bias = lin.bias; d.act = act;
    d.nprod = 0;  // the GEMM mode of the moment
    PgRowsExt x;
    memset(&x, 0, sizeof(x));
    x.nsplit = nsplit; x.nhi = nhi; x.splitk = splitk;
    if (Cp) x.also_planes = c_planes, x.also_ld = ld_cp;
    else d.c_planes = c_planes, d.ld_cp = ld_cp;
    return mit_pgemm_rows(d, x, s);
}

// The same with A = LayerNorm(x) computed by the GEMM's own waves (pgemm_rows_ln.hip; K == 320): bit for bit ocrk_layernorm + pgemm.
inline int pgemm_ln(const MitLinear &lin, const float *xin, int64_t ldx, const float *ln_w, const float *ln_b, int M, float *Cp, int64_t ldc, int act,
                    uint16_t *c_planes, int64_t ld_cp, hipStream_t s, int nsplit = 0, int64_t nhi = 0) {
    MitPGemm d;
    memset(&d, 0, sizeof(d));
    d.w_planes = lin.w_split; d.ldw = lin.ldw;
    d.M = M; d.N = lin.N; d.K = lin.K; d.Z = 1;
    d.c = Cp; d.ldc = ldc;
    d.scale = lin.scale; d.bias = lin.bias; d.act = act;
    d.nprod = 0;
    PgRowsExt x;
    memset(&x, 0, sizeof(x));
    x.nsplit = nsplit; x.nhi = nhi;
    if (Cp) x.also_planes = c_planes, x.also_ld = ld_cp;
    else d.c_planes = c_planes, d.ld_cp = ld_cp;
    const PgRowsLn ln{xin, ldx, ln_w, ln_b, 1e-5f};
    return mit_pgemm_rows_ln(d, x, ln, s);
}

inline bool rows_ok(const MitLinear &l) { return l.w_split && l.Kp == l.K && (l.K % 16) == 0 && (l.N % 8) == 0; }

}  // namespace ocrlin
