/*
 * mit_hip.h — C-ABI of the MI355X (gfx950) dense-stage engine for manga-image-translator.
 *
 * This is the drop-in boundary beneath the reference's Python plugin classes
 * (SURVEY.md §8b).  Nothing native exists in the reference for this path: every FLOP goes
 * through stock ATen ops called from `async _infer()` bodies.  Each entry point below names
 * the reference call site whose device work it replaces; the Python shim that binds it
 * (ctypes) is `manga_image_translator_amd/lib.py`, and INTEGRATION.md shows the stub a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch / HIP types in signatures.  `stream` is a
 *     hipStream_t passed as void* (0 = default stream).
 *   - every pointer named *_dev is a DEVICE pointer (e.g. torch.Tensor.data_ptr()).
 *   - all functions return 0 on success, non-zero on error; `mit_last_error()` returns a
 *     thread-local, NUL-terminated description (the Python shim raises RuntimeError with it;
 *     reference errors are Python exceptions: manga_translator.py:469-477,496-502,583-590).
 *   - all kernels are asynchronous on `stream`; nothing synchronises unless documented.
 *   - activations are fp32 NHWC ("pixel-major, channel-contiguous").
 */
#ifndef MIT_HIP_H
#define MIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIT_ABI_VERSION 26
#define MIT_MAX_TAPS 64

/* activation codes for fused epilogues */
enum MitAct {
    MIT_ACT_NONE = 0,
    MIT_ACT_RELU = 1,    /* nn.ReLU            (inpainting_lama_mpe.py:372-399, basemodel.py:20-22) */
    MIT_ACT_LEAKY = 2,   /* nn.LeakyReLU(alpha) (yolov5/common.py:39-40: 0.1; esrgan: 0.2)          */
    MIT_ACT_SILU = 3,    /* nn.SiLU             (yolov5/common.py:37)                                */
    MIT_ACT_SIGMOID = 4, /* nn.Sigmoid          (basemodel.py:52,107,136; lama generator :599-600)   */
    MIT_ACT_GELU = 5     /* nn.GELU (erf)       (model_48px.py:199,534)                              */
};
/* OR-ed into MitConvGemm.act: the ``post`` operand is added BEFORE the activation, act(v*scale + bias + post) — the
 * ``out += identity; relu(out)`` of torchvision's BasicBlock (default detector backbone, default_utils/DBNet_resnet34.py:76). */
#define MIT_ACT_POST_FIRST 0x100

enum MitPad {
    MIT_PAD_ZERO = 0,    /* nn.Conv2d default                                   */
    MIT_PAD_REFLECT = 1  /* padding_mode='reflect' / nn.ReflectionPad2d (inpainting_lama_mpe.py:334-340,554,597) */
};

/* Addressing of a logical [z][nb][oy][ox][n] fp32 tensor, element strides.
 * z = z1 * zdiv + z0.  Column n maps to (n / nsplit) * nhi + (n % nsplit); nsplit == 0
 * means plain contiguous columns.  base == NULL disables the operand. */
typedef struct MitTensorMap {
    float *base;
    int64_t zs1, zs0, bs, ys, xs;
    int64_t nhi;
    int32_t nsplit;
    int32_t _pad;
} MitTensorMap;

/* mit_conv_gemm — the one dense contraction kernel of the engine (implicit-GEMM on
 * v_mfma_f32_32x32x2_f32, exact fp32, k-ordered fmaf chain).
 *
 *   C[z][m][n] = epilogue( sum_{t<ntaps} sum_{ci<Cin} A[z][m, t, ci] * W[z][t*Cin+ci][n] )
 *
 *   m = (nb, oy, ox), nb < NB, oy < Ho, ox < Wo
 *   A[z][m,t,ci] = a[z1*a_zs1 + z0*a_zs0 + nb*a_bs + iy*a_ys + ix*a_xs + tap_off[t] + ci]
 *        iy = oy*sy + tap_dy[t], ix = ox*sx + tap_dx[t]; outside [0,Hi)x[0,Wi): zero or reflect
 *   W[z][k][n]   = w[z1*w_zs1 + z0*w_zs0 + k*ldw + n]          (rows k >= Kw, cols n >= Nw read as 0)
 *   epilogue(v)  = act( (v + pre[..]) * scale[n] + bias[n] ) + post[..]      (MIT_ACT_POST_FIRST: post joins inside act)
 *
 * Replaces (with BatchNorm folded into scale/bias by the packer):
 *   nn.Conv2d / nn.ConvTranspose2d (as stride-parity sub-convolutions) / nn.Linear calls in
 *   inpainting_lama_mpe.py:349-369,286-307,603-613; ctd_utils/basemodel.py:56-72,100-119;
 *   ctd_utils/yolov5/common.py:30-49,94-135; ocr/model_48px.py:203-276,327-394,548-572;
 *   and torch.fft.rfftn / irfftn of FourierUnit (inpainting_lama_mpe.py:228,252) expressed as
 *   dense DFT matrices (W operand = activations, A operand = the DFT matrix).
 *
 * Requirements: Cin % 4 == 0, ldw % 4 == 0, Nw % 4 == 0, all bases 16-byte aligned,
 *   a_xs/a_ys/a_bs/tap_off multiples of 4 (float4 loads).
 */
typedef struct MitConvGemm {
    /* A operand */
    const float *a;
    int64_t a_zs1, a_zs0, a_bs, a_ys, a_xs;
    int32_t NB, Hi, Wi, Cin;
    int32_t Ho, Wo, sy, sx;
    int32_t ntaps, pad_mode;
    int8_t tap_dy[MIT_MAX_TAPS];
    int8_t tap_dx[MIT_MAX_TAPS];
    int32_t tap_off[MIT_MAX_TAPS];
    /* W operand */
    const float *w;
    int64_t w_zs1, w_zs0, ldw;
    int32_t Kw, Nw;
    /* problem */
    int32_t N;      /* output columns actually stored */
    int32_t Z, zdiv;
    /* epilogue */
    MitTensorMap c, pre, post;
    const float *scale, *bias;
    int32_t act;
    float act_alpha;
    /* optional: W pre-split into three bf16 planes (mit_gemm_split_pack) for the split-bf16 tiles; NULL = fp32 MFMA only.
     * ws_zs0 = uint16 elements between z0 slices (the z1 stride must be 0 when this is set). */
    const uint16_t *w_split;
    int64_t ws_zs0;
    /* optional: a two-table row lookup joined AFTER the activation and the post residual — y += lut1[r1][n]; y += lut2[r2][n], in that
     * order — where output row m (= its pixel index, batch-major) carries lut_rows[m] = r1 | r2 << 16 and both tables have lut_ld floats
     * per row.  LaMa's masked position encoding rides on it: the 7x7 stem writes relu(bn(conv)) + alpha5 * emb[rel] + alpha6 * dir in
     * one pass instead of a separate read-modify-write of the 64-channel stem output (inpainting_lama_mpe.py:609-613).  NULL = off.
     * Implemented as its own instantiation of the float4 epilogue of the fast / split tiles (every other launch compiles to the code it
     * had without it): needs Cin % 16 == 0 and <= 16 taps, N % 4 == 0, lut_ld % 4 == 0, 16-byte aligned maps and tables, Z == 1, no
     * post residual, act none or relu — anything else is refused with an error. */
    const int32_t *lut_rows;
    const float *lut1, *lut2;
    int64_t lut_ld;
    /* precision of THIS launch.  0: follow the GEMM mode (mit_gemm_mode_set) — fp32 results on the split-bf16 or fp32 MFMA tiles.
     * 1: the one-product tiles ("p1"): both operands rounded to bf16 (round to nearest even, the rounding of tensor.to(torch.bfloat16))
     * while they are staged, ONE bf16 MFMA product per 16-wide k-step, fp32 accumulation (k ascending) and the fp32 epilogue — what
     * a convolution computes under torch.autocast(dtype=torch.bfloat16), the reference's GPU path of LaMa
     * (inpainting_lama_mpe.py:106), WITHOUT the rounding of the layer output to bf16.  W is plane 0 of w_split.  Taken whatever the
     * GEMM mode is and whatever the launch size (mit_gemm_split_min_tiles is ignored), identical bits on every p1 tile.  A launch
     * that carries no w_split or misses the split tiles' preconditions (Cin % 16 == 0, <= 16 taps, 32-bit offsets) is refused: the
     * caller asked for a precision, there is no silent fp32 fallback.  Any other value is refused.  (An explicit p1 tile index through
     * mit_conv_gemm_cfg runs with nprod = 0 as well, like the test-only 3-pair tile: the tile decides; nprod = 1 with a tile that
     * is not a p1 tile is refused.) */
    int32_t nprod;
    /* optional: compute only a device-side list of live 8 x 8 blocks of the (nb, oy, ox) output grid (LaMa's decoder tail, whose result
     * is read only under the mask).  An image has ceil(Ho / 8) * ceil(Wo / 8) blocks in raster order (edge blocks are clipped); block
     * b of image i has the id i * blocks_per_image + b.  live_blocks holds the ids of the live blocks of the whole batch, ascending;
     * live_start[i] is the index in live_blocks of image i's first entry and live_start[NB] the total (NB + 1 entries, live_start[0]
     * need not be 0).  Row r of the launch is then position r & 63 (row-major in the block) of block live_blocks[live_start[0] + (r >> 6)];
     * rows past 64 * (live_start[NB] - live_start[0]) and positions of an edge block outside Ho x Wo are dead rows: gathered as zeros
     * and never stored, like the rows m >= M of a dense launch.  The host launches the dense grid and reads nothing back: a workgroup
     * loads the count and returns when its tile lies past the live tiles (the XCD-contiguous tile order is formed over the live tiles).
     * A batch that is cut into runs of whole images moves live_start and live_img0 (the batch index of the run's first image) along
     * with the operands, so every run finds its own segment.  Live rows get the bits of the dense launch.  NULL = the dense launch,
     * unchanged.  Implemented by the fast (fp32 MFMA) and split tiles for Z == 1 without lut_rows; any other tile refuses it. */
    int32_t live_img0;
    const int32_t *live_blocks;
    const int32_t *live_start;
    /* optional: the ``pre`` operand taken from the 36 Winograd F(4x4, 3x3) products of a 3x3 convolution over the same output grid,
     * wino_m [36][T][wino_n] (T = NB * wino_th * wino_tw tiles of 4 x 4 outputs, image-major raster; what the Z = 36 launch of
     * WinogradConv3x3 writes), wino_zs floats between two of the 36 slices:
     *     epilogue(v) = act( (v + (A^T m A)[oy & 3][ox & 3]) * scale[n] + bias[n] ) + post[..]
     * with m the 6 x 6 products of tile (oy >> 2, ox >> 2) and column n — the value mit_wino43_output (no scale, bias or activation)
     * would have stored at (nb, oy, ox, n), computed by the same expression sequence, so the result has the bits of that launch
     * followed by this one with its output as ``pre``; the staging tensor and its launch disappear.  Needs the 8 x 8 block row order
     * (live_blocks / live_start: list every block for a dense layer), under which the 16 rows a lane holds of one accumulator block are
     * one whole tile; one tap with sy == sx == 1, pre.base == NULL, no column-split map, N % 4 == 0, wino_n == N,
     * wino_th == ceil(Ho / 4), wino_tw == ceil(Wo / 4), wino_zs >= T * wino_n — anything else is refused.  A batch cut into runs moves
     * wino_m along with the operands.  NULL = off.  Replaces nothing of the reference by itself (convl2g(x_l) joins conv2's output in
     * FFC.forward, inpainting_lama_mpe.py:365-368). */
    const float *wino_m;
    int64_t wino_zs;
    int32_t wino_n, wino_th, wino_tw;
    int32_t _pad_wino;
} MitConvGemm;

const char *mit_last_error(void);
int mit_abi_version(void);
/* sha256 over the sources (every .hip / .h under csrc, this header) and compiler flags the library was built from; the Python
 * binding refuses (or rebuilds) a library whose digest differs from the tree's, so stale kernels are never measured. */
const char *mit_source_digest(void);

/* device / runtime ------------------------------------------------------------------- */
int mit_device_count(int *count);
int mit_device_name(int device, char *buf, int buflen);

/* dense contraction -------------------------------------------------------------------- */
int mit_conv_gemm(const MitConvGemm *desc, void *stream);
/* tile configuration override for tuning/tests: cfg = -1 auto, else index into the table
 * reported by mit_conv_gemm_config_name(). */
int mit_conv_gemm_cfg(const MitConvGemm *desc, int cfg, void *stream);
const char *mit_conv_gemm_config_name(int cfg);
/* What mit_conv_gemm_cfg(desc, cfg, stream) would do, without doing it: the same validation (same return value and mit_last_error()
 * text for a refused descriptor), then *tile = the tile of the first launch and *nb_run = its images — desc->NB unless the batch is
 * cut into runs (activations past 2^31 elements, or past the 2^31 bytes the buffer-load tiles address); a shorter last run is planned
 * by itself when it is launched.  Makes no HIP call and dereferences no operand pointer: it works without a GPU, which is how
 * tests/test_conv_gemm_plan.py pins the automatic tile choice. */
int mit_conv_gemm_plan(const MitConvGemm *desc, int cfg, int32_t *tile, int32_t *nb_run);
/* Grouped launch: n convolutions that share everything but the image — weights, taps, strides, padding, N, K, epilogue vectors and
 * activation come from ``base``; the operand and result base pointers, NB, Hi, Wi, Ho, Wo and the image / row strides come from the
 * member records (base's own a, c.base, c.bs, c.ys, a_bs, a_ys, NB, Hi, Wi, Ho, Wo are ignored; a_xs and c.xs are shared).  The 48px OCR
 * runs the chunks of a page group through it: their padded widths differ, everything else is one layer (Ocr48Engine.encode_group).
 *
 * One launch whose grid is the concatenation of the members' grids: a workgroup finds its member from the prefix of tile counts
 * (scalar code) and runs the tile body of the single launch with that member's sizes and pointers, so every member's result has the
 * bits of mit_conv_gemm on that member alone.  The tile is the one mit_conv_gemm would choose for ONE launch with the group's total
 * rows (all tiles of a family give the same bits).  The records travel by value in the kernel arguments: no allocation, no
 * synchronisation, no device table; more than MIT_CONV_GROUP_MAX members run as several grouped launches of up to that many.
 *
 * Falls back to member-by-member mit_conv_gemm launches, inside the same call, when the group cannot run as one grid: the chosen tile
 * has no grouped form (they exist for the generic 128x128 / 128x64 tiles, the fp32 MFMA 128x128 / 128x64 / 64x64 tiles and the p6
 * buffer-load tiles 128x64, 128x96, 128x160, 64x64x16, 64x64x32), a member is not eligible for it, or the base carries a live-block
 * list, wino_m, lut_rows, Z > 1, or a member's batch would be cut into runs.  base.pre / base.post must be NULL (refused otherwise:
 * a residual is per member and the records carry none).  With mit_prof_enable a grouped launch is ONE launch under its tile's index
 * with the members' summed FLOPs. */
#define MIT_CONV_GROUP_MAX 32
typedef struct MitConvGemmMember {
    const float *a;        /* A operand of this member */
    float *c;              /* its result */
    int64_t a_bs, a_ys;    /* image / row strides of A */
    int64_t c_bs, c_ys;    /* image / row strides of the result */
    int32_t NB, Hi, Wi, Ho, Wo, _pad;
} MitConvGemmMember;
int mit_conv_gemm_group(const MitConvGemm *base, const MitConvGemmMember *members, int n, void *stream);
/* What mit_conv_gemm_group would do, without doing it (no HIP call, no operand dereferenced: works without a GPU).  *tile = the tile
 * chosen for the group's total rows; per member i: launch[i] = the index of the grouped launch it rides in (0, 1, ... — a new one
 * every MIT_CONV_GROUP_MAX members) or -1 when the group falls back to member-by-member launches, first_tile[i] = its first workgroup
 * in that launch's grid (0 on the fallback), ntiles[i] = its workgroups on *tile.  Any output may be NULL. */
int mit_conv_gemm_group_plan(const MitConvGemm *base, const MitConvGemmMember *members, int n, int32_t *tile, int32_t *launch,
                             int32_t *first_tile, int32_t *ntiles);
/* the kernel's template-id as rocprofv3 prints it (without namespace), e.g. "conv_gemm_fast_kernel<128, 128, 16, 1, 4, 4, 4>":
 * lets bench.py join its per-tile probe numbers with the profiler's kernel-trace / PMC rows; NULL past the table. */
const char *mit_conv_gemm_config_kernel(int cfg);

/* Split-bf16 form of the same contraction (the GEMM mode: mit_gemm_mode_set / MIT_GEMM_SPLIT, or an explicit "split*" tile through
 * mit_conv_gemm_cfg).  gfx950's bf16 MFMA runs at 16x the rate of the fp32 one; an fp32 number is EXACTLY the sum of three bf16
 * numbers (x = hi + mid + lo, each the round-to-nearest bf16 of what the previous ones left), so
 *     a * b = sum over plane pairs (p, q) of a_p * b_q        every such product is exact in fp32 (8 x 8 significant bits)
 * and the contraction becomes 9 bf16 MFMA products accumulated in fp32 ("p9": the error is that of the fp32 accumulation alone, as
 * for the fp32 MFMA chain), or 6 when the three pairs with p + q >= 3 (relative weight <= 2^-24 of the product) are dropped ("p6").
 * Activations are split in the kernel while they are staged to LDS; the constant W operand is split once:
 *   mit_gemm_split_pack: w [nz][Kw][ldw] fp32 (slices w_zs floats apart; Kw % 8 == 0, ldw % 4 == 0)
 *                        -> out [nz][3 planes][Kw / 8][ldw][8] bf16 (16-byte cells of 8 consecutive k of one column),
 *                        nz * 3 * Kw * ldw uint16 elements; pass it as MitConvGemm.w_split with ws_zs0 = 3 * Kw * ldw.
 * Nothing in the reference corresponds to it (the reference computes these layers with fp32 torch kernels). */
int mit_gemm_split_pack(const float *w_dev, int64_t w_zs, int nz, int Kw, int64_t ldw, uint16_t *out_dev, void *stream);
/* The GEMM mode of mit_conv_gemm's automatic tile choice, process-wide, switchable at run time (launches already queued keep the tile
 * they were given):
 *   6 (default)  layers that carry w_split and fill the chip run on the split-bf16 tiles with 6 of the 9 plane products ("p6": the
 *                dropped terms are <= 2^-25 |a b| each, below one fp32 multiply rounding);
 *   9            the same with all 9 plane products (no term dropped: fp32 accumulation order is the only difference to the fp32 MFMA);
 *   0            fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere, w_split ignored.
 * The initial value is MIT_GEMM_SPLIT from the environment (0 | 6 | 9) when set, else 6.  mit_gemm_mode_set returns non-zero for any
 * other value.  Nothing in the reference corresponds to it. */
int mit_gemm_mode_set(int mode);
int mit_gemm_mode_get(void);
/* Smallest launch, counted in 128 x 64 output tiles (x Z), that the automatic choice hands to the split tiles (default 0 — every
 * eligible launch, which keeps a page's result independent of the batch it is part of); n >= 0 sets it, n < 0 only queries.  Returns
 * the previous value.  A tuning knob: 1280 = one full wave of workgroups. */
int64_t mit_gemm_split_min_tiles(int64_t n);

/* ---- planar operands: the plain GEMMs of the split-bf16 mode with activations that ARRIVE split ---------------------------------
 * In mit_conv_gemm's split tiles the activations are split into their three bf16 planes by VALU work inside the K loop, once per
 * output-column tile.  When the producer of an activation tensor writes the planes itself (mit_split_planes, or mit_pgemm's own
 * planar epilogue) a plain GEMM (1x1 convolution, nn.Linear, the 36
 * Winograd products) needs no VALU work in its K loop at all: both operands go global -> LDS by the LDS-DMA (global_load_lds_dwordx4)
 * in the cell layout the bf16 MFMA consumes, a ring of stages keeps the loads one or two K-tiles ahead behind counted vmcnt waits, and
 * a workgroup walks several output tiles so that the next tile's loads are in flight during an epilogue.
 *
 * "planes" of a row-major fp32 matrix X[R][K] (K % 8 == 0), ld >= R:   P[3][K / 8][ld][8] bf16 (uint16 bit patterns),
 *     X[r][8 c + j] == bf16(P[0][c][r][j]) + bf16(P[1][c][r][j]) + bf16(P[2][c][r][j])      exactly, each plane the
 *     round-to-nearest-even bf16 of what the previous ones left (the same split as conv_gemm_split_kernel and mit_gemm_split_pack:
 *     the weights' planes [3][Kw / 8][ldw][8] ARE this layout with r = output column).
 * mit_pgemm:  C[z][m][n] = epilogue( sum_k A[z][m][k] * W[z][k][n] ),  the sum taken as NPROD (6 | 9) bf16 MFMA products per 16-wide k
 *     step in the order of the split tiles: results are bit-identical to mit_conv_gemm on a "split*p6*" / "split*p9*" tile for the
 *     same operands.  epilogue(v) = act((v + pre) * scale[n] + bias[n]) + post   (MIT_ACT_POST_FIRST as in MitConvGemm).
 *     Output either fp32 row-major (c, ldc) or planes (c_planes, ld_cp: N % 8 == 0; pre / post must be NULL), or both NULL = error.
 * Replaces the same reference calls as mit_conv_gemm for these layers: the pointwise convolutions of ConvNeXtBlock
 * (ocr/model_48px.py:203-214) and the convl2l / convl2g / convg2l products of the FFC blocks (inpainting_lama_mpe.py:349-369). */
typedef struct MitPGemm {
    const uint16_t *a_planes; /* [Z][3][K/8][lda][8] */
    int64_t a_zs;             /* uint16 elements between z slices of A (0 for Z == 1) */
    int64_t lda;              /* rows per (plane, k-cell) slab, >= M */
    const uint16_t *w_planes; /* [Z][3][K/8][ldw][8] (mit_gemm_split_pack) */
    int64_t w_zs;             /* uint16 elements between z slices of W (0: shared) */
    int64_t ldw;              /* columns per slab, >= N */
    int32_t M, N, K, Z;       /* K % 16 == 0 */
    float *c;                 /* fp32 output [Z][M][ldc] or NULL */
    int64_t ldc, c_zs;
    const float *pre;         /* optional fp32 operands of the epilogue, row-major like c (own strides) */
    int64_t ld_pre, pre_zs;
    const float *post;
    int64_t ld_post, post_zs;
    uint16_t *c_planes;       /* planar output [Z][3][N/8][ld_cp][8] or NULL */
    int64_t ld_cp, cp_zs;
    const float *scale, *bias;
    int32_t act;
    float act_alpha;
    int32_t nprod;            /* 6 | 9 (0 = follow mit_gemm_mode_get(), which must then be 6 or 9) */
    int32_t tile;             /* -1 = automatic; else an index into mit_pgemm_tile_name() (tests / tuning) */
} MitPGemm;
int mit_pgemm(const MitPGemm *desc, void *stream);
const char *mit_pgemm_tile_name(int tile); /* NULL past the table */
/* 1 when mit_pgemm accepts the problem (sizes / alignment); 0 otherwise, with the reason in mit_last_error(). */
int mit_pgemm_supported(const MitPGemm *desc);
/* X fp32 [R][K] (row stride ldx floats, ldx % 4 == 0, K % 8 == 0) -> planes [3][K/8][ld][8] as above.  The stand-alone producer
 * (tests, and tensors whose producer has no planar form). */
int mit_split_planes(const float *x_dev, int64_t ldx, int R, int K, uint16_t *planes_dev, int64_t ld, void *stream);
/* planes -> fp32 (the exact sum hi + mid + lo): tests and debugging. */
int mit_join_planes(const uint16_t *planes_dev, int64_t ld, int R, int K, float *x_dev, int64_t ldx, void *stream);

/* k x k (3, 5, 7) stride-1 "same" convolution with 1..4 output channels on the fp32 VALU (an MFMA tile would idle 29 of
 * its 32 columns): out[b,y,x,n] = act(sum in[b,y+dy,x+dx,c] * w4[(ky*k+kx)*Cin + c][n] + bias[n]).  in: NHWC with pixel
 * stride in_pixstride floats (Cin % 16 == 0 channels used); w4: [k*k][Cin][4] (output channel padded to 4, zeros beyond
 * Cout); out: pixel stride out_pixstride, Cout floats written.  w_pairs (optional, Cout <= 3, 32-byte aligned): the same weights
 * channel-fastest, [k*k][Cin / 4][4 outputs (zeros beyond Cout)][4 channels] — the operand pairs (channels c, c + 1 of one output) of
 * the packed-FMA kernel that Cout <= 3 takes when it is given (2.7x fewer VALU instructions; accumulators hold even / odd channel
 * sums, no packed instruction carries an op_sel / neg modifier); NULL = the plain kernel.  in_planestride != 0 (packed kernel only): the
 * input arrives as Cin / 16 planes of [B,H,W,16] (in_pixstride = 16), in_planestride floats apart — what the producing convolution
 * writes through a column-split output map (MitTensorMap.nsplit = 16): a 16-channel group of a tile is then a run of whole 128-byte
 * lines instead of a quarter of every pixel's 256 bytes.
 * Round 6: in_pixstride == 4 with in_planestride != 0 = planes of FOUR channels [Cin / 4][B][H][W][4]: each 4-channel slice's halo tile
 * goes global -> LDS by global_load_lds_dwordx4 (no staging registers, 4 workgroups per CU; reflect padding only); a NEGATIVE
 * in_planestride (-stride) says every plane stores its images parity-major, [2 (y & 1)][2 (x & 1)][H / 2][W / 2][4] — the layout in
 * which the stride-2 transposed convolution that produces them writes consecutive pixels per launch.  Same bits in every layout.
 * live_cells (optional, device): a byte per 8-row x 32-column cell of the output, [B][ceil(H / 8)][ceil(W / 32)].  A workgroup whose tile
 * (16 x 64 in the packed kernels, 8 x 32 in the plain one) covers only zero cells issues no load or LDS-DMA request and stores nothing;
 * every other tile computes what it computes without the map.  NULL = every tile.
 * Replaces ReflectionPad2d(3) + Conv2d(64, 3, 7) + sigmoid at the end of FFCResNetGenerator (inpainting_lama_mpe.py:597-600). */
int mit_conv_small_cout(const float *in_dev, int64_t in_pixstride, int64_t in_planestride, const float *w4_dev, const float *w_pairs_dev, const float *bias_dev, float *out_dev,
                        int64_t out_pixstride, int B, int H, int W, int Cin, int Cout, int k, int pad_mode, int act,
                        float act_alpha, const uint8_t *live_cells, void *stream);

/* ConvTranspose2d(Cin -> 1, stride 2) (+ scale, bias, activation) in ONE pass over the input and over a given output extent only
 * (ABI 24; csrc/convt_cout1.hip).  Two forms, anything else is refused: k4 s2 p1 at Cin = 64 (`upconv6`, ctd_utils/basemodel.py:20) and
 * k2 s2 p0 at Cin = 16 (the last layer of both DB branches, basemodel.py:93,96).
 *   x:    [B][Hi][Wi][Cin] fp32 with strides x_bs / x_ys / x_xs floats (each a multiple of 4; channel stride 1), 16-byte aligned
 *   w:    [Cin][1][k][k] as the layer holds it, 16-byte aligned;  scale / bias: one float each, or NULL (1 / 0)
 *   out:  a one-channel map with strides out_bs / out_ys / out_xs floats; the layer's output is 2 Hi x 2 Wi, and only rows < out_h and
 *         columns < out_w of it are computed and written (the rest of `out` is left as it is)
 * Bit-identical to the four parity launches of mit_conv_gemm on its N <= 4 kernel (same lane partition of the channels, tap order,
 * shuffle tree and epilogue).  A workgroup owns MIT_CONVT_COUT1_STRIP_K4 / _K2 columns of input positions. */
#define MIT_CONVT_COUT1_STRIP_K4 16
#define MIT_CONVT_COUT1_STRIP_K2 64
int mit_convt_cout1(const float *x_dev, int64_t x_bs, int64_t x_ys, int64_t x_xs, int B, int Hi, int Wi, int Cin, const float *w_dev, int k,
                    int stride, int pad, const float *scale_dev, const float *bias_dev, int act, float act_alpha, float *out_dev,
                    int64_t out_bs, int64_t out_ys, int64_t out_xs, int out_h, int out_w, void *stream);

/* Which parts of LaMa's decoder tail a composite reads (lama_post takes the prediction only where mask >= 127): from mask [B][H][W] u8
 * (H, W multiples of 8), on `stream`, with no allocation, synchronisation or copy to the host,
 *   cells                the live-cell map of mit_conv_small_cout, [B][H / 8][ceil(W / 32)] bytes;
 *   listL / startL       the live-block list of the L-th transposed convolution (L = 0: output H/4, 1: H/2, 2: H) as MitConvGemm takes
 *                        it (live_blocks / live_start) for that layer's parity sub-grid [B][H >> (3 - L)][W >> (3 - L)] — one list for
 *                        its four parity launches; listL holds up to B * ceil(h / 8) * ceil(w / 8) ids, startL B + 1 entries.
 * A block is live when one of its positions has an output, in one of the 2 x 2 parities, that a needed position of the next layer reads:
 * need(H) = dilate(mask >= 127, 3) for the 7x7 window; need(input) = dilate(pool2x2_any(need(output)), 1) per transposed convolution
 * (k3 s2 p1 op1: input i feeds outputs 2i-1, 2i, 2i+1).  Lists are in block-raster order, image after image.
 * work: mit_lama_tail_need_work(B, H, W) bytes of scratch, 16-byte aligned.  Nothing in the reference corresponds to it. */
int64_t mit_lama_tail_need_work(int B, int H, int W);
int mit_lama_tail_need(const uint8_t *mask_dev, int B, int H, int W, uint8_t *cells_dev, int32_t *list0_dev, int32_t *start0_dev, int32_t *list1_dev,
                       int32_t *start1_dev, int32_t *list2_dev, int32_t *start2_dev, uint8_t *work_dev, void *stream);

/* The ConvNeXt block's pointwise pair as ONE launch (round 5): out = post + scale2 * (W2 . gelu(W1 . x + b1)) + bias2 per row, i.e.
 * pwconv1 -> GELU -> pwconv2 -> gamma -> + input of ConvNeXtBlock.forward (manga_translator/ocr/model_48px.py:203-214), in the
 * split-bf16 p6 arithmetic of mit_conv_gemm's tiles; the 4C-wide hidden activations stay in registers (as two launches the C = 80 stage
 * writes and re-reads [M, 320] fp32).  x [M, C] (row stride ldx floats), w1_planes = mit_gemm_split_pack of pwconv1's packed weight
 * [K = C][ldw = 4C]; w2perm_planes = mit_gemm_split_pack of pwconv2's packed weight [K = 4C][ldn2] AFTER permuting its rows to the order
 * in which the first contraction's accumulator registers hold the hidden index (k' = 32 hb + 16 s + 8 lh + j  <-  hidden
 * 32 hb + (j & 3) + 8 (2 s + (j >> 2)) + 4 lh; manga_image_translator_amd/ocr48.py builds it); b1 [4C]; scale2 / bias2 [C] (gamma,
 * gamma * bias; NULL = 1 / 0); post [M, C] or NULL (may be out itself).  mit_convnext_mlp_supported(C): 1 for the instantiated
 * widths (80).  The hidden activations are bit-identical to the two-launch form's; the second contraction adds the same products with
 * the 16 values of an MFMA step in other k slots (last-bit differences in the fp32 sums, same bound). */
int mit_convnext_mlp_supported(int C);
int mit_convnext_mlp(const float *x_dev, int64_t ldx, int M, int C, const uint16_t *w1_planes_dev, const float *b1_dev,
                     const uint16_t *w2perm_planes_dev, int64_t ldn2, const float *scale2_dev, const float *bias2_dev,
                     const float *post_dev, int64_t ldp, float *out_dev, int64_t ldo, void *stream);

/* ---- Winograd F(4x4, 3x3) for the stride-1 3x3 convolutions of the FFC blocks (inpainting_lama_mpe.py:349-369: convl2l,
 * convg2l, convl2g under ReflectionPad; the reference calls nn.Conv2d = 9 multiplies per output, this form 2.25):
 *   mit_wino43_input : x NHWC [B,H,W,C] (strides in floats) -> V [36][T][C], T = B * ceil(H/4) * ceil(W/4), the B^T d B
 *                      transform of the 6x6 patch (pad 1, MIT_PAD_REFLECT or MIT_PAD_ZERO) of every 4x4 output tile;
 *   the 36 products M_z = V_z [T x C] @ U_z [C x N] (U = G g G^T, transformed once on the host) run on mit_conv_gemm, Z = 36;
 *   mit_wino43_output: M [36][T][N] -> y NHWC = act((A^T m A) * scale[n] + bias[n]) + post, outputs past H / W dropped.
 * fp32 throughout; per-layer error ~1e-5 of the output range against 3e-7 for the direct form (tests/test_winograd_gpu.py). */
int mit_wino43_input(const float *x_dev, int64_t x_bs, int64_t x_ys, int64_t x_xs, float *v_dev, int B, int H, int W, int C,
                     int pad_mode, void *stream);
int mit_wino43_output(const float *m_dev, float *y_dev, int64_t y_bs, int64_t y_ys, int64_t y_xs, const float *post_dev,
                      int64_t p_bs, int64_t p_ys, int64_t p_xs, const float *scale_dev, const float *bias_dev, int B, int H,
                      int W, int N, int act, float alpha, void *stream);

/* kernel-time probe (measurement only; bench.py's roofline leg).  While enabled every mit_conv_gemm launch — from the
 * host or from the native decoder loop — is bracketed by HIP events on its own stream; mit_prof_read synchronises those
 * events and returns, per tile configuration, the launch count, the summed kernel time and the summed FLOPs
 * (exec = 2*M*N*K*Z as launched; alg = the caller's figure given through mit_prof_tag_next for the next launch of
 * this thread, else exec).  Nothing in the reference corresponds to it (the reference has no profiler hooks on this path). */
typedef struct MitProfStat {
    int64_t launches;
    double ms, exec_flops, alg_flops;
} MitProfStat;
int mit_prof_enable(int on); /* clears the records; on != 0 starts recording */
int mit_prof_tag_next(double alg_flops);
int mit_prof_read(MitProfStat *stats, int max_cfgs, int *n_cfgs);
/* One CSV line per recorded launch (tile, M, N, K, taps, Z, act, ms, executed / algorithmic FLOPs, bytes of the Winograd
 * pre-operand its epilogue read — MitConvGemm.wino_m, 0 without one): the per-layer view behind
 * bench.py's per-tile totals (scripts/ocr_layers.py).  Call before mit_prof_enable() clears the records. */
int mit_prof_dump(const char *path);
/* The same probe for the kernels that are NOT mit_conv_gemm (the HBM-bound transforms / FFTs / element-wise passes, the VALU
 * output convolution, the OCR attention / softmax kernels): per kernel name, launches, summed time and the summed ALGORITHMIC
 * bytes (inputs read once + outputs written once at the stored precision) and FLOPs of its launches.
 * mit_prof_enable() arms and clears it together with the conv probe. */
typedef struct MitProfKernelStat {
    char name[48];
    int64_t launches;
    double ms, alg_bytes, alg_flops;
} MitProfKernelStat;
int mit_prof_kernels_read(MitProfKernelStat *stats, int max_stats, int *n_stats);

/* 8-bit image resizes around the inpainter, on device bytes [B,H,W,C] -> [B,dh,dw,C] (1 <= C <= 4):
 *   mode 0 = cv2.INTER_LINEAR (8-bit path, 11-bit coefficients)   — the resize to a multiple of 8 and back
 *            (inpainting_lama_mpe.py:77-79,112-113), detection/common.py:79-84
 *   mode 1 = exact 2x shrink = 2x2 box mean (what OpenCV substitutes for both linear flavours at scale 1/2)
 *   mode 2 = cv2.INTER_LINEAR_EXACT (8.8 fixed point)             — resize_keep_aspect (utils/generic.py:251-255, _infer :64-66)
 *   mode 3 = cv2.INTER_AREA at any ratio, both directions (ABI 13)  — the colorizer's denoiser cap and resize_pad
 *            (colorization/manga_colorization_v2_utils/denoising/denoiser.py:75-77, utils/utils.py:17-38)
 * Tap tables (modes 0, 2, 3) come from the host (manga_image_translator_amd/imgproc.py): per destination index the first source
 * index (int32) and two uint16 weights {w(idx), w(idx+1)}; idx+1 is clamped to the last row / column by the kernel.  Mode 3: K
 * uint16 numerators per destination index over the source length (K = ceil(src / dst) + 1 when both sides shrink, else 2; H, W
 * <= 65535), result (2 N + H W) / (2 H W) with N the integer weighted sum. */
int mit_resize_u8(const uint8_t *src_dev, int B, int H, int W, int C, uint8_t *dst_dev, int dh, int dw, int mode, const int *yidx_dev,
                  const uint16_t *ycoef_dev, const int *xidx_dev, const uint16_t *xcoef_dev, void *stream);
/* Pillow's 8-bit ImagingResample for ONE axis of device bytes [B,H,W,C] (C = 1 or 3; ABI 18): axis 0 resamples W -> n_out
 * (dst [B,H,n_out,C]), axis 1 resamples H -> n_out (dst [B,n_out,W,C]).  `Image.resize` is the horizontal pass followed by the vertical
 * pass on its 8-bit result, a pass whose size does not change skipped: the caller launches this once per pass.  It is the final
 * BILINEAR resize by ratio / 4 of the ESRGAN upscaler (upscaling/esrgan_pytorch.py:546) and the BICUBIC resizes of the ratio
 * correction (upscaling/common.py:32) and of the revert to the input size (manga_translator.py:629).  Tables from the host
 * (manga_image_translator_amd/imgproc.py pil_coeffs): bounds int32 [n_out, 2] = {xmin, cnt} with xmin >= 0, xmin + cnt <= the axis
 * length and cnt <= ksize; coef int32 [n_out, ksize], Pillow's 22-bit integer coefficients.  Output byte
 * clamp((2^21 + sum_x src[xmin + x] * coef[x]) >> 22, 0, 255), int32 arithmetic.  src and dst must not alias. */
int mit_resample_pil_u8(const uint8_t *src_dev, int B, int H, int W, int C, uint8_t *dst_dev, int n_out, int axis, const int *bounds_dev,
                        const int *coef_dev, int ksize, void *stream);
/* cv2.bilateralFilter on 8-bit RGB pages [B,H,W,3] (mask_refinement/text_mask_utils.py:159 and detection/default.py:64 call it
 * with d = 17, sigmaColor = sigmaSpace = 80): BORDER_REFLECT_101, `ntaps` taps of the circular support in row-major order, tap k at
 * (dy, dx) = (tap_ofs[k] >> 16, (int16)(tap_ofs[k] & 0xffff)) with spatial weight tap_w[k]; colour weight
 * color_w[|dr| + |dg| + |db|] (768 floats); fp32 sums in tap order, result = round-half-even(sum / wsum).  The tables are OpenCV's
 * ((float)exp(double)), built by the host (imgproc.bilateral_tables).  radius <= 16.  src and dst must not alias. */
int mit_bilateral_u8c3(const uint8_t *src_dev, uint8_t *dst_dev, int B, int H, int W, int radius, int ntaps, const int *tap_ofs_dev,
                       const float *tap_w_dev, const float *color_w_dev, void *stream);
/* out = mask >= thr ? a : b per pixel (C channels): ``img_inpainted * mask_original + img_original * (1 - mask_original)`` with the
 * original mask thresholded at 127 (inpainting_lama_mpe.py:57-61,116). */
int mit_select_u8(const uint8_t *mask_dev, int thr, const uint8_t *a_dev, const uint8_t *b_dev, uint8_t *out_dev, int64_t npix, int C,
                  void *stream);
/* The mask tail of the DBNet detectors (detection/default.py:89-95, dbnet_convnext.py the same lines): cv2.resize(mask, (2w, 2h),
 * INTER_LINEAR) of the float text mask, the crop of the padding and np.clip(m * 255, 0, 255).astype(np.uint8), in one pass.
 * src f32 [B,h,w] with `src_batch_stride` / `src_row_stride` in elements (unit stride along w: an engine's workspace view as it is);
 * out u8 [B,oh,ow] dense, oh <= 2h and ow <= 2w (the top-left oh x ow of the 2x map), oh and B at most 65535 a launch.  Output index i taps (i + 0.5) * 0.5 - 0.5:
 * weights 0.75 / 0.25 on the two nearest sources, 1 / 0 on the edge element at both borders; the horizontal pass
 * r = m[x0] * wx0 + m[x1] * wx1 first (fp32: two rounded products, one rounded sum, no FMA), the vertical pass the same way on its
 * results, then v * 255.0f, clamp to [0, 255], truncate.  Inputs are finite; NaN has no defined result.  Additive in ABI 25. */
int mit_dbnet_mask_tail(const float *src_dev, int64_t src_batch_stride, int64_t src_row_stride, int B, int h, int w, uint8_t *out_dev,
                        int oh, int ow, void *stream);

/* Webtoon strips: det_rearrange_forward's tiling around the detector network, on the device (ABI 25) ----------------------
 * Reference: utils/generic.py:876-997 (called from detection/ctd.py:137 and detection/default.py:60).  The plan (transpose, w, pw_num,
 * ph_num, ph_step, p_num; patch = pw_num * w) is rearrange.plan()'s restatement of :940-975.
 *
 * mit_rearrange_squares — the einops rearranges of :920-924 before square_pad_resize (:849-874): u8 page [H,W,3] -> the unshrunk squares
 * u8 [p_num, patch, patch, 3], band b = s * pw_num + j of square s cut at strip row b * ph_step:
 *   plain plan      sq[s][r][j*w + c]  = page[b*ph_step + r][c]        (w = W, strip length H)
 *   transposed plan sq[s][j*w + a][r]  = page[a][b*ph_step + r]        (w = H, strip length W: the wide strip's band^T)
 * Bands >= ph_num of the last square are zero.  The INTER_LINEAR shrink to the detect size (:871-872) is mit_resize_u8 on the result. */
int mit_rearrange_squares(const uint8_t *page_dev, int H, int W, int transpose, int w, int pw_num, int ph_num, int ph_step, int p_num,
                          uint8_t *sq_dev, void *stream);
/* mit_rearrange_stitch — _unrearrange (utils/generic.py:891-918): the network's output squares f32 [n, C, m, m] with element strides
 * (sn, sc, sy, sx) (a view of an engine's workspace as it is) -> the strip's map f32 [C, hh, pw] (transposed plan: [C, pw, hh]), dense.
 * step = int(ph_step * m / patch), pw = int(m / pw_num), hh = int(pw / w * h) and starts_dev (int32 [ph_num], non-decreasing: band p
 * starts at int(round(rel_step[p] * hh)), :904) come from the host.  Per element (c, y along the strip, x across it), in float32:
 *   v = 0;  for p = 0 .. ph_num-1:   t = starts[p]
 *     if t <= y < min(t + m, hh):        v = v + src[p / pw_num][c][y - t][(p % pw_num) * pw + x]     (transposed plan: [..x][y - t])
 *     if p > 0 and t <= y < t + m - step: v = v * 0.5f                                                    (:909-911, the running average)
 * which is the reference's band-by-band accumulation restated per element: bit-identical.  ops = 1 also writes dst_u8_dev (same shape):
 * (uint8)(v * 255.0f), truncating — postprocess_mask of the ctd detector (detection/ctd.py:41-44).  ops = 0: dst_u8_dev may be NULL. */
int mit_rearrange_stitch(const float *src_dev, int n, int C, int m, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int transpose, int pw_num,
                         int ph_num, int step, int pw, int hh, const int *starts_dev, float *dst_dev, uint8_t *dst_u8_dev, int ops, void *stream);

/* ctd detector: refine_mask on the GPU ------------------------------------------------------------
 * Reference: manga_translator/detection/ctd_utils/textmask.py:158-174 (refine_mask; :29-132 its helpers), called from
 * detection/ctd.py:177 with refine_mode=None.  Three phases over all text-line windows of a page; the host does numpy's histogram /
 * top-k colour / Otsu arithmetic between them (hostglue.refine_mask_gpu).  Bit-identical to hostglue.refine_mask. */
typedef struct MitRefineWindow {
    int x1, y1, x2, y2; /* crop [y1:y2, x1:x2] of the page (enlarge_window of the line's box) */
} MitRefineWindow;
typedef struct MitRefineCand {
    int kind;   /* 0 = none, 1 = inRange(grey, lo, hi), 2 + c = channel c > lo */
    int lo, hi; /* bounds (already rounded / saturated like cv2.inRange) or the Otsu threshold in lo */
    int invert; /* 1: take the complement (minxor_thresh picked cv2.bitwise_not) */
} MitRefineCand;
int64_t mit_ctd_refine_workspace_bytes(const MitRefineWindow *windows, int n);
/* phase A: hist_host[n][4][256] = grey levels under erode3x3(mask crop) > 127, then the three channel histograms of the crop.
 * page_dev u8 [H,W,3], pred_dev u8 [H,W] (the network's mask at page size), windows: HOST array.  Synchronises the stream. */
int mit_ctd_refine_hist(const uint8_t *page_dev, const uint8_t *pred_dev, int H, int W, const MitRefineWindow *windows, int n, int *hist_host,
                        void *workspace_dev, int64_t workspace_bytes, void *stream);
/* phase B: sums_host[n][6] = sum over the crop of (candidate ^ mask) as bytes for 6 raw candidates per line (cands_host[n][6]). */
int mit_ctd_refine_scores(const uint8_t *page_dev, const uint8_t *pred_dev, int H, int W, const MitRefineWindow *windows, int n,
                          const MitRefineCand *cands_host, uint64_t *sums_host, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* phase C: merge_mask_list per line over its (up to 4) candidates in the given order (order_host[n][4]), hole filling, and
 * out_dev[H,W] |= merged inside each window (out_dev must be zeroed by the caller).  Asynchronous on the stream. */
int mit_ctd_refine_merge(const uint8_t *page_dev, const uint8_t *pred_dev, int H, int W, const MitRefineWindow *windows, int n,
                         const MitRefineCand *order_host, uint8_t *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Mask refinement between OCR and inpainting -----------------------------------------------------
 * Reference: manga_translator/mask_refinement/text_mask_utils.py:68-94 (refine_mask -> pydensecrf). */

typedef struct MitCrfCrop {
    int x, y, w, h; /* crop rectangle inside the page, pixels */
} MitCrfCrop;

/* Elliptical dilation of byte masks, batched over jobs (cv2.dilate with cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), k odd, default
 * anchor and border: text_mask_utils.py:178-195).  Job j reads the source rectangle (sx, sy, sw, sh) — page coordinates — whose pixels
 * live at src_dev + src_off with row pitch spitch, and writes the window (dx, dy, dw, dh) of dst_dev [H, W]: source pixels outside the
 * source rectangle or outside the window count as 0 (the host form dilates the window as a sub-array).  merge = 0: dst = dilated;
 * merge = 1: dst |= dilated for {0, 255} masks (the union over the lines of a page; windows may overlap).  jobs_host is copied to
 * jobs_dev (n_jobs entries of device scratch) on the stream. */
typedef struct MitDilateJob {
    int32_t sx, sy, sw, sh;
    int32_t dx, dy, dw, dh;
    int32_t k, spitch;
    int64_t src_off;
} MitDilateJob;
int mit_mask_dilate_jobs(const uint8_t *src_dev, const MitDilateJob *jobs_host, int n_jobs, uint8_t *dst_dev, int H, int W, int merge,
                         MitDilateJob *jobs_dev, void *stream);
/* buf[i] = buf[i] ? 255 : 0 in place (mask_refinement/__init__.py:29 after the resize back to page size). */
int mit_binarize_u8(uint8_t *buf_dev, int64_t n, void *stream);

/* Bytes of device workspace mit_densecrf_refine needs for these crops (-1: bad crops / batch too large). */
int64_t mit_densecrf_workspace_bytes(const MitCrfCrop *crops, int n_crops);
/* DenseCRF2D mean-field refinement of every text line's mask crop of one page, batched:
 *   unary = -log(clip([1 - m, m], 1e-5, 1)) through unary_lut_dev (256 x 2 floats, built by the host),
 *   pairwise Gaussian (x, y) / sxy_gauss with Potts weight w_gauss + bilateral (x, y) / sxy_bilateral, rgb / srgb_bilateral with
 *   w_bilateral, both through a permutohedral-lattice filter (DIAG_KERNEL, NO_NORMALIZATION), `iterations` mean-field steps,
 *   out = 255 * argmax(Q).   The reference's call is (1, 3, 23, 7, 20, 5).
 * page_dev: u8 [H,W,3] on the device (the bilateral-filtered page); crops: HOST array; mask_dev / out_dev: the crops' masks back to
 * back (crop c at offset sum_{c'<c} w*h, row-major); q_dev (optional): float [sum w*h][2] final marginals.  Synchronises the stream. */
int mit_densecrf_refine(const uint8_t *page_dev, int H, int W, const MitCrfCrop *crops, int n_crops, const uint8_t *mask_dev,
                        uint8_t *out_dev, float *q_dev, float sxy_gauss, float w_gauss, float sxy_bilateral, float srgb_bilateral,
                        float w_bilateral, int iterations, const float *unary_lut_dev, void *workspace_dev, int64_t workspace_bytes,
                        void *stream);

/* LaMa inpainting stage: memory-bound pieces ----------------------------------------------
 * Reference: manga_translator/inpainting/inpainting_lama_mpe.py. */

/* Complex FFT of length h (power of two <= 512) along the row axis of planar re/im data, ncols independent columns (column
 * stride 1), B batches: element (b, t, r, c) at base + b*bs + t*ts + r*hs + c with t = 0 (re) / 1 (im).
 * out[k] = scale * sum_r in[r] * exp(-/+ 2 pi i k r / h) (inverse != 0: +).  twiddle_dev: h/2 (cos, sin) pairs of 2 pi k / h.
 * In-place (in == out with equal strides) is allowed.  The H-axis half of torch.fft.rfftn / irfftn(norm='ortho') in
 * FourierUnit.forward (inpainting_lama_mpe.py:228,252); the W axis is mit_rfft_rows / mit_irfft_rows (or a dense DFT on
 * mit_conv_gemm for widths those do not cover). */
int mit_fft_cols(const float *in_dev, int64_t in_bs, int64_t in_ts, int64_t in_hs, float *out_dev, int64_t out_bs,
                 int64_t out_ts, int64_t out_hs, const float *twiddle_dev, int B, int h, int64_t ncols, int inverse, float scale,
                 void *stream);

/* Real FFT of length w along the W axis of NHWC rows: x[b, h, :, c] (element at in + b*in_bs + h*in_hs + x*in_ws + c) -> the
 * w/2+1 Hermitian bins, planar: element (b, t, h, k, c) at out + b*out_bs + t*out_ts + h*out_hs + k*out_ks + c, t = 0 (re) / 1 (im),
 * multiplied by `scale` (1/sqrt(w) for norm='ortho').  w must be even, <= 512, with w/2 a product of {2,3,5,7,11,13}
 * (mit_rfft_rows_supported); C % 4 == 0.  tables_dev: w/2 (cos, sin) pairs of 2 pi j / (w/2) followed by w/2+1 pairs of
 * 2 pi k / w (fp32, rounded from float64 on the host).  Mixed-radix Stockham butterflies in LDS on the packed sequence
 * z[n] = x[2n] + i x[2n+1].  The W-axis half of torch.fft.rfftn(norm='ortho') in FourierUnit.forward (inpainting_lama_mpe.py:228). */
int mit_rfft_rows_supported(int w);
int mit_rfft_rows(const float *in_dev, int64_t in_bs, int64_t in_hs, int64_t in_ws, float *out_dev, int64_t out_bs, int64_t out_ts,
                  int64_t out_hs, int64_t out_ks, const float *tables_dev, int B, int h, int w, int C, float scale, void *stream);
/* Inverse of mit_rfft_rows: out[b, h, x, c] = scale * irfft_w(in[b, :, h, :, c]) (+ res[b, h, x, c] when res_dev != NULL), the
 * imaginary parts of the DC and Nyquist bins ignored like pocketfft's c2r.  The W-axis half of torch.fft.irfftn(norm='ortho') and
 * the ``x + fu(x)`` of SpectralTransform.forward (inpainting_lama_mpe.py:252,305). */
int mit_irfft_rows(const float *in_dev, int64_t in_bs, int64_t in_ts, int64_t in_hs, int64_t in_ks, float *out_dev, int64_t out_bs,
                   int64_t out_hs, int64_t out_ws, const float *res_dev, int64_t res_bs, int64_t res_hs, int64_t res_ws,
                   const float *tables_dev, int B, int h, int w, int C, float scale, void *stream);

/* u8 page [B,H,W,3] + u8 mask [B,H,W] -> fp32 NHWC [B,H,W,4] = (rgb/255*(1-m), m), m = (mask/255 >= 0.5).
 * Replaces the host-side tensor prep of LamaMPEInpainter._infer :82-92 and the torch.cat of
 * FFCResNetGenerator.forward :604. */
int mit_lama_prep(const uint8_t *img_dev, const uint8_t *mask_dev, float *out_dev, int B, int H, int W, void *stream);

/* The same network input, written as the reflect-padded image [B, H + 2*pad, Wp, 4] (Wp >= W + 2*pad, the surplus columns zero) that
 * the row-packed stem convolution reads: ReflectionPad2d(3) of FFCResNetGenerator.model[0] (inpainting_lama_mpe.py:560) materialised
 * once, so that each kernel row of the 7x7 4->64 stem is ONE contiguous 32-float read (7 pixels x 4 channels + 4 zero-weight floats). */
int mit_lama_prep_padded(const uint8_t *img_dev, const uint8_t *mask_dev, float *out_dev, int B, int H, int W, int pad, int Wp, void *stream);

/* Masked positional-encoding index maps on the 256x256 structure grid:
 * hole = (INTER_AREA resize of the binary mask) > 0; relpos = clipped ring distance; direct = 4 direction bits.
 * Replaces LamaFourier.load_masked_position_encoding :751-807 (cv2.resize + the cv2.filter2D loop on the CPU).
 * ys/yc/yw (xs/xc/xw): DEVICE arrays describing the separable resize: destination row d averages source rows
 * [ys[d], ys[d]+yc[d]) with weights yw[d*ymax + j] (doubles). */
int mit_lama_mpe_index(const uint8_t *mask_dev, int B, int H, int W, const int *ys_dev, const int *yc_dev,
                       const double *yw_dev, int ymax, const int *xs_dev, const int *xc_dev, const double *xw_dev,
                       int xmax, uint8_t *hole_dev, uint8_t *relpos_dev, uint8_t *direct_dev, void *stream);

/* x[B,H,W,64] += alpha5 * rel_pos_emb[rel] + alpha6 * (direct @ direct_emb), with the 256-grid maps
 * nearest-resized through ymap[H] / xmap[W] (cv2.INTER_NEAREST :810-813) and zeroed outside the mask.
 * Replaces MPE.forward :625-632 and the two adds of FFCResNetGenerator.forward :611-612. */
int mit_lama_mpe_add(float *x_dev, const uint8_t *mask_dev, const uint8_t *relpos_dev, const uint8_t *direct_dev,
                     const int *ymap_dev, const int *xmap_dev, const float *emb_dev, const float *dirw_dev, float alpha5,
                     float alpha6, int B, int H, int W, void *stream);
/* The same lookup as per-pixel TABLE ROWS for the stem convolution's epilogue (MitConvGemm.lut_rows): rows[b][y][x] = rel | bits << 16
 * inside the mask, 0 outside, with rel / bits read from the 256-grid maps through ymap / xmap exactly as mit_lama_mpe_add reads them.
 * With lut1[rel] = alpha5 * rel_pos_emb[rel] (128 rows) and lut2[bits] = alpha6 * sum of the set directions' rows of direct_emb (16 rows,
 * summed in bit order), the stem launch performs the two adds of FFCResNetGenerator.forward :611-612 itself — bit-identical to
 * mit_lama_mpe_add after the stem, without the extra read-modify-write of [B,H,W,64]. */
int mit_lama_mpe_rows(const uint8_t *mask_dev, const uint8_t *relpos_dev, const uint8_t *direct_dev, const int *ymap_dev,
                      const int *xmap_dev, int32_t *rows_dev, int B, int H, int W, void *stream);

/* predicted fp32 (pixel stride pred_pixstride floats, 3 used) + page + mask -> inpainted u8 [B,H,W,3]:
 * pred*m + (1-m)*img (:726), *255 truncated to u8 (:111), composited with the original through mask >= 127 (:59-60,117).
 * composite == 0 stops after the truncation (``img_inpainted`` of :111, every pixel from the network): what the plugin resizes
 * back to the page size before compositing there (:112-117) when the page had to be resized. */
int mit_lama_post(const float *pred_dev, int64_t pred_pixstride, const uint8_t *img_dev, const uint8_t *mask_dev,
                  uint8_t *out_dev, int B, int H, int W, int composite, void *stream);

/* AOT inpainter (the reference's ``Inpainter.default``): memory-bound pieces ---------------------------------------------
 * Reference: manga_translator/inpainting/inpainting_aot.py (AOTGenerator :240-274) and the plugin path it inherits,
 * inpainting_lama_mpe.py:_infer :82-117.  The convolutions run on mit_conv_gemm; every gated layer is ONE launch whose 2C
 * output columns are (signal | gate). */

/* u8 page [B,H,W,3] + u8 mask [B,H,W] -> fp32 NHWC [B,H,W,4] = (m, (rgb / 127.5f - 1) * (1 - m)), m = (mask / 255.0f >= 0.5):
 * the inputs of AOTGenerator.forward, torch.cat([mask, img]) (:266), as _infer builds them (inpainting_lama_mpe.py:84-92). */
int mit_aot_prep(const uint8_t *img_dev, const uint8_t *mask_dev, float *out_dev, int B, int H, int W, void *stream);

/* The gate of GatedWSConvPadded / GatedWSTransposeConvPadded (:128-133, :142-146): per pixel, in [.., 2C] = (signal | gate) ->
 * out [.., C] = signal * sigmoid(gate) * 1.8, then relu_nf (relu(x) * 1.7139588594436646, :35-36) when relu_nf != 0.  npix pixels
 * with pixel strides in floats (the output may be a channel slice of a wider tensor).  C % 4 == 0, 16-byte aligned operands. */
int mit_aot_gate(const float *in_dev, int64_t in_pixstride, float *out_dev, int64_t out_pixstride, int64_t npix, int C, int relu_nf,
                 void *stream);

/* Bytes of the workspace mit_aot_plane_stats needs for B planes of hw pixels x C channels. */
int64_t mit_aot_plane_stats_ws(int B, int hw, int C);
/* The plane statistics of my_layer_norm (:163-168) on NHWC x [B, hw, C] (batch / pixel strides in floats): mean [B, C] and
 * istd [B, C] = 1 / (std + 1e-9) with the unbiased std over the hw pixels of each (b, c).  Two passes (the second sums around
 * the mean of the first, so |mean| >> std stays accurate), double partial sums over fixed 512-pixel chunks reduced in a fixed
 * order: deterministic, and a page's result does not depend on the batch it is in.  C a power of two in [4, 1024]. */
int mit_aot_plane_stats(const float *x_dev, int64_t batch_stride, int64_t pixstride, int B, int hw, int C, void *ws_dev, int64_t ws_bytes,
                        float *mean_dev, float *istd_dev, void *stream);

/* AOTBlock's output (:189-192), in place over x: m = sigmoid(5 * (2 * (gate - mean) * istd - 1)), x = x * (1 - m) + fuse * m.
 * x / fuse / gate [B, hw, C] with their own batch / pixel strides (floats); mean / istd [B, C] from mit_aot_plane_stats. */
int mit_aot_blend(float *x_dev, int64_t x_bs, int64_t x_ps, const float *fuse_dev, int64_t f_bs, int64_t f_ps, const float *gate_dev,
                  int64_t g_bs, int64_t g_ps, const float *mean_dev, const float *istd_dev, int B, int hw, int C, void *stream);

/* The last gated layer's pair (tail[8], 3 signal + 3 gate channels at pixel stride pre_pixstride) -> signal * sigmoid(gate) * 1.8
 * -> clip(-1, 1) (:274) -> ((x + 1) * 127.5f) truncated to u8 (inpainting_lama_mpe.py:114), composited with the page through
 * mask >= 127 (:57-61,117).  composite == 0 stops after the truncation (``img_inpainted``, every pixel from the network), as in
 * mit_lama_post.  preclip_dev (NULL = off): the value before the clip, [B,H,W,3], on every pixel (also where the composite hands
 * back the page).  A NaN product (NaN or inf * 0 in the pair) has no defined byte in the reference (astype(uint8) of NaN); here
 * fmaxf(NaN, -1) clips it to -1, so its byte is 0, and preclip_dev receives the NaN. */
int mit_aot_post(const float *pre_dev, int64_t pre_pixstride, const uint8_t *img_dev, const uint8_t *mask_dev, uint8_t *out_dev,
                 float *preclip_dev, int B, int H, int W, int composite, void *stream);

/* manga-colorization-v2 colorizer (the reference's ``Colorizer.mc2``) -----------------------------------------------------
 * Reference: manga_translator/colorization/manga_colorization_v2.py:_infer :42-74 and manga_colorization_v2_utils/.  The dense
 * convolutions run on mit_conv_gemm; these are the grouped convolution, squeeze-and-excitation and the u8 glue (ABI 13). */

/* Grouped 3x3 convolution of the ResNeXt blocks (networks/extractor.py:37-38, networks/models.py:131-133): NHWC fp32, Cin = Cout = C
 * (a multiple of 16) in groups of cpg = 2 | 4 | 8 | 16 channels, stride 1 | 2, dilation d = padding = 1 | 2 | 4, zero padding, torch
 * weight layout [C][cpg][3][3]; then v * scale[c] (optional) + bias[c] (optional) and act (MIT_ACT_NONE | RELU | LEAKY with alpha).
 * Input and output are strided channel views: batch and pixel strides in floats (multiples of 4; rows are W pixels), 16-byte aligned.
 * Each output is one fmaf chain over (tap, input channel) in that order: deterministic and independent of B. */
int mit_grouped_conv3x3(const float *in_dev, int64_t in_bs, int64_t in_ps, int B, int H, int W, int C, int cpg, int stride, int dilation,
                        const float *w_dev, const float *scale_dev, const float *bias_dev, int act, float alpha, float *out_dev,
                        int64_t out_bs, int64_t out_ps, void *stream);
/* LDS bytes one workgroup of mit_grouped_conv3x3 stages at that stride / dilation / group width. */
int64_t mit_grouped_conv3x3_lds_bytes(int stride, int dilation, int cpg);

/* Squeeze of Selayer (global_avgpool, networks/models.py:88-106): double partial sums per (sample, fixed 256-pixel chunk, channel)
 * of x [B, hw, C] (batch / pixel strides in floats) into the workspace [B][ceil(hw / 256)][C]; C a power of two in [4, 1024].
 * The strides must be multiples of 4 and x 16-byte aligned (checked); the caller sees to pixstride >= C and
 * batch stride >= hw * pixstride (not checked: with smaller strides pixels or planes overlap and the sums count them twice). */
int64_t mit_se_squeeze_ws(int B, int hw, int C);
int mit_se_squeeze(const float *x_dev, int64_t bs, int64_t ps, int B, int hw, int C, void *ws_dev, int64_t ws_bytes, void *stream);
/* Excite, one workgroup per sample: mean = (sum of the chunks in index order) / hw, s = sigmoid(w2 relu(w1 mean + b1) + b2) with
 * w1 [C/16][C], w2 [C][C/16] (the 1x1 convolutions conv1 / conv2); s [B][C]. */
int mit_se_excite(const void *ws_dev, int B, int hw, int C, const float *w1_dev, const float *b1_dev, const float *w2_dev,
                  const float *b2_dev, float *s_dev, void *stream);
/* out = act(x * s[b][c] + residual), act MIT_ACT_RELU (encoder blocks, extractor.py:64-67) or MIT_ACT_NONE (tunnel blocks,
 * models.py:150).  Each operand has its own batch / pixel strides (floats, multiples of 4); out may alias x or residual. */
int mit_se_apply(const float *x_dev, int64_t x_bs, int64_t x_ps, const float *s_dev, const float *res_dev, int64_t r_bs, int64_t r_ps,
                 float *out_dev, int64_t o_bs, int64_t o_ps, int B, int hw, int C, int act, void *stream);

/* FFDNet input (denoiser.py:79-103, functions.py:16-56): u8 RGB(A) pages [B,H,W,Cin] -> fp32 [B,ceil(H/2),ceil(W/2),16] =
 * (sigma, sigma, sigma, space-to-depth channel 3 + c*4 + (i*2 + j), 0).  Values are divided by 255 only on a page whose max
 * (over RGB, found on the device into pmax_dev [B]) exceeds 1.2; odd sides repeat their last row / column. */
int mit_mc2_ffd_pack(const uint8_t *img_dev, int B, int H, int W, int Cin, float sigma, unsigned *pmax_dev, float *out_dev, void *stream);
/* FFDNet output (functions.py:58-83, denoiser.py:107-118, utils.py:17-33): depth-to-space of the 12-channel noise estimate (pixel
 * stride in floats), clamp(x - noise, 0, 1), crop to H x W, RGB -> BGR, (v * 255) truncated to u8.  plane_dev [B,H,W] receives B (the
 * channel the colorizer keeps, utils/utils.py:44), bgr_dev [B,H,W,3] the whole page; either may be NULL. */
int mit_mc2_ffd_unpack(const uint8_t *img_dev, int B, int H, int W, int Cin, const unsigned *pmax_dev, const float *noise_dev,
                       int64_t noise_pixstride, uint8_t *plane_dev, uint8_t *bgr_dev, void *stream);
/* Generator input (utils/utils.py:27-38, ToTensor, manga_colorization_v2.py:58-59): u8 plane [B,h,w] -> fp32 [B,Hp,Wp,4] =
 * (v / 255, 0, 0, 0) with np.pad(.., 'maximum') on the one padded side (rows: column max; columns: row max). */
int mit_mc2_gen_in(const uint8_t *plane_dev, int B, int h, int w, float *out_dev, int Hp, int Wp, void *stream);
/* Generator output (manga_colorization_v2.py:61-74): tanh(pre) * 0.5 + 0.5, crop to h x w, * 255 truncated -> u8 RGB [B,h,w,3].
 * Evaluated in double, so the byte is floor((tanh(x) * 0.5 + 0.5) * 255) of the exact value; the reference's float32 evaluation
 * can differ by one only within float32 rounding of a truncation boundary (it rounds x = 9 up to 255; the exact value is 254.999996). */
int mit_mc2_post(const float *pre_dev, int64_t pre_pixstride, int B, int Hp, int Wp, uint8_t *out_dev, int h, int w, void *stream);

/* Text-detection stage (dbconvnext): the norms of DBNet on ConvNeXt ---------------------------
 * Reference: manga_translator/detection/dbnet_convnext.py (DBNetConvNext :450-491).  The convolutions and both MLP layers run on
 * mit_conv_gemm; these are the LayerNorms, which the network has where the other detectors have BatchNorm. */

/* nn.LayerNorm over the last dimension of fp32 [rows, D], row strides in floats (input and output may each be a channel slice of
 * a wider NHWC buffer: a pixel is a row).  timm's LayerNorm2d of the stem (:273), of every stage's downsample.0 (:156) and
 * LayerNorm of the up-blocks (:103).  D % 4 == 0, D <= 1024, strides multiples of 4, 16-byte aligned operands.  Two passes
 * (mean, then the centred second moment) in fp32; the order of the sums depends on D alone. */
int mit_layernorm_rows(const float *in_dev, int64_t in_rowstride, const float *w_dev, const float *b_dev, float *out_dev,
                       int64_t out_rowstride, int64_t rows, int D, float eps, void *stream);
/* ConvNeXtBlock.forward up to the MLP for a depthwise block (:114, :119-120): out = LayerNorm_C(dwconv7x7(x) + bdw) * g + b, zero
 * padding 3, NHWC with pixel strides in floats (x may be a slice of a concat buffer, out a slice or dense); w is [49][C] (tap-major).
 * C in {128, 256, 512, 1024}; any B, H, W >= 1.  The channel sums are fp32 in an order that depends on C alone, so an image's result
 * does not depend on the batch it is in.  One pass: a pixel's channels stay in one workgroup. */
int mit_dwconv7_ln_nhwc(const float *x_dev, int64_t x_pixstride, const float *w_dev, const float *bdw_dev, const float *g_dev,
                        const float *b_dev, float eps, float *out_dev, int64_t out_pixstride, int B, int H, int W, int C, void *stream);
/* 1 when the one-pass kernel above is the form to use at width C — it exists for that C and was measured faster there than
 * mit_dwconv_nhwc followed by mit_layernorm_rows (profiles/r23a_dbconvnext.json) —, else 0: the caller then runs the two launches. */
int mit_dwconv7_ln_supported(int C);

/* Text-detection stage (ctd): memory-bound pieces and NHWC helpers ---------------------------
 * Reference: manga_translator/detection/ctd.py, ctd_utils/. */

/* u8 pages [B,H,W,3] -> letterboxed fp32 NHWC [B,S,S,4] (rgb/255, 4th channel 0; bottom/right zero pad).
 * Replaces preprocess_img (ctd.py:17-28) + letterbox (ctd_utils/utils/imgproc_utils.py:69-100, cv2.resize
 * INTER_LINEAR + copyMakeBorder).  mode 0: no resize; 1: exact 2x shrink (OpenCV routes it to the 2x2 box
 * mean); 2: OpenCV 11-bit fixed-point bilinear with per-axis DEVICE tables (source index, two coefficients). */
int mit_ctd_prep(const uint8_t *img_dev, int B, int H, int W, int nh, int nw, int S, int mode, const int *yidx_dev,
                 const short *ycoef_dev, const int *xidx_dev, const short *xcoef_dev, float *out_dev, void *stream);

/* NHWC max-pool k x k, stride 1, pad k/2 — nn.MaxPool2d of SPPF (yolov5/common.py:181-197). Pixel strides in floats. */
int mit_maxpool_nhwc(const float *in_dev, int64_t in_pixstride, float *out_dev, int64_t out_pixstride, int B, int H,
                     int W, int C, int k, void *stream);
/* NHWC max-pool k x k, stride s, pad p (implicit -inf padding): torchvision ResNet's MaxPool2d(3, 2, 1)
 * (default detector, default_utils/DBNet_resnet34.py:104).  out [B,Ho,Wo,C] dense. */
int mit_maxpool2d_nhwc(const float *in_dev, float *out_dev, int B, int H, int W, int C, int k, int s, int p, void *stream);
/* NHWC 2x2/2 average pool — nn.AvgPool2d(2, 2) of double_conv_c3 (ctd_utils/basemodel.py:28-39). */
int mit_avgpool2_nhwc(const float *in_dev, int64_t in_pixstride, float *out_dev, int64_t out_pixstride, int B, int Ho,
                      int Wo, int C, void *stream);
/* channel-slice copy between NHWC buffers (torch.cat inputs that need a second home, basemodel.py:62-68,102-103). */
int mit_copy_channels(const float *in_dev, int64_t in_pixstride, float *out_dev, int64_t out_pixstride, int64_t npix,
                      int C, void *stream);
/* fp32 map -> u8. mode 0: (uint8)(v*255) truncation (postprocess_mask ctd.py:30-44); mode 1: v > thr
 * (SegDetectorRepresenter.binarize, ctd_utils/utils/db_utils.py:75); mode 2: (uint8)(clip(v,0,1)*255)
 * (ESRGANUpscalerPytorch._infer, upscaling/esrgan_pytorch.py:545). */
int mit_map_to_u8(const float *in_dev, uint8_t *out_dev, int64_t n, int mode, float thr, void *stream);

/* out = a * x + y over n floats (n % 4 == 0): RRDB.forward's ``out * 0.2 + x`` (upscaling/esrgan_pytorch.py:112). */
int mit_axpy(float *out_dev, float a, const float *x_dev, const float *y_dev, int64_t n, void *stream);

/* Host-side (CPU) detector post-processing: thresholded bitmap -> contours -> min-area boxes -> score -> unclip -> boxes.
 * pred: f32 [H,W] probability map (host), bitmap: u8 [H,W] (pred > thresh, host).  Every contour (outer and hole borders,
 * last-found first, at most max_candidates) yields one slot of boxes_out [n,4,2] (int64 x,y scaled to dest_w x dest_h,
 * rounded, clipped; corner order tl,tr,br,bl, or starting at the smallest x+y when roll_start) and scores_out [n]; skipped
 * contours leave zeros (the callers filter on score / non-zero boxes like the reference).  Replaces
 * SegDetectorRepresenter.boxes_from_bitmap of ctd_utils/utils/db_utils.py:127-171 (min_sside 2, box_thresh 0,
 * min_sside_out 0, roll_start 0, unclip 1.5) and default_utils/dbnet_utils.py:97-144 (min_sside 3, box_thresh, min_sside_out 5,
 * roll_start 1), i.e. cv2.findContours/minAreaRect/boxPoints/fillPoly/mean + pyclipper JT_ROUND offset + shapely area/length.
 * boxes_out / scores_out must hold max_candidates slots. */
int mit_boxes_from_bitmap(const float *pred, const uint8_t *bitmap, int H, int W, int dest_w, int dest_h, int max_candidates,
                          float unclip_ratio, float min_sside, float box_thresh, float min_sside_out, int roll_start,
                          int64_t *boxes_out, float *scores_out, int *n_out);
/* The same chain ON THE GPU for a batch of pages (csrc/ctd_boxes.hip; replaces the per-page host call of
 * SegDetectorRepresenter.boxes_from_bitmap, db_utils.py:127-216 / dbnet_utils.py:97-144): pred_dev f32 [B,H,W] with pred_bs elements
 * between pages (0 = H * W; a channel of an NCHW map is 2 H W apart); the bitmap is bitmap_dev u8 [B,H,W] (non-zero = set, bitmap_bs
 * between pages) or, when bitmap_dev is NULL, pred > thresh.  One union-find labelling of the padded bitmap
 * finds every border's first pixel (outer borders: a foreground component's first pixel; hole borders: the left neighbour of an
 * enclosed background component's first pixel — the pixels Suzuki-Abe's raster scan starts them at), one wave per border walks it and
 * does minAreaRect / score / round-join offset / minAreaRect / scaling.  boxes_dev int64 [B,max_candidates,4,2] and scores_dev f32
 * [B,max_candidates] in OpenCV's list order (last border found first; zeros = skipped, as the reference leaves them); counts_dev i32
 * [B] = borders found (min with max_candidates = slots used); overflow_dev i32 [B] != 0: a border of that page exceeds what a wave
 * holds in LDS (8192 points / 4096 corners) — run mit_boxes_from_bitmap for that page (same results).  Results equal the host
 * routine's (tests/test_ctd_boxes_gpu.py).  workspace_dev: mit_boxes_from_bitmap_dev_workspace_bytes(B, H, W, max_candidates) bytes. */
int64_t mit_boxes_from_bitmap_dev_workspace_bytes(int B, int H, int W, int max_candidates);
/* Development aid: a device buffer of 8 x max_candidates x B int64 in which every border records wall_clock64() (100 MHz) at its phase
 * boundaries (walk, rectangle, score, offset, end; [7] = contour length); NULL switches it off (scripts/bench_boxes.py --stamps). */
int mit_boxes_debug_stamps(void *stamps_dev);
int mit_boxes_from_bitmap_dev(const float *pred_dev, int64_t pred_bs, const uint8_t *bitmap_dev, int64_t bitmap_bs, float thresh, int B, int H, int W, int dest_w, int dest_h,
                              int max_candidates, float unclip_ratio, float min_sside, float box_thresh, float min_sside_out, int roll_start,
                              void *workspace_dev, int64_t workspace_bytes, int64_t *boxes_dev, float *scores_dev, int *counts_dev,
                              int *overflow_dev, void *stream);
/* Minimum distance between the quadrilaterals of index pairs (host code, no GPU): quads [n][4][2] doubles (vertex rings), pairs [m][2]
 * -> out [m]; 0 when the two rings touch, cross or contain one another, else the smallest vertex-to-edge distance.  What shapely's
 * Polygon(a.pts).distance(Polygon(b.pts)) returns in Quadrilateral.can_merge / quadrilateral_can_merge_region (utils/generic.py:660-662),
 * which the OCR direction vote (ocr/common.py:12-39) and the text-line merge graph (textline_merge/__init__.py:112-141) evaluate for
 * every pair of neighbouring lines of a page.  The arithmetic is textline.polygon_distance's, operation for operation (doubles). */
int mit_quad_pair_distances(const double *quads, int n, const int32_t *pairs, int m, double *out);
/* Number of contours / border points cv2.findContours(RETR_LIST) would trace in a 0/1 bitmap (diagnostics, tests). */
int mit_find_contours_count(const uint8_t *bitmap, int H, int W, int *n_contours, int64_t *n_points);

/* Mask refinement, host half ahead of the per-line DenseCRF — complete_mask of mask_refinement/text_mask_utils.py:100-170 (host
 * pointers only; CPU code).  mask: u8 [H,W] at the working scale, MODIFIED like the reference's (every line's bounding box outlined
 * with zeros, cv2.rectangle).  Its 8-connected components (cv2.connectedComponentsWithStats) come back as row runs — runs[r] =
 * {y, x0, x1 (exclusive), comp}, comp = 1..n in raster order of the component's first pixel — and assign[comp] is the text line
 * the component belongs to, or -1 (assign[0] = -1): more than 9 pixels, smaller than the line, and either the line polygon covers
 * more than keep_threshold of min(component pixels, line area) of the component's bounding rectangle (largest such ratio, fp32, first
 * wins) or no line does and the nearest polygon is closer to the rectangle's centre than half of max(min(font size, w, h), 10).
 * polys: f64 [M,V,2] (V = 4 for text lines), boxes_xywh: i32 [M,4] (BBox.xywh), font_size: f64 [M]; line_rects: i32 [M,4] = union
 * (x1, y1, x2, y2) of the bounding rectangles of the line's components, -1 when it has none.  runs_cap <= H * ceil(W / 2) runs and
 * assign_cap <= ceil(H / 2) * ceil(W / 2) + 1 entries always suffice. */
typedef struct MitMaskRun {
    int32_t y, x0, x1, comp;
} MitMaskRun;
int mit_mask_assign_lines(uint8_t *mask, int H, int W, const int32_t *boxes_xywh, const double *polys, const double *font_size, int M, int V,
                          double keep_threshold, MitMaskRun *runs, int64_t runs_cap, int32_t *assign, int64_t assign_cap, int32_t *line_rects,
                          int64_t *n_runs_out, int32_t *n_comp_out);
/* The component image of a line inside a rectangle, for n_jobs (line, x, y, w, h) jobs at once (jobs: i32 [n_jobs,5]): out +
 * offsets[j] receives the u8 [h,w] crop that is 255 on the pixels of the components assigned to the job's line — what the reference
 * reads out of its page-sized per-line images (text_mask_utils.py:145,173). */
int mit_mask_line_crops(const MitMaskRun *runs, int64_t n_runs, const int32_t *assign, const int32_t *jobs, int n_jobs, uint8_t *out,
                        const int64_t *offsets);
/* Mask refinement, the same half on the DEVICE (csrc/mask_assign.hip) for a working-scale mask that already lives there; V must be 4.
 * mask_dev: u8 [H,W], outlined in place like the host routine's.  boxes_xywh_dev / polys_dev / font_size_dev: the host routine's
 * arrays in device memory.  ws_dev: mit_mask_assign_workspace_bytes(H, W) bytes (int32 planes of H*W entries: root label per pixel,
 * area / rectangle / line per root — no cap on the number of components); it holds the labelling for mit_mask_line_crops_dev until
 * the next call.  line_rects_dev: i32 [4*M + 4]: the host routine's line_rects, then a status word {components assigned, components
 * of more than 9 pixels, components, 0}.  Decisions are the host routine's (same double / fp32 expressions, no contraction): equal
 * rectangles, not close ones.  Asynchronous on the stream; no allocation, no synchronisation. */
int64_t mit_mask_assign_workspace_bytes(int H, int W);
int mit_mask_assign_lines_dev(uint8_t *mask_dev, int H, int W, const int32_t *boxes_xywh_dev, const double *polys_dev,
                              const double *font_size_dev, int M, int V, double keep_threshold, void *ws_dev, int64_t ws_bytes,
                              int32_t *line_rects_dev, void *stream);
/* mit_mask_line_crops from the workspace mit_mask_assign_lines_dev left: jobs_dev i32 [n_jobs,5] (line, x, y, w, h), offsets_dev
 * i64 [n_jobs] ascending, total = bytes of all crops; out_dev is the packed crop buffer mit_densecrf_refine reads as mask_dev. */
int mit_mask_line_crops_dev(const void *ws_dev, int64_t ws_bytes, int H, int W, const int32_t *jobs_dev, const int64_t *offsets_dev,
                            int n_jobs, int64_t total, uint8_t *out_dev, void *stream);
/* The --ignore-bubble stage of mask_refinement.dispatch (mask_refinement/__init__.py:31-50, utils/bubble.py:28-84) on the DEVICE
 * (csrc/bubble.hip): mask_dev u8 [H,W] (the refined mask at page size) is dilated by a k x k square (k = int(max(H, W) * 0.025), anchor
 * k / 2, 0 copies), and every external contour of the result — an 8-connected component of the dilated mask with its holes filled — whose
 * page rectangle (its bounding rectangle, one pixel larger to the right and below, clamped) is_ignore() rejects is cleared: when
 * lo <= total - bright <= hi, bright = the elements > 127 of page_dev u8 [H,W,3] inside the rectangle AND inside the 2-pixel frame of
 * the whole page, total = the frame's elements, or when more than 10 of the rectangle's pixels are coloured (sum_c (1000 c - G)^2 >
 * 10^8, G = 299 r + 587 g + 114 b: the reference's float64 rule on every colour).  [lo, hi] is the integer form of the reference's
 * `ignore_bubble <= round(v / total, 6) * 100 <= 100 - ignore_bubble` (mask_refinement.bubble_interval); lo > hi switches that rule off.
 * out_dev u8 [H,W] receives the bytes of mask_refinement.bubble_filter and may be mask_dev.  ws_dev: 4-byte aligned,
 * mit_bubble_filter_workspace_bytes(H, W) bytes (planes of H*W entries: no cap on the number of components); negative for H or W < 4
 * or H * W >= 2^31.  Asynchronous on the stream; no allocation, no synchronisation, no host round trip. */
int64_t mit_bubble_filter_workspace_bytes(int H, int W);
int mit_bubble_filter(const uint8_t *mask_dev, const uint8_t *page_dev, int H, int W, int k, int lo, int hi, uint8_t *out_dev, void *ws_dev,
                      int64_t ws_bytes, void *stream);
/* is_ignore() (utils/bubble.py:28-84) on the lines of a rectified chunk, where the OCR models call it per crop
 * (ocr/model_48px_ctc.py:90, ocr/model_32px.py:84, manga_translator.py:1358): region_dev u8 [n,h,wp,3], lines_dev i32 [n,3] = (w, lo, hi)
 * per line, 2 <= w <= wp.  Line j is rejected when lo <= dark <= hi, dark = the elements <= 127 of the crop's 2-pixel frame counted
 * slice by slice ([0:2, 0:w], [h-2:h, 0:w], [2:h-2, 0:2], [2:h-2, w-2:w]: the last two overlap for w < 4), or when more than 10 of
 * its pixels are coloured (the rule above).  flags_dev u8 [n]: 1 rejected — all h*wp*3 bytes of the line are then set to zero, as the
 * reference's `continue` leaves its row of the chunk —, 0 kept, 2 for a width outside 2..wp (nothing read or written).  Columns >= w
 * are never read.  One workgroup per line; asynchronous on the stream. */
int mit_bubble_crop_flags(uint8_t *region_dev, int n, int h, int wp, const int32_t *lines_dev, uint8_t *flags_dev, void *stream);
/* The page filters of CommonDetector.detect (detection/common.py:18-35) on the DEVICE (csrc/det_filters.hip), for dense pages
 * u8 [B,H,W,3].  The filtered frame is (W, H) when rotated (np.rot90(image, k=-1), :101-102), else (H, W); `side` > 0 adds the zero
 * border of _add_border (:71-79) — the frame at the top left of a side x side square, side >= max(H, W) — and 0 adds none.  The order is
 * the reference's: rotation, border, inversion (cv2.bitwise_not, :115-116), gamma (:118-124), so the border is inverted, counted in the
 * gamma mean and sent through the gamma table like every other pixel.
 * mit_det_filter_gray_sum: sums_dev u64 [B] (8-byte aligned) receives, per page, the sum over the filtered pre-gamma image of the 8-bit
 * gray value cv2.cvtColor(image, COLOR_BGR2GRAY) (:119) in the fixed-point form (c0*1868 + c1*9617 + c2*4899 + 8192) >> 14 — the
 * numerator of np.mean(gray) (:121), exact (integer partial sums and 64-bit atomics: no order dependence).  The rotation does not change
 * it, so there is no rotate argument; a border pixel adds 0, or 255 under `invert`.
 * mit_det_filter_apply: dst_dev u8 [B,fh,fw,3] (not src_dev) receives lut[b][inv(v)] for every byte v of the rotated, bordered page,
 * inv(v) = 255 - v when `invert`; lut_dev u8 [B,256] is the per-page table np.power(...).clip(0, 255).astype(np.uint8) (:123) takes on
 * the 256 byte values (det_filters.gamma_lut), NULL for no gamma.  Rotated: out[i, j] = src[H - 1 - j, i] through a padded LDS tile,
 * reads and writes along image rows; any H and W.
 * Arguments are checked before any HIP call (null pointers, non-positive sizes, a side smaller than the frame).  Asynchronous on the
 * stream; no allocation, no synchronisation. */
int mit_det_filter_gray_sum(const uint8_t *pages_dev, int B, int H, int W, int side, int invert, uint64_t *sums_dev, void *stream);
int mit_det_filter_apply(const uint8_t *src_dev, int B, int H, int W, int rotate, int side, int invert, const uint8_t *lut_dev,
                         uint8_t *dst_dev, void *stream);
/* _remove_border's crop and _remove_rotation's np.rot90 (detection/common.py:84,87,105-107) on u8 maps [B,h,w] in one pass:
 * out_dev u8 [B,cw,ch] (not maps_dev) = np.rot90(m[:ch, :cw]), i.e. out[i, j] = m[j, cw - 1 - i]; ch <= h, cw <= w (a crop outside the
 * map is refused).  The same LDS tile as above.  Asynchronous on the stream. */
int mit_det_unrotate_u8(const uint8_t *maps_dev, int B, int h, int w, int ch, int cw, uint8_t *out_dev, void *stream);
/* merge_mask_list of the ctd detector's refine_mask (detection/ctd_utils/textmask.py:74-132; filter_with_lines False), HOST
 * pointers: n_cands candidate masks [n_cands][h*w] (0 / 255) with their xor scores, the network's mask window pred_mask [h*w];
 * merged [h*w] receives the result.  Candidates in ascending score, their 8-connected components in raster order of the first
 * pixel, each joined when that lowers sum(xor(merged, erode(pred) > 60)); inpaint_dilate != 0 adds the 5x5 dilation
 * (REFINEMASK_INPAINT); then small holes are filled the same way. */
int mit_merge_mask_list(const uint8_t *cands, const int64_t *scores, int n_cands, const uint8_t *pred_mask, int h, int w,
                        int inpaint_dilate, uint8_t *merged);
/* cv2.threshold(..., THRESH_OTSU)'s threshold (getThreshVal_Otsu_8u) for n 256-bin histograms (host arrays): the per-channel
 * Otsu splits of get_otsuthresh_masklist (ctd_utils/textmask.py:44-54) on the histograms mit_ctd_refine_hist returns. */
int mit_otsu_from_hist(const int32_t *hist, int n, int32_t *thresholds);


/* 48px OCR stage -----------------------------------------------------------------------------
 * Reference: manga_translator/ocr/model_48px.py, ocr/xpos_relative_position.py. */

/* XPOS tables, computed once on the host with the reference's own fp32 expressions
 * (xpos_relative_position.py:9-16,54-59): cos_t/sin_t [imax][40] for index i = 0..imax-1;
 * scale_t / iscale_t [2*pmax][40]: row (p + pmax) holds scale**(p/320) and its reciprocal. */
typedef struct MitXposTables {
    const float *cos_t, *sin_t, *scale_t, *iscale_t;
    int32_t imax, pmax;
} MitXposTables;

/* A packed nn.Linear: w [Kp][ldw] (k-major), out = act((x @ w) * scale + bias); scale may be NULL.  w_split: the same matrix as
 * three bf16 planes (mit_gemm_split_pack) for the split-bf16 tiles, or NULL (fp32 MFMA only). */
typedef struct MitLinear {
    const float *w, *scale, *bias;
    int64_t ldw;
    int32_t K, N, Kp, Np;
    const uint16_t *w_split;
} MitLinear;

typedef struct MitOcrDecoderLayer {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
    MitLinear qkv;  /* self_attn q|k|v fused, N = 960; the q columns carry the head_dim**-0.5 scaling */
    MitLinear out;  /* self_attn.out_proj */
    MitLinear q2;   /* multihead_attn.q_proj (scaled) */
    MitLinear out2; /* multihead_attn.out_proj */
    MitLinear ff1, ff2;
} MitOcrDecoderLayer;

typedef struct MitOcr48Decoder {
    MitOcrDecoderLayer layers[5];
    const float *embd; /* [dict][320] */
    MitLinear pred1;   /* + GELU */
    MitLinear pred;    /* tied to embd, N = dict */
    MitLinear color1;  /* 320 -> 64, ReLU */
    MitLinear color_heads; /* 64 -> 10 = fg(3) | bg(3) | fg_ind(2) | bg_ind(2) */
    MitXposTables xpos;
    int32_t dict_size, _pad;
} MitOcr48Decoder;

/* Kernel forms of a beam-search step inside mit_ocr48_decode.  Each is taken where the GEMM mode, the row count R = 5 N (lines x
 * beams) and the packed weights allow; a call can refuse any of them per call (MitOcr48DecodeArgs.forms_off) and reports the ones it
 * took (forms_run).  Nothing in the reference corresponds to them: forms_off exists so that tests and A/B runs can compare a form with
 * the one it replaces, production passes 0.  LN_FUSED, Q2_FUSED and FF2_SPLITK exist inside the ROWS form only, Q2_FUSED inside LN_FUSED
 * only.  All forms give bit-identical results except FF2_SPLITK. */
#define MIT_OCR48_FORM_ROWS 1        /* the few-row step (pgemm_rows): every Linear of a step as one wave per 32 x 32 output block on
                                      * bf16-plane activations, the LayerNorm / attention kernels producing the planes — instead of the
                                      * tiled form that pays off on full batches; a third of the time per Linear at one page.  Needs
                                      * GEMM mode 6 | 9 and R <= MIT_OCR48_ROWS_MAX */
#define MIT_OCR48_FORM_LN_FUSED 2    /* LayerNorm inside the consuming Linear (norm1 / norm2 / norm3 computed by the waves of the
                                      * Linear that reads them) instead of two launches */
#define MIT_OCR48_FORM_Q2_FUSED 4    /* norm2 + q projection inside the cross-attention kernel instead of separate launches; GEMM
                                      * mode 6 and up to 128 lines */
#define MIT_OCR48_FORM_FF2_SPLITK 8  /* K-cut FFN output Linear (<= 640 rows): K = 2048 cut across the four waves of a workgroup and
                                      * summed in a fixed order.  Its sums round differently from the k-sequential chain every other
                                      * form uses, so a page decoded alone differs from the same page inside a group of more than 640
                                      * rows in the last bits of the log-probabilities (tokens equal, probabilities within 1e-4); with
                                      * it off the step is bit for bit the tiled form */
#define MIT_OCR48_FORM_SELF_ROWS 16  /* row-staged self-attention kernel: one workgroup per row stages the row's key history once for
                                      * its four heads (attention_self_kernel) instead of one single-wave workgroup per (head, row)
                                      * (attention_kernel) */
#define MIT_OCR48_ROWS_MAX 2560      /* rows up to which FORM_ROWS is taken (16 pages of 32 lines): measured equal to the 64 x 64
                                      * split tiles there, 2-3.5x faster per Linear at 160 .. 640 rows */

typedef struct MitOcr48DecodeArgs {
    int32_t N, L;               /* text lines; padded encoder-memory length */
    const float *mem_k;         /* [5][N][L][320] cross-attention keys (k_proj + XPOS) per decoder layer */
    const float *mem_v;         /* [5][N][L][320] */
    const int32_t *mem_len;     /* [N] valid memory length (w+3)/4+2 (model_48px.py:684-688) */
    int32_t max_seq_length;     /* T: decode steps (255 in the reference call, :120) */
    int32_t start_tok, end_tok, max_finished, suppress_eos;
    void *workspace;            /* device scratch of mit_ocr48_decode_workspace_bytes() */
    int64_t workspace_bytes;
    int32_t *res_tok;           /* [N][T+1] tokens incl. the start token */
    int32_t *res_len;           /* [N] number of valid tokens in res_tok */
    float *res_prob;            /* [N] exp(sum of log-probs) (:752) */
    int32_t *res_row;           /* [N] beam row whose activation cache feeds the colour heads */
    float *colors;              /* [N*5][T][12] colour-head outputs for every beam row (10 used) */
    float *trace_logits;        /* optional [T][N*5][dict] raw logits (pred(pred1(decoded)), :713); NULL in production */
    int32_t *trace_hist;        /* optional [T][N*5][T+1] beam tokens after each step */
    int32_t steps_run;          /* out: steps executed */
    int32_t forms_off;          /* MIT_OCR48_FORM_* this call must not take; 0 = what ships */
    int32_t forms_run;          /* out: MIT_OCR48_FORM_* at least one step of this call took */
} MitOcr48DecodeArgs;

/* One text line to rectify: cv2.warpPerspective of the page crop [y1:y1+ch, x1:x1+cw] to (dw, dh) with inverse map minv
 * (row-major 3x3, destination -> crop coordinates), then ROTATE_90_COUNTERCLOCKWISE when vertical; the result lands in
 * row out_row of the chunk tensor.  Replaces Quadrilateral.get_transformed_region (utils/generic.py:445-481). */
typedef struct MitWarpLine {
    double minv[9];
    int32_t page, x1, y1, cw, ch, dw, dh, vertical, out_row, _pad;
} MitWarpLine;
/* pages u8 [P,H,W,3] -> chunk u8 [N,Hout,Wp,3], zero beyond each line's width (model_48px.py:83-91: np.zeros + copy).
 * 8-bit bilinear with OpenCV's fixed-point rules (INTER_BITS 5, 15-bit weights), BORDER_CONSTANT 0. */
int mit_ocr_warp_lines(const uint8_t *pages_dev, int H, int W, const MitWarpLine *lines_dev, int n_lines, uint8_t *out_dev,
                       int Hout, int Wp, void *stream);
int mit_ocr_prep(const uint8_t *lines_dev, float *out_dev, int N, int H, int Wp, void *stream);
/* The same for the chunks of a page group in ONE launch, over a device table in the manner of MitRaggedSeg: segment s converts the
 * N * H * Wp pixels at src to the output slab from pixel pixel_start on; block_start = running count of MIT_OCR_PREP_BLOCK-pixel work
 * items = sum over earlier segments of ceil(N * H * Wp / MIT_OCR_PREP_BLOCK), total_blocks = that sum over all (the grid).  Per pixel
 * the expression of mit_ocr_prep: same bits. */
#define MIT_OCR_PREP_BLOCK 1024
typedef struct MitOcrPrepSeg {
    const uint8_t *src;
    int64_t pixel_start, block_start;
    int32_t N, Wp;
} MitOcrPrepSeg;
int mit_ocr_prep_ragged(const MitOcrPrepSeg *segs_dev, int nsegs, int64_t total_blocks, float *out_dev, int H, void *stream);
/* depthwise k x k conv + per-channel scale/bias (ConvNeXtBlock.dwconv + norm, model_48px.py:195-196,205-206). w [k*k][C]. */
int mit_dwconv_nhwc(const float *in_dev, const float *w_dev, const float *scale_dev, const float *bias_dev, float *out_dev,
                    int B, int H, int W, int C, int k, void *stream);
/* Ragged variant: nsegs images [B_s,H_s,W_s,C] stored back to back along the pixel axis (the OCR chunks of a page group,
 * whose padded widths differ, model_48px.py:83-86).  Segment s starts at pixel pixel_start; group_start = running count of
 * (image row, 4-column group) work items = sum over earlier segments of B*H*ceil(W/4); total_groups = that sum over all. */
typedef struct MitRaggedSeg {
    int64_t pixel_start, group_start;
    int32_t B, H, W, _pad;
} MitRaggedSeg;
int mit_dwconv_nhwc_ragged(const float *in_dev, const float *w_dev, const float *scale_dev, const float *bias_dev,
                           float *out_dev, const MitRaggedSeg *segs_dev, int nsegs, int64_t total_groups, int C, int k,
                           void *stream);
/* The same when every segment has height common_H: rows are processed YT = 4 (or 2) at a time per thread with the weights in LDS
 * (bit-identical results, about a third of the L1 loads).  common_H <= 0, odd heights or K*K*C*4 > 64 KB fall back to the call above. */
int mit_dwconv_nhwc_ragged_rows(const float *in_dev, const float *w_dev, const float *scale_dev, const float *bias_dev,
                                float *out_dev, const MitRaggedSeg *segs_dev, int nsegs, int64_t total_groups, int C, int k,
                                int common_H, void *stream);
/* nn.LayerNorm over the last dim (transformer norm1/2/3). */
int mit_layernorm(const float *in_dev, int64_t in_rowstride, const float *w_dev, const float *b_dev, float *out_dev,
                  int64_t out_rowstride, int rows, int D, float eps, void *stream);
/* XPOS.forward on [R, T, 4*80] (row / time strides in floats): index i0+t, centred position p0+t. */
int mit_xpos_rotate(const float *in_dev, int64_t in_rs, int64_t in_ts, float *out_dev, int64_t out_rs, int64_t out_ts, int R,
                    int T, int i0, int p0, int downscale, const MitXposTables *tables, void *stream);
/* softmax(q k^T + key-padding mask) v for 4 heads x 80 (XposMultiheadAttention.forward :369-384); q already scaled and
 * rotated, k rotated.  Row r reads keys/values of row r / kv_div; klen_dev (optional) = valid keys per kv row. */
int mit_attention(const float *q_dev, int64_t q_rs, int64_t q_ts, const float *k_dev, int64_t k_rs, int64_t k_ts,
                  const float *v_dev, int64_t v_rs, int64_t v_ts, float *out_dev, int64_t o_rs, int64_t o_ts,
                  const int *klen_dev, int R, int Tq, int Tk, int kv_div, void *stream);
/* The encoder's self-attention (XposMultiheadAttention.forward, ocr/model_48px.py:327-394) for ALL lines of a page group in one launch
 * with the XPOS rotation of q (scale) and k (inverse scale) folded in (xpos_relative_position.py:44-71): line r owns lines[r] = {first row,
 * L_r} rows of the flat [rows, heads * head_dim] q / k / v / out tensors (row stride in floats), L_r = its chunk's memory length = its
 * query and key count, positions centred per chunk (p0 = -((L_r + 1) / 2)), klen[r] valid keys.  Bitwise equal to mit_xpos_rotate (q),
 * mit_xpos_rotate (k, downscale) and mit_attention chunk by chunk.  Lmax = the longest line (LDS sizing). */
int mit_attention_lines_xpos(const float *q_dev, const float *k_dev, const float *v_dev, float *out_dev, int64_t row_stride,
                             const int32_t *lines_dev, const int *klen_dev, int n_lines, int Lmax, int heads, int head_dim,
                             const MitXposTables *tables, void *stream);
/* Longest line (Lmax) whose keys + per-wave score rows fit mit_attention_lines_xpos's LDS form for this head_dim (308 at head_dim 80);
 * longer lines take the chunk-by-chunk path (mit_xpos_rotate + mit_attention), which has no such limit.  0 for an unsupported head_dim. */
int mit_attention_lines_xpos_max_len(int head_dim);
/* Cross-attention memory of one decoder layer for the same lines: mem_k[first_line + r][t][:] = the XPOS-rotated (inverse scale) k rows,
 * mem_v[...] = the v rows, t < L_r (line_stride floats between lines of the pooled [n, Lmax, heads * head_dim] memory); n_rows = the
 * rows the lines cover.  Replaces one mit_xpos_rotate and one copy per chunk (OCR.infer_beam_batch_tensor's memory, :678-704). */
int mit_memory_kv_lines(const float *k_dev, const float *v_dev, int64_t row_stride, float *mem_k_dev, float *mem_v_dev, int64_t line_stride,
                        const int32_t *lines_dev, int n_lines, int first_line, int64_t n_rows, int Lmax, int head_dim,
                        const MitXposTables *tables, void *stream);
/* Same with an explicit head layout (heads x head_dim contiguous in the feature axis): 8 x 40 for the 48px_ctc encoder's
 * nn.MultiheadAttention (model_48px_ctc.py:216-217,259-265; q already scaled by head_dim**-0.5, PE already added to q/k). */
int mit_attention_heads(const float *q_dev, int64_t q_rs, int64_t q_ts, const float *k_dev, int64_t k_rs, int64_t k_ts,
                        const float *v_dev, int64_t v_rs, int64_t v_ts, float *out_dev, int64_t o_rs, int64_t o_ts,
                        const int *klen_dev, int R, int Tq, int Tk, int kv_div, int heads, int head_dim, void *stream);
/* nn.AvgPool2d(kernel, stride, padding) with count_include_pad=True on NHWC fp32 — the FAN backbone's pools
 * (model_48px_ctc.py:291,297,303: 2/2/0 twice, then kernel 2, stride (2,1), padding (0,1)). out [B,Ho,Wo,C] dense. */
int mit_avgpool_nhwc(const float *in_dev, float *out_dev, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph,
                     int pw, void *stream);
/* y = relu?(x * scale[c] + bias[c]) per pixel: eval BatchNorm2d (+ ReLU) that cannot ride in a conv epilogue because its
 * input also feeds a residual (pre-activation BasicBlock.forward, model_48px_ctc.py:389-403). */
int mit_affine_act_nhwc(const float *in_dev, int64_t in_pixstride, const float *scale_dev, const float *bias_dev, float *out_dev,
                        int64_t out_pixstride, int64_t npix, int C, int relu, void *stream);
/* u8 RGB [npix,3] -> fp32 [npix,4] (4th channel 0).  mode 0: (x-127.5)/127.5 (model_48px.py:115); mode 1: x/127.5 - 1
 * (det_batch_forward_default, detection/default.py:19); mode 2: x/255.  Each is the reference's own fp32 expression. */
int mit_u8_to_f32_nhwc4(const uint8_t *in_dev, float *out_dev, int64_t npix, int mode, void *stream);
/* x <- sigmoid(x): the ``db.sigmoid()`` that det_batch_forward_default applies on top of DBHead's output (default.py:23). */
int mit_sigmoid_inplace(float *x_dev, int64_t n, void *stream);
/* x <- gelu(x) (erf form) over n floats: the nn.GELU of char_pred_norm (model_48px_ctc.py:435). */
int mit_gelu_inplace(float *x_dev, int64_t n, void *stream);
/* log_softmax over D columns + the 5 largest (value, index) per row, ties to the lower index; suppress_tok < 0: none.
 * Row r: vals_dev[5r..], idx_dev[5r..].  decode_ctc_top1's log_softmax + max (model_48px_ctc.py:477-478) uses entry 0.
 * loop_form 0: a thread's elements loaded once and every pass on registers where D allows (what every model runs); non-zero: the
 * three-pass loop form for every D — bit for bit the same values and indices (tests/test_ocr_gpu.py compares the two). */
int mit_logsoftmax_top5(const float *logits_dev, int64_t ld, int R, int D, int suppress_tok, float *vals_dev, int *idx_dev,
                        int loop_form, void *stream);
/* The whole beam search of OCR.infer_beam_batch_tensor (:691-784) after the encoder, as one native call: per step
 * embedding -> 5 decoder layers (KV cache instead of the reference's per-step K/V recomputation) -> pred1/pred ->
 * log-softmax/top-5 -> beam bookkeeping, all on `stream`; synchronises the stream every few steps to test for early exit. */
int64_t mit_ocr48_decode_workspace_bytes(int N, int T, int dict_size);
int mit_ocr48_decode(const MitOcr48Decoder *dec, MitOcr48DecodeArgs *args, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * 32px OCR (``--ocr 32px``): reference manga_translator/ocr/model_32px.py.  Backbone and encoder run on the entry points above
 * (FAN ResNet [3, 6, 7, 5] :143-234, 3 x post-norm nn.TransformerEncoderLayer :474-476); the decoder is the call below. */

/* OCR(dictionary, 768)'s decoder side (:467-489): 2 x nn.TransformerDecoderLayer(320, 4) (post-norm, FFN 2048, ReLU), embedding,
 * sinusoidal table pe.pe, pred1 (+ ReLU), pred (weight tied to embd), color_pred1 (+ ReLU) and the six 64 -> 1 colour heads packed as
 * one 64 -> 6 Linear in the order fg_r, fg_g, fg_b, bg_r, bg_g, bg_b (:484-489). */
typedef struct MitOcr32Decoder {
    MitOcrDecoderLayer layers[2];
    const float *embd;     /* [dict][320] */
    const float *pe;       /* [pe_len][320]: PositionalEncoding.pe (:289-300) */
    MitLinear pred1;       /* 320 -> 320, ReLU */
    MitLinear pred;        /* 320 -> dict */
    MitLinear color1;      /* 320 -> 64, ReLU */
    MitLinear color_heads; /* 64 -> 6 */
    int32_t dict_size, pe_len;
} MitOcr32Decoder;

typedef struct MitOcr32DecodeArgs {
    int32_t N, L;               /* text lines; padded encoder-memory length */
    const float *mem_k;         /* [2][N][L][320] cross-attention keys of the memory per decoder layer (multihead_attn's k projection) */
    const float *mem_v;         /* [2][N][L][320] */
    const int32_t *mem_len;     /* [N] valid memory length (w + 3) / 4 + 2 (:523); keys beyond it are masked */
    int32_t max_seq_length;     /* T: iterations of the beam loop after the first step (255 in the reference call, :100) */
    int32_t start_tok, end_tok; /* 1, 2 (:518) */
    int32_t max_finished;       /* max_finished_hypos (2, :518); 1 or 2 */
    void *workspace;            /* device scratch of mit_ocr32_decode_workspace_bytes() */
    int64_t workspace_bytes;
    int32_t *res_tok;           /* [N][T+2] tokens incl. the start token, 0 beyond res_len */
    int32_t *res_len;           /* [N] number of valid tokens in res_tok */
    float *res_prob;            /* [N] exp(mean(out_logprobs)), the start token's 0.0 included (:398-399) */
    float *colors;              /* [N][T+1][8]: the six colour heads over the chosen hypothesis's output history (res_len - 1 positions) */
    int32_t *res_src;           /* optional [N][T+1]: beam row that holds position t of the chosen hypothesis's history, -1 beyond it */
    float *trace_logits;        /* optional [T+1][N*5][dict] raw logits per step (pred(pred1(decoded)), :533,:546); NULL in production */
    int32_t *trace_hist;        /* optional [T+1][N*5][T+2] kept hypotheses after each step (rows of done lines are stale) */
    int32_t steps_run;          /* out: network evaluations executed (first step included) */
    int32_t form;               /* 0: the few-row form of a step (every Linear on bf16-plane activations, one wave per 32 x 32 block) where
                                 * the GEMM mode (6 | 9) and the row count allow, else the tiled form; 1: always the tiled form.  Same
                                 * arithmetic except the FFN output Linear's K cut across four waves (few rows): tokens equal, the
                                 * probabilities in their last bits (tests/test_ocr32_gpu.py) */
} MitOcr32DecodeArgs;

/* The whole beam search of OCR.infer_beam_batch (:518-595) after the encoder as one native call: per step embedding + pe[len] ->
 * 2 post-norm decoder layers (per-layer K / V history that follows the beam's parent links, instead of next_token_batch's
 * re-projection of the whole history, :444-451) -> pred1 / pred -> log-softmax / top-5 -> Hypothesis bookkeeping (:549-572), the final
 * pick (:576-585) and the colour heads (:586-593).  Lines keep their five rows in place after they are done.  Synchronises the stream
 * every four steps to test for the early exit (:573-574). */
int64_t mit_ocr32_decode_workspace_bytes(int N, int T, int dict_size);
int mit_ocr32_decode(const MitOcr32Decoder *dec, MitOcr32DecodeArgs *args, void *stream);
/* The bookkeeping kernels of mit_ocr32_decode alone, fed with given top-5 tables vals_dev / idx_dev [steps][N*5][5] (log-probabilities
 * descending and their tokens; step 0 reads row 5 n of line n) instead of a network: fills res_tok / res_len / res_prob / res_src and
 * trace_hist ([steps][N*5][T+2]) of args (N, max_seq_length, start_tok, end_tok, max_finished, workspace as for the decode). */
int mit_ocr32_beam_replay(const float *vals_dev, const int32_t *idx_dev, int steps, MitOcr32DecodeArgs *args, void *stream);

/* ESRGAN dense blocks on bf16-resident activations (additive in ABI 25) ------------------------------------------------------------
 * mit_rdb_conv3x3_bf16 — the 3x3, stride 1, zero-pad 1 convolution of ResidualDenseBlock_5C (upscaling/esrgan_pytorch.py:152-166) for
 * the upscaler's bf16 precision, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The dense block lives in one bf16 NHWC buffer
 * [B,H,W,ld] = [x | x1 | x2 | x3 | x4]; a launch reads its first Cin channels and may write its N results into a later channel slice of
 * the SAME buffer.  A workgroup owns MIT_RDB_TILE_H x MIT_RDB_TILE_W output pixels: per chunk of 32 input channels it stages the tile
 * plus its one-pixel halo (zeros outside the image) and the chunk's 9 x 32 weight rows to LDS once and serves all nine taps from
 * there; nothing is rounded or split in the kernel on the way to the MFMA.
 *
 *   acc[n]  = sum_{tap = (ky, kx)} sum_{c < Cin} in[b, y + ky - 1, x + kx - 1, c] * w[(tap * Cin + c) * N + n]        (fp32, exact products)
 *   v       = acc * scale[n] + bias[n]                  scale NULL = 1, bias NULL = 0; two rounded operations, no FMA
 *   v       = act == MIT_ACT_LEAKY ? (v >= 0 ? v : v * act_alpha) : v
 *   v       = v + post[b, y, x, n]                      when post  != NULL
 *   v       = v * s2 + post2[b, y, x, n]                when post2 != NULL   (the RRDB's outer x * 0.2 + rrdb_in, :139-148)
 *   out_f32[b, y, x, n] = v                             when out_f32  != NULL
 *   out_bf16[b, y, x, n] = bf16(v)                      when out_bf16 != NULL: round to nearest even of the fp32 value, the bits of
 *                                                       torch.Tensor.to(torch.bfloat16)
 * A pixel's result depends on nothing but its own 3 x 3 x Cin window: not on B, the tile it falls in or the launch's other images.
 *
 * Requirements (anything else is refused before any HIP call): Cin % 32 == 0 and 64 <= Cin <= 192; N 32 or 64; act NONE or LEAKY;
 * at least one output; B, H, W > 0; every x stride >= the channels addressed through it, y stride >= x stride, batch stride >= 0;
 * in, w 16-byte aligned and the input strides multiples of 8 elements (16-byte loads); one image of every tensor spans fewer than
 * 2^31 elements (image bases are 64-bit, offsets inside an image 32-bit); ceil(H / MIT_RDB_TILE_H) and B <= 65535 (grid y / z);
 * out_bf16 must not overlap the Cin input channels (same strides: disjoint channel ranges; other strides: disjoint extents).
 * All strides are element counts of the tensor's own type. */
#define MIT_RDB_TILE_H 8
#define MIT_RDB_TILE_W 32
typedef struct MitRdbConv {
    const uint16_t *in;               /* bf16 bits, NHWC */
    int64_t in_bs, in_ys, in_xs;
    int32_t B, H, W, Cin;
    const uint16_t *w;                /* [9 * Cin][N] bf16 bits, k = (ky * 3 + kx) * Cin + c */
    int32_t N;
    int32_t act;
    float act_alpha;
    float s2;
    const float *scale, *bias;        /* [N] */
    const float *post;
    int64_t post_bs, post_ys, post_xs;
    const float *post2;
    int64_t post2_bs, post2_ys, post2_xs;
    float *out_f32;
    int64_t of_bs, of_ys, of_xs;
    uint16_t *out_bf16;
    int64_t ob_bs, ob_ys, ob_xs;
} MitRdbConv;
int mit_rdb_conv3x3_bf16(const MitRdbConv *d, void *stream);
/* dst[b, y, x, c] = bf16(src[b, y, x, c]) for c < Cn: an NHWC channel-slice cast, fp32 -> bf16 bits, round to nearest even (the bits of
 * torch.Tensor.to(torch.bfloat16)); element strides, x stride >= Cn, y stride >= x stride, batch stride >= 0.  Puts ``fea`` into the
 * first 64 channels of the dense-block buffer.  Four channels a lane where every stride and base allows (16-byte loads, 8-byte
 * stores), else one. */
int mit_cast_f32_bf16(const float *src_dev, int64_t s_bs, int64_t s_ys, int64_t s_xs, uint16_t *dst_dev, int64_t d_bs, int64_t d_ys,
                      int64_t d_xs, int B, int H, int W, int Cn, void *stream);

/* AOT blocks on bf16-resident convolution operands (additive in ABI 26) -------------------------------------------------------------
 * mit_aot_conv3x3_bf16 — the 3x3, stride 1 convolutions of an AOTBlock (inpainting/inpainting_aot.py:170-193) for the AOT inpainter's
 * bf16 precision: dilation r in 1 .. MIT_AOT_MAX_RATE with ReflectionPad2d(r), on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
 * One launch runs 1 .. MIT_AOT_MAX_GROUPS convolutions ("groups") of the SAME input that differ in rate, weight, bias and the channel
 * offset of their N-column slice in the output(s): the four dilated branches of a block are one launch that fills the 128-channel
 * concatenation; fuse and gate are launches of one group.  A workgroup owns MIT_AOT_TILE_H x MIT_AOT_TILE_W output pixels of one
 * (image, group).  Per 32-channel chunk the chunk's 9 x 32 weight rows go to LDS; the activations take one of two forms, chosen per
 * group by its rate alone: staged — the reflected region the nine windows touch goes to LDS once and serves all taps (regions of up to
 * 640 pixels: rates 1 .. 4) — or direct — a lane loads its A fragments (8 channels of one reflected tap pixel, 16 contiguous bytes)
 * straight from the input (larger rates, whose nine windows do not overlap).  Both forms add the same products in the same order:
 * the same bits.  Nothing is rounded or split on the way to the MFMA.
 *
 *   refl(p, L) = p < 0 ? -p : (p >= L ? 2 (L - 1) - p : p)
 *   acc[n] = sum_{tap = (ky, kx)} sum_{c < Cin} in[b, refl(y + (ky - 1) r, H), refl(x + (kx - 1) r, W), c] * w[g][(tap * Cin + c) * N + n]
 *            (fp32, exact products; order: 32-channel chunk, tap, channel — the same for every pixel, batch and grid)
 *   v      = acc + bias[g][n]                               bias[g] NULL = 0
 *   v      = act == MIT_ACT_RELU ? max(v, 0) : v
 *   out_f32[b, y, x, out_c0[g] + n]  = v                    when out_f32  != NULL
 *   out_bf16[b, y, x, out_c0[g] + n] = bf16(v)              when out_bf16 != NULL: round to nearest even of the fp32 value
 * A pixel's result depends on nothing but its own window: not on B, the tile it falls in, the other groups or the other images.
 *
 * Requirements (anything else is refused before any HIP call): 1 <= groups <= MIT_AOT_MAX_GROUPS; Cin % 32 == 0, 32 <= Cin <= 512;
 * N 32 or 128; act NONE or RELU; at least one output; every used w[g] non-NULL; 1 <= rate[g] <= MIT_AOT_MAX_RATE and rate[g] < H, W;
 * B, H, W > 0; input x stride >= Cin; out_c0[g] >= 0 and out_c0[g] + N <= the x stride of every output (a slice stays inside its pixel),
 * the slices of two groups disjoint; y stride >= x stride, batch stride >= 0; in and every w[g] 16-byte aligned and the input strides
 * multiples of 8 elements; one image of every tensor spans fewer than 2^31 elements (image bases are 64-bit); ceil(H / MIT_AOT_TILE_H)
 * and B * groups <= 65535 (grid y / z); out_bf16 must not overlap the input.  All strides are element counts of the tensor's own type. */
#define MIT_AOT_TILE_H 8
#define MIT_AOT_TILE_W 32
#define MIT_AOT_MAX_GROUPS 4
#define MIT_AOT_MAX_RATE 16
typedef struct MitAotConv {
    const uint16_t *in;               /* bf16 bits, NHWC */
    int64_t in_bs, in_ys, in_xs;
    int32_t B, H, W, Cin;
    int32_t N;                        /* columns of every group */
    int32_t act;
    int32_t groups;
    int32_t rate[MIT_AOT_MAX_GROUPS];
    int32_t out_c0[MIT_AOT_MAX_GROUPS];
    const uint16_t *w[MIT_AOT_MAX_GROUPS];     /* [9 * Cin][N] bf16 bits, k = (ky * 3 + kx) * Cin + c */
    const float *bias[MIT_AOT_MAX_GROUPS];     /* [N] */
    float *out_f32;
    int64_t of_bs, of_ys, of_xs;
    uint16_t *out_bf16;
    int64_t ob_bs, ob_ys, ob_xs;
} MitAotConv;
int mit_aot_conv3x3_bf16(const MitAotConv *d, void *stream);

/* Plain 3x3 convolution on bf16-resident activations (additive in ABI 26) ------------------------------------------------------------
 * mit_conv3x3_bf16 — a 3x3, stride 1, zero-pad 1 convolution of a bf16 NHWC input with per-channel scale / bias (a folded eval
 * BatchNorm) and ReLU / LeakyReLU, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: the layers of FFDNet (96 features) for the mc2
 * colorizer's bf16 precision, whose activations live in HBM as bf16 between the layers.  A workgroup owns MIT_CONV3X3_TILE_H x
 * MIT_CONV3X3_TILE_W output pixels and all N columns: per chunk of 32 input channels it stages the tile plus its one-pixel halo (zeros
 * outside the image) and the chunk's 9 x 32 weight rows to LDS once and serves all nine taps from there; nothing is rounded or split in
 * the kernel on the way to the MFMA.  N = 96 takes 83 KB of LDS (one workgroup a CU; N = 32 | 64 fit two): the same 96 columns as
 * two launches of 64 + 32 columns into channel slices of the output give the same bits.
 *
 *   acc[n]  = sum_{tap = (ky, kx)} sum_{c < Cin} in[b, y + ky - 1, x + kx - 1, c] * w[(tap * Cin + c) * N + n]
 *             (fp32, exact products; order: 32-channel chunk, tap, channel — the same for every pixel, batch and grid)
 *   v       = acc * scale[n] + bias[n]                  scale NULL = 1, bias NULL = 0; two rounded operations, no FMA
 *   v       = act == MIT_ACT_RELU ? max(v, 0) : act == MIT_ACT_LEAKY ? (v >= 0 ? v : v * act_alpha) : v
 *   out_f32[b, y, x, n]  = v                            when out_f32  != NULL
 *   out_bf16[b, y, x, n] = bf16(v)                      when out_bf16 != NULL: round to nearest even of the fp32 value, the bits of
 *                                                       torch.Tensor.to(torch.bfloat16)
 * A pixel's result depends on nothing but its own 3 x 3 x Cin window: not on B, the tile it falls in or the launch's other images.
 *
 * Requirements (anything else is refused before any HIP call): Cin % 32 == 0 and 32 <= Cin <= 192; N 32, 64 or 96; act NONE, RELU or
 * LEAKY; at least one output; B, H, W > 0; every x stride >= the channels addressed through it, y stride >= x stride, batch stride
 * >= 0; in, w 16-byte aligned and the input strides multiples of 8 elements (16-byte loads); one image of every tensor spans fewer
 * than 2^31 elements (image bases are 64-bit, offsets inside an image 32-bit); ceil(H / MIT_CONV3X3_TILE_H) and B <= 65535 (grid y /
 * z); out_bf16 must not overlap the Cin input channels (same strides: disjoint channel ranges; other strides: disjoint extents).
 * All strides are element counts of the tensor's own type. */
#define MIT_CONV3X3_TILE_H 8
#define MIT_CONV3X3_TILE_W 32
typedef struct MitConv3x3Bf16 {
    const uint16_t *in;               /* bf16 bits, NHWC */
    int64_t in_bs, in_ys, in_xs;
    int32_t B, H, W, Cin;
    const uint16_t *w;                /* [9 * Cin][N] bf16 bits, k = (ky * 3 + kx) * Cin + c */
    int32_t N;
    int32_t act;
    float act_alpha;
    const float *scale, *bias;        /* [N] */
    float *out_f32;
    int64_t of_bs, of_ys, of_xs;
    uint16_t *out_bf16;
    int64_t ob_bs, ob_ys, ob_xs;
} MitConv3x3Bf16;
int mit_conv3x3_bf16(const MitConv3x3Bf16 *d, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * manga-ocr recogniser (``--ocr mocr``, additive in ABI 26): reference manga_translator/ocr/model_manga_ocr.py:132-295, whose text comes
 * from a HuggingFace VisionEncoderDecoderModel (ViT / DeiT encoder, BERT decoder with cross-attention) driven by ``generate``.  The
 * encoder runs on the Linear / attention entry points above plus the three below; the whole of ``generate`` after the encoder is
 * mit_mocr_decode.  Every size comes from the model's config: nothing here is fixed to a checkpoint. */

/* nn.LayerNorm over the last dim for any D in 1 .. 8192 (mit_layernorm stops at 512): one wave per row, mean then centred variance. */
int mit_layernorm_wide(const float *in_dev, int64_t in_rowstride, const float *w_dev, const float *b_dev, float *out_dev,
                       int64_t out_rowstride, int rows, int D, float eps, void *stream);
/* Pillow's Image.convert("L").convert("RGB") on u8 RGB pixels: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in all three channels. */
int mit_mocr_gray(const uint8_t *rgb_dev, int64_t npix, uint8_t *out_dev, void *stream);
/* u8 RGB images [N][S][S][3] -> the ViT patch rows fp32 [N][(S / ps)^2][3 ps ps], column = (c, py, px) as the axes of the patch
 * projection's weight, value = (u8 * (1 / 255) - 0.5) / 0.5 in fp32 (ViTImageProcessor: rescale, then normalize).  S % ps == 0. */
int mit_mocr_patches(const uint8_t *img_dev, int N, int S, int ps, float *out_dev, void *stream);

/* One post-LN BertLayer with cross-attention: q = attention.self.query scaled by head_dim**-0.5, kv = attention.self key|value fused
 * (their rows go straight into the K / V history), out = attention.output.dense, ln1 = attention.output.LayerNorm, q2 (scaled) / out2 /
 * ln2 = crossattention, ff1 = intermediate.dense (+ erf GELU), ff2 = output.dense, ln3 = output.LayerNorm. */
typedef struct MitMocrLayer {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
    MitLinear q, kv, out, q2, out2, ff1, ff2;
} MitMocrLayer;

typedef struct MitMocrDecoder {
    const MitMocrLayer *layers;       /* HOST array [n_layers] */
    int32_t n_layers, hidden, heads, inter, vocab, max_pos;
    const float *word_emb, *pos_emb, *type_emb; /* [vocab][hidden], [max_pos][hidden], [hidden] (token type 0) */
    const float *emb_ln_w, *emb_ln_b;
    MitLinear head_dense;              /* cls.predictions.transform.dense (+ erf GELU) */
    const float *head_ln_w, *head_ln_b;
    MitLinear head_out;                /* cls.predictions.decoder: hidden -> vocab, with its bias */
    float ln_eps;
    int32_t _pad;
} MitMocrDecoder;

typedef struct MitMocrDecodeArgs {
    int32_t N, L;                 /* text lines; encoder tokens per line */
    const float *mem_k, *mem_v;   /* [n_layers][N][L][hidden] cross-attention keys / values, projected once per line */
    int32_t num_beams;            /* 1 (greedy) .. 8 */
    int32_t max_length;           /* tokens of a result, decoder_start_token_id included */
    int32_t no_repeat_ngram_size; /* 0: off */
    int32_t early_stopping;       /* 0 | 1 (GenerationConfig.early_stopping False | True) */
    int32_t eos_token_id, pad_token_id, decoder_start_token_id;
    int32_t form;                 /* 0: the few-row form of a step where the GEMM mode (6 | 9) and the packed weights allow; 1: tiled */
    double length_penalty;
    void *workspace;              /* device scratch of mit_mocr_decode_workspace_bytes() */
    int64_t workspace_bytes;
    int32_t *res_tok;             /* [N][max_length], pad_token_id beyond res_len */
    int32_t *res_len;             /* [N] */
    float *res_score;             /* [N] sum of log-probabilities / generated length ** length_penalty (sequences_scores) */
    float *trace_logits;          /* optional [max_length - 1][N * num_beams][vocab]: log-probabilities after the logits processors */
    int32_t *trace_hist;          /* optional [max_length - 1][N * num_beams][max_length]: running beams after each step */
    int32_t steps_run;            /* out */
    int32_t form_run;             /* out: 0 every Linear of a step ran on the tiled GEMM; 1 on the few-row form except the vocabulary Linear
                                   * (vocab % 8 != 0); 2 on the few-row form throughout */
} MitMocrDecodeArgs;

/* HuggingFace beam search (transformers generation/utils.py, _beam_search; num_beams == 1: greedy) as one native call: per step
 * embeddings + LayerNorm -> the decoder layers (self-attention over a K / V history that follows the beams' parent links,
 * cross-attention over mem_k / mem_v) -> LM head -> log-softmax -> no-repeat-n-gram ban -> top 2 num_beams over beams x vocab ->
 * running / finished beam bookkeeping.  A line that can no longer change keeps its rows in place and is not touched again.
 * The workspace holds the K / V history [n_layers][2][N * num_beams][max_length][hidden] in fp32 (the bulk of it): callers with many
 * lines decode them in chunks (results do not depend on what else is in the call).
 * Synchronises the stream every four steps to test for the early exit. */
int64_t mit_mocr_decode_workspace_bytes(int N, int num_beams, int max_length, int hidden, int inter, int vocab, int n_layers);
int mit_mocr_decode(const MitMocrDecoder *dec, MitMocrDecodeArgs *args, void *stream);
/* The bookkeeping kernels alone on given log-probability tables logp_dev [steps][N * num_beams][vocab] (before the n-gram ban): fills
 * res_tok / res_len / res_score and trace_hist of args.  The workspace is sized with hidden = inter = n_layers = 0. */
int mit_mocr_beam_replay(const float *logp_dev, int steps, int vocab, MitMocrDecodeArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIT_HIP_H */
