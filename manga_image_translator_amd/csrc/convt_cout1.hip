// convt_cout1.hip — ConvTranspose2d(Cin -> 1, stride 2) in one pass over the input, over a given output extent only (mit_convt_cout1).
//
// The ctd detector ends in three such layers (ctd_utils/basemodel.py:20 `upconv6` 64 -> 1 k4 s2 p1, :93,96 the DB branches' last
// 16 -> 1 k2 s2).  As four parity launches of conv_gemv_kernel each of them walked its whole input four times, letterbox padding
// included.  Here every input line is fetched once: a lane group owns a CELL of the input and produces the 2 x 2 output pixels that
// depend on it, for all four parities, and rows / columns at or beyond (out_h, out_w) are neither computed nor written.
//
// Cells.  k2 s2 p0: cell (i, j) is input pixel (i, j); its outputs are Y = 2i + a, X = 2j + b (a, b in {0, 1}), one tap each:
// w[c][a][b].  k4 s2 p1: cell (i, j), i in [-1, Hi), is the input neighbourhood rows {i, i + 1} x columns {j, j + 1}; its outputs
// are Y = 2i + 1 + a, X = 2j + 1 + b — exactly the four output pixels whose 2 x 2 taps all fall on that neighbourhood.
//
// Bit identity with the four-launch form (conv_gemv_kernel, csrc/conv_gemm_kernels.h) — what each output pixel computes:
//   * LPR lanes (16 at Cin = 64, 4 at Cin = 16) share a pixel; lane `sub` of the group owns channel quad q = sub, as there.
//   * A lane's partial sum is ONE fmaf chain from 0 over the taps in the order ops.ConvTranspose2d builds for the pixel's parity
//     (ky ascending within the parity's rows, then kx), .x .y .z .w inside a tap.  For k4 s2 p1 that order is the same for all four
//     parities in cell terms: (row i + 1, col j + 1), (i + 1, j), (i, j + 1), (i, j) with ky = a (row i + 1) or a + 2 (row i) and
//     kx = b (col j + 1) or b + 2 (col j):  py = 1 (a = 0): kys = [0, 2] -> dy = +1, 0;  py = 0 (a = 1): kys = [1, 3] -> dy = 0, -1
//     seen from oy = i + 1.  A tap outside the image contributes fmaf(0, w, acc); it is not skipped.
//   * The partial sums meet in the same xor butterfly, o = LPR / 2 ... 1: acc += shfl_xor(acc, o).
//   * Epilogue: v * (scale ? scale[0] : 1) + (bias ? bias[0] : 0), then mitcg::apply_act — the gemv kernel's expression sequence
//     (fp contraction is off in the build).
//
// Schedule.  A workgroup of four waves owns a strip of 256 / LPR cell columns (16 at k4, 64 at k2: MIT_CONVT_COUT1_STRIP_*) and ROWS
// cell rows, walks the rows downwards and keeps the previous input row in registers (k4), so a wave instruction loads 1 KiB of
// consecutive channels and an input row is fetched (ROWS + 1) / ROWS times by the strips above and below each other and 17 / 16 times
// by neighbouring strips — through L2 mostly.  The row after the next is requested ahead of the current row's arithmetic.  The
// 1024 (k4) or 64 (k2) weights live in registers: 64 or 16 per lane, the lane's four channels.  After the butterfly every lane of a
// group holds the four sums; lanes 0..3 of it run the epilogue of one pixel each and store it.
#include "conv_gemm_kernels.h"

namespace {

template <int K>
struct Geo {
    static constexpr int LPR = K == 4 ? 16 : 4;  // lanes per cell = Cin / 4
    static constexpr int CPW = 64 / LPR;         // cells per wave
    static constexpr int STRIP = 4 * CPW;        // cell columns per workgroup
    static constexpr int ROWS = K == 4 ? 16 : 8;  // cell rows per workgroup
    static constexpr int OFF = K == 4 ? 1 : 0;   // output pixel of cell (i, j), (a, b): (2i + OFF + a, 2j + OFF + b); first cell is -OFF
};

struct Args {
    const float *x;
    int64_t x_bs, x_ys, x_xs;
    int Hi, Wi;
    const float *w, *scale, *bias;
    int act;
    float act_alpha;
    float *out;
    int64_t o_bs, o_ys, o_xs;
    int out_h, out_w, ncy, ncx;  // output extent; cell rows / columns that have an output inside it
};

__device__ __forceinline__ float fma4(const f32x4 v, const float w0, const float w1, const float w2, const float w3, float acc) {
    acc = __builtin_fmaf(v.x, w0, acc);
    acc = __builtin_fmaf(v.y, w1, acc);
    acc = __builtin_fmaf(v.z, w2, acc);
    acc = __builtin_fmaf(v.w, w3, acc);
    return acc;
}

template <int K>
__global__ __launch_bounds__(256) void convt_cout1_kernel(const Args p) {
    using G = Geo<K>;
    constexpr int LPR = G::LPR, KK = K * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, slot = lane / LPR;
    const int cx = (blockIdx.x * 4 + wave) * G::CPW + slot;  // cell column; its (left) input column:
    const int j = cx - G::OFF;
    const int cy0 = blockIdx.y * G::ROWS;
    const bool cok = cx < p.ncx;
    const float *xb = p.x + (int64_t)blockIdx.z * p.x_bs + sub * 4;

    float wr[4][KK];  // the lane's four channels: w[4 sub + c][0][ky][kx]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < KK; t += 4) {
            const f32x4 w4 = *reinterpret_cast<const f32x4 *>(p.w + (sub * 4 + c) * KK + t);
            wr[c][t] = w4.x, wr[c][t + 1] = w4.y, wr[c][t + 2] = w4.z, wr[c][t + 3] = w4.w;
        }

    // Loads are unconditional, from a clamped (always valid) position, and the zero of a tap outside the image is selected when the
    // value is first used: a branch around a load would make the compiler wait for every outstanding load at once.
    auto in_img = [&](const int iy, const int ix) -> bool { return cok && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi; };
    auto ld = [&](const int iy, const int ix) -> f32x4 {
        const int y = iy < 0 ? 0 : (iy >= p.Hi ? p.Hi - 1 : iy), x = ix < 0 ? 0 : (ix >= p.Wi ? p.Wi - 1 : ix);
        return *reinterpret_cast<const f32x4 *>(xb + (int64_t)y * p.x_ys + (int64_t)x * p.x_xs);
    };
    // (a, b) = (sub >> 1, sub & 1) is the pixel lane sub < 4 of a group finishes and stores
    const int X = 2 * j + G::OFF + (sub & 1);
    const bool xok = cok && sub < 4 && X >= 0 && X < p.out_w;
    float *ob = p.out + (int64_t)blockIdx.z * p.o_bs + (int64_t)X * p.o_xs;
    const float scale = p.scale ? p.scale[0] : 1.f, bias = p.bias ? p.bias[0] : 0.f;

    const int i0 = cy0 - G::OFF;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // k4: rows i (t) and i + 1 (b), columns j (0) and j + 1 (1); k2: b0 is the pixel.  n0 / n1: the row requested ahead, as loaded
    f32x4 t0 = zero4, t1 = zero4, n0, n1 = zero4;
    bool nok0, nok1 = false;
    if (K == 4) {
        t0 = in_img(i0, j) ? ld(i0, j) : zero4, t1 = in_img(i0, j + 1) ? ld(i0, j + 1) : zero4;
        n0 = ld(i0 + 1, j), n1 = ld(i0 + 1, j + 1);
        nok0 = in_img(i0 + 1, j), nok1 = in_img(i0 + 1, j + 1);
    } else {
        n0 = ld(i0, j);
        nok0 = in_img(i0, j);
    }
#pragma unroll 1
    for (int r = 0; r < G::ROWS; ++r) {
        const int cy = cy0 + r;
        if (cy >= p.ncy) break;
        const int i = cy - G::OFF;
        const f32x4 b0 = nok0 ? n0 : zero4, b1 = nok1 ? n1 : zero4;
        // the next cell row's new input row, requested ahead of this row's arithmetic (past the last cell row: a repeat of a valid row)
        const int iyn = i + (K == 4 ? 2 : 1);
        const bool more = r + 1 < G::ROWS && cy + 1 < p.ncy;
        n0 = ld(iyn, j);
        nok0 = more && in_img(iyn, j);
        if (K == 4) {
            n1 = ld(iyn, j + 1);
            nok1 = more && in_img(iyn, j + 1);
        }

        float acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float s = 0.f;
                if (K == 4) {
                    const int k11 = a * 4 + b, k10 = a * 4 + b + 2, k01 = (a + 2) * 4 + b, k00 = (a + 2) * 4 + b + 2;
                    s = fma4(b1, wr[0][k11], wr[1][k11], wr[2][k11], wr[3][k11], s);
                    s = fma4(b0, wr[0][k10], wr[1][k10], wr[2][k10], wr[3][k10], s);
                    s = fma4(t1, wr[0][k01], wr[1][k01], wr[2][k01], wr[3][k01], s);
                    s = fma4(t0, wr[0][k00], wr[1][k00], wr[2][k00], wr[3][k00], s);
                } else {
                    const int k0 = a * 2 + b;
                    s = fma4(b0, wr[0][k0], wr[1][k0], wr[2][k0], wr[3][k0], s);
                }
#pragma unroll
                for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
                acc[a][b] = s;
            }
        const int a = sub >> 1;
        const int Y = 2 * i + G::OFF + a;
        if (xok && Y >= 0 && Y < p.out_h) {
            float v = (sub & 2) ? ((sub & 1) ? acc[1][1] : acc[1][0]) : ((sub & 1) ? acc[0][1] : acc[0][0]);
            v = v * scale + bias;
            switch (p.act) {
                case MIT_ACT_RELU: v = mitcg::apply_act<MIT_ACT_RELU>(v, p.act_alpha); break;
                case MIT_ACT_LEAKY: v = mitcg::apply_act<MIT_ACT_LEAKY>(v, p.act_alpha); break;
                case MIT_ACT_SILU: v = mitcg::apply_act<MIT_ACT_SILU>(v, p.act_alpha); break;
                case MIT_ACT_SIGMOID: v = mitcg::apply_act<MIT_ACT_SIGMOID>(v, p.act_alpha); break;
                case MIT_ACT_GELU: v = mitcg::apply_act<MIT_ACT_GELU>(v, p.act_alpha); break;
                default: break;
            }
            ob[(int64_t)Y * p.o_ys] = v;
        }
        if (K == 4) t0 = b0, t1 = b1;
    }
}

template <int K>
void launch(const Args &a, int B, hipStream_t st) {
    using G = Geo<K>;
    dim3 grid((a.ncx + G::STRIP - 1) / G::STRIP, (a.ncy + G::ROWS - 1) / G::ROWS, B);
    hipLaunchKernelGGL(convt_cout1_kernel<K>, grid, dim3(256), 0, st, a);
}

}  // namespace

static_assert(Geo<4>::STRIP == MIT_CONVT_COUT1_STRIP_K4 && Geo<2>::STRIP == MIT_CONVT_COUT1_STRIP_K2, "strip widths of mit_hip.h");

extern "C" int mit_convt_cout1(const float *x_dev, int64_t x_bs, int64_t x_ys, int64_t x_xs, int B, int Hi, int Wi, int Cin, const float *w_dev, int k,
                               int stride, int pad, const float *scale_dev, const float *bias_dev, int act, float act_alpha, float *out_dev,
                               int64_t out_bs, int64_t out_ys, int64_t out_xs, int out_h, int out_w, void *stream) {
    if (!x_dev || !w_dev || !out_dev) return mit_set_error("mit_convt_cout1: null pointer");
    if (!(stride == 2 && ((k == 4 && pad == 1 && Cin == 64) || (k == 2 && pad == 0 && Cin == 16))))
        return mit_set_error("mit_convt_cout1: only k4 s2 p1 at Cin = 64 and k2 s2 p0 at Cin = 16 (got k%d s%d p%d, Cin = %d)", k, stride, pad, Cin);
    if (B <= 0 || B > 65535 || Hi <= 0 || Wi <= 0) return mit_set_error("mit_convt_cout1: need 0 < B < 65536 and a non-empty input");
    if (out_h <= 0 || out_w <= 0 || out_h > 2 * (int64_t)Hi || out_w > 2 * (int64_t)Wi)
        return mit_set_error("mit_convt_cout1: extent %d x %d is not inside the layer's output %lld x %lld", out_h, out_w, 2LL * Hi, 2LL * Wi);
    if ((reinterpret_cast<uintptr_t>(x_dev) & 15) || (reinterpret_cast<uintptr_t>(w_dev) & 15) || (x_bs & 3) || (x_ys & 3) || (x_xs & 3))
        return mit_set_error("mit_convt_cout1: x and w must be 16-byte aligned, the input strides multiples of 4 floats");
    if (act != MIT_ACT_NONE && act != MIT_ACT_RELU && act != MIT_ACT_LEAKY && act != MIT_ACT_SILU && act != MIT_ACT_SIGMOID && act != MIT_ACT_GELU)
        return mit_set_error("mit_convt_cout1: unknown activation %d", act);
    Args a;
    a.x = x_dev, a.x_bs = x_bs, a.x_ys = x_ys, a.x_xs = x_xs, a.Hi = Hi, a.Wi = Wi;
    a.w = w_dev, a.scale = scale_dev, a.bias = bias_dev, a.act = act, a.act_alpha = act_alpha;
    a.out = out_dev, a.o_bs = out_bs, a.o_ys = out_ys, a.o_xs = out_xs, a.out_h = out_h, a.out_w = out_w;
    // cells with an output inside the extent, and the input rows / columns they read (clipped to the image)
    int rows_in, cols_in;
    if (k == 4) {
        a.ncy = (out_h >> 1) + 1, a.ncx = (out_w >> 1) + 1;
        rows_in = a.ncy < Hi ? a.ncy : Hi, cols_in = a.ncx < Wi ? a.ncx : Wi;
    } else {
        a.ncy = rows_in = (out_h + 1) >> 1, a.ncx = cols_in = (out_w + 1) >> 1;
    }
    if ((a.ncy + 7) / 8 > 65535) return mit_set_error("mit_convt_cout1: extent exceeds the grid");
    hipStream_t st = (hipStream_t)stream;
    MitProbeScope probe("convt_cout1_kernel", st, 4.0 * B * ((double)rows_in * cols_in * Cin + (double)out_h * out_w));
    if (k == 4)
        launch<4>(a, B, st);
    else
        launch<2>(a, B, st);
    MIT_CHECK_LAUNCH("mit_convt_cout1");
    return 0;
}
