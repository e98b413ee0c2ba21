// rdb_bf16.hip — the 3x3 convolutions of ESRGAN's residual dense blocks (ResidualDenseBlock_5C, upscaling/esrgan_pytorch.py:152-166) for the
// upscaler's bf16 precision: bf16-RESIDENT activations, v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue (mit_hip.h has the
// arithmetic).  Plus the channel-slice cast that puts an fp32 tensor into the dense-block buffer.
//
// Why a kernel of its own: the layers are narrow (N = 32 or 64, K = 9 * Cin <= 1728).  On the conv_gemm tiles every one of the nine taps
// re-reads its fp32 activations from cache and re-rounds them; here a dense block's activations live in HBM as bf16 (every consumer of
// x, x1 .. x4 is a convolution that would round them anyway), and a workgroup stages each input element to LDS ONCE per launch.
//
// Workgroup = 256 lanes = 4 waves, one tile of TH x TW = 8 x 32 output pixels; wave w owns rows 2w, 2w + 1 (two 32-pixel MFMA row
// blocks) and all N columns: 2 x N / 32 accumulators of 16 registers.  The K loop walks chunks of 32 input channels:
//   A image  [10 x 34 halo pixels][32 ch] bf16, 80 bytes a pixel (64 of data + 16 of pad: the 16 lanes of a ds_read_b128 group then
//            fall on 16 different 16-byte bank slots — 5 r mod 16 is a bijection over each group's rows);
//   W image  [9 taps x 4 k-groups][N] cells of 16 bytes = 8 consecutive k of one output column, which is the B fragment of a lane; a
//            k-group's row of N cells is followed by 16 bytes of pad.  The packed weight is [9 * Cin][N] row-major, so a lane takes
//            8 rows x 8 columns (eight 16-byte loads), transposes them in registers and writes eight cells.  Eight consecutive lanes
//            (one ds_write_b128 group) hold eight k-groups of the same columns: with the pad their cells fall on eight different
//            16-byte slots (the same k-group in neighbouring lanes would put all eight on one slot), while a load instruction of
//            the wave still reads whole 128-byte weight rows.
// 27200 + 36 * (N * 16 + 16) bytes = 64640 at N = 64: static LDS, two workgroups a CU.  The next chunk's global loads are issued before the
// MFMAs of the current one and written to LDS after them, so the loads travel under 18 k-steps of 2 x N / 32 MFMAs.
// Accumulation order of a pixel: chunk, tap, channel — fixed, whatever the batch or the tile.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "bf16_split.h"
#include "common.h"

namespace {

using mitcg::bf16x8;
using mitcg::u32x4;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TH = MIT_RDB_TILE_H, TW = MIT_RDB_TILE_W;
constexpr int HH = TH + 2, HW = TW + 2, HALO = HH * HW;   // 10 x 34 = 340 halo pixels
constexpr int CK = 32;                                     // input channels a chunk
constexpr int PIX_B = 80;                                  // LDS bytes a halo pixel
constexpr int A_BYTES = HALO * PIX_B;                      // 27200
constexpr int THREADS = 256;
constexpr int A_UNITS = HALO * (CK / 8);                   // 16-byte units of the A image: 1360
constexpr int A_ROUNDS = (A_UNITS + THREADS - 1) / THREADS;
constexpr int KG = 9 * CK / 8;                             // k-groups (8 rows) of a chunk's weights: 36
static_assert(TW == 32 && TH == 8, "a wave owns two 32-pixel rows of the tile");
static_assert(A_BYTES % 16 == 0, "the W image starts on a 16-byte boundary");

__device__ __forceinline__ unsigned short bf16_bits(float v) {   // round to nearest even (v_cvt_pk_bf16_f32)
    return (unsigned short)(mitcg::pack_bf16(v, 0.0f) & 0xffffu);
}

// VEC: the epilogue goes through LDS so that a lane owns four consecutive channels of a pixel (16-byte loads and stores of the fp32
// operands, 8-byte stores of the bf16 output); the host takes it when every epilogue tensor is aligned for that.  Otherwise a lane
// keeps the column the accumulator layout gives it (4- and 2-byte accesses).  Same expression sequence: the same bits.
template <int N, bool VEC>
__global__ __launch_bounds__(THREADS, 2) void rdb_conv3x3_kernel(const MitRdbConv d) {
    constexpr int NB = N / 32, NG = N / 8, W_ROW = N * 16 + 16;                          // bytes of a k-group's row of cells, padded
    constexpr int SLOTS = (KG + 7) / 8 * 8 * NG, W_ROUNDS = (SLOTS + THREADS - 1) / THREADS;   // task slots: 8 k-groups x NG column groups a block
    __shared__ u32x4 lds[(A_BYTES + KG * W_ROW) / 16];
    unsigned char *ldsA = reinterpret_cast<unsigned char *>(lds);
    unsigned char *ldsW = ldsA + A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int64_t b = blockIdx.z;
    const int H = d.H, W = d.W, Cin = d.Cin;
    const uint16_t *in = d.in + b * d.in_bs;
    const uint16_t *wt = d.w;

    // what this lane stages of every chunk.  A image: unit u = pixel * 4 + part; offset -1 = outside the image (zeros), -2 = no unit
    int a_off[A_ROUNDS];
#pragma unroll
    for (int i = 0; i < A_ROUNDS; ++i) {
        const int u = tid + i * THREADS;
        const int p = u >> 2, part = u & 3;
        const int hy = p / HW, hx = p - hy * HW;
        const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        a_off[i] = u >= A_UNITS ? -2 : (inside ? (int)(gy * d.in_ys + gx * d.in_xs) + part * 8 : -1);
    }
    // W image: a task = (k-group, column group): rows (tap * Cin + c8 .. + 7), columns ng * 8 .. + 7; k-group fastest over the lanes
    int w_off[W_ROUNDS], w_cell[W_ROUNDS];
#pragma unroll
    for (int i = 0; i < W_ROUNDS; ++i) {
        const int task = tid + i * THREADS;
        const int kg = (task & 7) + 8 * (task / (8 * NG)), ng = (task >> 3) % NG;
        const int tap = kg >> 2, c8 = (kg & 3) * 8;
        w_off[i] = kg < KG ? (tap * Cin + c8) * N + ng * 8 : -1;
        w_cell[i] = kg * W_ROW + ng * 128;
    }

    u32x4 a_reg[A_ROUNDS], w_reg[W_ROUNDS][8];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < A_ROUNDS; ++i) {
            a_reg[i] = u32x4{0u, 0u, 0u, 0u};
            if (a_off[i] >= 0) a_reg[i] = *reinterpret_cast<const u32x4 *>(in + a_off[i] + c0);
        }
#pragma unroll
        for (int i = 0; i < W_ROUNDS; ++i)
            if (w_off[i] >= 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w_reg[i][j] = *reinterpret_cast<const u32x4 *>(wt + w_off[i] + (c0 + j) * N);
            }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < A_ROUNDS; ++i) {
            const int u = tid + i * THREADS;
            if (a_off[i] != -2) *reinterpret_cast<u32x4 *>(ldsA + (u >> 2) * PIX_B + (u & 3) * 16) = a_reg[i];
        }
#pragma unroll
        for (int i = 0; i < W_ROUNDS; ++i)
            if (w_off[i] >= 0) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {   // column c of the 8 x 8 block: rows 2q, 2q + 1 share dword q of the cell
                    u32x4 cell;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned lo = w_reg[i][2 * q][c >> 1], hi = w_reg[i][2 * q + 1][c >> 1];
                        cell[q] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
                    }
                    *reinterpret_cast<u32x4 *>(ldsW + w_cell[i] + c * 16) = cell;
                }
            }
    };

    f32x16 acc[2][NB];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][nb][e] = 0.0f;

    // this lane's fragment addresses at tap (0, 0), k-step 0
    const unsigned char *a_base = ldsA + ((wave * 2) * HW + r) * PIX_B + h * 16;
    const unsigned char *w_base = ldsW + h * W_ROW + r * 16;

    fetch(0);
    for (int c0 = 0; c0 < Cin; c0 += CK) {
        __syncthreads();   // the previous chunk's fragments have been read
        stage();
        __syncthreads();
        if (c0 + CK < Cin) fetch(c0 + CK);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 fa[2], fb[NB];
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    fa[m] = *reinterpret_cast<const bf16x8 *>(a_base + ((m + dy) * HW + dx) * PIX_B + s * 32);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    fb[nb] = *reinterpret_cast<const bf16x8 *>(w_base + (tap * 4 + 2 * s) * W_ROW + nb * 512);
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) acc[m][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], fb[nb], acc[m][nb], 0, 0, 0);
            }
        }
    }

    const bool leaky = d.act == MIT_ACT_LEAKY;
    const float *post = d.post ? d.post + b * d.post_bs : nullptr;
    const float *post2 = d.post2 ? d.post2 + b * d.post2_bs : nullptr;
    float *of = d.out_f32 ? d.out_f32 + b * d.of_bs : nullptr;
    uint16_t *ob = d.out_bf16 ? d.out_bf16 + b * d.ob_bs : nullptr;
    if (VEC) {
        // one row of the wave's two at a time: 32 pixels x N fp32 of LDS a wave (pixel rows of N floats: the ds_read_b128 lane groups
        // fall on 16 different slots without padding), then lane = (pixel, four channels)
        constexpr int Q = N / 4, PX_IT = 64 / Q;
        float *tile = reinterpret_cast<float *>(lds) + wave * (32 * N);
        const int q = lane % Q, pl = lane / Q;
        float sc[4], bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sc[j] = d.scale ? d.scale[4 * q + j] : 1.0f;
            bi[j] = d.bias ? d.bias[4 * q + j] : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            __syncthreads();   // the images (m = 0) or the previous row (m = 1) have been read
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) tile[((e & 3) + 8 * (e >> 2) + 4 * h) * N + nb * 32 + r] = acc[m][nb][e];
            __syncthreads();
            const int y = ty0 + wave * 2 + m;
            if (y >= H) continue;
#pragma unroll
            for (int it = 0; it < 32 / PX_IT; ++it) {
                const int xi = it * PX_IT + pl, x = tx0 + xi;
                if (x >= W) continue;
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(tile + xi * N + 4 * q);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = v[j] * sc[j] + bi[j];
                    if (leaky) v[j] = v[j] >= 0.0f ? v[j] : v[j] * d.act_alpha;
                }
                if (post) {
                    const f32x4 p4 = *reinterpret_cast<const f32x4 *>(post + (int)(y * d.post_ys + x * d.post_xs) + 4 * q);
                    v[0] = v[0] + p4.x, v[1] = v[1] + p4.y, v[2] = v[2] + p4.z, v[3] = v[3] + p4.w;
                }
                if (post2) {
                    const f32x4 p4 = *reinterpret_cast<const f32x4 *>(post2 + (int)(y * d.post2_ys + x * d.post2_xs) + 4 * q);
                    v[0] = v[0] * d.s2 + p4.x, v[1] = v[1] * d.s2 + p4.y, v[2] = v[2] * d.s2 + p4.z, v[3] = v[3] * d.s2 + p4.w;
                }
                if (of) *reinterpret_cast<f32x4 *>(of + (int)(y * d.of_ys + x * d.of_xs) + 4 * q) = f32x4{v[0], v[1], v[2], v[3]};
                if (ob)
                    *reinterpret_cast<mitcg::u32x2 *>(ob + (int)(y * d.ob_ys + x * d.ob_xs) + 4 * q) =
                        mitcg::u32x2{mitcg::pack_bf16(v[0], v[1]), mitcg::pack_bf16(v[2], v[3])};
            }
        }
        return;
    }
    // the lane holds column n = nb * 32 + r of the pixels x = tx0 + (e & 3) + 8 (e >> 2) + 4 h of its two rows
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = nb * 32 + r;
        const float sc = d.scale ? d.scale[n] : 1.0f, bi = d.bias ? d.bias[n] : 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int y = ty0 + wave * 2 + m;
            if (y >= H) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int x = tx0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (x >= W) continue;
                float v = acc[m][nb][e] * sc + bi;
                if (leaky) v = v >= 0.0f ? v : v * d.act_alpha;
                if (post) v = v + post[(int)(y * d.post_ys + x * d.post_xs) + n];
                if (post2) v = v * d.s2 + post2[(int)(y * d.post2_ys + x * d.post2_xs) + n];
                if (of) of[(int)(y * d.of_ys + x * d.of_xs) + n] = v;
                if (ob) ob[(int)(y * d.ob_ys + x * d.ob_xs) + n] = bf16_bits(v);
            }
        }
    }
}

constexpr int CAST_BLOCK = 256;

// VEC: one lane = four channels of a pixel (float4 in, two packed pairs out); else one channel.  Cg = channel groups a pixel.
template <bool VEC>
__global__ __launch_bounds__(CAST_BLOCK) void cast_f32_bf16_kernel(const float *src, int64_t s_bs, int64_t s_ys, int64_t s_xs, uint16_t *dst,
                                                                   int64_t d_bs, int64_t d_ys, int64_t d_xs, int H, int W, int Cn, int Cg,
                                                                   int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * CAST_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % Cg);
    int64_t p = i / Cg;
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H);
    const int64_t b = p / H;
    const float *s = src + b * s_bs + y * s_ys + x * s_xs;
    uint16_t *o = dst + b * d_bs + y * d_ys + x * d_xs;
    if (VEC) {
        const int c = g * 4;
        if (c + 4 <= Cn) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(s + c);
            *reinterpret_cast<mitcg::u32x2 *>(o + c) = mitcg::u32x2{mitcg::pack_bf16(v.x, v.y), mitcg::pack_bf16(v.z, v.w)};
        } else {
            for (int k = c; k < Cn; ++k) o[k] = bf16_bits(s[k]);
        }
    } else {
        o[g] = bf16_bits(s[g]);
    }
}

// [lo, hi) element extent of a strided NHWC tensor with C channels addressed
int64_t extent(int B, int H, int W, int C, int64_t bs, int64_t ys, int64_t xs) {
    return (int64_t)(B - 1) * bs + (int64_t)(H - 1) * ys + (int64_t)(W - 1) * xs + C;
}

// strides of one tensor: x stride >= channels, y stride >= x stride, batch stride >= 0, one image below 2^31 elements
const char *bad_strides(int H, int W, int C, int64_t bs, int64_t ys, int64_t xs) {
    if (xs < C) return "x stride smaller than the channel count";
    if (ys < xs || bs < 0) return "y stride smaller than the x stride, or a negative batch stride";
    if (ys > INT32_MAX || extent(1, H, W, C, 0, ys, xs) > INT32_MAX) return "one image spans 2^31 elements or more (32-bit offsets inside an image)";
    return nullptr;
}

}  // namespace

extern "C" int mit_rdb_conv3x3_bf16(const MitRdbConv *dp, void *stream) {
    if (!dp) return mit_set_error("mit_rdb_conv3x3_bf16: null descriptor");
    const MitRdbConv &d = *dp;
    if (!d.in || !d.w) return mit_set_error("mit_rdb_conv3x3_bf16: null pointer (in / w)");
    if (!d.out_f32 && !d.out_bf16) return mit_set_error("mit_rdb_conv3x3_bf16: null pointer (no output: out_f32 and out_bf16 are both NULL)");
    if (d.B <= 0 || d.H <= 0 || d.W <= 0) return mit_set_error("mit_rdb_conv3x3_bf16: sizes must be positive (B %d, H %d, W %d)", d.B, d.H, d.W);
    if (d.Cin % CK != 0 || d.Cin < 64 || d.Cin > 192)
        return mit_set_error("mit_rdb_conv3x3_bf16: Cin must be a multiple of 32 in [64, 192] (got %d)", d.Cin);
    if (d.N != 32 && d.N != 64) return mit_set_error("mit_rdb_conv3x3_bf16: N must be 32 or 64 (got %d)", d.N);
    if (d.act != MIT_ACT_NONE && d.act != MIT_ACT_LEAKY) return mit_set_error("mit_rdb_conv3x3_bf16: act must be none or leaky (got %d)", d.act);
    const char *why;
    if ((why = bad_strides(d.H, d.W, d.Cin, d.in_bs, d.in_ys, d.in_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: input strides: %s", why);
    if (d.post && (why = bad_strides(d.H, d.W, d.N, d.post_bs, d.post_ys, d.post_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: post strides: %s", why);
    if (d.post2 && (why = bad_strides(d.H, d.W, d.N, d.post2_bs, d.post2_ys, d.post2_xs)))
        return mit_set_error("mit_rdb_conv3x3_bf16: post2 strides: %s", why);
    if (d.out_f32 && (why = bad_strides(d.H, d.W, d.N, d.of_bs, d.of_ys, d.of_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: out_f32 strides: %s", why);
    if (d.out_bf16 && (why = bad_strides(d.H, d.W, d.N, d.ob_bs, d.ob_ys, d.ob_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: out_bf16 strides: %s", why);
    if (reinterpret_cast<uintptr_t>(d.in) % 16 || reinterpret_cast<uintptr_t>(d.w) % 16 || d.in_xs % 8 || d.in_ys % 8 || d.in_bs % 8)
        return mit_set_error("mit_rdb_conv3x3_bf16: in and w must be 16-byte aligned and the input strides multiples of 8 elements");
    if (mit_div_up(d.H, TH) > 65535 || d.B > 65535)
        return mit_set_error("mit_rdb_conv3x3_bf16: at most 65535 tile rows and 65535 images a launch (grid y / z)");
    if (d.out_bf16) {
        // byte addresses as integers: the two may be one buffer (the dense block's) or two
        const int64_t din = (int64_t)(reinterpret_cast<intptr_t>(d.out_bf16) - reinterpret_cast<intptr_t>(d.in)) / 2;
        bool overlap;
        if (d.ob_bs == d.in_bs && d.ob_ys == d.in_ys && d.ob_xs == d.in_xs && din > -d.in_xs && din < d.in_xs)
            overlap = din > -(int64_t)d.N && din < d.Cin;   // one buffer, same pixel grid: the channel ranges [0, Cin) and [din, din + N)
        else
            overlap = din < extent(d.B, d.H, d.W, d.Cin, d.in_bs, d.in_ys, d.in_xs) && -din < extent(d.B, d.H, d.W, d.N, d.ob_bs, d.ob_ys, d.ob_xs);
        if (overlap) return mit_set_error("mit_rdb_conv3x3_bf16: out_bf16 overlaps the input channels it is computed from");
    }
    const dim3 grid((unsigned)mit_div_up(d.W, TW), (unsigned)mit_div_up(d.H, TH), (unsigned)d.B);
    const double px = (double)d.B * d.H * d.W;
    // the wide epilogue: fp32 tensors on 16 bytes, the bf16 output on 8, every stride a multiple of four elements
    auto wide = [](const void *p, int64_t bs, int64_t ys, int64_t xs, int align) {
        return !p || (reinterpret_cast<uintptr_t>(p) % align == 0 && bs % 4 == 0 && ys % 4 == 0 && xs % 4 == 0);
    };
    const bool vec = wide(d.post, d.post_bs, d.post_ys, d.post_xs, 16) && wide(d.post2, d.post2_bs, d.post2_ys, d.post2_xs, 16) &&
                     wide(d.out_f32, d.of_bs, d.of_ys, d.of_xs, 16) && wide(d.out_bf16, d.ob_bs, d.ob_ys, d.ob_xs, 8);
    MitProbeScope probe(d.N == 64 ? "rdb_conv3x3_kernel<64>" : "rdb_conv3x3_kernel<32>", (hipStream_t)stream,
                        px * (2.0 * d.Cin + (d.out_bf16 ? 2.0 : 0.0) * d.N + 4.0 * d.N * ((d.out_f32 ? 1 : 0) + (d.post ? 1 : 0) + (d.post2 ? 1 : 0))) +
                            18.0 * d.Cin * d.N,
                        px * 18.0 * d.Cin * d.N);
    const auto kern = d.N == 64 ? (vec ? rdb_conv3x3_kernel<64, true> : rdb_conv3x3_kernel<64, false>)
                                : (vec ? rdb_conv3x3_kernel<32, true> : rdb_conv3x3_kernel<32, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, (hipStream_t)stream, d);
    MIT_CHECK_LAUNCH("mit_rdb_conv3x3_bf16");
    return 0;
}

extern "C" int mit_cast_f32_bf16(const float *src_dev, int64_t s_bs, int64_t s_ys, int64_t s_xs, uint16_t *dst_dev, int64_t d_bs, int64_t d_ys,
                                 int64_t d_xs, int B, int H, int W, int Cn, void *stream) {
    if (!src_dev || !dst_dev) return mit_set_error("mit_cast_f32_bf16: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Cn <= 0) return mit_set_error("mit_cast_f32_bf16: sizes must be positive (B %d, H %d, W %d, C %d)", B, H, W, Cn);
    if (s_xs < Cn || d_xs < Cn) return mit_set_error("mit_cast_f32_bf16: x stride smaller than the channel count");
    if (s_ys < s_xs || d_ys < d_xs || s_bs < 0 || d_bs < 0)
        return mit_set_error("mit_cast_f32_bf16: y stride smaller than the x stride, or a negative batch stride");
    const bool vec = Cn >= 4 && reinterpret_cast<uintptr_t>(src_dev) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_dev) % 8 == 0 &&
                     s_xs % 4 == 0 && s_ys % 4 == 0 && s_bs % 4 == 0 && d_xs % 4 == 0 && d_ys % 4 == 0 && d_bs % 4 == 0;
    const int Cg = vec ? (Cn + 3) / 4 : Cn;
    const int64_t total = (int64_t)B * H * W * Cg;
    const int64_t blocks = (total + CAST_BLOCK - 1) / CAST_BLOCK;
    if (blocks > INT32_MAX) return mit_set_error("mit_cast_f32_bf16: %lld lanes are more than one launch addresses", (long long)total);
    MitProbeScope probe("cast_f32_bf16_kernel", (hipStream_t)stream, 6.0 * B * H * W * Cn);
    if (vec)
        hipLaunchKernelGGL(cast_f32_bf16_kernel<true>, dim3((unsigned)blocks), dim3(CAST_BLOCK), 0, (hipStream_t)stream, src_dev, s_bs, s_ys, s_xs,
                           dst_dev, d_bs, d_ys, d_xs, H, W, Cn, Cg, total);
    else
        hipLaunchKernelGGL(cast_f32_bf16_kernel<false>, dim3((unsigned)blocks), dim3(CAST_BLOCK), 0, (hipStream_t)stream, src_dev, s_bs, s_ys,
                           s_xs, dst_dev, d_bs, d_ys, d_xs, H, W, Cn, Cg, total);
    MIT_CHECK_LAUNCH("mit_cast_f32_bf16");
    return 0;
}
