// aot_bf16.hip — the 3x3 convolutions of the AOT generator's blocks (AOTBlock, inpainting/inpainting_aot.py:170-193) for the inpainter's
// bf16 precision: the four dilated branches 128 -> 32 (rates 2, 4, 8, 16; ReflectionPad2d(rate)) as ONE launch of four groups, and the
// fuse / gate convolutions 128 -> 128 (rate 1), on bf16-RESIDENT operands, v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue
// (mit_hip.h has the arithmetic).
//
// Workgroup = 256 lanes = 4 waves, one tile of TH x TW = 8 x 32 output pixels of one (image, group); wave w owns rows 2w, 2w + 1 (two
// 32-pixel MFMA row blocks) and all N columns: 2 x N / 32 accumulators of 16 registers.  The K loop walks chunks of 32 input channels:
//   W  image [9 taps x 4 k-groups][N] cells of 16 bytes = 8 consecutive k of one output column (the B fragment of a lane), a k-group's
//      row of N cells followed by 16 bytes of pad: the layout, the in-register 8 x 8 transposition and the bank argument of
//      rdb_bf16.hip.  36 * (N * 16 + 16) bytes: 19008 at N = 32, 74304 at N = 128.  The next chunk's weight rows are requested before
//      the MFMAs of the current one and written to LDS after them.
//   A  one of two forms, chosen per workgroup from its group's rate alone (so a launch of four groups mixes them):
//      staged   the region the nine windows of the tile touch — columns tx0 - rate .. tx0 + 31 + rate of the rows ty0 - rate ..
//               ty0 + 7 + rate (rate <= 8) or of three 8-row bands (larger rates) — goes to LDS once per chunk, reflected, 80 bytes a
//               pixel (64 of data + 16 of pad: the 16 lanes of a ds_read_b128 group fall on 16 different 16-byte slots, as in
//               rdb_bf16.hip), and serves all nine taps.  The global loads are whole 64-byte pixel chunks by four neighbouring lanes.
//               The A image holds AR * 64 = 640 pixels (51200 bytes): rates 1 .. 4 (a 16 x 40 region at rate 4).  The regions of
//               rates 8 and 16 (24 x 48 and 24 x 64 pixels: 92 and 123 KB) fit the LDS only at one workgroup a CU and were measured
//               slower there than the direct form.
//      direct   no LDS.  Lane (r = lane & 31, h = lane >> 5) of a 32x32x16 MFMA holds A[pixel r][k = 8 h .. 8 h + 7]: eight consecutive
//               channels of ONE pixel, 16 contiguous bytes of a bf16 NHWC tensor.  So a lane loads its fragment of a tap straight from
//               the input at the reflected tap pixel.  At rate >= 8 the nine windows of a tile are disjoint: there is no halo to
//               share, and every element of a window is loaded by exactly one lane of the workgroup, which is what staging the
//               windows would load as well.  The fragments of the tap three steps ahead are requested before the MFMAs of the
//               current one (a ring of three).
// 70208 bytes of static LDS at N = 32 (two workgroups a CU), 125504 at N = 128 (one).
// Accumulation order of a pixel: chunk, tap, channel — fixed, whatever the form, the batch, the group count or the tile.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/mit_hip.h"
#include "bf16_split.h"
#include "common.h"

namespace {

using mitcg::bf16x8;
using mitcg::u32x4;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TH = MIT_AOT_TILE_H, TW = MIT_AOT_TILE_W;
constexpr int CK = 32;                                     // input channels a chunk
constexpr int THREADS = 256;
constexpr int KG = 9 * CK / 8;                             // k-groups (8 rows) of a chunk's weights: 36
constexpr int PF = 3;                                      // taps the A fragments are requested ahead (direct form)
constexpr int AR = 10;                                     // rounds of 256 16-byte units the staged form's A image holds: 640 region pixels
constexpr int PIX_B = 80;                                  // LDS bytes a region pixel (staged form): 64 of data + 16 of pad, as in rdb_bf16.hip
static_assert(TW == 32 && TH == 8, "a wave owns two 32-pixel rows of the tile");
static_assert(9 % PF == 0, "a tap keeps its ring slot from chunk to chunk");

__device__ __forceinline__ unsigned short bf16_bits(float v) {   // round to nearest even (v_cvt_pk_bf16_f32)
    return (unsigned short)(mitcg::pack_bf16(v, 0.0f) & 0xffffu);
}

// ReflectionPad2d: p in [-rate, L - 1 + rate] with rate <= L - 1
__device__ __forceinline__ int reflect(int p, int L) { return p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p); }

// VEC: the epilogue goes through LDS so that a lane owns four consecutive channels of a pixel (16-byte stores of the fp32 output, 8-byte
// stores of the bf16 output); the host takes it when every output is aligned for that.  Otherwise a lane keeps the column the
// accumulator layout gives it (4- and 2-byte stores).  Same expression sequence: the same bits.
template <int N, bool VEC>
__global__ __launch_bounds__(THREADS, N == 32 ? 2 : 1) void aot_conv3x3_kernel(const MitAotConv d) {
    constexpr int NB = N / 32, NG = N / 8, W_ROW = N * 16 + 16;                          // bytes of a k-group's row of cells, padded
    constexpr int SLOTS = (KG + 7) / 8 * 8 * NG, W_ROUNDS = (SLOTS + THREADS - 1) / THREADS;   // task slots: 8 k-groups x NG column groups a block
    constexpr int A_BYTES = AR * (THREADS / 4) * PIX_B;                                  // room for AR * 64 region pixels
    constexpr int W_BYTES = KG * W_ROW, E_BYTES = 4 * 32 * N * 4;
    __shared__ u32x4 lds[(A_BYTES + W_BYTES > E_BYTES ? A_BYTES + W_BYTES : E_BYTES) / 16];
    unsigned char *ldsA = reinterpret_cast<unsigned char *>(lds);
    unsigned char *ldsW = ldsA + A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int g = (int)(blockIdx.z % (unsigned)d.groups);
    const int64_t b = blockIdx.z / (unsigned)d.groups;
    const int H = d.H, W = d.W, Cin = d.Cin;
    const int rate = d.rate[g];
    const uint16_t *in = d.in + b * d.in_bs;
    const uint16_t *wt = d.w[g];

    // element offsets of this lane's tap pixels: rows 2 wave + m at the three tap rows, its column at the three tap columns.  A pixel
    // past the image's edge (partial tile) reads the edge pixel's window; its result is not stored.
    int row_off[2][3], col_off[3];
    const int BW = TW + 2 * rate, NR = rate <= TH ? TH + 2 * rate : 3 * TH;
    const bool staged = NR * BW * 4 <= AR * THREADS;   // the form of this workgroup's group: its region fits the A image, or direct
    if (!staged) {
        const int x = min(tx0 + r, W - 1);
#pragma unroll
        for (int t = 0; t < 3; ++t) col_off[t] = reflect(x + (t - 1) * rate, W) * (int)d.in_xs + h * 8;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int y = min(ty0 + wave * 2 + m, H - 1);
#pragma unroll
            for (int t = 0; t < 3; ++t) row_off[m][t] = reflect(y + (t - 1) * rate, H) * (int)d.in_ys;
        }
    }
    // Staged form.  The region: columns tx0 - rate .. tx0 + 31 + rate (BW of them) of the rows the nine windows touch — the 8 + 2 rate
    // contiguous rows ty0 - rate .. ty0 + 7 + rate while the three tap rows' bands overlap or touch (rate <= 8), else three bands of 8
    // rows at ty0 + (dy - 1) rate.  Unit u = pixel * 4 + part; offset -1 = no unit.  Coordinates are reflected, then clamped: a clamp
    // only ever changes a pixel that nothing but an output pixel outside the image reads.
    int a_off[AR];
    if (staged) {
        const int units = NR * BW * 4;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int u = tid + i * THREADS;
            const int p = u >> 2, part = u & 3;
            const int j = p / BW, cx = p - j * BW;
            const int v = rate <= TH ? ty0 - rate + j : ty0 + (j / TH - 1) * rate + (j % TH);
            const int gy = min(max(reflect(v, H), 0), H - 1), gx = min(max(reflect(tx0 - rate + cx, W), 0), W - 1);
            a_off[i] = u < units ? gy * (int)d.in_ys + gx * (int)d.in_xs + part * 8 : -1;
        }
        // LDS byte offsets of this lane's fragments: region row of (tile row 2 wave + m, tap row dy), tap column dx
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 3; ++t) row_off[m][t] = ((rate <= TH ? t * rate : t * TH) + wave * 2 + m) * BW * PIX_B;
#pragma unroll
        for (int t = 0; t < 3; ++t) col_off[t] = (t * rate + r) * PIX_B + h * 16;
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

    u32x4 w_reg[W_ROUNDS][8];
    auto fetch_w = [&](int c0) {
#pragma unroll
        for (int i = 0; i < W_ROUNDS; ++i)
            if (w_off[i] >= 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w_reg[i][j] = *reinterpret_cast<const u32x4 *>(wt + w_off[i] + (c0 + j) * N);
            }
    };
    auto stage_w = [&]() {
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

    const unsigned char *w_base = ldsW + h * W_ROW + r * 16;   // this lane's B fragment at tap 0, k-step 0

    // The K loop, once per form (two bodies, so that neither carries the other's registers); st: std::true_type = staged.
    auto k_loop = [&](auto st) {
        constexpr bool ST = decltype(st)::value;
        u32x4 a_reg[ST ? AR : 1];
        auto fetch_region = [&](int c0) {
#pragma unroll
            for (int i = 0; i < AR; ++i)
                if (a_off[i] >= 0) a_reg[ST ? i : 0] = *reinterpret_cast<const u32x4 *>(in + a_off[i] + c0);
        };
        auto stage_region = [&]() {
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int u = tid + i * THREADS;
                if (a_off[i] >= 0) *reinterpret_cast<u32x4 *>(ldsA + (u >> 2) * PIX_B + (u & 3) * 16) = a_reg[ST ? i : 0];
            }
        };
        // direct form: A fragments of one tap of one chunk, [row m][k-step s]
        bf16x8 ring[ST ? 1 : PF][2][2];
        auto fetch_a = [&](int slot, int c0, int tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    ring[ST ? 0 : slot][m][s] = *reinterpret_cast<const bf16x8 *>(in + row_off[m][dy] + col_off[dx] + c0 + s * 16);
        };

        fetch_w(0);
        if (ST) {
            fetch_region(0);
        } else {
#pragma unroll
            for (int t = 0; t < PF; ++t) fetch_a(t, 0, t);
        }
        for (int c0 = 0; c0 < Cin; c0 += CK) {
            __syncthreads();   // the previous chunk's fragments have been read
            stage_w();
            if (ST) stage_region();
            __syncthreads();
            const bool more = c0 + CK < Cin;
            if (more) fetch_w(c0 + CK);
            if (ST && more) fetch_region(c0 + CK);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                bf16x8 fa[2][2];
                if (ST) {
                    const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            fa[m][s] = *reinterpret_cast<const bf16x8 *>(ldsA + row_off[m][dy] + col_off[dx] + s * 32);
                } else {
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int s = 0; s < 2; ++s) fa[m][s] = ring[ST ? 0 : tap % PF][m][s];
                    if (tap + PF < 9)
                        fetch_a(tap % PF, c0, tap + PF);
                    else if (more)
                        fetch_a(tap % PF, c0 + CK, tap + PF - 9);
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8 fb[NB];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        fb[nb] = *reinterpret_cast<const bf16x8 *>(w_base + (tap * 4 + 2 * s) * W_ROW + nb * 512);
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[m][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m][s], fb[nb], acc[m][nb], 0, 0, 0);
                }
            }
        }
    };
    if (staged)
        k_loop(std::true_type{});
    else
        k_loop(std::false_type{});

    const bool relu = d.act == MIT_ACT_RELU;
    const int oc0 = d.out_c0[g];
    const float *bias = d.bias[g];
    float *of = d.out_f32 ? d.out_f32 + b * d.of_bs + oc0 : nullptr;
    uint16_t *ob = d.out_bf16 ? d.out_bf16 + b * d.ob_bs + oc0 : nullptr;
    if (VEC) {
        // one row of the wave's two at a time: 32 pixels x N fp32 of LDS a wave (pixel rows of N floats: the ds_read_b128 lane groups
        // fall on 16 different slots without padding), then lane = (pixel, four channels)
        constexpr int Q = N / 4, PX_IT = 64 / Q;
        float *tile = reinterpret_cast<float *>(lds) + wave * (32 * N);
        const int q = lane % Q, pl = lane / Q;
        float bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bi[j] = bias ? bias[4 * q + j] : 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            __syncthreads();   // the W image (m = 0) or the previous row (m = 1) has been read
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
                    v[j] = v[j] + bi[j];
                    if (relu) v[j] = fmaxf(v[j], 0.0f);
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
        const float bi = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int y = ty0 + wave * 2 + m;
            if (y >= H) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int x = tx0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (x >= W) continue;
                float v = acc[m][nb][e] + bi;
                if (relu) v = fmaxf(v, 0.0f);
                if (of) of[(int)(y * d.of_ys + x * d.of_xs) + n] = v;
                if (ob) ob[(int)(y * d.ob_ys + x * d.ob_xs) + n] = bf16_bits(v);
            }
        }
    }
}

// [lo, hi) element extent of a strided NHWC tensor with C channels addressed
int64_t extent(int B, int H, int W, int64_t C, int64_t bs, int64_t ys, int64_t xs) {
    return (int64_t)(B - 1) * bs + (int64_t)(H - 1) * ys + (int64_t)(W - 1) * xs + C;
}

// strides of one tensor whose pixels hold C addressed channels: x stride >= C, y stride >= x stride, batch stride >= 0, one image below
// 2^31 elements
const char *bad_strides(int H, int W, int64_t C, int64_t bs, int64_t ys, int64_t xs) {
    if (xs < C) return "x stride smaller than the channels addressed";
    if (ys < xs || bs < 0) return "y stride smaller than the x stride, or a negative batch stride";
    if (ys > INT32_MAX || extent(1, H, W, xs, 0, ys, xs) > INT32_MAX) return "one image spans 2^31 elements or more (32-bit offsets inside an image)";
    return nullptr;
}

}  // namespace

extern "C" int mit_aot_conv3x3_bf16(const MitAotConv *dp, void *stream) {
    if (!dp) return mit_set_error("mit_aot_conv3x3_bf16: null descriptor");
    const MitAotConv &d = *dp;
    if (!d.in) return mit_set_error("mit_aot_conv3x3_bf16: null pointer (in)");
    if (!d.out_f32 && !d.out_bf16) return mit_set_error("mit_aot_conv3x3_bf16: null pointer (no output: out_f32 and out_bf16 are both NULL)");
    if (d.groups < 1 || d.groups > MIT_AOT_MAX_GROUPS)
        return mit_set_error("mit_aot_conv3x3_bf16: groups must be in [1, %d] (got %d)", MIT_AOT_MAX_GROUPS, d.groups);
    if (d.B <= 0 || d.H <= 0 || d.W <= 0) return mit_set_error("mit_aot_conv3x3_bf16: sizes must be positive (B %d, H %d, W %d)", d.B, d.H, d.W);
    if (d.Cin % CK != 0 || d.Cin < 32 || d.Cin > 512)
        return mit_set_error("mit_aot_conv3x3_bf16: Cin must be a multiple of 32 in [32, 512] (got %d)", d.Cin);
    if (d.N != 32 && d.N != 128) return mit_set_error("mit_aot_conv3x3_bf16: N must be 32 or 128 (got %d)", d.N);
    if (d.act != MIT_ACT_NONE && d.act != MIT_ACT_RELU) return mit_set_error("mit_aot_conv3x3_bf16: act must be none or relu (got %d)", d.act);
    int64_t top = 0;   // channels addressed through an output pixel
    for (int g = 0; g < d.groups; ++g) {
        if (!d.w[g]) return mit_set_error("mit_aot_conv3x3_bf16: null pointer (w of group %d)", g);
        if (reinterpret_cast<uintptr_t>(d.w[g]) % 16) return mit_set_error("mit_aot_conv3x3_bf16: w of group %d must be 16-byte aligned", g);
        if (d.rate[g] < 1 || d.rate[g] > MIT_AOT_MAX_RATE)
            return mit_set_error("mit_aot_conv3x3_bf16: rate must be in [1, %d] (group %d: %d)", MIT_AOT_MAX_RATE, g, d.rate[g]);
        if (d.rate[g] >= d.H || d.rate[g] >= d.W)
            return mit_set_error("mit_aot_conv3x3_bf16: reflect padding needs H, W > rate (group %d: rate %d, H %d, W %d)", g, d.rate[g], d.H, d.W);
        if (d.out_c0[g] < 0) return mit_set_error("mit_aot_conv3x3_bf16: negative output channel offset (group %d: %d)", g, d.out_c0[g]);
        for (int k = 0; k < g; ++k)
            if (d.out_c0[g] < d.out_c0[k] + d.N && d.out_c0[k] < d.out_c0[g] + d.N)
                return mit_set_error("mit_aot_conv3x3_bf16: the output slices of groups %d and %d overlap", k, g);
        if (top < (int64_t)d.out_c0[g] + d.N) top = (int64_t)d.out_c0[g] + d.N;
    }
    const char *why;
    if ((why = bad_strides(d.H, d.W, d.Cin, d.in_bs, d.in_ys, d.in_xs))) return mit_set_error("mit_aot_conv3x3_bf16: input strides: %s", why);
    if (d.out_f32 && (why = bad_strides(d.H, d.W, top, d.of_bs, d.of_ys, d.of_xs)))
        return mit_set_error("mit_aot_conv3x3_bf16: out_f32 slice overruns its buffer or bad strides: %s", why);
    if (d.out_bf16 && (why = bad_strides(d.H, d.W, top, d.ob_bs, d.ob_ys, d.ob_xs)))
        return mit_set_error("mit_aot_conv3x3_bf16: out_bf16 slice overruns its buffer or bad strides: %s", why);
    if (reinterpret_cast<uintptr_t>(d.in) % 16 || d.in_xs % 8 || d.in_ys % 8 || d.in_bs % 8)
        return mit_set_error("mit_aot_conv3x3_bf16: in must be 16-byte aligned and the input strides multiples of 8 elements");
    if (mit_div_up(d.H, TH) > 65535 || (int64_t)d.B * d.groups > 65535)
        return mit_set_error("mit_aot_conv3x3_bf16: at most 65535 tile rows and 65535 (image, group) pairs a launch (grid y / z)");
    if (d.out_bf16) {
        // byte addresses as integers
        const int64_t din = (int64_t)(reinterpret_cast<intptr_t>(d.out_bf16) - reinterpret_cast<intptr_t>(d.in)) / 2;
        if (din < extent(d.B, d.H, d.W, d.Cin, d.in_bs, d.in_ys, d.in_xs) && -din < extent(d.B, d.H, d.W, top, d.ob_bs, d.ob_ys, d.ob_xs))
            return mit_set_error("mit_aot_conv3x3_bf16: out_bf16 overlaps the input");
    }
    const dim3 grid((unsigned)mit_div_up(d.W, TW), (unsigned)mit_div_up(d.H, TH), (unsigned)(d.B * d.groups));
    const double px = (double)d.B * d.H * d.W;
    // the wide epilogue: the fp32 output on 16 bytes, the bf16 output on 8, every stride and channel offset a multiple of four elements
    auto wide = [&](const void *p, int64_t bs, int64_t ys, int64_t xs, int align) {
        return !p || (reinterpret_cast<uintptr_t>(p) % align == 0 && bs % 4 == 0 && ys % 4 == 0 && xs % 4 == 0);
    };
    bool vec = wide(d.out_f32, d.of_bs, d.of_ys, d.of_xs, 16) && wide(d.out_bf16, d.ob_bs, d.ob_ys, d.ob_xs, 8);
    for (int g = 0; g < d.groups; ++g) vec = vec && d.out_c0[g] % 4 == 0;
    const auto kern = d.N == 128 ? (vec ? aot_conv3x3_kernel<128, true> : aot_conv3x3_kernel<128, false>)
                                 : (vec ? aot_conv3x3_kernel<32, true> : aot_conv3x3_kernel<32, false>);
    MitProbeScope probe(d.N == 128 ? "aot_conv3x3_kernel<128>" : "aot_conv3x3_kernel<32>", (hipStream_t)stream,
                        px * (2.0 * d.Cin + d.groups * d.N * ((d.out_bf16 ? 2.0 : 0.0) + (d.out_f32 ? 4.0 : 0.0))) + 18.0 * d.Cin * d.N * d.groups,
                        px * 18.0 * d.Cin * d.N * d.groups);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, (hipStream_t)stream, d);
    MIT_CHECK_LAUNCH("mit_aot_conv3x3_bf16");
    return 0;
}
