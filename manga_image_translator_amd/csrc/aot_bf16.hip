// aot_bf16.hip — the 3x3 convolutions of the AOT generator's blocks (AOTBlock, inpainting/inpainting_aot.py:170-193) for the inpainter's
// bf16 precision: the four dilated branches 128 -> 32 (rates 2, 4, 8, 16; ReflectionPad2d(rate)) as ONE launch of four groups, and the
// fuse / gate convolutions 128 -> 128 (rate 1), on bf16-RESIDENT operands, v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue
// (mit_hip.h has the arithmetic).
//
// The tile (256 lanes, 8 x 32 output pixels of one (image, group), chunks of 32 input channels), the W image, the MFMA step and the
// epilogue's stores are conv3x3_bf16_tile.h's.  The W image is 36 * (N * 16 + 16) bytes: 19008 at N = 32, 74304 at N = 128; the next
// chunk's weight rows are requested before the MFMAs of the current one and written to LDS after them.  This kernel's A operand:
//   A  one of two forms, chosen per workgroup from its group's rate alone (so a launch of four groups mixes them):
//      staged   the region the nine windows of the tile touch — columns tx0 - rate .. tx0 + 31 + rate of the rows ty0 - rate ..
//               ty0 + 7 + rate (rate <= 8) or of three 8-row bands (larger rates) — goes to LDS once per chunk, reflected, 80 padded
//               bytes a pixel, and serves all nine taps.  The global loads are whole 64-byte pixel chunks by four neighbouring lanes.
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
#include <type_traits>
#include "conv3x3_bf16_tile.h"

namespace {

using namespace conv3x3;

constexpr int PF = 3;                                      // taps the A fragments are requested ahead (direct form)
constexpr int AR = 10;                                     // rounds of 256 16-byte units the staged form's A image holds: 640 region pixels
static_assert(9 % PF == 0, "a tap keeps its ring slot from chunk to chunk");

// ReflectionPad2d: p in [-rate, L - 1 + rate] with rate <= L - 1
__device__ __forceinline__ int reflect(int p, int L) { return p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p); }

// VEC: the wide form of the epilogue (store_tile).
template <int N, bool VEC>
__global__ __launch_bounds__(THREADS, N == 32 ? 2 : 1) void aot_conv3x3_kernel(const MitAotConv d) {
    constexpr int NB = N / 32;
    constexpr int A_BYTES = AR * (THREADS / 4) * PIX_B;   // room for AR * 64 region pixels
    constexpr int K_BYTES = A_BYTES + WImage<N>::BYTES, E_BYTES = store_tile_bytes<N>();
    __shared__ u32x4 lds[(K_BYTES > E_BYTES ? K_BYTES : E_BYTES) / 16];
    unsigned char *ldsA = reinterpret_cast<unsigned char *>(lds);

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
    WImage<N> wi(ldsA + A_BYTES, Cin);

    f32x16 acc[2][NB];
    clear(acc);

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

        wi.fetch(wt, 0);
        if (ST) {
            fetch_region(0);
        } else {
#pragma unroll
            for (int t = 0; t < PF; ++t) fetch_a(t, 0, t);
        }
        for (int c0 = 0; c0 < Cin; c0 += CK) {
            __syncthreads();   // the previous chunk's fragments have been read
            wi.stage();
            if (ST) stage_region();
            __syncthreads();
            const bool more = c0 + CK < Cin;
            if (more) wi.fetch(wt, c0 + CK);
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
                for (int s = 0; s < 2; ++s) mfma_step(acc, wi, tap, s, fa[0][s], fa[1][s]);
            }
        }
    };
    if (staged)
        k_loop(std::true_type{});
    else
        k_loop(std::false_type{});

    const int act = d.act;
    const int oc0 = d.out_c0[g];
    const float *bias = d.bias[g];
    float *of = d.out_f32 ? d.out_f32 + b * d.of_bs + oc0 : nullptr;
    uint16_t *ob = d.out_bf16 ? d.out_bf16 + b * d.ob_bs + oc0 : nullptr;
    auto chan = [=](int n) { return bias ? bias[n] : 0.0f; };
    // bias, then ReLU: in this order in both forms
    auto fin = [=](auto &v, const auto &k, int, int, int) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = v[j] + k[j];
                if (act == MIT_ACT_RELU) v[j] = fmaxf(v[j], 0.0f);
            }
        } else {
            v = v + k;
            if (act == MIT_ACT_RELU) v = fmaxf(v, 0.0f);
        }
    };
    store_tile<N, VEC>(acc, lds, TileOut{H, W, ty0, tx0, of, d.of_ys, d.of_xs, ob, d.ob_ys, d.ob_xs}, chan, fin);
}

// a tensor whose pixels hold C addressed channels; its span is counted in whole pixels
const char *bad_strides(const MitAotConv &d, int64_t C, int64_t bs, int64_t ys, int64_t xs) {
    return conv3x3::bad_strides(d.H, d.W, C, xs, bs, ys, xs, "x stride smaller than the channels addressed");
}

}  // namespace

extern "C" int mit_aot_conv3x3_bf16(const MitAotConv *dp, void *stream) {
    const char *fn = "mit_aot_conv3x3_bf16";
    if (!dp) return mit_set_error("mit_aot_conv3x3_bf16: null descriptor");
    const MitAotConv &d = *dp;
    if (!d.in) return mit_set_error("mit_aot_conv3x3_bf16: null pointer (in)");
    if (check_outputs(fn, d)) return 1;
    if (d.groups < 1 || d.groups > MIT_AOT_MAX_GROUPS)
        return mit_set_error("mit_aot_conv3x3_bf16: groups must be in [1, %d] (got %d)", MIT_AOT_MAX_GROUPS, d.groups);
    if (check_sizes(fn, d)) return 1;
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
    if ((why = bad_strides(d, d.Cin, d.in_bs, d.in_ys, d.in_xs))) return mit_set_error("mit_aot_conv3x3_bf16: input strides: %s", why);
    if (d.out_f32 && (why = bad_strides(d, top, d.of_bs, d.of_ys, d.of_xs)))
        return mit_set_error("mit_aot_conv3x3_bf16: out_f32 slice overruns its buffer or bad strides: %s", why);
    if (d.out_bf16 && (why = bad_strides(d, top, d.ob_bs, d.ob_ys, d.ob_xs)))
        return mit_set_error("mit_aot_conv3x3_bf16: out_bf16 slice overruns its buffer or bad strides: %s", why);
    if (check_alignment_and_grid(fn, d, nullptr, (int64_t)d.B * d.groups, "(image, group) pairs")) return 1;
    if (d.out_bf16 && extents_overlap(d, out_bf16_offset(d), top)) return mit_set_error("mit_aot_conv3x3_bf16: out_bf16 overlaps the input");
    const dim3 grid((unsigned)mit_div_up(d.W, TW), (unsigned)mit_div_up(d.H, TH), (unsigned)(d.B * d.groups));
    const double px = (double)d.B * d.H * d.W;
    // the wide epilogue: every channel offset a multiple of four elements as well
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
