// mc2_bf16.hip — the plain 3x3 convolution on bf16-resident activations for the mc2 colorizer's bf16 precision: FFDNet's chain of
// 3x3 convolutions at 96 features (colorization/manga_colorization_v2_utils/denoising/models.py) with the folded BatchNorm and the ReLU
// in the epilogue.  v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue (mit_hip.h has the arithmetic).
//
// The tile (256 lanes, 8 x 32 output pixels, chunks of 32 input channels), the A image (the zero-padded halo of the tile), the W image,
// the MFMA step and the epilogue's stores are conv3x3_bf16_tile.h's; this unit adds N = 96 and the scale / bias / ReLU epilogue.
// LDS = 27200 + 36 * (N * 16 + 16) bytes: 46208 at N = 32 and 64640 at N = 64 (two workgroups a CU), 83072 at N = 96 — above the 64 KB
// a kernel gets without asking, so the LDS is dynamic and the N = 96 instantiation opts in (one workgroup a CU).  The next chunk's
// global loads are issued before the MFMAs of the current one and written to LDS after them.
// Accumulation order of a pixel: chunk, tap, channel — fixed, whatever the batch or the tile.
#include "conv3x3_bf16_tile.h"

namespace {

using namespace conv3x3;

static_assert(MIT_CONV3X3_TILE_H == TH && MIT_CONV3X3_TILE_W == TW, "the exported tile sides are the tile's");

template <int N>
constexpr int lds_bytes() {
    return HaloImage::BYTES + WImage<N>::BYTES;
}
static_assert(HaloImage::BYTES % 16 == 0, "the W image starts on a 16-byte boundary");
static_assert(lds_bytes<32>() >= store_tile_bytes<32>() && lds_bytes<64>() >= store_tile_bytes<64>() && lds_bytes<96>() >= store_tile_bytes<96>(),
              "the epilogue's tile fits the K loop's images");
static_assert(lds_bytes<64>() <= 64 * 1024 && lds_bytes<96>() <= 160 * 1024, "N <= 64: two workgroups a CU; N = 96: one");

struct ChanConst {
    float sc, bi;
};

// VEC: the wide form of the epilogue (store_tile).
template <int N, bool VEC>
__global__ __launch_bounds__(THREADS, N == 96 ? 1 : 2) void conv3x3_bf16_kernel(const MitConv3x3Bf16 d) {
    constexpr int NB = N / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int64_t b = blockIdx.z;
    const int H = d.H, W = d.W, Cin = d.Cin;
    const uint16_t *in = d.in + b * d.in_bs;

    HaloImage ai(lds, H, W, ty0, tx0, d.in_ys, d.in_xs);
    WImage<N> wi(lds + HaloImage::BYTES, Cin);

    f32x16 acc[2][NB];
    clear(acc);

    ai.fetch(in, 0);
    wi.fetch(d.w, 0);
    for (int c0 = 0; c0 < Cin; c0 += CK) {
        __syncthreads();   // the previous chunk's fragments have been read
        ai.stage();
        wi.stage();
        __syncthreads();
        if (c0 + CK < Cin) {
            ai.fetch(in, c0 + CK);
            wi.fetch(d.w, c0 + CK);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int s = 0; s < 2; ++s) mfma_step(acc, wi, tap, s, ai.frag(0, dy, dx, s), ai.frag(1, dy, dx, s));
        }
    }

    // the epilogue's operands as locals, which the functors below copy (store_tile says why)
    const int act = d.act;
    const float alpha = d.act_alpha;
    const float *scale = d.scale, *bias = d.bias;
    float *of = d.out_f32 ? d.out_f32 + b * d.of_bs : nullptr;
    uint16_t *ob = d.out_bf16 ? d.out_bf16 + b * d.ob_bs : nullptr;
    auto chan = [=](int n) { return ChanConst{scale ? scale[n] : 1.0f, bias ? bias[n] : 0.0f}; };
    // scale, bias, activation: one rounded operation after the other, in this order in both forms
    auto fin = [=](auto &v, const auto &k, int, int, int) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = v[j] * k[j].sc + k[j].bi;
                if (act == MIT_ACT_RELU) v[j] = fmaxf(v[j], 0.0f);
                if (act == MIT_ACT_LEAKY) v[j] = v[j] >= 0.0f ? v[j] : v[j] * alpha;
            }
        } else {
            v = v * k.sc + k.bi;
            if (act == MIT_ACT_RELU) v = fmaxf(v, 0.0f);
            if (act == MIT_ACT_LEAKY) v = v >= 0.0f ? v : v * alpha;
        }
    };
    store_tile<N, VEC>(acc, lds, TileOut{H, W, ty0, tx0, of, d.of_ys, d.of_xs, ob, d.ob_ys, d.ob_xs}, chan, fin);
}

const char *bad_strides(const MitConv3x3Bf16 &d, int C, int64_t bs, int64_t ys, int64_t xs) {
    return conv3x3::bad_strides(d.H, d.W, C, C, bs, ys, xs, "x stride smaller than the channel count");
}

template <int N>
int launch(const MitConv3x3Bf16 &d, bool vec, const dim3 grid, hipStream_t stream) {
    static DynSmemOptIn optin[2];
    const auto kern = vec ? conv3x3_bf16_kernel<N, true> : conv3x3_bf16_kernel<N, false>;
    optin[vec].ensure(reinterpret_cast<const void *>(kern), lds_bytes<N>());
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), lds_bytes<N>(), stream, d);
    MIT_CHECK_LAUNCH("mit_conv3x3_bf16");
    return 0;
}

}  // namespace

extern "C" int mit_conv3x3_bf16(const MitConv3x3Bf16 *dp, void *stream) {
    const char *fn = "mit_conv3x3_bf16";
    if (!dp) return mit_set_error("mit_conv3x3_bf16: null descriptor");
    const MitConv3x3Bf16 &d = *dp;
    if (!d.in || !d.w) return mit_set_error("mit_conv3x3_bf16: null pointer (in / w)");
    if (check_outputs(fn, d) || check_sizes(fn, d)) return 1;
    if (d.Cin % CK != 0 || d.Cin < 32 || d.Cin > 192)
        return mit_set_error("mit_conv3x3_bf16: Cin must be a multiple of 32 in [32, 192] (got %d)", d.Cin);
    if (d.N != 32 && d.N != 64 && d.N != 96) return mit_set_error("mit_conv3x3_bf16: N must be 32, 64 or 96 (got %d)", d.N);
    if (d.act != MIT_ACT_NONE && d.act != MIT_ACT_RELU && d.act != MIT_ACT_LEAKY)
        return mit_set_error("mit_conv3x3_bf16: act must be none, relu or leaky (got %d)", d.act);
    const char *why;
    if ((why = bad_strides(d, d.Cin, d.in_bs, d.in_ys, d.in_xs))) return mit_set_error("mit_conv3x3_bf16: input strides: %s", why);
    if (d.out_f32 && (why = bad_strides(d, d.N, d.of_bs, d.of_ys, d.of_xs))) return mit_set_error("mit_conv3x3_bf16: out_f32 strides: %s", why);
    if (d.out_bf16 && (why = bad_strides(d, d.N, d.ob_bs, d.ob_ys, d.ob_xs))) return mit_set_error("mit_conv3x3_bf16: out_bf16 strides: %s", why);
    if (check_alignment_and_grid(fn, d, d.w, d.B, "images")) return 1;
    if (d.out_bf16) {
        const int64_t din = out_bf16_offset(d);   // the two may be one buffer or two
        bool overlap;
        if (d.ob_bs == d.in_bs && d.ob_ys == d.in_ys && d.ob_xs == d.in_xs && din > -d.in_xs && din < d.in_xs)
            overlap = din > -(int64_t)d.N && din < d.Cin;   // one buffer, same pixel grid: the channel ranges [0, Cin) and [din, din + N)
        else
            overlap = extents_overlap(d, din, d.N);
        if (overlap) return mit_set_error("mit_conv3x3_bf16: out_bf16 overlaps the input channels it is computed from");
    }
    const dim3 grid((unsigned)mit_div_up(d.W, TW), (unsigned)mit_div_up(d.H, TH), (unsigned)d.B);
    const double px = (double)d.B * d.H * d.W;
    const bool vec = wide(d.out_f32, d.of_bs, d.of_ys, d.of_xs, 16) && wide(d.out_bf16, d.ob_bs, d.ob_ys, d.ob_xs, 8);
    MitProbeScope probe(d.N == 96 ? "conv3x3_bf16_kernel<96>" : (d.N == 64 ? "conv3x3_bf16_kernel<64>" : "conv3x3_bf16_kernel<32>"), (hipStream_t)stream,
                        px * (2.0 * d.Cin + (d.out_bf16 ? 2.0 : 0.0) * d.N + (d.out_f32 ? 4.0 : 0.0) * d.N) + 18.0 * d.Cin * d.N,
                        px * 18.0 * d.Cin * d.N);
    if (d.N == 96) return launch<96>(d, vec, grid, (hipStream_t)stream);
    if (d.N == 64) return launch<64>(d, vec, grid, (hipStream_t)stream);
    return launch<32>(d, vec, grid, (hipStream_t)stream);
}
