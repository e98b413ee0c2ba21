// rdb_bf16.hip — the 3x3 convolutions of ESRGAN's residual dense blocks (ResidualDenseBlock_5C, upscaling/esrgan_pytorch.py:152-166) for the
// upscaler's bf16 precision: bf16-RESIDENT activations, v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue (mit_hip.h has the
// arithmetic).  Plus the channel-slice cast that puts an fp32 tensor into the dense-block buffer.
//
// Why a kernel of its own: the layers are narrow (N = 32 or 64, K = 9 * Cin <= 1728).  On the conv_gemm tiles every one of the nine taps
// re-reads its fp32 activations from cache and re-rounds them; here a dense block's activations live in HBM as bf16 (every consumer of
// x, x1 .. x4 is a convolution that would round them anyway), and a workgroup stages each input element to LDS ONCE per launch.
//
// The tile (256 lanes, 8 x 32 output pixels, chunks of 32 input channels), the W image, the MFMA step and the epilogue's stores are
// conv3x3_bf16_tile.h's.  This kernel's A operand is the zero-padded halo of the tile:
//   A image  [10 x 34 halo pixels][32 ch] bf16, 80 bytes a pixel.
// 27200 + 36 * (N * 16 + 16) bytes = 64640 at N = 64: static LDS, two workgroups a CU.  The next chunk's global loads are issued before the
// MFMAs of the current one and written to LDS after them, so the loads travel under 18 k-steps of 2 x N / 32 MFMAs.
// Accumulation order of a pixel: chunk, tap, channel — fixed, whatever the batch or the tile.
#include "conv3x3_bf16_tile.h"

namespace {

using namespace conv3x3;

constexpr int HH = TH + 2, HW = TW + 2, HALO = HH * HW;   // 10 x 34 = 340 halo pixels
constexpr int A_BYTES = HALO * PIX_B;                      // 27200
constexpr int A_UNITS = HALO * (CK / 8);                   // 16-byte units of the A image: 1360
constexpr int A_ROUNDS = (A_UNITS + THREADS - 1) / THREADS;
static_assert(A_BYTES % 16 == 0, "the W image starts on a 16-byte boundary");
static_assert(A_BYTES + WImage<32>::BYTES >= store_tile_bytes<32>() && A_BYTES + WImage<64>::BYTES >= store_tile_bytes<64>(),
              "the epilogue's tile fits the K loop's images");

struct ChanConst {
    float sc, bi;
};

// VEC: the wide form of the epilogue (store_tile), which also reads post and post2 with 16-byte loads.
template <int N, bool VEC>
__global__ __launch_bounds__(THREADS, 2) void rdb_conv3x3_kernel(const MitRdbConv d) {
    constexpr int NB = N / 32;
    __shared__ u32x4 lds[(A_BYTES + WImage<N>::BYTES) / 16];
    unsigned char *ldsA = reinterpret_cast<unsigned char *>(lds);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int64_t b = blockIdx.z;
    const int H = d.H, W = d.W, Cin = d.Cin;
    const uint16_t *in = d.in + b * d.in_bs;

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
    WImage<N> wi(ldsA + A_BYTES, Cin);

    u32x4 a_reg[A_ROUNDS];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < A_ROUNDS; ++i) {
            a_reg[i] = u32x4{0u, 0u, 0u, 0u};
            if (a_off[i] >= 0) a_reg[i] = *reinterpret_cast<const u32x4 *>(in + a_off[i] + c0);
        }
        wi.fetch(d.w, c0);
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < A_ROUNDS; ++i) {
            const int u = tid + i * THREADS;
            if (a_off[i] != -2) *reinterpret_cast<u32x4 *>(ldsA + (u >> 2) * PIX_B + (u & 3) * 16) = a_reg[i];
        }
        wi.stage();
    };

    f32x16 acc[2][NB];
    clear(acc);

    const unsigned char *a_base = ldsA + ((wave * 2) * HW + r) * PIX_B + h * 16;   // this lane's A fragment at tap (0, 0), k-step 0

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
                bf16x8 fa[2];
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    fa[m] = *reinterpret_cast<const bf16x8 *>(a_base + ((m + dy) * HW + dx) * PIX_B + s * 32);
                mfma_step(acc, wi, tap, s, fa[0], fa[1]);
            }
        }
    }

    // the epilogue's operands as locals, which the functors below copy (store_tile says why)
    const int act = d.act;
    const float alpha = d.act_alpha, s2 = d.s2;
    const float *scale = d.scale, *bias = d.bias;
    const float *post = d.post ? d.post + b * d.post_bs : nullptr;
    const float *post2 = d.post2 ? d.post2 + b * d.post2_bs : nullptr;
    const int64_t p_ys = d.post_ys, p_xs = d.post_xs, p2_ys = d.post2_ys, p2_xs = d.post2_xs;
    float *of = d.out_f32 ? d.out_f32 + b * d.of_bs : nullptr;
    uint16_t *ob = d.out_bf16 ? d.out_bf16 + b * d.ob_bs : nullptr;
    auto chan = [=](int n) { return ChanConst{scale ? scale[n] : 1.0f, bias ? bias[n] : 0.0f}; };
    // scale, bias, LeakyReLU, post, then * s2 + post2: one rounded operation after the other, in this order in both forms
    auto fin = [=](auto &v, const auto &k, int n, int y, int x) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = v[j] * k[j].sc + k[j].bi;
                if (act == MIT_ACT_LEAKY) v[j] = v[j] >= 0.0f ? v[j] : v[j] * alpha;
            }
            if (post) {
                const f32x4 p4 = *reinterpret_cast<const f32x4 *>(post + (int)(y * p_ys + x * p_xs) + n);
                v[0] = v[0] + p4.x, v[1] = v[1] + p4.y, v[2] = v[2] + p4.z, v[3] = v[3] + p4.w;
            }
            if (post2) {
                const f32x4 p4 = *reinterpret_cast<const f32x4 *>(post2 + (int)(y * p2_ys + x * p2_xs) + n);
                v[0] = v[0] * s2 + p4.x, v[1] = v[1] * s2 + p4.y, v[2] = v[2] * s2 + p4.z, v[3] = v[3] * s2 + p4.w;
            }
        } else {
            v = v * k.sc + k.bi;
            if (act == MIT_ACT_LEAKY) v = v >= 0.0f ? v : v * alpha;
            if (post) v = v + post[(int)(y * p_ys + x * p_xs) + n];
            if (post2) v = v * s2 + post2[(int)(y * p2_ys + x * p2_xs) + n];
        }
    };
    store_tile<N, VEC>(acc, lds, TileOut{H, W, ty0, tx0, of, d.of_ys, d.of_xs, ob, d.ob_ys, d.ob_xs}, chan, fin);
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

const char *bad_strides(const MitRdbConv &d, int C, int64_t bs, int64_t ys, int64_t xs) {
    return conv3x3::bad_strides(d.H, d.W, C, C, bs, ys, xs, "x stride smaller than the channel count");
}

}  // namespace

extern "C" int mit_rdb_conv3x3_bf16(const MitRdbConv *dp, void *stream) {
    const char *fn = "mit_rdb_conv3x3_bf16";
    if (!dp) return mit_set_error("mit_rdb_conv3x3_bf16: null descriptor");
    const MitRdbConv &d = *dp;
    if (!d.in || !d.w) return mit_set_error("mit_rdb_conv3x3_bf16: null pointer (in / w)");
    if (check_outputs(fn, d) || check_sizes(fn, d)) return 1;
    if (d.Cin % CK != 0 || d.Cin < 64 || d.Cin > 192)
        return mit_set_error("mit_rdb_conv3x3_bf16: Cin must be a multiple of 32 in [64, 192] (got %d)", d.Cin);
    if (d.N != 32 && d.N != 64) return mit_set_error("mit_rdb_conv3x3_bf16: N must be 32 or 64 (got %d)", d.N);
    if (d.act != MIT_ACT_NONE && d.act != MIT_ACT_LEAKY) return mit_set_error("mit_rdb_conv3x3_bf16: act must be none or leaky (got %d)", d.act);
    const char *why;
    if ((why = bad_strides(d, d.Cin, d.in_bs, d.in_ys, d.in_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: input strides: %s", why);
    if (d.post && (why = bad_strides(d, d.N, d.post_bs, d.post_ys, d.post_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: post strides: %s", why);
    if (d.post2 && (why = bad_strides(d, d.N, d.post2_bs, d.post2_ys, d.post2_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: post2 strides: %s", why);
    if (d.out_f32 && (why = bad_strides(d, d.N, d.of_bs, d.of_ys, d.of_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: out_f32 strides: %s", why);
    if (d.out_bf16 && (why = bad_strides(d, d.N, d.ob_bs, d.ob_ys, d.ob_xs))) return mit_set_error("mit_rdb_conv3x3_bf16: out_bf16 strides: %s", why);
    if (check_alignment_and_grid(fn, d, d.w, d.B, "images")) return 1;
    if (d.out_bf16) {
        const int64_t din = out_bf16_offset(d);   // the two may be one buffer (the dense block's) or two
        bool overlap;
        if (d.ob_bs == d.in_bs && d.ob_ys == d.in_ys && d.ob_xs == d.in_xs && din > -d.in_xs && din < d.in_xs)
            overlap = din > -(int64_t)d.N && din < d.Cin;   // one buffer, same pixel grid: the channel ranges [0, Cin) and [din, din + N)
        else
            overlap = extents_overlap(d, din, d.N);
        if (overlap) return mit_set_error("mit_rdb_conv3x3_bf16: out_bf16 overlaps the input channels it is computed from");
    }
    const dim3 grid((unsigned)mit_div_up(d.W, TW), (unsigned)mit_div_up(d.H, TH), (unsigned)d.B);
    const double px = (double)d.B * d.H * d.W;
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
