// conv3x3_bf16_tile.h — what the bf16-resident 3x3 convolutions (rdb_bf16.hip, aot_bf16.hip, mc2_bf16.hip) have in common: the tile
// geometry, the W image, the MFMA step of a (tap, k-step), the two store forms of the epilogue, and the host checks on strided NHWC
// tensors.  A kernel adds its A operand (where a lane's A fragments come from; HaloImage is mc2_bf16.hip's — rdb_bf16.hip keeps its own
// copy of the same staging, because rewriting it on the struct changed its device code), its pointwise epilogue and its own argument
// rules.
//
// Workgroup = THREADS = 256 lanes = 4 waves, one tile of TH x TW = 8 x 32 output pixels; wave w owns rows 2w, 2w + 1 (two 32-pixel MFMA
// row blocks) and all N columns: 2 x N / 32 accumulators of 16 registers.  The K loop walks chunks of CK = 32 input channels, nine taps
// a chunk, two k-steps of v_mfma_f32_32x32x16_bf16 a tap.  An A image in LDS gives a pixel PIX_B = 80 bytes (64 of data + 16 of pad: the
// 16 lanes of a ds_read_b128 group then fall on 16 different 16-byte bank slots — 5 r mod 16 is a bijection over each group's rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "bf16_split.h"
#include "common.h"

namespace conv3x3 {

using mitcg::bf16x8;
using mitcg::u32x4;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TH = 8, TW = 32;
constexpr int CK = 32;             // input channels a chunk
constexpr int THREADS = 256;
constexpr int KG = 9 * CK / 8;     // k-groups (8 rows) of a chunk's weights: 36
constexpr int PIX_B = 80;          // LDS bytes a pixel of an A image
static_assert(MIT_RDB_TILE_H == TH && MIT_RDB_TILE_W == TW && MIT_AOT_TILE_H == TH && MIT_AOT_TILE_W == TW,
              "a wave owns two 32-pixel rows of the tile");

__device__ __forceinline__ unsigned short bf16_bits(float v) {   // round to nearest even (v_cvt_pk_bf16_f32)
    return (unsigned short)(mitcg::pack_bf16(v, 0.0f) & 0xffffu);
}

// W image of a chunk: [9 taps x 4 k-groups][N] cells of 16 bytes = 8 consecutive k of one output column, which is the B fragment of a
// lane; a k-group's row of N cells is followed by 16 bytes of pad.  The packed weight is [9 * Cin][N] row-major, so a lane takes 8 rows
// x 8 columns (eight 16-byte loads), transposes them in registers and writes eight cells.  Eight consecutive lanes (one ds_write_b128
// group) hold eight k-groups of the same columns: with the pad their cells fall on eight different 16-byte slots (the same k-group in
// neighbouring lanes would put all eight on one slot), while a load instruction of the wave still reads whole 128-byte weight rows.
// fetch() requests a chunk's rows into registers and stage() writes them to LDS, so that a kernel can put the MFMAs of the previous
// chunk between the two.
template <int N>
struct WImage {
    static constexpr int NB = N / 32, NG = N / 8;
    static constexpr int ROW = N * 16 + 16;                      // bytes of a k-group's row of cells, padded
    static constexpr int BYTES = KG * ROW;
    static constexpr int SLOTS = (KG + 7) / 8 * 8 * NG;          // task slots: 8 k-groups x NG column groups a block
    static constexpr int ROUNDS = (SLOTS + THREADS - 1) / THREADS;

    unsigned char *lds;
    const unsigned char *frag0;        // this lane's B fragment at tap 0, k-step 0, column block 0
    int off[ROUNDS], cell[ROUNDS];     // a task = (k-group, column group): rows (tap * Cin + c8 .. + 7), columns ng * 8 .. + 7
    u32x4 reg[ROUNDS][8];

    __device__ __forceinline__ WImage(unsigned char *ldsW, int Cin) : lds(ldsW) {
        const int tid = threadIdx.x, lane = tid & 63;
        frag0 = ldsW + (lane >> 5) * ROW + (lane & 31) * 16;
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {   // k-group fastest over the lanes
            const int task = tid + i * THREADS;
            const int kg = (task & 7) + 8 * (task / (8 * NG)), ng = (task >> 3) % NG;
            const int tap = kg >> 2, c8 = (kg & 3) * 8;
            off[i] = kg < KG ? (tap * Cin + c8) * N + ng * 8 : -1;
            cell[i] = kg * ROW + ng * 128;
        }
    }
    __device__ __forceinline__ void fetch(const uint16_t *wt, int c0) {
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i)
            if (off[i] >= 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) reg[i][j] = *reinterpret_cast<const u32x4 *>(wt + off[i] + (c0 + j) * N);
            }
    }
    __device__ __forceinline__ void stage() {
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i)
            if (off[i] >= 0) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {   // column c of the 8 x 8 block: rows 2q, 2q + 1 share dword q of the cell
                    u32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned lo = reg[i][2 * q][c >> 1], hi = reg[i][2 * q + 1][c >> 1];
                        v[q] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
                    }
                    *reinterpret_cast<u32x4 *>(lds + cell[i] + c * 16) = v;
                }
            }
    }
    __device__ __forceinline__ bf16x8 frag(int tap, int s, int nb) const {
        return *reinterpret_cast<const bf16x8 *>(frag0 + (tap * 4 + 2 * s) * ROW + nb * 512);
    }
};

// A image of a chunk for the plain 3x3 (pad 1, no dilation): the tile plus its one-pixel halo, [10 x 34 halo pixels][32 ch] bf16 at
// PIX_B bytes a pixel, zeros outside the image.  A lane stages ROUNDS 16-byte units (unit u = pixel * 4 + part); fetch() / stage()
// split as WImage's do.
struct HaloImage {
    static constexpr int HH = TH + 2, HW = TW + 2, HALO = HH * HW;   // 340 halo pixels
    static constexpr int BYTES = HALO * PIX_B;                       // 27200
    static constexpr int UNITS = HALO * (CK / 8);                    // 1360
    static constexpr int ROUNDS = (UNITS + THREADS - 1) / THREADS;

    unsigned char *lds;
    int off[ROUNDS];   // element offset of the unit in the image at chunk 0; -1 = outside the image (zeros), -2 = no unit
    u32x4 reg[ROUNDS];

    __device__ __forceinline__ HaloImage(unsigned char *ldsA, int H, int W, int ty0, int tx0, int64_t in_ys, int64_t in_xs) : lds(ldsA) {
        const int tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            const int u = tid + i * THREADS;
            const int p = u >> 2, part = u & 3;
            const int hy = p / HW, hx = p - hy * HW;
            const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            off[i] = u >= UNITS ? -2 : (inside ? (int)(gy * in_ys + gx * in_xs) + part * 8 : -1);
        }
    }
    __device__ __forceinline__ void fetch(const uint16_t *in, int c0) {
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            reg[i] = u32x4{0u, 0u, 0u, 0u};
            if (off[i] >= 0) reg[i] = *reinterpret_cast<const u32x4 *>(in + off[i] + c0);
        }
    }
    __device__ __forceinline__ void stage() {
        const int tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            const int u = tid + i * THREADS;
            if (off[i] != -2) *reinterpret_cast<u32x4 *>(lds + (u >> 2) * PIX_B + (u & 3) * 16) = reg[i];
        }
    }
    // this lane's A fragment of its row m (0 | 1) at tap (dy, dx), k-step s
    __device__ __forceinline__ bf16x8 frag(int m, int dy, int dx, int s) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        return *reinterpret_cast<const bf16x8 *>(lds + ((wave * 2 + m + dy) * HW + (lane & 31) + dx) * PIX_B + (lane >> 5) * 16 + s * 32);
    }
};

template <int NB>
__device__ __forceinline__ void clear(f32x16 (&acc)[2][NB]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][nb][e] = 0.0f;
}

// k-step s of a tap: fa0, fa1 are the lane's A fragments of its two rows
template <int N>
__device__ __forceinline__ void mfma_step(f32x16 (&acc)[2][N / 32], const WImage<N> &w, int tap, int s, bf16x8 fa0, bf16x8 fa1) {
    constexpr int NB = N / 32;
    const bf16x8 fa[2] = {fa0, fa1};
    bf16x8 fb[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) fb[nb] = w.frag(tap, s, nb);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], fb[nb], acc[m][nb], 0, 0, 0);
}

// The epilogue's stores.  TileOut: the image's H, W, the tile's origin, and this workgroup's image (and channel slice) of the fp32 / bf16
// output (or null) with its y / x strides; lds is the workgroup's LDS, free to overwrite after the barrier taken here.
// chan(n) loads what the pointwise expression needs of output channel n (once per lane and channel, ahead of the stores), fin applies it:
//   VEC     fin(float (&v)[4], k[4], n, y, x) on channels n .. n + 3 of pixel (y, x).  The accumulators go through LDS so that a lane
//           owns four consecutive channels of a pixel: 16-byte fp32 stores, 8-byte bf16 stores (and as wide loads in fin).  The host
//           takes this form when every epilogue tensor is aligned for it (wide()).
//   narrow  fin(float &v, k, n, y, x): a lane keeps the column the accumulator layout gives it (4- and 2-byte accesses).
// fin must be the same expression sequence in both forms: then they give the same bits.  Both functors capture by value, and plain
// scalars and pointers only: through a reference to the kernel's descriptor, or with a bool in the closure, the compiler was seen to
// keep the closure in memory and re-evaluate uniform conditions per element.
template <int N>
constexpr int store_tile_bytes() {   // LDS the VEC form uses, from the base of the workgroup's LDS
    return 4 * 32 * N * 4;
}
struct TileOut {
    int H, W, ty0, tx0;
    float *of;
    int64_t of_ys, of_xs;
    uint16_t *ob;
    int64_t ob_ys, ob_xs;
};
template <int N, bool VEC, class Chan, class Fin>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[2][N / 32], void *lds, const TileOut o, Chan chan, Fin fin) {
    constexpr int NB = N / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    if constexpr (VEC) {
        // one row of the wave's two at a time: 32 pixels x N fp32 of LDS a wave (pixel rows of N floats: the ds_read_b128 lane groups
        // fall on 16 different slots without padding), then lane = (pixel, four channels)
        constexpr int Q = N / 4, PX_IT = 64 / Q;
        static_assert(32 % PX_IT == 0, "whole iterations over a row's 32 pixels");
        float *tile = reinterpret_cast<float *>(lds) + wave * (32 * N);
        const int q = lane % Q, pl = lane / Q;
        decltype(chan(0)) k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = chan(4 * q + j);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            __syncthreads();   // the K loop's images (m = 0) or the previous row (m = 1) have been read
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) tile[((e & 3) + 8 * (e >> 2) + 4 * h) * N + nb * 32 + r] = acc[m][nb][e];
            __syncthreads();
            const int y = o.ty0 + wave * 2 + m;
            if (y >= o.H) continue;
#pragma unroll
            for (int it = 0; it < 32 / PX_IT; ++it) {
                if constexpr (64 % Q != 0) {   // N = 96: 24 lane groups x 2 pixels occupy 48 lanes; lanes 48 .. 63 (pl = 2) would
                    if (pl >= PX_IT) continue;  // address a pixel of the next iteration (past the tile at the last one) and idle
                }
                const int xi = it * PX_IT + pl, x = o.tx0 + xi;
                if (x >= o.W) continue;
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(tile + xi * N + 4 * q);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
                fin(v, k, 4 * q, y, x);
                if (o.of) *reinterpret_cast<f32x4 *>(o.of + (int)(y * o.of_ys + x * o.of_xs) + 4 * q) = f32x4{v[0], v[1], v[2], v[3]};
                if (o.ob)
                    *reinterpret_cast<mitcg::u32x2 *>(o.ob + (int)(y * o.ob_ys + x * o.ob_xs) + 4 * q) =
                        mitcg::u32x2{mitcg::pack_bf16(v[0], v[1]), mitcg::pack_bf16(v[2], v[3])};
            }
        }
    } else {
        // the lane holds column n = nb * 32 + r of the pixels x = tx0 + (e & 3) + 8 (e >> 2) + 4 h of its two rows
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = nb * 32 + r;
            const auto k = chan(n);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int y = o.ty0 + wave * 2 + m;
                if (y >= o.H) continue;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int x = o.tx0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (x >= o.W) continue;
                    float v = acc[m][nb][e];
                    fin(v, k, n, y, x);
                    if (o.of) o.of[(int)(y * o.of_ys + x * o.of_xs) + n] = v;
                    if (o.ob) o.ob[(int)(y * o.ob_ys + x * o.ob_xs) + n] = bf16_bits(v);
                }
            }
        }
    }
}

// ---- host side: checks on strided NHWC tensors, shared by the entry points (fn = the entry point's name, the messages' prefix)

// [lo, hi) element extent of a strided NHWC tensor with C channels addressed
inline int64_t extent(int B, int H, int W, int64_t C, int64_t bs, int64_t ys, int64_t xs) {
    return (int64_t)(B - 1) * bs + (int64_t)(H - 1) * ys + (int64_t)(W - 1) * xs + C;
}

// strides of one tensor whose pixels hold C addressed channels: x stride >= C (`narrow` says it is not), y stride >= x stride, batch
// stride >= 0, one image — `tail` elements counted at its last pixel — below 2^31 elements
inline const char *bad_strides(int H, int W, int64_t C, int64_t tail, int64_t bs, int64_t ys, int64_t xs, const char *narrow) {
    if (xs < C) return narrow;
    if (ys < xs || bs < 0) return "y stride smaller than the x stride, or a negative batch stride";
    if (ys > INT32_MAX || extent(1, H, W, tail, 0, ys, xs) > INT32_MAX) return "one image spans 2^31 elements or more (32-bit offsets inside an image)";
    return nullptr;
}

// the wide epilogue: fp32 tensors on 16 bytes, the bf16 output on 8, every stride a multiple of four elements
inline bool wide(const void *p, int64_t bs, int64_t ys, int64_t xs, int align) {
    return !p || (reinterpret_cast<uintptr_t>(p) % align == 0 && bs % 4 == 0 && ys % 4 == 0 && xs % 4 == 0);
}

template <class D>
int check_outputs(const char *fn, const D &d) {
    return !d.out_f32 && !d.out_bf16 ? mit_set_error("%s: null pointer (no output: out_f32 and out_bf16 are both NULL)", fn) : 0;
}
template <class D>
int check_sizes(const char *fn, const D &d) {
    return d.B <= 0 || d.H <= 0 || d.W <= 0 ? mit_set_error("%s: sizes must be positive (B %d, H %d, W %d)", fn, d.B, d.H, d.W) : 0;
}

// 16-byte loads of the input (and of the weight w, where the descriptor holds one: else null) and the grid: gz = workgroups along z,
// `z_unit` what one of them is
template <class D>
int check_alignment_and_grid(const char *fn, const D &d, const void *w, int64_t gz, const char *z_unit) {
    if (reinterpret_cast<uintptr_t>(d.in) % 16 || reinterpret_cast<uintptr_t>(w) % 16 || d.in_xs % 8 || d.in_ys % 8 || d.in_bs % 8)
        return mit_set_error("%s: %s must be 16-byte aligned and the input strides multiples of 8 elements", fn, w ? "in and w" : "in");
    if (mit_div_up(d.H, TH) > 65535 || gz > 65535)
        return mit_set_error("%s: at most 65535 tile rows and 65535 %s a launch (grid y / z)", fn, z_unit);
    return 0;
}

// elements from the input's base to the bf16 output's (byte addresses as integers: the two may be one buffer or two), and whether the
// extents of the two — Cout channels addressed through an output pixel — intersect
template <class D>
int64_t out_bf16_offset(const D &d) {
    return (int64_t)(reinterpret_cast<intptr_t>(d.out_bf16) - reinterpret_cast<intptr_t>(d.in)) / 2;
}
template <class D>
bool extents_overlap(const D &d, int64_t din, int64_t Cout) {
    return din < extent(d.B, d.H, d.W, d.Cin, d.in_bs, d.in_ys, d.in_xs) && -din < extent(d.B, d.H, d.W, Cout, d.ob_bs, d.ob_ys, d.ob_xs);
}

}  // namespace conv3x3
