// conv_gemm.hip — tile choice, kernel-time probe and C entry points of mit_conv_gemm (validate -> plan -> launch).
// The kernels are in conv_gemm_kernels.h, their instantiations are compiled in conv_gemm_inst<group>.hip, the tile table is conv_gemm_table.h.
// mit_conv_gemm_group (several images of one layer as one grid) is at the end; its kernels are the grouped twins of conv_gemm_inst7.hip.
#include "conv_gemm_table.h"
#include <atomic>

using namespace mitcg;

// the grouped twins (conv_gemm_group_cfgs.inc), instantiated in conv_gemm_inst7.hip
#define G(name, fam, BM, BN, BK, ...) \
    extern template void mitcg::launch_##fam##_group<BM, BN, BK, __VA_ARGS__>(const mitcg::GroupArgs &, int, int, hipStream_t);
#include "conv_gemm_group_cfgs.inc"
#undef G

namespace {

// the largest element offset of A that a kernel forms, relative to the slice base; -1 for a negative stride or tap offset
int64_t max_a_offset(const MitConvGemm &p) {
    if (p.a_bs < 0 || p.a_ys < 0 || p.a_xs < 0) return -1;
    int tmax = 0;
    for (int t = 0; t < p.ntaps; ++t) {
        if (p.tap_off[t] < 0) return -1;
        if (p.tap_off[t] > tmax) tmax = p.tap_off[t];
    }
    return (int64_t)(p.NB - 1) * p.a_bs + (int64_t)(p.Hi - 1) * p.a_ys + (int64_t)(p.Wi - 1) * p.a_xs + p.Cin + tmax;
}
// fast kernel preconditions: whole K-tiles inside one tap, table fits, 32-bit element offsets
bool fast_eligible(const MitConvGemm &p, int BK) {
    if (p.Cin % BK || p.ntaps > FAST_MAX_TAPS) return false;
    const int64_t maxoff = max_a_offset(p);
    return maxoff >= 0 && maxoff < 0x7fffffffLL;
}

// conv_gemm_split_kernel preconditions: the fast kernel's, plus split planes of W laid out by mit_gemm_split_pack
bool split_eligible(const MitConvGemm &p, int BK) {
    if (!p.w_split || (reinterpret_cast<uintptr_t>(p.w_split) & 15) || (p.ws_zs0 & 7)) return false;
    if (p.w_zs1 != 0 || (p.Kw & 7) || p.ntaps * p.Cin > p.Kw) return false;
    if ((int64_t)3 * (p.Kw >> 3) * p.ldw > 0x7fffffffLL) return false;  // 32-bit cell indices
    return fast_eligible(p, BK);
}

// the "u" tiles (operand loads through buffer instructions: 32-bit byte offsets against a 2 GB descriptor, conv_gemm_split.h VAR bit
// 2048): every byte offset of A — relative to the slice base the kernel forms — and of the packed W planes must stay below 2^31
bool buf_eligible(const MitConvGemm &p) {
    const int64_t maxoff = max_a_offset(p);
    return maxoff >= 0 && maxoff * 4 < 0x80000000LL && (int64_t)3 * (p.Kw >> 3) * p.ldw * 16 < 0x80000000LL;
}
// a split tile as the automatic choice launches it: same arithmetic, operand loads through buffer instructions where the offsets fit
int buf_form(const MitConvGemm &p, int c) { return buf_eligible(p) ? kCfgs[c].twin : c; }

// conv_gemv_kernel preconditions: <= 4 output columns, plain (unbatched, unsplit) maps, the whole weight panel in LDS
bool gemv_eligible(const MitConvGemm &p, int lpr) {
    if (p.N > 4 || p.Z != 1 || p.Cin % (4 * lpr) || (int64_t)p.NB * p.Ho > 65535) return false;  // one output row per blockIdx.y
    if ((int64_t)p.ntaps * p.Cin * (p.N == 1 ? 1 : 4) * 4 > 60 * 1024) return false;            // the transposed weight panel must fit the default dynamic-LDS limit
    if (p.c.nsplit || p.pre.nsplit || p.post.nsplit || p.lut_rows) return false;
    return true;
}

// GEMM mode (include/mit_hip.h, mit_gemm_mode_set): -1 = not read yet
std::atomic<int> g_gemm_mode{-1};
int gemm_mode_now() {
    int m = g_gemm_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        const char *v = getenv("MIT_GEMM_SPLIT");
        m = (v && *v) ? atoi(v) : 6;
        if (m != 6 && m != 9) m = 0;
        g_gemm_mode.store(m, std::memory_order_relaxed);
    }
    return m;
}

// smallest launch (in 128 x 64 tiles) the automatic choice gives to the split tiles (mit_gemm_split_min_tiles).  Default 0: every
// eligible launch takes them, so that a layer's arithmetic — and with it a page's result — does not depend on how many pages share the
// batch (a size threshold made the same layer run on the fp32 tiles at B = 1 and on the split tiles at B = 16)
std::atomic<long long> g_split_min{0};
int64_t split_min_now() { return g_split_min.load(std::memory_order_relaxed); }

// ---- the tile choice.  One ladder for every kernel family, parameterised by the family's tiles and thresholds (-1: the family has no
// such tile).  All tiles of a family give the same bits, so a result depends neither on the rung nor on how many pages share the launch.
struct TileSet {
    int n32;                // N <= 32 (ESRGAN's growth-32 convolutions, small heads): a 128 x 32 tile, whatever the launch size
    int narrow, wide;       // 64 / 128 columns
    int small;              // 64 x 64 for under-filled launches (Z == 1, fewer than small_max 128 x 64 tiles)
    int64_t small_max;
    int small_k32;          // ... with two MFMA steps per barrier (BK = 32) for launches of at most 512 blocks
};
// measured on MI355X (scripts/bench_conv.py)
constexpr TileSet kGenericTiles = {CFG("128x32x16"), CFG("128x64x16"), CFG("128x128x16"), -1, 0, -1};
// small_max swept 640 .. 5120 on the OCR and detector stages (same-box A/B): 1280 = one full wave of workgroups.  wide: 4 waves of
// 128 x 32, <= 128 registers: 4 workgroups per CU (+3-7 % over the 2 x 2 layout)
constexpr TileSet kFp32Tiles = {CFG("fast128x32x16w4c"), CFG("fast128x64x16w5c"), CFG("fast128x128x16w4c"), CFG("fast64x64x16w8c"), 1280, -1};
// small_max 768: one wave of 128-row split tiles (3 workgroups per CU)
constexpr TileSet kP6Tiles = {CFG("split128x32x16p6o"), CFG("split128x64x16p6o"), CFG("split128x128x16p6o"), CFG("split64x64x16p6o"), 768, CFG("split64x64x32p6o")};
constexpr TileSet kP9Tiles = {CFG("split128x32x16p9m"), CFG("split128x64x16p9"), CFG("split128x128x16p9m"), CFG("split64x64x16p9m"), 768, CFG("split64x64x32p9m")};
// p1 (K-tile 32 throughout): no N <= 32 form — such a launch runs the 64-column tile with half its columns padded
constexpr TileSet kP1Tiles = {-1, CFG("split128x64x32p1o"), CFG("split128x128x32p1o"), CFG("split64x64x32p1o"), 768, -1};

int64_t tiles128(const MitConvGemm &p, int64_t M) { return ((M + 127) / 128) * ((p.N + 63) / 64); }

// exact: the family's exact-N tile for this launch (the caller's rule), -1 = none
int ladder(const TileSet &s, const MitConvGemm &p, int64_t M, int exact = -1) {
    if (p.N <= 32 && s.n32 >= 0) return s.n32;
    const int rem = p.N % 128;
    int c = (p.N <= 64 || (rem != 0 && rem <= 64)) ? s.narrow : s.wide;  // e.g. N = 192: 3 x 64 beats 2 x 128 with a half-empty tile
    if (exact >= 0) c = exact;
    // under-filled launches (one page through the plugins, the decoder's GEMMs: M = lines x beams = 10240; its Linears at M = 160): a
    // 128-row tiling leaves most CUs with one workgroup or none, 64 x 64 tiles double to quadruple the workgroup count; the arithmetic
    // per output element is that of the large tiles
    if (s.small >= 0 && p.Z == 1 && tiles128(p, M) < s.small_max) {
        c = s.small;
        // launches of at most two workgroups per CU (one page through the plugins: the decoder at M = 160 rows, the detector's deep
        // layers) are bound by the latency of a K-loop iteration, not by its throughput: two MFMA steps per barrier (BK = 32) take
        // 10-22 % off them and cost 2 % on fuller launches (profiles/r03l_split_check_bk32.log).  Same MFMA sequence per element.
        if (s.small_k32 >= 0 && ((M + 63) / 64) * ((p.N + 63) / 64) <= 512 && split_eligible(p, 32)) c = s.small_k32;
    }
    return c;
}

// Exact-N p6 tiles (round 5; wave tile 32 x BN, the A tile split once for all BN columns) where the 64-column tile would otherwise
// run 3 or 5 times over the same rows, or the 128-column tile would compute 48 padded columns — measured per shape
// (profiles/r07f_split_check_exact_n_tiles.log, r07g_split_check_tile192.log; same bits as every other p6 tile):
//   N = 160, K = 640 (ConvNeXt stage-2 pw2): 1.36x of 3 x 64;   N = 320, K = 1280 (stage-3 pw2): 1.13x of 5 x 64;
//   N = 80, K = 320 (stage-1 pw2): 1.08x of the 128-column tile;   N = 192, K = 384 (LaMa spectral conv1): 1.09x of 3 x 64.
// The short-K expansions (pw1: K = 80 / 160 / 320 into N = 4K) are 5-10 % SLOWER on them and keep the tiles of the ladder.
int exact_n_p6(const MitConvGemm &p) {
    if (p.Z != 1) return -1;
    const int K = p.ntaps * p.Cin;
    if ((p.N == 160 || p.N == 320) && K >= 512) return CFG("split128x160x16p6o");
    if (p.N > 64 && p.N <= 96 && K >= 256) return CFG("split128x96x16p6o");
    if (p.N == 192 && K >= 256) return CFG("split128x192x16p6o");
    return -1;
}

int pick_cfg(const MitConvGemm &p, int64_t M) {
    // MitConvGemm.nprod == 1: the one-product tiles, whatever the GEMM mode and the launch size (the caller checked split_eligible(p, 16)).
    // Measured on LaMa's shapes only (N = 128 / 256 / 512 wide, 64 narrow, 192 / 384 on the 192-column tile:
    // profiles/r17a_lama_precision.json); outside them the choice is UNMEASURED — the 192-column tile for every N % 192 == 0.
    if (p.nprod == 1) {
        if (!split_eligible(p, 32)) return buf_form(p, CFG("split64x64x16p1o"));  // Cin % 32 != 0
        return buf_form(p, ladder(kP1Tiles, p, M, p.N % 192 == 0 ? CFG("split128x192x32p1o") : -1));
    }
    if (gemv_eligible(p, 16)) return p.N == 1 ? CFG("gemv16n1") : CFG("gemv16");
    if (gemv_eligible(p, 4)) return p.N == 1 ? CFG("gemv4n1") : CFG("gemv4");
    // split-bf16 tiles (GEMM mode 6 | 9, mit_gemm_mode_set): layers whose packer attached split planes of W, large enough to fill the chip
    const int mode = gemm_mode_now();
    if ((mode == 6 || mode == 9) && p.w_split && split_eligible(p, 16) && tiles128(p, M) * p.Z >= split_min_now())
        return buf_form(p, mode == 6 ? ladder(kP6Tiles, p, M, exact_n_p6(p)) : ladder(kP9Tiles, p, M));
    if (!fast_eligible(p, 16)) return ladder(kGenericTiles, p, M);
    // batched launches (Z entries of M = 184 rows: W-axis DFTs): 2 x 128 rows would run a 40 % empty second tile.  Unbatched, one row of
    // 192 x 64 tiles leaves the chip empty (the decoder at B = 1: M = 160)
    if (p.N > 32 && M > 128 && M <= 192 && p.Z >= 8) return CFG("fast192x64x16w4c");
    return ladder(kFp32Tiles, p, M);
}

// ---- kernel-time probe (mit_prof_*): HIP events around every launch while enabled ----
struct ProbeRec {
    hipEvent_t start, stop;
    int cfg;
    double exec_flops, alg_flops;
    int M, N, K, ntaps, Z, act;
    double wino_bytes;  // the Winograd pre-operand read by the epilogue (MitConvGemm.wino_m): 36 products per tile and column
};
std::mutex g_probe_mu;
bool g_probe_on = false;
std::vector<ProbeRec> g_probe;
thread_local double g_next_alg_flops = -1.0;

}  // namespace

extern "C" int mit_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_probe_mu);
    for (auto &r : g_probe) {
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    g_probe.clear();
    g_probe_on = on != 0;
    mit_probe_reset(on != 0);
    return 0;
}

extern "C" int mit_prof_tag_next(double alg_flops) {
    g_next_alg_flops = alg_flops;
    return 0;
}

extern "C" int mit_prof_dump(const char *path) {
    if (!path) return mit_set_error("mit_prof_dump: null path");
    std::lock_guard<std::mutex> lk(g_probe_mu);
    FILE *f = fopen(path, "w");
    if (!f) return mit_set_error("mit_prof_dump: cannot open %s", path);
    fprintf(f, "tile,M,N,K,taps,Z,act,ms,exec_flops,alg_flops,wino_bytes\n");
    for (auto &r : g_probe) {
        float ms = 0.f;
        if (hipEventSynchronize(r.stop) != hipSuccess || hipEventElapsedTime(&ms, r.start, r.stop) != hipSuccess) {
            fclose(f);
            return mit_set_error("mit_prof_dump: event query failed");
        }
        fprintf(f, "%s,%d,%d,%d,%d,%d,%d,%.6f,%.0f,%.0f,%.0f\n", kCfgs[r.cfg].name, r.M, r.N, r.K, r.ntaps, r.Z, r.act, ms, r.exec_flops,
                r.alg_flops, r.wino_bytes);
    }
    fclose(f);
    return 0;
}

extern "C" int mit_prof_read(MitProfStat *stats, int max_cfgs, int *n_cfgs) {
    if (!stats || !n_cfgs) return mit_set_error("mit_prof_read: null");
    std::lock_guard<std::mutex> lk(g_probe_mu);
    const int n = max_cfgs < kNumCfgs ? max_cfgs : kNumCfgs;
    for (int i = 0; i < n; ++i) {
        stats[i].launches = 0;
        stats[i].ms = stats[i].exec_flops = stats[i].alg_flops = 0.0;
    }
    for (auto &r : g_probe) {
        MIT_CHECK_HIP(hipEventSynchronize(r.stop));
        float ms = 0.f;
        MIT_CHECK_HIP(hipEventElapsedTime(&ms, r.start, r.stop));
        if (r.cfg < n) {
            stats[r.cfg].launches += 1;
            stats[r.cfg].ms += ms;
            stats[r.cfg].exec_flops += r.exec_flops;
            stats[r.cfg].alg_flops += r.alg_flops;
        }
    }
    *n_cfgs = n;
    return 0;
}

extern "C" const char *mit_conv_gemm_config_name(int cfg) {
    if (cfg < 0 || cfg >= kNumCfgs) return nullptr;
    return kCfgs[cfg].name;
}

extern "C" const char *mit_conv_gemm_config_kernel(int cfg) {
    if (cfg < 0 || cfg >= kNumCfgs) return nullptr;
    return kCfgs[cfg].kernel;
}

namespace {
bool map_vec_ok(const MitTensorMap &m, bool split_ok = false) {
    if (m.nsplit != 0 && !(split_ok && !(m.nsplit & 3) && !(m.nhi & 3))) return false;  // (only the C map's float4 store handles a column split)
    return !(reinterpret_cast<uintptr_t>(m.base) & 15) && !((m.zs1 | m.zs0 | m.bs | m.ys | m.xs) & 3);
}
// dwordx4 epilogue (epilogue_store_vec): whole float4 column groups, contiguous and 16-byte aligned in every tensor it touches
bool vec_epilogue_ok(const MitConvGemm &p) {
    if ((p.N & 3) || !map_vec_ok(p.c, true)) return false;
    if (p.pre.base && !map_vec_ok(p.pre)) return false;
    if (p.post.base && !map_vec_ok(p.post)) return false;
    if (p.lut_rows && ((p.lut_ld & 3) || (reinterpret_cast<uintptr_t>(p.lut1) & 15) || (reinterpret_cast<uintptr_t>(p.lut2) & 15))) return false;
    return !(reinterpret_cast<uintptr_t>(p.scale) & 15) && !(reinterpret_cast<uintptr_t>(p.bias) & 15);
}

// rows of a launch that carries a live-block list: every 8 x 8 block of every image whole (edge blocks are clipped in the kernel), so
// that the dense grid covers the case "every block live"
int64_t list_rows(const MitConvGemm &p) { return (int64_t)p.NB * ((p.Ho + 7) / 8) * ((p.Wo + 7) / 8) * 64; }
int64_t rows_of(const MitConvGemm &p) { return p.live_blocks ? list_rows(p) : (int64_t)p.NB * p.Ho * p.Wo; }

// ---- validate -> plan -> launch ----
// stage 1: the descriptor by itself, whatever tile it takes.  p = *d with MIT_ACT_VEC_OK set where the float4 epilogue applies.
int validate(const MitConvGemm *d, MitConvGemm &p) {
    if (!d) return mit_set_error("mit_conv_gemm: null descriptor");
    p = *d;
    if (p.act & MIT_ACT_VEC_OK) return mit_set_error("mit_conv_gemm: reserved activation bits set");
    if (vec_epilogue_ok(p)) p.act |= MIT_ACT_VEC_OK;
    if (!p.a || !p.w || !p.c.base) return mit_set_error("mit_conv_gemm: null operand");
    if (p.Cin <= 0 || (p.Cin & 3)) return mit_set_error("mit_conv_gemm: Cin must be a positive multiple of 4 (got %d)", p.Cin);
    if ((p.ldw & 3) || (p.Nw & 3)) return mit_set_error("mit_conv_gemm: ldw/Nw must be multiples of 4 (ldw=%lld Nw=%d)", (long long)p.ldw, p.Nw);
    if (p.ntaps <= 0 || p.ntaps > MIT_MAX_TAPS) return mit_set_error("mit_conv_gemm: ntaps %d out of range", p.ntaps);
    if (p.NB <= 0 || p.Ho <= 0 || p.Wo <= 0 || p.N <= 0 || p.Z <= 0 || p.zdiv <= 0)
        return mit_set_error("mit_conv_gemm: empty problem");
    if ((reinterpret_cast<uintptr_t>(p.a) & 15) || (reinterpret_cast<uintptr_t>(p.w) & 15))
        return mit_set_error("mit_conv_gemm: operands must be 16-byte aligned");
    if ((p.a_xs & 3) || (p.a_ys & 3) || (p.a_bs & 3) || (p.a_zs0 & 3) || (p.a_zs1 & 3) || (p.w_zs0 & 3) || (p.w_zs1 & 3))
        return mit_set_error("mit_conv_gemm: strides must be multiples of 4 elements");
    for (int t = 0; t < p.ntaps; ++t)
        if (p.tap_off[t] & 3) return mit_set_error("mit_conv_gemm: tap_off must be multiples of 4");
    if (p.pad_mode == MIT_PAD_REFLECT) {
        for (int t = 0; t < p.ntaps; ++t) {
            int ady = p.tap_dy[t] < 0 ? -p.tap_dy[t] : p.tap_dy[t];
            int adx = p.tap_dx[t] < 0 ? -p.tap_dx[t] : p.tap_dx[t];
            if (ady >= p.Hi || adx >= p.Wi) return mit_set_error("mit_conv_gemm: reflect pad larger than input");
        }
    }
    if ((int64_t)p.NB * p.Ho * p.Wo > 0x7fffffffLL) return mit_set_error("mit_conv_gemm: M too large");
    if (p.lut_rows) {  // the row-lookup epilogue: both tables, rows long enough, one slice (lut_rows is indexed by the output row)
        if (!p.lut1 || !p.lut2 || p.lut_ld < p.N) return mit_set_error("mit_conv_gemm: lut_rows needs lut1, lut2 and lut_ld >= N");
        if (p.Z != 1) return mit_set_error("mit_conv_gemm: the row-lookup epilogue is for Z == 1 launches");
        if (p.lut_ld > 0x7fff) return mit_set_error("mit_conv_gemm: lut_ld too large (row offsets are 16-bit row x lut_ld in 32 bits)");
    }
    if (p.live_blocks || p.live_start) {  // the live-block list: both arrays, one slice, rows decoded per block (no per-row table)
        if (!p.live_blocks || !p.live_start) return mit_set_error("mit_conv_gemm: a live-block list needs live_blocks and live_start");
        if ((reinterpret_cast<uintptr_t>(p.live_blocks) | reinterpret_cast<uintptr_t>(p.live_start)) & 3) return mit_set_error("mit_conv_gemm: live_blocks / live_start must be 4-byte aligned");
        if (p.Z != 1) return mit_set_error("mit_conv_gemm: a live-block list is for Z == 1 launches");
        if (p.lut_rows) return mit_set_error("mit_conv_gemm: a live-block list together with lut_rows is not implemented");
        if (p.live_img0 < 0) return mit_set_error("mit_conv_gemm: live_img0 must be >= 0 (got %d)", p.live_img0);
        if (list_rows(p) > 0x7fffffffLL) return mit_set_error("mit_conv_gemm: M too large");
    } else if (p.live_img0 != 0) {
        return mit_set_error("mit_conv_gemm: live_img0 without a live-block list");
    }
    if (p.wino_m) {  // the Winograd pre-operand (wino_pre_add): a lane's 16 rows of an accumulator block must be one 4 x 4 tile
        if (!p.live_blocks) return mit_set_error("mit_conv_gemm: wino_m needs the 8 x 8 block row order (live_blocks / live_start; list every block for a dense layer)");
        if (p.ntaps != 1 || p.sy != 1 || p.sx != 1) return mit_set_error("mit_conv_gemm: wino_m is for one tap with stride 1 (got %d taps, stride %d x %d)", p.ntaps, p.sy, p.sx);
        if (p.pre.base) return mit_set_error("mit_conv_gemm: wino_m together with a pre operand is not implemented");
        if (p.c.nsplit || (p.post.base && p.post.nsplit)) return mit_set_error("mit_conv_gemm: wino_m with a column-split map is not implemented");
        if ((p.N & 3) || p.wino_n != p.N) return mit_set_error("mit_conv_gemm: wino_m needs N %% 4 == 0 and wino_n == N (N=%d wino_n=%d)", p.N, p.wino_n);
        if (p.wino_th != (p.Ho + 3) / 4 || p.wino_tw != (p.Wo + 3) / 4)
            return mit_set_error("mit_conv_gemm: wino_th x wino_tw must be ceil(Ho / 4) x ceil(Wo / 4) (got %d x %d for %d x %d)", p.wino_th, p.wino_tw, p.Ho, p.Wo);
        if (p.wino_zs < (int64_t)p.NB * p.wino_th * p.wino_tw * p.wino_n) return mit_set_error("mit_conv_gemm: wino_zs is shorter than one slice of tiles (NB * wino_th * wino_tw * wino_n)");
        if (reinterpret_cast<uintptr_t>(p.wino_m) & 3) return mit_set_error("mit_conv_gemm: wino_m must be 4-byte aligned");
    }
    if (p.Z > 65535) return mit_set_error("mit_conv_gemm: Z too large");
    if (p.nprod != 0 && p.nprod != 1) return mit_set_error("mit_conv_gemm: nprod must be 0 (the GEMM mode) or 1 (one bf16 product) (got %d)", p.nprod);
    if (p.nprod == 1 && !p.w_split) return mit_set_error("mit_conv_gemm: nprod = 1 needs w_split (mit_gemm_split_pack): there is no fp32 fallback for a requested precision");
    return 0;
}

// stage 2a: images per run of an automatic launch (p.NB: the batch is not cut).
// The fast kernels index A with 32-bit element offsets.  A batch whose activations exceed 2^31 elements (16 pages of
// 2048 x 1456 x 64: LaMa's first stride-2 conv) is cut into runs of whole images that fit, instead of falling to the generic kernel.
// Round 6: in the split mode the runs are cut to what the buffer-load tiles address (2^31 BYTES per run: buf_eligible) when one
// image fits that — every run is still thousands of workgroups, and each takes the "u" tile instead of its "o" twin.
int images_per_run(const MitConvGemm &p) {
    if (p.Z != 1 || p.NB <= 1) return p.NB;
    MitConvGemm q = p;
    q.NB = 1;
    const bool want_buf = (gemm_mode_now() == 6 || p.nprod == 1) && p.w_split != nullptr && split_eligible(p, 16) && buf_eligible(q);
    auto run_ok = [&](const MitConvGemm &r) { return fast_eligible(r, 16) && (!want_buf || buf_eligible(r)); };
    if (p.Cin % 16 != 0 || p.ntaps > FAST_MAX_TAPS || p.a_bs <= 0 || run_ok(p) || !fast_eligible(q, 16)) return p.NB;
    int nb = p.NB;
    while (nb > 1) {
        q.NB = nb;
        if (run_ok(q)) break;
        nb = (nb + 1) / 2;
    }
    return nb;
}
// the run of `nb` images from image b0 on
MitConvGemm run_of(const MitConvGemm &p, int b0, int nb) {
    MitConvGemm r = p;
    r.NB = nb;
    r.a += (int64_t)b0 * p.a_bs;
    r.c.base += (int64_t)b0 * p.c.bs;
    if (p.pre.base) r.pre.base += (int64_t)b0 * p.pre.bs;
    if (p.post.base) r.post.base += (int64_t)b0 * p.post.bs;
    if (p.lut_rows) r.lut_rows += (int64_t)b0 * p.Ho * p.Wo;
    if (p.wino_m) r.wino_m += (int64_t)b0 * p.wino_th * p.wino_tw * p.wino_n;
    if (p.live_blocks) r.live_start += b0, r.live_img0 += b0;  // the run's segment of the list: [live_start[b0], live_start[b0 + nb])
    return r;
}

// stage 2b: the tile of one run (cfg < 0: the automatic choice) and what that tile refuses
int plan_run(const MitConvGemm &p, int cfg, int *tile) {
    const int64_t M = rows_of(p);
    if (p.nprod == 1) {  // (per run: a batch past 2^31 elements is eligible run by run)
        if (!split_eligible(p, 16))
            return mit_set_error("mit_conv_gemm: nprod = 1 needs the split tiles' preconditions (Cin %% 16 == 0, <= %d taps, 32-bit element offsets, 16-byte aligned w_split with w_zs1 == 0 and Kw %% 8 == 0): there is no fp32 fallback for a requested precision", FAST_MAX_TAPS);
        if (cfg >= 0 && cfg < kNumCfgs && kCfgs[cfg].nprod() != 1) return mit_set_error("mit_conv_gemm: nprod = 1 with tile %s, which is not a one-product tile", kCfgs[cfg].name);
    }
    if (cfg < 0) cfg = pick_cfg(p, M);
    if (cfg >= kNumCfgs) return mit_set_error("mit_conv_gemm: bad cfg %d", cfg);
    const CfgEntry &c = kCfgs[cfg];
    const bool fast = c.family == TileFamily::fast, split = c.family == TileFamily::split, gemv = c.family == TileFamily::gemv;
    if (p.lut_rows) {  // the row-lookup epilogue exists as an instantiation of the vector store path of the fast / split tiles only
        if (!fast && !split)
            return mit_set_error("mit_conv_gemm: the row-lookup epilogue (lut_rows) needs a fast or split tile (Cin %% 16 == 0, <= %d taps); this launch takes %s", FAST_MAX_TAPS, c.name);
        if (!(p.act & MIT_ACT_VEC_OK)) return mit_set_error("mit_conv_gemm: lut_rows needs the float4 epilogue (N %% 4 == 0, 16-byte aligned maps, tables and lut_ld %% 4 == 0)");
        if (p.post.base) return mit_set_error("mit_conv_gemm: lut_rows together with a post residual is not implemented");
        if ((p.act & 0xff) != MIT_ACT_NONE && (p.act & 0xff) != MIT_ACT_RELU) return mit_set_error("mit_conv_gemm: lut_rows is implemented for act none / relu");
    }
    if (p.live_blocks && !fast && !split)  // no dense fallback: the caller's dead positions hold no defined value
        return mit_set_error("mit_conv_gemm: a live-block list needs a fast or split tile (Cin %% 16 == 0, <= %d taps, N > 4); this launch takes %s", FAST_MAX_TAPS, c.name);
    if (gemv && (!gemv_eligible(p, c.lanes_per_row()) || p.N > c.BN))
        return mit_set_error("mit_conv_gemm: cfg %s needs N <= %d, Z == 1, unsplit maps and Cin %% %d == 0", c.name, c.BN, 4 * c.lanes_per_row());
    if (split && !split_eligible(p, c.BK))
        return mit_set_error("mit_conv_gemm: cfg %s needs w_split (mit_gemm_split_pack, 16-byte aligned, w_zs1 == 0, Kw %% 8 == 0) and the fast tiles' preconditions", c.name);
    if (fast && !fast_eligible(p, c.BK))
        return mit_set_error("mit_conv_gemm: cfg %s needs Cin %% %d == 0, <= %d taps and 32-bit element offsets", c.name, c.BK, FAST_MAX_TAPS);
    if ((M + c.BM - 1) / c.BM * ((p.N + c.BN - 1) / c.BN) > 0x7fffffffLL) return mit_set_error("mit_conv_gemm: grid too large");
    *tile = cfg;
    return 0;
}

// stage 3: one planned run, inside the probe while it is enabled
int launch_run(const MitConvGemm &p, int cfg, hipStream_t hs) {
    const CfgEntry &c = kCfgs[cfg];
    const int M = (int)rows_of(p);
    const int MT = (M + c.BM - 1) / c.BM;
    const int NT = (p.N + c.BN - 1) / c.BN;
    const int Ktot = p.ntaps * p.Cin;
    const int KT = (Ktot + c.BK - 1) / c.BK;
    const double tagged = g_next_alg_flops;
    g_next_alg_flops = -1.0;
    if (g_probe_on) {
        std::lock_guard<std::mutex> lk(g_probe_mu);
        ProbeRec r;
        MIT_CHECK_HIP(hipEventCreate(&r.start));
        MIT_CHECK_HIP(hipEventCreate(&r.stop));
        r.cfg = cfg;
        r.exec_flops = 2.0 * (double)M * p.N * Ktot * p.Z;
        r.alg_flops = tagged >= 0.0 ? tagged : r.exec_flops;
        r.M = M, r.N = p.N, r.K = Ktot, r.ntaps = p.ntaps, r.Z = p.Z, r.act = p.act;
        r.wino_bytes = p.wino_m ? 4.0 * 36.0 * (double)p.NB * p.wino_th * p.wino_tw * p.wino_n : 0.0;
        MIT_CHECK_HIP(hipEventRecord(r.start, hs));
        c.launch(p, M, MT, NT, KT, hs);
        MIT_CHECK_HIP(hipEventRecord(r.stop, hs));
        if (p.live_blocks) {  // credit the live rows, not M: the count is read back behind the launch (probe only — a synchronising copy)
            int32_t s0 = 0, s1 = 0;
            MIT_CHECK_HIP(hipEventSynchronize(r.stop));
            MIT_CHECK_HIP(hipMemcpy(&s0, p.live_start, sizeof(s0), hipMemcpyDeviceToHost));
            MIT_CHECK_HIP(hipMemcpy(&s1, p.live_start + p.NB, sizeof(s1), hipMemcpyDeviceToHost));
            r.M = (s1 - s0) * 64;
            r.exec_flops = 2.0 * (double)r.M * p.N * Ktot * p.Z;
            r.alg_flops = r.exec_flops;
        }
        g_probe.push_back(r);
    } else {
        c.launch(p, M, MT, NT, KT, hs);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mit_set_error("mit_conv_gemm: launch failed: %s", hipGetErrorString(e));
    return 0;
}
}  // namespace

// The cut is applied twice, as two nested loops: to 2^31 elements first, and each such run — only now eligible for the split tiles — to
// the 2^31 bytes of the buffer-load tiles.  (Sixteen 2048 x 1456 x 64 pages run as 2 x 4 runs of two.)
extern "C" int mit_conv_gemm_plan(const MitConvGemm *d, int cfg, int32_t *tile, int32_t *nb_run) {
    if (!tile || !nb_run) return mit_set_error("mit_conv_gemm_plan: null output");
    MitConvGemm p;
    if (int rc = validate(d, p)) return rc;
    if (cfg < 0)
        for (int pass = 0; pass < 2; ++pass) {
            const int nb = images_per_run(p);
            if (nb < p.NB) p = run_of(p, 0, nb);
        }
    int t = -1;
    if (int rc = plan_run(p, cfg, &t)) return rc;
    *tile = t, *nb_run = p.NB;
    return 0;
}

extern "C" int mit_conv_gemm_cfg(const MitConvGemm *d, int cfg, void *stream) {
    MitConvGemm p;
    if (int rc = validate(d, p)) return rc;
    hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    int tile = -1;
    const int nb1 = cfg < 0 ? images_per_run(p) : p.NB;
    if (nb1 == p.NB) {
        if (int rc = plan_run(p, cfg, &tile)) return rc;
        return launch_run(p, tile, hs);
    }
    for (int b1 = 0; b1 < p.NB; b1 += nb1) {  // (a shorter last run is planned by itself)
        const MitConvGemm r1 = run_of(p, b1, p.NB - b1 < nb1 ? p.NB - b1 : nb1);
        const int nb2 = images_per_run(r1);
        for (int b2 = 0; b2 < r1.NB; b2 += nb2) {
            const MitConvGemm r2 = run_of(r1, b2, r1.NB - b2 < nb2 ? r1.NB - b2 : nb2);
            g_next_alg_flops = -1.0;  // a tagged cost does not survive the cut
            if (int rc = plan_run(r2, -1, &tile)) return rc;
            if (int rc = launch_run(r2, tile, hs)) return rc;
        }
    }
    return 0;
}

extern "C" int mit_conv_gemm(const MitConvGemm *d, void *stream) { return mit_conv_gemm_cfg(d, -1, stream); }

// ---- grouped launches: n convolutions that share everything but the image, as one grid (include/mit_hip.h, mit_conv_gemm_group) ----
namespace {
struct GroupTwin {
    int cfg;
    void (*launch)(const GroupArgs &, int NT, int KT, hipStream_t);
};
constexpr bool row_is(const CfgEntry &e, TileFamily f, int BM, int BN, int BK, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0) {
    return e.family == f && e.BM == BM && e.BN == BN && e.BK == BK && e.args[0] == a0 && e.args[1] == a1 && e.args[2] == a2 && e.args[3] == a3 && e.args[4] == a4;
}
#define G(name, fam, ...) static_assert(row_is(kCfgs[CFG(name)], TileFamily::fam, __VA_ARGS__), "grouped twin " name " differs from its row in conv_gemm_cfgs.inc");
#include "conv_gemm_group_cfgs.inc"
#undef G
const GroupTwin kGroupTwins[] = {
#define G(name, fam, BM, BN, BK, ...) {CFG(name), launch_##fam##_group<BM, BN, BK, __VA_ARGS__>},
#include "conv_gemm_group_cfgs.inc"
#undef G
};
const GroupTwin *group_twin(int cfg) {
    for (const GroupTwin &t : kGroupTwins)
        if (t.cfg == cfg) return &t;
    return nullptr;
}

// the base descriptor with member m's image in place of its own
MitConvGemm member_desc(const MitConvGemm &b, const MitConvGemmMember &m) {
    MitConvGemm d = b;
    d.a = m.a, d.a_bs = m.a_bs, d.a_ys = m.a_ys;
    d.NB = m.NB, d.Hi = m.Hi, d.Wi = m.Wi, d.Ho = m.Ho, d.Wo = m.Wo;
    d.c.base = m.c, d.c.bs = m.c_bs, d.c.ys = m.c_ys;
    return d;
}

struct GroupPlan {
    std::vector<MitConvGemm> desc;  // the members as descriptors of their own, as given (the fallback launches them)
    std::vector<MitConvGemm> p;     // ... validated
    int cfg = -1;                   // the tile of one launch with the group's total rows (-1: not determined, the group falls back)
    bool grouped = false;           // the group runs as concatenated grids on cfg's twin
    const GroupTwin *twin = nullptr;
};
// validate every member, choose the tile, decide between the grouped launch and the member-by-member fallback
int plan_group(const MitConvGemm *base, const MitConvGemmMember *members, int n, GroupPlan &g) {
    if (!base || !members) return mit_set_error("mit_conv_gemm_group: null pointer");
    if (n <= 0) return mit_set_error("mit_conv_gemm_group: empty group");
    if (base->pre.base || base->post.base) return mit_set_error("mit_conv_gemm_group: pre / post operands are per image and the member records carry none");
    g.desc.resize(n);
    g.p.resize(n);
    for (int i = 0; i < n; ++i) {
        g.desc[i] = member_desc(*base, members[i]);
        if (int rc = validate(&g.desc[i], g.p[i])) return rc;
    }
    const MitConvGemm &b = g.p[0];
    if (b.live_blocks || b.wino_m || b.lut_rows || b.Z != 1) return 0;  // forms the grouped kernels do not take: member by member
    int64_t Mtot = 0;
    for (int i = 0; i < n; ++i) {
        if (images_per_run(g.p[i]) != g.p[i].NB) return 0;  // a cut batch
        Mtot += rows_of(g.p[i]);
    }
    if (Mtot > 0x7fffffffLL) return 0;
    if (b.nprod == 1 && !split_eligible(b, 16)) return 0;  // (the member launches refuse it with their own message)
    g.cfg = pick_cfg(b, Mtot);
    const CfgEntry &c = kCfgs[g.cfg];
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const MitConvGemm &q = g.p[i];
        // every member eligible for the group's tile: the choice made for it alone at the group's size is the same tile (this covers the
        // fast / split / buffer-load preconditions, which depend on the member's offsets), and the tile does not refuse it
        if (q.act != b.act || (q.nprod == 1 && !split_eligible(q, 16)) || pick_cfg(q, Mtot) != g.cfg) return 0;
        int t = -1;
        if (plan_run(q, g.cfg, &t) != 0) return 0;
        tiles += (rows_of(q) + c.BM - 1) / c.BM * ((q.N + c.BN - 1) / c.BN);
    }
    if (tiles > 0x7fffffffLL) return 0;
    g.twin = group_twin(g.cfg);
    g.grouped = g.twin != nullptr;
    return 0;
}
int64_t member_tiles(const MitConvGemm &q, const CfgEntry &c) { return (rows_of(q) + c.BM - 1) / c.BM * ((q.N + c.BN - 1) / c.BN); }
}  // namespace

extern "C" int mit_conv_gemm_group_plan(const MitConvGemm *base, const MitConvGemmMember *members, int n, int32_t *tile, int32_t *launch,
                                        int32_t *first_tile, int32_t *ntiles) {
    GroupPlan g;
    if (int rc = plan_group(base, members, n, g)) return rc;
    if (tile) *tile = g.cfg;
    int32_t t0 = 0;
    for (int i = 0; i < n; ++i) {
        if (i % GROUP_MAX == 0) t0 = 0;
        const int32_t nt = g.cfg >= 0 ? (int32_t)member_tiles(g.p[i], kCfgs[g.cfg]) : 0;
        if (launch) launch[i] = g.grouped ? i / GROUP_MAX : -1;
        if (first_tile) first_tile[i] = g.grouped ? t0 : 0;
        if (ntiles) ntiles[i] = nt;
        t0 += nt;
    }
    return 0;
}

extern "C" int mit_conv_gemm_group(const MitConvGemm *base, const MitConvGemmMember *members, int n, void *stream) {
    GroupPlan g;
    if (int rc = plan_group(base, members, n, g)) return rc;
    hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    if (!g.grouped) {
        for (int i = 0; i < n; ++i)
            if (int rc = mit_conv_gemm_cfg(&g.desc[i], -1, stream)) return rc;
        return 0;
    }
    const CfgEntry &c = kCfgs[g.cfg];
    const MitConvGemm &b = g.p[0];
    const int NT = (b.N + c.BN - 1) / c.BN;
    const int Ktot = b.ntaps * b.Cin;
    const int KT = (Ktot + c.BK - 1) / c.BK;
    const double tagged = g_next_alg_flops;
    g_next_alg_flops = -1.0;
    for (int i0 = 0; i0 < n; i0 += GROUP_MAX) {
        GroupArgs ga = {};
        ga.p = b;
        ga.n = n - i0 < GROUP_MAX ? n - i0 : GROUP_MAX;
        int64_t rows = 0;
        for (int i = 0; i < ga.n; ++i) {
            ga.m[i] = members[i0 + i];
            ga.tile0[i + 1] = ga.tile0[i] + (int32_t)member_tiles(g.p[i0 + i], c);
            rows += rows_of(g.p[i0 + i]);
        }
        if (g_probe_on) {  // one launch under its tile's index with the members' summed FLOPs
            std::lock_guard<std::mutex> lk(g_probe_mu);
            ProbeRec r;
            MIT_CHECK_HIP(hipEventCreate(&r.start));
            MIT_CHECK_HIP(hipEventCreate(&r.stop));
            r.cfg = g.cfg;
            r.exec_flops = 2.0 * (double)rows * b.N * Ktot;
            r.alg_flops = tagged >= 0.0 && n <= GROUP_MAX ? tagged : r.exec_flops;
            r.M = (int)rows, r.N = b.N, r.K = Ktot, r.ntaps = b.ntaps, r.Z = 1, r.act = b.act;
            r.wino_bytes = 0.0;
            MIT_CHECK_HIP(hipEventRecord(r.start, hs));
            g.twin->launch(ga, NT, KT, hs);
            MIT_CHECK_HIP(hipEventRecord(r.stop, hs));
            g_probe.push_back(r);
        } else {
            g.twin->launch(ga, NT, KT, hs);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return mit_set_error("mit_conv_gemm_group: launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

extern "C" int mit_gemm_mode_set(int mode) {
    if (mode != 0 && mode != 6 && mode != 9) return mit_set_error("mit_gemm_mode_set: mode must be 0, 6 or 9 (got %d)", mode);
    g_gemm_mode.store(mode, std::memory_order_relaxed);
    return 0;
}

extern "C" int mit_gemm_mode_get(void) { return gemm_mode_now(); }

extern "C" int64_t mit_gemm_split_min_tiles(int64_t n) {
    const int64_t prev = split_min_now();
    if (n >= 0) g_split_min.store(n, std::memory_order_relaxed);
    return prev;
}

extern "C" int mit_gemm_split_pack(const float *w_dev, int64_t w_zs, int nz, int Kw, int64_t ldw, uint16_t *out_dev, void *stream) {
    if (!w_dev || !out_dev) return mit_set_error("mit_gemm_split_pack: null pointer");
    if (nz <= 0 || Kw <= 0 || (Kw & 7) || ldw <= 0 || (ldw & 3) || ldw > 0x7fffffffLL)
        return mit_set_error("mit_gemm_split_pack: need nz > 0, Kw %% 8 == 0, ldw %% 4 == 0 (nz=%d Kw=%d ldw=%lld)", nz, Kw, (long long)ldw);
    if ((reinterpret_cast<uintptr_t>(out_dev) & 15)) return mit_set_error("mit_gemm_split_pack: output must be 16-byte aligned");
    const int64_t total = (int64_t)nz * (Kw >> 3) * ldw;
    hipLaunchKernelGGL(gemm_split_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       w_dev, w_zs, Kw >> 3, (int)ldw, out_dev, total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mit_set_error("mit_gemm_split_pack: launch failed: %s", hipGetErrorString(e));
    return 0;
}
