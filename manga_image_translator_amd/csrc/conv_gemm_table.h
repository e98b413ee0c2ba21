// conv_gemm_table.h — the tile table of mit_conv_gemm as data: conv_gemm_cfgs.inc turned into CfgEntry rows with their traits, every
// entry's buffer-load twin, and the compile-time lookup by name.  Host code of conv_gemm.hip alone (the instantiation units do not see it).
#pragma once
#include "conv_gemm_kernels.h"
#include <string_view>

namespace mitcg {
// One row of conv_gemm_cfgs.inc.  What the tile choice needs to know about a tile is read off the launcher's template arguments,
// never off its name.
enum class TileFamily { generic, fast, gemv, split };  // conv_gemm_kernel | conv_gemm_fast_kernel (needs fast_eligible()) | conv_gemv_kernel (gemv_eligible()) | conv_gemm_split_kernel (split_eligible())
struct CfgEntry {
    const char *name;
    TileFamily family;
    int BM, BN, BK;
    int args[5];  // the launcher's template arguments behind BM, BN, BK (zero-padded)
    void (*launch)(const MitConvGemm &, int M, int MT, int NT, int KT, hipStream_t);
    const char *kernel;  // the kernel's template-id as profilers print it, e.g. "conv_gemm_fast_kernel<128, 128, 16, 1, 4, 4, 4>"
    int twin;            // the entry with the same launcher arguments plus buffer loads (VAR + 2048); the entry itself when there is none
    constexpr int nprod() const { return family == TileFamily::split ? args[3] : 0; }                // plane pairs per k-step (1 | 3 | 6 | 9)
    constexpr bool buf() const { return family == TileFamily::split && (args[4] & 2048) != 0; }      // operand loads through buffer instructions
    constexpr int lanes_per_row() const { return family == TileFamily::gemv ? args[0] : 0; }
};
}  // namespace mitcg

#define X(g, name, fam, BM, BN, BK, ...) \
    extern template void mitcg::launch_##fam<BM, BN, BK, __VA_ARGS__>(const MitConvGemm &, int, int, int, int, hipStream_t);
#include "conv_gemm_cfgs.inc"
#undef X

namespace mitcg {
namespace {

#define KNAME_generic "conv_gemm_kernel"
#define KNAME_fast "conv_gemm_fast_kernel"
#define KNAME_gemv "conv_gemv_kernel"
#define KNAME_split "conv_gemm_split_kernel"
constexpr CfgEntry kCfgRows[] = {
#define X(g, name, fam, BM, BN, BK, ...) \
    {name, TileFamily::fam, BM, BN, BK, {__VA_ARGS__}, launch_##fam<BM, BN, BK, __VA_ARGS__>, KNAME_##fam "<" #BM ", " #BN ", " #BK ", " #__VA_ARGS__ ">", 0},
#include "conv_gemm_cfgs.inc"
#undef X
};
constexpr int kNumCfgs = sizeof(kCfgRows) / sizeof(kCfgRows[0]);
static_assert(kNumCfgs < 64, "the probe's callers size their arrays for 64 tiles");

// the table with every entry's buffer-load twin filled in: the entry with the same launcher arguments but VAR + 2048
constexpr bool is_buf_twin(const CfgEntry &a, const CfgEntry &b) {
    return a.family == TileFamily::split && b.family == a.family && !a.buf() && a.BM == b.BM && a.BN == b.BN && a.BK == b.BK && a.args[0] == b.args[0] &&
           a.args[1] == b.args[1] && a.args[2] == b.args[2] && a.args[3] == b.args[3] && b.args[4] == a.args[4] + 2048;
}
struct CfgTable {
    CfgEntry e[kNumCfgs];
};
constexpr CfgTable kCfgTable = [] {
    CfgTable t{};
    for (int i = 0; i < kNumCfgs; ++i) {
        t.e[i] = kCfgRows[i];
        t.e[i].twin = i;
        for (int j = 0; j < kNumCfgs; ++j)
            if (is_buf_twin(kCfgRows[i], kCfgRows[j])) t.e[i].twin = j;
    }
    return t;
}();
constexpr const CfgEntry (&kCfgs)[kNumCfgs] = kCfgTable.e;

// a tile by its name, at compile time: a name that is not in the table does not compile
constexpr int find_cfg(std::string_view name) {
    for (int i = 0; i < kNumCfgs; ++i)
        if (name == kCfgRows[i].name) return i;
    return -1;
}
#define CFG(name) ([] { constexpr int i = find_cfg(name); static_assert(i >= 0, "no tile " name " in conv_gemm_cfgs.inc"); return i; }())
static_assert(CFG("128x128x16") == 0 && kCfgs[CFG("split64x64x32p1o")].twin == CFG("split64x64x32p1u") && kCfgs[CFG("split128x64x16p9")].twin == CFG("split128x64x16p9"), "table order, buffer-load twins");

}  // namespace
}  // namespace mitcg
