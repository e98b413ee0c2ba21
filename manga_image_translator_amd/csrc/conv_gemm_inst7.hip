// conv_gemm_inst7.hip — instantiates the grouped twins listed in conv_gemm_group_cfgs.inc (mit_conv_gemm_group).
#include "conv_gemm_kernels.h"

#define G(name, fam, BM, BN, BK, ...) \
    template void mitcg::launch_##fam##_group<BM, BN, BK, __VA_ARGS__>(const mitcg::GroupArgs &, int, int, hipStream_t);
#include "conv_gemm_group_cfgs.inc"
#undef G
