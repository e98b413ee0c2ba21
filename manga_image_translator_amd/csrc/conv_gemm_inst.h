// conv_gemm_inst.h — body of the conv_gemm_inst<N>.hip translation units: each defines MIT_INST_<N> as MIT_INST_YES and includes this
// file, which instantiates the launchers of the group-N tile configurations of conv_gemm_cfgs.inc (parallel compilation only).
#include "conv_gemm_kernels.h"

#define MIT_INST_YES(fam, BM, BN, BK, ...) \
    template void mitcg::launch_##fam<BM, BN, BK, __VA_ARGS__>(const MitConvGemm &, int, int, int, int, hipStream_t);
#define MIT_INST_NO(...)
// every group the including unit did not claim: one default per group
#ifndef MIT_INST_0
#define MIT_INST_0 MIT_INST_NO
#endif
#ifndef MIT_INST_1
#define MIT_INST_1 MIT_INST_NO
#endif
#ifndef MIT_INST_2
#define MIT_INST_2 MIT_INST_NO
#endif
#ifndef MIT_INST_3
#define MIT_INST_3 MIT_INST_NO
#endif
#ifndef MIT_INST_4
#define MIT_INST_4 MIT_INST_NO
#endif
#ifndef MIT_INST_5
#define MIT_INST_5 MIT_INST_NO
#endif
#ifndef MIT_INST_6
#define MIT_INST_6 MIT_INST_NO
#endif
#define X(g, name, fam, ...) MIT_INST_##g(fam, __VA_ARGS__)
#include "conv_gemm_cfgs.inc"
#undef X
