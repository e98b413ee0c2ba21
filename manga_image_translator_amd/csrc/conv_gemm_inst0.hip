// conv_gemm_inst0.hip — instantiates the group-0 tile configurations of conv_gemm_cfgs.inc (see conv_gemm_inst.h).
#define MIT_INST_0 MIT_INST_YES
#include "conv_gemm_inst.h"
