// conv_gemm_inst3.hip — instantiates the group-3 tile configurations of conv_gemm_cfgs.inc (see conv_gemm_inst.h).
#define MIT_INST_3 MIT_INST_YES
#include "conv_gemm_inst.h"
