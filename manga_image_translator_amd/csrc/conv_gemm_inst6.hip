// conv_gemm_inst6.hip — instantiates the group-6 tile configurations of conv_gemm_cfgs.inc (see conv_gemm_inst.h).
#define MIT_INST_6 MIT_INST_YES
#include "conv_gemm_inst.h"
