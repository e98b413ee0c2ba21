// conv_gemm_inst5.hip — instantiates the group-5 tile configurations of conv_gemm_cfgs.inc (see conv_gemm_inst.h).
#define MIT_INST_5 MIT_INST_YES
#include "conv_gemm_inst.h"
