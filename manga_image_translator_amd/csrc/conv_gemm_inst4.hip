// conv_gemm_inst4.hip — instantiates the group-4 tile configurations of conv_gemm_cfgs.inc (see conv_gemm_inst.h).
#define MIT_INST_4 MIT_INST_YES
#include "conv_gemm_inst.h"
