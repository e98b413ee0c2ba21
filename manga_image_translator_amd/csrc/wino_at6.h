// wino_at6.h — one pass of the Winograd F(4x4, 3x3) output transform, shared by wino43_output_kernel (winograd.hip) and the GEMM
// epilogue that folds the transform in (wino_pre_add, conv_gemm_kernels.h).  Both compile this one expression sequence (fp contraction
// is off in the build), so a folded launch adds exactly the values the stand-alone transform would have stored.
#pragma once

#include <hip/hip_runtime.h>

// A^T (rows): [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
__device__ __forceinline__ void at6(const float m0, const float m1, const float m2, const float m3, const float m4, const float m5,
                                    float &y0, float &y1, float &y2, float &y3) {
    const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
    y0 = (m0 + s12) + s34;
    y1 = d12 + 2.f * d34;
    y2 = s12 + 4.f * s34;
    y3 = (d12 + 8.f * d34) + m5;
}
