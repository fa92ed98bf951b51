// What the two bodies of the large-batch token-axis kernels share: token_linear.hip (fp32 products) and token_linear_bf16.hip (bf16
// products: token_linear at NASREC_PRECISION_MEDIUM, token_dw at _HIGH / _MEDIUM).  One eligibility rule, one launch geometry, one LDS
// budget for both.
#pragma once
#include "gemm_tile.h"

#define TL_WAVES 16
#define TL_CHUNK 8        // k-steps (of 4 k) loaded before their MFMAs
#define TL_MAX_LDS 147456  // bytes of staged weights per workgroup (one 16-wave workgroup per CU; 160 KB LDS)
#define TL_BIAS_FLOATS 80  // the row biases sit in front of the weights (M <= 80)

template <int RB>
struct TlPad {
  static constexpr int v = RB == 1 ? 16 : (RB <= 3 ? 48 : 80);
};

#define TDW_WAVES 16

// token_linear_bf16.hip: the same launches with the geometry launch_token_linear / launch_token_dw worked out
void launch_token_linear_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int grid, int wgs, size_t lds);
void launch_token_dw_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int cb, int grid, int Mmax, int Nmax);
