// Internal launchers of amx_gemm64.hip's 64 x 64 f32 products, for callers inside the library
// that have validated their shapes themselves (the checked entry points are amx_gemm_nn_f32 and
// amx_gemm_tn_f32 of include/amx_hip.h).
#pragma once

#include "amx_common.h"

namespace amx {

struct Gemm64Args {
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  const float* mask; int ldm, mask_mod;  // C * (mask[row % mask_mod] > 0); mask_mod 0: row
  float* colsum; int cs_rows;            // gemm64_tn: colsum[m] = sum_{r < cs_rows} A[r][m]
  int M, N, K;
};

AMX_INTERNAL int gemm64_nn(const Gemm64Args& a, hipStream_t st);  // C [M][N] = A [M][K] B [K][N]
AMX_INTERNAL int gemm64_nt(const Gemm64Args& a, hipStream_t st);  // C [M][N] = A [M][K] W^T, B = W [N][K]
AMX_INTERNAL int gemm64_tn(const Gemm64Args& a, hipStream_t st);  // C [M][N] = A^T B, A [K][M], B [K][N]

}  // namespace amx
