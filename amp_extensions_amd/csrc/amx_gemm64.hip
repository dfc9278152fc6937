// The fp32 products on 64 x 64 tiles (v_mfma_f32_32x32x2_f32): four waves of one 32 x 32 block
// each, K-tiles of 32 double-buffered in LDS, one barrier per K-tile.  They serve the few hundred
// rows of a training step, where 128 x 128 tiles would leave compute units idle:
//   k_gemm64_fwd       C = act(A W^T + b) per group, the forward (amx_gemm_bias_act_t64); global
//                      loads one K-tile ahead
//   k_gemm64<AK, BK>   C = A B, A W^T or A^T B with a ReLU-mask epilogue and column sums of A
//                      (amx_gemm_nn_f32, amx_gemm_tn_f32, amx_gemm64.h); loads two K-tiles ahead
// The forward and k_gemm64<0, 0> run the same K chain; they stay two kernels until the deeper
// prefetch has been measured on the forward's shapes.
#include <type_traits>

#include "amx_gemm64.h"

namespace {

using amx::Gemm64Args;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The forward GEMM of amx_gemm.hip's k_gemm_nt (C = act(A W^T + b) on v_mfma_f32_32x32x2_f32,
// K-tiles of 32 double-buffered in LDS, one barrier per K-tile) on 64 x 64 tiles: four waves of
// one 32 x 32 block each.  Every output element runs the same K chain as in the 128 x 128 tile
// (lanes 0-31 supply k, lanes 32-63 k + 16 of each K-tile), so the results are bit-identical; a
// training step's few hundred rows give four times the workgroups.
constexpr int FBK = 32, FLD = FBK + 4, FSTAGE = 128 * FLD;  // K-tile, floats per LDS row, floats per stage

struct FwdArgs {
  const float* A; long long strideA; int lda;
  const float* W; long long strideW; int ldw;
  const float* bias; long long strideBias;
  float* C; long long strideC; int ldc, col_off;
  int K, act;
};

__global__ __launch_bounds__(256, 2) void k_gemm64_fwd(FwdArgs a) {
  __shared__ __align__(16) float smem[2 * FSTAGE];
  const int tn = blockIdx.x, tm = blockIdx.y, g = blockIdx.z;
  const float* __restrict__ Ag = a.A + g * a.strideA + (long long)tm * 64 * a.lda;
  const float* __restrict__ Wg = a.W + g * a.strideW + (long long)tn * 64 * a.ldw;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  // staging: float4 of row (t >> 3) + 32 j, column 4 (t & 7), of the A and the W tile
  const int st_r = t >> 3, st_c = (t & 7) * 4;
  const float* a_src = Ag + (long long)st_r * a.lda + st_c;
  const float* w_src = Wg + (long long)st_r * a.ldw + st_c;
  const long long a_step = 32LL * a.lda, w_step = 32LL * a.ldw;
  float* const a_dst0 = smem + st_r * FLD + st_c;
  float* const w_dst0 = smem + 64 * FLD + st_r * FLD + st_c;
  f32x4 ra[2], rw[2];
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int nk = a.K / FBK;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ra[j] = *reinterpret_cast<const f32x4*>(a_src + j * a_step);
    rw[j] = *reinterpret_cast<const f32x4*>(w_src + j * w_step);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    *reinterpret_cast<f32x4*>(a_dst0 + j * 32 * FLD) = ra[j];
    *reinterpret_cast<f32x4*>(w_dst0 + j * 32 * FLD) = rw[j];
  }
  __syncthreads();
  const int a_off = (wm * 32 + li) * FLD + lh * 16;
  const int w_off = 64 * FLD + (wn * 32 + li) * FLD + lh * 16;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int kn = (kt + 1 < nk ? kt + 1 : kt) * FBK;  // the last iteration re-reads its own tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ra[j] = *reinterpret_cast<const f32x4*>(a_src + j * a_step + kn);
      rw[j] = *reinterpret_cast<const f32x4*>(w_src + j * w_step + kn);
    }
    __builtin_amdgcn_sched_barrier(0);  // the prefetch stays ahead of the MFMA block
    const float* As = smem + cur * FSTAGE + a_off;
    const float* Ws = smem + cur * FSTAGE + w_off;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 fa = *reinterpret_cast<const f32x4*>(As + v * 4);
      const f32x4 fb = *reinterpret_cast<const f32x4*>(Ws + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
    }
    const int nb = (cur ^ 1) * FSTAGE;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<f32x4*>(a_dst0 + nb + j * 32 * FLD) = ra[j];
      *reinterpret_cast<f32x4*>(w_dst0 + nb + j * 32 * FLD) = rw[j];
    }
    __syncthreads();
  }
  // C/D map of the 32x32 f32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = tn * 64 + wn * 32 + li;
  const float bv = a.bias[g * a.strideBias + col];
  float* Cg = a.C + g * a.strideC;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = tm * 64 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
    float v = acc[e] + bv;
    if (a.act == AMX_ACT_RELU) v = (v < 0.f) ? 0.f : v;  // keeps NaN, as torch.relu
    Cg[(long long)row * a.ldc + a.col_off + col] = v;
  }
}

// ---- 64 x 64 tile products with either operand in either form -------------------------------
// Four waves of one 32 x 32 block each, K-tiles of 32 double-buffered in LDS, one barrier per
// K-tile (k_gemm64_fwd's loop, with the global loads two K-tiles ahead).  An operand whose
// reduction index is its contiguous one in memory ("row form": A of A B, W of A W^T) is staged as 64 rows of 36 floats and read as
// float4 along k (k_gemm_nt's conflict-free rows); one whose reduction index is its row index
// ("k form": B of A B, both operands of A^T B) is staged as 32 rows of 64 floats, the rows of
// the upper k half rotated by 32 columns, and read as scalars: lanes 0-31 (k) and 32-63
// (k + 16) then hit disjoint banks.  Either way lane (i, h) supplies k = 16 h + q, q = 0..15,
// of each K-tile, so every output element runs one fp32 FMA chain in ascending k pairs.
constexpr int GBK = 32, GLD = GBK + 4, GOP = 64 * GLD, GSTAGE = 2 * GOP;

// this thread's two float4 of the K-tile at k0; x0 = tile origin, nx = extent of the other index
template <int KF>
__device__ inline void op_load(const float* __restrict__ P, int ld, int x0, int nx, int k0, int t, f32x4 (&r)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (KF) {
      const int c = x0 + (t & 15) * 4, k = k0 + (t >> 4) + 16 * j;
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      r[j] = c < nx ? *reinterpret_cast<const f32x4*>(P + (long long)k * ld + c) : z;
    } else {
      const int row = x0 + (t >> 3) + 32 * j;
      r[j] = *reinterpret_cast<const f32x4*>(P + (long long)row * ld + k0 + (t & 7) * 4);
    }
  }
}

template <int KF>
__device__ inline void op_store(float* S, int t, const f32x4 (&r)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (KF) *reinterpret_cast<f32x4*>(S + ((t >> 4) + 16 * j) * 64 + (((t & 15) * 4) ^ (j << 5))) = r[j];
    else *reinterpret_cast<f32x4*>(S + ((t >> 3) + 32 * j) * GLD + (t & 7) * 4) = r[j];
  }
}

template <int KF>
__device__ inline void op_frag(const float* S, int w, int li, int lh, float (&f)[16]) {
  if (KF) {
#pragma unroll
    for (int q = 0; q < 16; ++q) f[q] = S[(lh * 16 + q) * 64 + ((w * 32 + li) ^ (lh << 5))];
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(S + (w * 32 + li) * GLD + lh * 16 + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[4 * v + e] = x[e];
    }
  }
}

// AK: A is given as [K][M] (C = A^T B); BK: B is given as [K][N] (else as W [N][K], C = A W^T)
template <int AK, int BK>
__global__ __launch_bounds__(256, 2) void k_gemm64(Gemm64Args a) {
  __shared__ __align__(16) float smem[2 * GSTAGE];
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  // register sets: set p receives tile kt + 2 at the top of iteration kt (p = kt & 1) while set
  // p ^ 1 holds tile kt + 1, stored to the other LDS stage at the iteration's end: two
  // iterations of MFMAs cover a global load's latency (a 256-row step gives one workgroup per CU)
  f32x4 ra[2][2], rb[2][2];
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int nk = a.K / GBK;
  op_load<AK>(a.A, a.lda, tm * 64, a.M, 0, t, ra[0]);
  op_load<BK>(a.B, a.ldb, tn * 64, a.N, 0, t, rb[0]);
  op_store<AK>(smem, t, ra[0]);
  op_store<BK>(smem + GOP, t, rb[0]);
  const int k1 = (nk > 1 ? 1 : 0) * GBK;
  op_load<AK>(a.A, a.lda, tm * 64, a.M, k1, t, ra[1]);
  op_load<BK>(a.B, a.ldb, tn * 64, a.N, k1, t, rb[1]);
  __syncthreads();
  // column sums of A (the first column tile's workgroups): wave w sums rows 8 w .. 8 w + 7 of
  // every K-tile for column `lane`; the four partial sums meet in a fixed tree after the loop
  const bool do_cs = AK && a.colsum != nullptr && tn == 0;
  float cs = 0.f;
  auto body = [&](auto pc, int kt) {
    constexpr int P = decltype(pc)::value;
    const int kn = (kt + 2 < nk ? kt + 2 : nk - 1) * GBK;  // the last iterations re-read the last tile
    op_load<AK>(a.A, a.lda, tm * 64, a.M, kn, t, ra[P]);
    op_load<BK>(a.B, a.ldb, tn * 64, a.N, kn, t, rb[P]);
    __builtin_amdgcn_sched_barrier(0);  // the prefetch stays ahead of the MFMA block
    const float* As = smem + P * GSTAGE;
    const float* Bs = As + GOP;
    float fa[16], fb[16];
    op_frag<AK>(As, wm, li, lh, fa);
    op_frag<BK>(Bs, wn, li, lh, fb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[q], acc, 0, 0, 0);
    if (AK && do_cs) {
      const int left = a.cs_rows - kt * GBK - wave * 8;
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = As[(wave * 8 + q) * 64 + (lane ^ ((wave >> 1) << 5))];
#pragma unroll
      for (int q = 0; q < 8; ++q) cs += q < left ? v[q] : 0.f;
    }
    float* nxt = smem + (P ^ 1) * GSTAGE;
    op_store<AK>(nxt, t, ra[P ^ 1]);
    op_store<BK>(nxt + GOP, t, rb[P ^ 1]);
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    body(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) body(std::integral_constant<int, 1>{}, kt + 1);
  }
  // C/D map of the 32x32 f32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = tn * 64 + wn * 32 + li;
  if (col < a.N) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = tm * 64 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      float v = acc[e];
      if (a.mask) {
        const int mr = a.mask_mod ? row % a.mask_mod : row;
        v = a.mask[(long long)mr * a.ldm + col] > 0.f ? v : 0.f;
      }
      a.C[(long long)row * a.ldc + col] = v;
    }
  }
  if (AK && do_cs) {  // (the loop's last barrier is behind every read of smem)
    smem[wave * 64 + lane] = cs;
    __syncthreads();
    if (wave == 0) a.colsum[tm * 64 + lane] = (smem[lane] + smem[64 + lane]) + (smem[128 + lane] + smem[192 + lane]);
  }
}

template <int AK, int BK>
int launch_gemm(const Gemm64Args& a, hipStream_t st) {
  hipLaunchKernelGGL((k_gemm64<AK, BK>), dim3((a.N + 63) / 64, a.M / 64), dim3(256), 0, st, a);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

int check_gemm(const char* fn, const amx_ctx* ctx, const Gemm64Args& a, int a_cols, int b_cols) {
  AMX_CHECK_ARG(ctx, "%s: null ctx", fn);
  AMX_CHECK_ARG(a.M > 0 && a.M % 64 == 0, "%s: M=%d must be a positive multiple of 64", fn, a.M);
  AMX_CHECK_ARG(a.N > 0 && a.N % 4 == 0, "%s: N=%d must be a positive multiple of 4", fn, a.N);
  AMX_CHECK_ARG(a.K > 0 && a.K % GBK == 0, "%s: the reduction length %d must be a positive multiple of %d", fn, a.K,
                GBK);
  AMX_CHECK_ARG(a.A && a.B && a.C && amx::aligned16(a.A) && amx::aligned16(a.B), "%s: null/unaligned operand", fn);
  AMX_CHECK_ARG(a.lda >= a_cols && a.lda % 4 == 0 && a.ldb >= b_cols && a.ldb % 4 == 0 && a.ldc >= a.N,
                "%s: lda=%d (>= %d) ldb=%d (>= %d) must be multiples of 4, ldc=%d (>= %d)", fn, a.lda, a_cols, a.ldb,
                b_cols, a.ldc, a.N);
  AMX_CHECK_ARG(!a.mask || (a.ldm >= a.N && a.mask_mod >= 0), "%s: ldm=%d mask_mod=%d", fn, a.ldm, a.mask_mod);
  return AMX_OK;
}

}  // namespace

namespace amx {

int gemm64_nn(const Gemm64Args& a, hipStream_t st) { return launch_gemm<0, 1>(a, st); }
int gemm64_nt(const Gemm64Args& a, hipStream_t st) { return launch_gemm<0, 0>(a, st); }
int gemm64_tn(const Gemm64Args& a, hipStream_t st) { return launch_gemm<1, 1>(a, st); }

}  // namespace amx

extern "C" int amx_gemm_bias_act_t64(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                                     long long strideA, const float* W, int ldw, long long strideW,
                                     const float* bias, long long strideBias, float* C, int ldc, long long strideC,
                                     int col_off, int act, void* stream) {
  const char* fn = "amx_gemm_bias_act_t64";
  AMX_CHECK_ARG(ctx, "%s: null ctx", fn);
  AMX_CHECK_ARG(groups >= 1 && groups <= AMX_MAX_MODELS, "%s: groups=%d", fn, groups);
  AMX_CHECK_ARG(rows >= 0 && rows % AMX_ROW_TILE == 0, "%s: rows=%d must be a multiple of %d", fn, rows, AMX_ROW_TILE);
  AMX_CHECK_ARG(K > 0 && K % AMX_K_TILE == 0, "%s: K=%d must be a positive multiple of %d", fn, K, AMX_K_TILE);
  AMX_CHECK_ARG(A && W && amx::aligned16(A) && amx::aligned16(W), "%s: null/unaligned operand", fn);
  AMX_CHECK_ARG(lda >= K && lda % 4 == 0 && ldw >= K && ldw % 4 == 0 && strideA % 4 == 0 && strideW % 4 == 0,
                "%s: lda=%d ldw=%d (K=%d) must be >= K and, like the strides, multiples of 4", fn, lda, ldw, K);
  AMX_CHECK_ARG(N > 0 && N % 64 == 0, "%s: N=%d must be a multiple of 64", fn, N);
  AMX_CHECK_ARG(bias && C, "%s: null bias/C", fn);
  AMX_CHECK_ARG(col_off >= 0 && col_off + N <= ldc, "%s: col_off=%d N=%d ldc=%d", fn, col_off, N, ldc);
  AMX_CHECK_ARG(act == AMX_ACT_NONE || act == AMX_ACT_RELU, "%s: act=%d", fn, act);
  if (rows == 0) return AMX_OK;
  FwdArgs a = {};
  a.A = A; a.strideA = strideA; a.lda = lda;
  a.W = W; a.strideW = strideW; a.ldw = ldw;
  a.bias = bias; a.strideBias = strideBias;
  a.C = C; a.strideC = strideC; a.ldc = ldc; a.col_off = col_off;
  a.K = K; a.act = act;
  hipLaunchKernelGGL(k_gemm64_fwd, dim3(N / 64, rows / 64, groups), dim3(256), 0, (hipStream_t)stream, a);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_gemm_nn_f32(amx_ctx* ctx, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                               float* C, int ldc, const float* mask, int ldm, int mask_mod, void* stream) {
  Gemm64Args a = {};
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc;
  a.mask = mask; a.ldm = ldm; a.mask_mod = mask_mod;
  a.M = M; a.N = N; a.K = K;
  const int rc = check_gemm("amx_gemm_nn_f32", ctx, a, K, N);
  if (rc) return rc;
  return launch_gemm<0, 1>(a, (hipStream_t)stream);
}

extern "C" int amx_gemm_tn_f32(amx_ctx* ctx, int R, int M, int N, const float* A, int lda, const float* B, int ldb,
                               float* C, int ldc, const float* mask, int ldm, float* colsum, int colsum_rows,
                               void* stream) {
  Gemm64Args a = {};
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc;
  a.mask = mask; a.ldm = ldm; a.mask_mod = 0;
  a.colsum = colsum; a.cs_rows = colsum_rows;
  a.M = M; a.N = N; a.K = R;
  const int rc = check_gemm("amx_gemm_tn_f32", ctx, a, M, N);
  if (rc) return rc;
  AMX_CHECK_ARG(!colsum || (colsum_rows >= 0 && colsum_rows <= R), "amx_gemm_tn_f32: colsum_rows=%d (R=%d)",
                colsum_rows, R);
  return launch_gemm<1, 1>(a, (hipStream_t)stream);
}
