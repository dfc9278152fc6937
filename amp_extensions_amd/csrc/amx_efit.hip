// Training the dynamics ensemble on the device: one optimizer step of DynamicsModel.train_step
// (milo/milo/dynamics.py:236-250) for all M members at once, each on its own index batch.
//
//   k_efit_gather   x0 = [(s - mu_s)/sd_s, (a - mu_a)/sd_a, 0-pad] and the normalised target
//                   ((s' - s) - mu_d)/sd_d of the batch's rows; rows >= n_b zero
//   amx_gemm_bias_act[_t64] x (L + 1)   the forward on the fp32 master weights (f32 MFMA; 64 x 64
//                   tiles while 128 x 128 ones would leave compute units idle)
//   k_efit_loss     dZ_L = 2 (pred - target)/(n_b S), the step's MSE into loss[g]
//   per layer i = L .. 0:
//     k_efit_wgrad  gW_i = dZ_i^T act, gb_i = column sums of dZ_i
//     k_efit_dgrad  dact[:, hidden slices < i] (+)= dZ_i W_i; the tiles of slice i - 1, final
//                   after this launch, write dZ_{i-1} = dact * (act > 0)
//   k_efit_sumsq    per-workgroup partial sums of g^2 (grad_clip > 0)
//   k_efit_prep     clip_grad_norm_'s coefficient, the step count and Adam's bias corrections
//   k_efit_update   torch.optim.Adam / SGD(nesterov=True) on every padded tensor
//
// Stream order is the only synchronisation: no workgroup waits on another.  Every sum runs in
// a fixed order, so a fit is deterministic.  The backward products are fp32 FMA chains on the
// VALU over LDS tiles (the step is bound by its launches and weight traffic).
// Zero-padded weights see a zero gradient, so they and their optimizer state stay exactly 0.
#include <math.h>

#include "amx_common.h"

namespace {

constexpr int EF_MAX_LAYERS = 8;           // L + 1
constexpr int EF_MAX_T = 2 * EF_MAX_LAYERS;  // weight and bias tensors
constexpr int EF_NB_SQ = 64;               // workgroups per member of k_efit_sumsq
constexpr int EF_CONST = 16;               // floats of a member's step constants

// a member's step constants (k_efit_prep -> k_efit_update)
struct StepConst {
  float coef;                                   // clip_grad_norm_'s clip_coef_clamped
  float step, bc2s, omb1, b2, omb2, eps;        // Adam
  float lr, mu;                                 // SGD
};
static_assert(sizeof(StepConst) <= EF_CONST * sizeof(float), "step constants");

struct Tensors {
  float* w[EF_MAX_T];            // member 0's tensor
  long long stride[EF_MAX_T];    // member stride of w
  long long off[EF_MAX_T + 1];   // offsets in the flat gradient / state vectors
  int n;
};

struct Plan {
  int M, L, Hp, k0, ldk, NO, S, A;
  long long P;                   // floats of a member's flat gradient
  long long offW[EF_MAX_LAYERS], offB[EF_MAX_LAYERS];
};

int make_plan(const char* fn, const amx_ctx* c, Plan* p) {
  AMX_CHECK_ARG(c, "%s: null ctx", fn);
  AMX_CHECK_ARG(c->L >= 1 && c->L + 1 <= EF_MAX_LAYERS, "%s: %d hidden layers (supported: 1..%d)", fn, c->L,
                EF_MAX_LAYERS - 1);
  p->M = c->M; p->L = c->L; p->Hp = c->H; p->k0 = c->k0_pad; p->ldk = c->ldk; p->NO = c->n_out_pad;
  p->S = c->S; p->A = c->A;
  long long o = 0;
  for (int i = 0; i <= c->L; ++i) {
    const long long N = i == c->L ? c->n_out_pad : c->H, K = i == c->L ? c->ldk : c->k0_pad + (long long)i * c->H;
    p->offW[i] = o;
    o += N * K;
    p->offB[i] = o;
    o += N;
  }
  p->P = o;
  return AMX_OK;
}

// workspace layout in floats
struct Work {
  long long act, pred, target, dzL, dz, dact, part, cst, total;
};

Work work_layout(const Plan& p, int Bt) {
  Work w;
  long long o = 0;
  const long long MB = (long long)p.M * Bt;
  w.act = o;    o += MB * p.ldk;
  w.pred = o;   o += MB * p.NO;
  w.target = o; o += MB * p.NO;
  w.dzL = o;    o += MB * p.NO;
  w.dz = o;     o += 2 * MB * p.Hp;
  w.dact = o;   o += MB * p.L * p.Hp;
  w.part = o;   o += 2LL * p.M * EF_NB_SQ;  // doubles
  w.cst = o;    o += (long long)p.M * EF_CONST;
  w.total = o;
  return w;
}

__global__ __launch_bounds__(256) void k_efit_gather(int n_b, int n_rows, const int32_t* __restrict__ idx,
                                                     long long strideIdx, const float* __restrict__ states,
                                                     const float* __restrict__ actions,
                                                     const float* __restrict__ next_states,
                                                     const float* __restrict__ norm, int S, int A, int k0, int NO,
                                                     float* __restrict__ act, int ldk, long long strideA,
                                                     float* __restrict__ target, long long strideT) {
  const int r = blockIdx.x, g = blockIdx.y;
  float* x = act + g * strideA + (long long)r * ldk;
  float* t = target + g * strideT + (long long)r * NO;
  if (r >= n_b) {
    for (int c = threadIdx.x; c < k0; c += 256) x[c] = 0.f;
    for (int c = threadIdx.x; c < NO; c += 256) t[c] = 0.f;
    return;
  }
  int i = idx[g * strideIdx + r];
  i = i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i);
  const float* s = states + (long long)i * S;
  const float* a = actions + (long long)i * A;
  const float* s2 = next_states + (long long)i * S;
  const float *mu_s = norm, *sd_s = norm + S, *mu_a = norm + 2 * S, *sd_a = mu_a + A, *mu_d = sd_a + A,
              *sd_d = mu_d + S;
  for (int c = threadIdx.x; c < k0; c += 256) {
    float v = 0.f;
    if (c < S) v = (s[c] - mu_s[c]) / sd_s[c];
    else if (c < S + A) v = (a[c - S] - mu_a[c - S]) / sd_a[c - S];
    x[c] = v;
  }
  for (int c = threadIdx.x; c < NO; c += 256) t[c] = c < S ? ((s2[c] - s[c]) - mu_d[c]) / sd_d[c] : 0.f;
}

// The forward GEMM of amx_gemm.hip's k_gemm_nt (C = act(A W^T + b) on v_mfma_f32_32x32x2_f32,
// K-tiles of 32 double-buffered in LDS, one barrier per K-tile) on 64 x 64 tiles: four waves of
// one 32 x 32 block each.  Every output element runs the same K chain as in the 128 x 128 tile
// (lanes 0-31 supply k, lanes 32-63 k + 16 of each K-tile), so the results are bit-identical; a
// training step's few hundred rows give four times the workgroups.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int FBK = 32, FLD = FBK + 4, FSTAGE = 128 * FLD;  // K-tile, floats per LDS row, floats per stage

struct FwdArgs {
  const float* A; long long strideA; int lda;
  const float* W; long long strideW; int ldw;
  const float* bias; long long strideBias;
  float* C; long long strideC; int ldc, col_off;
  int K, act;
};

__global__ __launch_bounds__(256, 2) void k_efit_fwd64(FwdArgs a) {
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

// nn.MSELoss (mean over n_b x S) and its gradient; one workgroup per member
__global__ __launch_bounds__(1024) void k_efit_loss(int n_b, int Bt, int S, int NO, const float* __restrict__ pred,
                                                    const float* __restrict__ target, float* __restrict__ dzL,
                                                    float* __restrict__ loss, long long strideLoss) {
  __shared__ double red[1024];
  const int g = blockIdx.x, tid = threadIdx.x;
  const long long base = (long long)g * Bt * NO, total = (long long)Bt * NO;
  const double cnt = (double)n_b * (double)S;
  const float scale = (float)(2.0 / cnt);
  double acc = 0.0;
  for (long long e = tid; e < total; e += 1024) {
    const int r = (int)(e / NO), n = (int)(e % NO);
    float z = 0.f;
    if (r < n_b && n < S) {
      const float d = pred[base + e] - target[base + e];
      z = scale * d;
      acc += (double)d * (double)d;
    }
    dzL[base + e] = z;
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[g * strideLoss] = (float)(red[0] / cnt);
}

// gW[n][k] = sum_r dz[r][n] act[r][k]: 64 x 64 tiles, 16 rows of the reduction staged at a
// time; thread (tn, tk) owns a 4 x 4 block.  The workgroups of the first K tile also sum dz's
// columns into gb.
__global__ __launch_bounds__(256) void k_efit_wgrad(int rows, int K, const float* __restrict__ dz, int ldz,
                                                    long long strideZ, const float* __restrict__ act, int lda,
                                                    long long strideA, float* __restrict__ gW,
                                                    float* __restrict__ gb, long long strideG) {
  __shared__ float4 sz[16][16], sa[16][16];
  const int tid = threadIdx.x, g = blockIdx.z, n0 = blockIdx.y * 64, kb = blockIdx.x * 64;
  const int lr = tid >> 4, lc = tid & 15, tn = tid >> 4, tk = tid & 15;
  const float* z = dz + g * strideZ + n0 + lc * 4;
  const float* a = act + g * strideA + kb + lc * 4;
  const bool a_in = kb + lc * 4 < K;
  float acc[4][4] = {};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < rows; r0 += 16) {
    const float4 vz = *(const float4*)(z + (long long)(r0 + lr) * ldz);
    const float4 va = a_in ? *(const float4*)(a + (long long)(r0 + lr) * lda) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0) __syncthreads();
    sz[lr][lc] = vz;
    sa[lr][lc] = va;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 zz = sz[q][tn], aa = sa[q][tk];
      const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, av[4] = {aa.x, aa.y, aa.z, aa.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bsum[j] += zv[j];
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[j][l] = fmaf(zv[j], av[l], acc[j][l]);
      }
    }
  }
  float* out = gW + g * strideG;
  if (kb + tk * 4 < K) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *(float4*)(out + (long long)(n0 + tn * 4 + j) * K + kb + tk * 4) =
          make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  }
  if (blockIdx.x == 0 && tk == 0)
    *(float4*)(gb + g * strideG + n0 + tn * 4) = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
}

// dact[r][c] (+)= sum_n dz[r][n] W[n][k0 + c] for the hidden columns c < ncols: 64 x 64 tiles,
// 16 of the reduction's n staged at a time.  Tiles of the slice that is final after this launch
// (columns >= final_c0) write dz_out = dact * (act > 0) instead of dact.
__global__ __launch_bounds__(256) void k_efit_dgrad(int Nred, int k0, int accumulate, int final_c0,
                                                    const float* __restrict__ dz, int ldz, long long strideZ,
                                                    const float* __restrict__ W, int ldw, long long strideW,
                                                    const float* __restrict__ act, int lda, long long strideA,
                                                    float* __restrict__ dact, int ldd, long long strideD,
                                                    float* __restrict__ dz_out, int ldo, long long strideO) {
  __shared__ __align__(16) float szt[16][68];  // dz tile, transposed: [n][r]
  __shared__ float4 sw[16][16];
  const int tid = threadIdx.x, g = blockIdx.z, r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int zr = tid >> 2, zn = (tid & 3) * 4;  // dz load: row zr, columns zn .. zn + 3
  const int wr = tid >> 4, wc = tid & 15;        // W load: row wr, columns 4 wc .. 4 wc + 3
  const int tr = tid >> 4, tc = tid & 15;
  const float* z = dz + g * strideZ + (long long)(r0 + zr) * ldz + zn;
  const float* w = W + g * strideW + (long long)wr * ldw + k0 + c0 + wc * 4;
  float acc[4][4] = {};
  for (int nn = 0; nn < Nred; nn += 16) {
    const float4 vz = *(const float4*)(z + nn);
    const float4 vw = *(const float4*)(w + (long long)nn * ldw);
    if (nn) __syncthreads();
    szt[zn + 0][zr] = vz.x;
    szt[zn + 1][zr] = vz.y;
    szt[zn + 2][zr] = vz.z;
    szt[zn + 3][zr] = vz.w;
    sw[wr][wc] = vw;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 zz = *(const float4*)&szt[q][tr * 4], ww = sw[q][tc];
      const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[j][l] = fmaf(zv[j], wv[l], acc[j][l]);
    }
  }
  const bool fin = c0 >= final_c0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long r = r0 + tr * 4 + j;
    const int c = c0 + tc * 4;
    float4* pd = (float4*)(dact + g * strideD + r * ldd + c);
    float4 v = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    if (accumulate) {
      const float4 d = *pd;
      v = make_float4(d.x + v.x, d.y + v.y, d.z + v.z, d.w + v.w);
    }
    if (!fin) {
      *pd = v;
      continue;
    }
    const float4 h = *(const float4*)(act + g * strideA + r * lda + k0 + c);
    *(float4*)(dz_out + g * strideO + r * ldo + (c - final_c0)) =
        make_float4(h.x > 0.f ? v.x : 0.f, h.y > 0.f ? v.y : 0.f, h.z > 0.f ? v.z : 0.f, h.w > 0.f ? v.w : 0.f);
  }
}

__global__ __launch_bounds__(256) void k_efit_sumsq(const float* __restrict__ grad, long long P,
                                                    double* __restrict__ part) {
  __shared__ double red[256];
  const int g = blockIdx.y, tid = threadIdx.x;
  const float4* p = (const float4*)(grad + g * P);
  double acc = 0.0;
  for (long long e = (long long)blockIdx.x * 256 + tid; e < P / 4; e += (long long)EF_NB_SQ * 256) {
    const float4 v = p[e];
    acc += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[g * EF_NB_SQ + blockIdx.x] = red[0];
}

// per member: clip_grad_norm_'s coefficient (max_norm / (norm + 1e-6), clamped to 1), the step
// count, Adam's bias corrections (beta^t in double)
__global__ void k_efit_prep(int M, int adam, double lr, double p1, double grad_clip, const double* __restrict__ part,
                            long long* __restrict__ step, float* __restrict__ cst) {
  const int g = threadIdx.x;
  if (g >= M) return;
  StepConst c = {};
  c.coef = 1.f;
  if (grad_clip > 0.0) {
    double s = 0.0;
    for (int b = 0; b < EF_NB_SQ; ++b) s += part[g * EF_NB_SQ + b];
    const float norm = (float)sqrt(s);
    const float cc = (float)grad_clip / (norm + 1e-6f);
    c.coef = cc < 1.f ? cc : 1.f;
  }
  const long long t = step[g] + 1;
  step[g] = t;
  if (adam) {
    const double b1 = 0.9, b2 = 0.999;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    c.step = (float)(lr / bc1);
    c.bc2s = (float)sqrt(bc2);
    c.omb1 = (float)(1.0 - b1);
    c.b2 = (float)b2;
    c.omb2 = (float)(1.0 - b2);
    c.eps = (float)p1;
  } else {
    c.lr = (float)lr;
    c.mu = (float)p1;
  }
  *(StepConst*)(cst + g * EF_CONST) = c;
}

// torch.optim.Adam's single-tensor update, op for op (amx_vfit.hip's adam_math without decay)
__device__ inline void adam1(float& w, float& m, float& v, float g, const StepConst& a) {
  m = m + (g - m) * a.omb1;
  v = v * a.b2 + (a.omb2 * g) * g;
  const float den = sqrtf(v) / a.bc2s + a.eps;
  w = w - a.step * (m / den);
}

// torch.optim.SGD, momentum, nesterov, dampening 0: buf = mu buf + g (the first step's zero
// buffer gives g exactly); p -= lr (g + mu buf)
__device__ inline void sgd1(float& w, float& buf, float g, const StepConst& a) {
  buf = buf * a.mu + g;
  w = w - a.lr * (g + a.mu * buf);
}

__global__ __launch_bounds__(256) void k_efit_update(Tensors T, int adam, const float* __restrict__ grad,
                                                     float* __restrict__ s1, float* __restrict__ s2, long long P,
                                                     const float* __restrict__ cst) {
  const int g = blockIdx.y;
  const StepConst a = *(const StepConst*)(cst + g * EF_CONST);
  const long long gs = (long long)gridDim.x * 256;
  for (int t = 0; t < T.n; ++t) {
    const long long n4 = (T.off[t + 1] - T.off[t]) / 4;
    float4* w = (float4*)(T.w[t] + g * T.stride[t]);
    const float4* gr = (const float4*)(grad + g * P + T.off[t]);
    float4* m = (float4*)(s1 + g * P + T.off[t]);
    float4* v = (float4*)(s2 + g * P + T.off[t]);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n4; e += gs) {
      float4 gg = gr[e], ww = w[e], mm = m[e];
      gg = make_float4(gg.x * a.coef, gg.y * a.coef, gg.z * a.coef, gg.w * a.coef);
      if (adam) {
        float4 vv = v[e];
        adam1(ww.x, mm.x, vv.x, gg.x, a);
        adam1(ww.y, mm.y, vv.y, gg.y, a);
        adam1(ww.z, mm.z, vv.z, gg.z, a);
        adam1(ww.w, mm.w, vv.w, gg.w, a);
        v[e] = vv;
      } else {
        sgd1(ww.x, mm.x, gg.x, a);
        sgd1(ww.y, mm.y, gg.y, a);
        sgd1(ww.z, mm.z, gg.z, a);
        sgd1(ww.w, mm.w, gg.w, a);
      }
      w[e] = ww;
      m[e] = mm;
    }
  }
}

}  // namespace

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
  hipLaunchKernelGGL(k_efit_fwd64, dim3(N / 64, rows / 64, groups), dim3(256), 0, (hipStream_t)stream, a);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" long long amx_efit_param_count(const amx_ctx* ctx) {
  Plan p;
  if (make_plan("amx_efit_param_count", ctx, &p)) return -1;
  return p.P;
}

extern "C" long long amx_efit_work_floats(const amx_ctx* ctx, int Bt) {
  Plan p;
  if (make_plan("amx_efit_work_floats", ctx, &p)) return -1;
  if (Bt <= 0 || Bt % AMX_ROW_TILE) {
    amx::set_error("amx_efit_work_floats: Bt=%d is not a positive multiple of %d", Bt, AMX_ROW_TILE);
    return -1;
  }
  return work_layout(p, Bt).total;
}

extern "C" int amx_efit_step(amx_ctx* ctx, int train, int n_b, int Bt, const int32_t* idx, long long strideIdx,
                             int n_rows, const float* states, const float* actions, const float* next_states,
                             float* const* W, float* const* b, float* grad, float* state1, float* state2,
                             long long* step, int optim, double lr, double p1, double grad_clip, float* loss,
                             long long strideLoss, float* work, void* stream) {
  Plan p;
  int rc = make_plan("amx_efit_step", ctx, &p);
  if (rc) return rc;
  AMX_CHECK_ARG(ctx->have_norm, "amx_efit_step: context has no normalizers");
  AMX_CHECK_ARG(Bt > 0 && Bt % AMX_ROW_TILE == 0 && n_b >= 1 && n_b <= Bt, "amx_efit_step: n_b=%d Bt=%d", n_b, Bt);
  AMX_CHECK_ARG(idx && strideIdx >= n_b && n_rows >= 1, "amx_efit_step: idx / strideIdx=%lld / n_rows=%d", strideIdx,
                n_rows);
  AMX_CHECK_ARG(states && actions && next_states && W && b && loss && work, "amx_efit_step: null pointer");
  AMX_CHECK_ARG(amx::aligned16(work), "amx_efit_step: misaligned work");
  AMX_CHECK_ARG(optim == AMX_EFIT_ADAM || optim == AMX_EFIT_SGD, "amx_efit_step: optim=%d", optim);
  if (train) {
    AMX_CHECK_ARG(grad && state1 && step && (optim == AMX_EFIT_SGD || state2), "amx_efit_step: null training state");
    AMX_CHECK_ARG(amx::aligned16(grad) && amx::aligned16(state1) && amx::aligned16(state2) &&
                      ((uintptr_t)step & 7u) == 0, "amx_efit_step: misaligned training state");
    AMX_CHECK_ARG(lr > 0.0 && grad_clip >= 0.0 && (optim == AMX_EFIT_ADAM ? p1 > 0.0 : p1 >= 0.0),
                  "amx_efit_step: lr=%g %s=%g grad_clip=%g", lr, optim == AMX_EFIT_ADAM ? "eps" : "momentum", p1,
                  grad_clip);
  }
  for (int i = 0; i <= p.L; ++i)
    AMX_CHECK_ARG(W[i] && b[i] && amx::aligned16(W[i]) && amx::aligned16(b[i]), "amx_efit_step: layer %d pointers", i);
  const int M = p.M, L = p.L, Hp = p.Hp, k0 = p.k0, ldk = p.ldk, NO = p.NO;
  const Work wl = work_layout(p, Bt);
  float* act = work + wl.act;
  float* pred = work + wl.pred;
  float* target = work + wl.target;
  float* dzL = work + wl.dzL;
  float* dzb[2] = {work + wl.dz, work + wl.dz + (long long)M * Bt * Hp};
  float* dact = work + wl.dact;
  double* part = (double*)(work + wl.part);
  float* cst = work + wl.cst;
  const long long sA = (long long)Bt * ldk, sO = (long long)Bt * NO, sH = (long long)Bt * Hp,
                  sD = (long long)Bt * L * Hp;
  hipStream_t st = (hipStream_t)stream;

  hipLaunchKernelGGL(k_efit_gather, dim3(Bt, M), dim3(256), 0, st, n_b, n_rows, idx, strideIdx, states, actions,
                     next_states, ctx->d_norm, p.S, p.A, k0, NO, act, ldk, sA, target, sO);
  AMX_CHECK_LAUNCH();
  // 64 x 64 tiles while 128 x 128 ones would leave compute units idle (bit-identical results)
  const bool small = (long long)M * (Bt / 128) * (Hp / 128) < ctx->n_cus;
  const auto fwd = small ? amx_gemm_bias_act_t64 : amx_gemm_bias_act;
  for (int i = 0; i < L; ++i) {
    const int K = k0 + i * Hp;
    rc = fwd(ctx, M, Bt, Hp, K, act, ldk, sA, W[i], K, (long long)Hp * K, b[i], Hp, act, ldk, sA, K,
                           AMX_ACT_RELU, stream);
    if (rc) return rc;
  }
  rc = fwd(ctx, M, Bt, NO, ldk, act, ldk, sA, W[L], ldk, (long long)NO * ldk, b[L], NO, pred, NO, sO, 0,
                         AMX_ACT_NONE, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_efit_loss, dim3(M), dim3(1024), 0, st, n_b, Bt, p.S, NO, pred, target, dzL, loss, strideLoss);
  AMX_CHECK_LAUNCH();
  if (!train) return AMX_OK;

  const int rows16 = amx::round_up(n_b, 16), rows64 = amx::round_up(n_b, 64);
  const float* dz = dzL;
  int ldz = NO;
  long long sZ = sO;
  for (int i = L; i >= 0; --i) {
    const int N = i == L ? NO : Hp, K = i == L ? ldk : k0 + i * Hp;
    hipLaunchKernelGGL(k_efit_wgrad, dim3((K + 63) / 64, N / 64, M), dim3(256), 0, st, rows16, K, dz, ldz, sZ, act, ldk,
                       sA, grad + p.offW[i], grad + p.offB[i], p.P);
    AMX_CHECK_LAUNCH();
    if (i == 0) break;
    // the reduction of the output layer stops at the last valid column's 16-block (dzL is zero past S)
    const int Nred = i == L ? amx::round_up(p.S, 16) : Hp;
    float* out = dzb[i & 1];
    hipLaunchKernelGGL(k_efit_dgrad, dim3(i * Hp / 64, rows64 / 64, M), dim3(256), 0, st, Nred, k0, i == L ? 0 : 1,
                       (i - 1) * Hp, dz, ldz, sZ, W[i], K, (long long)N * K, act, ldk, sA, dact, L * Hp, sD, out, Hp,
                       sH);
    AMX_CHECK_LAUNCH();
    dz = out;
    ldz = Hp;
    sZ = sH;
  }
  if (grad_clip > 0.0) {
    hipLaunchKernelGGL(k_efit_sumsq, dim3(EF_NB_SQ, M), dim3(256), 0, st, grad, p.P, part);
    AMX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_efit_prep, dim3(1), dim3(64), 0, st, M, optim == AMX_EFIT_ADAM, lr, p1, grad_clip, part, step,
                     cst);
  AMX_CHECK_LAUNCH();
  Tensors T = {};
  T.n = 2 * (L + 1);
  for (int i = 0; i <= L; ++i) {
    const long long N = i == L ? NO : Hp, K = i == L ? ldk : k0 + (long long)i * Hp;
    T.w[2 * i] = W[i]; T.stride[2 * i] = N * K; T.off[2 * i] = p.offW[i];
    T.w[2 * i + 1] = b[i]; T.stride[2 * i + 1] = N; T.off[2 * i + 1] = p.offB[i];
  }
  T.off[T.n] = p.P;
  hipLaunchKernelGGL(k_efit_update, dim3(256, M), dim3(256), 0, st, T, optim == AMX_EFIT_ADAM, grad, state1, state2,
                     p.P, cst);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}
