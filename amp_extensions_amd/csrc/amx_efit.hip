// Training the dynamics ensemble on the device: one optimizer step of DynamicsModel.train_step
// (milo/milo/dynamics.py:236-250) for all M members at once, each on its own index batch.
//
//   k_efit_gather   x0 = [(s - mu_s)/sd_s, (a - mu_a)/sd_a, 0-pad] and the normalised target
//                   ((s' - s) - mu_d)/sd_d of the batch's rows; rows >= n_b zero
//   amx_gemm_bias_act[_t64] x (L + 1)   the forward on the fp32 master weights (f32 MFMA; the
//                   64 x 64 tiles of amx_gemm64.hip while 128 x 128 ones would leave compute
//                   units idle)
//   k_efit_loss     dZ_L = 2 (pred - target)/(n_b S), the step's MSE into loss[g]
//   per layer i = L .. 0:
//     k_efit_wgrad  gW_i = dZ_i^T act, gb_i = column sums of dZ_i
//     k_efit_dgrad  dact[:, hidden slices < i] (+)= dZ_i W_i; the tiles of slice i - 1, final
//                   after this launch, write dZ_{i-1} = dact * (act > 0)
//   A plain context (AMX_CONNECT_PLAIN): layer i >= 1 has K = Hp and reads the window of layer
//   i - 1 alone, so its weight gradient is taken against that window and its k_efit_dgrad launch
//   covers that one slice, final at once (no accumulation, dact unused).
//   k_optim_sumsq   per-workgroup partial sums of g^2 (grad_clip > 0; amx_optim.hip)
//   k_efit_prep     clip_grad_norm_'s coefficient, the step count and Adam's bias corrections
//   k_optim_update  torch.optim.Adam / SGD(nesterov=True) on every padded tensor (amx_optim.hip)
//
// Stream order is the only synchronisation: no workgroup waits on another.  Every sum runs in
// a fixed order, so a fit is deterministic.  The backward products are fp32 FMA chains on the
// VALU over LDS tiles (the step is bound by its launches and weight traffic).
// Zero-padded weights see a zero gradient, so they and their optimizer state stay exactly 0.
#include <math.h>

#include "amx_optim.h"

namespace {

constexpr int EF_MAX_LAYERS = 8;           // L + 1
static_assert(2 * EF_MAX_LAYERS <= amx::OPTIM_MAX_T, "weight and bias tensors of the update's list");
constexpr int EF_NB_SQ = amx::SUMSQ_NB;    // partial sums of g^2 per member
constexpr int EF_CONST = amx::STEP_CONST_FLOATS;  // floats of a member's step constants

struct Plan {
  int M, L, Hp, k0, ldk, NO, S, A;
  int plain;                     // layer i >= 1 reads the window of layer i - 1 only
  int K[EF_MAX_LAYERS];          // columns of W_i
  int in0[EF_MAX_LAYERS];        // first column of the activation row that layer i reads
  long long P;                   // floats of a member's flat gradient
  long long offW[EF_MAX_LAYERS], offB[EF_MAX_LAYERS];
};

int make_plan(const char* fn, const amx_ctx* c, Plan* p) {
  AMX_CHECK_ARG(c, "%s: null ctx", fn);
  AMX_CHECK_ARG(c->L >= 1 && c->L + 1 <= EF_MAX_LAYERS, "%s: %d hidden layers (supported: 1..%d)", fn, c->L,
                EF_MAX_LAYERS - 1);
  p->M = c->M; p->L = c->L; p->Hp = c->H; p->k0 = c->k0_pad; p->ldk = c->ldk; p->NO = c->n_out_pad;
  p->S = c->S; p->A = c->A;
  p->plain = c->plain;
  long long o = 0;
  for (int i = 0; i <= c->L; ++i) {
    const long long N = i == c->L ? c->n_out_pad : c->H;
    p->K[i] = (c->plain && i > 0) ? c->H : (i == c->L ? c->ldk : c->k0_pad + i * c->H);
    p->in0[i] = (c->plain && i > 0) ? c->k0_pad + (i - 1) * c->H : 0;
    const long long K = p->K[i];
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
  const int i = amx::clamp_row(idx[g * strideIdx + r], n_rows);
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
  const double sum = amx::block_sum<1024>(red, acc);
  if (tid == 0) loss[g * strideLoss] = (float)(sum / cnt);
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

// per member: clip_grad_norm_'s coefficient (max_norm / (norm + 1e-6), clamped to 1), the step
// count, Adam's bias corrections (beta^t in double)
__global__ void k_efit_prep(int M, int adam, double lr, double p1, double grad_clip, const double* __restrict__ part,
                            long long* __restrict__ step, float* __restrict__ cst) {
  const int g = threadIdx.x;
  if (g >= M) return;
  amx::StepConst c = {};
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
    c.adam = amx::AdamConst(t, lr, 0.9, 0.999, p1);
  } else {
    c.lr = (float)lr;
    c.mu = (float)p1;
  }
  *(amx::StepConst*)(cst + g * EF_CONST) = c;
}

}  // namespace

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
    const int K = p.K[i];
    rc = fwd(ctx, M, Bt, Hp, K, act + p.in0[i], ldk, sA, W[i], K, (long long)Hp * K, b[i], Hp, act, ldk, sA,
                           k0 + i * Hp, AMX_ACT_RELU, stream);
    if (rc) return rc;
  }
  rc = fwd(ctx, M, Bt, NO, p.K[L], act + p.in0[L], ldk, sA, W[L], p.K[L], (long long)NO * p.K[L], b[L], NO, pred, NO,
                         sO, 0, AMX_ACT_NONE, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_efit_loss, dim3(M), dim3(1024), 0, st, n_b, Bt, p.S, NO, pred, target, dzL, loss, strideLoss);
  AMX_CHECK_LAUNCH();
  if (!train) return AMX_OK;

  const int rows16 = amx::round_up(n_b, 16), rows64 = amx::round_up(n_b, 64);
  const float* dz = dzL;
  int ldz = NO;
  long long sZ = sO;
  for (int i = L; i >= 0; --i) {
    const int N = i == L ? NO : Hp, K = p.K[i];
    hipLaunchKernelGGL(k_efit_wgrad, dim3((K + 63) / 64, N / 64, M), dim3(256), 0, st, rows16, K, dz, ldz, sZ,
                       act + p.in0[i], ldk, sA, grad + p.offW[i], grad + p.offB[i], p.P);
    AMX_CHECK_LAUNCH();
    if (i == 0) break;
    // the reduction of the output layer stops at the last valid column's 16-block (dzL is zero past S)
    const int Nred = i == L ? amx::round_up(p.S, 16) : Hp;
    float* out = dzb[i & 1];
    if (p.plain) {
      // dZ_{i-1} = (dZ_i W_i) * (h_{i-1} > 0): W_i's Hp columns are that one window, whose ReLU
      // mask is read at act + in0[i] (k0 = 0, final_c0 = 0: every tile is final, dact untouched)
      hipLaunchKernelGGL(k_efit_dgrad, dim3(Hp / 64, rows64 / 64, M), dim3(256), 0, st, Nred, 0, 0, 0, dz, ldz, sZ, W[i],
                         K, (long long)N * K, act + p.in0[i], ldk, sA, dact, L * Hp, sD, out, Hp, sH);
      AMX_CHECK_LAUNCH();
      dz = out;
      ldz = Hp;
      sZ = sH;
      continue;
    }
    hipLaunchKernelGGL(k_efit_dgrad, dim3(i * Hp / 64, rows64 / 64, M), dim3(256), 0, st, Nred, k0, i == L ? 0 : 1,
                       (i - 1) * Hp, dz, ldz, sZ, W[i], K, (long long)N * K, act, ldk, sA, dact, L * Hp, sD, out, Hp,
                       sH);
    AMX_CHECK_LAUNCH();
    dz = out;
    ldz = Hp;
    sZ = sH;
  }
  if (grad_clip > 0.0) {
    amx::TensorList G = {};  // every member's flat gradient
    G.n = 1;
    G.w[0] = grad; G.stride[0] = p.P; G.off[1] = p.P;
    if ((rc = amx::sum_squares(G, M, 1.0, part, st))) return rc;
  }
  hipLaunchKernelGGL(k_efit_prep, dim3(1), dim3(64), 0, st, M, optim == AMX_EFIT_ADAM, lr, p1, grad_clip, part, step,
                     cst);
  AMX_CHECK_LAUNCH();
  amx::TensorList T = {};
  T.n = 2 * (L + 1);
  for (int i = 0; i <= L; ++i) {
    const long long N = i == L ? NO : Hp, K = p.K[i];
    T.w[2 * i] = W[i]; T.stride[2 * i] = N * K; T.off[2 * i] = p.offW[i];
    T.w[2 * i + 1] = b[i]; T.stride[2 * i + 1] = N; T.off[2 * i + 1] = p.offB[i];
  }
  T.off[T.n] = p.P;
  return amx::update_tensors(T, M, optim == AMX_EFIT_ADAM ? amx::OPTIM_ADAM : amx::OPTIM_SGD_NESTEROV, grad, state1,
                             state2, p.P, cst, st);
}
