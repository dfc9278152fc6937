// Training the AMP/GAIL discriminator on the device: one optimizer step of GAILCost.update_disc
// (milo/milo/gail_cost.py:104-204) for the two-hidden-layer ReLU discriminator
//   x [B, D] -> h0 = relu(x W0^T + b0) -> h1 = relu(h0 W1^T + b1) -> out = h1 w2^T + b2.
//
// Row-stacked workspaces of Bt rows per block: X = [x_e | x_m | U], H0s = [h0_e | h0_m | q0],
// Z1 = [dz1_e | dz1_m | a1], Z0 = [dz0_e | dz0_m | a0], so every product of the gradient
// penalty's double backward rides in the launch of the ordinary backward product of the same
// weight.  With the ReLU masks m0 = (h0_e > 0), m1 = (h1_e > 0) constant in the double backward:
//   a1 = m1 * w2, a0 = m0 * (a1 W1), g = a0 W0 = d out / d x, U = (lambda / (2 bs)) g / |g|,
//   gW0 += a0^T U, q0 = m0 * (U W0^T), gW1 += a1^T q0, gw2 += sum_rows m1 * (q0 W1^T).
//
//   k_dfit_gather   expert / agent rows through the two index vectors into X[0 : 2 Bt]
//   amx_gemm_bias_act_t64 x 2   the forward on the fp32 master weights (f32 MFMA, amx_gemm64.hip)
//   k_dfit_head     out, d out by loss type, Z1's three blocks
//   k_optim_sumsq   partial sums of the logged regularizer sum 1/2 W^2 over W0, W1, w2 (no
//                   gradient; the padding is zero; amx_optim.hip)
//   k_gemm64<NN>    Z0 = (Z1 W1) * (h0 > 0);  g = a0 W0               (amx_gemm64.hip)
//   k_dfit_unit     |g| per expert row, U into X[2 Bt : 3 Bt]
//   k_gemm64<NT>    q0 = (U W0^T) * m0 into H0s[2 Bt :];  P1 = (q0 W1^T) * m1
//   k_gemm64<TN>    gW1 = Z1^T H0s, gb1 = column sums of Z1[: 2 Bt];  gW0 = Z0^T X, gb0
//   k_dfit_gw2      gw2 = dout^T h1 + column sums of P1
//   k_dfit_prep     the metrics (fp64, fixed tree), gb2, the step count and Adam's corrections
//   k_optim_update  torch.optim.SGD (momentum, no Nesterov) / Adam on the six padded tensors
//                   (amx_optim.hip)
//
// Stream order is the only synchronisation; every sum runs in a fixed order, so a step is
// bit-reproducible.  Zero-padded weights see a zero gradient and stay exactly 0 with their state.
#include <math.h>

#include "amx_gemm64.h"
#include "amx_optim.h"

namespace {

using amx::wave_sum;

constexpr int DF_NB_REG = amx::SUMSQ_NB;        // partial sums of the regularizer
constexpr int DF_CONST = amx::STEP_CONST_FLOATS;  // floats of the step constants
constexpr int DF_T = 6;                         // W0, b0, W1, b1, w2, b2

struct Plan {
  int Dp, H0p, H1p;
  long long off[DF_T + 1];
};

int make_plan(const char* fn, int Dp, int H0p, int H1p, Plan* p) {
  AMX_CHECK_ARG(Dp > 0 && Dp % 32 == 0 && H0p > 0 && H0p % 128 == 0 && H1p > 0 && H1p % 128 == 0,
                "%s: Dp=%d (multiple of 32) H0p=%d H1p=%d (multiples of 128)", fn, Dp, H0p, H1p);
  p->Dp = Dp; p->H0p = H0p; p->H1p = H1p;
  const long long n[DF_T] = {(long long)H0p * Dp, H0p, (long long)H1p * H0p, H1p, H1p, 4};
  p->off[0] = 0;
  for (int i = 0; i < DF_T; ++i) p->off[i + 1] = p->off[i] + n[i];
  return AMX_OK;
}

// workspace layout in floats (every offset a multiple of 4)
struct Work {
  long long X, H0s, H1, Z1, Z0, G, P1, out, dout, norm, grad, part, cst, total;
};

Work work_layout(const Plan& p, int Bt) {
  Work w;
  long long o = 0;
  w.X = o;    o += 3LL * Bt * p.Dp;
  w.H0s = o;  o += 3LL * Bt * p.H0p;
  w.H1 = o;   o += 2LL * Bt * p.H1p;
  w.Z1 = o;   o += 3LL * Bt * p.H1p;
  w.Z0 = o;   o += 3LL * Bt * p.H0p;
  w.G = o;    o += (long long)Bt * p.Dp;
  w.P1 = o;   o += (long long)Bt * p.H1p;
  w.out = o;  o += 2LL * Bt;
  w.dout = o; o += 2LL * Bt;
  w.norm = o; o += Bt;
  w.grad = o; o += p.off[DF_T];
  w.part = o; o += 2LL * DF_NB_REG;  // doubles
  w.cst = o;  o += DF_CONST;
  w.total = o;
  return w;
}

__global__ __launch_bounds__(128) void k_dfit_gather(int bs, int Bt, int D, int Dp, const int32_t* __restrict__ idx_e,
                                                     const int32_t* __restrict__ idx_m,
                                                     const float* __restrict__ expert, long long lde, int n_e,
                                                     const float* __restrict__ agent, long long lda, int n_a,
                                                     float* __restrict__ X) {
  const int r = blockIdx.x, half = r >= Bt, rl = r - half * Bt;
  float* x = X + (long long)r * Dp;
  const float* src = nullptr;
  if (rl < bs) {
    const int32_t* idx = half ? idx_m : idx_e;
    const int n = half ? n_a : n_e;
    const int i = amx::clamp_row(idx ? idx[rl] : rl, n);
    src = half ? agent + i * lda : expert + i * lde;
  }
  for (int c = threadIdx.x; c < Dp; c += 128) x[c] = (src && c < D) ? src[c] : 0.f;
}

// one wave per row of H1 = [h1_e | h1_m]: out = h1 . w2 + b2, d out by loss type (ce, cm: the
// loss's coefficients over bs), dz1 = dout w2 (h1 > 0), and for expert rows a1 = w2 (h1 > 0)
__global__ __launch_bounds__(256) void k_dfit_head(int ls, int bs, int Bt, int H1p, float ce, float cm,
                                                   const float* __restrict__ H1, const float* __restrict__ w2,
                                                   const float* __restrict__ b2, float* __restrict__ out,
                                                   float* __restrict__ dout, float* __restrict__ Z1) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int half = r >= Bt, rl = r - half * Bt;
  const float* h = H1 + (long long)r * H1p;
  float s = 0.f;
  for (int c = lane; c < H1p; c += 64) s = fmaf(h[c], w2[c], s);
  const float o = wave_sum(s) + b2[0];
  float d = 0.f;
  if (rl < bs) {
    if (ls) {
      d = half ? cm * (o + 1.f) : ce * (o - 1.f);
    } else {
      const float sg = 1.f / (1.f + expf(-o));
      d = half ? cm * sg : -ce * (1.f - sg);
    }
  }
  if (lane == 0) {
    out[r] = o;
    dout[r] = d;
  }
  float* z = Z1 + (long long)r * H1p;
  for (int c = lane; c < H1p; c += 64) z[c] = h[c] > 0.f ? d * w2[c] : 0.f;
  if (!half) {
    float* a1 = Z1 + (long long)(2 * Bt + r) * H1p;
    for (int c = lane; c < H1p; c += 64) a1[c] = (rl < bs && h[c] > 0.f) ? w2[c] : 0.f;
  }
}

// one wave per expert row: |g|_2 and U = coef g / |g| (0 for rows >= bs and where |g| = 0,
// as torch's norm backward)
__global__ __launch_bounds__(256) void k_dfit_unit(int bs, int Dp, float coef, const float* __restrict__ G,
                                                   float* __restrict__ U, float* __restrict__ norm) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const float* g = G + (long long)r * Dp;
  float s = 0.f;
  for (int c = lane; c < Dp; c += 64) s = fmaf(g[c], g[c], s);
  const float nr = r < bs ? sqrtf(wave_sum(s)) : 0.f;
  if (lane == 0) norm[r] = nr;
  float* u = U + (long long)r * Dp;
  for (int c = lane; c < Dp; c += 64) u[c] = nr > 0.f ? (coef * g[c]) / nr : 0.f;
}

// gw2[c] = sum_{r < 2 Bt} dout[r] h1[r][c] + sum_{r < Bt} P1[r][c]: 64 columns per workgroup,
// sixteen row phases summed in a fixed tree
__global__ __launch_bounds__(1024) void k_dfit_gw2(int Bt, int H1p, const float* __restrict__ dout,
                                                   const float* __restrict__ H1, const float* __restrict__ P1,
                                                   float* __restrict__ gw2) {
  __shared__ float red[16][64];
  const int lc = threadIdx.x & 63, c = blockIdx.x * 64 + lc, ph = threadIdx.x >> 6;
  float s = 0.f;
  for (int r = ph; r < 2 * Bt; r += 16) s = fmaf(dout[r], H1[(long long)r * H1p + c], s);
  for (int r = ph; r < Bt; r += 16) s += P1[(long long)r * H1p + c];
  red[ph][lc] = s;
  __syncthreads();
  // (a tree of its own: fp32, over the 16 row phases of each column, not amx::block_sum's fp64 over threads)
  for (int o = 8; o > 0; o >>= 1) {
    if (ph < o) red[ph][lc] += red[ph + o][lc];
    __syncthreads();
  }
  if (ph == 0) gw2[c] = red[0][lc];
}

__device__ inline double softplus(double x) { return log1p(exp(-fabs(x))) + (x > 0.0 ? x : 0.0); }

// metrics[0..7] = expert loss, agent loss, penalty (x grad_lambda), regularizer (x reg_coef),
// total, expert accuracy, agent accuracy, step count; gb2; the optimizer's step constants
__global__ __launch_bounds__(256) void k_dfit_prep(int ls, int bs, int Bt, int adam, double lr, double p1, double c,
                                                   double reg_coef, double grad_lambda, const float* __restrict__ out,
                                                   const float* __restrict__ dout, const float* __restrict__ norm,
                                                   const double* __restrict__ part, float* __restrict__ gb2,
                                                   long long* __restrict__ step, float* __restrict__ cst,
                                                   double* __restrict__ metrics) {
  __shared__ double red[256];
  __shared__ double tot[7];
  const int tid = threadIdx.x;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};  // e, m, acc_e, acc_m, norm, reg, gb2
  for (int r = tid; r < bs; r += 256) {
    const double oe = out[r], om = out[Bt + r];
    if (ls) {
      v[0] += (oe - 1.0) * (oe - 1.0);
      v[1] += (om + 1.0) * (om + 1.0);
    } else {
      v[0] += softplus(-oe);   // -log sigmoid(out_e)
      v[1] += softplus(om);    // -log(1 - sigmoid(out_m))
    }
    v[2] += out[r] > 0.f ? 1.0 : 0.0;
    v[3] += out[Bt + r] < 0.f ? 1.0 : 0.0;
    v[4] += (double)norm[r];
    v[6] += (double)dout[r] + (double)dout[Bt + r];
  }
  for (int b = tid; b < DF_NB_REG; b += 256) v[5] += part[b];
  for (int k = 0; k < 7; ++k) {
    const double s = amx::block_sum<256>(red, v[k]);
    if (tid == 0) tot[k] = s;
    __syncthreads();
  }
  if (tid != 0) return;
  const double e = tot[0] / bs, m = tot[1] / bs, pen = grad_lambda * 0.5 * tot[4] / bs, reg = reg_coef * tot[5];
  const long long t = step[0] + 1;
  step[0] = t;
  metrics[0] = e;
  metrics[1] = m;
  metrics[2] = pen;
  metrics[3] = reg;
  metrics[4] = c * e + (1.0 - c) * m + reg + pen;
  metrics[5] = tot[2] / bs;
  metrics[6] = tot[3] / bs;
  metrics[7] = (double)t;
  gb2[0] = (float)tot[6];
  gb2[1] = gb2[2] = gb2[3] = 0.f;
  amx::StepConst s = {};
  s.coef = 1.f;  // no clipping
  if (adam) {
    s.adam = amx::AdamConst(t, lr, 0.9, 0.999, p1);
  } else {
    s.lr = (float)lr;
    s.mu = (float)p1;
  }
  *(amx::StepConst*)cst = s;
}

}  // namespace

extern "C" long long amx_dfit_param_count(int Dp, int H0p, int H1p) {
  Plan p;
  if (make_plan("amx_dfit_param_count", Dp, H0p, H1p, &p)) return -1;
  return p.off[DF_T];
}

extern "C" long long amx_dfit_work_floats(int Dp, int H0p, int H1p, int Bt) {
  Plan p;
  if (make_plan("amx_dfit_work_floats", Dp, H0p, H1p, &p)) return -1;
  if (Bt <= 0 || Bt % 64) {
    amx::set_error("amx_dfit_work_floats: Bt=%d is not a positive multiple of 64", Bt);
    return -1;
  }
  return work_layout(p, Bt).total;
}

extern "C" int amx_dfit_step(amx_ctx* ctx, int loss_type, int optim, double lr, double p1, double scaling_coef,
                             double reg_coef, double grad_lambda, int bs, int Bt, int D, int Dp, int H0p, int H1p,
                             const int32_t* idx_e, const int32_t* idx_m, const float* expert, long long ld_expert,
                             int n_expert, const float* agent, long long ld_agent, int n_agent, float* W0, float* b0,
                             float* W1, float* b1, float* w2, float* b2, float* state1, float* state2,
                             long long* step, float* work, double* metrics, void* stream) {
  const char* fn = "amx_dfit_step";
  AMX_CHECK_ARG(ctx, "%s: null ctx", fn);
  Plan p;
  int rc = make_plan(fn, Dp, H0p, H1p, &p);
  if (rc) return rc;
  AMX_CHECK_ARG(loss_type == AMX_DISC_LEAST_SQUARES || loss_type == AMX_DISC_LOG_LIKELIHOOD, "%s: loss_type=%d", fn,
                loss_type);
  AMX_CHECK_ARG(optim == AMX_DFIT_SGD || optim == AMX_DFIT_ADAM, "%s: optim=%d", fn, optim);
  AMX_CHECK_ARG(Bt > 0 && Bt % 64 == 0 && bs >= 1 && bs <= Bt, "%s: bs=%d Bt=%d", fn, bs, Bt);
  AMX_CHECK_ARG(D >= 1 && D <= Dp, "%s: D=%d Dp=%d", fn, D, Dp);
  AMX_CHECK_ARG(idx_e && expert && agent && ld_expert >= D && ld_agent >= D && n_expert >= 1 && n_agent >= 1,
                "%s: tables (ld_expert=%lld ld_agent=%lld D=%d n_expert=%d n_agent=%d)", fn, ld_expert, ld_agent, D,
                n_expert, n_agent);
  AMX_CHECK_ARG(idx_m || n_agent >= bs, "%s: %d agent rows given for bs=%d and no index vector", fn, n_agent, bs);
  AMX_CHECK_ARG(W0 && b0 && W1 && b1 && w2 && b2 && state1 && step && work && metrics, "%s: null pointer", fn);
  AMX_CHECK_ARG(optim == AMX_DFIT_SGD || state2, "%s: Adam needs state2", fn);
  AMX_CHECK_ARG(amx::aligned16(W0) && amx::aligned16(b0) && amx::aligned16(W1) && amx::aligned16(b1) &&
                    amx::aligned16(w2) && amx::aligned16(b2) && amx::aligned16(state1) && amx::aligned16(state2) &&
                    amx::aligned16(work) && ((uintptr_t)step & 7u) == 0 && ((uintptr_t)metrics & 7u) == 0,
                "%s: misaligned pointer", fn);
  AMX_CHECK_ARG(lr > 0.0 && (optim == AMX_DFIT_ADAM ? p1 > 0.0 : p1 >= 0.0) && scaling_coef >= 0.0 &&
                    scaling_coef <= 1.0 && grad_lambda >= 0.0,
                "%s: lr=%g %s=%g scaling_coef=%g grad_lambda=%g", fn, lr, optim == AMX_DFIT_ADAM ? "eps" : "momentum",
                p1, scaling_coef, grad_lambda);
  const Work wl = work_layout(p, Bt);
  float* X = work + wl.X;
  float* H0s = work + wl.H0s;
  float* H1 = work + wl.H1;
  float* Z1 = work + wl.Z1;
  float* Z0 = work + wl.Z0;
  float* G = work + wl.G;
  float* P1 = work + wl.P1;
  float* out = work + wl.out;
  float* dout = work + wl.dout;
  float* norm = work + wl.norm;
  float* grad = work + wl.grad;
  double* part = (double*)(work + wl.part);
  float* cst = work + wl.cst;
  float* U = X + 2LL * Bt * Dp;
  hipStream_t st = (hipStream_t)stream;
  const int ls = loss_type == AMX_DISC_LEAST_SQUARES;

  hipLaunchKernelGGL(k_dfit_gather, dim3(2 * Bt), dim3(128), 0, st, bs, Bt, D, Dp, idx_e, idx_m, expert, ld_expert,
                     n_expert, agent, ld_agent, n_agent, X);
  AMX_CHECK_LAUNCH();
  rc = amx_gemm_bias_act_t64(ctx, 1, 2 * Bt, H0p, Dp, X, Dp, 0, W0, Dp, 0, b0, 0, H0s, H0p, 0, 0, AMX_ACT_RELU, stream);
  if (rc) return rc;
  rc = amx_gemm_bias_act_t64(ctx, 1, 2 * Bt, H1p, H0p, H0s, H0p, 0, W1, H0p, 0, b1, 0, H1, H1p, 0, 0, AMX_ACT_RELU,
                             stream);
  if (rc) return rc;
  const double c = scaling_coef;
  const float ce = (float)((ls ? 2.0 : 1.0) * c / bs), cm = (float)((ls ? 2.0 : 1.0) * (1.0 - c) / bs);
  hipLaunchKernelGGL(k_dfit_head, dim3(2 * Bt / 4), dim3(256), 0, st, ls, bs, Bt, H1p, ce, cm, H1, w2, b2, out, dout,
                     Z1);
  AMX_CHECK_LAUNCH();
  amx::TensorList R = {};  // the regularizer sum 1/2 W^2 runs over the three weights
  R.n = 3;
  R.w[0] = W0; R.w[1] = W1; R.w[2] = w2;
  R.off[1] = p.off[1] - p.off[0];
  R.off[2] = R.off[1] + (p.off[3] - p.off[2]);
  R.off[3] = R.off[2] + (p.off[5] - p.off[4]);
  if ((rc = amx::sum_squares(R, 1, 0.5, part, st))) return rc;
  amx::Gemm64Args g = {};
  // Z0 = (Z1 W1) * (h0 > 0); the a1 block takes the expert rows' h0
  g.A = Z1; g.lda = H1p; g.B = W1; g.ldb = H0p; g.C = Z0; g.ldc = H0p;
  g.mask = H0s; g.ldm = H0p; g.mask_mod = 2 * Bt;
  g.M = 3 * Bt; g.N = H0p; g.K = H1p;
  if ((rc = amx::gemm64_nn(g, st))) return rc;
  // g = a0 W0
  g = amx::Gemm64Args{};
  g.A = Z0 + 2LL * Bt * H0p; g.lda = H0p; g.B = W0; g.ldb = Dp; g.C = G; g.ldc = Dp;
  g.M = Bt; g.N = Dp; g.K = H0p;
  if ((rc = amx::gemm64_nn(g, st))) return rc;
  hipLaunchKernelGGL(k_dfit_unit, dim3(Bt / 4), dim3(256), 0, st, bs, Dp, (float)(grad_lambda / (2.0 * bs)), G, U,
                     norm);
  AMX_CHECK_LAUNCH();
  // q0 = (U W0^T) * (h0_e > 0)
  g = amx::Gemm64Args{};
  g.A = U; g.lda = Dp; g.B = W0; g.ldb = Dp; g.C = H0s + 2LL * Bt * H0p; g.ldc = H0p;
  g.mask = H0s; g.ldm = H0p;
  g.M = Bt; g.N = H0p; g.K = Dp;
  if ((rc = amx::gemm64_nt(g, st))) return rc;
  // P1 = (q0 W1^T) * (h1_e > 0)
  g = amx::Gemm64Args{};
  g.A = H0s + 2LL * Bt * H0p; g.lda = H0p; g.B = W1; g.ldb = H0p; g.C = P1; g.ldc = H1p;
  g.mask = H1; g.ldm = H1p;
  g.M = Bt; g.N = H1p; g.K = H0p;
  if ((rc = amx::gemm64_nt(g, st))) return rc;
  // gW1 = Z1^T H0s, gb1 = column sums of Z1's ordinary rows
  g = amx::Gemm64Args{};
  g.A = Z1; g.lda = H1p; g.B = H0s; g.ldb = H0p; g.C = grad + p.off[2]; g.ldc = H0p;
  g.colsum = grad + p.off[3]; g.cs_rows = 2 * Bt;
  g.M = H1p; g.N = H0p; g.K = 3 * Bt;
  if ((rc = amx::gemm64_tn(g, st))) return rc;
  // gW0 = Z0^T X, gb0
  g = amx::Gemm64Args{};
  g.A = Z0; g.lda = H0p; g.B = X; g.ldb = Dp; g.C = grad + p.off[0]; g.ldc = Dp;
  g.colsum = grad + p.off[1]; g.cs_rows = 2 * Bt;
  g.M = H0p; g.N = Dp; g.K = 3 * Bt;
  if ((rc = amx::gemm64_tn(g, st))) return rc;
  hipLaunchKernelGGL(k_dfit_gw2, dim3(H1p / 64), dim3(1024), 0, st, Bt, H1p, dout, H1, P1, grad + p.off[4]);
  AMX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dfit_prep, dim3(1), dim3(256), 0, st, ls, bs, Bt, optim == AMX_DFIT_ADAM, lr, p1, c, reg_coef,
                     grad_lambda, out, dout, norm, part, grad + p.off[5], step, cst, metrics);
  AMX_CHECK_LAUNCH();
  amx::TensorList T = {};
  float* w[DF_T] = {W0, b0, W1, b1, w2, b2};
  T.n = DF_T;
  for (int i = 0; i < DF_T; ++i) {
    T.w[i] = w[i];
    T.off[i] = p.off[i];
  }
  T.off[DF_T] = p.off[DF_T];
  const bool adam = optim == AMX_DFIT_ADAM;
  return amx::update_tensors(T, 1, adam ? amx::OPTIM_ADAM : amx::OPTIM_SGD, grad, state1, adam ? state2 : state1,
                             p.off[DF_T], cst, st);
}
