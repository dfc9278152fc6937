// Fitting the MLP value baseline on the device: one epoch of mjrl's fit_data
// (mjrl/mjrl/utils/optimize_model.py:21-35) as MLPBaseline.fit drives it
// (mjrl/mjrl/baselines/mlp_baseline.py:61-97): mini-batches of 64 rows gathered through a
// permutation, the (S+4) -> H0 -> H1 -> 1 ReLU MLP forward, MSELoss, autograd's backward and
// torch.optim.Adam with weight decay, all in fp32 on the VALU.
//
// The steps of an epoch depend on each other (every step reads the weights the one before
// wrote), and no workgroup here ever waits on another: a step is a chain of four launches, and
// the stream order is the only synchronisation.
//   k_vfit_l0    gather + h0 = relu(x W0^T + b0); keeps the gathered batch   8 workgroups (16 columns each)
//   k_vfit_l1    h1 = relu(h0 W1^T + b1), per-workgroup head partials        8 workgroups
//   k_vfit_bwd   y^, dy, dz1; gW1 = dz1^T h0 (workgroups 0-7); dz0 = (dz1 W1) * (h0 > 0) from the
//                old W1 (8-15); the loss sum, Adam's step count and bias corrections (16)
//   k_vfit_adam  gW0 = dz0^T x per owned element, straight into Adam (workgroups 0-15); Adam on
//                W1, the biases and the head (16-23)
// Adam's step count lives in device memory (one thread of k_vfit_bwd advances it by a plain
// store; nothing else in that launch reads it); the mini-batch index is a launch argument.
//
// The kernels are latency-bound (a step is 17.7 MFLOP over 8-24 workgroups), so each one issues
// all the global loads it can before its first barrier: a launch pays one or two memory round
// trips, not one per K chunk.  Activations and their gradients are stored feature-major
// ([column][row], 64 rows), which keeps every global access of the chain coalesced.
// Reductions run in a fixed order: the result is deterministic.  Zero-padded weights see a zero
// gradient and no decay (wd * 0), so Adam leaves them, and their moments, exactly 0.
// Adam's constants and update are amx_optim.h's (AdamConst, adam_apply); the decay is added here.
#include <math.h>

#include "amx_optim.h"

namespace {

constexpr int VB = 64;    // mini-batch rows (MLPBaseline's batch_size)
constexpr int VH = 128;   // padded hidden width (both layers)
constexpr int VT = 16;    // columns per workgroup tile
constexpr int VNB = VH / VT;
constexpr int KC = 128;   // K columns staged in LDS at a time

// workspace layout in floats; the gathered batch xb [VB][kf] follows at W_XB
constexpr int W_LOSS = 0;                   // sum of the epoch's step losses
constexpr int W_ADAM = 8;                   // struct Adam of the current step (k_vfit_bwd -> k_vfit_adam)
constexpr int W_H0 = 64;                    // h0t [VH][VB]
constexpr int W_H1 = W_H0 + VH * VB;        // h1t [VH][VB]
constexpr int W_DZ1 = W_H1 + VH * VB;       // dz1t [VH][VB]
constexpr int W_DZ0 = W_DZ1 + VH * VB;      // dz0t [VH][VB]
constexpr int W_GW1 = W_DZ0 + VH * VB;      // gW1 [VH][VH]
constexpr int W_HP = W_GW1 + VH * VH;       // head partials [VNB][VB]
constexpr int W_Y = W_HP + VNB * VB;        // batch targets [VB]
constexpr int W_DY = W_Y + VB;              // dy [VB]
constexpr int W_XB = W_DY + VB;

struct Adam {
  amx::AdamConst c;
  float wd;
};
static_assert(W_ADAM + sizeof(Adam) / sizeof(float) <= W_H0, "workspace header");

// torch.optim.Adam with weight decay: grad.add(p, alpha=wd), then amx_optim.h's update
__device__ inline void adam_math(float& w, float& m, float& v, float g, const Adam& a) {
  g = g + a.wd * w;
  amx::adam_apply(w, m, v, g, a.c);
}

__device__ inline void adam_update(float* w, float* m, float* v, float g, const Adam& a) {
  float w1 = *w, m1 = *m, v1 = *v;
  adam_math(w1, m1, v1, g, a);
  *w = w1;
  *m = m1;
  *v = v1;
}

// y^ from the head partials in workgroup order, then d = y^ - y (one thread per batch row)
__device__ inline float batch_residual(const float* __restrict__ work, const float* __restrict__ b2, int r) {
  float yh = work[W_HP + r];
#pragma unroll
  for (int b = 1; b < VNB; ++b) yh += work[W_HP + b * VB + r];
  return (yh + b2[0]) - work[W_Y + r];
}

// rows of mini-batch mb; an index outside [0, n_rows) is clamped (callers validate perm)
__device__ inline void batch_rows(int* sidx, const int32_t* __restrict__ perm, int mb, int n_rows) {
  if (threadIdx.x < VB) {
    sidx[threadIdx.x] = amx::clamp_row(perm[(long long)mb * VB + threadIdx.x], n_rows);
  }
}

__global__ void k_vfit_begin(float* __restrict__ work) {
  if (threadIdx.x == 0) work[W_LOSS] = 0.f;
}

// 64 x 16 output tile of A W^T: thread (r = tid & 63, cg = tid >> 6) owns row r, columns
// cg*4 .. cg*4+3 of the tile; up to KC columns of K staged in LDS (rows padded to KC + 1).
struct TileLds {
  float a[VB][KC + 1];
  float w[VT][KC + 1];
};

__device__ inline void tile_mac(const TileLds& s, int kc, float acc[4]) {
  const int r = threadIdx.x & 63, cg = threadIdx.x >> 6;
#pragma unroll 8
  for (int k = 0; k < kc; ++k) {
    const float x = s.a[r][k];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(x, s.w[cg * 4 + j][k], acc[j]);
  }
}

__global__ __launch_bounds__(256) void k_vfit_l0(int mb, int n_rows, const float* __restrict__ feat, int ldf,
                                                 const int32_t* __restrict__ perm, int kf,
                                                 const float* __restrict__ W0, const float* __restrict__ b0,
                                                 float* __restrict__ work) {
  __shared__ TileLds s;
  __shared__ int sidx[VB];
  const int tid = threadIdx.x, r = tid & 63, cg = tid >> 6, c0 = blockIdx.x * VT;
  const int kk = tid & (KC - 1), rh = tid >> 7;  // staging: column kk of rows rh + 2 i / W rows rh + 2 i
  batch_rows(sidx, perm, mb, n_rows);
  __syncthreads();
  float ra[32], rw[8];
  float* xb = work + W_XB;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // all of a K block's loads in flight at once; the next block's during this block's products
  auto load = [&](int k0) {
    if (k0 + kk < kf) {
#pragma unroll
      for (int i = 0; i < 32; ++i) ra[i] = feat[(long long)sidx[rh + 2 * i] * ldf + k0 + kk];
#pragma unroll
      for (int i = 0; i < 8; ++i) rw[i] = W0[(long long)(c0 + rh + 2 * i) * kf + k0 + kk];
    }
  };
  load(0);
  for (int k0 = 0; k0 < kf; k0 += KC) {
    const int kc = kf - k0 < KC ? kf - k0 : KC;
    if (k0) __syncthreads();  // the previous block's reads of the tile are done
    if (kk < kc) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        s.a[rh + 2 * i][kk] = ra[i];
        // this workgroup's 8 rows of the gathered batch, for k_vfit_adam
        if ((i >> 2) == (int)blockIdx.x) xb[(rh + 2 * i) * kf + k0 + kk] = ra[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s.w[rh + 2 * i][kk] = rw[i];
    }
    __syncthreads();
    if (k0 + KC < kf) load(k0 + KC);
    tile_mac(s, kc, acc);
  }
  float* h0t = work + W_H0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + cg * 4 + j;
    const float z = acc[j] + b0[c];
    h0t[c * VB + r] = z > 0.f ? z : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_vfit_l1(int mb, int n_rows, const float* __restrict__ returns,
                                                 const int32_t* __restrict__ perm, const float* __restrict__ W1,
                                                 const float* __restrict__ b1, const float* __restrict__ w2,
                                                 float* __restrict__ work) {
  __shared__ TileLds s;
  __shared__ float red[4][VB];
  const int tid = threadIdx.x, r = tid & 63, cg = tid >> 6, c0 = blockIdx.x * VT;
  const float* h0t = work + W_H0;
  float ra[32], rw[8];
#pragma unroll
  for (int i = 0; i < 32; ++i) ra[i] = h0t[(cg + 4 * i) * VB + r];  // h0[r][k], k = cg + 4 i
#pragma unroll
  for (int i = 0; i < 8; ++i) rw[i] = W1[(c0 + (tid >> 7) + 2 * i) * VH + (tid & 127)];
  if (blockIdx.x == 0 && tid < VB) {  // the batch's targets, for k_vfit_bwd
    work[W_Y + tid] = returns[amx::clamp_row(perm[(long long)mb * VB + tid], n_rows)];
  }
#pragma unroll
  for (int i = 0; i < 32; ++i) s.a[r][cg + 4 * i] = ra[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) s.w[(tid >> 7) + 2 * i][tid & 127] = rw[i];
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  tile_mac(s, VH, acc);
  float* h1t = work + W_H1;
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + cg * 4 + j;
    const float z = acc[j] + b1[c];
    const float h = z > 0.f ? z : 0.f;
    h1t[c * VB + r] = h;
    p = fmaf(h, w2[c], p);
  }
  red[cg][r] = p;
  __syncthreads();
  if (tid < VB) work[W_HP + blockIdx.x * VB + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void k_vfit_bwd(const float* __restrict__ W1, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, float* __restrict__ work,
                                                  long long* __restrict__ adam_step, int num_steps, double lr,
                                                  double beta1, double beta2, double eps, double wd,
                                                  float* __restrict__ epoch_loss) {
  __shared__ float big[VB][VH + 1];  // h0 (workgroups 0-7) or dz1 (8-15), row-major
  __shared__ float small[VH * VT];   // dz1 tile [VB][VT] or W1 tile [VH][VT]
  __shared__ float sdy[VB];
  const int tid = threadIdx.x, r = tid & 63, cg = tid >> 6;
  const float* h0t = work + W_H0;
  const float* h1t = work + W_H1;
  if (blockIdx.x == 2 * VNB) {  // bookkeeping, beside the two products
    if (tid < VB) {
      const float d = batch_residual(work, b2, tid);
      work[W_DY + tid] = (2.f * d) * (1.f / VB);
      const float loss = amx::wave_sum(d * d) * (1.f / VB);
      if (tid == 0) {
        const float ls = work[W_LOSS] + loss;
        work[W_LOSS] = ls;
        epoch_loss[0] = ls / (float)num_steps;
        const long long t = adam_step[0] + 1;
        adam_step[0] = t;
        *(Adam*)(work + W_ADAM) = Adam{amx::AdamConst(t, lr, beta1, beta2, eps), (float)wd};  // beta^t in double
      }
    }
    return;
  }
  const bool gw = blockIdx.x < VNB;
  const int t0 = (gw ? blockIdx.x : blockIdx.x - VNB) * VT;  // first column of this workgroup's tile
  // every global load before the first barrier: element (r, cg + 4 i) of h0 / h1, the small tile's source
  float rb[32], rs[8], w2r[32], hk[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 32; ++i) rb[i] = (gw ? h0t : h1t)[(cg + 4 * i) * VB + r];
  if (gw) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rs[i] = h1t[(t0 + cg + 4 * i) * VB + r];
      w2r[i] = w2[t0 + cg + 4 * i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) rs[i] = W1[((tid >> 4) + 16 * i) * VH + t0 + (tid & 15)];
#pragma unroll
    for (int i = 0; i < 32; ++i) w2r[i] = w2[cg + 4 * i];
#pragma unroll
    for (int j = 0; j < 4; ++j) hk[j] = h0t[(t0 + cg * 4 + j) * VB + r];
  }
  if (tid < VB) sdy[tid] = (2.f * batch_residual(work, b2, tid)) * (1.f / VB);
  __syncthreads();
  if (gw) {
    // gW1[c][k] = sum_r dz1[r][c] h0[r][k] for the 16 columns c of this workgroup
    float* dz1t = work + W_DZ1;
#pragma unroll
    for (int i = 0; i < 32; ++i) big[r][cg + 4 * i] = rb[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cc = cg + 4 * i;
      const float z = rs[i] > 0.f ? sdy[r] * w2r[i] : 0.f;
      small[r * VT + cc] = z;
      dz1t[(t0 + cc) * VB + r] = z;
    }
    __syncthreads();
    const int k = tid & 127, half = tid >> 7;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = 0; q < VB; ++q) {
      const float a = big[q][k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(small[q * VT + half * 8 + j], a, acc[j]);
    }
    float* gW1 = work + W_GW1;
#pragma unroll
    for (int j = 0; j < 8; ++j) gW1[(t0 + half * 8 + j) * VH + k] = acc[j];
  } else {
    // dz0[r][k] = (sum_c dz1[r][c] W1[c][k]) * (h0[r][k] > 0) for the 16 columns k of this workgroup
#pragma unroll
    for (int i = 0; i < 32; ++i) big[r][cg + 4 * i] = rb[i] > 0.f ? sdy[r] * w2r[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) small[((tid >> 4) + 16 * i) * VT + (tid & 15)] = rs[i];
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int c = 0; c < VH; ++c) {
      const float z = big[r][c];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(z, small[c * VT + cg * 4 + j], acc[j]);
    }
    float* dz0t = work + W_DZ0;
#pragma unroll
    for (int j = 0; j < 4; ++j) dz0t[(t0 + cg * 4 + j) * VB + r] = hk[j] > 0.f ? acc[j] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_vfit_adam(int kf, float* __restrict__ W0, float* __restrict__ b0,
                                                   float* __restrict__ W1, float* __restrict__ b1,
                                                   float* __restrict__ w2, float* __restrict__ b2,
                                                   float* __restrict__ am, float* __restrict__ av,
                                                   const float* __restrict__ work) {
  constexpr int JT = 8, NW0 = VH / JT;  // W0 rows per workgroup, workgroups over W0
  __shared__ float zs[VB][JT];
  const int tid = threadIdx.x;
  const Adam a = *(const Adam*)(work + W_ADAM);
  // parameter order of the moments: W0 | b0 | W1 | b1 | w2 | b2
  const long long o_b0 = (long long)VH * kf, o_W1 = o_b0 + VH, o_b1 = o_W1 + VH * VH, o_w2 = o_b1 + VH,
                  o_b2 = o_w2 + VH;
  if (blockIdx.x < NW0) {
    // W0 rows j0 .. j0+7: gW0[j][k] = sum_r dz0[r][j] x[r][k], thread = column k
    const int j0 = blockIdx.x * JT;
    const float* dz0t = work + W_DZ0;
    const float* xb = work + W_XB;
#pragma unroll
    for (int i = 0; i < JT / 4; ++i) zs[tid & 63][(tid >> 6) + 4 * i] = dz0t[(j0 + (tid >> 6) + 4 * i) * VB + (tid & 63)];
    __syncthreads();
    for (int k = tid; k < kf; k += 256) {
      float w[JT], m[JT], v[JT], acc[JT];
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const long long o = (long long)(j0 + j) * kf + k;
        w[j] = W0[o];
        m[j] = am[o];
        v[j] = av[o];
        acc[j] = 0.f;
      }
#pragma unroll 8
      for (int r = 0; r < VB; ++r) {
        const float x = xb[r * kf + k];
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[j] = fmaf(zs[r][j], x, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const long long o = (long long)(j0 + j) * kf + k;
        adam_math(w[j], m[j], v[j], acc[j], a);
        W0[o] = w[j];
        am[o] = m[j];
        av[o] = v[j];
      }
    }
    return;
  }
  // W1 rows j0 .. j0+15 from gW1, and the b0, b1, w2 entries j0 .. j0+15 (one wave per entry,
  // lane = batch row); b2 with the first of these workgroups
  const int j0 = (blockIdx.x - NW0) * VT;
  const float* gW1 = work + W_GW1;
  const int lane = tid & 63, wv = tid >> 6;
  const float dy = work[W_DY + lane];
  float gb[3 * VT / 4];
#pragma unroll
  for (int i = 0; i < 3 * VT / 4; ++i) {
    const int q = wv + 4 * i, which = q / VT, j = j0 + q % VT;
    gb[i] = which == 0 ? work[W_DZ0 + j * VB + lane] : (which == 1 ? work[W_DZ1 + j * VB + lane]
                                                                   : dy * work[W_H1 + j * VB + lane]);
  }
#pragma unroll
  for (int i = 0; i < VT * VH / 256; ++i) {
    const int o = j0 * VH + tid + i * 256;
    adam_update(W1 + o, am + o_W1 + o, av + o_W1 + o, gW1[o], a);
  }
  // lane i of the wave updates the wave's entry i (every lane holds every sum): one memory round
  // trip for the 12 entries, not one each; lane 12 of the first wave of workgroup NW0 takes b2
  float g = amx::wave_sum(dy);
#pragma unroll
  for (int i = 0; i < 3 * VT / 4; ++i) {
    const float s = amx::wave_sum(gb[i]);
    if (lane == i) g = s;
  }
  float* pw = nullptr;
  long long om = 0;
  if (lane < 3 * VT / 4) {
    const int q = wv + 4 * lane, which = q / VT, j = j0 + q % VT;
    pw = which == 0 ? b0 + j : (which == 1 ? b1 + j : w2 + j);
    om = (which == 0 ? o_b0 : (which == 1 ? o_b1 : o_w2)) + j;
  } else if (lane == 3 * VT / 4 && wv == 0 && blockIdx.x == NW0) {
    pw = b2;
    om = o_b2;
  }
  if (pw) adam_update(pw, am + om, av + om, g, a);
}

int check_shape(const char* fn, int kf, int H0p, int H1p) {
  AMX_CHECK_ARG(kf > 0 && kf % AMX_K_TILE == 0, "%s: kf=%d is not a positive multiple of %d", fn, kf, AMX_K_TILE);
  AMX_CHECK_ARG(H0p == VH && H1p == VH, "%s: padded hidden widths %d, %d (supported: %d, %d)", fn, H0p, H1p, VH, VH);
  return AMX_OK;
}

}  // namespace

extern "C" long long amx_vfit_work(int kf, int H0p, int H1p) {
  if (check_shape("amx_vfit_work", kf, H0p, H1p)) return -1;
  return ((long long)W_XB + (long long)VB * kf) * (long long)sizeof(float);
}

extern "C" long long amx_vfit_param_count(int kf, int H0p, int H1p) {
  if (check_shape("amx_vfit_param_count", kf, H0p, H1p)) return -1;
  return (long long)H0p * kf + H0p + (long long)H1p * H0p + 2LL * H1p + 1;
}

extern "C" int amx_vfit_epoch(amx_ctx* ctx, int n_rows, const float* feat, int ldf, const float* returns,
                              const int32_t* perm, int kf, int H0p, int H1p, float* W0, float* b0, float* W1,
                              float* b1, float* w2, float* b2, float* adam_m, float* adam_v, long long* adam_step,
                              double lr, double beta1, double beta2, double eps, double weight_decay, void* work,
                              float* epoch_loss, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_vfit_epoch: null ctx");
  AMX_CHECK_ARG(n_rows >= 2 * VB, "amx_vfit_epoch: n_rows=%d (need >= %d: int(n / %d) - 1 steps)", n_rows, 2 * VB, VB);
  int rc = check_shape("amx_vfit_epoch", kf, H0p, H1p);
  if (rc) return rc;
  AMX_CHECK_ARG(feat && returns && perm, "amx_vfit_epoch: null feat / returns / perm");
  AMX_CHECK_ARG(W0 && b0 && W1 && b1 && w2 && b2, "amx_vfit_epoch: null weight pointer");
  AMX_CHECK_ARG(adam_m && adam_v && adam_step && work && epoch_loss, "amx_vfit_epoch: null state / work pointer");
  AMX_CHECK_ARG(ldf >= kf, "amx_vfit_epoch: ldf=%d < kf=%d", ldf, kf);
  AMX_CHECK_ARG(kf >= ctx->S + 4, "amx_vfit_epoch: kf=%d < S + 4 = %d", kf, ctx->S + 4);
  AMX_CHECK_ARG(amx::aligned16(work) && ((uintptr_t)adam_step & 7u) == 0, "amx_vfit_epoch: misaligned work / adam_step");
  AMX_CHECK_ARG(lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 &&
                    weight_decay >= 0.0,
                "amx_vfit_epoch: lr=%g betas=(%g, %g) eps=%g weight_decay=%g", lr, beta1, beta2, eps, weight_decay);
  const int num_steps = n_rows / VB - 1;
  hipStream_t st = (hipStream_t)stream;
  float* wk = (float*)work;
  hipLaunchKernelGGL(k_vfit_begin, dim3(1), dim3(64), 0, st, wk);
  AMX_CHECK_LAUNCH();
  for (int mb = 0; mb < num_steps; ++mb) {
    hipLaunchKernelGGL(k_vfit_l0, dim3(VNB), dim3(256), 0, st, mb, n_rows, feat, ldf, perm, kf, W0, b0, wk);
    hipLaunchKernelGGL(k_vfit_l1, dim3(VNB), dim3(256), 0, st, mb, n_rows, returns, perm, W1, b1, w2, wk);
    hipLaunchKernelGGL(k_vfit_bwd, dim3(2 * VNB + 1), dim3(256), 0, st, W1, w2, b2, wk, adam_step, num_steps, lr,
                       beta1, beta2, eps, weight_decay, epoch_loss);
    hipLaunchKernelGGL(k_vfit_adam, dim3(3 * VNB), dim3(256), 0, st, kf, W0, b0, W1, b1, w2, b2, adam_m, adam_v, wk);
    AMX_CHECK_LAUNCH();
  }
  return AMX_OK;
}
