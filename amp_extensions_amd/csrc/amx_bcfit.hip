// The behaviour-cloning warm start on the device: BC.fit's training loop
// (mjrl/mjrl/algos/behavior_cloning.py:106-139) for the policy's S -> 32 -> 32 -> A tanh MLP
// (mjrl/mjrl/policies/gaussian_mlp.py:7-62), with the MSE loss (behavior_cloning.py:94-104) or
// the negative mean log-likelihood (behavior_cloning.py:82-92, gaussian_mlp.py:106-122) and
// torch.optim.Adam.
//
// k_bcfit_steps runs n_steps dependent Adam steps in ONE launch of ONE workgroup of 16 waves.
// The whole policy (8 616 floats at S/A = 197/36) stays in LDS for the launch, in padded
// row-major images (W1 [32][XS], W2 [32][36], W3 [A16][36], b1, b2, b3, log_std); every
// parameter has one owner thread, which computes that parameter's gradient, keeps its two Adam
// moments in registers for the whole launch and applies the update in LDS.  Nothing goes to
// global memory between steps but the step's loss; theta, the moments and the step count are
// written back once, at the end.  __syncthreads-style workgroup barriers are the only
// synchronisation (there is no other workgroup).
//
// Every product is a 16x16 tile on the f32 matrix pipe (v_mfma_f32_16x16x4_f32, an exact fp32
// fma chain in a fixed order, so a fit is bit-reproducible):
//   P1  layer 1, K = S split in two halves: 8 tiles x 2 halves on the 16 waves -> partials
//   P1b H1 = tanh(part0 + part1 + b1)                                  (all threads)
//   P2  H2 = tanh(H1 W2^T + b2)           waves 0-7; wave 8 forms the step's Adam constants
//       (1 - beta^t in double), wave 9 the column scales of d mu
//   P3  mu = H2 W3^T + b3; Z = mu - a (MSE) or (a - mu) / sigma (MLE), over the actions in LDS
//   P4  D2 = ((Z sc) W3) (1 - H2^2)       waves 0-7;  gW3 = (Z^T H2) sc   waves 8-15 (kept in
//       registers); b3, the log_std gradient (MLE) and the loss on waves 13-15
//   P5  d1 = (D2 W2) (1 - H1^2)           waves 0-7 (registers);  Adam on W3, gW2 = D2^T H1 on
//       waves 8-11, b2 on wave 12, log_std on wave 14
//   P5b D1 = d1 over H1's buffer; Adam on W2
//   P6  gW1 = D1^T X: 2 ceil(S / 16) tiles, two per wave, each straight into Adam on W1; b1
//   P7  the next batch (gathered into registers since the top of the step) -> LDS
// d mu = Z sc with sc = 2 / (64 A) (MSE) or -1 / (64 sigma_c) (MLE).  The owner of a weight is
// the lane that holds it in the MFMA accumulator of its gradient tile: lane (i = lane & 15,
// kq = lane >> 4) of the tile's wave owns rows 4 kq .. 4 kq + 3, column i of the tile.
//
// The batch indices of all steps are known up front: the rows of step k + 1 are gathered into
// registers at the top of step k (16 + 4 floats per thread) and stored to LDS at its end, and
// the indices of step k + 2 are staged the same way, so no step waits on a dependent load.
// The barriers between phases wait on LDS only (amx_common.h's lds_barrier), never on those
// loads.  Adam's constants and update are amx_optim.h's (AdamConst, adam_apply); the decay is
// added here.
//
// k_bcfit_eval is the same forward over all N rows (BC.fit's loss_before / loss_after), 64 rows
// at a time on as many workgroups as fill the chip: fp32 per row as the reference, fp64 per
// workgroup, and k_bcfit_eval_sum adds the workgroups' partials in workgroup order.
//
// k_ppo_steps is the same step body (steps_body<true>) with PPO's clipped surrogate
// (mjrl/mjrl/algos/ppo_clip.py:48-55, 88-97) in place of BC's loss: the MLE forward and
// backward with a weight g_r on every row.  Its additions:
//   gather  adv[row] and (snapshot mode) ll_old[row] travel with the batch (wave 15, lane = row)
//   P2      waves 10 / 11 form sum log_std / sum log_std_old
//   P3      each lane also squares its z, a butterfly adds the 16 columns of a tile, and the
//           tile's partial goes to PN [CT][64]; in tracks-mean mode the same for
//           z_old = (a - mu) / sigma_old into PO (mu is the step's own: the old mean network
//           shares the new one's storage)
//   P3b     wave 0, lane = row: LL_new and LL_old from the partials in tile order (row_ll; the
//           snapshot's LL_old was formed by the same code in k_ppo_old_ll, so equal policies
//           give LR = exp(0)), LR, g = adv LR pass -> G, the row's surrogate term -> SURR, the
//           count of rows outside [lo, hi] by ballot -> step_clipped
//   P4      D2, gW3, b3 and the log_std gradient take g_r as a factor of row r's Z; wave 15
//           sums SURR into the step's loss
// P5 - P7 and Adam are BC's.  BC's instantiation (steps_body<false>) compiles none of this in
// and its LDS image ends ahead of PPO's fields.  k_ppo_old_ll is eval_body<true>: LL of every
// row at theta.
#include <math.h>

#include "amx_optim.h"

namespace {

using amx::lds_barrier;

constexpr int NH = 32;      // hidden width (both layers)
constexpr int BB = 64;      // mini-batch rows (BC's batch_size)
constexpr int NT = 1024;    // threads: 16 waves, 4 per SIMD
constexpr int NW = NT / 64;
constexpr int MAXS = 256, MAXA = 64;  // DeviceNPG's limits
constexpr int HS = 36;      // row stride of the 32-wide images (= 4 mod 32: float4 reads of 8 rows hit 32 banks)
constexpr int XU = 16, AU = 4;        // gathered floats per thread: 64 x 256 / 1024, 64 x 64 / 1024
constexpr int EVAL_MAXB = 1024;       // most workgroups of k_bcfit_eval
constexpr int LOSS_MSE = 0, LOSS_MLE = 1;

typedef float pf4 __attribute__((ext_vector_type(4)));

// LDS image in floats.  The parameters come first ([0, X)); pads are zero for the whole launch.
struct Lay {
  int S, A, KP, XS, A16, AS, CT, KT;
  int W1, W2, W3, b1, b2, b3, ls, X, ACT, H1, H2, D2, PART, SC, ADAM, IDX, total;
  int ADV, LLO, G, SURR, LSO, PN, PO, SL;  // PPO only
  __host__ __device__ Lay(int S_, int A_, bool ppo = false) : S(S_), A(A_) {
    KP = (S + 15) / 16 * 16;
    XS = KP + 4 + (KP % 32 ? 16 : 0);  // = 4 mod 32
    A16 = (A + 15) / 16 * 16;
    AS = A16 + 4;
    CT = A16 / 16;
    KT = KP / 16;
    int o = 0;
    W1 = o; o += NH * XS;
    W2 = o; o += NH * HS;
    W3 = o; o += A16 * HS;
    b1 = o; o += NH;
    b2 = o; o += NH;
    b3 = o; o += MAXA;
    ls = o; o += MAXA;
    X = o; o += BB * XS;        // the batch's observations | zeros
    ACT = o; o += BB * AS;      // the batch's actions, then Z in place
    H1 = o; o += BB * HS;       // tanh activations; D1 from P5b on
    H2 = o; o += BB * HS;
    D2 = o; o += BB * HS;
    PART = H2;                  // layer 1's two K-half partials [2][64][HS]: H2 and D2 are idle then
    SC = o; o += MAXA;          // column scales of d mu
    ADAM = o; o += 8;
    IDX = o; o += 2 * BB;       // row indices of the next two steps (int)
    ADV = LLO = G = SURR = LSO = PN = PO = SL = o;
    if (ppo) {                  // BC's image ends above
      ADV = o; o += BB;         // the batch's whitened advantages
      LLO = o; o += BB;         // the batch's LL_old (snapshot mode)
      G = o; o += BB;           // row weights g = adv LR pass
      SURR = o; o += BB;        // rows' min(LR adv, clamp(LR) adv)
      LSO = o; o += MAXA;       // log_std_old (tracks-mean mode) | zeros
      PN = o; o += MAXA / 16 * BB;  // sum_c z^2 per column tile [CT][64]
      PO = o; o += MAXA / 16 * BB;  // the same of z_old (tracks-mean mode)
      SL = o; o += 8;           // sum log_std, sum log_std_old
    }
    total = o;
  }
  __host__ __device__ size_t bytes() const { return (size_t)total * sizeof(float); }
};

// offsets of the reference's flat parameter order: W1 | b1 | W2 | b2 | W3 | b3 | log_std
struct Flat {
  int b1, W2, b2, W3, b3, ls, P;
  __host__ __device__ Flat(int S, int A) {
    b1 = NH * S;
    W2 = b1 + NH;
    b2 = W2 + NH * NH;
    W3 = b2 + NH;
    b3 = W3 + A * NH;
    ls = b3 + A;
    P = ls + A;
  }
};

struct Adam {
  amx::AdamConst c;
  float wd;
};

// torch.optim.Adam with weight decay on a parameter in LDS, its moments in registers:
// grad.add(p, alpha=wd), then amx_optim.h's update
__device__ inline void adam_lds(float* w, float& m, float& v, float g, const Adam& a) {
  float p = *w;
  g = g + a.wd * p;
  amx::adam_apply(p, m, v, g, a.c);
  *w = p;
}

__device__ __forceinline__ pf4 mma(float a, float b, pf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// row r of MFMA step s (0..15) for lane group kq of a K = 64-rows product: the two groups of a
// 32-lane half read rows 4 apart (16 banks apart at a row stride = 4 mod 32)
__device__ __forceinline__ int krow(int s, int kq) { return 16 * (s >> 2) + 4 * kq + (s & 3); }

// C tile += A[16 rows i][K] B[16 rows i][K]^T, both row-major in LDS with K contiguous
// (float4 per lane and 16 k: lane group kq takes k = 16 jj + 4 kq .. + 3)
__device__ __forceinline__ pf4 tile_nt(const float* __restrict__ a, const float* __restrict__ b, int jj0, int jj1,
                                       pf4 acc) {
  for (int jj = jj0; jj < jj1; ++jj) {
    const pf4 x = *reinterpret_cast<const pf4*>(a + 16 * jj);
    const pf4 w = *reinterpret_cast<const pf4*>(b + 16 * jj);
    acc = mma(x.x, w.x, acc);
    acc = mma(x.y, w.y, acc);
    acc = mma(x.z, w.z, acc);
    acc = mma(x.w, w.w, acc);
  }
  return acc;
}

// C tile = sum over the 64 rows r of A[r][ca] B[r][cb] (A: stride lda, B: stride ldb; ca / cb
// already include the lane's column)
__device__ __forceinline__ pf4 tile_tn(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb,
                                       int kq) {
  pf4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = 0; s < 16; ++s) {
    const int r = krow(s, kq);
    acc = mma(a[r * lda], b[r * ldb], acc);
  }
  return acc;
}

// the same with row weights: sum over r of (A[r][ca] g[r]) B[r][cb]
__device__ __forceinline__ pf4 tile_tn_w(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb,
                                         const float* __restrict__ g, int kq) {
  pf4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = 0; s < 16; ++s) {
    const int r = krow(s, kq);
    acc = mma(a[r * lda] * g[r], b[r * ldb], acc);
  }
  return acc;
}

// The thread's indices, re-derived at every phase of a step from a thread id the compiler cannot
// see through: otherwise it hoists every per-thread LDS address of the step out of the step
// loop, which costs some 80 registers (spilled to scratch at 128 per thread) for a few integer
// operations saved.
struct Tid {
  int t, lane, wave, i, kq;
  __device__ __forceinline__ Tid() {
    t = threadIdx.x;
    asm volatile("" : "+v"(t));
    lane = t & 63;
    wave = t >> 6;
    i = lane & 15;
    kq = lane >> 4;
  }
};

// a phase's own copies of the kernel's thread indices (shadowing them)
#define BCFIT_PHASE_TID()                                                                        \
  const Tid q_;                                                                                  \
  const int t = q_.t, lane = q_.lane, wave = q_.wave, i = q_.i, kq = q_.kq, ct3 = (wave - 8) >> 1, \
            jt3 = wave & 1;                                                                      \
  (void)t; (void)lane; (void)i; (void)kq; (void)ct3; (void)jt3

// sum over n (a multiple of 8) elements p[e * ld] of f(element), in element order.  The reads
// go out 8 at a time: written as a plain loop, every read waits for the add before it (some
// 100 clocks each, three such sums per step on the critical path).
template <typename F>
__device__ __forceinline__ float strided_sum(const float* __restrict__ p, int ld, int n, F f) {
  float s = 0.f;
#pragma unroll 1
  for (int e0 = 0; e0 < n; e0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(e0 + u) * ld];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += f(v[u]);
  }
  return s;
}

// the same over two arrays: sum of f(p[e * ld], q[e])
template <typename F>
__device__ __forceinline__ float strided_sum2(const float* __restrict__ p, int ld, const float* __restrict__ q, int n,
                                              F f) {
  float s = 0.f;
#pragma unroll 1
  for (int e0 = 0; e0 < n; e0 += 8) {
    float v[8], w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[u] = p[(e0 + u) * ld];
      w[u] = q[e0 + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += f(v[u], w[u]);
  }
  return s;
}

// sum over the 16 lanes that share lane >> 4, as a butterfly: every lane of the group gets the
// same bits (a + b == b + a), in an order that depends on nothing but the lane numbers
__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// PPO's per-row log-likelihood, the one form of the step kernel and of k_ppo_old_ll (so a
// ratio of equal policies is exp(0)): sum_c z^2 from P3's column-tile partials in tile order,
// LL = (-0.5 sum z^2 - sum log_std) - 0.5 A log(2 pi) as gaussian_mlp.py:119-121 groups it
__device__ __forceinline__ float sum_log_std(const float* __restrict__ ls, const Lay& L) {
  return strided_sum(ls, 1, L.A16, [](float x) { return x; });  // zero past A
}
__device__ __forceinline__ float row_ll(const float* __restrict__ part, float sl, const Lay& L, int r) {
  float s = 0.f;
  for (int ct = 0; ct < L.CT; ++ct) s += part[ct * BB + r];
  return (-0.5f * s - sl) - (float)(0.5 * (double)L.A * 1.8378770664093453);  // log(2 pi)
}

struct StepConsts {
  long long t;  // Adam's step count of this step (1-based)
  double lr, beta1, beta2, eps, wd;
};

// The forward of the 64 rows in X / ACT (P1 - P3): leaves H1, H2 and Z (over ACT).  STEP: the
// idle waves of P2 form the step's Adam constants and the d mu column scales.
// PPO (loss_type MLE): P3 also leaves each row's sum_c z^2 as one partial per column tile in PN
// (and, with `tracks`, that of z_old = (a - mu) / sigma_old in PO), and the step's idle waves
// of P2 form sum log_std (and sum log_std_old).
// MEAN (PPO): P3 also writes the policy mean of rows < mean_rows to mean[row][A] (amx_npg_ll).
template <bool STEP, bool PPO = false, bool MEAN = false>
__device__ __forceinline__ void forward(float* __restrict__ sm, const Lay& L, int loss_type, const StepConsts* sc,
                                        bool tracks = false, float* __restrict__ mean = nullptr, int mean_rows = 0) {
  {  // P1
    const Tid q;
    const int wave = q.wave, i = q.i, kq = q.kq;
    const int tile = wave & 7, kh = wave >> 3, rt = tile >> 1, jt = tile & 1;
    const int jj0 = kh ? L.KT / 2 : 0, jj1 = kh ? L.KT : L.KT / 2;
    pf4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = tile_nt(sm + L.X + (rt * 16 + i) * L.XS + 4 * kq, sm + L.W1 + (jt * 16 + i) * L.XS + 4 * kq, jj0, jj1, acc);
    float* pp = sm + L.PART + kh * BB * HS + (rt * 16 + 4 * kq) * HS + jt * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) pp[r * HS] = acc[r];
  }
  lds_barrier();
  const Tid q1;
#pragma unroll
  for (int e = q1.t; e < BB * NH; e += NT) {  // P1b
    const int r = e >> 5, j = e & 31;
    const float z = (sm[L.PART + r * HS + j] + sm[L.PART + BB * HS + r * HS + j]) + sm[L.b1 + j];
    sm[L.H1 + r * HS + j] = tanhf(z);
  }
  lds_barrier();
  const Tid q2;
  const int lane = q2.lane, wave = q2.wave, i = q2.i, kq = q2.kq;
  if (wave < 8) {  // P2
    const int rt = wave >> 1, jt = wave & 1;
    pf4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = tile_nt(sm + L.H1 + (rt * 16 + i) * HS + 4 * kq, sm + L.W2 + (jt * 16 + i) * HS + 4 * kq, 0, 2, acc);
    const float b = sm[L.b2 + jt * 16 + i];
    float* ph = sm + L.H2 + (rt * 16 + 4 * kq) * HS + jt * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) ph[r * HS] = tanhf(acc[r] + b);
  } else if (STEP && wave == 8) {
    // the two powers side by side on lanes 0 and 1
    const double bc = 1.0 - pow(lane == 1 ? sc->beta2 : sc->beta1, (double)sc->t), bc2 = __shfl(bc, 1);
    if (lane == 0)
      *reinterpret_cast<Adam*>(sm + L.ADAM) = Adam{amx::AdamConst(bc, bc2, sc->lr, sc->beta1, sc->beta2, sc->eps), (float)sc->wd};
  } else if (STEP && wave == 9) {
    float s = 0.f;
    if (lane < L.A) s = loss_type == LOSS_MLE ? -1.f / ((float)BB * expf(sm[L.ls + lane])) : 2.f / (float)(BB * L.A);
    sm[L.SC + lane] = s;
  } else if (PPO && STEP && (wave == 10 || (wave == 11 && tracks))) {
    const float sl = sum_log_std(sm + (wave == 10 ? L.ls : L.LSO), L);
    if (lane == 0) sm[L.SL + wave - 10] = sl;
  }
  lds_barrier();
  const Tid q3;
  for (int item = q3.wave; item < 4 * L.CT; item += NW) {  // P3
    const int i = q3.i, kq = q3.kq;
    const int rt = item / L.CT, ct = item - rt * L.CT, c = ct * 16 + i;
    pf4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = tile_nt(sm + L.H2 + (rt * 16 + i) * HS + 4 * kq, sm + L.W3 + c * HS + 4 * kq, 0, 2, acc);
    const float b = sm[L.b3 + c];
    const float sig = loss_type == LOSS_MLE ? expf(sm[L.ls + c]) : 1.f;
    float* pz = sm + L.ACT + (rt * 16 + 4 * kq) * L.AS + c;
    if constexpr (PPO) {
      const float sigo = tracks ? expf(sm[L.LSO + c]) : 1.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = pz[r * L.AS] - (acc[r] + b);
        if constexpr (MEAN) {
          const int row = rt * 16 + 4 * kq + r;
          if (mean && row < mean_rows && c < L.A) mean[(long long)row * L.A + c] = acc[r] + b;
        }
        const float z = c < L.A ? d / sig : 0.f;
        pz[r * L.AS] = z;
        const float s = group16_sum(z * z);
        if (i == 0) sm[L.PN + ct * BB + rt * 16 + 4 * kq + r] = s;
        if (tracks) {
          const float zo = c < L.A ? d / sigo : 0.f;
          const float so = group16_sum(zo * zo);
          if (i == 0) sm[L.PO + ct * BB + rt * 16 + 4 * kq + r] = so;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mu = acc[r] + b, a = pz[r * L.AS];
        pz[r * L.AS] = c < L.A ? (loss_type == LOSS_MLE ? (a - mu) / sig : mu - a) : 0.f;
      }
    }
  }
  lds_barrier();
}

// row r's term of the loss from Z, fp32 as the reference: sum_c (mu - a)^2 (MSE) or LL_r (MLE)
__device__ inline float row_term(const float* __restrict__ sm, const Lay& L, int loss_type, int r) {
  // over the padded width: Z and log_std are zero past A
  const float s = strided_sum(sm + L.ACT + r * L.AS, 1, L.A16, [](float z) { return z * z; });
  if (loss_type == LOSS_MSE) return s;
  const float sl = strided_sum(sm + L.ls, 1, L.A16, [](float x) { return x; });
  return (-0.5f * s - sl) - (float)(0.5 * (double)L.A * 1.8378770664093453);  // log(2 pi)
}

// theta (flat) -> the LDS images; everything else in LDS zero
__device__ inline void stage_theta(float* __restrict__ sm, const Lay& L, const Flat& F, const float* __restrict__ theta) {
  const int t = threadIdx.x;
  for (int e = t; e < L.total; e += NT) sm[e] = 0.f;
  __syncthreads();
  for (int e = t; e < NH * L.S; e += NT) {
    const int j = e / L.S, k = e - j * L.S;
    sm[L.W1 + j * L.XS + k] = theta[e];
  }
  for (int e = t; e < NH * NH; e += NT) sm[L.W2 + (e >> 5) * HS + (e & 31)] = theta[F.W2 + e];
  for (int e = t; e < L.A * NH; e += NT) sm[L.W3 + (e >> 5) * HS + (e & 31)] = theta[F.W3 + e];
  if (t < NH) {
    sm[L.b1 + t] = theta[F.b1 + t];
    sm[L.b2 + t] = theta[F.b2 + t];
  }
  if (t < L.A) {
    sm[L.b3 + t] = theta[F.b3 + t];
    sm[L.ls + t] = theta[F.ls + t];
  }
}

struct StepArgs {
  int S, A, N, n_steps, loss_type;
  const float* obs;
  long long ldo;
  const float* act;
  long long lda;
  const int32_t* idx;
  float* theta;
  float* am;
  float* av;
  long long* adam_step;
  double lr, beta1, beta2, eps, wd;
  float* step_loss;
};

// PPO's additions to a step (ppo_clip.py:48-55): adv [N] (whitened, fp32) and ll_old [N] are
// gathered with the rows; ll_old == nullptr is the tracks-mean mode (log_std_old [A] given)
struct PpoArgs {
  const float* adv;
  const float* ll_old;
  const float* log_std_old;
  float lo, hi;  // float32(1 - clip_coef), float32(1 + clip_coef): torch.clamp's bounds
  int32_t* step_clipped;
};

// The step loop of k_bcfit_steps (PPO = false: `p` unused) and of k_ppo_steps.
template <bool PPO>
__device__ __forceinline__ void steps_body(const StepArgs& a, const PpoArgs& p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Lay L(a.S, a.A, PPO);
  const bool tracks = PPO && p.ll_old == nullptr;
  const Flat F(a.S, a.A);
  const int S = a.S, A = a.A;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 15, kq = lane >> 4;
  const bool mle = a.loss_type == LOSS_MLE;
  int* sidx = reinterpret_cast<int*>(sm + L.IDX);

  stage_theta(sm, L, F, a.theta);
  if (PPO && tracks && t < A) sm[L.LSO + t] = p.log_std_old[t];

  // ---- ownership: flat offset of each owned parameter (-1: none) and its moments ---------------
  // W1: tiles T = wave + 16 u (jt = T & 1, kt = T >> 1); W3: waves 8-15 (ct = (wave - 8) >> 1,
  // jt = wave & 1); W2: waves 8-11 (j2t = (wave - 8) >> 1, j1t = wave & 1); b2 / b3 / log_std /
  // b1: lanes of waves 12 / 13 / 14 / 15
  float m1[2][4], v1[2][4], m3[4], v3[4], m2[4], v2[4], ms = 0.f, vs = 0.f;
  int os = -1;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int T = wave + NW * u, jt = T & 1, k = (T >> 1) * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool own = T < 2 * L.KT && k < S;
      const int o = (jt * 16 + 4 * kq + r) * S + k;
      m1[u][r] = own ? a.am[o] : 0.f;
      v1[u][r] = own ? a.av[o] : 0.f;
    }
  }
  const int ct3 = (wave - 8) >> 1, jt3 = wave & 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = ct3 * 16 + 4 * kq + r;
    const bool own3 = wave >= 8 && ct3 < L.CT && c < A;
    const int o3 = F.W3 + c * NH + jt3 * 16 + i;
    m3[r] = own3 ? a.am[o3] : 0.f;
    v3[r] = own3 ? a.av[o3] : 0.f;
    const bool own2 = wave >= 8 && wave < 12;
    const int o2 = F.W2 + (ct3 * 16 + 4 * kq + r) * NH + jt3 * 16 + i;
    m2[r] = own2 ? a.am[o2] : 0.f;
    v2[r] = own2 ? a.av[o2] : 0.f;
  }
  if (wave == 12 && lane < NH) os = F.b2 + lane;
  if (wave == 13 && lane < A) os = F.b3 + lane;
  if (wave == 14 && lane < A && mle) os = F.ls + lane;
  if (wave == 15 && lane < NH) os = F.b1 + lane;
  if (os >= 0) {
    ms = a.am[os];
    vs = a.av[os];
  }
  const long long t0 = a.adam_step[0];

  // ---- the first batch, and the indices of the first two ----------------------------------------
  auto clampi = [&](int v) { return amx::clamp_row(v, a.N); };
  if (t < BB) {
    sidx[t] = clampi(a.idx[t]);
    if (a.n_steps > 1) sidx[BB + t] = clampi(a.idx[BB + t]);
  }
  __syncthreads();
  float xr[XU], ar[AU], advr = 0.f, llor = 0.f;
  // gather map: wave w takes rows 4 w .. 4 w + 3; lane = column within a 64-column group
  auto gather = [&](const int* rows, int lane, int wave) {
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int c = lane + 64 * (u & 3);
      xr[u] = c < S ? a.obs[(long long)rows[wave * 4 + (u >> 2)] * a.ldo + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) ar[u] = lane < A ? a.act[(long long)rows[wave * 4 + u] * a.lda + lane] : 0.f;
    if (PPO && wave == 15) {  // lane = row
      advr = p.adv[rows[lane]];
      if (!tracks) llor = p.ll_old[rows[lane]];
    }
  };
  auto scatter = [&](int lane, int wave) {
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int c = lane + 64 * (u & 3);
      if (c < S) sm[L.X + (wave * 4 + (u >> 2)) * L.XS + c] = xr[u];
    }
#pragma unroll
    for (int u = 0; u < AU; ++u)
      if (lane < A) sm[L.ACT + (wave * 4 + u) * L.AS + lane] = ar[u];
    if (PPO && wave == 15) {
      sm[L.ADV + lane] = advr;
      sm[L.LLO + lane] = llor;
    }
  };
  gather(sidx, lane, wave);
  scatter(lane, wave);
  __syncthreads();

  for (int k = 0; k < a.n_steps; ++k) {
    // the next step's rows and the step after's indices: in flight until P7
    int inext = 0;
    {
      BCFIT_PHASE_TID();
      if (k + 1 < a.n_steps) gather(sidx + ((k + 1) & 1) * BB, lane, wave);
      if (k + 2 < a.n_steps && t < BB) inext = a.idx[(long long)(k + 2) * BB + t];
    }

    StepConsts sc = {t0 + k + 1, a.lr, a.beta1, a.beta2, a.eps, a.wd};
    forward<true, PPO>(sm, L, a.loss_type, &sc, tracks);
    const Adam ad = *reinterpret_cast<const Adam*>(sm + L.ADAM);

    // ---- P3b (PPO): the rows' ratio, surrogate term and weight g = adv LR pass -------------------
    // pass = 1 inside [lo, hi] (min's two arguments are equal there: its backward halves add up
    // to the whole, clamp's is inclusive at the bounds); outside only where min takes LR adv
    if constexpr (PPO) {
      BCFIT_PHASE_TID();
      if (wave == 0) {
        const float lln = row_ll(sm + L.PN, sm[L.SL], L, lane);
        const float llo = tracks ? row_ll(sm + L.PO, sm[L.SL + 1], L, lane) : sm[L.LLO + lane];
        const float lr = expf(lln - llo), adv = sm[L.ADV + lane];
        const bool inside = lr >= p.lo && lr <= p.hi;
        const bool pass = inside || (lr > p.hi && adv < 0.f) || (lr < p.lo && adv > 0.f);
        sm[L.G + lane] = pass ? adv * lr : 0.f;
        sm[L.SURR + lane] = fminf(lr * adv, fminf(fmaxf(lr, p.lo), p.hi) * adv);
        const unsigned long long out = __ballot(!inside);
        if (lane == 0) p.step_clipped[k] = __popcll(out);
      }
      lds_barrier();
    }

    // ---- P4 -------------------------------------------------------------------------------------
    pf4 g3 = {0.f, 0.f, 0.f, 0.f};
    float gls = 0.f;
    {
    BCFIT_PHASE_TID();
    if (wave < 8) {
      // D2 = ((Z sc) W3) (1 - H2^2): rows rt, hidden units jt
      const int rt = wave >> 1, jt = wave & 1;
      pf4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* pz = sm + L.ACT + (rt * 16 + i) * L.AS + 4 * kq;
      const float* ps = sm + L.SC + 4 * kq;
      const float* pw = sm + L.W3 + (4 * kq) * HS + jt * 16 + i;
      for (int jj = 0; jj < L.CT; ++jj) {
        pf4 z = *reinterpret_cast<const pf4*>(pz + 16 * jj) * *reinterpret_cast<const pf4*>(ps + 16 * jj);
        if constexpr (PPO) z *= sm[L.G + rt * 16 + i];
        const float* w = pw + 16 * jj * HS;
        acc = mma(z.x, w[0], acc);
        acc = mma(z.y, w[HS], acc);
        acc = mma(z.z, w[2 * HS], acc);
        acc = mma(z.w, w[3 * HS], acc);
      }
      const float* ph = sm + L.H2 + (rt * 16 + 4 * kq) * HS + jt * 16 + i;
      float* pd = sm + L.D2 + (rt * 16 + 4 * kq) * HS + jt * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float h = ph[r * HS];
        pd[r * HS] = acc[r] * (1.f - h * h);
      }
    } else {
      if (ct3 < L.CT) {  // gW3[c][j] = sc[c] sum_r Z[r][c] H2[r][j]
        g3 = PPO ? tile_tn_w(sm + L.ACT + ct3 * 16 + i, L.AS, sm + L.H2 + jt3 * 16 + i, HS, sm + L.G, kq)
                 : tile_tn(sm + L.ACT + ct3 * 16 + i, L.AS, sm + L.H2 + jt3 * 16 + i, HS, kq);
#pragma unroll
        for (int r = 0; r < 4; ++r) g3[r] *= sm[L.SC + ct3 * 16 + 4 * kq + r];
      }
      if (wave == 13 && lane < A) {  // b3
        const float s = PPO ? strided_sum2(sm + L.ACT + lane, L.AS, sm + L.G, BB, [](float z, float g) { return z * g; })
                            : strided_sum(sm + L.ACT + lane, L.AS, BB, [](float x) { return x; });
        adam_lds(sm + L.b3 + lane, ms, vs, s * sm[L.SC + lane], ad);
      } else if (wave == 14 && lane < A && mle) {  // d log_std_c = -(1 / 64) sum_r (z^2 - 1)
        // PPO: -(1 / 64) sum_r g_r (z^2 - 1)
        const float s = PPO ? strided_sum2(sm + L.ACT + lane, L.AS, sm + L.G, BB,
                                           [](float z, float g) { return g * (z * z - 1.f); })
                            : strided_sum(sm + L.ACT + lane, L.AS, BB, [](float z) { return z * z - 1.f; });
        gls = -s * (1.f / BB);  // applied in P5: the loss (wave 15) reads log_std in this phase
      } else if (wave == 15) {  // the step's loss
        const float tot = amx::wave_sum(PPO ? sm[L.SURR + lane] : row_term(sm, L, a.loss_type, lane));
        if (lane == 0) a.step_loss[k] = mle ? -tot * (1.f / BB) : tot / (float)(BB * A);
      }
    }
    }
    lds_barrier();

    // ---- P5 -------------------------------------------------------------------------------------
    float d1[4] = {0.f, 0.f, 0.f, 0.f};
    pf4 g2 = {0.f, 0.f, 0.f, 0.f};
    {
    BCFIT_PHASE_TID();
    if (wave < 8) {
      // d1 = (D2 W2) (1 - H1^2)
      const int rt = wave >> 1, jt = wave & 1;
      pf4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* pz = sm + L.D2 + (rt * 16 + i) * HS + 4 * kq;
      const float* pw = sm + L.W2 + (4 * kq) * HS + jt * 16 + i;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const pf4 z = *reinterpret_cast<const pf4*>(pz + 16 * jj);
        const float* w = pw + 16 * jj * HS;
        acc = mma(z.x, w[0], acc);
        acc = mma(z.y, w[HS], acc);
        acc = mma(z.z, w[2 * HS], acc);
        acc = mma(z.w, w[3 * HS], acc);
      }
      const float* ph = sm + L.H1 + (rt * 16 + 4 * kq) * HS + jt * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float h = ph[r * HS];
        d1[r] = acc[r] * (1.f - h * h);
      }
    } else {
      if (ct3 < L.CT) {  // Adam on W3 (P4 was its last reader)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct3 * 16 + 4 * kq + r;
          if (c < A) adam_lds(sm + L.W3 + c * HS + jt3 * 16 + i, m3[r], v3[r], g3[r], ad);
        }
      }
      if (wave < 12) {  // gW2[j2][j1] = sum_r D2[r][j2] H1[r][j1]
        g2 = tile_tn(sm + L.D2 + ct3 * 16 + i, HS, sm + L.H1 + jt3 * 16 + i, HS, kq);
      } else if (wave == 12 && lane < NH) {  // b2
        const float s = strided_sum(sm + L.D2 + lane, HS, BB, [](float x) { return x; });
        adam_lds(sm + L.b2 + lane, ms, vs, s, ad);
      } else if (wave == 14 && lane < A && mle) {
        adam_lds(sm + L.ls + lane, ms, vs, gls, ad);
      }
    }
    }
    lds_barrier();

    // ---- P5b: D1 over H1 (its readers are done); Adam on W2 (P5 was its last reader) -----------
    {
    BCFIT_PHASE_TID();
    if (wave < 8) {
      float* pd = sm + L.H1 + ((wave >> 1) * 16 + 4 * kq) * HS + (wave & 1) * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) pd[r * HS] = d1[r];
    } else if (wave < 12) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        adam_lds(sm + L.W2 + (ct3 * 16 + 4 * kq + r) * HS + jt3 * 16 + i, m2[r], v2[r], g2[r], ad);
    }
    }
    lds_barrier();

    // ---- P6: gW1[j][k] = sum_r D1[r][j] X[r][k], straight into Adam -----------------------------
    {
    BCFIT_PHASE_TID();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int T = wave + NW * u, jt = T & 1, kc = (T >> 1) * 16 + i;
      if (T < 2 * L.KT) {
        const pf4 g = tile_tn(sm + L.H1 + jt * 16 + i, HS, sm + L.X + kc, L.XS, kq);
        if (kc < S) {
#pragma unroll
          for (int r = 0; r < 4; ++r) adam_lds(sm + L.W1 + (jt * 16 + 4 * kq + r) * L.XS + kc, m1[u][r], v1[u][r], g[r], ad);
        }
      }
    }
    if (wave == 15 && lane < NH) {  // b1
      const float s = strided_sum(sm + L.H1 + lane, HS, BB, [](float x) { return x; });
      adam_lds(sm + L.b1 + lane, ms, vs, s, ad);
    }
    }
    lds_barrier();

    // ---- P7: the next batch -----------------------------------------------------------------------
    {
      BCFIT_PHASE_TID();
      if (k + 1 < a.n_steps) scatter(lane, wave);
      if (k + 2 < a.n_steps && t < BB) sidx[(k & 1) * BB + t] = clampi(inext);
    }
    lds_barrier();
  }

  // ---- write-back -------------------------------------------------------------------------------
  __syncthreads();
  for (int e = t; e < NH * S; e += NT) {
    const int j = e / S, k = e - j * S;
    a.theta[e] = sm[L.W1 + j * L.XS + k];
  }
  for (int e = t; e < NH * NH; e += NT) a.theta[F.W2 + e] = sm[L.W2 + (e >> 5) * HS + (e & 31)];
  for (int e = t; e < A * NH; e += NT) a.theta[F.W3 + e] = sm[L.W3 + (e >> 5) * HS + (e & 31)];
  if (t < NH) {
    a.theta[F.b1 + t] = sm[L.b1 + t];
    a.theta[F.b2 + t] = sm[L.b2 + t];
  }
  if (t < A) {
    a.theta[F.b3 + t] = sm[L.b3 + t];
    if (mle) a.theta[F.ls + t] = sm[L.ls + t];  // MSE: log_std has no gradient, no moment, no step
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int T = wave + NW * u, jt = T & 1, kc = (T >> 1) * 16 + i;
    if (T < 2 * L.KT && kc < S) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (jt * 16 + 4 * kq + r) * S + kc;
        a.am[o] = m1[u][r];
        a.av[o] = v1[u][r];
      }
    }
  }
  if (wave >= 8) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct3 * 16 + 4 * kq + r;
      if (ct3 < L.CT && c < A) {
        const int o3 = F.W3 + c * NH + jt3 * 16 + i;
        a.am[o3] = m3[r];
        a.av[o3] = v3[r];
      }
      if (wave < 12) {
        const int o2 = F.W2 + c * NH + jt3 * 16 + i;
        a.am[o2] = m2[r];
        a.av[o2] = v2[r];
      }
    }
  }
  if (os >= 0) {
    a.am[os] = ms;
    a.av[os] = vs;
  }
  if (t == 0) a.adam_step[0] = t0 + a.n_steps;
}

__global__ __launch_bounds__(NT, 1) void k_bcfit_steps(StepArgs a) { steps_body<false>(a, PpoArgs{}); }

__global__ __launch_bounds__(NT, 1) void k_ppo_steps(StepArgs a, PpoArgs p) { steps_body<true>(a, p); }

struct EvalArgs {
  int S, A, N, loss_type;
  const float* obs;
  long long ldo;
  const float* act;
  long long lda;
  const float* theta;
  double* partials;
};

// The forward over all rows, 64 at a time: BC's loss (PPO = false: the workgroup's fp64 partial)
// or every row's LL at theta into ll[N] (PPO = true: the step kernel's row_ll).
template <bool PPO>
__device__ __forceinline__ void eval_body(const EvalArgs& a, float* __restrict__ ll) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Lay L(a.S, a.A, PPO);
  const Flat F(a.S, a.A);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  stage_theta(sm, L, F, a.theta);
  __syncthreads();
  if (PPO && wave == 0) {
    const float sl = sum_log_std(sm + L.ls, L);
    if (lane == 0) sm[L.SL] = sl;
  }
  double bsum = 0.0;
  const int chunks = (a.N + BB - 1) / BB;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int r0 = ch * BB;
    // rows past N read row N - 1 and are left out of the sum
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int c = lane + 64 * (u & 3), r = wave * 4 + (u >> 2);
      const int g = r0 + r < a.N ? r0 + r : a.N - 1;
      if (c < a.S) sm[L.X + r * L.XS + c] = a.obs[(long long)g * a.ldo + c];
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int r = wave * 4 + u;
      const int g = r0 + r < a.N ? r0 + r : a.N - 1;
      if (lane < a.A) sm[L.ACT + r * L.AS + lane] = a.act[(long long)g * a.lda + lane];
    }
    __syncthreads();
    forward<false, PPO>(sm, L, a.loss_type, nullptr);
    if (wave == 0) {
      if constexpr (PPO) {
        if (r0 + lane < a.N) ll[r0 + lane] = row_ll(sm + L.PN, sm[L.SL], L, lane);
      } else {
        const double v = r0 + lane < a.N ? (double)row_term(sm, L, a.loss_type, lane) : 0.0;
        bsum += amx::wave_sum(v);
      }
    }
    __syncthreads();
  }
  if (!PPO && t == 0) a.partials[blockIdx.x] = bsum;
}

__global__ __launch_bounds__(NT, 1) void k_bcfit_eval(EvalArgs a) { eval_body<false>(a, nullptr); }

__global__ __launch_bounds__(NT, 1) void k_ppo_old_ll(EvalArgs a, float* ll) { eval_body<true>(a, ll); }

// NPG's log-likelihood pass (amx_npg_ll): k_ppo_old_ll's rows and arithmetic (the same LL bits, so
// a ratio of equal policies is exp(0)); each workgroup also leaves the fp64 sum of its rows' LL
// (its chunks in order, a wave butterfly per chunk) in partials[block], and, when asked, every
// row's LL and policy mean.
__global__ __launch_bounds__(NT, 1) void k_npg_ll(EvalArgs a, float* __restrict__ ll, float* __restrict__ mean) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Lay L(a.S, a.A, true);
  const Flat F(a.S, a.A);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  stage_theta(sm, L, F, a.theta);
  __syncthreads();
  if (wave == 0) {
    const float sl = sum_log_std(sm + L.ls, L);
    if (lane == 0) sm[L.SL] = sl;
  }
  double bsum = 0.0;
  const int chunks = (a.N + BB - 1) / BB;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int r0 = ch * BB;
    // rows past N read row N - 1 and are left out of the sum
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int c = lane + 64 * (u & 3), r = wave * 4 + (u >> 2);
      const int g = r0 + r < a.N ? r0 + r : a.N - 1;
      if (c < a.S) sm[L.X + r * L.XS + c] = a.obs[(long long)g * a.ldo + c];
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int r = wave * 4 + u;
      const int g = r0 + r < a.N ? r0 + r : a.N - 1;
      if (lane < a.A) sm[L.ACT + r * L.AS + lane] = a.act[(long long)g * a.lda + lane];
    }
    __syncthreads();
    forward<false, true, true>(sm, L, LOSS_MLE, nullptr, false, mean ? mean + (long long)r0 * a.A : nullptr,
                               a.N - r0);
    if (wave == 0) {
      const bool ok = r0 + lane < a.N;
      const float v = row_ll(sm + L.PN, sm[L.SL], L, lane);
      if (ll && ok) ll[r0 + lane] = v;
      bsum += amx::wave_sum(ok ? (double)v : 0.0);
    }
    __syncthreads();
  }
  if (t == 0) a.partials[blockIdx.x] = bsum;
}

// the workgroups' partials in workgroup order -> mean((mu - a)^2) or -mean(LL)
__global__ void k_bcfit_eval_sum(const double* __restrict__ partials, int nb, int N, int A, int loss_type,
                                 double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += partials[b];
    out[0] = loss_type == LOSS_MLE ? -s / (double)N : s / ((double)N * (double)A);
  }
}

int check_shape(const char* fn, int S, int A) {
  AMX_CHECK_ARG(S > 0 && S <= MAXS && A > 0 && A <= MAXA, "%s: S=%d (1..%d), A=%d (1..%d)", fn, S, MAXS, A, MAXA);
  return AMX_OK;
}

int check_data(const char* fn, const amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act,
               long long lda, int loss_type) {
  int rc = check_shape(fn, ctx->S, ctx->A);
  if (rc) return rc;
  AMX_CHECK_ARG(N > 0, "%s: N=%d", fn, N);
  AMX_CHECK_ARG(obs && act, "%s: null obs / act", fn);
  AMX_CHECK_ARG(ldo >= ctx->S && lda >= ctx->A, "%s: ldo=%lld < S=%d or lda=%lld < A=%d", fn, ldo, ctx->S, lda, ctx->A);
  AMX_CHECK_ARG(loss_type == LOSS_MSE || loss_type == LOSS_MLE, "%s: loss_type=%d (0 = MSE, 1 = MLE)", fn, loss_type);
  return AMX_OK;
}

template <typename K>
int allow_lds(K kern, size_t bytes) {
  AMX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bytes));
  return AMX_OK;
}

}  // namespace

extern "C" long long amx_bcfit_work(int S, int A) {
  if (check_shape("amx_bcfit_work", S, A)) return -1;
  return (long long)EVAL_MAXB * (long long)sizeof(double);
}

extern "C" int amx_bcfit_steps(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
                               const int32_t* idx, int n_steps, float* theta, float* adam_m, float* adam_v,
                               long long* adam_step, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int loss_type, float* step_loss, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_bcfit_steps: null ctx");
  AMX_CHECK_ARG(n_steps >= 0, "amx_bcfit_steps: n_steps=%d", n_steps);
  AMX_CHECK_ARG(idx, "amx_bcfit_steps: null idx");
  int rc = check_data("amx_bcfit_steps", ctx, N, obs, ldo, act, lda, loss_type);
  if (rc) return rc;
  AMX_CHECK_ARG(theta && adam_m && adam_v && adam_step && step_loss,
                "amx_bcfit_steps: null theta / adam_m / adam_v / adam_step / step_loss");
  AMX_CHECK_ARG(((uintptr_t)adam_step & 7u) == 0, "amx_bcfit_steps: misaligned adam_step");
  AMX_CHECK_ARG(lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 &&
                    weight_decay >= 0.0,
                "amx_bcfit_steps: lr=%g betas=(%g, %g) eps=%g weight_decay=%g", lr, beta1, beta2, eps, weight_decay);
  if (n_steps == 0) return AMX_OK;
  const Lay L(ctx->S, ctx->A);
  AMX_CHECK_ARG(L.bytes() <= 160 * 1024, "amx_bcfit_steps: %zu B of LDS", L.bytes());
  rc = allow_lds(k_bcfit_steps, L.bytes());
  if (rc) return rc;
  StepArgs a = {ctx->S, ctx->A, N, n_steps, loss_type, obs, ldo, act, lda, idx, theta, adam_m, adam_v, adam_step,
                lr, beta1, beta2, eps, weight_decay, step_loss};
  hipLaunchKernelGGL(k_bcfit_steps, dim3(1), dim3(NT), L.bytes(), (hipStream_t)stream, a);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_bcfit_eval(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
                              const float* theta, int loss_type, void* work, double* loss, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_bcfit_eval: null ctx");
  int rc = check_data("amx_bcfit_eval", ctx, N, obs, ldo, act, lda, loss_type);
  if (rc) return rc;
  AMX_CHECK_ARG(theta && work && loss, "amx_bcfit_eval: null theta / work / loss");
  AMX_CHECK_ARG(((uintptr_t)work & 7u) == 0 && ((uintptr_t)loss & 7u) == 0, "amx_bcfit_eval: misaligned work / loss");
  const Lay L(ctx->S, ctx->A);
  AMX_CHECK_ARG(L.bytes() <= 160 * 1024, "amx_bcfit_eval: %zu B of LDS", L.bytes());
  rc = allow_lds(k_bcfit_eval, L.bytes());
  if (rc) return rc;
  const int chunks = (N + BB - 1) / BB;
  int nb = ctx->n_cus > 0 ? ctx->n_cus : 1;  // one workgroup per CU (the image takes most of its LDS)
  if (nb > chunks) nb = chunks;
  if (nb > EVAL_MAXB) nb = EVAL_MAXB;
  EvalArgs a = {ctx->S, ctx->A, N, loss_type, obs, ldo, act, lda, theta, (double*)work};
  hipLaunchKernelGGL(k_bcfit_eval, dim3(nb), dim3(NT), L.bytes(), (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_bcfit_eval_sum, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work, nb, N, ctx->A,
                     loss_type, loss);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

// ---- PPO (ppo_clip.py:23-121) ------------------------------------------------------------------

extern "C" int amx_ppo_steps(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
                             const float* adv, const float* ll_old, const float* log_std_old, int old_mode,
                             const int32_t* idx, int n_steps, float* theta, float* adam_m, float* adam_v,
                             long long* adam_step, double lr, double beta1, double beta2, double eps,
                             double clip_coef, float* step_loss, int32_t* step_clipped, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_ppo_steps: null ctx");
  AMX_CHECK_ARG(n_steps >= 0, "amx_ppo_steps: n_steps=%d", n_steps);
  AMX_CHECK_ARG(idx, "amx_ppo_steps: null idx");
  int rc = check_data("amx_ppo_steps", ctx, N, obs, ldo, act, lda, LOSS_MLE);
  if (rc) return rc;
  AMX_CHECK_ARG(adv, "amx_ppo_steps: null adv");
  AMX_CHECK_ARG(old_mode == AMX_PPO_OLD_SNAPSHOT || old_mode == AMX_PPO_OLD_TRACKS_MEAN,
                "amx_ppo_steps: old_mode=%d (0 = snapshot, 1 = tracks mean)", old_mode);
  AMX_CHECK_ARG(old_mode != AMX_PPO_OLD_SNAPSHOT || ll_old, "amx_ppo_steps: null ll_old in snapshot mode");
  AMX_CHECK_ARG(old_mode != AMX_PPO_OLD_TRACKS_MEAN || log_std_old,
                "amx_ppo_steps: null log_std_old in tracks-mean mode");
  AMX_CHECK_ARG(theta && adam_m && adam_v && adam_step && step_loss && step_clipped,
                "amx_ppo_steps: null theta / adam_m / adam_v / adam_step / step_loss / step_clipped");
  AMX_CHECK_ARG(((uintptr_t)adam_step & 7u) == 0, "amx_ppo_steps: misaligned adam_step");
  AMX_CHECK_ARG(lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                "amx_ppo_steps: lr=%g betas=(%g, %g) eps=%g", lr, beta1, beta2, eps);
  AMX_CHECK_ARG(clip_coef >= 0.0 && clip_coef < 1.0, "amx_ppo_steps: clip_coef=%g (0 <= c < 1)", clip_coef);
  if (n_steps == 0) return AMX_OK;
  const Lay L(ctx->S, ctx->A, true);
  AMX_CHECK_ARG(L.bytes() <= 160 * 1024, "amx_ppo_steps: %zu B of LDS", L.bytes());
  rc = allow_lds(k_ppo_steps, L.bytes());
  if (rc) return rc;
  StepArgs a = {ctx->S, ctx->A, N, n_steps, LOSS_MLE, obs, ldo, act, lda, idx, theta, adam_m, adam_v, adam_step,
                lr, beta1, beta2, eps, 0.0, step_loss};
  PpoArgs p = {adv, old_mode == AMX_PPO_OLD_SNAPSHOT ? ll_old : nullptr, log_std_old, (float)(1.0 - clip_coef),
               (float)(1.0 + clip_coef), step_clipped};
  hipLaunchKernelGGL(k_ppo_steps, dim3(1), dim3(NT), L.bytes(), (hipStream_t)stream, a, p);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_ppo_old_ll(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
                              const float* theta, float* ll_old, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_ppo_old_ll: null ctx");
  int rc = check_data("amx_ppo_old_ll", ctx, N, obs, ldo, act, lda, LOSS_MLE);
  if (rc) return rc;
  AMX_CHECK_ARG(theta && ll_old, "amx_ppo_old_ll: null theta / ll_old");
  const Lay L(ctx->S, ctx->A, true);
  AMX_CHECK_ARG(L.bytes() <= 160 * 1024, "amx_ppo_old_ll: %zu B of LDS", L.bytes());
  rc = allow_lds(k_ppo_old_ll, L.bytes());
  if (rc) return rc;
  const int chunks = (N + BB - 1) / BB;
  int nb = ctx->n_cus > 0 ? ctx->n_cus : 1;
  if (nb > chunks) nb = chunks;
  EvalArgs a = {ctx->S, ctx->A, N, LOSS_MLE, obs, ldo, act, lda, theta, nullptr};
  hipLaunchKernelGGL(k_ppo_old_ll, dim3(nb), dim3(NT), L.bytes(), (hipStream_t)stream, a, ll_old);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

// ---- NPG's log-likelihood pass (the BC term of NPG.CPI_surrogate and its dist-info entries) ------

namespace {
int npg_ll_blocks(const amx_ctx* ctx, int N) {
  const int chunks = (N + BB - 1) / BB;
  int nb = ctx->n_cus > 0 ? ctx->n_cus : 1;
  if (nb > EVAL_MAXB) nb = EVAL_MAXB;
  return nb > chunks ? chunks : nb;
}
}  // namespace

extern "C" int amx_npg_ll_blocks(amx_ctx* ctx, int N) {
  if (!ctx || N <= 0) return -1;
  return npg_ll_blocks(ctx, N);
}

extern "C" int amx_npg_ll(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
                          const float* theta, double* partials, float* ll, float* mean, void* stream) {
  AMX_CHECK_ARG(ctx, "amx_npg_ll: null ctx");
  int rc = check_data("amx_npg_ll", ctx, N, obs, ldo, act, lda, LOSS_MLE);
  if (rc) return rc;
  AMX_CHECK_ARG(theta && partials, "amx_npg_ll: null theta / partials");
  AMX_CHECK_ARG(((uintptr_t)partials & 7u) == 0, "amx_npg_ll: misaligned partials");
  const Lay L(ctx->S, ctx->A, true);
  AMX_CHECK_ARG(L.bytes() <= 160 * 1024, "amx_npg_ll: %zu B of LDS", L.bytes());
  rc = allow_lds(k_npg_ll, L.bytes());
  if (rc) return rc;
  EvalArgs a = {ctx->S, ctx->A, N, LOSS_MLE, obs, ldo, act, lda, theta, partials};
  hipLaunchKernelGGL(k_npg_ll, dim3(npg_ll_blocks(ctx, N)), dim3(NT), L.bytes(), (hipStream_t)stream, a, ll, mean);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}
