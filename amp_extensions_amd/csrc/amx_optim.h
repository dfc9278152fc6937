// The optimizers of the device fits (amx_vfit / amx_efit / amx_dfit / amx_bcfit.hip), once:
// torch.optim.Adam's and torch.optim.SGD's single-tensor updates restated op for op in fp32, the
// bias corrections 1 - beta^t formed in double.  The library is built with -ffp-contract=off and
// every product is written out, so the sequence of operations below is the sequence of roundings.
// amx_optim.hip holds the two kernels that need nothing but this arithmetic: the update of a
// list of flat tensors and the sum of squares of one.
#pragma once

#include <math.h>

#include "amx_common.h"

namespace amx {

// Adam's constants of one step.
struct AdamConst {
  float step, bc2s, omb1, b2, omb2, eps;  // lr / bc1, sqrt(bc2), 1 - beta1, beta2, 1 - beta2, eps
  AdamConst() = default;
  // from the bias corrections bc = 1 - beta^t (a caller that forms the two powers side by side)
  __host__ __device__ AdamConst(double bc1, double bc2, double lr, double b1, double b2_, double eps_)
      : step((float)(lr / bc1)), bc2s((float)sqrt(bc2)), omb1((float)(1.0 - b1)), b2((float)b2_),
        omb2((float)(1.0 - b2_)), eps((float)eps_) {}
  // of step t (1-based)
  __host__ __device__ AdamConst(long long t, double lr, double b1, double b2_, double eps_)
      : AdamConst(1.0 - pow(b1, (double)t), 1.0 - pow(b2_, (double)t), lr, b1, b2_, eps_) {}
};

// torch.optim.Adam's single-tensor update: exp_avg.lerp_(g, 1 - b1);
// exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2); denom = sqrt(v) / sqrt(bc2) + eps; p.addcdiv_.
// Weight decay is the caller's: g = g + wd * w (grad.add(p, alpha=wd)) ahead of the call.
__host__ __device__ inline void adam_apply(float& w, float& m, float& v, float g, const AdamConst& c) {
  m = m + (g - m) * c.omb1;
  v = v * c.b2 + (c.omb2 * g) * g;
  const float den = sqrtf(v) / c.bc2s + c.eps;
  w = w - c.step * (m / den);
}

// torch.optim.SGD with momentum, dampening 0: buf = mu buf + g (the first step's zero buffer
// gives g exactly); p -= lr (g + mu buf) with Nesterov, p -= lr buf without.
template <bool NESTEROV>
__host__ __device__ inline void sgd_apply(float& w, float& buf, float g, float lr, float mu) {
  buf = buf * mu + g;
  w = NESTEROV ? w - lr * (g + mu * buf) : w - lr * buf;
}

// ---- the two shared kernels (amx_optim.hip) --------------------------------------------------

enum OptimKind { OPTIM_ADAM, OPTIM_SGD, OPTIM_SGD_NESTEROV };

// A member's constants of one step, as a fit's prep kernel publishes them to update_tensors.
struct StepConst {
  float coef;      // the gradient's factor: clip_grad_norm_'s clip_coef_clamped, or 1
  AdamConst adam;  // OPTIM_ADAM
  float lr, mu;    // OPTIM_SGD*
};
constexpr int STEP_CONST_FLOATS = 16;  // floats between two members' constants
static_assert(sizeof(StepConst) <= STEP_CONST_FLOATS * sizeof(float), "step constants");

constexpr int OPTIM_MAX_T = 16;  // tensors of a list
constexpr int SUMSQ_NB = 64;     // workgroups (partial sums) per group of sum_squares

// Tensors of member 0, each `stride` floats from the next member's, and their places in the flat
// gradient / state vectors: tensor t is off[t] .. off[t + 1] (multiples of 4, 16-byte aligned).
struct TensorList {
  float* w[OPTIM_MAX_T];
  long long stride[OPTIM_MAX_T];
  long long off[OPTIM_MAX_T + 1];
  int n;
};

// w, s1 (and s2: Adam) of every tensor of every member <- one optimizer step on grad * coef.
// grad / s1 / s2: [members][P] flat vectors; cst: [members][STEP_CONST_FLOATS].
AMX_INTERNAL int update_tensors(const TensorList& T, int members, OptimKind kind, const float* grad, float* s1,
                                float* s2, long long P, const float* cst, hipStream_t st);

// part[g * SUMSQ_NB + b] = scale * (workgroup b's share of the sum of x^2 over the tensors of
// group g), in fp64; the SUMSQ_NB partials of a group are the caller's to add.
AMX_INTERNAL int sum_squares(const TensorList& T, int groups, double scale, double* part, hipStream_t st);

}  // namespace amx
