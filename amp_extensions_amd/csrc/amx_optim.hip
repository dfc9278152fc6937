// The two kernels the device fits share (amx_optim.h): one optimizer step over a list of flat
// tensors, and the sum of squares of one.  Both are internal: the fits launch them between
// their own kernels, and stream order is the only synchronisation.
#include "amx_optim.h"

namespace amx {
namespace {

// grid (256, members): workgroup (x, g) walks every tensor of member g in float4, 256 x 256
// threads apart.  The gradient is scaled by the member's coefficient first (g * 1.0f is exact).
template <OptimKind KIND>
__global__ __launch_bounds__(256) void k_optim_update(TensorList T, const float* __restrict__ grad,
                                                      float* __restrict__ s1, float* __restrict__ s2, long long P,
                                                      const float* __restrict__ cst) {
  const int g = blockIdx.y;
  const StepConst a = *(const StepConst*)(cst + g * STEP_CONST_FLOATS);
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
      if (KIND == OPTIM_ADAM) {
        float4 vv = v[e];
        adam_apply(ww.x, mm.x, vv.x, gg.x, a.adam);
        adam_apply(ww.y, mm.y, vv.y, gg.y, a.adam);
        adam_apply(ww.z, mm.z, vv.z, gg.z, a.adam);
        adam_apply(ww.w, mm.w, vv.w, gg.w, a.adam);
        v[e] = vv;
      } else {
        constexpr bool NV = KIND == OPTIM_SGD_NESTEROV;
        sgd_apply<NV>(ww.x, mm.x, gg.x, a.lr, a.mu);
        sgd_apply<NV>(ww.y, mm.y, gg.y, a.lr, a.mu);
        sgd_apply<NV>(ww.z, mm.z, gg.z, a.lr, a.mu);
        sgd_apply<NV>(ww.w, mm.w, gg.w, a.lr, a.mu);
      }
      w[e] = ww;
      m[e] = mm;
    }
  }
}

// grid (SUMSQ_NB, groups): per thread tensor after tensor in float4, SUMSQ_NB x 256 apart, fp64
// accumulation; then the workgroup's fixed tree
__global__ __launch_bounds__(256) void k_optim_sumsq(TensorList T, double scale, double* __restrict__ part) {
  __shared__ double red[256];
  const int g = blockIdx.y;
  double acc = 0.0;
  for (int t = 0; t < T.n; ++t) {
    const float4* p = (const float4*)(T.w[t] + g * T.stride[t]);
    const long long n4 = (T.off[t + 1] - T.off[t]) / 4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long long)SUMSQ_NB * 256) {
      const float4 v = p[e];
      acc += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
  }
  const double s = block_sum<256>(red, acc);
  if (threadIdx.x == 0) part[g * SUMSQ_NB + blockIdx.x] = scale * s;
}

}  // namespace

int update_tensors(const TensorList& T, int members, OptimKind kind, const float* grad, float* s1, float* s2,
                   long long P, const float* cst, hipStream_t st) {
  const auto kern = kind == OPTIM_ADAM ? k_optim_update<OPTIM_ADAM>
                    : kind == OPTIM_SGD ? k_optim_update<OPTIM_SGD> : k_optim_update<OPTIM_SGD_NESTEROV>;
  hipLaunchKernelGGL(kern, dim3(256, members), dim3(256), 0, st, T, grad, s1, s2, P, cst);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

int sum_squares(const TensorList& T, int groups, double scale, double* part, hipStream_t st) {
  hipLaunchKernelGGL(k_optim_sumsq, dim3(SUMSQ_NB, groups), dim3(256), 0, st, T, scale, part);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

}  // namespace amx
