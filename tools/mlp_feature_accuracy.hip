// Host check of mlp_feature (csrc/amx_h3.h: the EPI_MLPF epilogue's phi = cos(tanh(z)) * scale)
// against long double: the function is host-callable, so the device's arithmetic (fp64 FMAs; the
// device's reciprocal is v_rcp_f64 + one Newton step, the host's a division) is measured without
// a GPU.  Prints the worst error in units of the fp32 result's ulp over a dense grid and at the
// edges.
//   hipcc -O3 -ffp-contract=off -I include -I amp_extensions_amd/csrc tools/mlp_feature_accuracy.hip \
//         -o tools/mlp_feature_accuracy && tools/mlp_feature_accuracy
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "amx_h3.h"

static double ulp_of(float v) {
  const float a = std::fabs(v);
  return (double)std::nextafterf(a, INFINITY) - (double)a;
}

int main() {
  const float scales[] = {0.0625f, 0.125f, 0.088388346f, 0.044194173f};
  double worst = 0.0, worst_z = 0.0, worst_abs = 0.0;
  long n = 0;
  for (float scale : scales) {
    for (long i = -12000000; i <= 12000000; ++i) {
      const float z = (float)((double)i * 1e-6);
      const float got = mlp_feature(z, scale);
      const long double ref = cosl(tanhl((long double)z)) * (long double)scale;
      const double err = std::fabs((double)((long double)got - ref));
      const double u = err / ulp_of(got);
      if (u > worst) { worst = u; worst_z = z; }
      if (err / scale > worst_abs) worst_abs = err / scale;
      ++n;
    }
  }
  std::printf("grid: %ld values of z in [-12, 12], 4 scales: max error %.4f ulp of phi (z = %.6f), "
              "max |error| / scale %.3e\n", n, worst, worst_z, worst_abs);
  const float edge[] = {0.0f, -0.0f, 1e-30f, -1e-30f, 1e-8f, 24.9f, 25.0f, 25.1f, -25.0f, 88.0f, -88.0f, 1e10f,
                        -1e10f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY};
  int bad = 0;
  for (float z : edge) {
    const float got = mlp_feature(z, 0.0625f);
    const long double ref = cosl(tanhl((long double)z)) * 0.0625L;
    const double u = std::fabs((double)((long double)got - ref)) / ulp_of(got);
    std::printf("  z = %-12g phi = %.9g  (%.3f ulp)\n", z, got, u);
    bad += !(u <= 0.51);
  }
  const float nan_out = mlp_feature(std::numeric_limits<float>::quiet_NaN(), 0.0625f);
  std::printf("  z = nan          phi = %g\n", nan_out);
  bad += !std::isnan(nan_out);
  bad += !(worst <= 0.51);
  std::printf(bad ? "FAIL\n" : "ok: within 0.51 ulp everywhere, NaN propagates\n");
  return bad != 0;
}
