// Parker's short-scan weight in closed form (internal; fbp.hip has the derivation next to parker_kernel).  Shared by the
// weighting of the sinogram (fbp.hip) and of its variance (fbp_var.hip): one sequence of float64 operations, so both see
// the same weight bit for bit (csrc is built with contraction off).
#pragma once

namespace dexct {

// w of view v (0-based in the whole scan of n_views_total views over theta_tot) and channel c; theta_tot < 2 pi.
__device__ __forceinline__ double parker_weight(double theta_tot, int v, int n_views_total, int c, int n_channels,
                                                double dgamma) {
  const double kPi = 3.14159265358979323846;
  const double beta = theta_tot * (double)v / (double)n_views_total;
  const double gam = ((double)c - 0.5 * (double)(n_channels - 1)) * dgamma;
  const double G = 0.5 * (theta_tot - kPi);
  double w = 1.0;
  if (beta < 2.0 * (G - gam)) {
    const double sn = sin(0.25 * kPi * beta / (G - gam));
    w = sn * sn;
  } else if (beta > kPi - 2.0 * gam) {
    const double sn = sin(0.25 * kPi * (kPi + 2.0 * G - beta) / (G + gam));
    w = sn * sn;
  }
  return w;
}

}  // namespace dexct
