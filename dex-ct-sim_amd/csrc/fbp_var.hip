// Noise propagation through the filtered back-projection of fbp.hip for gfx950: the (co)variance of every image pixel
// from the (co)variance of independent sinogram pixels.
//
// The FBP is linear, image = M sino, and the sinogram pixels are independent (the library's noise model), so the image
// pixel's (co)variance is (M o M) s: the element-wise square of the FBP matrix applied to the sinogram (co)variance s.
// With the filter and the interpolating back-projection written out (include/dexct.h has the full statement):
//   filter:        A(line, n) = dg^2 sum_m s(line, m) W_m^2 (2 w_P)^2 g[n - m]^2
//                  B(line, n) = dg^2 sum_m s(line, m) W_m^2 (2 w_P)^2 g[n - m] g[n + 1 - m]       (n < N - 1; B[N - 1] = 0)
//   back-project:  K s(x, y)  = dbeta^2 sum_views [ (1 - w)^2 A[k] + w^2 A[k + 1] + 2 w (1 - w) B[k] ] / L^4
// A is the variance of a filtered sample, B the covariance of two neighbouring ones (which the linear interpolation
// mixes); k, w, L^2 and the in-fan condition are those of fbp_backproject_kernel.  The operator is linear in s, so every
// plane of a packed covariance (00, 01, 11, ...) goes through it unchanged.  Everything is float64: the consumer
// (dexct_cov_quadform) cancels the planes against each other by 1 / (1 - rho^2).
#include <type_traits>

#include "common.h"
#include "fan_pixel.h"
#include "parker.h"

namespace dexct {

constexpr int kVarBlock = 256;

// One workgroup per (line, plane).  LDS: weighted line [n] + taps [2n - 1], float64.  cov is [line][channel][plane];
// qa, qb likewise.  Output k walks m upwards, so the tap index k - m walks downwards and the tap of the step before is
// g[k + 1 - m]: one LDS read of a tap per step serves both sums.  Two accumulator chains per sum (even and odd m).
__global__ __launch_bounds__(kVarBlock) void fbp_var_filter_kernel(const double* __restrict__ cov,
                                                                   const double* __restrict__ taps,
                                                                   const double* __restrict__ weight, int n, int n_rows,
                                                                   int n_planes, double dgamma, double theta_tot,
                                                                   int view_offset, int n_views_total,
                                                                   double* __restrict__ qa, double* __restrict__ qb) {
  extern __shared__ __attribute__((aligned(16))) double lds_var[];
  double* line = lds_var;       // [n]
  double* g = lds_var + n;      // [2n - 1], g[j] = tap of offset j - (n - 1)
  const int plane = blockIdx.y;
  const size_t base = (size_t)blockIdx.x * n;
  const int view = (int)(blockIdx.x / (unsigned)n_rows) + view_offset;
  const bool short_scan = theta_tot < 2.0 * 3.14159265358979323846;
  for (int i = threadIdx.x; i < n; i += kVarBlock) {
    const double wt = weight[i];
    double s = cov[(base + i) * n_planes + plane] * (wt * wt);
    if (short_scan) {
      const double p = 2.0 * parker_weight(theta_tot, view, n_views_total, i, n, dgamma);
      s *= p * p;
    }
    line[i] = s;
  }
  for (int i = threadIdx.x; i < 2 * n - 1; i += kVarBlock) g[i] = taps[i];
  __syncthreads();
  const double dg2 = dgamma * dgamma;
  for (int k = threadIdx.x; k < n; k += kVarBlock) {
    const double* gk = g + k + (n - 1);        // gk[-m] = g[(k - m) + n - 1]
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    double prev = k < n - 1 ? gk[1] : 0.0;     // the tap of offset k + 1 (m = -1); none for the last channel
    int m = 0;
    for (; m + 1 < n; m += 2) {
      const double g0 = gk[-m], g1 = gk[-m - 1];
      const double t0 = line[m] * g0, t1 = line[m + 1] * g1;
      a0 = fma(t0, g0, a0);
      b0 = fma(t0, prev, b0);
      a1 = fma(t1, g1, a1);
      b1 = fma(t1, g0, b1);
      prev = g1;
    }
    if (m < n) {
      const double g0 = gk[-m];
      const double t0 = line[m] * g0;
      a0 = fma(t0, g0, a0);
      b0 = fma(t0, prev, b0);
    }
    const size_t o = (base + k) * n_planes + plane;
    qa[o] = (a0 + a1) * dg2;
    qb[o] = k < n - 1 ? (b0 + b1) * dg2 : 0.0;
  }
}

struct VarGeom {
  int n_views, n_channels, n_rows, n_matrix, n_planes, plane0;
  double sid, dgamma, dbeta, pixel;   // pixel = FOV / n_matrix
};

// One thread per pixel (x, y), T planes from plane0 on and R consecutive rows.  qa, qb are [view][row][channel][plane].
// The geometry of a (pixel, view) pair is that of fbp_backproject_kernel: both call fan_hit (fan_pixel.h); the three
// interpolation weights carry 1 / L^4 and are formed once per pair, then applied to T x R accumulators in registers.
template <int T, int R>
__global__ __launch_bounds__(kVarBlock) void fbp_var_backproject_kernel(const double* __restrict__ qa,
                                                                        const double* __restrict__ qb,
                                                                        const double* __restrict__ view_cs, VarGeom g,
                                                                        double* __restrict__ img) {
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
  const int iy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int row0 = blockIdx.z * R;
  if (ix >= g.n_matrix || iy >= g.n_matrix) return;
  const double x = pixel_centre(ix, g.n_matrix, g.pixel), y = pixel_centre(iy, g.n_matrix, g.pixel);
  const double inv_dg = 1.0 / g.dgamma, half = 0.5 * (g.n_channels - 1);
  const int n_rows_here = g.n_rows - row0 < R ? g.n_rows - row0 : R;
  const size_t row_stride = (size_t)g.n_channels * g.n_planes;
  double acc[R][T];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < T; ++t) acc[r][t] = 0.0;
  for (int v = 0; v < g.n_views; ++v) {
    const FanHit h = fan_hit(x, y, g.sid, view_cs[2 * v], view_cs[2 * v + 1], inv_dg, half);   // view_cs: wave-uniform
    if (h.in_fan(g.n_channels)) {
      const double w = h.frac, u = 1.0 - w;
      const double l2 = h.dx * h.dx + h.dy * h.dy;
      const double inv_l4 = 1.0 / (l2 * l2);
      const double c0 = u * u * inv_l4, c1 = w * w * inv_l4, c2 = 2.0 * w * u * inv_l4;
      const size_t o = (((size_t)v * g.n_rows + row0) * g.n_channels + h.k) * g.n_planes + g.plane0;
      const double* pa = qa + o;
      const double* pb = qb + o;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < n_rows_here) {
#pragma unroll
          for (int t = 0; t < T; ++t)
            acc[r][t] = fma(c0, pa[t], fma(c1, pa[g.n_planes + t], fma(c2, pb[t], acc[r][t])));
        }
        pa += row_stride;
        pb += row_stride;
      }
    }
  }
  const double db2 = g.dbeta * g.dbeta;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r < n_rows_here) {
      double* out = img + (((size_t)(row0 + r) * g.n_matrix + iy) * g.n_matrix + ix) * g.n_planes + g.plane0;
#pragma unroll
      for (int t = 0; t < T; ++t) out[t] = acc[r][t] * db2;
    }
}

struct FdkVarGeom {
  int n_views, n_channels, n_rows, n_matrix, n_slices, n_planes, plane0;
  double sid, sdd, dgamma, dbeta, pixel;
  double row_z0, row_dz, src_z, z0, dz;
};

// Feldkamp: fdk_backproject_kernel's geometry.  The detector rows are independent, so the row interpolation adds the
// squares of its two weights: with V_r = (1 - w)^2 A[r, k] + w^2 A[r, k + 1] + 2 w (1 - w) B[r, k] a view contributes
// [ (1 - wr)^2 c_r0^2 V_r0 + wr^2 c_(r0 + 1)^2 V_(r0 + 1) ] / L^4, c_r = row_weight[r] the cone weight.
template <int T, int R>
__global__ __launch_bounds__(kVarBlock) void fdk_var_backproject_kernel(const double* __restrict__ qa,
                                                                        const double* __restrict__ qb,
                                                                        const double* __restrict__ view_cs,
                                                                        const double* __restrict__ row_weight,
                                                                        FdkVarGeom g, double* __restrict__ img) {
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
  const int iy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int k0 = blockIdx.z * R;
  if (ix >= g.n_matrix || iy >= g.n_matrix) return;
  const double x = pixel_centre(ix, g.n_matrix, g.pixel), y = pixel_centre(iy, g.n_matrix, g.pixel);
  const double inv_dg = 1.0 / g.dgamma, half = 0.5 * (g.n_channels - 1), inv_rdz = 1.0 / g.row_dz;
  const int n_here = g.n_slices - k0 < R ? g.n_slices - k0 : R;
  const size_t row_stride = (size_t)g.n_channels * g.n_planes;
  double acc[R][T];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < T; ++t) acc[r][t] = 0.0;
  for (int v = 0; v < g.n_views; ++v) {
    const FanHit h = fan_hit(x, y, g.sid, view_cs[2 * v], view_cs[2 * v + 1], inv_dg, half);
    if (!h.in_fan(g.n_channels)) continue;
    const double w = h.frac, u = 1.0 - w;
    const double c0 = u * u, c1 = w * w, c2 = 2.0 * w * u;
    const double l2 = h.dx * h.dx + h.dy * h.dy;
    const double inv_l4 = 1.0 / (l2 * l2);
    const double mag = g.sdd / sqrt(l2);                  // magnification of heights from the voxel to the detector
    const size_t ov = ((size_t)v * g.n_rows * g.n_channels + h.k) * g.n_planes + g.plane0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < n_here) {
        const RowHit rh = fdk_row(g.z0 + (k0 + r) * g.dz, g.src_z, mag, g.row_z0, inv_rdz);
        if (rh.on_detector(g.n_rows)) {
          const int r0 = rh.r0;
          const double wr = rh.frac, ur = 1.0 - wr;
          const double ra = row_weight[r0], rb = row_weight[r0 + 1];
          const double fa = ur * ur * (ra * ra) * inv_l4, fb = wr * wr * (rb * rb) * inv_l4;
          const double* pa = qa + ov + (size_t)r0 * row_stride;
          const double* pb = qb + ov + (size_t)r0 * row_stride;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const double va = fma(c0, pa[t], fma(c1, pa[g.n_planes + t], c2 * pb[t]));
            const double vb = fma(c0, pa[row_stride + t], fma(c1, pa[row_stride + g.n_planes + t], c2 * pb[row_stride + t]));
            acc[r][t] = fma(fa, va, fma(fb, vb, acc[r][t]));
          }
        }
      }
    }
  }
  const double db2 = g.dbeta * g.dbeta;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r < n_here) {
      double* out = img + (((size_t)(k0 + r) * g.n_matrix + iy) * g.n_matrix + ix) * g.n_planes + g.plane0;
#pragma unroll
      for (int t = 0; t < T; ++t) out[t] = acc[r][t] * db2;
    }
}

// The planes of one call go through launches of 6, 3 and 1 planes (any n_planes >= 1; a plane's arithmetic does not depend
// on the launch it is in).  Rows per thread: T x R = 24 accumulators at the most stay in registers.
template <int T>
constexpr int var_rows() { return T == 6 ? 4 : 8; }

template <int T>
void launch_var_backproject(const double* qa, const double* qb, const double* view_cs, VarGeom g, double* img,
                            hipStream_t st) {
  constexpr int R = var_rows<T>();
  const unsigned gx = (g.n_matrix + 63) / 64, gy = (g.n_matrix + 3) / 4;
  if (g.n_rows > 1)
    hipLaunchKernelGGL((fbp_var_backproject_kernel<T, R>), dim3(gx, gy, (g.n_rows + R - 1) / R), dim3(kVarBlock), 0, st, qa,
                       qb, view_cs, g, img);
  else
    hipLaunchKernelGGL((fbp_var_backproject_kernel<T, 1>), dim3(gx, gy, 1), dim3(kVarBlock), 0, st, qa, qb, view_cs, g, img);
}

template <int T>
void launch_fdk_var_backproject(const double* qa, const double* qb, const double* view_cs, const double* row_weight,
                                FdkVarGeom g, double* img, hipStream_t st) {
  constexpr int R = T == 6 ? 2 : 4;
  dim3 grid((g.n_matrix + 63) / 64, (g.n_matrix + 3) / 4, (g.n_slices + R - 1) / R);
  hipLaunchKernelGGL((fdk_var_backproject_kernel<T, R>), grid, dim3(kVarBlock), 0, st, qa, qb, view_cs, row_weight, g, img);
}

// Walks the planes of a call in groups of 6, 3 and 1; ``launch(tag, plane0)`` starts the kernel of std::integral_constant<int,
// T> planes from plane0 on.  Stops at the first launch error (earlier groups have then written their planes).
template <class Launch>
int for_plane_groups(int n_planes, Launch launch) {
  for (int plane0 = 0; plane0 < n_planes;) {
    const int left = n_planes - plane0;
    if (left >= 6) {
      launch(std::integral_constant<int, 6>{}, plane0);
      plane0 += 6;
    } else if (left >= 3) {
      launch(std::integral_constant<int, 3>{}, plane0);
      plane0 += 3;
    } else {
      launch(std::integral_constant<int, 1>{}, plane0);
      plane0 += 1;
    }
    DEXCT_LAUNCH_CHECK();
  }
  return DEXCT_OK;
}

}  // namespace dexct

using namespace dexct;

extern "C" {

int dexct_fbp_var_filter(const double* cov, int32_t n_views, int32_t n_rows, int32_t n_channels, int32_t n_planes,
                         const double* taps, const double* weight, double dgamma, double theta_tot, int32_t view_offset,
                         int32_t n_views_total, double* qa, double* qb, void* stream) {
  if (!cov || !taps || !weight || !qa || !qb || n_views < 1 || n_rows < 1 || n_channels < 2 || n_planes < 1 ||
      n_views_total < n_views || view_offset < 0 || view_offset > n_views_total - n_views)
    return DEXCT_EINVAL;
  if (!(dgamma > 0.0) || !(theta_tot > 0.0)) return DEXCT_EINVAL;
  // a short scan needs pi + the full fan angle (dexct_fbp_parker's rule); 2 pi and beyond carries no Parker weight
  if (theta_tot < 2.0 * kPi && !short_scan_complete(theta_tot, n_channels, dgamma)) return DEXCT_EINVAL;
  if (n_channels > DEXCT_FBP_VAR_MAX_CHANNELS || n_planes > 65535 || (int64_t)n_views * n_rows > 0x7FFFFFFFll)
    return DEXCT_ERANGE;
  const size_t lds = (size_t)(3 * n_channels - 1) * sizeof(double);
  hipLaunchKernelGGL(fbp_var_filter_kernel, dim3((unsigned)(n_views * n_rows), (unsigned)n_planes), dim3(kVarBlock), lds,
                     as_stream(stream), cov, taps, weight, n_channels, n_rows, n_planes, dgamma, theta_tot, view_offset,
                     n_views_total, qa, qb);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_fbp_var_backproject(const double* qa, const double* qb, const double* view_cs, int32_t n_views,
                              int32_t n_channels, int32_t n_rows, int32_t n_planes, double sid, double dgamma,
                              double dbeta, int32_t n_matrix, double fov, double* image_cov, void* stream) {
  const int bad = check_fan_args(qa && qb && view_cs && image_cov && n_planes >= 1, n_views, n_channels, n_rows, n_matrix, sid,
                                 dgamma, fov);
  if (bad) return bad;
  VarGeom g{n_views, n_channels, n_rows, n_matrix, n_planes, 0, sid, dgamma, dbeta, fov / n_matrix};
  hipStream_t st = as_stream(stream);
  return for_plane_groups(n_planes, [&](auto planes, int plane0) {
    g.plane0 = plane0;
    launch_var_backproject<decltype(planes)::value>(qa, qb, view_cs, g, image_cov, st);
  });
}

int dexct_fdk_var_backproject(const double* qa, const double* qb, const double* view_cs, const double* row_weight,
                              int32_t n_views, int32_t n_channels, int32_t n_rows, int32_t n_planes, double sid, double sdd,
                              double dgamma, double dbeta, double row_z0, double row_dz, double src_z, int32_t n_matrix,
                              double fov, int32_t n_slices, double z0, double dz, double* image_cov, void* stream) {
  const int bad = check_cone_args(qa && qb && view_cs && row_weight && image_cov && n_planes >= 1, n_views, n_channels, n_rows,
                                  n_matrix, n_slices, 2, sid, sdd, dgamma, fov, row_dz, dz);
  if (bad) return bad;
  FdkVarGeom g{n_views, n_channels, n_rows, n_matrix, n_slices, n_planes, 0, sid, sdd, dgamma, dbeta, fov / n_matrix,
               row_z0, row_dz, src_z, z0, dz};
  hipStream_t st = as_stream(stream);
  return for_plane_groups(n_planes, [&](auto planes, int plane0) {
    g.plane0 = plane0;
    launch_fdk_var_backproject<decltype(planes)::value>(qa, qb, view_cs, row_weight, g, image_cov, st);
  });
}

}  // extern "C"
