// The (pixel, view) geometry of the pixel-driven fan-beam back-projection, float64: the one copy for the image kernels of
// fbp.hip and the (co)variance kernels of fbp_var.hip, which must hit the same channel with the same fraction for the noise map
// to be that of the image.  With it the argument checks their entry points share (internal).
#pragma once
#include "common.h"

namespace dexct {

// centre of pixel i of n on an axis [cm]
__device__ __forceinline__ double pixel_centre(int i, int n, double pixel) { return (i - 0.5 * n + 0.5) * pixel; }

// Where the ray from the source of a view (cos, sin of its angle: cb, sb; distance sid) through the pixel (x, y) meets the
// equiangular detector: between channels k and k + 1, `frac` of the way.  dx, dy: source to pixel (L^2 = dx^2 + dy^2).
struct FanHit {
  double dx, dy, frac;
  int k;
  __device__ __forceinline__ bool in_fan(int n_channels) const { return k >= 0 && k < n_channels - 1; }
};

// inv_dg = 1 / dgamma, half = (n_channels - 1) / 2
__device__ __forceinline__ FanHit fan_hit(double x, double y, double sid, double cb, double sb, double inv_dg, double half) {
  const double dx = x - sid * cb, dy = y - sid * sb;
  const double dot = -(cb * dx + sb * dy), cross = -(cb * dy - sb * dx);
  const double pos = atan2(cross, dot) * inv_dg + half;
  const double fl = floor(pos);
  return {dx, dy, pos - fl, (int)fl};
}

// Feldkamp: the detector row a voxel at height z is seen at, between rows r0 and r0 + 1, `frac` of the way.  mag = SDD / L,
// the magnification of heights from the voxel to the cylindrical detector; rows at row_z0 + r / inv_rdz.
struct RowHit {
  double frac;
  int r0;
  __device__ __forceinline__ bool on_detector(int n_rows) const { return r0 >= 0 && r0 < n_rows - 1; }
};

__device__ __forceinline__ RowHit fdk_row(double z, double src_z, double mag, double row_z0, double inv_rdz) {
  const double rpos = (src_z + (z - src_z) * mag - row_z0) * inv_rdz;
  const double rfl = floor(rpos);
  return {rpos - rfl, (int)rfl};
}

// ---- host: the argument checks of the entry points, in the order they are made.  `own` = the caller's own pointers and
// counts are acceptable.

constexpr double kPi = 3.14159265358979323846;

// a scan over theta_tot < 2 pi has every ray at least once: pi + the full fan angle
inline bool short_scan_complete(double theta_tot, int n_channels, double dgamma) {
  return 0.5 * (theta_tot - kPi) >= 0.5 * (double)(n_channels - 1) * dgamma * (1.0 - 1e-12);
}

// dexct_fbp_backproject, dexct_fbp_var_backproject: grid z = rows
inline int check_fan_args(bool own, int n_views, int n_channels, int n_rows, int n_matrix, double sid, double dgamma, double fov) {
  if (!own || n_views <= 0 || n_channels < 2 || n_rows <= 0 || n_matrix <= 0) return DEXCT_EINVAL;
  if (n_rows > 65535 || (n_matrix + 3) / 4 > 65535) return DEXCT_ERANGE;
  if (!(sid > 0) || !(dgamma > 0) || !(fov > 0)) return DEXCT_EINVAL;
  return DEXCT_OK;
}

// dexct_fdk_backproject, dexct_fdk_var_backproject: grid z = slices / per_block (the fewest slices one block takes)
inline int check_cone_args(bool own, int n_views, int n_channels, int n_rows, int n_matrix, int n_slices, int per_block,
                           double sid, double sdd, double dgamma, double fov, double row_dz, double dz) {
  if (!own || n_views <= 0 || n_channels < 2 || n_rows < 2 || n_matrix <= 0 || n_slices <= 0) return DEXCT_EINVAL;
  if (!(sid > 0) || !(sdd >= sid) || !(dgamma > 0) || !(fov > 0) || !(row_dz > 0) || !(dz > 0)) return DEXCT_EINVAL;
  if ((n_slices + per_block - 1) / per_block > 65535 || (n_matrix + 3) / 4 > 65535) return DEXCT_ERANGE;
  return DEXCT_OK;
}

}  // namespace dexct
