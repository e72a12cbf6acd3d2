// What the two per-pixel K x M kernels share, gn_multi.hip (the Newton solve) and gn_cov.hip (its covariance): block size and
// workspace frame, the energy list of the tables kernels, the symmetric adjugate, the entry points' argument checks and the
// (K, M) dispatch (internal).  Each file keeps its own row layout (row_len), tables kernel, pixel kernel and launch.
#pragma once
#include <type_traits>

#include "common.h"
#include "exp_table.h"

namespace dexct {
namespace gnpix {

constexpr int kBlock = 256;
constexpr int kHeader = 16;                    // doubles: [0] = energies kept (as a double), the rest 0
constexpr int kMaxEnergies = 4096;

__host__ __device__ constexpr int n_sym(int M) { return M * (M + 1) / 2; }
// index of element (i, j), i <= j, in the row-major upper triangle
__host__ __device__ constexpr int sym(int M, int i, int j) { return i * M - i * (i - 1) / 2 + (j - i); }

// workspace: the header, n_e rows of row_len doubles, the list of kept energies (n_e ints)
inline size_t tables_bytes(int row_len, int n_e) {
  const size_t b = sizeof(double) * (kHeader + (size_t)n_e * row_len) + sizeof(int) * (size_t)n_e;
  return (b + 15) & ~(size_t)15;
}

// what the exported *_workspace_bytes return: 0 for a shape the entry point refuses
inline int64_t workspace_bytes(int n_meas, int n_mats, int n_energies, int (*row_len)(int, int)) {
  if (n_mats < 2 || n_mats > DEXCT_GN_MAX_MATS || n_meas < n_mats || n_meas > DEXCT_GN_MAX_MEAS) return 0;
  if (n_energies <= 0 || n_energies > kMaxEnergies) return 0;
  return (int64_t)tables_bytes(row_len(n_meas, n_mats), n_energies);
}

__device__ __forceinline__ double load_count(const void* p, int is_f64, int64_t i) {
  return is_f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

// One thread of the tables kernel: lists in perm the energies that some measurement weights - weighted(k * n_e + e) for a k; a
// zero weight contributes exactly 0 to every sum, the attenuation factor being finite thanks to the clip - and writes the
// workspace header.  Returns their number.
template <class Weighted>
__device__ __forceinline__ int list_energies(int K, int n_e, Weighted weighted, int* __restrict__ perm, double* __restrict__ ws) {
  int n = 0;
  for (int e = 0; e < n_e; ++e) {
    bool any = false;
    for (int k = 0; k < K; ++k) any = any || weighted((size_t)k * n_e + e);
    if (any) perm[n++] = e;
  }
  ws[0] = (double)n;
  for (int j = 1; j < kHeader; ++j) ws[j] = 0.0;
  return n;
}
// a weight that is not zero; NaN counts as a weight
__device__ __forceinline__ bool is_weight(double x) { return !(x == 0.0); }

// c[sym] = the adjugate of the symmetric matrix h[sym] (2 x 2 or 3 x 3); returns 1 / det h, so that h^-1 = c * (1 / det h).
// The two are left apart because the callers scale different things: gn_multi.hip the product (c dF), gn_cov.hip c itself.
// A singular or non-finite h gives inf / NaN, as IEEE arithmetic has it.
template <int M>
__device__ __forceinline__ double sym_adjugate(const double (&h)[n_sym(M)], double (&c)[n_sym(M)]) {
  static_assert(M == 2 || M == 3, "closed form for 2 x 2 and 3 x 3");
  if constexpr (M == 2) {
    const double h00 = h[0], h01 = h[1], h11 = h[2];
    c[0] = h11;
    c[1] = -h01;
    c[2] = h00;
    return exptab::rcp_f64(h00 * h11 - h01 * h01);
  } else {
    const double h00 = h[0], h01 = h[1], h02 = h[2], h11 = h[3], h12 = h[4], h22 = h[5];
    const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
    const double c11 = h00 * h22 - h02 * h02, c12 = h01 * h02 - h00 * h12, c22 = h00 * h11 - h01 * h01;
    c[0] = c00, c[1] = c01, c[2] = c02, c[3] = c11, c[4] = c12, c[5] = c22;
    return exptab::rcp_f64((h00 * c00 + h01 * c01) + h02 * c02);
  }
}

// The argument checks of dexct_gn_decompose_multi and dexct_gn_covariance, in the order both make them.  `first` and `then`
// are the caller's own conditions (true = acceptable) on either side of the K / M limits: pointers that must not be null
// and its own scalars first, what it asks after the limits then.  f64_a .. f64_c must be 8-byte aligned, `counts` (may be
// null) like its element type.
inline int check_args(bool first, int64_t n_pix, int n_meas, int n_mats, int n_energies, int counts_is_f64, bool then,
                      const void* counts, const void* f64_a, const void* f64_b, const void* f64_c) {
  if (!first || n_pix < 0 || n_energies <= 0) return DEXCT_EINVAL;
  if (counts_is_f64 != 0 && counts_is_f64 != 1) return DEXCT_EINVAL;
  if (n_meas < 2 || n_mats < 2 || n_mats > n_meas) return DEXCT_EINVAL;
  if (n_meas > DEXCT_GN_MAX_MEAS || n_mats > DEXCT_GN_MAX_MATS) return DEXCT_ERANGE;
  if (!then) return DEXCT_EINVAL;
  const uintptr_t f64s = reinterpret_cast<uintptr_t>(f64_a) | reinterpret_cast<uintptr_t>(f64_b) | reinterpret_cast<uintptr_t>(f64_c);
  if (f64s & 7u) return DEXCT_EINVAL;
  if (reinterpret_cast<uintptr_t>(counts) & (counts_is_f64 ? 7u : 3u)) return DEXCT_EINVAL;
  if (n_energies > kMaxEnergies) return DEXCT_ERANGE;
  if ((n_pix + kBlock - 1) / kBlock > 0x7FFFFFFFll) return DEXCT_ERANGE;
  return DEXCT_OK;
}

// The (K, M) shapes the kernels are instantiated for: launch(K, M) gets them as std::integral_constant.
template <class Launch>
int for_shape(int n_meas, int n_mats, Launch launch) {
  using std::integral_constant;
  if (n_meas == 2 && n_mats == 2) return launch(integral_constant<int, 2>{}, integral_constant<int, 2>{});
  if (n_meas == 3 && n_mats == 2) return launch(integral_constant<int, 3>{}, integral_constant<int, 2>{});
  if (n_meas == 4 && n_mats == 2) return launch(integral_constant<int, 4>{}, integral_constant<int, 2>{});
  if (n_meas == 3 && n_mats == 3) return launch(integral_constant<int, 3>{}, integral_constant<int, 3>{});
  if (n_meas == 4 && n_mats == 3) return launch(integral_constant<int, 4>{}, integral_constant<int, 3>{});
  return DEXCT_EINVAL;
}

}  // namespace gnpix
}  // namespace dexct
