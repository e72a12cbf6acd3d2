// Per-detector-pixel Newton basis-material decomposition for K = 2..4 measurements and M = 2..3 basis materials (gfx950).
//
// The general form of optimize_sino_cpu (matdecomp.py:87-127 of the reference): every pixel minimises the Poisson negative
// log-likelihood of its K counts over M thicknesses.  Per iteration it needs, for every measurement k, the sums over energy of
// {1, mu_m, mu_m mu_n (m <= n)} * i0_k(e) * exp(clip(-sum_m a_m mu_m(e), +-700)) - P = 1 + M + M(M+1)/2 sums per measurement -
// then the gradient dF, the full Newton Hessian incl. the (g/nu - 1) * hessian term (:122-123) and a closed-form symmetric
// M x M solve (:125).  Start 1e-6 (:98-99), fixed iteration count, float64 throughout, no damping: exactly the reference.
//
// Mapping: one lane per pixel, 256-thread blocks, all iterations in registers; the kernel is a template on <K, M> so that the
// K * P accumulators (12 .. 40 doubles) are named registers.  gn_multi_tables_kernel writes one row of M + K * P doubles per
// energy into the workspace - the scaled -mu_m, then per measurement the products with the reference's rounding of ssff / ssff2
// (:102, :105) - and the energy loop reads those rows at wave-uniform addresses: they arrive through the scalar cache and are
// SGPR operands of the v_fma_f64 that use them.  One exponential per energy serves all measurements; its only per-lane lookup
// is the 2048-entry 2^(j/2048) table in LDS (16 KB).  Like gn.hip the kernel is bound by the FP64 vector rate.
//
// Left out on purpose: the tolerance stop, the short cut tables, mixed precision, the run queue and the tile order of gn.hip
// (dexct_gn_decompose keeps all of them for K = M = 2), and channel-dependent spectra.
#include "gn_pixel.h"

namespace dexct {
namespace {

using namespace gnpix;
using exptab::exp_tab;
using exptab::kExpClip;
using exptab::kExpScale;
using exptab::kPowN;
using exptab::pow_entry;
using exptab::rcp_f64;

__host__ __device__ constexpr int n_products(int M) { return 1 + M + M * (M + 1) / 2; }
__host__ __device__ constexpr int row_len(int K, int M) { return M + K * n_products(M); }

// One block.  Thread 0 lists the energies at least one measurement weights (a zero weight contributes exactly 0 to every sum:
// the attenuation factor is finite thanks to the clip), the block then writes their rows.  Row of energy e:
//   [0 .. M)                     -mu_m(e) * 2048/ln2
//   per k, at M + k * P:         i0_k, i0_k mu_0 .. i0_k mu_(M-1), then i0_k (mu_m mu_n) for m <= n, row-major
__global__ __launch_bounds__(kBlock) void gn_multi_tables_kernel(const double* __restrict__ i0, const double* __restrict__ mus,
                                                                 int K, int M, int n_e, double* __restrict__ ws) {
  __shared__ int s_used;
  const int R = row_len(K, M), P = n_products(M);
  double* __restrict__ tab = ws + kHeader;
  int* __restrict__ perm = reinterpret_cast<int*>(tab + (size_t)n_e * R);
  if (threadIdx.x == 0) s_used = list_energies(K, n_e, [&](size_t i) { return is_weight(i0[i]); }, perm, ws);
  __syncthreads();
  const int n_used = s_used;
  for (int j = threadIdx.x; j < n_used; j += blockDim.x) {
    const int e = perm[j];
    double* __restrict__ t = tab + (size_t)j * R;
    double mu[DEXCT_GN_MAX_MATS];
    for (int m = 0; m < M; ++m) {
      mu[m] = mus[(size_t)m * n_e + e];
      t[m] = -mu[m] * kExpScale;
    }
    for (int k = 0; k < K; ++k) {
      const double w = i0[(size_t)k * n_e + e];
      double* __restrict__ tk = t + M + k * P;
      int c = 0;
      tk[c++] = w;
      for (int m = 0; m < M; ++m) tk[c++] = w * mu[m];
      for (int m = 0; m < M; ++m)
        for (int n = m; n < M; ++n) tk[c++] = w * (mu[m] * mu[n]);
    }
  }
}

// The Newton step from the sums acc[k][0 .. P): nu, G_m = sum i0 mu_m at, S_mn = sum i0 mu_m mu_n at.
//   c_k = g_k / nu_k - 1, q_k = g_k / nu_k^2;   dF_m = sum_k c_k G_km;   H_mn = sum_k (q_k G_km G_kn - c_k S_kmn);   a -= H^-1 dF
// (the signs of matdecomp.py:119, :122-123 multiplied out).  The solve is the closed form through the adjugate; a singular or
// non-finite H leaves inf / NaN, as IEEE arithmetic gives it.
template <int K, int M>
__device__ __forceinline__ void newton_solve(const double (&acc)[K][n_products(M)], const double (&g)[K], double (&a)[M]) {
  constexpr int NS = n_sym(M);
  double dF[M], H[NS];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double nu = acc[k][0];
    const double inv = rcp_f64(nu), ratio = g[k] * inv;
    // g / nu - 1 as (g - nu) / nu: near the solution the subtraction is exact (see gn.hip, newton_solve_f64); an overflowed
    // nu keeps the reference's value g / inf - 1 = -1
    const double c = fabs(nu) < __builtin_huge_val() ? (g[k] - nu) * inv : ratio - 1.0;
    const double q = ratio * inv;
    int s = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double Gm = acc[k][1 + m];
      dF[m] = k == 0 ? c * Gm : dF[m] + c * Gm;
#pragma unroll
      for (int n = m; n < M; ++n, ++s) {
        const double h = q * (Gm * acc[k][1 + n]) - c * acc[k][1 + M + s];
        H[s] = k == 0 ? h : H[s] + h;
      }
    }
  }
  double c[NS];
  const double inv_det = sym_adjugate<M>(H, c);
  if constexpr (M == 2) {
    const double d0 = (c[0] * dF[0] + c[1] * dF[1]) * inv_det;
    const double d1 = (c[2] * dF[1] + c[1] * dF[0]) * inv_det;
    a[0] -= d0;
    a[1] -= d1;
  } else {
    const double d0 = ((c[0] * dF[0] + c[1] * dF[1]) + c[2] * dF[2]) * inv_det;
    const double d1 = ((c[1] * dF[0] + c[3] * dF[1]) + c[4] * dF[2]) * inv_det;
    const double d2 = ((c[2] * dF[0] + c[4] * dF[1]) + c[5] * dF[2]) * inv_det;
    a[0] -= d0;
    a[1] -= d1;
    a[2] -= d2;
  }
}

template <int K, int M>
__global__ __launch_bounds__(kBlock) void gn_multi_kernel(const void* __restrict__ g, int g_is_f64, int64_t n_pix,
                                                          const double* __restrict__ ws, int n_iters,
                                                          const double* __restrict__ mask_max, double mask_frac, int full_loop,
                                                          double* __restrict__ out_a) {
  constexpr int P = n_products(M), R = row_len(K, M);
  __shared__ double lds_pow[kPowN];     // 2^(j/2048) in pow_entry's form, 16 KB
  // the loop of exptab::fill_pow_table, kept as text: the call compiles to another instruction order (tools/device_asm_diff.py)
  for (int j = threadIdx.x; j < kPowN; j += kBlock) lds_pow[j] = pow_entry(j);
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_pix) return;
  const int n_e = (int)ws[0];
  const double* __restrict__ tab = ws + kHeader;
  double gk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gk[k] = load_count(g, g_is_f64, (int64_t)k * n_pix + p);
  double* __restrict__ out = out_a + (int64_t)M * p;
  // the air mask of the reference's get_basismat_sinos (matdecomp.py:195-196, :204-205), from measurement 0
  if (mask_max && gk[0] >= mask_frac * mask_max[0]) {
#pragma unroll
    for (int m = 0; m < M; ++m) out[m] = 0.0;
    return;
  }
  double a[M];
#pragma unroll
  for (int m = 0; m < M; ++m) a[m] = 1e-6;
  for (int it = 0; it < n_iters; ++it) {
    double acc[K][P];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < P; ++c) acc[k][c] = 0.0;
#pragma unroll 2
    for (int e = 0; e < n_e; ++e) {
      const double* __restrict__ t = tab + (size_t)e * R;     // wave-uniform: scalar loads
      double y = a[0] * t[0];
#pragma unroll
      for (int m = 1; m < M; ++m) y = fma(a[m], t[m], y);
      y = fmin(fmax(y, -kExpClip), kExpClip);
      const double at = exp_tab(y, lds_pow);
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < P; ++c) acc[k][c] = fma(t[M + k * P + c], at, acc[k][c]);
    }
    double n[M];
#pragma unroll
    for (int m = 0; m < M; ++m) n[m] = a[m];
    newton_solve<K, M>(acc, gk, n);
    // The update is a pure function of the state: once it returns the state it was given, bit for bit in every component,
    // every later iterate is that state, and the loop may end without changing what n_iters iterations produce.
    bool same = true;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      same = same && __double_as_longlong(n[m]) == __double_as_longlong(a[m]);
      a[m] = n[m];
    }
    if (same && !full_loop) break;
  }
#pragma unroll
  for (int m = 0; m < M; ++m) out[m] = a[m];
}

template <int K, int M>
int launch(const void* g, int g_is_f64, int64_t n_pix, const double* ws, int n_iters, const double* mask_max, double mask_frac,
           int full_loop, double* out_a, hipStream_t st) {
  const int64_t nblk = (n_pix + kBlock - 1) / kBlock;
  hipLaunchKernelGGL((gn_multi_kernel<K, M>), dim3((unsigned)nblk), dim3(kBlock), 0, st, g, g_is_f64, n_pix, ws, n_iters,
                     mask_max, mask_frac, full_loop, out_a);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // namespace
}  // namespace dexct

using namespace dexct;

extern "C" {

int64_t dexct_gn_multi_workspace_bytes(int32_t n_meas, int32_t n_mats, int32_t n_energies) {
  return workspace_bytes(n_meas, n_mats, n_energies, row_len);
}

int dexct_gn_decompose_multi(const void* g, int32_t g_is_f64, int64_t n_pix, int32_t n_meas, int32_t n_mats, const double* i0,
                             const double* mus, int32_t n_energies, int32_t n_iters, const double* mask_max, double mask_frac,
                             int32_t flags, double* out_a, void* workspace, void* stream) {
  const int bad = check_args(g && i0 && mus && out_a && workspace && n_iters >= 1, n_pix, n_meas, n_mats, n_energies, g_is_f64,
                             !(flags & ~DEXCT_GN_MULTI_FULL_LOOP), g, out_a, workspace, nullptr);
  if (bad) return bad;
  if (n_pix == 0) return DEXCT_OK;
  hipStream_t st = as_stream(stream);
  double* ws = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(gn_multi_tables_kernel, dim3(1), dim3(kBlock), 0, st, i0, mus, n_meas, n_mats, n_energies, ws);
  DEXCT_LAUNCH_CHECK();
  const int full_loop = (flags & DEXCT_GN_MULTI_FULL_LOOP) ? 1 : 0;
  return for_shape(n_meas, n_mats, [&](auto K, auto M) {
    return launch<decltype(K)::value, decltype(M)::value>(g, g_is_f64, n_pix, ws, n_iters, mask_max, mask_frac, full_loop, out_a, st);
  });
}

}  // extern "C"
