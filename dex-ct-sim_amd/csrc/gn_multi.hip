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
#include "common.h"

namespace dexct {
namespace {

constexpr int kBlock = 256;
constexpr int kHeader = 16;                    // doubles: [0] = energies kept (as a double), the rest 0
constexpr int kMaxEnergies = 4096;

__host__ __device__ constexpr int n_products(int M) { return 1 + M + M * (M + 1) / 2; }
__host__ __device__ constexpr int row_len(int K, int M) { return M + K * n_products(M); }

inline size_t tables_bytes(int K, int M, int n_e) {
  const size_t b = sizeof(double) * (kHeader + (size_t)n_e * row_len(K, M)) + sizeof(int) * (size_t)n_e;
  return (b + 15) & ~(size_t)15;
}

// ---- the table exponential and the reciprocal of gn.hip (a private copy: the kernels there are not touched) ----------
// exp(x) for |x| <= 700, given y = x * 2048/ln2: y = n + f with n = rint(y) = 2048 k + j, |f| <= 1/2, and
// exp(x) = 2^k * 2^(j/2048) * e^(f ln2/2048), a cubic in f for e^r - 1 (truncation r^4/24 < 4e-17, r = f ln2/2048).
// n comes out of the low mantissa bits of y + 1.5 * 2^52 (round to nearest even, like rint); f = y - n is exact.  The table
// entry j holds 2^(j/2048) with j << 9 subtracted from its high word, so that adding n << 9 = (k << 20) + (j << 9) to the high
// word of what was loaded gives 2^k 2^(j/2048) before the last FMA.  About 1 ulp; NaN stays NaN.
constexpr int kPowBits = 11;
constexpr int kPowN = 1 << kPowBits;
constexpr double kExpScale = 0x1.71547652b82fep+11;          // 2048 / ln 2
constexpr double kExpClip = 700.0 * kExpScale;               // the reference's clip of the exponent (matdecomp.py:116)
__device__ __forceinline__ double pow_entry(int j) {
  const double v = exp2((double)j * (1.0 / kPowN));
  return __hiloint2double(__double2hiint(v) - (j << (20 - kPowBits)), __double2loint(v));
}
__device__ __forceinline__ double exp_tab(double y, const double* __restrict__ lds_pow) {
  const double kMagic = 6755399441055744.0;   // 1.5 * 2^52
  constexpr double c1 = 0x1.62e42fefa39efp-12;               // ln2 / 2048
  constexpr double c2 = c1 * c1 / 2.0, c3 = c1 * c1 * c1 / 6.0;
  const double tm = y + kMagic;
  const int ni = __double2loint(tm);
  const double f = y - (tm - kMagic);
  double q = fma(f, c3, c2);
  q = fma(f, q, c1);
  const double p = f * q;
  const double tr = lds_pow[ni & (kPowN - 1)];
  const double tj = __hiloint2double((int)((unsigned)__double2hiint(tr) + ((unsigned)ni << (20 - kPowBits))), __double2loint(tr));
  return fma(tj, p, tj);
}

// 1 / x by v_rcp_f64 and two Newton refinements; for x = 0, +-inf or NaN the hardware's answer (inf, 0, NaN - what IEEE
// division gives) is kept, so an overflowed sum behaves as in the reference (g / inf = 0).
__device__ __forceinline__ double rcp_f64(double x) {
  const double r0 = __builtin_amdgcn_rcp(x);
  double r = fma(r0, fma(-x, r0, 1.0), r0);
  r = fma(r, fma(-x, r, 1.0), r);
  const double ax = fabs(x);
  return (ax > 0.0 && ax < __builtin_huge_val()) ? r : r0;
}

__device__ __forceinline__ double load_count(const void* p, int is_f64, int64_t i) {
  return is_f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

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
  if (threadIdx.x == 0) {
    int n = 0;
    for (int e = 0; e < n_e; ++e) {
      bool any = false;
      for (int k = 0; k < K; ++k) any = any || !(i0[(size_t)k * n_e + e] == 0.0);      // NaN counts as a weight
      if (any) perm[n++] = e;
    }
    s_used = n;
    ws[0] = (double)n;
    for (int j = 1; j < kHeader; ++j) ws[j] = 0.0;
  }
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
  constexpr int NS = M * (M + 1) / 2;
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
  if constexpr (M == 2) {
    const double h00 = H[0], h01 = H[1], h11 = H[2];
    const double inv_det = rcp_f64(h00 * h11 - h01 * h01);
    const double d0 = (h11 * dF[0] - h01 * dF[1]) * inv_det;
    const double d1 = (h00 * dF[1] - h01 * dF[0]) * inv_det;
    a[0] -= d0;
    a[1] -= d1;
  } else {
    const double h00 = H[0], h01 = H[1], h02 = H[2], h11 = H[3], h12 = H[4], h22 = H[5];
    const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
    const double c11 = h00 * h22 - h02 * h02, c12 = h01 * h02 - h00 * h12, c22 = h00 * h11 - h01 * h01;
    const double inv_det = rcp_f64((h00 * c00 + h01 * c01) + h02 * c02);
    const double d0 = ((c00 * dF[0] + c01 * dF[1]) + c02 * dF[2]) * inv_det;
    const double d1 = ((c01 * dF[0] + c11 * dF[1]) + c12 * dF[2]) * inv_det;
    const double d2 = ((c02 * dF[0] + c12 * dF[1]) + c22 * dF[2]) * inv_det;
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
  if (n_mats < 2 || n_mats > DEXCT_GN_MAX_MATS || n_meas < n_mats || n_meas > DEXCT_GN_MAX_MEAS) return 0;
  if (n_energies <= 0 || n_energies > kMaxEnergies) return 0;
  return (int64_t)tables_bytes(n_meas, n_mats, n_energies);
}

int dexct_gn_decompose_multi(const void* g, int32_t g_is_f64, int64_t n_pix, int32_t n_meas, int32_t n_mats, const double* i0,
                             const double* mus, int32_t n_energies, int32_t n_iters, const double* mask_max, double mask_frac,
                             int32_t flags, double* out_a, void* workspace, void* stream) {
  if (!g || !i0 || !mus || !out_a || !workspace) return DEXCT_EINVAL;
  if (n_pix < 0 || n_energies <= 0 || n_iters < 1) return DEXCT_EINVAL;
  if (g_is_f64 != 0 && g_is_f64 != 1) return DEXCT_EINVAL;
  if (n_meas < 2 || n_mats < 2 || n_mats > n_meas) return DEXCT_EINVAL;
  if (n_meas > DEXCT_GN_MAX_MEAS || n_mats > DEXCT_GN_MAX_MATS) return DEXCT_ERANGE;
  if (flags & ~DEXCT_GN_MULTI_FULL_LOOP) return DEXCT_EINVAL;
  if (reinterpret_cast<uintptr_t>(out_a) & 7u) return DEXCT_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return DEXCT_EINVAL;
  if (reinterpret_cast<uintptr_t>(g) & (g_is_f64 ? 7u : 3u)) return DEXCT_EINVAL;
  if (n_energies > kMaxEnergies) return DEXCT_ERANGE;
  const int64_t nblk = (n_pix + kBlock - 1) / kBlock;
  if (nblk > 0x7FFFFFFFll) return DEXCT_ERANGE;
  if (n_pix == 0) return DEXCT_OK;
  hipStream_t st = as_stream(stream);
  double* ws = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(gn_multi_tables_kernel, dim3(1), dim3(kBlock), 0, st, i0, mus, n_meas, n_mats, n_energies, ws);
  DEXCT_LAUNCH_CHECK();
  const int full_loop = (flags & DEXCT_GN_MULTI_FULL_LOOP) ? 1 : 0;
#define DEXCT_GN_MULTI_CASE(K, M) \
  if (n_meas == K && n_mats == M) return launch<K, M>(g, g_is_f64, n_pix, ws, n_iters, mask_max, mask_frac, full_loop, out_a, st)
  DEXCT_GN_MULTI_CASE(2, 2);
  DEXCT_GN_MULTI_CASE(3, 2);
  DEXCT_GN_MULTI_CASE(4, 2);
  DEXCT_GN_MULTI_CASE(3, 3);
  DEXCT_GN_MULTI_CASE(4, 3);
#undef DEXCT_GN_MULTI_CASE
  return DEXCT_EINVAL;
}

}  // extern "C"
