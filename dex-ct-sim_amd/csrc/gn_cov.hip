// Per-detector-pixel noise covariance of the basis-material decomposition, K = 2..4 measurements, M = 2..3 materials (gfx950).
//
// For the state a[M] of a pixel (what dexct_gn_decompose / dexct_gn_decompose_multi returned, or a noise-free truth), with
// t_e = exp(clip(-sum_m a_m mu_m(e), +-700)):
//   nu_k = sum_e i0_k(e) t_e      expected counts
//   v_k  = sum_e i0v_k(e) t_e     their variance (i0v = i0 x E for an energy-integrating detector, i0 for a counting one)
//   G_km = sum_e i0_k(e) mu_m(e) t_e = -d nu_k / d a_m
// and the covariance of the estimated a is
//   estimator:  C = H^-1 (G^T diag(v / nu^2) G) H^-1,  H = G^T diag(1 / nu) G     (delta method on the Poisson-likelihood Newton
//                                                                                 solve of gn_multi.hip, whose fixed point
//                                                                                 solves G^T diag(1/nu) (g - nu) = 0)
//   crlb:       C = (G^T diag(1 / v) G)^-1                                        (Cramer-Rao bound for Gaussian data of
//                                                                                 variance v)
// They coincide for K = M and for i0v = i0.  The inverse is closed form (2 x 2, or the 3 x 3 adjugate as in gn_multi.hip).
//
// Mapping (that of gn_multi.hip): one lane per pixel, 256-thread blocks, one launch; the kernel is a template on <K, M, KIND> so
// that the K (M + 2) <= 20 accumulators are named registers.  gn_cov_tables_kernel writes one row of M + K (M + 2) doubles per
// weighted energy into the workspace - the scaled -mu_m, then per measurement i0_k, i0v_k, i0_k mu_m - and the energy loop reads
// the rows at wave-uniform addresses: scalar loads whose results are SGPR operands of the v_fma_f64.  One table exponential per
// energy serves every accumulator.  float64 throughout: the correlation matrix of a three-material covariance has a condition
// number of 1e3 .. 1e5, which a float32 exponential would turn into 1e-3 .. 1e-2 of the result.
//
// dexct_cov_quadform is the element-wise u^T C_p u: the variance of the VMI line integral sum_m u_m a_m.
#include "gn_pixel.h"

namespace dexct {
namespace {

using namespace gnpix;
using exptab::exp_tab;
using exptab::kExpClip;
using exptab::kExpScale;
using exptab::kPowN;
using exptab::rcp_f64;

__host__ __device__ constexpr int per_meas(int M) { return M + 2; }
__host__ __device__ constexpr int row_len(int K, int M) { return M + K * per_meas(M); }

// One block.  Thread 0 lists the energies that some measurement weights in i0 or i0v (a zero weight contributes exactly 0 to
// every sum: the attenuation factor is finite thanks to the clip), the block then writes their rows.  Row of energy e:
//   [0 .. M)                      -mu_m(e) * 2048/ln2
//   per k, at M + k * (M + 2):    i0_k, i0v_k, i0_k mu_0 .. i0_k mu_(M-1)
__global__ __launch_bounds__(kBlock) void gn_cov_tables_kernel(const double* __restrict__ i0, const double* __restrict__ i0v,
                                                               const double* __restrict__ mus, int K, int M, int n_e,
                                                               double* __restrict__ ws) {
  __shared__ int s_used;
  const int R = row_len(K, M), P = per_meas(M);
  double* __restrict__ tab = ws + kHeader;
  int* __restrict__ perm = reinterpret_cast<int*>(tab + (size_t)n_e * R);
  if (threadIdx.x == 0)
    s_used = list_energies(K, n_e, [&](size_t i) { return is_weight(i0[i]) || is_weight(i0v[i]); }, perm, ws);
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
      tk[0] = w;
      tk[1] = i0v[(size_t)k * n_e + e];
      for (int m = 0; m < M; ++m) tk[2 + m] = w * mu[m];
    }
  }
}

// inv[sym] = the inverse of the symmetric matrix h[sym], closed form; a singular or non-finite h leaves inf / NaN
template <int M>
__device__ __forceinline__ void sym_inverse(const double (&h)[n_sym(M)], double (&inv)[n_sym(M)]) {
  double c[n_sym(M)];
  const double inv_det = sym_adjugate<M>(h, c);
#pragma unroll
  for (int t = 0; t < n_sym(M); ++t) inv[t] = c[t] * inv_det;
}

// out[sym] = sum_k w_k G_km G_kn for m <= n; G_km = acc[k][2 + m]
template <int K, int M>
__device__ __forceinline__ void weighted_gram(const double (&acc)[K][per_meas(M)], const double (&w)[K], double (&out)[n_sym(M)]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int s = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double wg = w[k] * acc[k][2 + m];
#pragma unroll
      for (int n = m; n < M; ++n, ++s) {
        const double h = wg * acc[k][2 + n];
        out[s] = k == 0 ? h : out[s] + h;
      }
    }
  }
}

template <int K, int M, int KIND>
__global__ __launch_bounds__(kBlock) void gn_cov_kernel(const double* __restrict__ a_in, int64_t n_pix, const double* __restrict__ ws,
                                                        const void* __restrict__ mask_g, int g_is_f64,
                                                        const double* __restrict__ mask_max, double mask_frac,
                                                        double* __restrict__ out_cov) {
  constexpr int P = per_meas(M), R = row_len(K, M), T = n_sym(M);
  __shared__ double lds_pow[kPowN];     // 2^(j/2048) in pow_entry's form, 16 KB
  exptab::fill_pow_table<kBlock>(lds_pow);
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_pix) return;
  double* __restrict__ out = out_cov + (int64_t)T * p;
  // the air mask of dexct_gn_decompose_multi, from the counts of measurement 0
  if (mask_g && load_count(mask_g, g_is_f64, p) >= mask_frac * mask_max[0]) {
#pragma unroll
    for (int t = 0; t < T; ++t) out[t] = 0.0;
    return;
  }
  const int n_e = (int)ws[0];
  const double* __restrict__ tab = ws + kHeader;
  double a[M];
#pragma unroll
  for (int m = 0; m < M; ++m) a[m] = a_in[(int64_t)M * p + m];
  double acc[K][P];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int c = 0; c < P; ++c) acc[k][c] = 0.0;
  bool is_nan = false;
#pragma unroll 2
  for (int e = 0; e < n_e; ++e) {
    const double* __restrict__ t = tab + (size_t)e * R;     // wave-uniform: scalar loads
    double y = a[0] * t[0];
#pragma unroll
    for (int m = 1; m < M; ++m) y = fma(a[m], t[m], y);
    // The hardware's max / min return their other operand for a NaN one, so a NaN exponent - a NaN component of the state or of
    // the tables, infinite components of opposite sign, an infinite component against mu = 0 - would be clipped like a large
    // one: it is noted here and the pixel made NaN below, as NumPy's clip keeps it.
    is_nan = is_nan || y != y;
    y = fmin(fmax(y, -kExpClip), kExpClip);
    const double at = exp_tab(y, lds_pow);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < P; ++c) acc[k][c] = fma(t[M + k * P + c], at, acc[k][c]);
  }

  double C[T];
  if constexpr (KIND == DEXCT_COV_CRLB) {
    double w[K], F[T];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = rcp_f64(acc[k][1]);
    weighted_gram<K, M>(acc, w, F);
    sym_inverse<M>(F, C);
  } else {
    double w[K], s[K], H[T], B[T], Hi[T];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      w[k] = rcp_f64(acc[k][0]);
      s[k] = (acc[k][1] * w[k]) * w[k];
    }
    weighted_gram<K, M>(acc, w, H);
    weighted_gram<K, M>(acc, s, B);
    sym_inverse<M>(H, Hi);
    // X = B Hi (full), then C = Hi X, upper triangle
    double X[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        double x = 0.0;
#pragma unroll
        for (int l = 0; l < M; ++l) {
          const double b = B[i <= l ? sym(M, i, l) : sym(M, l, i)], h = Hi[l <= j ? sym(M, l, j) : sym(M, j, l)];
          x = l == 0 ? b * h : x + b * h;
        }
        X[i][j] = x;
      }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = i; j < M; ++j) {
        double c = 0.0;
#pragma unroll
        for (int l = 0; l < M; ++l) {
          const double h = Hi[i <= l ? sym(M, i, l) : sym(M, l, i)];
          c = l == 0 ? h * X[l][j] : c + h * X[l][j];
        }
        C[sym(M, i, j)] = c;
      }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) out[t] = is_nan ? __builtin_nan("") : C[t];
}

struct QuadVec {
  double u[DEXCT_GN_MAX_MATS];
};

// out[p] = u^T C_p u = sum_i u_i^2 C_ii + 2 sum_(i<j) u_i u_j C_ij, summed in the order of the packed triangle
template <int M>
__global__ __launch_bounds__(kBlock) void cov_quadform_kernel(const double* __restrict__ cov, int64_t n_pix, QuadVec q,
                                                              double* __restrict__ out) {
  constexpr int T = n_sym(M);
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_pix) return;
  const double* __restrict__ c = cov + (int64_t)T * p;
  double r = 0.0;
  int s = 0;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i; j < M; ++j, ++s) {
      const double w = i == j ? q.u[i] * q.u[i] : 2.0 * (q.u[i] * q.u[j]);
      r = s == 0 ? w * c[s] : r + w * c[s];
    }
  out[p] = r;
}

template <int K, int M>
int launch(int kind, const double* a, int64_t n_pix, const double* ws, const void* mask_g, int g_is_f64, const double* mask_max,
           double mask_frac, double* out_cov, hipStream_t st) {
  const int64_t nblk = (n_pix + kBlock - 1) / kBlock;
  if (kind == DEXCT_COV_CRLB)
    hipLaunchKernelGGL((gn_cov_kernel<K, M, DEXCT_COV_CRLB>), dim3((unsigned)nblk), dim3(kBlock), 0, st, a, n_pix, ws, mask_g,
                       g_is_f64, mask_max, mask_frac, out_cov);
  else
    hipLaunchKernelGGL((gn_cov_kernel<K, M, DEXCT_COV_ESTIMATOR>), dim3((unsigned)nblk), dim3(kBlock), 0, st, a, n_pix, ws, mask_g,
                       g_is_f64, mask_max, mask_frac, out_cov);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // namespace
}  // namespace dexct

using namespace dexct;

extern "C" {

int64_t dexct_gn_cov_workspace_bytes(int32_t n_meas, int32_t n_mats, int32_t n_energies) {
  return workspace_bytes(n_meas, n_mats, n_energies, row_len);
}

int dexct_gn_covariance(const double* a, int64_t n_pix, int32_t n_meas, int32_t n_mats, const double* i0, const double* i0v,
                        const double* mus, int32_t n_energies, int32_t kind, const void* mask_g, int32_t g_is_f64,
                        const double* mask_max, double mask_frac, double* out_cov, void* workspace, void* stream) {
  const bool kind_ok = kind == DEXCT_COV_ESTIMATOR || kind == DEXCT_COV_CRLB;
  const int bad = check_args(a && i0 && i0v && mus && out_cov && workspace && kind_ok, n_pix, n_meas, n_mats, n_energies, g_is_f64,
                             !(mask_g && !mask_max), mask_g, a, out_cov, workspace);
  if (bad) return bad;
  if (n_pix == 0) return DEXCT_OK;
  hipStream_t st = as_stream(stream);
  double* ws = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(gn_cov_tables_kernel, dim3(1), dim3(kBlock), 0, st, i0, i0v, mus, n_meas, n_mats, n_energies, ws);
  DEXCT_LAUNCH_CHECK();
  return for_shape(n_meas, n_mats, [&](auto K, auto M) {
    return launch<decltype(K)::value, decltype(M)::value>(kind, a, n_pix, ws, mask_g, g_is_f64, mask_max, mask_frac, out_cov, st);
  });
}

int dexct_cov_quadform(const double* cov, int64_t n_pix, int32_t n_mats, const double* u, double* out, void* stream) {
  if (!cov || !u || !out) return DEXCT_EINVAL;
  if (n_pix < 0 || n_mats < 2) return DEXCT_EINVAL;
  if (n_mats > DEXCT_GN_MAX_MATS) return DEXCT_ERANGE;
  if ((reinterpret_cast<uintptr_t>(cov) | reinterpret_cast<uintptr_t>(out)) & 7u) return DEXCT_EINVAL;
  const int64_t nblk = (n_pix + kBlock - 1) / kBlock;
  if (nblk > 0x7FFFFFFFll) return DEXCT_ERANGE;
  if (n_pix == 0) return DEXCT_OK;
  QuadVec q;
  for (int m = 0; m < DEXCT_GN_MAX_MATS; ++m) q.u[m] = m < n_mats ? u[m] : 0.0;
  hipStream_t st = as_stream(stream);
  if (n_mats == 2)
    hipLaunchKernelGGL(cov_quadform_kernel<2>, dim3((unsigned)nblk), dim3(kBlock), 0, st, cov, n_pix, q, out);
  else
    hipLaunchKernelGGL(cov_quadform_kernel<3>, dim3((unsigned)nblk), dim3(kBlock), 0, st, cov, n_pix, q, out);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // extern "C"
