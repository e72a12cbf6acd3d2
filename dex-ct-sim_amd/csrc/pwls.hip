// The element-wise and stencil steps of the joint penalised weighted least-squares reconstruction (dex-ct-sim_amd/iterative.py,
// pwls): K = 1 .. 3 channels (basis-material sinograms and images) coupled by one symmetric K x K weight matrix per ray.
//   cov_precision_kernel   the packed float64 covariance of a ray -> its inverse in float32, plane-major
//   pwls_majorizer_kernel  m_k = (sum_l |w_kl|) R: what the adjoint turns into the diagonal majoriser d_k
//   pwls_residual_kernel   q_k = sum_l w_kl (ax_l - b_l) over the lines of a subset, and 1/2 sum r^T W r
//   pwls_update_kernel     the separable-surrogate step with the Huber penalty of the in-plane 4-neighbourhood (Jacobi: it
//                          reads the old images and writes the new ones)
// The projections in between are the matched pair of iterative.hip.  Symmetric matrices are packed as the row-major upper
// triangle (tri below), the layout of dexct_gn_covariance.  Every kernel is memory bound: a thread handles V = 4 neighbouring
// elements with 16-byte loads and stores where pointers and strides allow, one element otherwise; the two objective sums go
// through a wave reduction to one float64 atomic per workgroup, as in sirt_residual_kernel.
#include "common.h"

#include <cmath>

namespace dexct {

// index of element (k, l) of a symmetric K x K matrix in its packed upper triangle
__host__ __device__ constexpr int tri(int K, int k, int l) {
  return k <= l ? k * K - k * (k - 1) / 2 + (l - k) : l * K - l * (l - 1) / 2 + (k - l);
}

template <int V>
struct Vec {
  float v[V];
};

template <int V>
__device__ __forceinline__ Vec<V> load_vec(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void store_vec(float* p, const Vec<V>& r) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else *p = r.v[0];
}

// sum over the workgroup, then one atomic (none for a zero partial: a consistent problem keeps an exact 0)
__device__ __forceinline__ void block_add(double acc, double* out) {
  __shared__ double part[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = (part[0] + part[1]) + (part[2] + part[3]);
    if (s != 0.0) atomicAdd(out, s);
  }
}

template <int K>
__global__ __launch_bounds__(256) void cov_precision_kernel(const double* __restrict__ cov, int64_t n, float fill,
                                                            float* __restrict__ w) {
  constexpr int T = K * (K + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    double c[T], inv[T];
    bool ok = true;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      c[t] = cov[T * p + t];
      ok = ok && std::isfinite(c[t]);
    }
    // usable: every leading principal minor is positive (and finite); the inverse is the adjugate over the determinant
    if constexpr (K == 1) {
      ok = ok && c[0] > 0.0;
      inv[0] = 1.0 / c[0];
    } else if constexpr (K == 2) {
      const double det = c[0] * c[2] - c[1] * c[1];
      ok = ok && c[0] > 0.0 && det > 0.0 && std::isfinite(det);
      inv[0] = c[2] / det;
      inv[1] = -c[1] / det;
      inv[2] = c[0] / det;
    } else {
      const double a = c[0], b = c[1], cc = c[2], d = c[3], e = c[4], f = c[5];
      const double C00 = d * f - e * e, C01 = cc * e - b * f, C02 = b * e - cc * d;
      const double C11 = a * f - cc * cc, C12 = b * cc - a * e, C22 = a * d - b * b;
      const double det = (a * C00 + b * C01) + cc * C02;
      ok = ok && a > 0.0 && C22 > 0.0 && det > 0.0 && std::isfinite(det);
      inv[0] = C00 / det; inv[1] = C01 / det; inv[2] = C02 / det;
      inv[3] = C11 / det; inv[4] = C12 / det; inv[5] = C22 / det;
    }
    // ... and the inverse must survive the rounding: a variance below the float32 range would weigh inf and turn the
    // residual into NaN
    float r[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      r[t] = (float)inv[t];
      ok = ok && std::isfinite(r[t]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int l = k; l < K; ++l) {
        const int t = tri(K, k, l);
        w[(int64_t)t * n + p] = ok ? r[t] : (k == l ? fill : 0.0f);
      }
  }
}

template <int K, int V>
__global__ __launch_bounds__(256) void pwls_majorizer_kernel(const float* __restrict__ w, const float* __restrict__ row_sum,
                                                             int64_t n, float* __restrict__ m) {
  constexpr int T = K * (K + 1) / 2;
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i * V;
    const Vec<V> R = load_vec<V>(row_sum + p);
    Vec<V> a[T];
#pragma unroll
    for (int t = 0; t < T; ++t) a[t] = load_vec<V>(w + (int64_t)t * n + p);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      Vec<V> out;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float s = fabsf(a[tri(K, k, 0)].v[e]);
#pragma unroll
        for (int l = 1; l < K; ++l) s += fabsf(a[tri(K, k, l)].v[e]);
        out.v[e] = s * R.v[e];
      }
      store_vec<V>(m + (int64_t)k * n + p, out);
    }
  }
}

// element (j, e) of the subset: line j * step of every plane, e < line; V divides line, step * line and plane.  q may be ax:
// a thread reads its K values of ax before it writes its K values of q, and no other thread touches them.
template <int K, int V>
__global__ __launch_bounds__(256) void pwls_residual_kernel(const float* __restrict__ b, const float* ax,
                                                            const float* __restrict__ w, const float* __restrict__ row_sum,
                                                            int64_t plane, int64_t n_sub, int64_t step, int64_t line, float* q,
                                                            double* objective) {
  constexpr int T = K * (K + 1) / 2;
  const int64_t lv = line / V, total = n_sub * lv;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t j = i / lv;
    const int64_t o = j * step * line + (i - j * lv) * V;
    const Vec<V> R = load_vec<V>(row_sum + o);
    Vec<V> bb[K], aa[K], ww[T];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      bb[k] = load_vec<V>(b + (int64_t)k * plane + o);
      aa[k] = load_vec<V>(ax + (int64_t)k * plane + o);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) ww[t] = load_vec<V>(w + (int64_t)t * plane + o);
    if (q) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        Vec<V> out;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          float s = ww[tri(K, k, 0)].v[e] * (aa[0].v[e] - bb[0].v[e]);
#pragma unroll
          for (int l = 1; l < K; ++l) s += ww[tri(K, k, l)].v[e] * (aa[l].v[e] - bb[l].v[e]);
          out.v[e] = R.v[e] > 0.0f ? s : 0.0f;               // a ray with R = 0 has missed the grid
        }
        store_vec<V>(q + (int64_t)k * plane + o, out);
      }
    }
    if (objective) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (!(R.v[e] > 0.0f)) continue;
        double r[K], s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = (double)aa[k].v[e] - (double)bb[k].v[e];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          s += (double)ww[tri(K, k, k)].v[e] * r[k] * r[k];
#pragma unroll
          for (int l = k + 1; l < K; ++l) s += 2.0 * ((double)ww[tri(K, k, l)].v[e] * r[k] * r[l]);
        }
        acc += 0.5 * s;
      }
    }
  }
  if (objective) block_add(acc, objective);
}

struct PwlsPenalty {
  float beta[3], delta[3];
};

__device__ __forceinline__ double huber(double t, double delta) {
  const double a = fabs(t);
  return a <= delta ? 0.5 * t * t : delta * a - 0.5 * delta * delta;
}

// One thread per pixel j of the nz * ny * nx grid with its K channels (plane k of x_old, g, d, x_new); lanes along x, so
// the loads of the centre, of the left / right neighbours and of the rows above and below, and the store, are contiguous.
template <int K>
__global__ __launch_bounds__(256) void pwls_update_kernel(const float* __restrict__ x_old, const float* __restrict__ g,
                                                          const float* __restrict__ d, int64_t n, int nx, int ny,
                                                          PwlsPenalty pen, float g_scale, int nonneg,
                                                          float* __restrict__ x_new, double* penalty) {
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int ix = (int)(j % nx), iy = (int)((j / nx) % ny);
    const bool has[4] = {ix > 0, ix + 1 < nx, iy > 0, iy + 1 < ny};          // left, right, up, down
    const int64_t at[4] = {j - 1, j + 1, j - nx, j + nx};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* __restrict__ xk = x_old + (int64_t)k * n;
      const float beta = pen.beta[k], delta = pen.delta[k];
      const float x = xk[j];
      float sp = 0.0f, sc = 0.0f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (!has[m]) continue;
        const float t = x - xk[at[m]];
        const float a = fabsf(t);
        sp += fminf(fmaxf(t, -delta), delta);
        sc += a > delta ? delta / a : 1.0f;
        if (penalty && (m & 1)) acc += (double)beta * huber((double)x - (double)xk[at[m]], (double)delta);   // right, down
      }
      const float den = d[(int64_t)k * n + j] + (2.0f * beta) * sc;
      float v = x;
      if (den > 0.0f) v = x - (g_scale * g[(int64_t)k * n + j] + beta * sp) / den;     // other pixels stay as they are
      if (nonneg) v = fmaxf(v, 0.0f);
      x_new[(int64_t)k * n + j] = v;
    }
  }
  if (penalty) block_add(acc, penalty);
}

// the grid cap of every kernel here; tests/grid_caps.py holds its value, tests/test_gpu_grid_passes.py runs past it
constexpr int kPwlsMaxBlocks = 4096;

static int64_t pwls_blocks(int64_t n) {
  int64_t nb = (n + 255) / 256;
  return nb < 1 ? 1 : (nb > kPwlsMaxBlocks ? kPwlsMaxBlocks : nb);
}

constexpr int64_t kPwlsMaxElems = (int64_t)1 << 40;   // per plane: keeps every byte offset far inside int64

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static bool overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(float);
  return pa < pb + len && pb < pa + len;
}

}  // namespace dexct

using namespace dexct;

#define PWLS_BY_K(K_, CALL)        \
  switch (K_) {                    \
    case 1: { constexpr int KK = 1; CALL; } break; \
    case 2: { constexpr int KK = 2; CALL; } break; \
    default: { constexpr int KK = 3; CALL; } break; \
  }

extern "C" {

int dexct_cov_precision(const double* cov, int64_t n, int32_t n_mats, double w_fill, float* w, void* stream) {
  if (!cov || !w || n < 0 || n_mats < 1 || n_mats > 3 || !(w_fill >= 0.0) || !std::isfinite(w_fill)) return DEXCT_EINVAL;
  if (n > kPwlsMaxElems) return DEXCT_ERANGE;
  if (n == 0) return DEXCT_OK;
  const dim3 grid((unsigned)pwls_blocks(n));
  PWLS_BY_K(n_mats, hipLaunchKernelGGL(cov_precision_kernel<KK>, grid, dim3(256), 0, as_stream(stream), cov, n, (float)w_fill, w));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_pwls_majorizer(const float* w, const float* row_sum, int64_t n, int32_t n_mats, float* m, void* stream) {
  if (!w || !row_sum || !m || n < 0 || n_mats < 1 || n_mats > 3) return DEXCT_EINVAL;
  if (n > kPwlsMaxElems) return DEXCT_ERANGE;
  if (n == 0) return DEXCT_OK;
  hipStream_t st = as_stream(stream);
  if (n % 4 == 0 && aligned16(w) && aligned16(row_sum) && aligned16(m)) {
    const dim3 grid((unsigned)pwls_blocks(n / 4));
    PWLS_BY_K(n_mats, hipLaunchKernelGGL((pwls_majorizer_kernel<KK, 4>), grid, dim3(256), 0, st, w, row_sum, n, m));
  } else {
    const dim3 grid((unsigned)pwls_blocks(n));
    PWLS_BY_K(n_mats, hipLaunchKernelGGL((pwls_majorizer_kernel<KK, 1>), grid, dim3(256), 0, st, w, row_sum, n, m));
  }
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_pwls_residual(const float* b, const float* ax, const float* w, const float* row_sum, int64_t plane, int32_t n_mats,
                        int32_t n_lines, int32_t line_step, int64_t line, float* q, double* objective, void* stream) {
  if (!b || !ax || !w || !row_sum || (!q && !objective) || n_mats < 1 || n_mats > 3) return DEXCT_EINVAL;
  if (n_lines <= 0 || line_step < 1 || line <= 0 || plane < (int64_t)n_lines * line) return DEXCT_EINVAL;
  if (plane > kPwlsMaxElems) return DEXCT_ERANGE;
  hipStream_t st = as_stream(stream);
  if (objective) DEXCT_HIP_TRY(hipMemsetAsync(objective, 0, sizeof(double), st));
  const int64_t n_sub = (n_lines + line_step - 1) / line_step;
  const bool wide = line % 4 == 0 && plane % 4 == 0 && aligned16(b) && aligned16(ax) && aligned16(w) && aligned16(row_sum) &&
                    (!q || aligned16(q));
  if (wide) {
    const dim3 grid((unsigned)pwls_blocks(n_sub * (line / 4)));
    PWLS_BY_K(n_mats, hipLaunchKernelGGL((pwls_residual_kernel<KK, 4>), grid, dim3(256), 0, st, b, ax, w, row_sum, plane, n_sub,
                                         (int64_t)line_step, line, q, objective));
  } else {
    const dim3 grid((unsigned)pwls_blocks(n_sub * line));
    PWLS_BY_K(n_mats, hipLaunchKernelGGL((pwls_residual_kernel<KK, 1>), grid, dim3(256), 0, st, b, ax, w, row_sum, plane, n_sub,
                                         (int64_t)line_step, line, q, objective));
  }
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_pwls_update(const float* x_old, const float* g, const float* d, int32_t n_mats, int32_t nz, int32_t ny, int32_t nx,
                      double g_scale, const double* beta, const double* delta, int32_t nonneg, float* x_new, double* penalty, void* stream) {
  if (!x_old || !g || !d || !beta || !delta || !x_new || n_mats < 1 || n_mats > 3 || nz <= 0 || ny <= 0 || nx <= 0)
    return DEXCT_EINVAL;
  if (!(g_scale > 0.0) || !std::isfinite(g_scale)) return DEXCT_EINVAL;
  const int64_t n = (int64_t)nz * ny * nx;
  if (n > kPwlsMaxElems) return DEXCT_ERANGE;
  if (overlap(x_old, x_new, n * n_mats)) return DEXCT_EINVAL;      // a Jacobi step: every pixel reads the OLD neighbours
  PwlsPenalty pen{};
  for (int k = 0; k < n_mats; ++k) {
    if (!(beta[k] >= 0.0) || !std::isfinite(beta[k]) || !(delta[k] > 0.0) || !std::isfinite(delta[k])) return DEXCT_EINVAL;
    pen.beta[k] = (float)beta[k];
    pen.delta[k] = (float)delta[k];
    if (!(pen.delta[k] > 0.0f) || !std::isfinite(pen.beta[k]) || !std::isfinite(pen.delta[k])) return DEXCT_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  if (penalty) DEXCT_HIP_TRY(hipMemsetAsync(penalty, 0, sizeof(double), st));
  const dim3 grid((unsigned)pwls_blocks(n));
  PWLS_BY_K(n_mats, hipLaunchKernelGGL(pwls_update_kernel<KK>, grid, dim3(256), 0, st, x_old, g, d, n, (int)nx, (int)ny, pen,
                                       (float)g_scale, (int)nonneg, x_new, penalty));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // extern "C"
