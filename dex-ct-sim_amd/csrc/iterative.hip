// A matched projector pair on float32 images, and the element-wise steps of SIRT / OS-SART built on it.
//
// The system matrix A is the one the label projector (siddon.hip) defines: ray i = (view, channel) walks the slabs of
// its dominant axis with the fixed-point plan of dexct_fan_plan, and slab s gives dda_slab's two pieces (ja, t) and
// (jb, 1 - t).  slab_coef below turns them into the coefficients of row i - it is the ONLY place a coefficient is
// formed, and both kernels call it, so the back-projector is the transpose of the projector by construction:
//   image_project_kernel      sino[i]  = sum_j a_ij image[j]      a gather: one value per ray, no atomics, bit-reproducible
//   image_backproject_kernel  image[j] += sum_i a_ij sino[i]      the scatter of the same loop with float atomics
// Mapping: lanes along channels (adjacent channels hit adjacent minor indices of the same slab), a lane loops over the
// slabs of its ray like rays_kernel; NS stacked slices per lane share the slab geometry.  The accesses of a wave are
// contiguous where the MINOR axis is the contiguous one: y-dominant rays (minor x) on the image [slice][iy][ix] itself,
// x-dominant rays (minor y) on an in-plane transposed copy [slice][ix][iy] - read from it in the forward, accumulated
// into it in the adjoint and merged by one transposing add at the end.  Without the transposed buffer both kernels
// work on the image alone (x-dominant rays then touch one image row per lane).
#include "common.h"

namespace dexct {

// The coefficients of one slab: a_(i,(s,ja)) = t len_per_u and a_(i,(s,jb)) = (1 - t) len_per_u where the pieces lie in two
// pixels, the single coefficient len_per_u (on piece b) where they share one; a piece outside the grid has none.
struct SlabCoef {
  int32_t ja, jb;
  float ca, cb;
  bool has_a, has_b;
};

__device__ __forceinline__ SlabCoef slab_coef(long long V, long long SV, uint32_t smask, float kf, float len_per_u, int nv) {
  const SlabPieces sp = dda_slab(V, SV, smask, kf);
  SlabCoef c;
  c.ja = sp.ja;
  c.jb = sp.jb;
  const bool one = sp.ja == sp.jb;
  c.has_a = !one && (uint32_t)sp.ja < (uint32_t)nv;
  c.has_b = (uint32_t)sp.jb < (uint32_t)nv;
  c.ca = sp.t * len_per_u;
  c.cb = one ? len_per_u : (1.0f - sp.t) * len_per_u;
  return c;
}

struct IterArgs {
  dexct_fan_geom g;
  const dexct_ray_plan* plan;   // of view_begin onwards
  int view_step;
};

// Where the pixels of dominant-axis slab i, minor index j live: element i * su + j * sv of a slice.
struct Walk {
  uint32_t su, sv;
  bool transposed;
};

__device__ __forceinline__ Walk walk_of(int axis, const dexct_fan_geom& g, bool have_t) {
  Walk w;
  if (axis == 1) { w.su = (uint32_t)g.nx; w.sv = 1u; w.transposed = false; }          // u = y, v = x: image rows
  else if (have_t) { w.su = (uint32_t)g.ny; w.sv = 1u; w.transposed = true; }          // u = x, v = y: rows of the transposed copy
  else { w.su = 1u; w.sv = (uint32_t)g.nx; w.transposed = false; }
  return w;
}

template <int NS>
__global__ __launch_bounds__(256) void image_project_kernel(IterArgs a, const float* __restrict__ image,
                                                            const float* __restrict__ image_t, float* __restrict__ sino) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.g.n_channels) return;
  const int r0 = blockIdx.y * NS;
  const size_t vl = (size_t)blockIdx.z * a.view_step;                      // view - view_begin
  const dexct_ray_plan p = a.plan[vl * a.g.n_channels + c];
  const int axis = p.flags & 1u;
  const uint32_t smask = (p.flags & 2u) ? 0xFFFFFFFFu : 0u;
  const int nv = axis == 0 ? a.g.ny : a.g.nx;
  const Walk w = walk_of(axis, a.g, image_t != nullptr);
  const size_t plane = (size_t)a.g.nx * a.g.ny;
  const float* __restrict__ base = (w.transposed ? image_t : image) + (size_t)(a.g.z_first + r0) * plane;
  const int n_here = min(NS, a.g.n_rows - r0);
  float acc[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) acc[q] = 0.0f;
  long long V = p.V0 + (long long)p.i_first * p.SV;
  uint32_t off = (uint32_t)p.i_first * w.su;
  for (int s = 0; s < p.n_slabs; ++s) {
    const SlabCoef k = slab_coef(V, p.SV, smask, p.kf, p.len_per_u, nv);
    const uint32_t oa = off + (uint32_t)k.ja * w.sv, ob = off + (uint32_t)k.jb * w.sv;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      if (q < n_here) {
        if (k.has_a) acc[q] += k.ca * base[q * plane + oa];
        if (k.has_b) acc[q] += k.cb * base[q * plane + ob];
      }
    }
    V += p.SV;
    off += w.su;
  }
#pragma unroll
  for (int q = 0; q < NS; ++q)
    if (q < n_here) sino[(vl * a.g.n_rows + r0 + q) * a.g.n_channels + c] = acc[q];
}

template <int NS>
__global__ __launch_bounds__(256) void image_backproject_kernel(IterArgs a, const float* __restrict__ sino,
                                                                float* __restrict__ image, float* __restrict__ image_t) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.g.n_channels) return;
  const int r0 = blockIdx.y * NS;
  const size_t vl = (size_t)blockIdx.z * a.view_step;
  const dexct_ray_plan p = a.plan[vl * a.g.n_channels + c];
  const int axis = p.flags & 1u;
  const uint32_t smask = (p.flags & 2u) ? 0xFFFFFFFFu : 0u;
  const int nv = axis == 0 ? a.g.ny : a.g.nx;
  const Walk w = walk_of(axis, a.g, image_t != nullptr);
  const size_t plane = (size_t)a.g.nx * a.g.ny;
  float* __restrict__ base = (w.transposed ? image_t : image) + (size_t)(a.g.z_first + r0) * plane;
  const int n_here = min(NS, a.g.n_rows - r0);
  float y[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) y[q] = q < n_here ? sino[(vl * a.g.n_rows + r0 + q) * a.g.n_channels + c] : 0.0f;
  long long V = p.V0 + (long long)p.i_first * p.SV;
  uint32_t off = (uint32_t)p.i_first * w.su;
  for (int s = 0; s < p.n_slabs; ++s) {
    const SlabCoef k = slab_coef(V, p.SV, smask, p.kf, p.len_per_u, nv);
    const uint32_t oa = off + (uint32_t)k.ja * w.sv, ob = off + (uint32_t)k.jb * w.sv;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      if (q < n_here) {
        if (k.has_a) atomicAdd(base + q * plane + oa, k.ca * y[q]);
        if (k.has_b) atomicAdd(base + q * plane + ob, k.cb * y[q]);
      }
    }
    V += p.SV;
    off += w.su;
  }
}

// image[slice][iy][ix] += acc_t[slice][ix][iy], 32 x 32 tiles through LDS (coalesced on both sides).
__global__ __launch_bounds__(256) void merge_transposed_kernel(const float* __restrict__ acc_t, float* __restrict__ image,
                                                               int nx, int ny) {
  __shared__ float tile[32][33];
  const size_t base = (size_t)blockIdx.z * nx * ny;
  const int y0 = blockIdx.x * 32, x0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int x = x0 + k, y = y0 + tx;
    if (x < nx && y < ny) tile[k][tx] = acc_t[base + (size_t)x * ny + y];
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int y = y0 + k, x = x0 + tx;
    if (x < nx && y < ny) image[base + (size_t)y * nx + x] += tile[tx][k];
  }
}

// element (k, e) of the subset: line k * view_step of the sinogram, e < line
__global__ __launch_bounds__(256) void sirt_residual_kernel(const float* __restrict__ b, const float* ax,
                                                            const float* __restrict__ row_sum, int64_t n_sub, int64_t step,
                                                            int64_t line, float* r, double* norm2) {
  __shared__ double part[4];
  const int64_t total = n_sub * line;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t k = i / line;
    const int64_t o = k * step * line + (i - k * line);
    const float R = row_sum[o];
    const float bo = b[o], ao = ax[o];
    const float d = bo - ao;
    const bool hit = R > 0.0f;                 // a ray with R = 0 has missed the grid
    if (r) r[o] = hit ? d / R : 0.0f;
    if (norm2 && hit) {                        // from the float32 inputs in float64, like the objective of pwls_residual_kernel:
      const double dd = (double)bo - (double)ao;   // the float32 d would leave its rounding (2^-24 per term) in the sum
      acc += dd * dd / (double)R;
    }
  }
  if (!norm2) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = (part[0] + part[1]) + (part[2] + part[3]);
    if (s != 0.0) atomicAdd(norm2, s);
  }
}

__global__ __launch_bounds__(256) void sirt_update_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ col_sum, int64_t n, float relax, int nonneg) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float C = col_sum[i];
    float v = x[i];
    if (C > 0.0f) v = v + relax * (g[i] / C);  // pixels no ray of the subset crosses stay as they are
    if (nonneg) v = fmaxf(v, 0.0f);
    x[i] = v;
  }
}

constexpr int kIterSlices = 4;   // stacked slices per lane

static int check_pair(const dexct_fan_geom* g, const void* plan, int view_begin, int view_end, int view_step, const void* p0,
                      const void* p1) {
  if (!g || !plan || !p0 || !p1) return DEXCT_EINVAL;
  if (view_step < 1 || view_begin < 0 || view_end <= view_begin || view_end > g->n_views) return DEXCT_EINVAL;
  if (g->n_channels <= 0 || g->n_rows <= 0 || g->nx <= 0 || g->ny <= 0 || g->nz <= 0) return DEXCT_EINVAL;
  if (g->z_first < 0 || (int64_t)g->z_first + g->n_rows > g->nz) return DEXCT_EINVAL;
  if (g->nx > 8192 || g->ny > 8192) return DEXCT_ERANGE;          // the plan's fixed-point range
  if (view_end - view_begin > 65535 || g->n_rows > 65535 || g->nz > 65535) return DEXCT_ERANGE;
  return DEXCT_OK;
}

// the grid cap of the two SIRT steps; tests/grid_caps.py holds its value, tests/test_gpu_grid_passes.py runs past it
constexpr int kElementwiseMaxBlocks = 4096;

static int64_t elementwise_blocks(int64_t n) {
  int64_t nb = (n + 255) / 256;
  return nb < 1 ? 1 : (nb > kElementwiseMaxBlocks ? kElementwiseMaxBlocks : nb);
}

}  // namespace dexct

using namespace dexct;

extern "C" {

int dexct_image_project(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin, int32_t view_end,
                        int32_t view_step, const float* image, const float* image_t, float* sino, void* stream) {
  const int rc = check_pair(geom, plan, view_begin, view_end, view_step, image, sino);
  if (rc != DEXCT_OK) return rc;
  const int n_sub = (view_end - view_begin + view_step - 1) / view_step;
  const IterArgs a{*geom, plan, view_step};
  const unsigned bx = (unsigned)((geom->n_channels + 255) / 256);
  if (geom->n_rows == 1) {
    hipLaunchKernelGGL(image_project_kernel<1>, dim3(bx, 1, n_sub), dim3(256), 0, as_stream(stream), a, image, image_t, sino);
  } else {
    const unsigned by = (unsigned)((geom->n_rows + kIterSlices - 1) / kIterSlices);
    hipLaunchKernelGGL(image_project_kernel<kIterSlices>, dim3(bx, by, n_sub), dim3(256), 0, as_stream(stream), a, image,
                       image_t, sino);
  }
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_image_backproject(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin, int32_t view_end,
                            int32_t view_step, const float* sino, float* image, float* acc_t, int32_t accumulate,
                            void* stream) {
  const int rc = check_pair(geom, plan, view_begin, view_end, view_step, sino, image);
  if (rc != DEXCT_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int n_sub = (view_end - view_begin + view_step - 1) / view_step;
  const size_t plane = (size_t)geom->nx * geom->ny;
  float* acc_first = acc_t ? acc_t + (size_t)geom->z_first * plane : nullptr;
  if (!accumulate) DEXCT_HIP_TRY(hipMemsetAsync(image, 0, plane * geom->nz * sizeof(float), st));
  if (acc_t) DEXCT_HIP_TRY(hipMemsetAsync(acc_first, 0, plane * geom->n_rows * sizeof(float), st));
  const IterArgs a{*geom, plan, view_step};
  const unsigned bx = (unsigned)((geom->n_channels + 255) / 256);
  if (geom->n_rows == 1) {
    hipLaunchKernelGGL(image_backproject_kernel<1>, dim3(bx, 1, n_sub), dim3(256), 0, st, a, sino, image, acc_t);
  } else {
    const unsigned by = (unsigned)((geom->n_rows + kIterSlices - 1) / kIterSlices);
    hipLaunchKernelGGL(image_backproject_kernel<kIterSlices>, dim3(bx, by, n_sub), dim3(256), 0, st, a, sino, image, acc_t);
  }
  DEXCT_LAUNCH_CHECK();
  if (acc_t) {
    dim3 grid((geom->ny + 31) / 32, (geom->nx + 31) / 32, geom->n_rows);
    hipLaunchKernelGGL(merge_transposed_kernel, grid, dim3(256), 0, st, acc_first, image + (size_t)geom->z_first * plane,
                       geom->nx, geom->ny);
    DEXCT_LAUNCH_CHECK();
  }
  return DEXCT_OK;
}

int dexct_sirt_residual(const float* b, const float* ax, const float* row_sum, int32_t n_lines, int32_t line_step,
                        int64_t line, float* r, double* norm2, void* stream) {
  if (!b || !ax || !row_sum || (!r && !norm2) || n_lines <= 0 || line_step < 1 || line <= 0) return DEXCT_EINVAL;
  hipStream_t st = as_stream(stream);
  if (norm2) DEXCT_HIP_TRY(hipMemsetAsync(norm2, 0, sizeof(double), st));
  const int64_t n_sub = (n_lines + line_step - 1) / line_step;
  hipLaunchKernelGGL(sirt_residual_kernel, dim3((unsigned)elementwise_blocks(n_sub * line)), dim3(256), 0, st, b, ax, row_sum,
                     n_sub, (int64_t)line_step, line, r, norm2);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_sirt_update(float* x, const float* g, const float* col_sum, int64_t n, double relax, int32_t nonneg, void* stream) {
  if (!x || !g || !col_sum || n <= 0 || !(relax > 0.0)) return DEXCT_EINVAL;
  hipLaunchKernelGGL(sirt_update_kernel, dim3((unsigned)elementwise_blocks(n)), dim3(256), 0, as_stream(stream), x, g, col_sum,
                     n, (float)relax, (int)nonneg);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // extern "C"
