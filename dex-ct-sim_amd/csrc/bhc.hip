// First-order beam-hardening correction: every log value p goes through a tabulated inverse of the reference material's
// polychromatic log signal, out = mu_ref * P_m^{-1}(p) (dex-ct-sim_amd/bhc.py builds the table; include/dexct.h states the
// contract).  Element-wise and HBM-bound: 4 B read + 4 B written per value.
//
// Persistent grid-stride workgroups of 1024 lanes stage the table ({value, slope} per node, <= 64 KiB) into LDS once;
// each lane then streams 16-byte loads of p, two in flight, and evaluates the cubic Hermite cell in registers.  Neighbouring
// pixels have nearby p, so the LDS gathers of a wave mostly hit one or two nodes (broadcast).  Scalar head and tail cover
// any alignment; p and out with different offsets modulo 16 B take the scalar path throughout.
#include "common.h"

#include <math.h>

namespace dexct {

constexpr int kBhcBlock = 1024;
// workgroups per CU, the grid cap; tests/grid_caps.py holds its value, tests/test_gpu_grid_passes.py runs past it
constexpr int kBhcGroupsPerCu = 2;

// The table's cells: per sign of p a run of nodes in a = |p|, a linear run of C = 2^K cells over [0, 2^E] and then C cells
// per octave [2^(E+o), 2^(E+o+1)), o < n_oct (the layout of float32 itself: the exponent bits give the octave, the top K
// mantissa bits the cell, the rest the fraction t exactly - no logarithm, no rounding).  Node j holds {value, d value / da}.
struct BhcGrid {
  int32_t base_neg;    // index of the negative side's node 0
  int32_t cells;       // C
  int32_t e_min;       // E
  int32_t shift;       // 23 - K
  int32_t oct_pos, oct_neg;
  float lin_scale;     // 2^(K - E): a -> cell coordinate in the linear run
  float lin_width;     // 2^(E - K)
  float cell_frac;     // 2^-K
  float frac_scale;    // 2^-(23 - K)
  float a_max_pos, a_max_neg;   // 2^(E + n_oct) of each side
};

// One value: cubic Hermite in float32 in the basis form h00 f0 + h01 f1 + w (h10 s0 + h11 s1), whose two value weights are
// non-negative and sum to one.  Beyond a side's last node: linear from its value and slope (+-inf give +-inf); NaN passes.
__device__ __forceinline__ float bhc_eval(float p, const float2* __restrict__ tab, const BhcGrid& g) {
  if (p != p) return p;
  const bool neg = p < 0.0f;
  const float a = fabsf(p);
  const float2* side = tab + (neg ? g.base_neg : 0);
  const int n_oct = neg ? g.oct_neg : g.oct_pos;
  const uint32_t bits = __float_as_uint(a);
  const int o = (int)(bits >> 23) - (127 + g.e_min);
  if (o >= n_oct) {
    const float2 e = side[g.cells * (1 + n_oct)];
    return e.x + (a - (neg ? g.a_max_neg : g.a_max_pos)) * e.y;
  }
  int j;
  float t, w;
  if (o < 0) {                       // linear run below 2^E (zero and denormals included)
    const float u = a * g.lin_scale;
    j = (int)u;
    t = u - (float)j;
    w = g.lin_width;
  } else {
    const uint32_t man = bits & 0x7FFFFFu;
    j = g.cells * (1 + o) + (int)(man >> g.shift);
    t = (float)(man & ((1u << g.shift) - 1u)) * g.frac_scale;
    w = __uint_as_float(bits & 0x7F800000u) * g.cell_frac;
  }
  const float2 l = side[j], r = side[j + 1];
  const float s = 1.0f - t;
  const float h01 = t * t * (3.0f - 2.0f * t);
  const float h00 = 1.0f - h01;
  const float d = t * s * (s * l.y - t * r.y);
  return fmaf(h00, l.x, fmaf(h01, r.x, w * d));
}

__global__ __launch_bounds__(kBhcBlock) void bhc_linearize_kernel(const float* p, int64_t n, const float2* __restrict__ table,
                                                                  int n_nodes, BhcGrid g, float* out, int64_t head,
                                                                  int vector) {
  extern __shared__ float2 tab[];
  for (int i = threadIdx.x; i < n_nodes; i += kBhcBlock) tab[i] = table[i];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kBhcBlock;
  const int64_t gid = (int64_t)blockIdx.x * kBhcBlock + threadIdx.x;
  if (!vector) {
    for (int64_t i = gid; i < n; i += stride) out[i] = bhc_eval(p[i], tab, g);
    return;
  }
  // scalar head up to the first 16-byte boundary, float4 body, scalar tail
  if (gid < head) out[gid] = bhc_eval(p[gid], tab, g);
  const int64_t nv = (n - head) >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  float4* o4 = reinterpret_cast<float4*>(out + head);
  for (int64_t i = gid; i < nv; i += 2 * stride) {
    const int64_t j = i + stride;
    const float4 a = p4[i];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nv) b = p4[j];
    float4 ra, rb;
    ra.x = bhc_eval(a.x, tab, g);
    ra.y = bhc_eval(a.y, tab, g);
    ra.z = bhc_eval(a.z, tab, g);
    ra.w = bhc_eval(a.w, tab, g);
    o4[i] = ra;
    if (j < nv) {
      rb.x = bhc_eval(b.x, tab, g);
      rb.y = bhc_eval(b.y, tab, g);
      rb.z = bhc_eval(b.z, tab, g);
      rb.w = bhc_eval(b.w, tab, g);
      o4[j] = rb;
    }
  }
  const int64_t t0 = head + (nv << 2);
  if (t0 + gid < n) out[t0 + gid] = bhc_eval(p[t0 + gid], tab, g);
}

}  // namespace dexct

namespace dexct {
// node count of a table: per side C cells of the linear run, C per octave, and the end node
inline int bhc_nodes(int cells_log2, int octaves_pos, int octaves_neg) {
  return (1 << cells_log2) * (2 + octaves_pos + octaves_neg) + 2;
}
}  // namespace dexct

extern "C" int dexct_bhc_linearize(const float* p, int64_t n, const float* table, int32_t log2_min, int32_t cells_log2,
                                   int32_t octaves_pos, int32_t octaves_neg, float* out, void* stream) {
  using namespace dexct;
  if (!p || !table || !out || n < 0 || cells_log2 < 0 || cells_log2 > DEXCT_BHC_MAX_CELLS_LOG2 || octaves_pos < 0 ||
      octaves_neg < 0 || log2_min < -100 || log2_min + (octaves_pos > octaves_neg ? octaves_pos : octaves_neg) > 100 ||
      bhc_nodes(cells_log2, octaves_pos, octaves_neg) > DEXCT_BHC_MAX_NODES)
    return DEXCT_EINVAL;
  if (n == 0) return DEXCT_OK;
  const int n_nodes = bhc_nodes(cells_log2, octaves_pos, octaves_neg);
  BhcGrid g;
  g.cells = 1 << cells_log2;
  g.base_neg = g.cells * (1 + octaves_pos) + 1;
  g.e_min = log2_min;
  g.shift = 23 - cells_log2;
  g.oct_pos = octaves_pos;
  g.oct_neg = octaves_neg;
  g.lin_scale = ldexpf(1.0f, cells_log2 - log2_min);
  g.lin_width = ldexpf(1.0f, log2_min - cells_log2);
  g.cell_frac = ldexpf(1.0f, -cells_log2);
  g.frac_scale = ldexpf(1.0f, -(23 - cells_log2));
  g.a_max_pos = ldexpf(1.0f, log2_min + octaves_pos);
  g.a_max_neg = ldexpf(1.0f, log2_min + octaves_neg);
  static const int n_cu = [] {             // queried once per process (one GPU per process)
    int dev_id = 0, c = 0;
    if (hipGetDevice(&dev_id) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev_id) != hipSuccess || c <= 0)
      c = 256;
    return c;
  }();
  const uintptr_t ap = reinterpret_cast<uintptr_t>(p), ao = reinterpret_cast<uintptr_t>(out);
  // the float4 body needs p and out at one offset modulo 16 B (always true in place); float alignment is assumed
  const int vector = ((ap & 15u) == (ao & 15u)) && (ap & 3u) == 0;
  int64_t head = vector ? (int64_t)(((16u - (ap & 15u)) & 15u) >> 2) : 0;
  if (head > n) head = n;
  // resident workgroups only: two 1024-lane groups fill a CU (32 waves), and a full 64 KiB table still lets both in
  const size_t lds = (size_t)n_nodes * sizeof(float2);
  const int64_t per_block = (int64_t)kBhcBlock * (vector ? 8 : 1);
  int64_t nb = (n + per_block - 1) / per_block;
  if (nb > (int64_t)n_cu * kBhcGroupsPerCu) nb = (int64_t)n_cu * kBhcGroupsPerCu;
  DEXCT_ALLOW_LDS(bhc_linearize_kernel, lds);
  hipLaunchKernelGGL(bhc_linearize_kernel, dim3((unsigned)nb), dim3(kBhcBlock), lds, as_stream(stream), p, n,
                     reinterpret_cast<const float2*>(table), n_nodes, g, out, head, vector);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}
