// The float64 table exponential and the refined reciprocal of the Newton kernels: the one copy, included by gn.hip,
// gn_multi.hip and gn_cov.hip (internal).
#pragma once
#include <hip/hip_runtime.h>

namespace dexct {
namespace exptab {

// exp(x) for |x| <= 700, given y = x * 2048/ln2 (the tables hold -mu * 2048/ln2, so y costs the same instructions as x would):
// y = n + f with n = rint(y) = 2048 k + j, |f| <= 1/2, and
// exp(x) = 2^k * 2^(j/2048) * e^(f ln2/2048), a cubic in f for e^r - 1 (truncation r^4/24 < 4e-17, r = f ln2/2048).
// n comes out of the low mantissa bits of y + 1.5 * 2^52 (round to nearest even, like rint); f = y - n is exact.  About 1 ulp.
// 2^k without an instruction of its own: the table entry j holds 2^(j/2048) with j << 9 SUBTRACTED from its high word
// (pow_entry), so that adding n << 9 = (k << 20) + (j << 9) to the high word of what was loaded - one v_lshl_add_u32, no mask -
// gives 2^k 2^(j/2048) before the last FMA; scaling by a power of two is exact, so the bits are those of ldexp(fma(tj, p, tj), k)
// wherever that is a normal number - and it is for |x| <= 700 (e^-700 = 1e-304), which every caller guarantees: the clip of
// matdecomp.py:116, the clip-free bound of gn.hip's newton_sums_f64, float32-normal arguments of its log_pos.
// NaN stays NaN (f is NaN then, whatever the table entry became).
constexpr int kPowBits = 11;
constexpr int kPowN = 1 << kPowBits;                         // table entries: 16 KB of LDS
constexpr double kExpScale = 0x1.71547652b82fep+11;          // 2048 / ln 2
constexpr double kExpClip = 700.0 * kExpScale;               // the reference's clip of the exponent (matdecomp.py:116), in units of y

__device__ __forceinline__ double pow_entry(int j) {
  const double v = exp2((double)j * (1.0 / kPowN));
  return __hiloint2double(__double2hiint(v) - (j << (20 - kPowBits)), __double2loint(v));
}

// every thread of the block calls this before the first exp_tab; ends with a barrier.  gn_cov.hip calls it; the kernels of
// gn.hip and gn_multi.hip keep the same two lines as text, because the call compiles to another order of their prologues.
template <int kBlock>
__device__ __forceinline__ void fill_pow_table(double* __restrict__ lds_pow) {
  for (int j = threadIdx.x; j < kPowN; j += kBlock) lds_pow[j] = pow_entry(j);
  __syncthreads();
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

// 1 / x by v_rcp_f64 and two Newton refinements (what a float64 division starts with, without its scaling and fix-up steps:
// the operands here - expected counts, the Hessian's determinant - are far from the subnormal range).  For x = 0, +-inf or NaN
// the refinement would turn the hardware's answer (inf, 0, NaN - what IEEE division gives) into NaN, so it is skipped there: a
// sum that overflowed during a wild transient then behaves as in the reference (g / inf = 0) and the pixel can still recover.
__device__ __forceinline__ double rcp_f64(double x) {
  const double r0 = __builtin_amdgcn_rcp(x);
  double r = fma(r0, fma(-x, r0, 1.0), r0);
  r = fma(r, fma(-x, r, 1.0), r);
  const double ax = fabs(x);
  return (ax > 0.0 && ax < __builtin_huge_val()) ? r : r0;
}

}  // namespace exptab
}  // namespace dexct
