"""What every quantum-noise sample must be: a NumPy restatement of csrc/noise_sample.h (Philox4x32-10, the Box-Muller normals
of a pixel, noisy_count) and of poisson_draw / poisson_detect_kernel in csrc/noise.hip, with the bounds the device has to meet
and the inputs of tests/test_gpu_noise.py; plain NumPy, no device, no torch.  tests/test_noise_refs.py shows on the CPU that the
reference is right (published known answers, moments, edge words), that every comparison below rejects a sampler that is wrong
in one of eleven small ways, and that the caps on the undecidable elements hold for exactly the inputs the GPU module uses.

The sample is a pure function of integers: (seed, global view, row, channel, spectrum[, energy]) -> four 32-bit words -> a
float32 pair (u1, u2).  Up to there the reference is exact - the float32 roundings of u1 = ((float)w + 1) 2^-32 and
u2 = (float)w 2^-32 are part of the definition of the sample.  From there on the reference is float64 and the device float32;
u = 2^-24 is the float32 unit round-off.

The Gaussian sample (pixel_normals, noisy_count)
  z = sqrt(-2 ln u1) {cos, sin}(2 pi u2) comes from the hardware's v_log_f32, v_sqrt_f32, v_cos_f32 / v_sin_f32, for which
  neither the project nor its guides hold an accuracy figure.  The bound is therefore chosen for what it has to separate, not
  measured: |z_gpu - z_ref| <= Z_TOL = 1e-3, absolute.  A structural error (another word, another pixel, sine for cosine)
  replaces z by a different normal, O(1) away, that lands within 1e-3 with probability < 1e-3 per pixel; a float32 libm
  evaluation of the same formula sits 1.3e-6 from float64 (131 072 pixels, largest radius 5.33).
  noisy_count = fmaxf(fmaf(sqrt(fmaxf(var, 0)), z, mean), 1e-20): the square root (<= 1 ulp = 2 u) and the fmaf (u) on top:
      |err| <= sqrt(var) Z_TOL + 4 u (|mean| + sqrt(var) |z|)
  fmaxf returns its other operand for a NaN one: a NaN variance counts as 0 (the mean comes back bit for bit), a NaN mean
  becomes 1e-20 (include/dexct.h says so).

The per-bin Poisson sample (poisson_detect_kernel<MB>, one bin = one (ray, spectrum, energy))
  lambda.  The kernel forms, in float32,
      L_m = pathlen[m] * (float)log2(e)                                   the constant's rounding (< u) and the product's (u)
      pe  = fmaf(mu[M-1], L[M-1], ... fmaf(mu[0], L[0], 0))               term m (from 0) passes through M - m roundings
      t   = v_exp_f32(-pe)                                                1 ulp by the public CDNA ISA guide; 2 ulp = 4 u allowed
      lambda = photons * t                                                u
  An error d in pe is a factor 2^d = exp(d ln 2) on t, and ln 2 log2(e) = 1, so with x_m = mu_m pathlen_m (natural units)
      eps = 1.001 u (5 + sum_m (M - m + 2) |x_m|)                         (1.001: the second-order terms, eps < 1e-3)
  is the relative error of the device's lambda against lambda_ref = photons exp(-sum_m x_m) in float64 from the same float32
  inputs.  Where every x_m is 0 the chain is exact (pe = 0, 2^-0 = 1, photons * 1): eps = 0, so a test with pathlen = 0
  knows lambda, and the side of 30 it lies on, exactly.  For 48 energies, lambda <= 3e3 and x <= 20: eps <= 3e-7 + 6e-8
  (M + 2) x, i.e. 3.6e-7 at x = 0 up to 6.2e-5 for 49 materials at x = 20 (where lambda < 1e-5 and no draw can change).
  Both branches of poisson_draw are non-decreasing in lambda for a fixed Philox block - the Poisson CDF falls with lambda;
  lambda + sqrt(lambda) z has the derivative 1 + z / (2 sqrt(lambda)) >= 0.39 for z >= -6.67 (u1 >= 2^-32) and lambda >= 30 -
  so the device's draw lies between the draws at lambda_lo = lambda (1 - eps) and lambda_hi = lambda (1 + eps), each taken at
  the unfavourable end of what follows; where [lambda_lo, lambda_hi] holds 30 the window is the union of both branches.
  inversion (lambda < 30), all in float64 on the device too: u = (r0 2^32 + r1 + 0.5) 2^-64, p = exp(-lambda), k steps of
      p *= lambda / k, cdf += p while u > cdf.  Device and host may differ by the exp (1 ulp) and three roundings per step, 200
      steps at most: < 7e-14 relative on cdf; the reference compares u with cdf (1 +- 1e-13).
  rounded normal (lambda >= 30): z = sqrtf(-2 logf(u1)) cospif(2 u2) from r0 and r2, then
      floorf(fmaf(sqrtf(lambda), z, lambda) + 0.5f).  With the OpenCL limits of the float32 library (logf 3 ulp, sqrtf 3 ulp,
      cospif 4 ulp; HIP documents 1 ulp each) z carries (3 + 6 + 8 + 1) u = 18 u relative, sqrtf(lambda) 6 u more, the fmaf u
      and the sum with 0.5 another u:
          delta = 1.001 u (24 sqrt(lambda) |z| + 2 (|x| + 0.5)),   x = lambda + sqrt(lambda) z
      delta <= 6e-8 (24 * 55 * 6.7 + 2 * 3400) = 9.4e-4 at lambda = 3e3, and 2e-4 for a typical |z| of 1.  It is an error of the
      ARGUMENT of floor and is applied there: floor(x(lambda_lo) - delta + 0.5) .. floor(x(lambda_hi) + delta + 0.5).  (Moving
      lambda by delta instead would move x by only 0.39 delta for the most negative z, and would blur which branch an exactly
      known lambda = 30 takes.)
  A bin whose window holds more than one integer is ambiguous: it widens the interval [lo, hi] of its ray's signal
  sum_e gain_e draw_e and is never excluded.  The float32 sum acc = fmaf(gain, draw, acc) of non-negative terms adds at most
  n_e u hi (poisson_within).
"""
import numpy as np

U = 2.0 ** -24
F32, F64, U64 = np.float32, np.float64, np.uint64
Z_TOL = 1e-3
FLOOR = 1e-20
MASK = U64(0xFFFFFFFF)
TWO_M32 = F32(2.0 ** -32)
CDF_SLACK = 1e-13

# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -------------------------

PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)
SHIFT = U64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1); arrays broadcast.  Four uint64 arrays below 2^32."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=U64) & MASK for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                              # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SHIFT) ^ c1 ^ k0, p1 & MASK, (p0 >> SHIFT) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + PHILOX_W0) & MASK, (k1 + PHILOX_W1) & MASK
    return c0, c1, c2, c3


def seed_words(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def unit_pair(w_radius, w_angle):
    """(u1, u2) as the header defines them, in float32 (returned as float64): u1 in (0, 1], u2 in [0, 1]."""
    u1 = (np.asarray(w_radius, dtype=U64).astype(F32) + F32(1.0)) * TWO_M32
    u2 = np.asarray(w_angle, dtype=U64).astype(F32) * TWO_M32
    return u1.astype(F64), u2.astype(F64)


def box_muller(w_radius, w_angle):
    """(rad cos, rad sin) in float64 from one pair of Philox words."""
    u1, u2 = unit_pair(w_radius, w_angle)
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def pixel_normals_ref(view, row, chan, seed):
    """z [4, ...] float64: the standard normals of spectra 0 .. 3 of the pixels (view = the GLOBAL view)."""
    lo, hi = seed_words(seed)
    w = philox4x32_10(view, row, chan, 0, lo, hi)
    return np.stack(box_muller(w[0], w[1]) + box_muller(w[2], w[3]))


# ---- the two memory layouts of include/dexct.h ---------------------------------------------------------------------------------

def decode(shape, layout):
    """(v, r, c) of every ray index of a (n_views, n_rows, n_channels) sinogram: layout 0 = [view][row][channel], 1 =
    [view][channel][row]."""
    n_views, n_rows, n_ch = shape
    ray = np.arange(n_views * n_rows * n_ch, dtype=np.int64)
    if layout == 0:
        return ray // (n_rows * n_ch), (ray // n_ch) % n_rows, ray % n_ch
    if layout == 1:
        return ray // (n_rows * n_ch), ray % n_rows, (ray // n_rows) % n_ch
    raise ValueError(layout)


# ---- dexct_add_noise -----------------------------------------------------------------------------------------------------------

def add_noise_ref(counts, variance, shape, layout, view_offset, seed, raw=False):
    """counts, variance float32 [S][n_rays] (any shape of S * n_rays values) -> (ref, bound) float64 [S][n_rays]:
    ref = max(mean + sqrt(max(var, 0)) z, 1e-20).  ``raw``: also mean + sd z before the clip."""
    v, r, c = decode(shape, layout)
    mean = np.asarray(counts, dtype=F32).astype(F64).reshape(-1, v.size)
    var = np.asarray(variance, dtype=F32).astype(F64).reshape(mean.shape)
    if not 1 <= mean.shape[0] <= 4:
        raise ValueError(mean.shape)
    z = pixel_normals_ref(v + view_offset, r, c, seed)[:mean.shape[0]]
    sd = np.sqrt(np.where(var > 0.0, var, 0.0))                              # (NaN > 0 is False: fmaxf(NaN, 0) = 0)
    unclipped = mean + sd * z
    ref = np.fmax(unclipped, FLOOR)                                          # (fmax, like fmaxf: NaN -> 1e-20)
    bound = sd * Z_TOL + 4.0 * U * (np.abs(mean) + sd * np.abs(z))
    return (ref, bound, unclipped) if raw else (ref, bound)


def z_within(z_got, z_ref):
    z_got = np.asarray(z_got, F64)
    return bool(np.all(np.isfinite(z_got)) and np.all(np.abs(z_got - z_ref) <= Z_TOL))


def within(got, ref, bound):
    """|got - ref| <= bound everywhere; a NaN or inf in ``got`` fails."""
    got = np.asarray(got, F64)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound))


def worst(got, ref, bound):
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, np.abs(np.asarray(got, F64) - ref) / bound, np.where(np.asarray(got, F64) == ref, 0.0, np.inf))
    return float(np.max(q))


def clip_classes(unclipped, bound):
    """(below, above, between): the reference is below minus its bound (the device must clip), above it (must not), or within it
    of zero (either)."""
    below, above = unclipped < -bound, unclipped > bound
    return below, above, ~(below | above)


def clip_ok(got, unclipped, bound):
    """The clipping case: exactly 1e-20 where the reference is below minus its bound, within the bound above it, and one of the
    two in between."""
    got = np.asarray(got, F32)
    below, above, between = clip_classes(unclipped, bound)
    g = got.astype(F64)
    ok_value = np.abs(g - unclipped) <= bound
    return bool(np.all(np.isfinite(g)) and np.all(got[below] == F32(FLOOR)) and np.all(ok_value[above])
                and np.all((got[between] == F32(FLOOR)) | ok_value[between]))


# ---- dexct_poisson_detect ------------------------------------------------------------------------------------------------------

def _inversion(lam, u, slack):
    """poisson_draw's sequential inversion in float64, u compared with cdf (1 + slack)."""
    lam = np.maximum(np.asarray(lam, F64), 0.0)
    k = np.zeros(lam.shape, np.int64)
    p = np.exp(-lam)
    cdf = p.copy()
    idx = np.flatnonzero(u > cdf * (1.0 + slack))
    n = 0
    while idx.size and n < 200:
        n += 1
        p[idx] *= lam[idx] / n
        cdf[idx] += p[idx]
        k[idx] = n
        idx = idx[u[idx] > cdf[idx] * (1.0 + slack)]
    return k


def _rounded_normal(lam, z, sign):
    """floor(lambda + sqrt(lambda) z + sign delta + 0.5), not below 0."""
    sq = np.sqrt(lam)
    x = lam + sq * z
    delta = 1.001 * U * (24.0 * sq * np.abs(z) + 2.0 * (np.abs(x) + 0.5))
    return np.maximum(np.floor(x + sign * delta + 0.5), 0.0).astype(np.int64)


def lambda_ref(pathlen, mu, photons, n_materials, n_energies, n_spectra):
    """(lambda [S][rays][E] float64, eps [rays][E]) of the module docstring from the float32 arrays the kernel is given."""
    pl = np.asarray(pathlen, F32).astype(F64).reshape(-1, n_materials)
    mu = np.asarray(mu, F32).astype(F64).reshape(n_materials, n_energies)
    ph = np.asarray(photons, F32).astype(F64).reshape(n_spectra, n_energies)
    x = pl[:, :, None] * mu[None, :, :]                                      # [rays][M][E]
    passes = (n_materials - np.arange(n_materials) + 2.0)[None, :, None]
    mag = np.sum(passes * np.abs(x), axis=1)
    eps = np.where(np.any(x != 0.0, axis=1), 1.001 * U * (5.0 + mag), 0.0)
    lam = ph[:, None, :] * np.exp(-np.sum(x, axis=1))[None]
    return lam, eps


def poisson_detect_ref(pathlen, mu, photons, gain, n_materials, n_energies, n_spectra, n_views, n_rows, n_channels, layout,
                       view_offset, seed):
    """The arguments of dexct_poisson_detect (arrays as float32 NumPy, pathlen [ray][n_materials] in the ray order of
    ``layout``) -> (lo, hi, ambiguous, detail): lo, hi float64 [S][n_rays], the closed interval of admissible signals;
    ``ambiguous`` the share of the bins with lambda > 0 whose window holds more than one integer; ``detail`` a dict of the per-bin
    arrays [S][n_rays][E]: k_lo, k_hi (the window of the draw), lam, normal (lambda_ref >= 30) and live (lambda_ref > 0)."""
    S, E = n_spectra, n_energies
    v, r, c = decode((n_views, n_rows, n_channels), layout)
    lam, eps = lambda_ref(pathlen, mu, photons, n_materials, E, S)
    g = np.asarray(gain, F32).astype(F64).reshape(E)
    lo_w, hi_w = seed_words(seed)
    ctr3 = (np.arange(S, dtype=np.int64)[:, None, None] << 24) | np.arange(E, dtype=np.int64)[None, None, :]
    w = philox4x32_10((v + view_offset)[None, :, None], r[None, :, None], c[None, :, None], ctr3, lo_w, hi_w ^ 0x9E3779B9)
    live = lam > 0.0
    lam_lo, lam_hi = lam * (1.0 - eps[None]), lam * (1.0 + eps[None])
    u = (w[0].astype(F64) * 4294967296.0 + w[1].astype(F64) + 0.5) * (1.0 / 18446744073709551616.0)
    z = box_muller(w[0], w[2])[0]
    k_lo, k_hi = np.zeros(lam.shape, np.int64), np.zeros(lam.shape, np.int64)
    inv, nrm = live & (lam_lo < 30.0), live & (lam_hi >= 30.0)
    both = inv & nrm
    # inversion at both ends (a window that holds 30 ends at 30 on this branch)
    k_lo[inv] = _inversion(lam_lo[inv], u[inv], +CDF_SLACK)
    k_hi[inv] = _inversion(np.minimum(lam_hi[inv], 30.0), u[inv], -CDF_SLACK)
    n_lo = _rounded_normal(np.maximum(lam_lo[nrm], 30.0), z[nrm], -1.0)
    n_hi = _rounded_normal(lam_hi[nrm], z[nrm], +1.0)
    only = nrm & ~inv
    k_lo[only], k_hi[only] = n_lo[only[nrm]], n_hi[only[nrm]]
    k_lo[both] = np.minimum(k_lo[both], n_lo[both[nrm]])
    k_hi[both] = np.maximum(k_hi[both], n_hi[both[nrm]])
    assert np.all(k_lo <= k_hi)
    lo = np.maximum(np.sum(g * k_lo, axis=2), FLOOR)
    hi = np.maximum(np.sum(g * k_hi, axis=2), FLOOR)
    ambiguous = float(np.count_nonzero(k_hi[live] > k_lo[live])) / max(int(np.count_nonzero(live)), 1)
    return lo, hi, ambiguous, dict(k_lo=k_lo, k_hi=k_hi, lam=lam, normal=live & (lam >= 30.0), live=live)


def poisson_within(signal, lo, hi, n_energies):
    """signal [S][n_rays] inside [lo, hi], widened by n_e u hi for the float32 sum over the energies."""
    s = np.asarray(signal, F64).reshape(lo.shape)
    slack = n_energies * U * hi
    return bool(np.all(np.isfinite(s)) and np.all(s >= lo - slack) and np.all(s <= hi + slack))


def decode_draws(signal, gain):
    """The per-bin draws out of signal = sum_e gain_e draw_e for gains 1, 2^8, 2^16, ... and draws below 256 (the sum is exact in
    float32); the 1e-20 floor stands for no photon at all.  [S][n_rays][E] int64, or None where a signal is not a whole number
    below 2^24."""
    s = np.asarray(signal, F64)
    s = np.where(s == F64(F32(FLOOR)), 0.0, s)
    if not (np.all(np.isfinite(s)) and np.all(s == np.floor(s)) and np.all(s >= 0) and np.all(s < 2.0 ** 24)):
        return None
    n = s.astype(np.int64)
    assert [int(x) for x in gain] == [256 ** e for e in range(len(gain))]
    return np.stack([(n >> (8 * e)) & 255 for e in range(len(gain))], axis=-1)


def decode_ok(signal, detail, gain):
    """Every bin's draw, recovered from the signal, lies in the reference's window (one value outside the delta window of a
    rounded-normal bin)."""
    d = decode_draws(np.asarray(signal).reshape(detail['k_lo'].shape[:2]), gain)
    return d is not None and bool(np.all(d >= detail['k_lo']) and np.all(d <= detail['k_hi']))


# ---- the inputs of tests/test_gpu_noise.py (tests/test_noise_refs.py checks their caps on the CPU) -----------------------------

SEEDS = (1234, (0xDEADBEEF << 32) | 0x12345678)                              # the second with a non-zero high word
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 4, 67), (9, 4, 131)]                     # (V, R, Ch); 9 * 4 * 131 = 4 716 = 18 * 256 + 108
VIEW_OFFSETS = (0, 17)
AMBIGUOUS_CAP = 0.01
CLIP_CAP = 0.001


def add_noise_cases(shape):
    """(n_spectra, layout, view_offset, seed) for one shape: every combination the issue names."""
    return [(s, layout, off, seed) for s in (1, 2, 3, 4) for layout in (0, 1) for off in VIEW_OFFSETS for seed in SEEDS]


def physical_inputs(n_spectra, shape, salt=0):
    """Means log-uniform in 1e2 .. 1e6, variance = mean x U(0.5, 2); float32 [S][n_rays]."""
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(1000 * n + n_spectra + salt)
    mean = (10.0 ** rng.uniform(2.0, 6.0, (n_spectra, n))).astype(F32)
    return mean, (mean * rng.uniform(0.5, 2.0, mean.shape)).astype(F32)


def constant_inputs(n_spectra, shape, mean, variance):
    n = shape[0] * shape[1] * shape[2]
    return np.full((n_spectra, n), mean, F32), np.full((n_spectra, n), variance, F32)


POISSON_SHAPE = (5, 4, 67)                                                   # 1 340 rays: five blocks of 256 and a ragged sixth
DECODE_GAIN = np.array([1.0, 256.0, 65536.0], F32)
# photons [S = 2][E = 3] between 0.05 and 60: over the two tables every (spectrum, energy) sees both branches
DECODE_TABLES = [np.array([[0.05, 12.0, 45.0], [60.0, 29.5, 3.0]], F32), np.array([[40.0, 31.0, 0.7], [8.0, 55.0, 33.0]], F32)]
BELOW_30 = np.nextafter(F32(30.0), F32(0.0))
BOUNDARY_TABLE = np.array([[30.0, BELOW_30, 30.0], [BELOW_30, 30.0, BELOW_30]], F32)
DARK_TABLE = np.array([[0.0, -1.0, 0.0], [-5.0, 0.0, -0.0]], F32)


def unattenuated_problem(photons, layout=0, view_offset=0, seed=SEEDS[0], shape=POISSON_SHAPE):
    """pathlen = 0 on one material: lambda = photons exactly.  The keyword arguments of poisson_detect_ref / the C entry point."""
    n = shape[0] * shape[1] * shape[2]
    photons = np.asarray(photons, F32)
    return dict(pathlen=np.zeros((n, 1), F32), mu=np.full((1, photons.shape[1]), 0.3, F32), photons=photons,
                gain=DECODE_GAIN[:photons.shape[1]].copy(), n_materials=1, n_energies=photons.shape[1], n_spectra=photons.shape[0],
                n_views=shape[0], n_rows=shape[1], n_channels=shape[2], layout=layout, view_offset=view_offset, seed=seed)


ATTENUATED_MATERIALS = (1, 4, 5, 17, 49)                                     # the 4 / 16 / 48 / 256 templates, both sides of each
X_MAX = 10.0


def attenuated_problem(n_mat, layout):
    """48 energies, 3 spectra, POISSON_SHAPE, view_offset 17, an energy-integrating gain; lambda from 3e3 (ray 0 crosses
    nothing, photons up to 3e3) to below 1e-3, roughly log-uniform.  Spectrum 1 weights no energy of the upper half."""
    n_e, S = 48, 3
    n = POISSON_SHAPE[0] * POISSON_SHAPE[1] * POISSON_SHAPE[2]
    rng = np.random.default_rng(100 + n_mat)
    E = np.linspace(30.0, 124.0, n_e)
    a, b = rng.uniform(0.1, 0.5, n_mat), rng.uniform(0.3, 1.0, n_mat)
    mu = a[:, None] * (E[None, :] / 60.0) ** -b[:, None]
    x_ray = rng.uniform(0.0, X_MAX, n)
    x_ray[0] = 0.0
    pathlen = x_ray[:, None] * rng.dirichlet(np.ones(n_mat), n) / a[None, :]
    photons = 3e3 * rng.uniform(0.3, 1.0, (S, n_e))
    photons[0, 0] = 3e3
    photons[1, n_e // 2:] = 0.0
    return dict(pathlen=pathlen.astype(F32), mu=mu.astype(F32), photons=photons.astype(F32), gain=E.astype(F32),
                n_materials=n_mat, n_energies=n_e, n_spectra=S, n_views=POISSON_SHAPE[0], n_rows=POISSON_SHAPE[1],
                n_channels=POISSON_SHAPE[2], layout=layout, view_offset=17, seed=SEEDS[1])
