"""What every polychromatic detection must return: the float64 sum over the energies of the kernel's own float32 path lengths, with
the error bound a float32 evaluation has to meet; the log sinogram's reference; the tables and scans of tests/test_gpu_detect.py;
float32 emulations of the four summation orders the kernels use and a list of subtly wrong variants of them.  Plain NumPy, no
device.  tests/test_detect_refs.py shows on the CPU that the bound holds for every emulated order, that it rejects every variant
of MUTANTS on inputs of the GPU matrix, and that the sweep reaches what it claims.

The detected signal of spectrum s on a ray with the per-material path lengths L[m] (table rows mu[m][e], weights w[s][e]):
    P_e = sum_m mu[m][e] L[m],   t_e = exp(-P_e),   exact[s] = sum_e w[s][e] t_e
The reference takes the float32 path lengths the kernel itself returns (pinned bit for bit to the oracle elsewhere in the suite)
and the float32 tables the kernel is given, and evaluates the sums in float64.  The variance is the same sum with w2 = w x gain.

The bound (u = 2^-24 the float32 unit round-off, M table rows, n_e energies; every constant derived, none measured):
    |got - exact[s]| <= u sum_e |w[s][e]| t_e ((M + 3.5) P_e + 2 + n_e)  +  2^-125 sum_e |w[s][e]|
  the exponent.  The kernels scale the lengths (wave_ray_kernel: the table) by the float32 log2(e) once: the constant is 0.3 u
      from log2(e), the product rounds (u): 1.3 u on every term.  The chain pe = fma(mu[M-1], L2[M-1], ... fma(mu[0], L2[0], 0))
      rounds M times (its first fma is exact up to the one rounding of the product); every term is non-negative, so every partial
      sum is at most the result and each rounding is at most u pe: M u, and with the second-order terms and the scaling
      (M + 2.5) u relative in the base-2 exponent.  2^(-pe) = exp(-pe ln 2) and ln 2 log2(e) = 1: an ABSOLUTE error
      (M + 2.5) u P_e of the natural exponent, a RELATIVE error of the same size on t_e.
      detect_store_lds and detect_kernel_chunked form the exponent in natural units and scale it afterwards, -p * kLog2e: the
      product is one further rounding of the whole exponent (the lengths are then unscaled, the constant's 0.3 u stays): M + 3.5
      serves every form.
  v_exp_f32 is accurate to 1 ulp (the public CDNA ISA guide) = 2 u relative on t_e.
  the weighted sum acc = fma(w[e], t_e, acc), n_e roundings of partial sums of non-negative terms (w >= 0 here; |w| in the bound):
      n_e u relative to the sum, charged to every term.  An even/odd pair of accumulators, a 64-lane strided sum and a shuffle tree
      round fewer times on the way of any one term (n_e / 2 + 2, n_e / 64 + 6): no worse.
  the absolute term: v_exp_f32 returns 0 for a result below 2^-126 (no denormals), so a term may be missing entirely; the
      exponent's own error moves the threshold by less than a factor 2.
  Where a path length of material 0 comes out a rounding below zero (chord minus the others) the bound uses |L| |mu|.

log_ref: ln(air / counts) of the counts the device returned, as np.log(np.float32(air) / counts) defines it.
  Where the float32 quotient is finite: |got - ln(air / counts)| <= 2^-22 (1 + |ln(air / counts)|): v_rcp_f32 (1 ulp) and the
  product (half an ulp) are 1.5 ulp = 3 u of the ratio, i.e. 3 u absolute on its logarithm; v_log_f32 1 ulp of its result and the
  product with the float32 ln 2 (constant and rounding, 1 ulp together) 4 u |ln|: below 4 u (1 + |ln|) = 2^-22 (1 + |ln|).
  Where the float32 quotient overflows or counts == 0: exactly +inf.  Never NaN.
"""
import os

import numpy as np

U = 2.0 ** -24
F16, F32, F64 = np.float16, np.float32, np.float64
TINY = 2.0 ** -126                                                           # below this v_exp_f32 returns 0
ABS_TERM = 2.0 ** -125
LOG2E = F32(1.44269504088896340736)
LOG_TOL = 2.0 ** -22


# ---- the references -------------------------------------------------------------------------------------------------------------

def exponents(pathlen, mu):
    """(P [rays][E], |P| [rays][E]) float64 from float32 pathlen [..., M] and mu [M][E]."""
    mu = np.asarray(mu, F32).astype(F64)
    pl = np.asarray(pathlen, F32).astype(F64).reshape(-1, mu.shape[0])
    return pl @ mu, np.abs(pl) @ np.abs(mu)


def detect_ref(pathlen, mu, w):
    """(exact, bound) float64 [S][rays] of the module docstring; pathlen [..., M] in the memory order of the rays."""
    w = np.asarray(w, F32).astype(F64)
    P, Pabs = exponents(pathlen, mu)
    M, n_e = np.shape(mu)
    t = np.exp(-P)
    aw = np.abs(w)
    exact = w @ t.T
    bound = U * (aw @ (t * ((M + 3.5) * Pabs + 2.0 + n_e)).T) + ABS_TERM * aw.sum(axis=1)[:, None]
    return exact, bound


def log_ref(air, counts):
    """(exact, bound) float64 [S][rays] for float32 counts [S][...]: +inf (bound 0) where np.float32(air) / counts is not finite
    in float32."""
    c = np.asarray(counts, F32)
    c = c.reshape(c.shape[0], -1)
    a = np.asarray(air, F64).astype(F32)[:c.shape[0], None]
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        finite = np.isfinite(a / c)                                          # the float32 quotient
        exact = np.where(finite, np.log(a.astype(F64) / np.where(finite, c, 1).astype(F64)), np.inf)
    return exact, np.where(finite, LOG_TOL * (1.0 + np.abs(np.where(finite, exact, 0.0))), 0.0)


def within(got, exact, bound):
    """|got - exact| <= bound everywhere, got finite and not negative."""
    g = np.asarray(got, F64).reshape(exact.shape)
    return bool(np.all(np.isfinite(g)) and np.all(g >= 0.0) and np.all(np.abs(g - exact) <= bound))


def worst(got, exact, bound):
    """Largest |got - exact| / bound (inf for a NaN)."""
    g = np.asarray(got, F64).reshape(exact.shape)
    q = np.abs(g - exact) / bound
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def log_within(got, exact, bound):
    """+inf exactly where the reference is, within the bound elsewhere, never NaN."""
    g = np.asarray(got, F64).reshape(exact.shape)
    inf = np.isinf(exact)
    return bool(not np.any(np.isnan(g)) and np.all(g[inf] == np.inf) and np.all(np.isfinite(g[~inf]))
                and np.all(np.abs(g[~inf] - exact[~inf]) <= bound[~inf]))


def log_worst(got, exact, bound):
    g = np.asarray(got, F64).reshape(exact.shape)
    fin = np.isfinite(exact)
    return float(np.max(np.abs(g[fin] - exact[fin]) / bound[fin])) if fin.any() else 0.0


# ---- the tables of the sweep ----------------------------------------------------------------------------------------------------

STEPS = (0, 1, 10, 40, 80, 120, 'steep')                                     # the largest exponent of the scan, or the steep table
AIR_BASE = 0.03


def base_rows(n_mat):
    """Relative attenuation of the table rows: air 0.03, the others 0.7 .. 1.0 (a narrow band, so that the thickest rays of the
    step-120 table lose every energy)."""
    base = 0.7 + 0.3 * np.modf(0.6180339887498949 * np.arange(n_mat))[0]
    base[0] = AIR_BASE
    return base


def p_unit(pathlen, n_mat):
    """The largest exponent over all rays of the unscaled base table (whose largest shape value is 1): max_ray sum_m L[m] base[m]."""
    pl = np.asarray(pathlen, F32).astype(F64).reshape(-1, n_mat)
    return float(np.max(pl @ base_rows(n_mat)))


def weights(n_e, n_s):
    """w [S][E] float32, positive, with the zero patterns of test_detection_skips_only_exact_zeros over blocks of four energies:
    whole blocks, part blocks, -0.0, a slot that ends early.  Blocks 0 and 1, the last whole block, the blocks from 64 on and the
    tail of an energy count that is no multiple of 4 stay weighted in every slot but the one that ends early."""
    rng = np.random.default_rng(n_e * 10 + n_s)
    w = rng.uniform(0.5, 2.0, (n_s, n_e)).astype(F32)
    n_blk = n_e // 4
    for s in range(n_s):
        for b in range(2, min(n_blk - 1, 64)):
            r, q = rng.random(), slice(4 * b, 4 * b + 4)
            if b == 2 + s or r < 0.25:
                w[s, q] = 0.0                                                # a whole block
            elif b == 5 or r < 0.35:
                w[s, 4 * b:4 * b + 2] = 0.0                                  # part of a block: not skippable
            elif b == 7 + s or r < 0.42:
                w[s, q] = -0.0                                               # sign bit set: runs, adds nothing
    if n_s == 2 and n_e >= 64:
        w[1, 32:] = 0.0                                                      # a slot that ends early
    return w


def gain(n_e):
    return 20.0 + 120.0 * np.linspace(0.0, 1.0, n_e)


def sweep_tables(n_mat, n_e, n_s, step, p_unit_):
    """(mu [M][E], w [S][E], w2 [S][E]) float32.  mu[m][e] = base[m] shape[e] k(step) with row 0 (air) scaled like the others;
    k puts the largest exponent of the scan at ``step``; 'steep': log-spaced over the energies from 1e-3 to 120 / p_unit."""
    base = base_rows(n_mat)
    if step == 'steep':
        col = np.logspace(-3.0, np.log10(120.0), n_e) if n_e > 1 else np.array([120.0])
    else:
        col = (1.0 - 0.15 * np.linspace(0.0, 1.0, n_e)) * float(step)
    mu = (base[:, None] * col[None, :] / p_unit_).astype(F32)
    w = weights(n_e, n_s)
    return mu, w, (w.astype(F64) * gain(n_e)).astype(F32)


# ---- float32 emulations of the kernels' summation orders -------------------------------------------------------------------------

ORDERS = ('loop', 'pairs', 'natural', 'tree')
# loop: detect_energies (detect_store, detect_store1, rows16_kernel, detect_kernel, the scalar cone loop); pairs: detect_energy_pairs;
# natural: detect_store_lds, detect_kernel_chunked; tree: wave_ray_kernel


def fma(a, b, c):
    """Round-to-float32 of the float64 a * b + c."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def mul(a, b):
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def to_bf16(x):
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16                         # round to nearest even
    return b.astype(np.uint32).view(F32).reshape(np.shape(x))


def exp2_f32(x, ulp):
    """v_exp_f32's model: the correctly rounded 2^x moved by ``ulp`` (-1, 0, +1 per element) float32 steps, 0 below 2^-126."""
    with np.errstate(under='ignore'):
        t = np.exp2(np.asarray(x, F32).astype(F64)).astype(F32)
    ulp = np.broadcast_to(np.asarray(ulp), t.shape)
    t = np.where(ulp > 0, np.nextafter(t, F32(np.inf)), np.where(ulp < 0, np.nextafter(t, F32(0.0)), t)).astype(F32)
    return np.where(t < F32(TINY), F32(0.0), t)


def _exponent(L, mu, order, mutant):
    """The base-2 exponent pe [rays][E] float32 (>= 0) of every ray and energy."""
    n, M = L.shape
    rows = range(M - 1) if mutant == 'drop_last_material' else range(M)
    pe = np.zeros((n, mu.shape[1]), F32)
    if mutant == 'f16_exponent':                                             # no fma, a half-precision accumulator
        L2 = mul(L, LOG2E)
        acc = pe.astype(F16)
        for m in rows:
            acc = (acc + mul(mu[m][None, :], L2[:, m, None]).astype(F16)).astype(F16)
        return acc.astype(F32)
    scale_first = order != 'natural'
    if mutant == 'log2e_never':
        Lm, mum, scale_first = L, mu, True
    elif order == 'tree':
        Lm, mum = L, mul(mu, LOG2E)                                          # the table is scaled as it is staged
    elif scale_first:
        Lm, mum = mul(L, LOG2E), mu
    else:
        Lm, mum = L, mu
    for m in rows:
        pe = fma(mum[m][None, :], Lm[:, m, None], pe)
    if not scale_first:
        pe = mul(pe, LOG2E)
    if mutant == 'log2e_twice':
        pe = mul(pe, LOG2E)
    return pe


def _live(w, mutant):
    """Which (slot, energy) terms are accumulated.  The kernels skip blocks of four energies whose weights are all +0, which
    changes no bit, so the faithful emulation accumulates everything."""
    S, n_e = w.shape
    live = np.ones((S, n_e), bool)
    if mutant == 'drop_tail':
        live[:, 4 * (n_e // 4):] = False
    elif mutant == 'drop_last_block':
        live[:, 256:] = False
    elif mutant == 'skip_nonzero_block':
        live[:, 4:8] = False
    elif mutant == 'negzero_ends_slot':
        bits = np.ascontiguousarray(w).view(np.uint32)
        for s in range(S):
            for b in range(n_e // 4):
                if np.all(bits[s, 4 * b:4 * b + 4] == 0x80000000):
                    live[s, 4 * b:] = False
                    break
    return live


def _sum(t, w, live, order):
    """sum_e w[s][e] t[ray][e] in the order of the kernel: [S][rays] float32."""
    S, n_e = w.shape
    n = t.shape[0]

    def run(acc, es):
        for e in es:
            new = fma(w[:, e, None], t[None, :, e], acc)
            acc = np.where(live[:, e, None], new, acc)
        return acc
    zero = np.zeros((S, n), F32)
    if order in ('loop', 'natural'):
        return run(zero, range(n_e))
    if order == 'pairs':
        n4 = 4 * (n_e // 4)
        even, odd, tail = run(zero, range(0, n4, 2)), run(zero, range(1, n4, 2)), run(zero, range(n4, n_e))
        return ((even + odd).astype(F32) + tail).astype(F32)
    if order == 'tree':
        lanes = np.zeros((S, n, 64), F32)
        for e0 in range(0, n_e, 64):
            k = min(64, n_e - e0)
            new = fma(w[:, None, e0:e0 + k], t[None, :, e0:e0 + k], lanes[:, :, :k])
            lanes[:, :, :k] = np.where(live[:, None, e0:e0 + k], new, lanes[:, :, :k])
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[:, :, idx ^ o]).astype(F32)
        return lanes[:, :, 0]
    raise ValueError(order)


def emulate(pathlen, mu, w, order, ulp=0, mutant=None):
    """The detection of ``order`` in float32: [S][rays].  ``ulp``: the offsets of the exponential, a scalar or [rays][E]."""
    mu, w = np.asarray(mu, F32), np.asarray(w, F32)
    L = np.asarray(pathlen, F32).reshape(-1, mu.shape[0])
    if mutant == 'bf16_tables':
        mu, w = to_bf16(mu), to_bf16(w)
    if mutant == 'odd_ray_gets_even_lengths':
        L = L.copy()
        k = L.shape[0] // 2
        L[1:2 * k:2] = L[0:2 * k:2]
    if mutant == 'slot1_reads_slot0':
        w = w.copy()
        w[1] = w[0]
    pe = _exponent(L, mu, order, mutant)
    t = exp2_f32(-pe, ulp)
    if mutant == 'exp_rel_2m18':
        t = (t.astype(F64) * (1.0 + 2.0 ** -18)).astype(F32)
    return _sum(t, w, _live(w, mutant), order)


def air_only(pathlen, n_mat):
    pl = np.asarray(pathlen, F32).reshape(-1, n_mat)
    return np.all(pl[:, 1:] == 0.0, axis=1) & (pl[:, 0] > 0.0)


def longest_air_run(pathlen, n_mat):
    """Most consecutive air-only rays (positive air length) in the memory order of ``pathlen``."""
    best = run = 0
    for a in air_only(pathlen, n_mat):
        run = run + 1 if a else 0
        best = max(best, run)
    return best


MUTANTS = ('drop_tail', 'drop_last_block', 'slot1_reads_slot0', 'odd_ray_gets_even_lengths', 'drop_last_material', 'log2e_twice',
           'log2e_never', 'skip_nonzero_block', 'negzero_ends_slot', 'variance_with_w', 'variance_from_slot0', 'air_shortcut_speck',
           'stale_air_cache', 'bf16_tables', 'exp_rel_2m18', 'f16_exponent')
PRECISION_MUTANTS = ('bf16_tables', 'exp_rel_2m18', 'f16_exponent')


def run_mutant(name, pathlen, mu, w, w2, order):
    """One wrong detection on the inputs of a launch: (got [S][rays] float32, the path lengths the launch had, the weights its
    result stands for) - the last two are what detect_ref is asked for - or None where the variant does not apply."""
    M, n_e = np.shape(mu)
    S = np.shape(w)[0]
    L = np.asarray(pathlen, F32).reshape(-1, M)
    if name == 'drop_tail' and n_e % 4 == 0 or name == 'drop_last_block' and n_e <= 256:
        return None
    if name in ('slot1_reads_slot0', 'variance_from_slot0') and S < 2:
        return None
    if name == 'skip_nonzero_block' and n_e < 8:
        return None
    if name == 'variance_with_w':                                            # the variance summed with w instead of w2
        return emulate(L, mu, w, order), L, w2
    if name == 'variance_from_slot0':                                        # both slots hand out the first slot's variance
        v = emulate(L, mu, w2, order)
        return np.broadcast_to(v[0], v.shape).copy(), L, w2
    if name in ('air_shortcut_speck', 'stale_air_cache'):
        air = np.flatnonzero(air_only(L, M))
        if air.size < 8:
            return None
        if name == 'air_shortcut_speck':
            # one ray of an air-only lane meets 1e-3 cm of material 1: the lane still takes the shortcut (the value of its first ray)
            L = L.copy()
            L[air[1::4], 1] = F32(1e-3)
            got = emulate(L, mu, w, order)
            got[:, air[1::4]] = got[:, air[0::4][:air[1::4].size]]
            return got, L, w
        got = emulate(L, mu, w, order)                                       # the cache is never invalidated: the first air value
        got[:, air] = got[:, air[:1]]
        return got, L, w
    return emulate(L, mu, w, order, mutant=name), L, w


# ---- the scans and the matrix of tests/test_gpu_detect.py ------------------------------------------------------------------------

INPUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dex-ct-sim_amd', 'input')
N_VIEWS, N_CHANNELS = 5, 37
SCANS = {                    # n_rows, nz, z_index, cone
    'row1': (1, 1, 0, False), 'rows64': (64, 64, 0, False), 'rows66': (66, 70, 2, False),
    'cone12': (12, 24, 0, True), 'cone40': (40, 24, 0, True)}
CONE = dict(cone12=dict(h_iso=0.8, src_z=0.3), cone40=dict(h_iso=0.5, src_z=0.3))


def scan(key, n_mat):
    """(ct, ph) of a scan of the matrix: small_scan(n=40), 5 views, 37 channels; every non-air voxel scrambled over the n_mat - 1
    materials (tests/test_gpu_siddon.py ph_many) with one speck of every id in every imaged slice, so that every table row is
    crossed."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import synthetic
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    n_rows, nz, z_index, cone = SCANS[key]
    det = os.path.join(INPUT, 'detector', 'eta_eid_mv.bin')
    kw = dict(N_channels=N_CHANNELS, N_proj=N_VIEWS, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True, detector_file=det,
              N_rows=n_rows)
    ct = dx.FanBeamGeometry(cone=True, **CONE[key], **kw) if cone else dx.FanBeamGeometry(**kw)
    ph = synthetic.make_phantom(40, nz, seed=1234, z_index=z_index)
    rng = np.random.default_rng(11)
    vol = np.where(ph.volume > 0, rng.integers(1, n_mat, ph.volume.shape, dtype=np.uint8), 0).astype(np.uint8)
    ids = np.arange(1, n_mat)
    for z in range(nz):                                                      # the specks: a block of 8 x 8 voxels at the centre
        vol[z, 16 + (ids + z) % 64 // 8, 16 + (ids + z) % 8] = ids
    ph.volume = vol
    ph.materials = ([AIR, WATER, BONE] + [Material(f'm{i}', 1.0 + 0.1 * i, 'H(11.2)O(88.8)') for i in range(3, n_mat)])[:n_mat]
    return ct, ph


def memory_layout(key):
    """The ray order of the kernels that serve the scan: 1 ([view][channel][row]) for the row-parallel kernels of the multi-row
    fans, 0 for the single row and the cone beam."""
    return 1 if key in ('rows64', 'rows66') else 0


_pathlen = {}


def oracle_pathlen(key, n_mat, layout=None):
    """The float32 path lengths [rays][M] of the scan from the C oracle's mirror of the kernel arithmetic - the values the device
    returns bit for bit - in the ray order of ``layout`` (default: memory_layout)."""
    from oracle import c_oracle as co
    if (key, n_mat) not in _pathlen:
        ct, ph = scan(key, n_mat)
        n_rows, nz, z_index, cone = SCANS[key]
        g = co.make_geom(ct.N_proj, ct.N_channels, ct.N_rows, 0 if cone else z_index, ph.Nx, ph.Ny, ph.Nz, ph.dx, ph.dy, ph.dz,
                         ct.SID, ct.SDD)
        mu, w = np.ones((n_mat, 1)), np.ones((1, 1))
        if cone:
            _, pl = co.project_cone(g, ct.view_cs(), ct.chan_cs(), 0, ct.N_proj, ct.row_z(), ct.src_z, ph.volume, mu, w, dda=True,
                                    n_threads=8)
        else:
            _, pl = co.project_dda(g, ct.view_cs(), ct.chan_cs(), 0, ct.N_proj, ph.volume, mu, w, True, n_threads=8)
        _pathlen[key, n_mat] = pl
    pl = _pathlen[key, n_mat]
    if (memory_layout(key) if layout is None else layout) == 1:
        pl = pl.transpose(0, 2, 1, 3)
    return np.ascontiguousarray(pl).reshape(-1, n_mat)


# (form, scan, kernel, M, n_e, n_s, order of the emulation, run on the CPU too).  Every form meets every energy count of
# 3, 7, 64, 139, 300 and every spectrum count it admits once.  kernel 7: also DEXCT_P16_STAGED 0 and 1.
CASES = [
    ('detect_store1', 'row1', 1, 2, 3, 1, 'loop', True),
    ('detect_store1', 'row1', 2, 3, 7, 2, 'loop', True),
    ('detect_store1', 'rows66', 2, 4, 64, 3, 'loop', False),
    ('detect_store1', 'row1', 1, 3, 139, 4, 'loop', True),
    ('detect_store1', 'row1', 2, 4, 300, 2, 'loop', True),
    ('detect_store_lds', 'row1', 1, 5, 3, 2, 'natural', True),
    ('detect_store_lds', 'row1', 2, 13, 7, 1, 'natural', True),
    ('detect_store_lds', 'row1', 1, 49, 64, 3, 'natural', True),
    ('detect_store_lds', 'row1', 2, 60, 139, 4, 'natural', True),
    ('detect_store_lds', 'rows66', 2, 5, 300, 2, 'natural', False),
    ('detect_store4', 'rows64', 3, 3, 7, 2, 'loop', True),
    ('detect_store4', 'rows64', 5, 2, 3, 1, 'loop', True),
    ('detect_store4', 'rows66', 3, 4, 139, 2, 'loop', False),
    ('detect_store4', 'rows64', 5, 4, 64, 3, 'loop', False),
    ('detect_store4', 'rows64', 3, 2, 300, 4, 'loop', False),
    ('detect_store4', 'rows64', 3, 3, 300, 2, 'loop', False),
    ('wave_ray_kernel', 'row1', 6, 3, 3, 1, 'tree', True),
    ('wave_ray_kernel', 'row1', 6, 4, 7, 2, 'tree', True),
    ('wave_ray_kernel', 'row1', 6, 3, 64, 3, 'tree', True),
    ('wave_ray_kernel', 'row1', 6, 4, 139, 4, 'tree', True),
    ('wave_ray_kernel', 'row1', 6, 3, 300, 2, 'tree', True),
    ('rows16_kernel', 'rows64', 7, 3, 7, 2, 'loop', False),
    ('rows16_kernel', 'rows64', 7, 2, 3, 1, 'loop', False),
    ('rows16_kernel', 'rows66', 7, 4, 139, 2, 'loop', True),
    ('rows16_kernel', 'rows64', 7, 3, 300, 3, 'loop', False),
    ('rows16_kernel', 'rows64', 7, 4, 64, 4, 'loop', False),
    ('detect_kernel', 'rows64', 4, 5, 7, 2, 'loop', True),
    ('detect_kernel', 'rows66', 8, 5, 3, 1, 'loop', True),
    ('detect_kernel', 'rows64', 8, 16, 64, 3, 'loop', False),
    ('detect_kernel', 'rows66', 4, 17, 7, 4, 'loop', False),
    ('detect_kernel', 'rows64', 4, 17, 139, 2, 'loop', False),
    ('detect_kernel', 'rows64', 8, 32, 3, 2, 'loop', False),
    ('detect_kernel', 'rows66', 8, 33, 7, 1, 'loop', False),
    ('detect_kernel', 'rows66', 4, 32, 64, 2, 'loop', False),
    ('detect_kernel', 'rows64', 4, 33, 3, 3, 'loop', False),
    ('detect_kernel', 'rows64', 4, 48, 300, 2, 'loop', False),
    ('detect_kernel', 'rows66', 8, 48, 7, 2, 'loop', False),
    ('detect_kernel', 'rows66', 8, 16, 139, 2, 'loop', False),
    ('detect_kernel_chunked', 'rows64', 4, 49, 64, 2, 'natural', False),
    ('detect_kernel_chunked', 'rows66', 8, 60, 7, 3, 'natural', True),
    ('detect_kernel_chunked', 'rows64', 8, 49, 3, 1, 'natural', True),
    ('detect_kernel_chunked', 'rows64', 4, 60, 139, 4, 'natural', False),
    ('detect_kernel_chunked', 'rows66', 4, 49, 300, 2, 'natural', False),
    ('detect_energy_pairs', 'cone12', 1, 2, 3, 1, 'pairs', True),
    ('detect_energy_pairs', 'cone40', 2, 3, 7, 2, 'pairs', True),
    ('detect_energy_pairs', 'cone12', 2, 3, 300, 2, 'pairs', True),
    ('detect_energy_pairs', 'cone40', 1, 2, 139, 2, 'pairs', True),
    ('detect_energy_pairs', 'cone12', 1, 3, 64, 1, 'pairs', True),
    ('cone_scalar_loop', 'cone12', 1, 3, 64, 3, 'loop', True),
    ('cone_scalar_loop', 'cone40', 2, 2, 139, 4, 'loop', False),
    ('cone_groups', 'cone40', 2, 4, 7, 2, 'loop', True),
    ('cone_groups', 'cone12', 2, 7, 64, 1, 'loop', True),
    ('cone_groups', 'cone40', 2, 50, 3, 3, 'natural', True),
    ('cone_groups', 'cone12', 2, 7, 139, 4, 'loop', False),
    ('cone_groups', 'cone40', 2, 4, 300, 2, 'loop', False),
]


def case_id(case):
    form, key, kernel, M, n_e, n_s = case[:6]
    return f'{form}-{key}-k{kernel}-M{M}-E{n_e}-S{n_s}'


def case_tables(case, pathlen):
    """The seven (step, mu, w, w2) of a case of the matrix."""
    _, _, _, M, n_e, n_s = case[:6]
    pu = p_unit(pathlen, M)
    return [(step,) + sweep_tables(M, n_e, n_s, step, pu) for step in STEPS]
