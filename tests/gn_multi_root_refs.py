"""What dexct_gn_decompose_multi (csrc/gn_multi.hip) must return, from outside float64: the root of the Poisson likelihood's
gradient in long double, an error scale per pixel and component, the long-double trajectory of the first Newton steps, a
float64 emulation of the kernel's own order of operations with wrong variants of it, and the cases all of this is asked on.
Plain NumPy, no device, no library.  tests/test_gn_multi_root_refs.py shows on the CPU that the references are usable on these
cases and that the comparisons reject the wrong variants; tests/test_gpu_gn_multi_root.py holds the kernel to them.

Arithmetic (``terms``), in float64 or np.longdouble, for states a [P, M], counts g [K, P], tables i0 [K, nE], mus [M, nE]:
    t = exp(-a . mus);  nu_k = sum_e i0_k t;  G_km = sum_e i0_k mu_m t;  S_kmn = sum_e i0_k mu_m mu_n t
    c_k = g_k / nu_k - 1;  q_k = g_k / nu_k^2;  dF_m = sum_k c_k G_km;  H_mn = sum_k (q_k G_km G_kn - c_k S_kmn);  a -= H^-1 dF
with H^-1 through the adjugate (gn_cov_refs.sym_inverse), so that the same code runs in either precision.  Every sum over the
energies is NumPy's pairwise one.  No exponent is clipped: the largest of all cases is below 30 (``largest_exponent``).

The root (``reference``).  The float64 restatement gn_multi_refs.newton_solve_multi after 50 steps, polished by full Newton steps
in long double, at most POLISH_STEPS, until a step is at the long-double rounding limit of its pixel,
|step_m| <= 8 * 2^-63 * (|H^-1| s)_m.

The error scale, per pixel and component:  scale_m = 2^-53 sum_n |H^-1|_mn s_n,  s_n = sum_k (g_k / nu_k + 1) G_kn,  everything
at the root in long double: what one float64 rounding of each term of the gradient sum_k (g_k / nu_k - 1) G_kn can move the
root by.  ``ratio`` = |a - root|_m / scale_m.

Usable pixels: the restatement ended finite, its steps 49 and 50 agree within 1e-9 max(|a|, 1), the polish reached its stop,
and the walk that led there is determined by float64 arithmetic (``walk_is_determined``: at none of its 50 states does one
rounding of the gradient move the next state by more than 1e-9 max(|a|, 1)).  The fourth condition was added on evidence from
this file alone: on pixel 762 of 'wide K=3 M=3 nE=8 noisy' the walk crosses a Hessian with a condition number of 1e15 at its
12th state; the restatement goes on to the root, the emulation of the kernel's order with every exponential one ulp up ends
NaN, one ulp down at the root again - "50 steps from 1e-6" has no float64 value there that a kernel could be held to.  The
condition sets aside 2 of the 104 128 pixels of all cases and count types (both in that case); the other three 3 (the same case).
At most UNUSABLE_CAP = 1 % of a case may be unusable; that is a condition on the cases below, not a measurement.

The allowance ``C`` = 4 x the worst ratio, over the wide and the gaps cases, of the restatement and of the three emulations
(every exponential one ulp up, one ulp down, and up or down by a seeded sign per energy).  It is computed on the CPU when this
module is imported and never from a device result.  The factor 4 is the one gn_cov_refs.sweep_ratio_f64 grants the sibling
kernel, for the same reasons: another summation order, a refined v_rcp_f64, a table exponential.

Early iterates (``trajectory``): the long-double states after 1, 2 and 3 steps from 1e-6; a pixel is usable when the float64
restatement agrees with all three within EARLY_USABLE = 1e-11 max(|a|, 1); the same 1 % cap.  The device is held to them at
the project's 1e-9 max(|a|, 1) (TOL of tests/test_gpu_gn_multi.py).
"""
import numpy as np

import gn_multi_refs as mr
from gn_cov_refs import sym_inverse

LD = np.longdouble
F64 = np.float64
if np.finfo(LD).nmant < 63:
    raise RuntimeError(f'gn_multi_root_refs needs a long double with a 64-bit mantissa; this platform has {np.finfo(LD).nmant + 1} bits')

A_WIDE = (45.0, 10.0, 0.3)         # upper ends of the line integrals [g/cm^2]: water-like, bone-like, K-edge material
WIDE_ENERGIES = (8, 49, 239)
N_PIX = 1000
CAP_ENERGIES = 4096                # kMaxEnergies of csrc/gn_pixel.h
CAP_PIXELS = 64
POLISH_STEPS = 12
UNUSABLE_CAP = 0.01
EARLY_STEPS = (1, 2, 3)
EARLY_USABLE = 1e-11
EARLY_TOL = 1e-9
ARRIVED = 1e-9
WARM_STEPS = 40                    # the emulation takes over from the restatement here (see ``emulate``)
FACTOR = 4.0
EXP_SCALE = float.fromhex('0x1.71547652b82fep+11')      # 2048 / ln 2 as csrc/exp_table.h has it
LN2_LD = np.log(LD(2.0))


# ---------------------------------------------------------------------------------------------------------------- arithmetic

def _pairs(M):
    return [(m, n) for m in range(M) for n in range(m, M)]


def sums(a, i0, mus, dtype=F64):
    """nu [P, K], G [P, K, M], S [P, K, M, M] at the states a [P, M], in ``dtype``; each a pairwise sum over the energies"""
    a, i0, mus = (np.asarray(x, dtype=dtype) for x in (a, i0, mus))
    K, M, P = i0.shape[0], mus.shape[0], a.shape[0]
    with np.errstate(all='ignore'):
        t = np.exp(-(a @ mus))                                               # [P, nE]
        nu, G, S = np.empty((P, K), dtype), np.empty((P, K, M), dtype), np.empty((P, K, M, M), dtype)
        for k in range(K):
            tk = t * i0[k]
            nu[:, k] = tk.sum(axis=1)
            for m in range(M):
                G[:, k, m] = (tk * mus[m]).sum(axis=1)
            for m, n in _pairs(M):
                S[:, k, m, n] = S[:, k, n, m] = (tk * (mus[m] * mus[n])).sum(axis=1)
    return nu, G, S


def terms(a, g, i0, mus, dtype=F64):
    """(nu, G, S, dF [P, M], H [P, M, M]) at the states a [P, M] for the counts g [K, P], in ``dtype``"""
    gp = np.asarray(g, dtype=dtype).T                                        # [P, K]
    nu, G, S = sums(a, i0, mus, dtype)
    with np.errstate(all='ignore'):
        c = gp / nu - 1.0
        q = gp / (nu * nu)
        dF = np.einsum('pk,pkm->pm', c, G)
        H = np.einsum('pk,pkm,pkn->pmn', q, G, G) - np.einsum('pk,pkmn->pmn', c, S)
    return nu, G, S, dF, H


def newton_step(a, g, i0, mus, dtype=F64):
    """one full Newton step from a [P, M], in ``dtype``"""
    a = np.asarray(a, dtype=dtype)
    _, _, _, dF, H = terms(a, g, i0, mus, dtype)
    with np.errstate(all='ignore'):
        return a - np.einsum('pmn,pn->pm', sym_inverse(H), dF)


def step_and_scale(a, g, i0, mus):
    """(step [P, M], reach [P, M] = (|H^-1| s)_m) at a, in long double; s_n = sum_k (g_k / nu_k + 1) G_kn"""
    nu, G, _, dF, H = terms(a, g, i0, mus, LD)
    with np.errstate(all='ignore'):
        Hi = sym_inverse(H)
        s = np.einsum('pk,pkn->pn', np.asarray(g, dtype=LD).T / nu + 1.0, G)
        return np.einsum('pmn,pn->pm', Hi, dF), np.einsum('pmn,pn->pm', np.abs(Hi), s)


def polish(a0, g, i0, mus):
    """(root [P, M] long double, stopped [P]): full long-double Newton steps from a0 until |step_m| <= 8 * 2^-63 (|H^-1| s)_m
    in every component, at most POLISH_STEPS; pixels that start non-finite are left alone and never stop"""
    a = np.array(a0, dtype=LD)
    g = np.asarray(g, dtype=LD)
    stopped = np.zeros(len(a), bool)
    live = np.all(np.isfinite(a), axis=1)
    for _ in range(POLISH_STEPS):
        idx = np.flatnonzero(live & ~stopped)
        if not idx.size:
            break
        step, reach = step_and_scale(a[idx], g[:, idx], i0, mus)
        with np.errstate(all='ignore'):
            a[idx] = a[idx] - step
            ok = np.all(np.abs(step) <= LD(8.0) * LD(2.0) ** -63 * reach, axis=1)
        stopped[idx] = ok
        live[idx] = np.all(np.isfinite(a[idx]), axis=1)
    return a, stopped


def walk_is_determined(g, i0, mus, n_iters=50):
    """[P]: at every one of the n_iters states of the float64 walk from 1e-6, one float64 rounding of each term of the gradient
    moves the next state by at most ARRIVED max(|a|, 1):  2^-53 (|H^-1| s)_m <= 1e-9 max(|a_m|, 1),  H and s at that state.
    A walk that crosses a nearly singular Hessian fails this at the crossing: where it goes from there - to the root, to
    another stationary point, to NaN - is decided by the last bits of the sums, differently for every order of summation.
    (The restatement's arithmetic with the adjugate for the solve; the threshold is nine orders above the usual reach.)"""
    g, i0, mus = (np.asarray(x, dtype=F64) for x in (g, i0, mus))
    K, M, nE = i0.shape[0], mus.shape[0], mus.shape[1]
    gp = g.T
    w1 = (i0[:, None, :] * mus[None, :, :]).reshape(K * M, nE)
    w2 = (i0[:, None, None, :] * (mus[None, :, :] * mus[:, None, :])[None]).reshape(K * M * M, nE)
    a = np.full((gp.shape[0], M), 1e-6)
    ok = np.ones(len(a), bool)
    with np.errstate(all='ignore'):
        for _ in range(n_iters):
            at = np.exp(-(a @ mus))
            nu = at @ i0.T
            G = (at @ w1.T).reshape(-1, K, M)
            S = (at @ w2.T).reshape(-1, K, M, M)
            c = gp / nu - 1.0
            Hi = sym_inverse(np.einsum('pk,pkm,pkn->pmn', gp / (nu * nu), G, G) - np.einsum('pk,pkmn->pmn', c, S))
            reach = np.einsum('pmn,pn->pm', np.abs(Hi), np.einsum('pk,pkn->pn', c + 2.0, G))
            ok &= np.all(2.0 ** -53 * reach <= ARRIVED * np.maximum(np.abs(a), 1.0), axis=1)
            a = a - np.einsum('pmn,pn->pm', Hi, np.einsum('pk,pkm->pm', c, G))
    return ok


def reference(g, i0, mus):
    """{'root' [P, M] long double, 'scale' [P, M] long double, 'usable' [P], 'a50' / 'a40' [P, M] the restatement's 50 / 40
    steps, 'reproducible' [P] = walk_is_determined, 'three' [P] = the other three conditions} for the float64 counts g [K, P]"""
    g = np.asarray(g, dtype=F64)
    a40 = mr.newton_solve_multi(g, i0, mus, WARM_STEPS)
    a49 = mr.newton_solve_multi(g, i0, mus, 49)
    a50 = mr.newton_solve_multi(g, i0, mus, 50)
    with np.errstate(all='ignore'):
        finite = np.all(np.isfinite(a50), axis=1)
        arrived = np.all(np.abs(a50 - a49) <= ARRIVED * np.maximum(np.abs(a50), 1.0), axis=1)
    reproducible = walk_is_determined(g, i0, mus)
    root, stopped = polish(a50, g, i0, mus)
    _, reach = step_and_scale(root, g, i0, mus)
    scale = LD(2.0) ** -53 * reach
    with np.errstate(all='ignore'):
        usable = finite & arrived & stopped & reproducible & np.all(np.isfinite(root), axis=1) & np.all(scale > 0, axis=1)
    return {'root': root, 'scale': scale, 'usable': usable, 'a50': a50, 'a40': a40, 'reproducible': reproducible,
            'three': finite & arrived & stopped}


def ratios(a, ref, n_pix=None):
    """|a - root|_m / scale_m [n, M] on the first n_pix pixels of the reference; unusable pixels give 0, NaN stays NaN"""
    n = len(a) if n_pix is None else n_pix
    with np.errstate(all='ignore'):
        r = (np.abs(np.asarray(a[:n], dtype=LD) - ref['root'][:n]) / ref['scale'][:n]).astype(F64)
    return np.where(ref['usable'][:n, None], r, 0.0)


def worst_ratio(a, ref, n_pix=None):
    """the largest of ``ratios``; NaN when a usable pixel is not finite"""
    r = ratios(a, ref, n_pix)
    return float('nan') if np.isnan(r).any() else float(r.max(initial=0.0))


def trajectory(g, i0, mus, steps=EARLY_STEPS):
    """{'a': {n: [P, M] long double after n steps from 1e-6}, 'usable' [P]}: usable where the float64 restatement agrees with
    every one of them within EARLY_USABLE max(|a|, 1)"""
    g = np.asarray(g, dtype=F64)
    a = np.full((g.shape[1], np.shape(mus)[0]), LD(F64(1e-6)), dtype=LD)
    out, usable = {}, np.ones(g.shape[1], bool)
    for n in range(1, max(steps) + 1):
        a = newton_step(a, g, i0, mus, LD)
        if n in steps:
            out[n] = a
            usable &= early_ok(mr.newton_solve_multi(g, i0, mus, n), a, EARLY_USABLE)
    return {'a': out, 'usable': usable}


def early_ok(a, ld, tol):
    """[P]: |a - ld| <= tol max(|ld|, 1) in every component (False for NaN)"""
    with np.errstate(all='ignore'):
        return np.all(np.abs(np.asarray(a, dtype=LD) - ld) <= LD(tol) * np.maximum(np.abs(ld), 1.0), axis=1)


def early_err(a, traj, n, n_pix=None):
    """max over the usable pixels and components of |a - ld_n| / max(|ld_n|, 1); NaN there gives NaN"""
    m = len(a) if n_pix is None else n_pix
    ld, use = traj['a'][n][:m], traj['usable'][:m]
    with np.errstate(all='ignore'):
        e = (np.abs(np.asarray(a[:m], dtype=LD) - ld) / np.maximum(np.abs(ld), 1.0)).astype(F64)[use]
    return float('nan') if np.isnan(e).any() else float(e.max(initial=0.0))


def largest_exponent(case):
    """the largest a . mus(e) over the case's true line integrals and energies"""
    return float(np.max(case['a_true'] @ case['mus']))


# --------------------------------------------------------------------------------------------------------------------- cases

def _wide_inputs(K, M, n_e, n_pix, seed, hard=False):
    E, mus3, S = mr.synthetic_tables(n_e)
    S = S * (60.0 / n_e)
    if hard:
        edges = mr.EDGES[K]
        i0 = np.stack([np.where((E >= lo) & (E < hi), S, 0.0) for lo, hi in zip(edges[:-1], edges[1:])])
    else:
        i0 = mr.synthetic_bins(E, S, mr.EDGES[K])
    mus = np.ascontiguousarray(mus3[:M])
    rng = np.random.default_rng([seed, K, M, n_e])
    a_true = rng.uniform(0.0, 1.0, (n_pix, M)) * np.array(A_WIDE[:M])
    return i0, mus, a_true, rng


def _case(name, K, M, i0, mus, a_true, g):
    return {'name': name, 'K': K, 'M': M, 'i0': i0, 'mus': mus, 'a_true': a_true, 'g': g}


def wide_case(K, M, n_e, noise, n_pix=N_PIX):
    """line integrals uniform in [0, A_WIDE] on the synthetic soft-edged bins at n_e energies; clean or gn_multi_refs.noisy counts"""
    i0, mus, a_true, rng = _wide_inputs(K, M, n_e, n_pix, 31)
    g = mr.forward_counts(a_true, i0, mus)
    return _case(f'wide K={K} M={M} nE={n_e} {"noisy" if noise else "clean"}', K, M, i0, mus, a_true, mr.noisy(g, rng) if noise else g)


GAP_FIRST, GAP_LEN = 23, 5


def gaps_case(K, M, odd, noise):
    """The wide case at 60 energies with hard-edged bins: every weight outside a measurement's window is an exact zero.  Five
    consecutive interior energies (GAP_FIRST ..) are weighted by no measurement, the last energy is weighted by none either (the
    synthetic spectrum ends in an exact 0 at 140 keV), and with ``odd`` the first energy is taken out too: 54 energies in use,
    or 53.  Every energy in use is weighted by exactly one measurement."""
    i0, mus, a_true, rng = _wide_inputs(K, M, 60, N_PIX, 32, hard=True)
    i0[:, GAP_FIRST:GAP_FIRST + GAP_LEN] = 0.0
    if odd:
        i0[:, 0] = 0.0
    g = mr.forward_counts(a_true, i0, mus)
    return _case(f'gaps K={K} M={M} {"odd" if odd else "even"} {"noisy" if noise else "clean"}', K, M, i0, mus, a_true,
                 mr.noisy(g, rng) if noise else g)


LINES = {2: (9, 40), 3: (3, 12, 40)}      # of the 60-energy tables: 38.3, 101.4 keV; 26.1 (below the K-edge), 44.4, 101.4 keV


def lines_case(K):
    """K = M, every measurement weights one energy of the 60-energy tables only: nu_k = i0_k exp(-a . mus[:, e_k]), and the root
    of the clean counts' likelihood is the solution of K linear equations (``closed_form``)"""
    E, mus3, S = mr.synthetic_tables(60)
    mus = np.ascontiguousarray(mus3[:K])
    i0 = np.zeros((K, 60))
    for k, e in enumerate(LINES[K]):
        i0[k, e] = 20.0 * S[e]
    rng = np.random.default_rng([33, K])
    a_true = rng.uniform(0.0, 1.0, (N_PIX, K)) * np.array(A_WIDE[:K])
    return _case(f'lines K=M={K}', K, K, i0, mus, a_true, mr.forward_counts(a_true, i0, mus))


def closed_form(case, g=None):
    """[P, M] long double: solve(mus[:, lines].T, -ln(g / i0)) for a lines case"""
    K = case['K']
    e = list(LINES[K])
    A = np.asarray(case['mus'], dtype=LD)[:, e].T                            # [K, M]: row k is mu(e_k)
    g = case['g'] if g is None else g
    b = -np.log(np.asarray(g, dtype=LD) / np.asarray(case['i0'], dtype=LD)[np.arange(K), e][:, None]).T      # [P, K]
    det = _det(A)
    cols = []
    for m in range(K):                                                       # Cramer's rule, column m replaced by b
        Am = np.broadcast_to(A, (len(b), K, K)).copy()
        Am[:, :, m] = b
        cols.append(_det(Am) / det)
    return np.stack(cols, axis=1)


def _det(A):
    """determinant of [..., 2, 2] or [..., 3, 3], any float dtype"""
    if A.shape[-1] == 2:
        return A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    return (A[..., 0, 0] * (A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1])
            - A[..., 0, 1] * (A[..., 1, 0] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 0])
            + A[..., 0, 2] * (A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]))


def cap_case():
    i0, mus, a_true, rng = _wide_inputs(4, 3, CAP_ENERGIES, CAP_PIXELS, 34)
    return _case(f'cap K=4 M=3 nE={CAP_ENERGIES}', 4, 3, i0, mus, a_true, mr.noisy(mr.forward_counts(a_true, i0, mus), rng))


_cases = {}


def cases(kind):
    """the cases of one kind - 'wide', 'gaps', 'lines', 'cap' -, built once"""
    if kind not in _cases:
        if kind == 'wide':
            _cases[kind] = [wide_case(K, M, n_e, noise) for K, M in mr.SHAPES for n_e in WIDE_ENERGIES for noise in (False, True)]
        elif kind == 'gaps':
            _cases[kind] = [gaps_case(K, M, odd, noise) for K, M in mr.SHAPES for odd in (False, True) for noise in (False, True)]
        elif kind == 'lines':
            _cases[kind] = [lines_case(2), lines_case(3)]
        else:
            assert kind == 'cap'
            _cases[kind] = [cap_case()]
    return _cases[kind]


KINDS = ('wide', 'gaps', 'lines', 'cap')


def all_cases():
    return [c for kind in KINDS for c in cases(kind)]


def case_named(name):
    return next(c for c in all_cases() if c['name'] == name)


def early_cases():
    """the wide noisy case of every shape and energy count"""
    return [c for c in cases('wide') if c['name'].endswith('noisy')]


_refs, _trajs = {}, {}


def reference_of(case, f32=False):
    """``reference`` of a case, once; ``f32``: of its counts rounded to float32 and widened again"""
    key = (case['name'], f32)
    if key not in _refs:
        _refs[key] = reference(counts_of(case, f32).astype(F64), case['i0'], case['mus'])
    return _refs[key]


def counts_of(case, f32=False):
    return case['g'].astype(np.float32) if f32 else case['g']


def trajectory_of(case):
    if case['name'] not in _trajs:
        _trajs[case['name']] = trajectory(case['g'], case['i0'], case['mus'])
    return _trajs[case['name']]


# ----------------------------------------------------------------------------------------- the kernel's order, in float64

def fma(x, y, z):
    """x * y + z of float64 arrays with the sum formed in long double and rounded once to float64.  (The 106-bit product is
    itself rounded to 64 bits first; the result differs from a true fused multiply-add by one ulp on about one in 2^10.)"""
    return (np.asarray(x, dtype=LD) * np.asarray(y, dtype=LD) + np.asarray(z, dtype=LD)).astype(F64)


ROOT_VARIANTS = ('exp_2m40', 'drop_energy', 'counts_f32', 'wrong_row', 'scale_f32')
EARLY_VARIANTS = ('drop_S', 'q_scaled', 'mu_mm', 'swap_cofactors')


def kernel_tables(i0, mus, variant=None):
    """(tmu [M, nU], rows [nU, K * P]) as gn_multi_tables_kernel writes them: the energies some measurement weights, in order;
    -mu_m 2048/ln2; per measurement i0_k, i0_k mu_m, i0_k (mu_m mu_n) for m <= n"""
    i0, mus = np.asarray(i0, dtype=F64), np.asarray(mus, dtype=F64)
    K, M = i0.shape[0], mus.shape[0]
    used = np.flatnonzero(np.any(~(i0 == 0.0), axis=0))
    if variant == 'drop_energy':          # the weakest weight of measurement 0 goes, and its energy with it
        w0 = np.abs(i0[0, used])
        used = np.delete(used, int(np.argmin(np.where(w0 > 0.0, w0, np.inf))))
    scale = float(np.float32(EXP_SCALE)) if variant == 'scale_f32' else EXP_SCALE
    mu = mus[:, used]
    rows = []
    for k in range(K):
        w = i0[k, used]
        rows.append(w)
        for m in range(M):
            wrong = variant == 'wrong_row' and (k, m) == (K - 1, 1)
            rows.append(w * mu[0 if wrong else m])
        for m, n in _pairs(M):
            wrong = variant == 'mu_mm' and (k, m, n) == (0, 0, 1)
            rows.append(w * (mu[m] * mu[m if wrong else n]))
    return -mu * scale, np.ascontiguousarray(np.stack(rows, axis=1))


def _kernel_step(a, g, tmu, rows, K, M, ulp, signs, variant):
    """one iteration of gn_multi_kernel on the pixels a [P, M], g [P, K], operation for operation in float64"""
    P = 1 + M + M * (M + 1) // 2
    with np.errstate(all='ignore'):
        y = a[:, 0:1] * tmu[0]
        for m in range(1, M):
            y = fma(a[:, m:m + 1], tmu[m], y)
        at = np.exp(y.astype(LD) * (LN2_LD / LD(2048.0))).astype(F64)          # the correctly rounded exponential of the kernel's y
        if ulp:
            at = np.nextafter(at, np.where(ulp * signs > 0, np.inf, -np.inf))
        if variant == 'exp_2m40':
            at = at * (1.0 + 2.0 ** -40)
        at_ld, rows_ld = at.astype(LD), rows.astype(LD)
        acc = np.zeros((len(a), rows.shape[1]))
        wide = np.empty(acc.shape, LD)
        for e in range(rows.shape[0]):                                       # acc = fma(row[e], at[e], acc), see ``fma``
            np.multiply(rows_ld[e], at_ld[:, e:e + 1], out=wide)
            np.add(wide, acc, out=wide)
            acc[...] = wide
        acc = acc.reshape(len(a), K, P)
        pairs = _pairs(M)
        dF = [None] * M
        H = [None] * len(pairs)
        for k in range(K):
            nu = acc[:, k, 0]
            inv = 1.0 / nu
            ratio = g[:, k] * inv
            c = np.where(np.abs(nu) < np.inf, (g[:, k] - nu) * inv, ratio - 1.0)
            q = ratio * inv
            if variant == 'q_scaled':
                q = q * (1.0 + 1e-6)
            for m in range(M):
                Gm = acc[:, k, 1 + m]
                dF[m] = c * Gm if k == 0 else dF[m] + c * Gm
            for s, (m, n) in enumerate(pairs):
                S = acc[:, k, 1 + M + s]
                if variant == 'drop_S' and (k, m, n) == (K - 1, 0, 1):
                    S = 0.0 * S
                h = q * (acc[:, k, 1 + m] * acc[:, k, 1 + n]) - c * S
                H[s] = h if k == 0 else H[s] + h
        if M == 2:
            h00, h01, h11 = H
            inv_det = 1.0 / (h00 * h11 - h01 * h01)
            d = [(h11 * dF[0] + -h01 * dF[1]) * inv_det, (h00 * dF[1] + -h01 * dF[0]) * inv_det]
        else:
            h00, h01, h02, h11, h12, h22 = H
            c00, c01, c02 = h11 * h22 - h12 * h12, h02 * h12 - h01 * h22, h01 * h12 - h02 * h11
            c11, c12, c22 = h00 * h22 - h02 * h02, h01 * h02 - h00 * h12, h00 * h11 - h01 * h01
            inv_det = 1.0 / ((h00 * c00 + h01 * c01) + h02 * c02)
            if variant == 'swap_cofactors':
                c01, c02 = c02, c01
            d = [((c00 * dF[0] + c01 * dF[1]) + c02 * dF[2]) * inv_det,
                 ((c01 * dF[0] + c11 * dF[1]) + c12 * dF[2]) * inv_det,
                 ((c02 * dF[0] + c12 * dF[1]) + c22 * dF[2]) * inv_det]
        return a - np.stack(d, axis=1)


def emulate(g, i0, mus, n_iters, ulp=0, variant=None, keep=(), start=None):
    """The kernel's result in float64 NumPy: the exponent as the fma chain over the materials, one sequential fma per energy in
    list order, (g - nu) / nu for c, the adjugate solve in the kernel's order, the exit on an update that returns its input.
    ``ulp``: 0, +1 / -1 (every exponential moved one ulp up / down) or 'seeded' (up or down by a seeded sign per energy).
    ``variant``: one of ROOT_VARIANTS / EARLY_VARIANTS.  ``start`` = (a [P, M], n): take over from the state a after n
    iterations instead of 1e-6 after none.  Returns [P, M], or {n: [P, M]} for the iteration counts in ``keep``."""
    g = np.asarray(g, dtype=F64)
    if variant == 'counts_f32':
        g = g.astype(np.float32).astype(F64)
    K, M = g.shape[0], np.shape(mus)[0]
    tmu, rows = kernel_tables(i0, mus, variant)
    if ulp == 'seeded':
        signs, ulp = np.where(np.random.default_rng(35).integers(0, 2, tmu.shape[1]) > 0, 1.0, -1.0), 1
    else:
        signs = np.ones(tmu.shape[1])
    gp = np.ascontiguousarray(g.T)
    a, done = (np.full((gp.shape[0], M), 1e-6), 0) if start is None else (np.array(start[0], dtype=F64), int(start[1]))
    live = np.flatnonzero(np.all(np.isfinite(a), axis=1))
    kept = {}
    for it in range(done + 1, int(n_iters) + 1):
        if live.size:
            new = _kernel_step(a[live], gp[live], tmu, rows, K, M, ulp, signs, variant)
            same = np.all(new.view(np.uint64) == a[live].view(np.uint64), axis=1)
            a[live] = new
            live = live[~same]
        if it in keep:
            kept[it] = a.copy()
    return kept if keep else a


def emulate_root(case, ulp=0, variant=None):
    """``emulate`` to 50 iterations on a case, taking over from the restatement's state after WARM_STEPS: where the iteration
    ends is decided by the arithmetic of its last steps (the update is a pure function of the state, and the restatement's
    state after 40 steps is within a few steps of every variant's root), and the 40 steps of the walk from 1e-6 in the
    kernel's order would be all but a tenth of the time.  tests/test_gn_multi_root_refs.py runs the walk from 1e-6 where the
    energies are few."""
    return emulate(case['g'], case['i0'], case['mus'], 50, ulp, variant, start=(reference_of(case)['a40'], WARM_STEPS))


EMULATIONS = (1, -1, 'seeded')


_emulated = {}


def emulated_ratio(case, ulp):
    """worst ratio of ``emulate_root`` on a case, once"""
    key = (case['name'], ulp)
    if key not in _emulated:
        _emulated[key] = worst_ratio(emulate_root(case, ulp), reference_of(case))
    return _emulated[key]


def restatement_ratio(case):
    ref = reference_of(case)
    return worst_ratio(ref['a50'], ref)


def allowance_table():
    """{(case name, who): worst ratio} over the wide and the gaps cases; who = 'restatement' or an entry of EMULATIONS"""
    out = {}
    for kind in ('wide', 'gaps'):
        for case in cases(kind):
            out[(case['name'], 'restatement')] = restatement_ratio(case)
            for ulp in EMULATIONS:
                out[(case['name'], ulp)] = emulated_ratio(case, ulp)
    return out


ALLOWANCE_TABLE = allowance_table()
C = FACTOR * float(np.max(list(ALLOWANCE_TABLE.values())))                   # NaN if any of them is
