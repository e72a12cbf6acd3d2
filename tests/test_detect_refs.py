"""tests/detect_refs.py on the CPU, on the inputs of tests/test_gpu_detect.py: the scans' path lengths come from the C oracle's
mirror of the kernel arithmetic (c_oracle.project_dda / project_cone(dda=True)), which the device returns bit for bit, so what is
shown here holds for the GPU run.  The derived bound holds for float32 emulations of the four summation orders whatever way
the exponential's last bit falls; it rejects every variant of detect_refs.MUTANTS on at least one (table, scan) of the matrix;
the sweep reaches starvation, the underflow threshold and the air shortcut where it claims to; log_ref is +inf exactly where
float32 NumPy is.

Worst |emulation - exact| / bound over the cases of the matrix marked for the CPU, all seven tables, the exponential moved by
+1 ulp everywhere, -1 ulp everywhere and at random (counts and variance weights):
    loop     0.54    (detect_energies, detect_kernel, the scalar cone loop)
    pairs    0.57    (detect_energy_pairs)
    natural  0.57    (detect_store_lds, detect_kernel_chunked)
    tree     0.48    (wave_ray_kernel)
test_sweep_reach asks for 64 consecutive air-only rays on the multi-row fans only - the scans whose kernels have the air shortcut:
a single-row view has 37 rays, and a cone beam's air length changes from row to row; both still have air-only rays.  "A ray
meets every material" is asserted of one ray up to 4 table rows and, beyond (a ray of a 40-voxel grid cannot cross 59 materials),
as: every table row is crossed by some ray.
"""
import numpy as np
import pytest

import detect_refs as dr

F32, F64 = np.float32, np.float64
CPU_CASES = [c for c in dr.CASES if c[7]]
MULTI_RAY_FORMS = ('detect_store4', 'rows16_kernel', 'detect_kernel')        # several rays per lane: pairs of rays, the air shortcut
SHORTCUT_SCANS = ('rows64', 'rows66')


def pathlen_of(case):
    return dr.oracle_pathlen(case[1], case[3])


# ---- the reference itself --------------------------------------------------------------------------------------------------------

def test_detect_ref_is_the_extended_precision_sum():
    case = dr.CASES[1]
    pl = pathlen_of(case)[::7]
    for step, mu, w, w2 in dr.case_tables(case, pathlen_of(case)):
        exact, bound = dr.detect_ref(pl, mu, w2)
        L, m, ww = pl.astype(np.longdouble), mu.astype(np.longdouble), w2.astype(np.longdouble)
        ref = np.array([[sum(ww[s, e] * np.exp(-sum(m[k, e] * L[r, k] for k in range(m.shape[0]))) for e in range(m.shape[1]))
                         for r in range(L.shape[0])] for s in range(ww.shape[0])])
        assert np.all(np.abs(exact - ref.astype(F64)) <= 1e-13 * np.abs(w2).sum() + 1e-300), step
        assert np.all(bound > 0.0) and exact.shape == bound.shape == (w.shape[0], pl.shape[0])


def test_tables_are_what_the_sweep_says():
    pl = pathlen_of(dr.CASES[4])
    for step, mu, w, w2 in dr.case_tables(dr.CASES[4], pl):
        P, _ = dr.exponents(pl, mu)
        assert mu.dtype == w.dtype == w2.dtype == F32 and np.all(mu >= 0.0)
        if step == 'steep':
            assert P.max(axis=0)[0] < 2e-3 and abs(P.max() - 120.0) < 1e-3 and np.all(np.diff(P.max(axis=0)) > 0.0)
        else:
            assert abs(P.max() - step) <= 1e-5 * step and (step == 0 or np.all(mu[0] > 0.0))       # (air is scaled with the others)
    w = dr.weights(300, 2)
    bits = w.view(np.uint32).reshape(2, 75, 4)
    assert np.all((w > 0.0) | (w == 0.0))                                                          # positive, or a zero of either sign
    assert np.any(np.all(bits == 0, axis=2)[0]) and np.any(np.all(bits == 0x80000000, axis=2)[0])  # whole +0 and -0 blocks
    assert np.any((bits[0, :, 0] == 0) & (bits[0, :, 3] != 0)) and np.all(w[1, 32:] == 0.0)        # part blocks, the early end
    assert np.all(w[0, 256:] > 0.0) and np.all(dr.weights(139, 2)[0, 136:] > 0.0) and np.all(dr.weights(7, 2) > 0.0)
    assert np.array_equal(dr.sweep_tables(3, 300, 2, 1, 1.0)[2], (w.astype(F64) * dr.gain(300)).astype(F32))


# ---- the bound holds for every emulated order ------------------------------------------------------------------------------------

_worst = {}


@pytest.mark.parametrize('case', CPU_CASES, ids=dr.case_id)
def test_bound_holds_for_every_emulated_order(case):
    order = case[6]
    pl = pathlen_of(case)
    rng = np.random.default_rng(5)
    for step, mu, w, w2 in dr.case_tables(case, pl):
        exact, bound = dr.detect_ref(pl, mu, w)
        exact2, bound2 = dr.detect_ref(pl, mu, w2)
        for ulp in (+1, -1, rng.integers(-1, 2, (pl.shape[0], mu.shape[1]))):
            got = dr.emulate(pl, mu, w, order, ulp)
            q = dr.worst(got, exact, bound)
            _worst[order] = max(_worst.get(order, 0.0), q)
            assert dr.within(got, exact, bound), (step, q)
        got = dr.emulate(pl, mu, w2, order, ulp)                             # the variance: the same sum with w2
        q = dr.worst(got, exact2, bound2)
        _worst[order] = max(_worst.get(order, 0.0), q)
        assert dr.within(got, exact2, bound2), (step, q)
    print('worst |emulation - exact| / bound so far: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(_worst.items())))


def test_every_order_is_emulated_on_the_cpu():
    assert {c[6] for c in CPU_CASES} == set(dr.ORDERS)
    assert {c[0] for c in CPU_CASES} == {c[0] for c in dr.CASES} and {c[1] for c in CPU_CASES} == set(dr.SCANS)
    for form in {c[0] for c in dr.CASES}:                                    # every form meets every energy and spectrum count
        mine = [c for c in dr.CASES if c[0] == form]
        if form in ('detect_energy_pairs', 'cone_scalar_loop'):              # (<= 2 spectra in pairs, the scalar loop beyond)
            mine = [c for c in dr.CASES if c[0] in ('detect_energy_pairs', 'cone_scalar_loop')]
        assert {c[4] for c in mine} == {3, 7, 64, 139, 300} and {c[5] for c in mine} == {1, 2, 3, 4}, form


# ---- every mutant is caught ------------------------------------------------------------------------------------------------------

def candidates(name):
    """The cases of the matrix a variant can occur in, the cheap ones first."""
    cases = sorted(dr.CASES, key=lambda c: dr.SCANS[c[1]][0] * c[3] * c[4])
    if name in ('air_shortcut_speck', 'stale_air_cache'):
        return [c for c in cases if c[0] in MULTI_RAY_FORMS and c[1] in SHORTCUT_SCANS and c[3] <= 4 and c[5] <= 2]
    if name == 'odd_ray_gets_even_lengths':
        return [c for c in cases if c[0] in MULTI_RAY_FORMS]
    if name.startswith('variance'):
        return [c for c in cases if c[0] != 'wave_ray_kernel']
    return cases


@pytest.mark.parametrize('name', dr.MUTANTS)
def test_every_mutant_breaks_its_bound(name):
    for case in candidates(name):
        pl = pathlen_of(case)
        for step, mu, w, w2 in dr.case_tables(case, pl):
            res = dr.run_mutant(name, pl, mu, w, w2, case[6])
            if res is None:
                continue
            got, pl_used, w_ref = res
            exact, bound = dr.detect_ref(pl_used, mu, w_ref)
            if not dr.within(got, exact, bound):
                n_bad = int(np.count_nonzero(np.abs(got.astype(F64) - exact) > bound))
                print(f'{name}: caught on {dr.case_id(case)}, table {step}: {n_bad} of {exact.size} values, worst '
                      f'{dr.worst(got, exact, bound):.3g} bounds')
                if name in dr.PRECISION_MUTANTS:
                    assert case[4] in (3, 7)                                 # (what the small energy counts are in the matrix for)
                return
    pytest.fail(f'{name} survives every table and scan of the matrix: the inputs are too weak')


def test_precision_mutants_need_the_small_energy_counts():
    """At 139 energies the worst-case n_e term hides a relative error of 2^-18 in the exponential; at 3 it does not."""
    big, small = dr.CASES[3], dr.CASES[0]
    for case, caught in ((big, False), (small, True)):
        pl = pathlen_of(case)
        hit = False
        for step, mu, w, w2 in dr.case_tables(case, pl):
            got, _, _ = dr.run_mutant('exp_rel_2m18', pl, mu, w, w2, case[6])
            hit = hit or not dr.within(got, *dr.detect_ref(pl, mu, w))
        assert hit == caught, dr.case_id(case)


# ---- the sweep reaches what it claims --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key,n_mat', sorted({(c[1], c[3]) for c in dr.CASES}))
def test_sweep_reach(key, n_mat):
    """Properties of the float64 reference alone, for every (scan, table rows) of the matrix, at the energy counts it is used with."""
    pl = dr.oracle_pathlen(key, n_mat)
    met = pl > 0.0
    assert np.all(met.any(axis=0)), 'a table row no ray crosses'            # every material is met by a ray
    if n_mat <= 4:
        assert np.any(met.all(axis=1))                                       # and, where a ray can, all of them by one ray
    air = dr.air_only(pl, n_mat)
    if key in SHORTCUT_SCANS:      # whole waves of air-only rays: the 64 rows of an edge channel.  (The single-row scan has 37 rays
        assert dr.longest_air_run(pl, n_mat) >= 64             # per view and the cone beam's air length changes from row to row:
    assert np.count_nonzero(air) >= 10                         # neither has the shortcut; both have air-only rays.)
    for n_e, n_s in sorted({(c[4], c[5]) for c in dr.CASES if (c[1], c[3]) == (key, n_mat)}):
        pu = dr.p_unit(pl, n_mat)
        mu, w, _ = dr.sweep_tables(n_mat, n_e, n_s, 120, pu)
        exact, _ = dr.detect_ref(pl, mu, w)
        sw = np.abs(w.astype(F64)).sum(axis=1)[:, None]
        starved, bright = np.mean(exact < dr.ABS_TERM * sw, axis=1), np.mean(exact > 1e-6 * sw, axis=1)
        slots = sw[:, 0] > 0.0
        assert np.all(starved[slots] >= 0.01) and np.all(bright[slots] >= 0.10), (n_e, n_s, starved, bright)
        mu80 = dr.sweep_tables(n_mat, n_e, n_s, 80, pu)[0]
        P, _ = dr.exponents(pl, mu80)
        assert np.exp(-P.min(axis=1)).min() > dr.TINY and abs(P.max() - 80.0) < 1e-3
        Ps, _ = dr.exponents(pl, dr.sweep_tables(n_mat, n_e, n_s, 'steep', pu)[0])
        if n_e >= 7:                                                         # one ray from e^-0 down to flushed terms
            ray = np.argmax(Ps.max(axis=1))
            assert Ps[ray].min() < 2e-3 and np.exp(-Ps[ray].max()) < dr.TINY


# ---- log_ref ----------------------------------------------------------------------------------------------------------------------

def test_log_ref_is_inf_exactly_where_float32_numpy_is():
    tiny = np.array([0.0, 1e-45, 1e-40, 8.9e-39, 1.0e-38, 1.17e-38, 1.1754944e-38, 2e-38, 1e-30, 1e-20, 1e-3, 1.0, 3.0, 1e6, 1e30],
                    F32)
    rng = np.random.default_rng(3)
    counts = np.concatenate([tiny, (10.0 ** rng.uniform(-44.0, 8.0, 4000)).astype(F32)])
    for air in (0.7, 3.0, 3.9, 150.0, 1e6):
        c = np.stack([counts, counts[::-1]])
        exact, bound = dr.log_ref([air, air], c)
        with np.errstate(divide='ignore', over='ignore'):
            ref32 = np.log(np.float32(air) / c)                              # what the reference program evaluates
        assert np.array_equal(np.isinf(exact), np.isinf(ref32)) and np.all(exact[np.isinf(exact)] > 0) and not np.isnan(exact).any()
        assert np.all(np.isinf(exact[c == 0.0])) and np.isinf(exact).sum() > 2 * np.count_nonzero(counts == 0.0)
        assert dr.log_within(ref32, exact, bound)                            # (NumPy's own float32 log is inside the bound)
        bad = ref32.copy()
        bad[0, 20] = np.nan
        assert not dr.log_within(bad, exact, bound)
        k = np.flatnonzero(np.isinf(exact[0]))[0]
        bad = ref32.copy()
        bad[0, k] = 88.0                                                     # a finite value where +inf is due
        assert not dr.log_within(bad, exact, bound)
        fin = np.flatnonzero(np.isfinite(exact[0]))
        bad = ref32.copy()
        bad[0, fin[5]] = np.inf
        assert not dr.log_within(bad, exact, bound)
        bad = ref32.copy()
        bad[0, fin[7]] += F32(1e-5) * (1 + abs(bad[0, fin[7]]))
        assert not dr.log_within(bad, exact, bound)
    assert np.isfinite(dr.log_ref([3.0], np.array([[1e-38]], F32))[0][0, 0])  # a denormal count whose quotient still fits
