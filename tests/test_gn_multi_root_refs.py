"""tests/gn_multi_root_refs.py on the CPU: the extended-precision root and the early trajectory are usable on every case, the
float64 restatement and the emulations of the kernel's order stay inside the allowance they define, the closed form of the line
cases agrees with the polished root, and both comparisons reject wrong variants of the emulation - each by a factor of ten.

What this does not detect.  Every variant listed in ROOT_VARIANTS and EARLY_VARIANTS is rejected, none had to be set aside
(worst ratios of the root variants on their best case: 2^-40 exponential 225, dropped energy 7e13, float32 counts 2e7, wrong
row 7e11, float32 exponent scale 7e6, against 10 C = 17.9).  A wrong i0_k mu_m row is invisible to the root comparison wherever
the fit is exact - K = M, or clean counts: c_k = 0 at the root whatever G is, ratios 0.03 .. 0.2 on three of the five cases -
and shows on noisy counts with K > M only.  By construction the root comparison is blind to anything that only costs iterations
(a wrong S_kmn, q_k or cofactor: the early iterates are there for those), and the early iterates, held to 1e-9, are blind to
gradient-side errors below 1e-9 (the root comparison is there for those); q_k scaled by 1 + 1e-6 shows as 1e-6, an error of
q_k below 1e-9 would show nowhere.  Neither sees the +-700 clip of the exponent (no exponent of a case exceeds 21.4), nor an
error in a pixel that the reference sets aside: the 1 % cap bounds how many those can be (5 of 1000 in one case, none else).
The emulations take over from the restatement after 40 steps (emulate_root): an error that only derails the walk from 1e-6
is seen by the device test, not by the allowance.
"""
import numpy as np
import pytest

import gn_multi_refs as mr
import gn_multi_root_refs as rr

ROOT_CASES = ('wide K=2 M=2 nE=8 clean', 'wide K=3 M=2 nE=49 noisy', 'wide K=4 M=3 nE=49 noisy', 'gaps K=3 M=3 odd noisy',
              'gaps K=4 M=2 even clean')


def test_allowance_is_four_times_the_worst_cpu_ratio():
    table = rr.ALLOWANCE_TABLE
    names = {c['name'] for kind in ('wide', 'gaps') for c in rr.cases(kind)}
    assert {n for n, _ in table} == names and {w for _, w in table} == {'restatement'} | set(rr.EMULATIONS)
    worst = max(table.values())
    who = max(table, key=table.get)
    print(f'worst CPU ratio {worst:.3f} ({who}); restatement alone {max(v for (_, w), v in table.items() if w == "restatement"):.3f}; C = {rr.C:.3f}')
    assert np.isfinite(worst) and rr.C == rr.FACTOR * worst and rr.FACTOR == 4.0
    # a scale that means what it says: float64 arithmetic stays below one rounding of every term, and is not far below it
    assert 0.1 < worst < 1.0


@pytest.mark.parametrize('kind', rr.KINDS)
def test_restatement_and_emulations_stay_within_the_allowance(kind):
    for case in rr.cases(kind):
        ref = rr.reference_of(case)
        n_bad = int((~ref['usable']).sum())
        figures = {'restatement': rr.restatement_ratio(case)}
        figures.update({ulp: rr.emulated_ratio(case, ulp) for ulp in rr.EMULATIONS})
        print(f"{case['name']}: usable {ref['usable'].sum()} / {len(ref['usable'])} (not reproducible alone: "
              f"{int((ref['three'] & ~ref['reproducible']).sum())}), largest exponent {rr.largest_exponent(case):.1f}, "
              + ', '.join(f'{k} {v:.3f}' for k, v in figures.items()))
        assert n_bad <= rr.UNUSABLE_CAP * len(ref['usable']), case['name']
        assert rr.largest_exponent(case) < 30.0
        for who, r in figures.items():
            assert r <= rr.C, (case['name'], who, r)


def test_cases_are_what_they_say():
    assert len(rr.cases('wide')) == 30 and len(rr.cases('gaps')) == 20
    for case in rr.cases('wide'):
        assert case['g'].shape == (case['K'], rr.N_PIX) and (case['K'], case['M']) in mr.SHAPES
        assert np.all(case['a_true'].max(axis=0) > 0.95 * np.array(rr.A_WIDE[:case['M']]))
    for case in rr.cases('gaps'):
        weighted = (case['i0'] != 0.0).sum(axis=0)
        odd = ' odd ' in case['name']
        gap = np.zeros(60, bool)
        gap[rr.GAP_FIRST:rr.GAP_FIRST + rr.GAP_LEN] = True
        gap[59] = True
        gap[0] = odd
        assert np.array_equal(weighted == 0, gap) and np.all(weighted[~gap] == 1)
        assert int((~gap).sum()) == (53 if odd else 54)
        assert rr.kernel_tables(case['i0'], case['mus'])[1].shape[0] == (53 if odd else 54)
    for case in rr.cases('lines'):
        assert np.array_equal(np.argwhere(case['i0'] != 0.0), np.array([[k, e] for k, e in enumerate(rr.LINES[case['K']])]))
    cap, = rr.cases('cap')
    assert cap['i0'].shape == (4, 4096) and cap['mus'].shape == (3, 4096) and cap['g'].shape == (4, 64)


def test_closed_form_of_the_line_cases():
    for case in rr.cases('lines'):
        ref = rr.reference_of(case)
        exact = rr.closed_form(case)
        assert ref['usable'].all()
        # the polished root against the closed form, on the root's own scale (2^-53 of the reach; long double resolves 2^-11 of it)
        r = float(np.max(np.abs(exact - ref['root']) / ref['scale']))
        e50 = mr.rel_err(ref['a50'], exact.astype(np.float64))
        print(f"{case['name']}: |closed form - polished root| = {r:.2e} of the scale; restatement vs closed form {e50:.2e}")
        assert r <= 2.0 ** -6
        assert e50 <= 1.1e-14
        closed = dict(ref, root=exact)
        assert rr.worst_ratio(ref['a50'], closed) <= rr.C


def test_a_walk_across_a_singular_hessian_is_set_aside():
    """Why a fourth condition: the three of the root alone accept a pixel whose result no float64 arithmetic determines.  From
    1e-6 in the kernel's order, pixel 762 of this case ends at the restatement's root with exact exponentials and with every
    exponential one ulp down, and nowhere with every exponential one ulp up; walk_is_determined sets it aside, and with it
    at most 1 % of any case (test_restatement_and_emulations_stay_within_the_allowance)."""
    case = rr.case_named('wide K=3 M=3 nE=8 noisy')
    ref = rr.reference_of(case)
    p = 762
    assert ref['three'][p] and not ref['reproducible'][p] and not ref['usable'][p]
    ends = {ulp: rr.emulate(case['g'][:, p:p + 1], case['i0'], case['mus'], 50, ulp)[0] for ulp in (0, -1, 1)}
    print({k: v.tolist() for k, v in ends.items()})
    for ulp in (0, -1):
        assert np.max(np.abs(ends[ulp] - ref['root'][p]) / ref['scale'][p]) <= rr.C
    assert not np.all(np.isfinite(ends[1]))
    # with the pixels set aside, the walk from 1e-6 in the kernel's order meets the root on the whole case in every emulation
    for ulp in (0,) + rr.EMULATIONS:
        assert rr.worst_ratio(rr.emulate(case['g'], case['i0'], case['mus'], 50, ulp), ref) <= rr.C


def test_float32_counts_have_their_own_root():
    case = rr.case_named('wide K=3 M=2 nE=8 noisy')
    ref, ref32 = rr.reference_of(case), rr.reference_of(case, f32=True)
    assert ref32['usable'].sum() >= 990
    assert rr.worst_ratio(ref32['a50'], ref32) <= rr.C
    assert rr.worst_ratio(ref32['a50'], ref) >= 10.0 * rr.C


@pytest.mark.parametrize('name', ['wide K=2 M=2 nE=8 noisy', 'wide K=4 M=3 nE=8 noisy', 'wide K=3 M=3 nE=49 clean'])
def test_walk_from_the_start_ends_where_the_warm_start_does(name):
    """all 50 iterations in the kernel's order, from 1e-6, against emulate_root's take-over after 40"""
    case = rr.case_named(name)
    ref = rr.reference_of(case)
    for ulp in (0,) + rr.EMULATIONS:
        r = rr.worst_ratio(rr.emulate(case['g'], case['i0'], case['mus'], 50, ulp), ref)
        print(f'{name} ulp {ulp}: from 1e-6 {r:.3f}, warm {rr.worst_ratio(rr.emulate_root(case, ulp), ref):.3f}')
        assert r <= rr.C


@pytest.mark.parametrize('variant', rr.ROOT_VARIANTS)
def test_root_comparison_rejects(variant):
    got = {}
    for name in ROOT_CASES:
        case = rr.case_named(name)
        r = rr.worst_ratio(rr.emulate_root(case, 0, variant), rr.reference_of(case))
        got[name] = float('inf') if np.isnan(r) else r
        assert rr.worst_ratio(rr.emulate_root(case, 0), rr.reference_of(case)) <= rr.C
    print(f'{variant}: ' + ', '.join(f'{n}: {r:.3g}' for n, r in got.items()) + f' (10 C = {10 * rr.C:.1f})')
    assert max(got.values()) >= 10.0 * rr.C


def test_early_iterates_are_usable_and_met():
    for case in rr.early_cases():
        traj = rr.trajectory_of(case)
        n_bad = int((~traj['usable']).sum())
        em = rr.emulate(case['g'], case['i0'], case['mus'], 3, keep=rr.EARLY_STEPS)
        errs = [rr.early_err(em[n], traj, n) for n in rr.EARLY_STEPS]
        print(f"{case['name']}: usable {traj['usable'].sum()} / {len(traj['usable'])}, emulation vs long double after 1 / 2 / 3 steps: "
              + ' / '.join(f'{e:.2e}' for e in errs))
        assert n_bad <= rr.UNUSABLE_CAP * len(traj['usable']), case['name']
        assert max(errs) <= rr.EARLY_TOL


@pytest.mark.parametrize('variant', rr.EARLY_VARIANTS + ('wrong_row',))      # the wrong row: invisible at an exactly fitted root, not here
def test_early_iterates_reject(variant):
    worst = 0.0
    for case in rr.early_cases():
        if case['mus'].shape[1] == 239 or (variant == 'swap_cofactors' and case['M'] != 3):
            continue
        traj = rr.trajectory_of(case)
        em = rr.emulate(case['g'], case['i0'], case['mus'], 3, variant=variant, keep=rr.EARLY_STEPS)
        errs = [rr.early_err(em[n], traj, n) for n in rr.EARLY_STEPS]
        e = float('inf') if np.isnan(errs).any() else max(errs)
        print(f"{variant} {case['name']}: " + ' / '.join(f'{x:.2e}' for x in errs))
        worst = max(worst, e)
    assert worst >= 10.0 * rr.EARLY_TOL
