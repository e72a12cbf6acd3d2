"""The GN oracle (NumPy and C restatements of matdecomp.py:87-207) against golden vectors captured
from the real reference (tests/golden/make_goldens.py)."""
import types

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import gn_oracle as go

ATOL = 1e-10    # relative to max(|a|, 1): rounding-level agreement, not bitwise


def close(a, b, tol=ATOL):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < tol


@pytest.mark.parametrize('ci', [0, 1, 2])
def test_tables_match_reference_bitwise(golden, ci):
    g = golden
    ee, dE, i0 = go.decomposition_tables(g[f'gn{ci}_det_E'], g[f'gn{ci}_det_eta'], bool(g[f'gn{ci}_eid']),
                                         g[f'gn{ci}_spec1_E'], g[f'gn{ci}_spec1_I0'], g[f'gn{ci}_spec2_E'],
                                         g[f'gn{ci}_spec2_I0'])
    assert np.array_equal(ee, g[f'gn{ci}_ee'])
    assert np.array_equal(i0, g[f'gn{ci}_i0'])
    assert bool(g[f'gn{ci}_i0_tiled_same'])       # the reference tiles one spectrum over all channels
    assert ee.size == (239 if ci == 1 else 140)


@pytest.mark.parametrize('ci', [0, 1, 2])
@pytest.mark.parametrize('n_iters', [1, 2, 50])
def test_numpy_oracle_trajectory(golden, ci, n_iters):
    g = golden
    a = go.newton_solve(g[f'gn{ci}_g'], g[f'gn{ci}_i0'], g[f'gn{ci}_mus'], n_iters)
    assert close(a, g[f'gn{ci}_a_iters{n_iters}'])


@pytest.mark.parametrize('ci', [0, 2])
def test_numpy_oracle_iter5(golden, ci):
    g = golden
    a = go.newton_solve(g[f'gn{ci}_g'], g[f'gn{ci}_i0'], g[f'gn{ci}_mus'], 5)
    assert close(a, g[f'gn{ci}_a_iters5'])


@pytest.mark.parametrize('ci', [0, 1, 2])
@pytest.mark.parametrize('n_iters', [1, 2, 50])
def test_c_oracle_trajectory(golden, ci, n_iters):
    g = golden
    a = co.gn_decompose(g[f'gn{ci}_g'][0], g[f'gn{ci}_g'][1], g[f'gn{ci}_i0'], g[f'gn{ci}_mus'], n_iters)
    assert close(a, g[f'gn{ci}_a_iters{n_iters}'], 1e-9)


@pytest.mark.parametrize('n_iters', [1, 3, 30])
def test_channel_dependent_i0(golden, n_iters):
    g = golden
    a = go.newton_solve(g['opt_g'], g['opt_i0'], g['opt_mus'], n_iters)
    assert close(a, g[f'opt_a_iters{n_iters}'])


@pytest.mark.parametrize('ci', [0, 1, 2])
def test_get_basismat_sinos_mask(golden, ci):
    g = golden
    ct = types.SimpleNamespace(det_E=g[f'gn{ci}_det_E'], det_eta_E=g[f'gn{ci}_det_eta'], eid=bool(g[f'gn{ci}_eid']))
    s1 = types.SimpleNamespace(E=g[f'gn{ci}_spec1_E'], I0=g[f'gn{ci}_spec1_I0'])
    s2 = types.SimpleNamespace(E=g[f'gn{ci}_spec2_E'], I0=g[f'gn{ci}_spec2_I0'])
    basis = lambda ee: g[f'gn{ci}_mus']
    for key, kw in (('50', dict(n_iters=50)), ('default', {}), ('thresh50', dict(n_iters=50, mask_thresh=0.5))):
        m1, m2 = go.get_basismat_sinos(ct, g[f'gn{ci}_g'][0].copy(), g[f'gn{ci}_g'][1].copy(), s1, s2, basis, **kw)
        r1, r2 = g[f'gn{ci}_mat1_{key}'], g[f'gn{ci}_mat2_{key}']
        assert np.array_equal(m1 == 0, r1 == 0) and np.array_equal(m2 == 0, r2 == 0)   # masked pixels exactly 0
        assert close(m1, r1) and close(m2, r2)


def test_noise_free_truth_recovered(golden):
    g = golden
    a = go.newton_solve(g['gn0_g'], g['gn0_i0'], g['gn0_mus'], 50)
    t = g['gn0_a_true']
    assert np.max(np.abs(a - t)) < 1e-9


def test_oracle_on_unscreened_live_default_pair():
    """tests/golden/ref_extra.npz (make_goldens_r2.py): detunedMV / 80 kV pixels drawn once, no redraw loop.  On every
    pixel the reference completes and answers stably (spurious roots included) the oracle agrees to rounding; the
    pixels on which the reference raises LinAlgError come out non-finite here in all but (at most) two cases -
    the closed-form 2x2 solve does not flag the exactly singular pivot LAPACK reports (matdecomp.py:125)."""
    import os
    from conftest import GOLDEN
    e = np.load(os.path.join(GOLDEN, 'ref_extra.npz'))
    ok = ~e['uns_raised'] & ~e['uns_ill']
    with np.errstate(all='ignore'):
        a_np = go.newton_solve(e['uns_g'], e['uns_i0'], e['uns_mus'], int(e['uns_n_iters']))
        a_c = co.gn_decompose(e['uns_g'][0].ravel(), e['uns_g'][1].ravel(), e['uns_i0'], e['uns_mus'],
                              int(e['uns_n_iters'])).reshape(a_np.shape)
    assert close(a_np[ok], e['uns_a50'][ok]) and close(a_c[ok], e['uns_a50'][ok])
    assert (np.abs(e['uns_a50'][ok] - e['uns_a_true'][ok]).max(-1) > 1.0).sum() > 0     # spurious roots are in the set
    r = e['uns_raised']
    assert (~np.isfinite(a_c[r]).all(-1)).sum() >= r.sum() - 2


def test_nan_count_masks_nothing(golden):
    """One NaN in sinogram 1: np.max is NaN, every comparison False, nothing masked (matdecomp.py:195-196)."""
    import os
    from conftest import GOLDEN
    e, g = np.load(os.path.join(GOLDEN, 'ref_extra.npz')), golden
    ct = types.SimpleNamespace(det_E=g['gn0_det_E'], det_eta_E=g['gn0_det_eta'], eid=bool(g['gn0_eid']))
    s1 = types.SimpleNamespace(E=g['gn0_spec1_E'], I0=g['gn0_spec1_I0'])
    s2 = types.SimpleNamespace(E=g['gn0_spec2_E'], I0=g['gn0_spec2_I0'])
    basis = lambda ee: g['gn0_mus']
    with np.errstate(all='ignore'):
        m1, m2 = go.get_basismat_sinos(ct, e['nan_g'][0].copy(), e['nan_g'][1].copy(), s1, s2, basis, n_iters=30)
    fin = np.isfinite(e['nan_mat1'])
    assert np.array_equal(np.isfinite(m1), fin) and (~fin).sum() == 1
    assert np.array_equal(m1 == 0, e['nan_mat1'] == 0)
    assert close(m1[fin], e['nan_mat1'][fin]) and close(m2[fin], e['nan_mat2'][fin])


# ---- round 3: the screen of the live-pair fixture is frozen; Poisson-noisy goldens (tests/golden/make_goldens_r3.py)
def _load(name):
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, name))


def test_committed_screen_is_what_the_generator_produces():
    """The pixels left out of the live-pair comparison (ref_extra.npz: uns_raised, uns_ill) are exactly what the frozen
    criterion (make_goldens_r2.CRITERION_VERSION = 2) computes from the REAL reference on the committed inputs - so the
    exclusion cannot be widened quietly after a kernel change.  The reference's answer to every call the screen makes
    (optimize_sino_cpu on a pixel or on its ulp-shifted counts, raised or not) is stored in ref_screen_calls.npz
    (make_goldens_screen.py, recorded from the real reference); the screen runs here on those answers, and a call the
    reference was never asked fails the test."""
    import sys
    from conftest import GOLDEN
    e = _load('ref_extra.npz')
    assert int(e['uns_criterion_version']) == 2
    assert int(e['uns_raised'].sum()) == 8 and int(e['uns_ill'].sum()) == 8 and e['uns_raised'].size == 192
    # criterion (2) of the frozen screen, recomputed from the committed arrays alone
    assert np.array_equal(e['uns_ill'] & ~e['uns_raised'] | ~(e['uns_cond'] <= 1e13) & ~e['uns_raised'], e['uns_ill'])
    sys.path.insert(0, GOLDEN)
    import make_goldens_r2 as r2
    assert r2.CRITERION_VERSION == int(e['uns_criterion_version'])
    rec = _load('ref_screen_calls.npz')
    ee_fix, i0_fix, mus_fix = e['uns_ee'], e['uns_i0'], e['uns_mus']
    answers = {(float(g0), float(g1), int(n)): (bool(r), a)
               for (g0, g1), n, r, a in zip(rec['calls_g'], rec['calls_n_iters'], rec['calls_raised'], rec['calls_a'])}

    def reference_answer(gp, ee, i0_1, mus, n_iters, verbose=False):
        assert np.array_equal(ee, ee_fix) and np.array_equal(mus, mus_fix) and np.array_equal(i0_1[:, 0, :], i0_fix)
        raised, a = answers[(float(gp[0, 0, 0]), float(gp[1, 0, 0]), int(n_iters))]
        if raised:
            raise np.linalg.LinAlgError('Singular matrix')
        return a.reshape(1, 1, 2)

    # a third of the fixture's views keeps this at a few seconds; pixels are independent, so rows reproduce row by row
    sel = slice(*rec['views'])
    assert (sel.start, sel.stop) == (0, 2)
    raised, raised_at, a50, ill, cond = r2.screen(reference_answer, e['uns_g'][:, sel], e['uns_ee'], e['uns_i0'],
                                                  e['uns_mus'], int(e['uns_n_iters']))
    assert np.array_equal(raised, e['uns_raised'][sel]) and np.array_equal(ill, e['uns_ill'][sel])
    assert np.array_equal(raised_at, e['uns_raised_at'][sel])
    assert np.array_equal(a50, e['uns_a50'][sel], equal_nan=True) and np.array_equal(cond, e['uns_cond'][sel], equal_nan=True)


@pytest.mark.parametrize('n_iters', [1, 2, 50])
def test_oracles_on_poisson_noisy_goldens(n_iters):
    """140 / 80 kVp at the default dose scaling (main.py:68) with per-bin Poisson noise: the frozen screen flags no
    pixel, and both restatements follow the reference's trajectory on every one of the 192 noisy pixels."""
    e = _load('ref_noisy.npz')
    assert int(e['noisy_criterion_version']) == 2 and not e['noisy_raised'].any() and not e['noisy_ill'].any()
    want = e['noisy_a50'] if n_iters == 50 else e[f'noisy_a{n_iters}']
    a = go.newton_solve(e['noisy_g'], e['noisy_i0'], e['noisy_mus'], n_iters)
    assert close(a, want)
    c = co.gn_decompose(e['noisy_g'][0], e['noisy_g'][1], e['noisy_i0'], e['noisy_mus'], n_iters)
    assert close(c.reshape(want.shape), want, 1e-9)
    if n_iters == 50:
        # the public call on the noisy pair: air channels (two per view) masked to exactly 0
        air = e['noisy_g'][0] >= 0.95 * e['noisy_g'][0].max()
        assert air.sum() >= 12 and np.all(e['noisy_mat1'][air] == 0) and np.all(e['noisy_mat2'][air] == 0)
        assert close(np.stack([e['noisy_mat1'], e['noisy_mat2']], -1)[~air], e['noisy_a50'][~air])


def test_stability_screen_sees_a_wandering_pixel():
    """The sensitivities newton_solve returns for tools/soak_gn.py's stability screen: a pixel that wanders for 35 iterations
    before it settles (soak seed 1795, pixel 2221) passes the sum of per-step uncertainties ('walk') and is caught by the twin
    trajectories; its converging neighbours pass both, and the result itself does not depend on asking for the sensitivities."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from soak_cases import draw
    c = draw(1795)
    v, ch = divmod(2221, c['n_c'])
    g = c['g'][:, v:v + 1, ch - 3:ch + 4]
    with np.errstate(all='ignore'):
        a, sens = go.newton_solve(g, c['i0'], c['mus'], c['n_iters'], return_sensitivity=True)
        plain = go.newton_solve(g, c['i0'], c['mus'], c['n_iters'])
    assert np.array_equal(a, plain, equal_nan=True)
    eps = np.finfo(np.float64).eps
    assert eps * sens['walk'][0, 3] <= 1e-11 and not sens['twin'][0, 3] <= 1e-11
    others = [k for k in range(7) if k != 3 and np.isfinite(a[0, k]).all() and eps * sens['walk'][0, k] <= 1e-11]
    assert len(others) >= 3 and all(sens['twin'][0, k] <= 1e-11 for k in others)
