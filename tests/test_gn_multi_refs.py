"""The decomposition for K = 2 .. 4 measurements and M = 2 .. 3 materials, the part that needs no GPU: the NumPy restatement
against arrays the real reference produced, the conditioning of the inputs of the GPU shape sweep, the host-side helpers and
the argument checks of the Python layer and of the C entry points (which return before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import gn_multi_refs as mr
from conftest import GOLDEN, INPUT, ROOT

SWEEP_ENERGIES = (8, 47, 48, 49, 239)


@pytest.fixture(scope='module')
def goldens():
    return mr.load_goldens(os.path.join(GOLDEN, 'ref_multi.npz'))


def test_goldens_cover_the_cases(goldens):
    names = [c['name'] for c in goldens]
    for K, M in ((3, 2), (4, 2), (3, 3), (4, 3)):
        for tag in 'ab':
            for kind in ('exact', 'noisy'):
                assert f'syn_k{K}m{M}{tag}_{kind}' in names
    assert 'kvp_k3m2_exact' in names and 'kvp_k3m2_noisy' in names
    for c in goldens:
        K, M = c['g'].shape[0], c['mus'].shape[0]
        assert c['g'].shape == (K, 4, 16) and c['i0'].shape == (K, c['mus'].shape[1])
        for n in (30, 50):
            assert c['a'][n].shape == (4, 16, M) and np.all(np.isfinite(c['a'][n]))
    assert os.path.getsize(os.path.join(GOLDEN, 'ref_multi.npz')) < 100 * 1024


def test_restatement_agrees_with_the_reference(goldens):
    """1e-12 of max(|a|, 1) per component on every pixel of every golden, at 30 and at 50 iterations"""
    for c in goldens:
        for n in (30, 50):
            err = mr.rel_err(mr.newton_solve_multi(c['g'], c['i0'], c['mus'], n), c['a'][n])
            print(f"{c['name']} n_iters={n}: {err:.2e}")
            assert err <= 1e-12, (c['name'], n, err)


@pytest.mark.parametrize('n_energies', SWEEP_ENERGIES)
def test_sweep_inputs_are_well_conditioned(n_energies):
    """Reversing the order of the energies moves the restatement's result on the inputs of the GPU shape sweep by at most
    1e-12: a kernel that sums in another order can be held to 1e-9 there on every pixel."""
    for K, M in mr.SHAPES:
        g, i0, mus = mr.sweep_case(K, M, n_energies)
        for counts in (g, g.astype(np.float32).astype(np.float64)):
            a = mr.newton_solve_multi(counts, i0, mus, 30)
            b = mr.newton_solve_multi(counts, np.ascontiguousarray(i0[:, ::-1]), np.ascontiguousarray(mus[:, ::-1]), 30)
            assert np.all(np.isfinite(a))
            err = mr.rel_err(b, a)
            print(f'K={K} M={M} nE={n_energies}: {err:.2e}')
            assert err <= 1e-12, (K, M, n_energies, err)


def test_restatement_keeps_a_bad_pixel_to_itself():
    g, i0, mus = mr.sweep_case(3, 2, 48, n_pix=5)
    ref = mr.newton_solve_multi(g, i0, mus, 10)
    g[1, 2] = np.nan
    got = mr.newton_solve_multi(g, i0, mus, 10)
    assert np.all(np.isnan(got[2])) and np.array_equal(np.delete(got, 2, axis=0), np.delete(ref, 2, axis=0))


def test_energy_bins_partition_a_spectrum():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import synthetic
    spec = synthetic.kramers_spectrum(120)
    edges = [20.0, 45.0, 70.0, 121.0]
    bins = dx.energy_bins(spec, edges)
    assert len(bins) == 3
    inside = (spec.E >= edges[0]) & (spec.E < edges[-1])
    assert np.array_equal(sum(b.I0 for b in bins), np.where(inside, spec.I0, 0.0))
    for j, b in enumerate(bins):
        assert np.array_equal(b.E, spec.E)
        mine = (spec.E >= edges[j]) & (spec.E < edges[j + 1])
        assert np.array_equal(b.I0[mine], spec.I0[mine]) and not b.I0[~mine].any() and b.I0[mine].sum() > 0.0
    for bad in ([50.0], [50.0, 50.0], [60.0, 50.0]):
        with pytest.raises(ValueError):
            dx.energy_bins(spec, bad)


def test_tables_multi_equal_the_two_spectrum_tables():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md
    ct = dx.FanBeamGeometry(N_channels=16, N_proj=4, eid=True, detector_file=os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'))
    specs = [dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV') for kv in (140, 80, 120)]
    ee2, i02, mus2 = md.decomposition_tables(ct, specs[0], specs[1])
    ee, i0, mus = md.decomposition_tables_multi(ct, specs[:2])
    assert np.array_equal(ee, ee2) and np.array_equal(i0, i02) and np.array_equal(mus, mus2)
    ee3, i03, mus3 = md.decomposition_tables_multi(ct, specs, (md.matcomp1, md.matcomp2, 'H(11.2)O(88.8)'))
    assert i03.shape == (3, ee3.size) and mus3.shape == (3, ee3.size) and np.array_equal(mus3[:2], mus2)


def test_tables_multi_reproduce_the_golden_tables(goldens):
    """the bundled 80 / 120 / 140 kV case was generated from tables built like matdecomp.py:140-160"""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md
    ct = dx.FanBeamGeometry(N_channels=16, N_proj=4, eid=True, detector_file=os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'))
    specs = [dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV') for kv in (80, 120, 140)]
    for s in specs:
        s.rescale_counts(5.0e-4)
    c = next(c for c in goldens if c['name'] == 'kvp_k3m2_exact')
    _, i0, mus = md.decomposition_tables_multi(ct, specs)
    assert np.allclose(i0, c['i0'], rtol=1e-14, atol=0.0) and np.array_equal(mus, c['mus'])


def test_value_errors_come_before_any_device_access():
    """every one of these raises from the shapes and keywords alone (this machine has no device to touch)"""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md
    nE = 12
    g = lambda K: np.ones((K, 2, 5))
    i0 = lambda K: np.ones((K, nE))
    mus = lambda M: np.ones((M, nE))
    per_channel = np.arange(3 * 5 * nE, dtype=np.float64).reshape(3, 5, nE)
    for args in ((g(5), i0(5), mus(2)),               # too many measurements
                 (g(4), i0(4), mus(4)),               # too many materials
                 (g(2), i0(2), mus(3)),               # more materials than measurements
                 (g(3), i0(3), mus(1)),               # a single material
                 (g(3), per_channel, mus(2)),         # genuinely channel-dependent spectra beyond 2 x 2
                 (g(3), i0(2), mus(2)),               # spectra and sinograms disagree
                 (g(3), np.ones((3, nE + 1)), mus(2)),
                 (np.ones((3, 10)), i0(3), mus(2))):  # not [K, nViews, nBins]
        with pytest.raises(ValueError):
            md.optimize_sino(args[0], None, args[1], args[2], 5, verbose=False)
    with pytest.raises(ValueError, match='4'):
        md.optimize_sino(g(5), None, i0(5), mus(2), 5, verbose=False)
    with pytest.raises(ValueError, match='3'):
        md.optimize_sino_cpu(g(4), None, i0(4), mus(4), 5, verbose=False)
    with pytest.raises(ValueError):
        md.optimize_sino(g(3), None, i0(3), mus(2), 0, verbose=False)
    # keywords of the 2 x 2 path are refused, not ignored
    for kw in (dict(precision='mixed'), dict(stop_tol=1e-12), dict(two_level=True), dict(two_level='start'), dict(audit=100.0),
               dict(audit_strict=True), dict(kernel=2), dict(natural_order=True), dict(blocks_per_cu=4), dict(reduced=False)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            md.optimize_sino(g(3), None, i0(3), mus(2), 5, verbose=False, **kw)
    # a tiled [K, nBins, nE] spectrum is collapsed and passes the shape checks: what stops this call is the iteration count
    tiled = np.ascontiguousarray(np.broadcast_to(i0(3)[:, None, :], (3, 5, nE)))
    with pytest.raises(ValueError, match='n_iters'):
        md.optimize_sino(g(3), None, tiled, mus(2), 0, verbose=False)
    ct = dx.FanBeamGeometry(N_channels=5, N_proj=2)
    spec = dx.xRaySpectrum.from_arrays('s', np.arange(1.0, nE + 1.0), np.ones(nE))
    s = np.ones((2, 5), np.float32)
    for sinos, specs, mats in (([s] * 3, [spec] * 2, (md.matcomp1, md.matcomp2)),
                               ([s] * 5, [spec] * 5, (md.matcomp1, md.matcomp2)),
                               ([s] * 2, [spec] * 2, (md.matcomp1, md.matcomp2, md.matcomp2)),
                               ([s] * 4, [spec] * 4, (md.matcomp1,) * 4),
                               ([s, s, np.ones((2, 6), np.float32)], [spec] * 3, (md.matcomp1, md.matcomp2))):
        with pytest.raises(ValueError):
            md.get_basismat_sinos_multi(ct, sinos, specs, mats)
    with pytest.raises(ValueError):
        md.get_basismat_sinos_multi(ct, [s] * 3, [spec] * 3, n_iters=0)
    import torch
    with pytest.raises(ValueError):
        md.gn_device_multi(torch.ones(5, 7), i0(5), mus(2), 5)
    with pytest.raises(ValueError):
        md.gn_device_multi(torch.ones(3, 7), i0(3), mus(2), 5, out=torch.empty(7, 3, dtype=torch.float64))


def test_library_exports_and_declares_the_pair():
    from dex_ct_sim_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    for name in ('dexct_gn_decompose_multi', 'dexct_gn_multi_workspace_bytes'):
        assert hasattr(lib, name) and name in _native.SYMBOLS and re.search(name + r'\s*\(', hdr), name
    for macro, value in (('DEXCT_GN_MAX_MEAS', 4), ('DEXCT_GN_MAX_MATS', 3), ('DEXCT_GN_MULTI_FULL_LOOP', 1)):
        assert re.search(rf'#define {macro} {value}\b', hdr), macro
    assert (_native.GN_MAX_MEAS, _native.GN_MAX_MATS, _native.GN_MULTI_FULL_LOOP) == (4, 3, 1)
    lib.dexct_abi_version.restype = ctypes.c_int
    assert lib.dexct_abi_version() == 6 == _native.ABI_VERSION


def test_entry_points_reject_bad_arguments_without_a_launch():
    C = ctypes
    from dex_ct_sim_amd import _native
    lib = _native.load()
    EINVAL, ERANGE = -1, -2
    one = C.c_void_p(64)

    def call(g=one, f64=1, n_pix=10, K=3, M=2, i0=one, mus=one, nE=16, n_iters=5, mask=None, flags=0, out=one, ws=one):
        return lib.dexct_gn_decompose_multi(g, f64, n_pix, K, M, i0, mus, nE, n_iters, mask, 0.95, flags, out, ws, None)

    for kw in (dict(g=None), dict(i0=None), dict(mus=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(K=2, M=3) == EINVAL and call(K=3, M=1) == EINVAL and call(K=1, M=1) == EINVAL
    assert call(K=5) in (EINVAL, ERANGE) and call(K=5, M=3) in (EINVAL, ERANGE)
    assert call(K=4, M=4) in (EINVAL, ERANGE)
    assert call(n_pix=-1) == EINVAL and call(n_iters=0) == EINVAL and call(n_iters=-3) == EINVAL
    assert call(nE=0) == EINVAL and call(nE=5000) == ERANGE
    assert call(flags=2) == EINVAL and call(f64=2) == EINVAL
    assert call(out=C.c_void_p(68)) == EINVAL and call(g=C.c_void_p(68)) == EINVAL and call(g=C.c_void_p(66), f64=0) == EINVAL
    assert call(n_pix=1 << 40) == ERANGE
    assert call(n_pix=0) == 0                                     # nothing to do, nothing launched
    # the workspace: rows of M + K (1 + M + M (M + 1) / 2) doubles per energy behind a header, and a list of kept energies
    wb = lib.dexct_gn_multi_workspace_bytes
    for K, M in mr.SHAPES:
        n = wb(K, M, 100)
        assert n >= 8 * 100 * (M + K * (1 + M + M * (M + 1) // 2)) and n % 16 == 0 and n < 64 * 1024
    for bad in ((5, 2, 100), (4, 4, 100), (2, 3, 100), (3, 1, 100), (3, 2, 0), (3, 2, 5000)):
        assert wb(*bad) == 0, bad
