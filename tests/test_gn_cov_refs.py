"""The noise covariance of the decomposition, the part that needs no GPU: the restatement tests/gn_cov_refs.py is what the
Newton solve's estimates scatter by (Monte Carlo), the two kinds against each other, dose scaling, the restatement's own rounding
error (the yardstick of tests/test_gpu_gn_cov.py), and the argument checks of the Python layer and of the C entry points (which
return before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import gn_cov_refs as cr
import gn_multi_refs as mr
from conftest import INPUT, ROOT

LD = np.longdouble
A_TEST = (10.0, 1.0, 0.02)
# The float64 restatement's worst error ratio over the sweep measures 4.91 (test_restatement_rounding_is_what_the_bound_expects
# prints it per case); 8 is that figure with room for another libm, and what the comparisons below grant a float64 result.
RATIO_F64 = 8.0


@pytest.mark.parametrize('eid', [False, True], ids=['counting', 'integrating'])
@pytest.mark.parametrize('K,M', cr.SHAPES)
def test_formula_is_the_estimators_covariance(K, M, eid):
    """20 000 samples g = nu + sqrt(v) z at a = (10, 1, 0.02)[:M], flux 100 x the synthetic spectrum, each solved by 30 Newton
    steps of the restatement of the decomposition: the sample covariance of the estimates equals kind='estimator' element by
    element within 5 sigma of its sampling error sqrt((C_ii C_jj + C_ij^2) / (N - 1)).  (At flux 1 the three-material estimates
    are visibly biased - up to 4.5 sigma of the mean - so the test stays at flux 100.)"""
    N = 20000
    i0, i0v, mus = cr.tables(K, M, 60, eid, flux=100.0)
    a = np.array(A_TEST[:M])
    nu, v, _ = cr.sums(a[None], i0, i0v, mus)
    rng = np.random.default_rng([5, K, M, int(eid)])
    g = nu[0][:, None] + np.sqrt(v[0])[:, None] * rng.standard_normal((K, N))
    est = mr.newton_solve_multi(g, i0, mus, 30)
    assert est.shape == (N, M) and np.all(np.isfinite(est))
    again = mr.newton_solve_multi(g[:, :500], i0, mus, 40)
    assert mr.rel_err(again, est[:500]) <= 1e-9                    # every sample has converged
    S = np.cov(est.T)
    C = cr.covariance_full(a, i0, i0v, mus, 'estimator')[0]
    sigma = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / (N - 1))
    z = np.abs(S - C) / sigma
    bias = np.abs(est.mean(axis=0) - a) / np.sqrt(np.diag(C) / N)
    print(f'K={K} M={M} eid={eid}: worst element {z.max():.2f} sigma, bias of the mean {bias.max():.2f} sigma')
    assert z.max() <= 5.0


def test_restatement_rounding_is_what_the_bound_expects():
    """|C_f64 - C_ld|_ij / (cond(corr_p) 2^-53 sqrt(C_ii C_jj)) of the float64 restatement over the GPU sweep, per pixel:
    measured 1.29 .. 4.91 (worst: K=4 M=3, 239 energies, estimator)."""
    r = cr.sweep_ratio_f64()
    for key, val in r.items():
        print(key, f'{val:.2f}')
    worst = max(r.values())
    print(f'worst {worst:.2f}')
    assert 0.5 <= worst <= RATIO_F64


@pytest.mark.parametrize('K,M', cr.SHAPES)
def test_crlb_against_estimator(K, M):
    for eid in (False, True):
        for n_e in (8, 60):
            a, i0, i0v, mus = cr.sweep_case(K, M, n_e, eid=eid, n_pix=200)
            est = cr.covariance_full(a, i0, i0v, mus, 'estimator', LD)
            crlb = cr.covariance_full(a, i0, i0v, mus, 'crlb', LD)
            assert np.all(np.isfinite(est.astype(np.float64))) and np.all(np.isfinite(crlb.astype(np.float64)))
            d = np.sqrt(np.einsum('pii->pi', est)).astype(np.float64)
            cond = cr.corr_cond(est)
            # crlb <= estimator in the Loewner order: the scaled difference has no eigenvalue below the rounding of either
            D = (est - crlb).astype(np.float64) / (d[:, :, None] * d[:, None, :])
            low = np.linalg.eigvalsh(D).min(axis=1)
            assert np.all(low >= -RATIO_F64 * M * cond * cr.EPS), (K, M, eid, n_e, low.min())
            ratio = (np.einsum('pii->pi', crlb) / np.einsum('pii->pi', est)).astype(np.float64)
            if K == M or not eid:
                # equal to rounding: in long double to 2^-11 of the float64 unit (x RATIO_F64, x 10 of room -> 0.05), and the
                # float64 results within the float64 restatement's own error of each other
                assert cr.error_ratio(cr.pack(est), crlb) <= 0.05, (K, M, eid, n_e)
                assert cr.error_ratio(cr.covariance(a, i0, i0v, mus, 'estimator'), crlb) <= RATIO_F64
                assert cr.error_ratio(cr.covariance(a, i0, i0v, mus, 'crlb'), est) <= RATIO_F64
            else:
                print(f'K={K} M={M} nE={n_e}: crlb / estimator on the diagonal {ratio.min():.4f} .. {ratio.max():.4f}')
                assert np.all(ratio < 0.999) and np.all(ratio > 0.5)


@pytest.mark.parametrize('kind', cr.KINDS)
def test_dose_scaling(kind):
    """C(flux f) = C(1) / f: bit for bit for a power of two, within the restatement's rounding for f = 100"""
    for K, M in cr.SHAPES:
        a, i0, i0v, mus = cr.sweep_case(K, M, 60, n_pix=100)
        one = cr.covariance(a, i0, i0v, mus, kind)
        assert np.array_equal(cr.covariance(a, 128.0 * i0, 128.0 * i0v, mus, kind) * 128.0, one)
        ld = cr.covariance_full(a, i0, i0v, mus, kind, LD)
        assert cr.error_ratio(cr.covariance(a, 100.0 * i0, 100.0 * i0v, mus, kind) * 100.0, ld) <= RATIO_F64 + 2.0


def test_packing_and_special_states():
    assert cr.tri_index(2) == [(0, 0), (0, 1), (1, 1)] and cr.tri_index(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    a, i0, i0v, mus = cr.sweep_case(4, 3, 60, n_pix=6)
    ref = cr.covariance(a, i0, i0v, mus)
    hurt = a.copy()
    hurt[2, 1] = np.nan
    got = cr.covariance(hurt, i0, i0v, mus)
    assert np.all(np.isnan(got[2])) and np.array_equal(np.delete(got, 2, axis=0), np.delete(ref, 2, axis=0))
    same = mus.copy()
    same[1] = same[0]
    assert not np.any(np.isfinite(cr.covariance(a, i0, i0v, same)))


def test_tables_with_variance():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md
    specs = [dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV') for kv in (140, 80)]
    for eid, det in ((True, 'eta_eid_mv.bin'), (False, 'eta_pcd_Si_30mm.bin')):
        ct = dx.FanBeamGeometry(N_channels=16, N_proj=4, eid=eid, detector_file=os.path.join(INPUT, 'detector', det))
        plain = md.decomposition_tables_multi(ct, specs)
        assert len(plain) == 3
        ee, i0, mus, i0v = md.decomposition_tables_multi(ct, specs, with_variance=True)
        assert all(np.array_equal(x, y) for x, y in zip(plain, (ee, i0, mus)))
        assert np.array_equal(i0v, i0 * ee if eid else i0) and i0v.shape == i0.shape


def test_value_errors_come_before_any_device_access():
    import torch
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md, plots
    nE = 12
    ct = dx.FanBeamGeometry(N_channels=5, N_proj=2)
    spec = dx.xRaySpectrum.from_arrays('s', np.arange(1.0, nE + 1.0), np.ones(nE))
    s = np.ones((2, 5))
    three = (md.matcomp1, md.matcomp2, 'H(11.2)O(88.8)')
    for args, kw in ((((s, s), [spec] * 2), dict(kind='fisher')),
                     (((s, s, s), [spec] * 3), {}),                                    # three sinograms, two materials
                     (((s, s), [spec] * 2), dict(materials=three)),                    # more materials than spectra
                     (((s, s), [spec] * 5), {}),                                       # too many spectra
                     (((s,), [spec] * 2), dict(materials=(md.matcomp1,))),             # a single material
                     (((s, np.ones((2, 6))), [spec] * 2), {}),                         # shapes disagree
                     (((s, s), [spec] * 2), dict(mask_from=np.ones((3, 5))))):
        with pytest.raises(ValueError):
            md.get_basismat_covariance(ct, *args, **kw)
    a = torch.ones(7, 2, dtype=torch.float64)
    i0, mus = np.ones((3, nE)), np.ones((2, nE))
    for args, kw in (((a, i0, i0, mus), dict(kind='bound')),
                     ((a, i0, np.ones((2, nE)), mus), {}),                             # i0v and i0 disagree
                     ((a, i0, i0, np.ones((3, nE))), {}),                              # a and mus disagree
                     ((torch.ones(7, 3, dtype=torch.float64), np.ones((2, nE)), np.ones((2, nE)), np.ones((3, nE))), {}),
                     ((a, np.ones((5, nE)), np.ones((5, nE)), mus), {}),
                     ((a, i0, i0, mus), dict(mask_g=torch.ones(7))),                   # a mask without its maximum
                     ((a, i0, i0, mus), dict(mask_g=torch.ones(6), mask_max=torch.ones(()))),
                     ((a, i0, i0, mus), dict(out=torch.empty(7, 2, dtype=torch.float64))),
                     ((np.ones((7, 2)), i0, i0, mus), {})):
        with pytest.raises(ValueError):
            md.gn_covariance_device(*args, **kw)
    # host memory is refused once the shapes are right: the kernel takes device addresses
    for kw in (dict(), dict(out=torch.empty(7, 3, dtype=torch.float64))):
        with pytest.raises(ValueError, match='device'):
            md.gn_covariance_device(a, i0, i0, mus, **kw)
    for cov, E, mats in ((np.ones((4, 6)), 60.0, None), (np.ones((4, 3)), 60.0, three), (np.ones((4, 3)), [50.0, 60.0], None)):
        with pytest.raises(ValueError):
            plots.vmi_variance(cov, E, mats)
    with pytest.raises(ValueError):
        plots.vmi_noise_sweep([50.0, 60.0], np.ones((4, 6)))


def test_noise_sweep_is_the_quadratic_form_of_the_mean():
    """host arithmetic only: NumPy in needs no device"""
    from dex_ct_sim_amd import matdecomp as md, plots, xcompy
    rng = np.random.default_rng(3)
    L = rng.standard_normal((50, 2, 2))
    C = L @ np.swapaxes(L, 1, 2)
    cov = cr.pack(C).reshape(5, 10, 3)
    Evals = np.arange(40.0, 141.0, 10.0)
    var, e_min = plots.vmi_noise_sweep(Evals, cov)
    u = np.stack([xcompy.mixatten(md.matcomp1, Evals), xcompy.mixatten(md.matcomp2, Evals)])
    ref = np.einsum('me,pmn,ne->e', u, C, u) / 50
    assert np.allclose(var, ref, rtol=1e-12, atol=0.0) and e_min == Evals[np.argmin(ref)]
    mask = np.zeros((5, 10), bool)
    mask[1:3] = True
    var_m, _ = plots.vmi_noise_sweep(Evals, cov, mask=mask)
    assert np.allclose(var_m, np.einsum('me,pmn,ne->e', u, C[10:30], u) / 20, rtol=1e-12, atol=0.0)


def test_library_exports_and_declares_the_entry_points():
    from dex_ct_sim_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    for name in ('dexct_gn_covariance', 'dexct_gn_cov_workspace_bytes', 'dexct_cov_quadform'):
        assert hasattr(lib, name) and name in _native.SYMBOLS and re.search(name + r'\s*\(', hdr), name
    for macro, value in (('DEXCT_COV_ESTIMATOR', 0), ('DEXCT_COV_CRLB', 1)):
        assert re.search(rf'#define {macro} {value}\b', hdr), macro
    assert (_native.COV_ESTIMATOR, _native.COV_CRLB) == (0, 1)
    lib.dexct_abi_version.restype = ctypes.c_int
    assert lib.dexct_abi_version() == 6 == _native.ABI_VERSION


def test_binding_return_types():
    """every size query returns int64 through the binding - a layout beyond 2 GiB comes back whole - , dexct_strerror a string,
    every other entry point the int status"""
    from dex_ct_sim_amd import _native
    lib = _native.load()
    sizes = sorted(n for n in _native.SYMBOLS if n.endswith('_bytes'))
    assert sizes == sorted(_native.SIZE_QUERIES) and len(sizes) == 4
    for name in _native.SYMBOLS:
        want = ctypes.c_int64 if name in sizes else ctypes.c_char_p if name == 'dexct_strerror' else ctypes.c_int
        assert getattr(lib, name).restype is want, name
    big = lib.dexct_cone_layout_bytes(2048, 2048, 640)
    assert big > 1 << 31 and big >= 2048 * 2048 * 640


def test_entry_points_reject_bad_arguments_without_a_launch():
    C = ctypes
    from dex_ct_sim_amd import _native
    lib = _native.load()
    EINVAL, ERANGE = -1, -2
    one = C.c_void_p(64)

    def call(a=one, n_pix=10, K=3, M=2, i0=one, i0v=one, mus=one, nE=16, kind=0, mask_g=None, f64=1, mask_max=None, out=one, ws=one):
        return lib.dexct_gn_covariance(a, n_pix, K, M, i0, i0v, mus, nE, kind, mask_g, f64, mask_max, 0.95, out, ws, None)

    for kw in (dict(a=None), dict(i0=None), dict(i0v=None), dict(mus=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(K=2, M=3) == EINVAL and call(K=3, M=1) == EINVAL and call(K=1, M=1) == EINVAL
    assert call(K=5) in (EINVAL, ERANGE) and call(K=5, M=3) in (EINVAL, ERANGE) and call(K=4, M=4) in (EINVAL, ERANGE)
    assert call(n_pix=-1) == EINVAL and call(nE=0) == EINVAL and call(nE=5000) == ERANGE
    assert call(kind=2) == EINVAL and call(kind=-1) == EINVAL and call(f64=2) == EINVAL
    assert call(mask_g=one) == EINVAL                              # a mask without its maximum
    assert call(a=C.c_void_p(68)) == EINVAL and call(out=C.c_void_p(68)) == EINVAL and call(ws=C.c_void_p(68)) == EINVAL
    assert call(mask_g=C.c_void_p(68), mask_max=one) == EINVAL and call(mask_g=C.c_void_p(66), f64=0, mask_max=one) == EINVAL
    assert call(n_pix=1 << 40) == ERANGE
    assert call(n_pix=0) == 0 and call(n_pix=0, kind=1, mask_g=one, mask_max=one) == 0       # nothing to do, nothing launched
    wb = lib.dexct_gn_cov_workspace_bytes
    for K, M in cr.SHAPES:
        n = wb(K, M, 100)
        assert n >= 8 * 100 * (M + K * (M + 2)) + 4 * 100 and n % 16 == 0 and n < 32 * 1024
    for bad in ((5, 2, 100), (4, 4, 100), (2, 3, 100), (3, 1, 100), (3, 2, 0), (3, 2, 5000)):
        assert wb(*bad) == 0, bad

    def quad(cov=one, n_pix=10, M=2, u=None, out=one):
        uv = (C.c_double * 3)(1.0, 2.0, 3.0)
        return lib.dexct_cov_quadform(cov, n_pix, M, uv if u is None else u, out, None)

    assert quad(cov=None) == EINVAL and quad(out=None) == EINVAL and quad(u=C.c_void_p(0)) == EINVAL
    assert quad(M=1) == EINVAL and quad(M=4) == ERANGE and quad(n_pix=-1) == EINVAL and quad(n_pix=1 << 40) == ERANGE
    assert quad(cov=C.c_void_p(68)) == EINVAL and quad(out=C.c_void_p(68)) == EINVAL
    assert quad(n_pix=0) == 0 and quad(n_pix=0, M=3) == 0
