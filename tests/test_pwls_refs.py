"""The joint PWLS iteration (dex-ct-sim_amd/iterative.py, pwls) on the CPU: properties of its restatement tests/pwls_refs.py on
the dense system matrix of tests/iter_refs.py, the argument checks of the four entry points of csrc/pwls.hip (they return
before any launch, so they need no device) and those of get_basismat_recon.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import iter_refs as ir
import pwls_refs as pr
from pwls_refs import F32, F64

EINVAL = -1


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = ir.system_matrix(ir.small(name))
    A.setflags(write=False)
    return A


def problem(name, K, rho, zero_fraction, seed):
    scan, A = ir.small(name), matrix(name)
    rng = np.random.default_rng(seed)
    shape = (scan.n_views, scan.n_rows, scan.n_ch)
    x_true = rng.uniform(0.0, 1.0, (K, A.shape[1]))
    b = np.stack([(A @ x_true[k]) * rng.uniform(0.8, 1.2, A.shape[0]) - 0.03 for k in range(K)]).reshape((K,) + shape)
    _, W = pr.correlated_weights(rng, shape, K, rho, zero_fraction)
    return scan, A, b, W


@pytest.mark.parametrize('K,rho,zero_fraction', [(2, -0.95, 0.0), (3, -0.6, 0.0), (2, -0.9, 0.1)])
def test_objective_never_increases_with_one_subset(K, rho, zero_fraction):
    scan, A, b, W = problem('c53', K, rho, zero_fraction, 21)
    if zero_fraction:
        assert 0 < np.mean(np.all(W.reshape(W.shape[0], -1) == 0, axis=0)) < 0.3
    beta, delta = [0.5, 2.0, 1.0][:K], [0.05, 0.2, 0.1][:K]
    hist = []
    x = pr.pwls_ref(A, b, W, 30, 1, beta, delta, False, None, (scan.nz, scan.ny, scan.nx), F64, hist)
    hist.append(pr.objective_ref(A, b, W, x, beta, delta, K))
    assert len(hist) == 31 and hist[-1] < hist[0]
    assert all(h1 <= h0 * (1 + 1e-13) for h0, h1 in zip(hist[:-1], hist[1:])), hist
    # the history is the objective: the last entry restated from scratch
    x29 = pr.pwls_ref(A, b, W, 29, 1, beta, delta, False, None, (scan.nz, scan.ny, scan.nx), F64)
    assert abs(pr.objective_ref(A, b, W, x29, beta, delta, K) - hist[29]) <= 1e-12 * hist[29]


@pytest.mark.parametrize('K,rho', [(1, 0.0), (2, -0.95), (3, -0.6)])
def test_majoriser_dominates_the_data_hessian(K, rho):
    scan, A = ir.small('c53'), matrix('c53')
    rng = np.random.default_rng(22)
    _, W = pr.correlated_weights(rng, (A.shape[0],), K, rho, 0.1)
    n = A.shape[1]
    R = A.sum(1)
    m = pr.majorizer_ref(W, R, K)
    d = np.concatenate([A.T @ m[k] for k in range(K)])
    H = np.zeros((K * n, K * n))
    for k in range(K):
        for l in range(K):
            H[k * n:(k + 1) * n, l * n:(l + 1) * n] = A.T @ (W[pr.tri(K, k, l)][:, None] * A)
    low = np.linalg.eigvalsh(np.diag(d) - H).min()
    print(f'K={K}: smallest eigenvalue of diag(d) - A^T W A = {low:.3e}, max d = {d.max():.3e}')
    assert low >= -1e-9 * d.max()


def test_precision_ref_inverts_and_fills():
    rng = np.random.default_rng(23)
    for K in (1, 2, 3):
        cov, _ = pr.correlated_weights(rng, (40,), K, -0.999 if K == 2 else -0.7)
        cov[3] = 0.0
        cov[5, 0] = np.nan
        cov[7, -1] = np.inf
        cov[9, 0] = -cov[9, 0]
        if K > 1:
            cov[11, 1] = 10.0 * cov[11, 0]                       # indefinite
        cov[13] *= 1e-42                                         # its inverse leaves the float32 range
        w, ok = pr.precision_ref(cov, K, 0.25)
        bad = [3, 5, 7, 9] + ([11] if K > 1 else []) + [13]
        assert not ok[bad].any() and ok.sum() == 40 - len(bad)
        prod = pr.full(cov[ok], K) @ pr.full(w.T[ok], K)
        assert np.allclose(prod, np.eye(K), rtol=0, atol=1e-9)
        for t in range(w.shape[0]):
            diag = t in [pr.tri(K, k, k) for k in range(K)]
            assert np.all(w[t, bad] == (0.25 if diag else 0.0))


def test_update_ref_is_the_formula_on_one_pixel():
    # one channel, a row of three pixels, the centre above its neighbours by less than, exactly and more than delta
    for t in (0.05, 0.1, 0.4):
        x = np.array([[[[1.0, 1.0 + t, 1.0]]]])
        g, d = np.full_like(x, 0.3), np.full_like(x, 2.0)
        new = pr.update_ref(x, g, d, [0.5], [0.1], False)
        b32, d32 = F64(F32(0.5)), F64(F32(0.1))
        clip = min(t, d32)
        wgt = 1.0 if t <= d32 else d32 / t
        assert np.isclose(new[0, 0, 0, 1], (1.0 + t) - (0.3 + b32 * 2 * clip) / (2.0 + 2 * b32 * 2 * wgt), rtol=1e-14, atol=0)
    assert pr.penalty_ref(np.array([[[[0.0, 0.05], [0.4, 0.05]]]]), [2.0], [0.1]) == pytest.approx(
        2.0 * (0.5 * 0.05 ** 2 + F64(F32(0.1)) * (0.35 + 0.4) - F64(F32(0.1)) ** 2), rel=1e-12)


# ---- the library and the host layer, without a device --------------------------------------------------------------------------

NAMES = ('dexct_cov_precision', 'dexct_pwls_majorizer', 'dexct_pwls_residual', 'dexct_pwls_update')


def test_library_exports_and_declares_the_entry_points():
    from conftest import ROOT
    from dex_ct_sim_amd import _native
    lib = C.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _native.SYMBOLS and re.search(name + r'\s*\(', hdr), name
    assert re.search(r'#define DEXCT_ABI_VERSION 6\b', hdr) and _native.ABI_VERSION == 6


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Every refusal comes back before the first launch and before any pointer is followed: the addresses below are not
    mapped, and the process has no device."""
    from dex_ct_sim_amd import _native
    lib = _native.load()
    P, Q = 0x10000, 0x20000000                                    # two "buffers" far apart
    two = (C.c_double * 3)(0.1, 0.1, 0.1)
    for K in (0, 4, -1):
        assert lib.dexct_cov_precision(P, 8, K, 0.0, Q, None) == EINVAL
        assert lib.dexct_pwls_majorizer(P, P, 8, K, Q, None) == EINVAL
        assert lib.dexct_pwls_residual(P, P, P, P, 64, K, 4, 1, 16, Q, None, None) == EINVAL
        assert lib.dexct_pwls_update(P, P, P, K, 1, 2, 4, 1.0, two, two, 0, Q, None, None) == EINVAL
    for w_fill in (-1.0, -1e-300, float('inf'), float('nan')):
        assert lib.dexct_cov_precision(P, 8, 2, w_fill, Q, None) == EINVAL
    assert lib.dexct_cov_precision(None, 8, 2, 0.0, Q, None) == EINVAL
    assert lib.dexct_cov_precision(P, 8, 2, 0.0, None, None) == EINVAL
    assert lib.dexct_cov_precision(P, -1, 2, 0.0, Q, None) == EINVAL
    for args in ((None, P, 8, 2, Q), (P, None, 8, 2, Q), (P, P, 8, 2, None), (P, P, -1, 2, Q)):
        assert lib.dexct_pwls_majorizer(*args, None) == EINVAL
    ok = [P, P, P, P, 64, 2, 4, 1, 16, Q, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (7, 0), (7, -1), (6, 0), (8, 0), (4, 63), (9, None)):
        args = list(ok)
        args[i] = v
        assert lib.dexct_pwls_residual(*args, None) == EINVAL, (i, v)          # (9: neither q nor an objective)
    ok = [P, P, P, 2, 1, 2, 4, 1.0, two, two, 0, Q, None]
    for i, v in ((0, None), (1, None), (2, None), (8, None), (9, None), (11, None), (4, 0), (5, 0), (6, 0), (7, 0.0), (7, float('nan')),
                 (11, P), (11, P + 4 * 15), (8, (C.c_double * 3)(0.1, -0.1, 0.1)), (9, (C.c_double * 3)(0.1, 0.0, 0.1)),
                 (9, (C.c_double * 3)(0.1, float('inf'), 0.1))):
        args = list(ok)
        args[i] = v
        assert lib.dexct_pwls_update(*args, None) == EINVAL, (i, v)           # (11, P...: old and new images overlap)
    assert lib.dexct_cov_precision(P, 2 ** 41, 2, 0.0, Q, None) == -2
    # nothing to do is no error, and launches nothing either
    assert lib.dexct_cov_precision(P, 0, 2, 0.0, Q, None) == 0 and lib.dexct_pwls_majorizer(P, P, 0, 2, Q, None) == 0


def test_host_argument_checks_need_no_device():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import back_project as bp, iterative
    assert dx.get_basismat_recon is bp.get_basismat_recon and 'get_basismat_recon' in dx.__all__
    ct = dx.FanBeamGeometry(N_channels=16, N_proj=12)
    s, cov = np.zeros((12, 16), F32), np.ones((12, 16, 3))
    cases = [
        (dict(sinos=(s, s[:, :15])), 'differ in shape'),
        (dict(sinos=(s[:11], s[:11])), 'does not match the scanner'),
        (dict(cov=np.ones((12, 16, 6))), 'covariance sinogram'),
        (dict(cov=np.ones((12, 16))), 'covariance sinogram'),
        (dict(sinos=()), 'channels'),
        (dict(sinos=(s,) * 4, cov=np.ones((12, 16, 10))), 'channels'),
        (dict(ct=dx.FanBeamGeometry(N_channels=16, N_proj=12, N_rows=4, cone=True)), 'cone-beam'),
        (dict(FOV=2.0 * ct.SID), 'source circle'),
        (dict(beta=-0.1), 'beta'),
        (dict(beta=(0.1, 0.1, 0.1)), 'beta'),
        (dict(delta=0.0), 'delta'),
        (dict(delta=(0.1, float('nan'))), 'delta'),
        (dict(n_subsets=0), 'n_subsets'),
        (dict(n_subsets=13), 'n_subsets'),
        (dict(n_iters=0), 'n_iters'),
        (dict(init='ones'), 'init'),
        (dict(w_fill=-1.0), 'w_fill'),
        (dict(window='boxcar'), 'window'),
    ]
    for kw, match in cases:
        kw = dict(kw)
        sinos, c, geo = kw.pop('sinos', (s, s)), kw.pop('cov', cov), kw.pop('ct', ct)
        pos = dict(FOV=30.0, beta=0.1, delta=0.01)
        pos.update({k: kw.pop(k) for k in list(kw) if k in pos})
        with pytest.raises(ValueError, match=match):
            bp.get_basismat_recon(sinos, c, geo, 8, pos['FOV'], 1.0, pos['beta'], pos['delta'], **kw)
    # get_recon: the K = 1 case
    with pytest.raises(ValueError, match='needs weights'):
        bp.get_recon(s, ct, None, 8, 30.0, 1.0, method='pwls')
    with pytest.raises(ValueError, match='shape of the sinogram'):
        bp.get_recon(s, ct, None, 8, 30.0, 1.0, method='pwls', weights=np.ones((12, 15)))
    with pytest.raises(ValueError, match='delta'):
        bp.get_recon(s, ct, None, 8, 30.0, 1.0, method='pwls', weights=np.ones((12, 16)), delta=-1.0)
    with pytest.raises(ValueError, match="method='pwls'"):
        bp.get_recon(s, ct, None, 8, 30.0, 1.0, weights=np.ones((12, 16)))
    with pytest.raises(ValueError, match='slices'):
        bp.get_recon(s, ct, None, 8, 30.0, 1.0, method='pwls', weights=np.ones((12, 16)), slices=(1, 0.0, 0.1))
    assert iterative.channels_of(1) == 1 and iterative.channels_of(3) == 2 and iterative.channels_of(6) == 3
    with pytest.raises(ValueError):
        iterative.channels_of(4)


def test_main_refuses_pwls_without_its_covariance(capsys):
    from dex_ct_sim_amd import main as m
    for argv, msg in ((['--recon', 'pwls'], 'needs --covariance'),
                      (['--recon', 'pwls', '--covariance', '--recon-delta', '0'], '--recon-delta > 0'),
                      (['--recon', 'pwls', '--covariance', '--recon-beta', '-1'], '--recon-beta must be >= 0'),
                      (['--recon', 'pwls', '--covariance', '--noise-maps'], 'needs --recon fbp')):
        with pytest.raises(SystemExit):
            m.main(argv)
        assert msg in capsys.readouterr().err
