"""dexct_gn_covariance and dexct_cov_quadform on the device, against the long-double restatement tests/gn_cov_refs.py (which
tests/test_gn_cov_refs.py shows to be the covariance of what the Newton solve returns).

The bound per pixel and element: |C_dev - C_ld|_ij <= c cond(corr_p) 2^-53 sqrt(C_ii C_jj), corr_p that pixel's long-double
correlation matrix.  c = 4 x the worst such ratio of the FLOAT64 NumPy restatement over the same sweep, computed at the start
of the module (gn_cov_refs.sweep_ratio_f64: 4.91 on x86-64, so c = 19.6): the kernel sums in another order, divides by a refined
v_rcp_f64 and uses a table exponential, and gets four times what NumPy's own rounding takes.
"""
import os

import numpy as np
import pytest
import torch

import gn_cov_refs as cr
from conftest import INPUT
from guarded import Arena, twice

pytestmark = pytest.mark.gpu
F64 = np.float64
LD = np.longdouble


@pytest.fixture(scope='module')
def c_bound():
    worst = max(cr.sweep_ratio_f64().values())
    print(f'float64 restatement: worst ratio {worst:.2f}; the kernel is allowed {4.0 * worst:.2f}')
    return 4.0 * worst


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dev_cov(a, i0, i0v, mus, kind, mask_g=None, mask_max=None, mask_frac=0.95):
    """states a [P, M] (NumPy) -> NumPy [P, T] through gn_covariance_device"""
    from dex_ct_sim_amd import matdecomp as md
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).to('cuda')
    if mask_g is not None:
        mask_g = torch.from_numpy(np.ascontiguousarray(mask_g)).to('cuda')
        mask_max = torch.tensor(float(mask_max), dtype=torch.float64, device='cuda')
    return md.gn_covariance_device(t, i0, i0v, mus, kind, mask_g=mask_g, mask_max=mask_max, mask_frac=mask_frac).cpu().numpy()


_ld = {}


def sweep_reference(K, M, n_e, kind):
    """the long-double restatement on the 1000 pixels of a sweep case (every smaller size is a prefix), once"""
    key = (K, M, n_e, kind)
    if key not in _ld:
        a, i0, i0v, mus = cr.sweep_case(K, M, n_e)
        _ld[key] = cr.covariance_full(a, i0, i0v, mus, kind, LD)
    return cr.sweep_case(K, M, n_e) + (_ld[key],)


@pytest.mark.parametrize('kind', cr.KINDS)
@pytest.mark.parametrize('n_e', cr.SWEEP_ENERGIES)
@pytest.mark.parametrize('K,M', cr.SHAPES)
def test_kernel_against_the_long_double_restatement(hip, c_bound, K, M, n_e, kind):
    """The c each result needs, per case (worst over the pixel counts and pixels).  The float64 NumPy restatement: 1.29 .. 4.91
    (CPU, tests/test_gn_cov_refs.py), hence the allowance 4 x 4.91 = 19.6.  The kernel, measured on the MI355X: 1.18 .. 4.83
    (worst: K=4 M=3, 239 energies, estimator; crlb 1.18 .. 3.68, estimator 2.25 .. 4.83)."""
    a, i0, i0v, mus, ld = sweep_reference(K, M, n_e, kind)
    worst = 0.0
    for n_pix in cr.SWEEP_PIXELS:
        got = dev_cov(a[:n_pix], i0, i0v, mus, kind)
        assert got.shape == (n_pix, M * (M + 1) // 2) and got.dtype == F64
        r = cr.error_ratio(got, ld[:n_pix])
        worst = max(worst, r) if np.isfinite(r) else float('nan')
        print(f'K={K} M={M} nE={n_e} {kind} n_pix={n_pix}: ratio {r:.2f} (allowed {c_bound:.2f})')
        assert r <= c_bound, (n_pix, r)
    print(f'K={K} M={M} nE={n_e} {kind}: worst ratio {worst:.2f}')


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('K,M,kind', [(4, 3, 'estimator'), (2, 2, 'crlb')])
def test_mask(hip, K, M, kind, f32):
    a, i0, i0v, mus = cr.sweep_case(K, M, 60)
    a = a[:300]
    T = M * (M + 1) // 2
    plain = dev_cov(a, i0, i0v, mus, kind)
    assert np.all(np.isfinite(plain))
    g0 = np.random.default_rng(2).uniform(1.0, 100.0, 300)
    g0 = g0.astype(np.float32) if f32 else g0
    gmax = float(g0.max())
    for frac in (0.3, 0.95):
        air = g0.astype(F64) >= frac * gmax
        assert air.any() and not air.all()
        got = dev_cov(a, i0, i0v, mus, kind, mask_g=g0, mask_max=gmax, mask_frac=frac)
        assert np.array_equal(bits(got[air]), np.zeros((int(air.sum()), T), np.uint64))          # +0.0 in every element
        assert np.array_equal(bits(got[~air]), bits(plain[~air]))
    # a mask that masks nothing gives the bits of no mask
    none = dev_cov(a, i0, i0v, mus, kind, mask_g=g0, mask_max=gmax, mask_frac=2.0)
    assert np.array_equal(bits(none), bits(plain))


@pytest.mark.parametrize('K,M', [(2, 2), (4, 3)])
def test_special_pixels(hip, c_bound, K, M):
    a, i0, i0v, mus = cr.sweep_case(K, M, 60)
    a = a[:130].copy()
    err_before = hip.dexct_last_hip_error()
    for kind in cr.KINDS:
        plain = dev_cov(a, i0, i0v, mus, kind)
        hurt = a.copy()
        hurt[3, 0], hurt[64, M - 1], hurt[129, 1], hurt[70, 0] = np.nan, np.inf, np.nan, -np.inf
        got = dev_cov(hurt, i0, i0v, mus, kind)
        keep = np.ones(130, bool)
        keep[[3, 64, 70, 129]] = False
        assert np.array_equal(bits(got[keep]), bits(plain[keep]))
        assert np.all(np.isnan(got[3])) and np.all(np.isnan(got[129]))
        # an infinite component acts through the clip, as in the restatement: +inf clips every exponent at -700 and the
        # determinant underflows, -inf clips at +700 and the sums overflow - nothing finite either way
        ref = cr.covariance(hurt[[64, 70]], i0, i0v, mus, kind)
        assert not np.any(np.isfinite(ref)) and not np.any(np.isfinite(got[[64, 70]]))
        # ... unless it meets mu = 0 at a weighted energy: inf * 0 is a NaN exponent, which the restatement's clip keeps
        zero_mu = mus.copy()
        zero_mu[M - 1, 7] = 0.0
        assert np.all(np.isnan(cr.covariance(hurt[[64]], i0, i0v, zero_mu, kind)))
        got0 = dev_cov(hurt, i0, i0v, zero_mu, kind)
        assert np.all(np.isnan(got0[64])) and np.all(np.isfinite(got0[keep]))
        # two identical basis rows: a singular matrix in every pixel, inf / NaN and no fault
        same = mus.copy()
        same[1] = same[0]
        sing = dev_cov(a, i0, i0v, same, kind)
        assert not np.any(np.isfinite(sing))
        # states that clip the exponent of EVERY energy (at -700 and at +700; the spectra scaled so that the sums stay in
        # range): without the clip the terms would differ by hundreds of orders of magnitude
        for a0, scale in ((7000.0, 1e250), (-7000.0, 1e-250)):
            st = np.array([[a0, 1.0, 0.02][:M]])
            ld = cr.covariance_full(st, i0 * scale, i0v * scale, mus, kind, LD)
            assert np.all(np.isfinite(ld.astype(F64)))
            r = cr.error_ratio(dev_cov(st, i0 * scale, i0v * scale, mus, kind), ld)
            print(f'K={K} M={M} {kind} a0={a0}: ratio {r:.2f}')
            assert r <= c_bound
    torch.cuda.synchronize()
    assert hip.dexct_last_hip_error() == err_before


def guarded_cov(lib, a, i0, i0v, mus, kind, mask_g=None, mask_max=None):
    """dexct_gn_covariance with every buffer between guards, run with 0x00 and with 0xFF fill (guarded.twice): outputs
    bit-identical (so every one of the T n_pix doubles is written and nothing is read from the workspace before it is written),
    guards of out_cov and of the promised workspace bytes intact.  The library's last HIP error is compared with its value before
    (it is per thread and never cleared), as tests/test_gpu_gn_multi.py does."""
    from dex_ct_sim_amd._device import stream_ptr
    n_pix, M = a.shape
    K, n_e = i0.shape
    T = M * (M + 1) // 2
    ar = Arena('cuda', None)
    err_before = lib.dexct_last_hip_error()
    for name, arr in (('a', a), ('i0', i0), ('i0v', i0v), ('mus', mus)):
        arr = np.ascontiguousarray(arr, F64)
        ar.alloc(name, arr.nbytes).put(arr)
    if mask_g is not None:
        ar.alloc('mask_g', mask_g.nbytes).put(mask_g)
        ar.alloc('mask_max', 8).put(np.array([mask_max], F64))
    ar.alloc('workspace', lib.dexct_gn_cov_workspace_bytes(K, M, n_e))
    ar.alloc('out_cov', 8 * T * n_pix)

    def launch():
        assert lib.dexct_gn_covariance(ar['a'].ptr, n_pix, K, M, ar['i0'].ptr, ar['i0v'].ptr, ar['mus'].ptr, n_e,
                                       cr.KINDS.index(kind), ar['mask_g'].ptr if mask_g is not None else None,
                                       int(mask_g is not None and mask_g.dtype == F64),
                                       ar['mask_max'].ptr if mask_g is not None else None, 0.5, ar['out_cov'].ptr,
                                       ar['workspace'].ptr, stream_ptr()) == 0

    out = twice(ar, launch, ['out_cov'], scratch=['workspace'])['out_cov'].view(F64).reshape(n_pix, T)
    assert lib.dexct_last_hip_error() == err_before
    return out


@pytest.mark.parametrize('n_pix', [1, 65, 1000])
@pytest.mark.parametrize('K,M,kind', [(4, 3, 'estimator'), (3, 2, 'crlb')])
def test_guard_banded_buffers(hip, K, M, kind, n_pix):
    a, i0, i0v, mus = cr.sweep_case(K, M, 60)
    a = np.ascontiguousarray(a[:n_pix])
    got = guarded_cov(hip, a, i0, i0v, mus, kind)
    assert np.array_equal(bits(got), bits(dev_cov(a, i0, i0v, mus, kind)))
    # with a mask (float32 counts), and with energies that no measurement weights (rows the workspace never receives)
    g0 = np.random.default_rng(4).uniform(1.0, 100.0, n_pix).astype(np.float32)
    sparse, sparse_v = i0.copy(), i0v.copy()
    sparse[:, ::3] = 0.0
    sparse_v[:, ::3] = 0.0
    masked = guarded_cov(hip, a, sparse, sparse_v, mus, kind, mask_g=g0, mask_max=100.0)
    air = g0 >= 50.0
    assert not masked[air].any()
    dense = dev_cov(a, np.ascontiguousarray(sparse[:, sparse.any(axis=0)]), np.ascontiguousarray(sparse_v[:, sparse.any(axis=0)]),
                    np.ascontiguousarray(mus[:, sparse.any(axis=0)]), kind)
    assert np.array_equal(bits(masked[~air]), bits(dense[~air]))          # dropping unweighted energies changes no bit


def quadform_numpy(cov, u):
    """sum_i u_i^2 C_ii + 2 sum_(i<j) u_i u_j C_ij in the order of the packed triangle, and sum |u_i C_ij u_j|"""
    M = len(u)
    r = np.zeros(cov.shape[0])
    s = np.zeros(cov.shape[0])
    for t, (i, j) in enumerate(cr.tri_index(M)):
        w = u[i] * u[i] if i == j else 2.0 * (u[i] * u[j])
        r = w * cov[:, t] if t == 0 else r + w * cov[:, t]
        s = s + np.abs(w * cov[:, t])
    return r, s


@pytest.mark.parametrize('M', [2, 3])
def test_quadform(hip, M):
    from dex_ct_sim_amd._device import stream_ptr
    rng = np.random.default_rng([9, M])
    T = M * (M + 1) // 2
    for n_pix in (1, 65, 1000):
        L = rng.standard_normal((n_pix, M, M)) * 10.0 ** rng.uniform(-3, 3, (n_pix, 1, 1))
        cov = cr.pack(L @ np.swapaxes(L, 1, 2))
        u = rng.standard_normal(M) * np.array([1.0, -3.0, 40.0][:M])
        ar = Arena('cuda', None)
        err_before = hip.dexct_last_hip_error()
        ar.alloc('cov', cov.nbytes).put(cov)
        ar.alloc('out', 8 * n_pix)
        uh = np.ascontiguousarray(u)

        def launch():
            assert hip.dexct_cov_quadform(ar['cov'].ptr, n_pix, M, uh.ctypes.data, ar['out'].ptr, stream_ptr()) == 0

        got = twice(ar, launch, ['out'])['out'].view(F64)
        assert hip.dexct_last_hip_error() == err_before
        ref, mag = quadform_numpy(cov, u)
        ulps = np.abs(got - ref) / np.spacing(mag)
        print(f'M={M} n_pix={n_pix}: {ulps.max():.2f} ulp of sum |u_i C_ij u_j|')
        assert np.all(ulps <= 4.0)
        assert got.shape == (n_pix,) and cov.shape == (n_pix, T)


@pytest.mark.parametrize('K,M', [(2, 2), (4, 3)])
def test_end_to_end_sample_covariance(hip, K, M):
    """20 000 pixels with one mean and one variance (the energy-integrating synthetic detector at flux 100, a = (10, 1, 0.02)),
    sampled by dexct_add_noise, decomposed by dexct_gn_decompose_multi: the sample covariance of the estimates against
    dexct_gn_covariance at the true state, within 5 sigma of its sampling error sqrt((C_ii C_jj + C_ij^2) / (N - 1))."""
    from dex_ct_sim_amd import matdecomp as md
    from dex_ct_sim_amd._device import stream_ptr
    n_views, n_channels = 200, 100
    N = n_views * n_channels
    i0, i0v, mus = cr.tables(K, M, 60, eid=True, flux=100.0)
    a = np.array([10.0, 1.0, 0.02][:M])
    nu, v, _ = cr.sums(a[None], i0, i0v, mus)
    counts = torch.from_numpy(np.repeat(nu[0].astype(np.float32)[:, None], N, axis=1)).to('cuda').contiguous()
    var = torch.from_numpy(np.repeat(v[0].astype(np.float32)[:, None], N, axis=1)).to('cuda').contiguous()
    assert hip.dexct_add_noise(counts.data_ptr(), var.data_ptr(), K, n_views, 1, n_channels, 0, 0, 20261019, stream_ptr()) == 0
    est = md.gn_device_multi(counts, i0, mus, 30).cpu().numpy()
    assert est.shape == (N, M) and np.all(np.isfinite(est))
    S = np.cov(est.T)
    C = np.zeros((M, M))
    packed = dev_cov(a[None], i0, i0v, mus, 'estimator')[0]
    for t, (i, j) in enumerate(cr.tri_index(M)):
        C[i, j] = C[j, i] = packed[t]
    sigma = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / (N - 1))
    z = np.abs(S - C) / sigma
    print(f'K={K} M={M}: sample covariance within {z.max():.2f} sigma of the prediction; '
          f'sd of the estimates {np.sqrt(np.diag(S))}, predicted {np.sqrt(np.diag(C))}')
    assert z.max() <= 5.0


def test_public_function(hip, c_bound):
    """The bundled 140 / 80 kV pair at a dose on a 3 x 40 sinogram: NumPy in and device tensors in, the mask, the restatement on
    decomposition_tables_multi(..., with_variance=True) within the bound of the sweep; vmi_variance and vmi_noise_sweep."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md, plots, xcompy
    ct = dx.FanBeamGeometry(N_channels=40, N_proj=3, eid=True, detector_file=os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'))
    specs = [dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV') for kv in (140, 80)]
    for sp, dose in zip(specs, (3.0, 7.0)):
        sp.rescale_counts(ct.A_iso * dose / 1200)
    ee, i0, mus, i0v = md.decomposition_tables_multi(ct, specs, with_variance=True)
    rng = np.random.default_rng(6)
    a = rng.uniform(0.0, 1.0, (3, 40, 2)) * np.array([30.0, 5.0])
    a[:, :4] = 0.0                                                            # air at one edge of the detector
    raw0 = cr.sums(a.reshape(-1, 2), i0, i0v, mus)[0][:, 0].reshape(3, 40).astype(np.float32)
    air = raw0 >= 0.95 * raw0.max()
    assert air[:, :4].all() and not air[:, 4:].any()
    basis = (a[..., 0], a[..., 1])
    for kind in cr.KINDS:
        cov = md.get_basismat_covariance(ct, basis, specs, kind=kind, mask_from=raw0)
        assert isinstance(cov, np.ndarray) and cov.shape == (3, 40, 3) and cov.dtype == F64
        assert not cov[air].any()
        ld = cr.covariance_full(a[~air], i0, i0v, mus, kind, LD)
        r = cr.error_ratio(cov[~air], ld)
        print(f'{kind}: ratio {r:.2f} (allowed {c_bound:.2f}); cond of the correlation up to {cr.corr_cond(ld).max():.0f}')
        assert r <= c_bound
        unmasked = md.get_basismat_covariance(ct, basis, specs, kind=kind)
        assert np.array_equal(bits(unmasked[~air]), bits(cov[~air])) and np.all(np.isfinite(unmasked))
        dev = md.get_basismat_covariance(ct, tuple(torch.from_numpy(b.copy()).to('cuda') for b in basis), specs, kind=kind,
                                         mask_from=torch.from_numpy(raw0).to('cuda'))
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(cov))
    cov = md.get_basismat_covariance(ct, basis, specs, mask_from=raw0)
    u = np.array([xcompy.mixatten(md.matcomp1, np.array([70.0]))[0], xcompy.mixatten(md.matcomp2, np.array([70.0]))[0]])
    var70 = plots.vmi_variance(cov, 70.0)
    ref70, mag = quadform_numpy(cov.reshape(-1, 3), u)
    assert isinstance(var70, np.ndarray) and var70.shape == (3, 40)
    assert np.all(np.abs(var70.reshape(-1) - ref70) <= 4.0 * np.spacing(mag))
    var70_d = plots.vmi_variance(torch.from_numpy(cov).to('cuda'), 70.0)
    assert isinstance(var70_d, torch.Tensor) and var70_d.is_cuda and np.array_equal(bits(var70_d.cpu().numpy()), bits(var70))
    Evals = np.arange(40.0, 141.0, 5.0)
    var, e_min = plots.vmi_noise_sweep(Evals, cov, mask=~air)
    ld = cr.covariance_full(a[~air], i0, i0v, mus, 'estimator', LD).astype(F64)
    uu = np.stack([xcompy.mixatten(md.matcomp1, Evals), xcompy.mixatten(md.matcomp2, Evals)])
    ref = np.einsum('me,pmn,ne->e', uu, ld, uu) / ld.shape[0]
    print(f'least VMI noise at {e_min} keV; NumPy arg-min {Evals[np.argmin(ref)]} keV')
    assert e_min == Evals[np.argmin(ref)] and Evals[0] < e_min < Evals[-1]
    assert np.allclose(var, ref, rtol=1e-9, atol=0.0)
    var_d, e_min_d = plots.vmi_noise_sweep(Evals, torch.from_numpy(cov).to('cuda'), mask=~air)
    assert e_min_d == e_min and np.allclose(var_d, var, rtol=1e-12, atol=0.0)
