"""The Python layer of the reconstruction calls (dex-ct-sim_amd/back_project.py) on the device: what its entry points must agree on
bit for bit - the FBP paths are gathers and deterministic - and the refusals that can only come after the upload.

The shapes are the smallest that take both lifts (a sinogram and a stack), both back-projectors (fan, Feldkamp) and Parker's
weights: a fan scanner of 24 views by 32 channels into 16 x 16 pixels over 20 cm, stacks of 1 and 3 rows, the same scanner as a
cone of 4 rows onto explicit slices, and as a short scan of 4.4 rad (pi + fan angle = 3.94 rad)."""
import warnings

import numpy as np
import pytest

from test_bhc import scanner, spectrum

pytestmark = pytest.mark.gpu

N, FOV, RAMP = 16, 20.0, 0.9
SLICES = (3, -0.6, 0.5)
SCANNERS = {'fan': {}, 'short': dict(theta_tot=4.4), 'cone': dict(N_rows=4, cone=True)}


def geometry(name):
    return scanner(N_channels=32, N_proj=24, **SCANNERS[name])


def sinogram(rows, seed=0):
    """[24, 32] for ``rows=None``, else the stack [24, rows, 32]"""
    shape = (24, 32) if rows is None else (24, rows, 32)
    return np.random.default_rng(seed).uniform(0.0, 4.0, shape).astype(np.float32)


def dev(a, dtype=None):
    import torch
    return torch.tensor(a, dtype=dtype, device='cuda')


def same(a, b):
    a, b = (t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name,rows', [('fan', None), ('fan', 1), ('fan', 3), ('short', None), ('short', 3), ('cone', 4)])
def test_get_recon_is_recon_device_of_the_uploaded_sinogram(hip, name, rows):
    from dex_ct_sim_amd import back_project as bp
    ct, spec, s = geometry(name), spectrum('80kV'), sinogram(rows)
    slices = SLICES if name == 'cone' else None
    raw, hu = bp.get_recon(s, ct, spec, N, FOV, RAMP, slices=slices)
    img = bp.recon_device(dev(s), ct, N, FOV, RAMP, slices=slices)
    assert raw.shape == ((N, N) if rows is None else (SLICES[0] if name == 'cone' else rows, N, N)) and raw.dtype == np.float32
    assert same(raw, img) and np.any(raw != 0.0)
    mu_w = bp.water_mu(ct, spec)
    assert same(hu, (1000.0 * (raw - mu_w) / mu_w).astype(np.float32))
    if name != 'cone' and rows is not None:             # a stack is its rows, one by one: as sinograms and as stacks of one
        for r in range(rows):
            assert same(raw[r], bp.recon_device(dev(s[:, r]), ct, N, FOV, RAMP))
            assert same(raw[r:r + 1], bp.recon_device(dev(s[:, r:r + 1]), ct, N, FOV, RAMP))


@pytest.mark.parametrize('name,rows', [('fan', None), ('fan', 3), ('short', 3), ('cone', 4)])
def test_beam_hardening_is_the_same_correction_wherever_it_is_applied(hip, name, rows):
    from dex_ct_sim_amd import back_project as bp, bhc
    ct, spec, s = geometry(name), spectrum('80kV'), sinogram(rows, 1)
    slices = SLICES if name == 'cone' else None
    table = bhc.linearization_table(ct, spec, 'water')
    s_d = dev(s)
    by_table = bp.get_recon(s, ct, spec, N, FOV, RAMP, slices=slices, bhc=table)[0]
    assert same(by_table, bp.get_recon(s, ct, spec, N, FOV, RAMP, slices=slices, bhc='water')[0])
    assert same(by_table, bp.recon_device(s_d, ct, N, FOV, RAMP, slices=slices, bhc=table))
    assert same(s_d, s)                                  # recon_device left its input alone
    assert same(by_table, bp.recon_device(bhc.linearize_device(s_d, table), ct, N, FOV, RAMP, slices=slices))
    assert not same(by_table, bp.get_recon(s, ct, spec, N, FOV, RAMP, slices=slices)[0])


def one_warning(record, text):
    assert [(w.category, str(w.message)) for w in record] == [(RuntimeWarning, text)]


@pytest.mark.parametrize('name,rows', [('fan', None), ('short', 3), ('cone', 4)])
def test_non_finite_sinogram_values_count_as_zeros(hip, name, rows):
    from dex_ct_sim_amd import back_project as bp
    ct, spec, s = geometry(name), spectrum('80kV'), sinogram(rows, 2)
    slices = SLICES if name == 'cone' else None
    bad, zeroed = s.copy(), s.copy()
    bad.reshape(-1)[[37, 500]] = np.nan, -np.inf
    zeroed.reshape(-1)[[37, 500]] = 0.0
    for kw in ({}, dict(bhc='water')):
        with warnings.catch_warnings(record=True) as record:
            warnings.simplefilter('always')
            got = bp.get_recon(bad, ct, spec, N, FOV, RAMP, slices=slices, **kw)
        one_warning(record, 'get_recon: 2 non-finite sinogram value(s) set to 0 before filtering')
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            want = bp.get_recon(zeroed, ct, spec, N, FOV, RAMP, slices=slices, **kw)
        assert same(got[0], want[0]) and same(got[1], want[1]) and np.all(np.isfinite(got[0]))


@pytest.mark.parametrize('name,shape', [('fan', (24, 32, 3)), ('short', (24, 3, 32, 1)), ('cone', (24, 4, 32, 2))])
def test_covariance_entry_points_agree(hip, name, shape):
    import torch
    from dex_ct_sim_amd import back_project as bp
    ct = geometry(name)
    slices = SLICES if name == 'cone' else None
    cov = np.random.default_rng(3).uniform(-1.0, 2.0, shape)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = bp.get_recon_covariance(cov, ct, N, FOV, RAMP, slices=slices)
        out_d = bp.get_recon_covariance(dev(cov), ct, N, FOV, RAMP, slices=slices)
        direct = bp.recon_covariance_device(dev(cov), ct, N, FOV, RAMP, slices=slices)
    lead = () if len(shape) == 3 else (SLICES[0] if name == 'cone' else shape[1],)
    assert isinstance(out, np.ndarray) and out.shape == lead + (N, N, shape[-1]) and out.dtype == np.float64
    assert isinstance(out_d, torch.Tensor) and out_d.is_cuda and same(out, out_d) and same(out, direct) and np.any(out != 0.0)
    if name == 'short':                                   # a stack is its rows
        for r in range(shape[1]):
            assert same(out[r], bp.recon_covariance_device(dev(cov[:, r]), ct, N, FOV, RAMP))
    bad, zeroed = cov.copy(), cov.copy()
    bad.reshape(-1)[[41, 900]] = np.inf, np.nan
    zeroed.reshape(-1)[[41, 900]] = 0.0
    for up in (np.asarray, dev):
        with warnings.catch_warnings(record=True) as record:
            warnings.simplefilter('always')
            got = bp.get_recon_covariance(up(bad), ct, N, FOV, RAMP, slices=slices)
        one_warning(record, 'get_recon_covariance: 2 non-finite covariance value(s) set to 0 before filtering')
        assert same(got, bp.get_recon_covariance(zeroed, ct, N, FOV, RAMP, slices=slices))


def test_refusals_that_follow_the_upload(hip):
    from dex_ct_sim_amd import back_project as bp
    fan, cone, spec = geometry('fan'), geometry('cone'), spectrum('80kV')

    def refused(message, sino, ct=fan, exc=ValueError, **kw):
        with pytest.raises(exc) as info:
            bp.get_recon(sino, ct, spec, N, FOV, RAMP, **kw)
        assert type(info.value) is exc and str(info.value) == message

    for method in ('fbp', 'sirt', 'os-sart'):
        refused('sinogram (23, 32) does not match the scanner (24 x 32)', np.zeros((23, 32), np.float32), method=method)
        refused('sinogram (24, 2, 31) does not match the scanner (24 x 32)', np.zeros((24, 2, 31), np.float32), method=method)
    refused('sinogram has 3 rows, the scanner 4', sinogram(3), ct=cone)
    refused('sinogram has 3 rows, the scanner 4', sinogram(3), ct=cone, bhc='water')
    refused("unknown filter window 'boxcar'; choose from ['cosine', 'hamming', 'hann', 'rect', 'sinc']", sinogram(None), window='boxcar')
    for value in (-1.0, np.nan, np.inf):
        w = np.ones((24, 32), np.float32)
        w[5, 7] = value
        refused('weights must be finite and >= 0', sinogram(None), method='pwls', weights=w)
    with pytest.raises(ValueError) as info:              # recon_device states the same rule for a device tensor
        bp.recon_device(dev(np.zeros((24, 33), np.float32)), fan, N, FOV, RAMP, method='sirt')
    assert str(info.value) == 'sinogram (24, 33) does not match the scanner (24 x 32)'


def test_pwls_gives_a_non_finite_value_no_weight(hip):
    """What tests/test_gpu_pwls.py asserts of it, on this module's shapes: the warning, and an image that is finite."""
    from dex_ct_sim_amd import back_project as bp
    ct, spec = geometry('fan'), spectrum('80kV')
    bad = sinogram(None, 4)
    bad[5, 7] = np.nan
    with pytest.warns(RuntimeWarning, match='non-finite'):
        raw, _ = bp.get_recon(bad, ct, spec, N, FOV, RAMP, method='pwls', weights=np.ones((24, 32), np.float32), n_iters=2)
    assert np.all(np.isfinite(raw))
