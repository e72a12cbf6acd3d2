"""The references of the FBP noise propagation against each other and against sample statistics, and the host checks of
back_project.get_recon_covariance (no GPU)."""
import numpy as np
import pytest

import recon_noise_refs as rn
from oracle import fbp_oracle as fo

# (views, channels, fan angle, SID, N_matrix, FOV, ramp, window, theta_tot)
FAN_CASES = {
    'plain': (12, 16, 0.8230337, 60.0, 9, 30.0, 1.0, 'rect', None),
    'hann-partly-outside': (10, 17, 0.5, 60.0, 8, 60.0, 0.7, 'hann', None),
    'short-scan': (14, 16, 0.6, 60.0, 9, 20.0, 1.0, 'rect', np.pi + 0.6 + 0.4),
    'unseen-corners': (12, 16, 0.1, 60.0, 9, 60.0, 1.0, 'rect', None),
}


def planes(shape, seed):
    """a positive plane and one of mixed sign (a cross-covariance), last axis"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.5, 4.0, shape), rng.uniform(-2.0, 2.0, shape)], axis=-1)


def seen_by_some_view(thetas, gammas, sid, n_matrix, fov):
    return np.any([ok for _, _, ok, _ in rn._views(thetas, gammas, sid, n_matrix, fov, len(gammas))], axis=0)


@pytest.mark.parametrize('name', sorted(FAN_CASES))
def test_closed_form_is_the_squared_operator(name):
    """(A o A) s from unit impulses through the oracle's get_recon against the closed form: both float64, 1e-12 of the plane's
    largest magnitude asked, 2 - 5e-16 measured."""
    n_views, n_ch, gamma_fan, sid, N, fov, ramp, window, theta_tot = FAN_CASES[name]
    thetas, gammas = rn.fan(n_views, n_ch, gamma_fan, theta_tot or 2 * np.pi)
    s = planes((n_views, n_ch), n_views)
    M = rn.operator_matrix(thetas, gammas, sid, N, fov, ramp, window, theta_tot)
    ref = rn.squared_operator(M, s).reshape(N, N, 2)
    got = rn.variance_recon(s, thetas, gammas, sid, N, fov, ramp, window, theta_tot)
    for t in range(2):
        err = np.max(np.abs(got[..., t] - ref[..., t])) / np.max(np.abs(ref[..., t]))
        print(f'{name} plane {t}: {err:.1e}')
        assert err <= 1e-12
    assert np.all(got[..., 0] >= 0.0)
    seen = seen_by_some_view(thetas, gammas, sid, N, fov)
    n_views_seen = np.sum([ok for _, _, ok, _ in rn._views(thetas, gammas, sid, N, fov, n_ch)], axis=0)
    if name == 'plain':
        assert np.all(n_views_seen == n_views)
    if name == 'hann-partly-outside':
        assert np.any((n_views_seen > 0) & (n_views_seen < n_views))
    if name == 'unseen-corners':
        assert not seen[0, 0] and not seen[-1, -1] and not seen[0, -1] and not seen[-1, 0] and seen[N // 2, N // 2]
    assert np.all(got[~seen] == 0.0) and np.all(ref[~seen] == 0.0)
    if theta_tot is not None:                                     # the Parker weights matter: without them the result differs
        full = rn.variance_recon(s, thetas, gammas, sid, N, fov, ramp, window, None)
        assert np.max(np.abs(full - got)) > 0.05 * np.max(np.abs(got))


def test_neighbour_covariance_cannot_be_dropped():
    """the correlation of neighbouring filtered samples of the plain ramp is -0.61 for a flat line"""
    thetas, gammas = rn.fan(1, 64, 0.8)
    A, B = rn.filter_variance(np.ones((1, 64, 1)) / (60.0 * np.cos(gammas))[None, :, None] ** 2, thetas, gammas, 60.0)
    rho = B[0, 31, 0] / np.sqrt(A[0, 31, 0] * A[0, 32, 0])
    assert -0.63 < rho < -0.59, rho
    assert B[0, -1, 0] == 0.0


def test_fdk_closed_form_is_the_squared_operator():
    """3 rows, 2 slices; the second slice reads outside the rows for the views far from its pixels"""
    n_views, n_ch, N, fov, sid, sdd = 10, 12, 7, 24.0, 60.0, 100.0
    thetas, gammas = rn.fan(n_views, n_ch, 0.6)
    row_z = (np.arange(3) - 1.0) * 1.0
    slices_z = np.array([0.1, 0.52])
    fdk = dict(sdd=sdd, row_z=row_z, src_z=0.05, slices_z=slices_z)
    s = planes((n_views, 3, n_ch), 5)
    M = rn.operator_matrix(thetas, gammas, sid, N, fov, 0.9, 'rect', fdk=fdk)
    ref = rn.squared_operator(M, s).reshape(2, N, N, 2)
    got = rn.variance_fdk(s, thetas, gammas, sid, sdd, row_z, 0.05, N, fov, 0.9, slices_z)
    for t in range(2):
        err = np.max(np.abs(got[..., t] - ref[..., t])) / np.max(np.abs(ref[..., t]))
        print(f'fdk plane {t}: {err:.1e}')
        assert err <= 1e-12
    # the case is what it claims: slice 1 leaves the rows for some (pixel, view) pairs and not for others, slice 0 for none
    inside = rn.fdk_inside(thetas, gammas, sid, sdd, row_z, 0.05, N, fov, slices_z)
    assert inside[0].all() and inside[1].any() and not inside[1].all()


def test_prediction_matches_the_sample_variance_of_the_oracle():
    """512 Gaussian realisations through fbp_oracle: the per-pixel sample variance over the prediction is chi^2_511 / 511.
    Measured with the oracle: mean 0.9977, range 0.815 .. 1.217, sd 0.0611; 3 s."""
    p = rn.STAT
    thetas, gammas = rn.fan(p['n_views'], p['n_channels'], p['gamma_fan'])
    s, noise = rn.stat_problem()
    assert s.min() >= 0.5e-4 and s.max() <= 4e-4
    predicted = rn.variance_recon(s, thetas, gammas, p['sid'], p['n_matrix'], p['fov'])
    q = fo.filter_sino(noise, gammas, p['sid'])
    images = np.stack([fo.back_project(q[r], thetas, gammas, p['sid'], p['n_matrix'], p['fov']) for r in range(len(q))])
    rn.stat_check(images, predicted)


def test_host_argument_checks_need_no_device():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import back_project as bp
    assert dx.get_recon_covariance is bp.get_recon_covariance and 'get_recon_covariance' in dx.__all__
    ct = dx.FanBeamGeometry(N_channels=16, N_proj=12)
    with pytest.raises(ValueError, match=r'var\[\.\.\., None\]'):
        bp.get_recon_covariance(np.ones((12, 16)), ct, 8, 30.0, 1.0)
    for shape in ((12, 15, 3), (11, 16, 3), (12, 2, 15, 3), (12, 16, 3, 1, 1)):
        with pytest.raises(ValueError):
            bp.get_recon_covariance(np.ones(shape), ct, 8, 30.0, 1.0)
    with pytest.raises(ValueError, match='window'):
        bp.get_recon_covariance(np.ones((12, 16, 3)), ct, 8, 30.0, 1.0, window='boxcar')
    short = dx.FanBeamGeometry(N_channels=16, N_proj=12, theta_tot=np.pi)
    with pytest.raises(ValueError, match='short scan'):
        bp.get_recon_covariance(np.ones((12, 16, 1)), short, 8, 30.0, 1.0)
    cone = dx.FanBeamGeometry(N_channels=16, N_proj=12, N_rows=4, cone=True)
    with pytest.raises(ValueError, match='rows'):
        bp.get_recon_covariance(np.ones((12, 3, 16, 1)), cone, 8, 30.0, 1.0)


def test_library_exports_and_declares_the_entry_points():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from dex_ct_sim_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    for name in ('dexct_fbp_var_filter', 'dexct_fbp_var_backproject', 'dexct_fdk_var_backproject'):
        assert hasattr(lib, name) and name in _native.SYMBOLS and re.search(name + r'\s*\(', hdr), name
    assert re.search(rf'#define DEXCT_FBP_VAR_MAX_CHANNELS {_native.FBP_VAR_MAX_CHANNELS}\b', hdr)
    assert _native.FBP_VAR_MAX_CHANNELS >= 2048 and 24 * _native.FBP_VAR_MAX_CHANNELS - 8 <= 64 * 1024
