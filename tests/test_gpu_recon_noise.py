"""Noise propagation through the FBP on the GPU (csrc/fbp_var.hip; back_project.recon_covariance_device, get_recon_covariance,
plots.vmi_noise_map, main.py --noise-maps) against the NumPy references of tests/recon_noise_refs.py, against the shipped FBP
itself and against sample statistics.

Kernel -> test:
  fbp_var_filter_kernel               every test; short scans: 'short' and the guarded shard with view_offset > 0; 2048 and
                                      2730 channels (the LDS limit): test_guarded_filter_at_the_channel_limit
  fbp_var_backproject_kernel<T, 1>    single rows, T = 1, 3, 6 and the 6 / 3 / 1 split of T = 2, 5
  fbp_var_backproject_kernel<T, R>    rows 3 (a partial group) and 11 (full groups and a partial one), T = 1, 3, 6
  fdk_var_backproject_kernel<T, R>    test_fdk_against_reference (5 rows -> 4 slices, T = 1, 3, 6), guarded
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import recon_noise_refs as rn
from conftest import INPUT, ROOT
from guarded import Arena, twice

pytestmark = pytest.mark.gpu

FAN = 0.8230337
F64 = np.float64


def scanner(n_views, n_ch, gamma_fan=FAN, theta_tot=2 * np.pi, **kw):
    import dex_ct_sim_amd as dx
    return dx.FanBeamGeometry(N_channels=n_ch, N_proj=n_views, gamma_fan=gamma_fan, SID=60.0, SDD=100.0, theta_tot=theta_tot, **kw)


def cov_planes(shape, T, seed):
    """T planes: the even ones positive (variances), the odd ones of mixed sign (cross-covariances)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 4.0, shape + (T,))
    c[..., 1::2] = rng.uniform(-2.0, 2.0, shape + (T,))[..., 1::2]
    return c


def run(cov, ct, N, fov, ramp=1.0, window=None, slices=None):
    import torch
    from dex_ct_sim_amd import back_project as bp
    return bp.recon_covariance_device(torch.from_numpy(np.ascontiguousarray(cov)).to('cuda'), ct, N, fov, ramp, window, slices).cpu().numpy()


def worst(got, ref):
    """per plane: the largest difference over the plane's largest magnitude"""
    ax = tuple(range(got.ndim - 1))
    return np.max(np.max(np.abs(got - ref), axis=ax) / np.max(np.abs(ref), axis=ax))


# id: (views, channels, fan angle, N_matrix, FOV, T, rows, ramp, window, theta_tot)
CASES = {
    'c257-N70': (20, 257, FAN, 70, 30.0, 3, 1, 1.0, 'rect', None),          # more than one block stride, odd; ragged against 64 x 4
    'c2': (8, 2, 0.5, 9, 10.0, 1, 1, 1.0, 'rect', None),                    # the minimum
    'v90-T6': (90, 33, FAN, 9, 30.0, 6, 1, 1.0, 'rect', None),
    'T2': (9, 20, FAN, 12, 30.0, 2, 1, 1.0, 'rect', None),                  # 1 + 1
    'T5-rows3': (9, 20, FAN, 12, 30.0, 5, 3, 1.0, 'rect', None),            # 3 + 1 + 1
    'rows3-T3': (16, 40, FAN, 33, 30.0, 3, 3, 1.0, 'rect', None),           # a partial group
    'rows11-T1': (12, 24, FAN, 20, 30.0, 1, 11, 1.0, 'rect', None),         # a full group of 8 and a partial one
    'rows11-T3': (12, 24, FAN, 20, 30.0, 3, 11, 1.0, 'rect', None),
    'rows11-T6': (12, 24, FAN, 20, 30.0, 6, 11, 1.0, 'rect', None),         # two full groups of 4 and a partial one
    'hann': (16, 33, FAN, 17, 30.0, 3, 1, 0.7, 'hann', None),
    'short': (30, 40, 0.6, 21, 20.0, 3, 3, 1.0, 'rect', np.pi + 0.6 + 0.3),
    'unseen-corners': (12, 16, 0.1, 9, 60.0, 3, 1, 1.0, 'rect', None),
}


@pytest.mark.parametrize('name', list(CASES))
def test_kernels_against_reference(hip, name):
    """Both sides float64, differing by summation order (about 2 N_channels + N_proj roundings, < 1e-13 here) times a
    cancellation of at most ~5 from B, and by the last bit of atan2 in the channel position: 1e-10 of each plane's largest
    magnitude.  Measured on the MI355X: 1.3e-12 at 257 channels (the position's own resolution: pos up to 257 has an ulp of 6e-14,
    and dV/dw is about 3 V), 4e-16 ... 3e-14 for the other shapes."""
    n_views, n_ch, gamma_fan, N, fov, T, rows, ramp, window, theta_tot = CASES[name]
    ct = scanner(n_views, n_ch, gamma_fan, theta_tot or 2 * np.pi)
    cov = cov_planes((n_views, rows, n_ch), T, n_views + n_ch)
    got = run(cov, ct, N, fov, ramp, window)
    ref = rn.variance_stack(cov, ct.thetas, ct.gammas, ct.SID, N, fov, ramp, window, theta_tot)
    assert got.shape == ref.shape == (rows, N, N, T) and got.dtype == F64
    print(f'{name}: worst error {worst(got, ref):.2e} of the plane maximum')
    assert worst(got, ref) <= 1e-10
    if rows == 1:                                                          # the 3-D form of the same call
        assert np.array_equal(run(cov[:, 0], ct, N, fov, ramp, window), got[0])
    if name == 'unseen-corners':
        for iy, ix in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert np.all(ref[:, iy, ix] == 0.0) and np.all(got[:, iy, ix] == 0.0)
        assert np.all(got[0, N // 2, N // 2, 0::2] > 0.0)
    if theta_tot is not None:
        full = rn.variance_stack(cov, ct.thetas, ct.gammas, ct.SID, N, fov, ramp, window, None)
        assert worst(got, full) > 0.05                                     # Parker's weights are in


@pytest.mark.parametrize('T', [1, 3, 6])
def test_fdk_against_reference(hip, T):
    """5 detector rows -> 4 slices, the outer ones reading outside the rows for the views that see them from close by"""
    ct = scanner(14, 24, 0.6, N_rows=5, cone=True, h_iso=0.5, src_z=0.1)
    N, fov, slices = 13, 20.0, (4, -1.0, 0.7)
    cov = cov_planes((14, 5, 24), T, 40 + T)
    got = run(cov, ct, N, fov, 0.9, None, slices)
    zs = slices[1] + slices[2] * np.arange(4)
    ref = rn.variance_fdk(cov, ct.thetas, ct.gammas, ct.SID, ct.SDD, ct.row_z(), ct.src_z, N, fov, 0.9, zs)
    assert got.shape == ref.shape == (4, N, N, T)
    print(f'fdk T={T}: worst error {worst(got, ref):.2e}')
    assert worst(got, ref) <= 1e-10
    inside = rn.fdk_inside(ct.thetas, ct.gammas, ct.SID, ct.SDD, ct.row_z(), ct.src_z, N, fov, zs)
    assert inside[0].any() and not inside[0].all() and inside[1].all()                        # the outer slice loses views
    assert np.all(got[..., 0] >= 0.0)


def test_against_the_shipped_fbp(hip):
    """The float32 FBP matrix from 192 unit impulses, the rows of ONE stacked-fan recon_device call; (M o M) s in float64 on the
    host against the new path.  1e-4 of the plane maximum: 5 x the project's 2e-5 bound of the float32 FBP against float64
    (squaring doubles a relative error, the rest is margin); about 1e-6 expected."""
    import torch
    from dex_ct_sim_amd import back_project as bp
    n_views, n_ch, N, fov = 12, 16, 16, 30.0
    ct = scanner(n_views, n_ch)
    imp = np.zeros((n_views, n_views * n_ch, n_ch), np.float32)
    j = np.arange(n_views * n_ch)
    imp[j // n_ch, j, j % n_ch] = 1.0
    img = bp.recon_device(torch.from_numpy(imp).to('cuda'), ct, N, fov, 1.0, 'rect').cpu().numpy().astype(F64)
    M = img.reshape(n_views * n_ch, N * N).T
    s = cov_planes((n_views, n_ch), 2, 3)
    ref = rn.squared_operator(M, s).reshape(N, N, 2)
    got = run(s, ct, N, fov, 1.0, 'rect')
    print(f'against the shipped FBP: {worst(got, ref):.2e} of the plane maximum')
    assert worst(got, ref) <= 1e-4


def test_structure(hip):
    n_views, n_ch, N, fov, rows = 14, 31, 19, 30.0, 11
    ct = scanner(n_views, n_ch)
    cov = cov_planes((n_views, rows, n_ch), 3, 8)
    full = run(cov, ct, N, fov)
    for t in range(3):                                       # a plane does not depend on the planes beside it
        assert np.array_equal(run(cov[..., t:t + 1], ct, N, fov)[..., 0], full[..., t]), t
    for r in range(rows):                                    # nor a row on the rows beside it
        assert np.array_equal(run(cov[:, r], ct, N, fov), full[r]), r
    six = np.concatenate([cov, 2.0 * cov], axis=-1)          # nor on the group sizes of the 6-plane launch
    assert np.array_equal(run(six, ct, N, fov)[..., :3], full)
    other = cov_planes((n_views, rows, n_ch), 3, 9)
    a, b = 0.7, -1.9
    mix = run(a * cov + b * other, ct, N, fov)
    lin = a * full + b * run(other, ct, N, fov)
    assert worst(mix, lin) <= 1e-12


def test_psd_and_noise_map(hip):
    """A pixel-wise PSD sinogram covariance (rho in [-0.99, -0.9]) gives a PSD image covariance: c00 c11 - c01^2 >= (1 - 0.99^2)
    c00 c11 exactly, far above rounding.  vmi_noise_map is sqrt(u^T C u) 1000 / u_water."""
    import torch
    from dex_ct_sim_amd import plots, xcompy
    n_views, n_ch, N, fov = 24, 48, 32, 30.0
    ct = scanner(n_views, n_ch)
    rng = np.random.default_rng(11)
    c00, c11 = rng.uniform(0.5, 4.0, (2, n_views, n_ch))
    rho = rng.uniform(-0.99, -0.9, (n_views, n_ch))
    cov = np.stack([c00, rho * np.sqrt(c00 * c11), c11], axis=-1)
    img = run(cov, ct, N, fov)
    i00, i01, i11 = img[..., 0], img[..., 1], img[..., 2]
    assert np.all(i00 > 0.0) and np.all(i11 > 0.0)
    assert np.all(i00 * i11 - i01 * i01 >= 0.019 * i00 * i11)
    for E, hu in ((70.0, True), (50.0, False)):
        u, _ = plots._basis_vector(E, None)
        u0, u1 = u[:, 0]
        uw = float(xcompy.mixatten(plots.WATER, np.array([E]))[0])
        ref = np.sqrt(u0 * u0 * i00 + 2.0 * u0 * u1 * i01 + u1 * u1 * i11) * (1000.0 / uw if hu else 1.0)
        got = plots.vmi_noise_map(img, E, HU=hu)
        assert got.shape == (N, N) and np.all(np.isfinite(got)) and np.all(got >= 0.0)
        assert np.max(np.abs(got - ref) / ref) <= 1e-12
        dev = plots.vmi_noise_map(torch.from_numpy(img).to('cuda'), E, HU=hu)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


def test_prediction_matches_the_sample_variance_of_the_shipped_fbp(hip):
    """tests/test_recon_noise_refs.py's statistical case through the real recon_device: the 512 realisations are the 512 rows of
    one stacked-fan call; same bounds."""
    import torch
    from dex_ct_sim_amd import back_project as bp
    p = rn.STAT
    ct = scanner(p['n_views'], p['n_channels'], p['gamma_fan'])
    s, noise = rn.stat_problem()
    stack = np.ascontiguousarray(noise.transpose(1, 0, 2), dtype=np.float32)
    images = bp.recon_device(torch.from_numpy(stack).to('cuda'), ct, p['n_matrix'], p['fov'], 1.0, 'rect').cpu().numpy()
    predicted = run(s[..., None], ct, p['n_matrix'], p['fov'], 1.0, 'rect')[..., 0]
    rn.stat_check(images, predicted)


def test_public_entry_point(hip):
    """NumPy in -> NumPy out, tensor in -> tensor out; non-finite entries become 0 with a warning instead of smearing"""
    import torch
    import dex_ct_sim_amd as dx
    ct = scanner(12, 16)
    cov = cov_planes((12, 16), 3, 2)
    ref = run(cov, ct, 9, 30.0)
    got = dx.get_recon_covariance(cov, ct, 9, 30.0, 1.0)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    dev = dx.get_recon_covariance(torch.from_numpy(cov).to('cuda'), ct, 9, 30.0, 1.0)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), ref)
    hurt, zeroed = cov.copy(), cov.copy()
    hurt[3, 4, 0], hurt[5, 6, 1] = np.nan, np.inf
    zeroed[3, 4, 0] = zeroed[5, 6, 1] = 0.0
    with pytest.warns(RuntimeWarning, match='2 non-finite'):
        got = dx.get_recon_covariance(hurt, ct, 9, 30.0, 1.0)
    assert np.array_equal(got, run(zeroed, ct, 9, 30.0))


# ---- guard bands through the bare C ABI ------------------------------------------------------------------------------------------
def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


def ok(rc):
    assert rc == 0, rc


def arena(hip):
    """(the library's last HIP error is per thread and is never cleared: an earlier test of the session that provoked a refusal
    on purpose leaves it set.  Every call here is checked by its return code, and the tests compare the value with the one they
    started from instead of with 0, which Arena.check would do - as tests/test_gpu_iter.py does.)"""
    ar = Arena('cuda', None)
    ar.hip_error_before = hip.dexct_last_hip_error()
    return ar


def filter_inputs(n_ch, gamma_fan, ramp=1.0):
    from oracle import fbp_oracle as fo
    dg = gamma_fan / n_ch
    gammas = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * dg
    return fo.ramp_taps(n_ch, dg, ramp), 60.0 * np.cos(gammas), gammas, dg


@pytest.mark.parametrize('n_ch, rows, short', [(129, 3, False), (257, 11, True), (129, 3, True)])
def test_guarded_filter(hip, n_ch, rows, short):
    """A view shard (view_offset > 0) of a full and of a short scan, T = 3: guards intact, qa and qb - B's last channel included -
    bit-identical under both fills, values those of the whole scan's reference."""
    n_views, view_offset, n_total, T = 4, 5, 11, 3
    taps, weight, gammas, dg = filter_inputs(n_ch, 0.6)
    theta_tot = np.pi + 0.6 + 0.3 if short else 2 * np.pi
    thetas = np.arange(n_total) * (theta_tot / n_total)
    cov = cov_planes((n_views, rows, n_ch), T, n_ch + rows)
    ar = arena(hip)
    ar.alloc('cov', cov.nbytes).put(cov)
    ar.alloc('taps', 8 * (2 * n_ch - 1)).put(taps)
    ar.alloc('weight', 8 * n_ch).put(weight)
    ar.alloc('qa', cov.nbytes)
    ar.alloc('qb', cov.nbytes)
    out = twice(ar, lambda: ok(hip.dexct_fbp_var_filter(ar['cov'].ptr, n_views, rows, n_ch, T, ar['taps'].ptr, ar['weight'].ptr, dg,
                                                        theta_tot, view_offset, n_total, ar['qa'].ptr, ar['qb'].ptr, sp())), ['qa', 'qb'])
    qa, qb = (out[k].view(F64).reshape(cov.shape) for k in ('qa', 'qb'))
    whole = np.zeros((n_total, rows, n_ch, T))
    whole[view_offset:view_offset + n_views] = cov
    A, B = rn.filter_variance(whole, thetas, gammas, 60.0, theta_tot=theta_tot if short else None)
    A, B = A[view_offset:view_offset + n_views], B[view_offset:view_offset + n_views]
    assert np.max(np.abs(qa - A)) <= 1e-12 * np.max(np.abs(A)) and np.max(np.abs(qb - B)) <= 1e-12 * np.max(np.abs(A))
    assert np.all(qb[:, :, -1, :] == 0.0)
    assert hip.dexct_last_hip_error() == ar.hip_error_before


@pytest.mark.parametrize('n_ch', [2048, 2730])
def test_guarded_filter_at_the_channel_limit(hip, n_ch):
    """One line, one plane at 2048 channels (what the filter must take) and at DEXCT_FBP_VAR_MAX_CHANNELS: 49 KB and 65 512 B of
    dynamic LDS.  Values against the reference within 1e-10 of A's maximum (float64 on both sides, 2 n_ch roundings and the
    cancellation of B), guards intact, bit-identical under both fills.  Measured on the MI355X: 9.0e-15 / 5.4e-15 (A / B) at 2048
    channels, 1.7e-13 / 1.0e-13 at 2730."""
    from dex_ct_sim_amd import _native
    assert n_ch <= _native.FBP_VAR_MAX_CHANNELS
    taps, weight, gammas, dg = filter_inputs(n_ch, FAN)
    cov = cov_planes((1, 1, n_ch), 1, n_ch)
    ar = arena(hip)
    ar.alloc('cov', cov.nbytes).put(cov)
    ar.alloc('taps', 8 * (2 * n_ch - 1)).put(taps)
    ar.alloc('weight', 8 * n_ch).put(weight)
    ar.alloc('qa', cov.nbytes)
    ar.alloc('qb', cov.nbytes)
    out = twice(ar, lambda: ok(hip.dexct_fbp_var_filter(ar['cov'].ptr, 1, 1, n_ch, 1, ar['taps'].ptr, ar['weight'].ptr, dg, 2 * np.pi, 0,
                                                        1, ar['qa'].ptr, ar['qb'].ptr, sp())), ['qa', 'qb'])
    qa, qb = (out[k].view(F64).reshape(cov.shape) for k in ('qa', 'qb'))
    A, B = rn.filter_variance(cov, np.zeros(1), gammas, 60.0)
    print(f'{n_ch} channels: A {np.max(np.abs(qa - A)) / np.max(np.abs(A)):.2e}, B {np.max(np.abs(qb - B)) / np.max(np.abs(A)):.2e} of max A')
    assert np.max(np.abs(qa - A)) <= 1e-10 * np.max(np.abs(A)) and np.max(np.abs(qb - B)) <= 1e-10 * np.max(np.abs(A))
    assert np.all(qa > 0.0) and qb[0, 0, -1, 0] == 0.0
    assert hip.dexct_last_hip_error() == ar.hip_error_before


def backproject_buffers(hip, n_views, n_ch, rows, T, out_rows, N, seed):
    rng = np.random.default_rng(seed)
    qa = rng.uniform(0.5, 4.0, (n_views, rows, n_ch, T))
    qb = rng.uniform(-2.0, 2.0, (n_views, rows, n_ch, T))
    th = np.arange(n_views) * (2 * np.pi / n_views)
    ar = arena(hip)
    ar.alloc('qa', qa.nbytes).put(qa)
    ar.alloc('qb', qb.nbytes).put(qb)
    ar.alloc('view_cs', 16 * n_views).put(np.stack([np.cos(th), np.sin(th)], axis=1))
    ar.alloc('image', 8 * out_rows * N * N * T)
    return ar


@pytest.mark.parametrize('n_ch, rows', [(129, 3), (257, 11)])
def test_guarded_backproject(hip, n_ch, rows):
    n_views, T, N, fov = 6, 3, 37, 30.0
    ar = backproject_buffers(hip, n_views, n_ch, rows, T, rows, N, n_ch)
    img = twice(ar, lambda: ok(hip.dexct_fbp_var_backproject(ar['qa'].ptr, ar['qb'].ptr, ar['view_cs'].ptr, n_views, n_ch, rows, T,
                                                             60.0, FAN / n_ch, 2 * np.pi / n_views, N, fov, ar['image'].ptr, sp())),
                ['image'])['image'].view(F64)
    assert np.all(np.isfinite(img)) and np.any(img != 0.0)
    assert hip.dexct_last_hip_error() == ar.hip_error_before


@pytest.mark.parametrize('n_ch, rows', [(129, 3), (257, 11)])
def test_guarded_fdk_backproject(hip, n_ch, rows):
    n_views, T, N, fov, n_slices = 6, 3, 21, 30.0, 5
    ar = backproject_buffers(hip, n_views, n_ch, rows, T, n_slices, N, n_ch + 1)
    row_z0 = -0.5 * (rows - 1) * 0.8
    ar.alloc('row_weight', 8 * rows).put(100.0 / np.sqrt(100.0 ** 2 + (row_z0 + 0.8 * np.arange(rows)) ** 2))
    img = twice(ar, lambda: ok(hip.dexct_fdk_var_backproject(ar['qa'].ptr, ar['qb'].ptr, ar['view_cs'].ptr, ar['row_weight'].ptr,
                                                             n_views, n_ch, rows, T, 60.0, 100.0, FAN / n_ch, 2 * np.pi / n_views,
                                                             row_z0, 0.8, 0.0, N, fov, n_slices, -1.0, 0.5, ar['image'].ptr, sp())),
                ['image'])['image'].view(F64)
    assert np.all(np.isfinite(img)) and np.any(img != 0.0)
    assert hip.dexct_last_hip_error() == ar.hip_error_before


def test_argument_errors_launch_nothing(hip):
    """One channel more than DEXCT_FBP_VAR_MAX_CHANNELS: DEXCT_ERANGE and the outputs keep their fill; null pointers and n_planes < 1:
    DEXCT_EINVAL, for the three entry points."""
    from dex_ct_sim_amd import _native
    EINVAL, ERANGE = -1, -2
    n_ch = _native.FBP_VAR_MAX_CHANNELS + 1
    ar = arena(hip)
    for name, n in (('cov', 2 * n_ch), ('taps', 2 * n_ch - 1), ('weight', n_ch), ('qa', 2 * n_ch), ('qb', 2 * n_ch), ('view_cs', 4),
                    ('row_weight', 2), ('image', 2 * 8 * 8)):
        ar.alloc(name, 8 * n)
    p = {k: ar[k].ptr for k in ar.buffers}

    def filt(cov=p['cov'], taps=p['taps'], weight=p['weight'], qa=p['qa'], qb=p['qb'], n=n_ch, T=1, theta=2 * np.pi, off=0, tot=2):
        return hip.dexct_fbp_var_filter(cov, 2, 1, n, T, taps, weight, 1e-4, theta, off, tot, qa, qb, sp())

    def back(qa=p['qa'], qb=p['qb'], cs=p['view_cs'], img=p['image'], T=1, n=16):
        return hip.dexct_fbp_var_backproject(qa, qb, cs, 2, n, 2, T, 60.0, 0.01, 3.14, 8, 30.0, img, sp())

    def fdk(qa=p['qa'], qb=p['qb'], cs=p['view_cs'], rw=p['row_weight'], img=p['image'], T=1, rows=2):
        return hip.dexct_fdk_var_backproject(qa, qb, cs, rw, 2, 16, rows, T, 60.0, 100.0, 0.01, 3.14, -0.5, 1.0, 0.0, 8, 30.0, 2, -0.5, 1.0,
                                             img, sp())

    for byte in (0x00, 0xFF):
        ar.fill(byte, inner=tuple(ar.buffers))
        assert filt() == ERANGE and filt(T=65536, n=16) == ERANGE
        for kw in (dict(cov=None), dict(taps=None), dict(weight=None), dict(qa=None), dict(qb=None), dict(T=0), dict(T=-1), dict(n=1),
                   dict(n=16, off=1), dict(n=16, off=-1), dict(n=16, tot=1), dict(n=16, theta=3.0), dict(n=16, theta=0.0)):
            assert filt(**kw) == EINVAL, kw
        for kw in (dict(qa=None), dict(qb=None), dict(cs=None), dict(img=None), dict(T=0), dict(n=1)):
            assert back(**kw) == EINVAL, kw
        for kw in (dict(qa=None), dict(qb=None), dict(cs=None), dict(rw=None), dict(img=None), dict(T=0), dict(rows=1)):
            assert fdk(**kw) == EINVAL, kw
        ar.check()
        for k in ('qa', 'qb', 'image'):
            assert np.all(ar[k].get() == byte), k
    assert hip.dexct_last_hip_error() == ar.hip_error_before


# ---- main.py --noise-maps ---------------------------------------------------------------------------------------------------------
def test_main_writes_the_noise_maps(hip, tmp_path):
    """The tiny scan of tests/test_gpu_main_covariance.py with a 24 x 24 reconstruction: the three cov*_recon files are
    get_recon_covariance of the written (float32) covariance sinograms, cast to float32 - exactly; without the flag they are absent
    and the other files are the same; --noise-maps without --covariance (or without a back-projection) is refused."""
    import dex_ct_sim_amd as dx
    params = json.load(open(os.path.join(INPUT, 'params.txt')))
    params.update({'RUN_ID': 'tiny', 'Nx': 48, 'Ny': 48, 'dx': 0.4, 'dy': 0.4, 'N_channels': 96, 'N_projections': 60,
                   'back_project': True, 'N_recon_matrix': 24, 'FOV_recon': 20.0})
    pf = tmp_path / 'params.txt'
    pf.write_text(json.dumps(params))
    main_py = os.path.join(ROOT, 'dex-ct-sim_amd', 'main.py')
    common = ['--params', str(pf), '--input-dir', INPUT, '--pairs', '140kV:80kV:5:5', '--n-iters', '30']
    subprocess.run([sys.executable, main_py, *common, '--out', str(tmp_path / 'o'), '--covariance', '--noise-maps'], check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    sub = os.path.join('tiny', 'matdecomp_140kV_80kV_5000uGy_5000uGy')
    d = tmp_path / 'o' / sub
    ct = dx.read_parameter_file(str(pf), base_dir=os.path.dirname(INPUT))[0][3]
    cov = np.stack([np.fromfile(d / f'cov{t}_sino_float32.bin', dtype=np.float32).reshape(ct.N_proj, ct.N_channels)
                    for t in ('11', '12', '22')], axis=-1)
    want = dx.get_recon_covariance(cov, ct, 24, 20.0, params['ramp_filter_percent_Nyquist']).astype(np.float32)
    assert np.all(want[..., 0] > 0.0) and np.all(want[..., 2] > 0.0)
    for t, name in enumerate(('cov11', 'cov12', 'cov22')):
        got = np.fromfile(d / f'{name}_recon_float32.bin', dtype=np.float32).reshape(24, 24)
        assert np.array_equal(got, want[..., t]), name
    # the same process from here on: main() of the same file
    spec = importlib.util.spec_from_file_location('dexct_main_under_test', main_py)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main([*common, '--out', str(tmp_path / 'p'), '--covariance'])
    plain = tmp_path / 'p' / sub
    with_maps, without = sorted(os.listdir(d)), sorted(os.listdir(plain))
    assert sorted(set(with_maps) - set(without)) == ['cov11_recon_float32.bin', 'cov12_recon_float32.bin', 'cov22_recon_float32.bin']
    for f in without:
        assert (plain / f).read_bytes() == (d / f).read_bytes(), f
    with pytest.raises(SystemExit) as e:
        mod.main([*common, '--out', str(tmp_path / 'q'), '--noise-maps'])
    assert e.value.code != 0 and not (tmp_path / 'q').exists()
    params['back_project'] = False
    pf.write_text(json.dumps(params))
    with pytest.raises(SystemExit) as e:
        mod.main([*common, '--out', str(tmp_path / 'q'), '--covariance', '--noise-maps'])
    assert e.value.code != 0 and not (tmp_path / 'q').exists()
