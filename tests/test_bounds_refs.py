"""CPU self-test of tests/bounds_refs.py: the comparisons of the guard-banded projection and reconstruction tests reject a
slightly wrong result, accept a correctly rounded float32 evaluation, and the exclusion caps hold for every chosen geometry.
No device: the "kernel" here is the float64 reference rounded to float32, or a float32 NumPy evaluation in the kernel's order."""
import numpy as np
import pytest

import bounds_refs as br
from bounds_refs import F32, F64, U


def shift(a, axis=-1):
    """``a`` moved by one along ``axis``, zeros moving in."""
    out = np.roll(a, 1, axis=axis)
    out[(slice(None),) * (axis % a.ndim) + (0,)] = 0
    return out


def test_parker_comparison():
    rng = np.random.default_rng(1)
    sino = rng.uniform(0.1, 6.0, (5, 3, 257)).astype(F32)
    args = (np.pi + br.FAN + 0.3, br.FAN / 257, 6, 11)
    ref, bound = br.parker_ref(sino, *args)
    assert br.within(ref.astype(F32), ref, bound)
    assert not br.within((ref * (1 + 4 * U)).astype(F32), ref, bound)
    shifted, _ = br.parker_ref(sino, args[0], args[1], 5, 11)                   # the weights of the view before
    assert not br.within(shifted.astype(F32), ref, bound)


def f32_filter(sino, taps, weight, dgamma):
    """fbp_filter_kernel's order in float32 NumPy: even and odd chains (sequential, without the fused multiply-add)."""
    n = sino.shape[-1]
    line = sino * weight
    out = np.zeros_like(sino)
    for k in range(n):
        gk = taps[k + n - 1 - np.arange(n)]
        p = line * gk
        a0 = a1 = np.zeros(sino.shape[0], F32)
        for m in range(0, n, 2):
            a0 = a0 + p[:, m]
        for m in range(1, n, 2):
            a1 = a1 + p[:, m]
        out[:, k] = (a0 + a1) * F32(dgamma)
    return out


@pytest.mark.parametrize('n_ch', [2, 3, 64, 257])
def test_filter_comparison(n_ch):
    from oracle import fbp_oracle as fo
    dgamma = br.FAN / n_ch
    rng = np.random.default_rng(n_ch)
    taps = fo.ramp_taps(n_ch, dgamma).astype(F32)
    weight = (br.SID * np.cos((np.arange(n_ch) - 0.5 * (n_ch - 1)) * dgamma)).astype(F32)
    sino = rng.uniform(0.0, 8.0, (2, n_ch)).astype(F32)
    sino[0] = 1.0
    ref, bound = br.filter_ref(sino, taps, weight, dgamma)
    assert br.within(f32_filter(sino, taps, weight, dgamma), ref, bound)
    assert br.within(ref.astype(F32), ref, bound + U * np.abs(ref))
    # one tap scaled by 1 + 4 n_ch u: the central tap, which every output uses
    bad = taps.copy()
    bad[n_ch - 1] *= F32(1 + 4 * n_ch * U)
    wrong, _ = br.filter_ref(sino, bad, weight, dgamma)
    assert not br.within(wrong, ref, bound)
    # the channels shifted by one
    assert not br.within(shift(ref), ref, bound)


def test_filter_reference_is_the_oracles():
    """filter_ref on exact inputs equals oracle/fbp_oracle.filter_sino (same taps, same weights)."""
    from oracle import fbp_oracle as fo
    n_ch, dgamma = 33, br.FAN / 33
    gam = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * dgamma
    sino = np.random.default_rng(0).uniform(0, 4, (3, n_ch)).astype(F32)
    taps, weight = fo.ramp_taps(n_ch, dgamma), br.SID * np.cos(gam)
    ref, _ = br.filter_ref(sino.astype(F64), taps, weight, dgamma)
    assert np.allclose(ref, fo.filter_sino(sino, gam, br.SID), rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize('case', br.BACKPROJECT, ids=lambda c: '-'.join(str(v) for v in c))
def test_backproject_comparison_and_edge_cap(case):
    p = br.backproject_problem(case)
    ref, bound, keep = br.backproject_ref(**p)
    assert (~keep).mean() <= 0.01
    assert br.within(ref.astype(F32)[keep], ref[keep], (bound + U * np.abs(ref))[keep])
    if np.any(bound > 0):
        # a dropped view
        q2 = dict(p, q=p['q'][:-1], view_cs=p['view_cs'][:-1])
        less, _, _ = br.backproject_ref(**q2)
        assert not br.within(less[keep], ref[keep], bound[keep])
        # the channels shifted by one
        shifted, _, _ = br.backproject_ref(**dict(p, q=shift(p['q'])))
        assert not br.within(shifted[keep], ref[keep], bound[keep])


def test_backproject_reference_is_the_oracles():
    from oracle import fbp_oracle as fo
    n_views, n_ch, N, fov = 12, 65, 33, 30.0
    th = 2 * np.pi * np.arange(n_views) / n_views
    gam = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * (br.FAN / n_ch)
    q = np.random.default_rng(3).standard_normal((n_views, 1, n_ch)).astype(F32)
    vcs = np.stack([np.cos(th), np.sin(th)], 1)
    ref, _, _ = br.backproject_ref(q, vcs, br.SID, br.FAN / n_ch, th[1] - th[0], N, fov)
    want = fo.back_project(q[:, 0], th, gam, br.SID, N, fov)
    assert np.allclose(ref[0], want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('case', br.FDK, ids=lambda c: '-'.join(str(v) for v in c))
def test_fdk_comparison_and_edge_cap(case):
    p = br.fdk_problem(case)
    ref, bound, keep = br.fdk_ref(**p)
    assert (~keep).mean() <= 0.01
    assert np.any(bound > 0)
    assert br.within(ref.astype(F32)[keep], ref[keep], (bound + U * np.abs(ref))[keep])
    less, _, _ = br.fdk_ref(**dict(p, q=p['q'][:-1], view_cs=p['view_cs'][:-1]))
    assert not br.within(less[keep], ref[keep], bound[keep])
    rows, _, _ = br.fdk_ref(**dict(p, q=shift(p['q'], 1)))             # the rows shifted by one
    assert not br.within(rows[keep], ref[keep], bound[keep])


def test_fdk_reference_is_the_oracles():
    """fdk_ref on a filtered sinogram equals the back-projection half of oracle/fbp_oracle.fdk_recon."""
    from oracle import fbp_oracle as fo
    p = br.fdk_problem((8, 33, 5, 17, 20.0, 3))
    n_views, n_rows, n_ch = p['q'].shape
    th = 0.013 + 2 * np.pi * np.arange(n_views) / n_views
    gam = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * p['dgamma']
    row_z = p['row_z0'] + p['row_dz'] * np.arange(n_rows)
    slices = p['z0'] + p['dz'] * np.arange(3)
    orig = fo.filter_sino
    fo.filter_sino = lambda s, *a, **k: np.asarray(s, F64)                      # q is already filtered
    try:
        want = fo.fdk_recon(p['q'], th, gam, br.SID, br.SDD, row_z, p['src_z'], 17, 20.0, 1.0, slices)
    finally:
        fo.filter_sino = orig
    p['row_weight'] = (br.SDD / np.sqrt(br.SDD ** 2 + (row_z - p['src_z']) ** 2))
    ref, _, _ = br.fdk_ref(**p)
    assert np.allclose(ref, want, rtol=1e-9, atol=1e-12)


def test_vmi_and_moments_references():
    rng = np.random.default_rng(5)
    m1, m2 = rng.uniform(0, 2, 300).astype(F32), rng.uniform(0, 2, 300).astype(F32)
    lab = rng.integers(0, 7, 300, dtype=np.uint8)
    out = br.moments_ref(m1, m2, lab, 5)
    assert out[:, 0].sum() == (lab < 5).sum()
    assert np.isclose(float(out[2, 4]), float((m1[lab == 2].astype(F64) * m2[lab == 2]).sum()), rtol=1e-13)
    assert br.vmi_ref(m1, m2, 0.2, 0.5, 0.2, 1).dtype == F32


@pytest.mark.parametrize('name', sorted(br.SCANS))
def test_tie_ray_cap_of_every_scan(name):
    """At most 2 % of a scan's rays run exactly along a grid plane, for every range of views."""
    s = br.scan(name)
    tie = br.tie_rays(s, 0, s.n_views)
    for vb in range(s.n_views):
        for ve in range(vb + 1, s.n_views + 1):
            if ve - vb > 1 or s.n_views == 1 or s.n_ch >= 50:              # (one view of a few channels: one tie ray is > 2 %)
                assert tie[vb:ve].mean() <= 0.02, (vb, ve)


def test_counts_comparison_rejects_a_wrong_ray():
    from oracle import c_oracle as co
    s = br.scan('r4')
    g = s.geom(co.make_geom)
    ref = co.project_classic(g, s.view_cs, s.chan_cs, 0, s.n_views, s.vol, s.mu, s.w, n_threads=8)
    dda = co.project_dda(g, s.view_cs, s.chan_cs, 0, s.n_views, s.vol, s.mu, s.w, n_threads=8)
    tie = br.tie_rays(s, 0, s.n_views)
    assert br.counts_close(dda.astype(F32), ref, tie, 1e-5)
    bad = dda.astype(F32).copy()
    live = np.argwhere(~tie)[0]
    bad[1, live[0], 2, live[1]] *= F32(1 + 3e-5)
    assert not br.counts_close(bad, ref, tie, 1e-5)
    assert not br.counts_close(np.roll(dda, 1, axis=-1).astype(F32), ref, tie, 1e-5)     # the channels shifted by one
    bad = dda.astype(F32).copy()
    bad[0, 0, 0, 0] = np.nan
    assert not br.counts_close(bad, ref, tie, 1e-5)
