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


# ---- the cone scans at the edge of the slope contract (bounds_refs.EDGE_SCANS) --------------------------------------------------

_edge_figures = {}


def edge_figures(name):
    """Both CPU references of an edge scan and what the tests below ask of it, computed once per scan."""
    if name not in _edge_figures:
        from oracle import c_oracle as co
        s = br.scan(name)
        g = s.geom(co.make_geom)
        cone = lambda dda: co.project_cone(g, s.view_cs, s.chan_cs, 0, s.n_views, s.row_z, s.src_z, s.vol, s.mu, s.w, dda=dda, n_threads=8)
        (cnt_m, pl_m), (cnt_c, pl_c) = cone(True), cone(False)
        tie = br.tie_rays(s, 0, s.n_views)
        live = ~np.broadcast_to(tie[:, None, :, None], pl_m.shape)
        rays = br.cone_rays_f64(s)
        fig = dict(tie=float(tie.mean()), pathlen=float(np.abs(pl_m.astype(F64) - pl_c)[live].max()),
                   counts=br.counts_rel(cnt_m, cnt_c, tie), past=float(rays['past'].max()),
                   sw=float(np.abs(rays['SW']).max() / 2.0 ** 40), ties=int(rays['ties'].sum()),
                   n_slabs=int(co.plan(g, s.view_cs, s.chan_cs, 0, s.n_views)['n_slabs'].max()),
                   material=(pl_c[..., 1:].sum(-1) if s.n_mat > 1 else pl_c[..., 0]) > 0.0)          # [views][rows][channels]
        print(name, {k: (round(float(v.mean()), 3) if k == 'material' else v) for k, v in fig.items()})
        _edge_figures[name] = fig
    return _edge_figures[name]


AT_THE_LIMIT = sorted(n for n in br.EDGE_SCANS if n != 'edge90')


@pytest.mark.parametrize('name', sorted(br.EDGE_SCANS))
def test_edge_scans_sit_on_the_slope_limit(name):
    """max_abs_dz of every edge scan is the last float64 the restated cone_slope_ok accepts: the next one is refused (edge90:
    0.9 of that value).  tests/test_gpu_bounds_projection.py shows the library draws the line at the same float64."""
    s = br.scan(name)
    limit = br.slope_limit(s.dx, s.dy, s.dz, s.sdd)
    up = float(np.nextafter(limit, np.inf))
    assert br.slope_ok(limit, s.dx, s.dy, s.dz, s.sdd) and not br.slope_ok(up, s.dx, s.dy, s.dz, s.sdd)
    assert br.slope_ok(s.max_abs_dz, s.dx, s.dy, s.dz, s.sdd)
    if name == 'edge90':
        assert abs(s.max_abs_dz / limit - 0.9) < 1e-12
    else:
        assert s.max_abs_dz == limit
        assert not br.slope_ok(float(np.nextafter(s.max_abs_dz, np.inf)), s.dx, s.dy, s.dz, s.sdd)


@pytest.mark.parametrize('name', sorted(br.EDGE_SCANS))
def test_edge_scan_mirror_against_float64_siddon(name):
    """The two CPU references agree at the slope limit as they do far below it: no tie rays beyond the 2 % cap, per-material path
    lengths of the mirror within 2e-6 cm of the float64 3-D Siddon on every other ray (3.5 x the worst of the CPU probes that
    chose these scans, both sides references; chords up to 11.3 cm), counts within REL_TOL.  Measured (tie share 0 everywhere):
                 path length [cm]  counts (rel)               path length [cm]  counts (rel)
      edge         4.5e-7           5.7e-8       edge288       1.8e-7           6.3e-8
      edge_m2      4.6e-7           1.1e-7       edge544       2.0e-7           7.7e-8
      edge_m1      6.8e-7           1.4e-10      edge1056      2.0e-7           5.3e-8
      edge_m5      3.2e-7           1.1e-7       edge1040      1.7e-7           8.1e-8
      edge_m7      2.1e-7           8.2e-8       edge_r257     2.5e-7           9.1e-8
      edge_thin    2.5e-7           1.0e-7       edge_slabs    5.1e-7           7.9e-8
      edge_above   3.0e-7           1.1e-7       edge90        3.7e-7           5.5e-8
      edge_aniso   4.1e-7           7.9e-8"""
    from test_gpu_siddon import REL_TOL
    fig = edge_figures(name)
    assert fig['tie'] <= 0.02
    assert fig['pathlen'] <= 2e-6, fig['pathlen']
    assert fig['counts'] < REL_TOL, fig['counts']


def test_edge_scans_reach_what_they_claim():
    """The figures that make the edge scans worth their run.  Measured:
      edge        every ray crosses material (the two outermost rows included); 34 slabs with tv == tw < 1 in float32
      edge_thin   29 % of the rays cross material; a ray's slice coordinate runs 33.4 slices past a z face
      edge_above  18 % cross material; 65.9 slices past a z face
      edge_slabs  131 slabs on the longest ray (its chord: 11.3 cm)
      max |SW| / 2^40: 1.000000 for every scan at the limit but edge_aniso (0.995013: dy = 0.99 dx), 0.9 for edge90"""
    edge = edge_figures('edge')
    assert edge['material'].mean() >= 0.9 and edge['material'][:, [0, -1]].all()
    assert edge['ties'] >= 1
    for name in ('edge_thin', 'edge_above'):
        fig = edge_figures(name)
        assert fig['past'] > 16.0 and fig['material'].mean() >= 0.1, name
    assert edge_figures('edge_slabs')['n_slabs'] > 128
    for name in AT_THE_LIMIT:
        assert edge_figures(name)['sw'] >= 0.99, name
    assert 0.89 < edge_figures('edge90')['sw'] <= 0.9


def test_row_centre_moves_the_rows_only():
    """Scan(row_centre=c): the same rows, centred on c; without it the scan is what it was."""
    a, b = br.Scan(**br.SCANS['cone']), br.Scan(**dict(br.SCANS['cone'], row_centre=0.25))
    assert np.array_equal(b.row_z, a.row_z + 0.25) and np.array_equal(a.row_z, (np.arange(10) - 4.5) * 0.8)
    assert np.array_equal(a.vol, b.vol) and np.array_equal(a.mu, b.mu) and np.array_equal(a.w, b.w)


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
