"""dexct_gn_decompose_multi on the device: K = 2 .. 4 measurements, M = 2 .. 3 basis materials, against arrays the real
reference produced (tests/golden/ref_multi.npz, gn_reference.npz) and against the NumPy restatement tests/gn_multi_refs.py,
which tests/test_gn_multi_refs.py pins to the same arrays at 1e-12.

Tolerances: 1e-9 of max(|a|, 1) per component on every pixel is the project's figure for decomposed thicknesses against the
reference (tests/test_gpu_gn.py, TOL_F64); no pixel is left out anywhere (the inputs are well conditioned: the reference and
the restatement move by < 1e-12 when the order of the energies is reversed)."""
import os

import numpy as np
import pytest
import torch

import gn_multi_refs as mr
from conftest import GOLDEN, INPUT
from guarded import Arena, twice

pytestmark = pytest.mark.gpu
TOL = 1e-9
F64 = np.float64


@pytest.fixture(scope='module')
def goldens():
    return mr.load_goldens(os.path.join(GOLDEN, 'ref_multi.npz'))


def solve(g, i0, mus, n_iters, **kw):
    """counts [K, ...] (NumPy; their dtype is kept) -> NumPy [..., M] through gn_device_multi"""
    from dex_ct_sim_amd import matdecomp as md
    t = torch.from_numpy(np.ascontiguousarray(g)).to('cuda')
    return md.gn_device_multi(t, i0, mus, n_iters, **kw).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize('n_iters', [30, 50])
def test_goldens_from_float64_counts(hip, goldens, n_iters):
    from dex_ct_sim_amd import matdecomp as md
    for c in goldens:
        a = solve(c['g'], c['i0'], c['mus'], n_iters)
        assert a.shape == c['a'][n_iters].shape and a.dtype == F64
        e = mr.rel_err(a, c['a'][n_iters])
        print(f"{c['name']} n_iters={n_iters}: {e:.2e}")
        assert e <= TOL, (c['name'], e)
        # the drop-in signature: the spectrum tiled over the channels, NumPy in and out
        tiled = np.ascontiguousarray(np.broadcast_to(c['i0'][:, None, :], (c['i0'].shape[0], 16, c['i0'].shape[1])))
        b = md.optimize_sino_cpu(c['g'], None, tiled, c['mus'], n_iters, verbose=False)
        assert isinstance(b, np.ndarray) and np.array_equal(bits(b), bits(a)), c['name']


# (ci = 1, the detunedMV pair, after 5 iterations is left to tests/test_gpu_gn.py, which documents why no restatement of the
# reference reproduces that transient to 1e-9.)
@pytest.mark.parametrize('ci,n_iters', [(0, 1), (0, 2), (0, 5), (0, 50), (1, 1), (1, 2), (1, 50), (2, 1), (2, 2), (2, 5), (2, 50)])
def test_two_by_two_through_the_new_entry_point(hip, golden, ci, n_iters):
    """K = M = 2 through dexct_gn_decompose_multi, on the pixels of gn_reference.npz: the reference's trajectories (after 1 / 2 /
    5 / 50 iterations) at 1e-9, and the 2 x 2 path itself with the fixed count (stop_tol = 0) at 1e-12 where the iteration has
    arrived (50 iterations), as tests/test_gpu_gn.py compares the 2 x 2 path's own two kernels.  The two sum the energies in
    different orders; an iterate still on its way carries cond(H) x that rounding, the fixed point does not (measured on the
    MI355X: after 1 - 5 steps both kernels are 2e-12 .. 4.5e-11 from the reference's own goldens and 2.6e-12 .. 3.7e-11 from each
    other; after 50 steps 2.2e-14 and 1.5e-14): on the way the 2 x 2 path is held to the 1e-9 of the goldens."""
    from dex_ct_sim_amd import matdecomp as md
    g, i0, mus = golden[f'gn{ci}_g'], golden[f'gn{ci}_i0'], golden[f'gn{ci}_mus']
    a = solve(g, i0, mus, n_iters)
    e_gold = mr.rel_err(a, golden[f'gn{ci}_a_iters{n_iters}'])
    two = md.optimize_sino(g, None, i0, mus, n_iters, verbose=False, precision='f64', stop_tol=0.0)
    e_two = mr.rel_err(a, two)
    print(f'case {ci} n_iters={n_iters}: vs golden {e_gold:.2e}, vs the 2 x 2 path {e_two:.2e}')
    assert e_gold <= TOL
    assert e_two <= (1e-12 if n_iters == 50 else TOL)


_sweep_refs = {}


def sweep_reference(K, M, n_e, f32):
    """the restatement on the 1000 pixels of a sweep case (pixels are independent: every smaller size is a prefix), once"""
    key = (K, M, n_e, f32)
    if key not in _sweep_refs:
        g, i0, mus = mr.sweep_case(K, M, n_e)
        g = g.astype(np.float32) if f32 else g
        _sweep_refs[key] = (g, i0, mus, mr.newton_solve_multi(g.astype(F64), i0, mus, 30))
    return _sweep_refs[key]


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('n_e', [8, 47, 48, 49, 239])
@pytest.mark.parametrize('K,M', mr.SHAPES)
def test_shape_sweep_against_the_restatement(hip, K, M, n_e, f32):
    g, i0, mus, ref = sweep_reference(K, M, n_e, f32)
    worst = 0.0
    for n_pix in (1, 63, 64, 65, 255, 256, 257, 1000):
        a = solve(g[:, :n_pix], i0, mus, 30)
        assert a.shape == (n_pix, M)
        e = mr.rel_err(a, ref[:n_pix])
        assert e <= TOL, (n_pix, e)
        worst = max(worst, e)
    print(f'K={K} M={M} nE={n_e} {"f32" if f32 else "f64"}: {worst:.2e}')


def test_full_loop_changes_no_bit(hip, goldens):
    """The exit on an update that returns its own input, against every iteration executed: the same bits on every golden case,
    the noisy ones included, at iteration counts before and after the pixels have settled."""
    for c in goldens:
        for n_iters in (1, 7, 30, 50):
            a = solve(c['g'], c['i0'], c['mus'], n_iters)
            b = solve(c['g'], c['i0'], c['mus'], n_iters, full_loop=True)
            assert np.array_equal(bits(a), bits(b)), (c['name'], n_iters)


@pytest.mark.parametrize('name', ['syn_k4m3a_noisy', 'syn_k3m2b_noisy'])
def test_mask(hip, goldens, name):
    c = next(c for c in goldens if c['name'] == name)
    M = c['mus'].shape[0]
    plain = solve(c['g'], c['i0'], c['mus'], 30)
    gmax = torch.tensor(float(c['g'][0].max()), dtype=torch.float64, device='cuda')
    masked_any = False
    for frac in (0.3, 0.95):
        air = c['g'][0] >= frac * c['g'][0].max()
        assert air.any() and not air.all()
        a = solve(c['g'], c['i0'], c['mus'], 30, mask_max=gmax, mask_frac=frac)
        assert np.array_equal(bits(a[air]), np.zeros((int(air.sum()), M), np.uint64))          # +0.0 in every component
        assert np.array_equal(bits(a[~air]), bits(plain[~air]))
        masked_any = masked_any or air.sum() > 1
    assert masked_any


def guarded_call(lib, g, i0, mus, K, M, n_iters=30):
    """dexct_gn_decompose_multi with counts, tables, workspace and output between guards, run with 0x00 and with 0xFF fill:
    outputs bit-identical, guards intact, no HIP error (guarded.twice); returns the output [n_pix, M].
    (The library's last HIP error is per thread and never cleared: an earlier test of the session that provoked a refusal on
    purpose leaves it set.  So it is compared with the value it had before the launches - 0 when this file runs alone - not
    with 0 as Arena.check would, as tests/test_gpu_gn_reduced.py does; every call is also checked by its return code.)"""
    from dex_ct_sim_amd._device import stream_ptr
    n_pix, n_e = g.shape[1], i0.shape[1]
    ar = Arena('cuda', None)
    hip_error_before = lib.dexct_last_hip_error()
    for name, arr in (('g', g), ('i0', np.ascontiguousarray(i0, F64)), ('mus', np.ascontiguousarray(mus, F64))):
        ar.alloc(name, arr.nbytes).put(arr)
    ar.alloc('workspace', lib.dexct_gn_multi_workspace_bytes(K, M, n_e))
    ar.alloc('out_a', 8 * M * n_pix)

    def launch():
        assert lib.dexct_gn_decompose_multi(ar['g'].ptr, int(g.dtype == F64), n_pix, K, M, ar['i0'].ptr, ar['mus'].ptr, n_e, n_iters,
                                            None, 0.95, 0, ar['out_a'].ptr, ar['workspace'].ptr, stream_ptr()) == 0

    out = twice(ar, launch, ['out_a'], scratch=['workspace'])['out_a'].view(F64).reshape(n_pix, M)
    assert lib.dexct_last_hip_error() == hip_error_before
    return out


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('K,M', [(4, 3), (3, 2)])
def test_guard_banded_buffers(hip, K, M, f32):
    n_pix = 257
    g, i0, mus, ref = sweep_reference(K, M, 47, f32)
    g = np.ascontiguousarray(g[:, :n_pix])
    clean = guarded_call(hip, g, i0, mus, K, M)
    assert mr.rel_err(clean, ref[:n_pix]) <= TOL
    # a few counts no scan produces: whatever they make of their own pixel, every other pixel keeps its bits
    bad = g.copy()
    where = {(0, 3): np.nan, (K - 1, 64): 0.0, (1, 130): -1.0, (0, 255): np.inf, (K - 1, 256): np.nan}
    for (k, p), v in where.items():
        bad[k, p] = v
    got = guarded_call(hip, bad, i0, mus, K, M)
    keep = np.ones(n_pix, bool)
    keep[[p for _, p in where]] = False
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    assert np.all(np.isnan(got[3])) and np.all(np.isnan(got[256]))


def test_end_to_end_photon_counting_bins(hip):
    """Three energy bins of one spectrum scanned in one traversal and decomposed into two materials, against the restatement
    applied to the same float32 counts; the reference's mask rule; a NaN count stays in its pixel."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md, synthetic
    ph = synthetic.make_phantom(32, 1)
    ct = dx.FanBeamGeometry(N_channels=64, N_proj=12, eid=False, detector_file=os.path.join(INPUT, 'detector', 'eta_pcd_Si_30mm.bin'))
    specs = dx.energy_bins(synthetic.kramers_spectrum(120), [25.0, 50.0, 70.0, 121.0])
    sinos = [raw for raw, _ in dx.get_sinos(ct, ph, specs)]
    assert len(sinos) == 3 and all(s.shape == (12, 64) and s.dtype == np.float32 for s in sinos)
    n_iters = 30
    out = md.get_basismat_sinos_multi(ct, sinos, specs, n_iters=n_iters)
    assert isinstance(out, tuple) and len(out) == 2
    assert all(isinstance(m, np.ndarray) and m.shape == (12, 64) and m.dtype == F64 for m in out)
    a = np.stack(out, axis=-1)
    # the reference's mask rule (matdecomp.py:195-196, :204-205), from the first sinogram
    air = sinos[0] >= 0.95 * np.max(sinos[0])
    assert air.any() and not air.all()
    assert not a[air].any()
    _, i0, mus = md.decomposition_tables_multi(ct, specs)
    ref = mr.newton_solve_multi(np.stack(sinos).astype(F64), i0, mus, n_iters)
    assert np.all(np.isfinite(ref[~air]))
    e = mr.rel_err(a[~air], ref[~air])
    print(f'end to end vs restatement: {e:.2e}; tissue up to {a[..., 0].max():.2f}, bone up to {a[..., 1].max():.2f} g/cm^2')
    assert e <= TOL
    assert a[..., 0].max() > 10.0                                  # the water cylinder is there
    # device tensors in, device tensors out, the same bits
    dev_out = md.get_basismat_sinos_multi(ct, [torch.from_numpy(s).to('cuda') for s in sinos], specs, n_iters=n_iters)
    assert all(isinstance(m, torch.Tensor) and m.is_cuda for m in dev_out)
    assert np.array_equal(bits(np.stack([m.cpu().numpy() for m in dev_out], axis=-1)), bits(a))
    # one count NaN: NaN there only; strict raises
    v, ch = np.argwhere(~air)[len(np.argwhere(~air)) // 2]
    hurt = [s.copy() for s in sinos]
    hurt[1][v, ch] = np.nan
    b = np.stack(md.get_basismat_sinos_multi(ct, hurt, specs, n_iters=n_iters), axis=-1)
    assert np.all(np.isnan(b[v, ch]))
    b[v, ch] = a[v, ch]
    assert np.array_equal(bits(b), bits(a))
    with pytest.raises(md.SingularHessianError):
        md.get_basismat_sinos_multi(ct, hurt, specs, n_iters=n_iters, strict=True)
    assert issubclass(md.SingularHessianError, np.linalg.LinAlgError)
