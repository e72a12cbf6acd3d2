"""dexct_gn_decompose_multi on the device against an extended-precision root (tests/gn_multi_root_refs.py, which
tests/test_gn_multi_root_refs.py shows to be usable and to reject wrong variants of the kernel's arithmetic).

Root.  After 50 iterations every usable pixel of every case must satisfy |a - root|_m <= C scale_m, with
scale_m = 2^-53 (|H^-1| s)_m at the long-double root and C = 4 x the worst such ratio of the float64 restatement and of three
emulations of the kernel's order on the CPU (1.79 on x86-64: worst CPU ratio 0.448), never a device figure.  Float64 counts, and
float32 counts against the root of the float32 values widened to float64; 1, 255, 256, 257 pixels and the whole case, as
prefixes.  The line cases are also held to their closed form on the same scale.  Early iterates: 1, 2 and 3 iterations against
the long-double trajectory at the project's 1e-9 max(|a|, 1).  The cap: 4096 energies are solved and bounded like the rest,
4097 are refused before anything is launched.

No clip claim: the largest exponent of any case is 21.4, so the +-700 clip of the exponent is never engaged here; it remains
covered by the special-pixel tests of tests/test_gpu_gn_multi.py.

Usable: 1000 / 1000 pixels of every case (64 / 64 of the cap case) but 'wide K=3 M=3 nE=8 noisy' with 995 / 1000; the early
trajectories 1000 / 1000 everywhere.

Measured on an MI355X, worst ratio per shape over the wide and gaps cases, float64 / float32 counts (allowed: 1.79):
    K x M     2 x 2         3 x 2         4 x 2         3 x 3         4 x 3
              0.40 / 0.45   0.40 / 0.46   0.37 / 0.42   0.10 / 0.09   0.14 / 0.15
    lines K = M = 2: 0.52 / 0.43, K = M = 3: 0.90 / 0.60 (root and closed form alike); 4096 energies: 0.50 / 0.50
    iterates 1 - 3: at most 2.9e-13 max(|a|, 1) from the long-double trajectory (K = M = 3, 8 energies, third step)
"""
import numpy as np
import pytest
import torch

import gn_multi_root_refs as rr
from guarded import Arena

pytestmark = pytest.mark.gpu
F64 = np.float64
PIXELS = (1, 255, 256, 257)
ERANGE = -2
NAMES = [c['name'] for c in rr.all_cases()]
EARLY_NAMES = [c['name'] for c in rr.early_cases()]


def solve(g, i0, mus, n_iters, **kw):
    """counts [K, P] (NumPy; their dtype is kept) -> NumPy [P, M] through gn_device_multi"""
    from dex_ct_sim_amd import matdecomp as md
    t = torch.from_numpy(np.ascontiguousarray(g)).to('cuda')
    return md.gn_device_multi(t, i0, mus, n_iters, **kw).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def held_to(case, ref, f32, what):
    """every prefix and the whole case, 50 iterations, each usable pixel within C of ``ref``; the worst ratio"""
    g = rr.counts_of(case, f32)
    n_all = g.shape[1]
    assert int((~ref['usable']).sum()) <= rr.UNUSABLE_CAP * n_all
    worst = 0.0
    for n_pix in tuple(n for n in PIXELS if n < n_all) + (n_all,):
        a = solve(g[:, :n_pix], case['i0'], case['mus'], 50)
        assert a.shape == (n_pix, case['M']) and a.dtype == F64
        r = rr.worst_ratio(a, ref, n_pix)
        print(f"{case['name']} {'f32' if f32 else 'f64'} {what} n_pix={n_pix}: ratio {r:.3f} (allowed {rr.C:.3f})")
        assert r <= rr.C, (case['name'], n_pix, r)
        worst = max(worst, r)
    print(f"{case['name']} {'f32' if f32 else 'f64'} {what}: worst ratio {worst:.3f}, usable {int(ref['usable'].sum())} / {n_all}")
    return worst


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', NAMES)
def test_root(hip, name, f32):
    case = rr.case_named(name)
    held_to(case, rr.reference_of(case, f32), f32, 'root')


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('K', [2, 3])
def test_line_cases_against_the_closed_form(hip, K, f32):
    case = rr.case_named(f'lines K=M={K}')
    ref = rr.reference_of(case, f32)
    exact = rr.closed_form(case, rr.counts_of(case, f32).astype(F64))
    held_to(case, dict(ref, root=exact), f32, 'closed form')


@pytest.mark.parametrize('name', NAMES)
def test_full_loop_changes_no_bit(hip, name):
    case = rr.case_named(name)
    a = solve(case['g'], case['i0'], case['mus'], 50)
    b = solve(case['g'], case['i0'], case['mus'], 50, full_loop=True)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize('name', EARLY_NAMES)
def test_early_iterates(hip, name):
    case = rr.case_named(name)
    traj = rr.trajectory_of(case)
    assert int((~traj['usable']).sum()) <= rr.UNUSABLE_CAP * len(traj['usable'])
    for n in rr.EARLY_STEPS:
        a = solve(case['g'], case['i0'], case['mus'], n)
        e = rr.early_err(a, traj, n)
        print(f"{name} after {n} iterations: {e:.2e} (usable {int(traj['usable'].sum())} / {len(traj['usable'])})")
        assert e <= rr.EARLY_TOL, (n, e)


def test_one_energy_past_the_cap_is_refused(hip):
    """4097 energies: no workspace size, DEXCT_ERANGE, nothing launched - the output keeps its fill, every guard is intact and
    the library's last HIP error is what it was before the call (it is per thread and never cleared, see
    test_gpu_gn_multi.guarded_call)."""
    from dex_ct_sim_amd import matdecomp as md
    from dex_ct_sim_amd._device import stream_ptr
    K, M, n_pix, n_e = 4, 3, rr.CAP_PIXELS, rr.CAP_ENERGIES + 1
    assert hip.dexct_gn_multi_workspace_bytes(K, M, rr.CAP_ENERGIES) > 0
    assert hip.dexct_gn_multi_workspace_bytes(K, M, n_e) == 0
    rng = np.random.default_rng(37)
    g, i0, mus = rng.uniform(10.0, 100.0, (K, n_pix)), rng.uniform(1.0, 2.0, (K, n_e)), rng.uniform(0.1, 0.2, (M, n_e))
    ar = Arena('cuda', None)
    for name, arr in (('g', g), ('i0', i0), ('mus', mus)):
        ar.alloc(name, arr.nbytes).put(arr)
    ar.alloc('workspace', hip.dexct_gn_multi_workspace_bytes(K, M, rr.CAP_ENERGIES))
    ar.alloc('out_a', 8 * M * n_pix)
    hip_error_before = hip.dexct_last_hip_error()
    for fill in (0x00, 0xFF, 0x5A):
        ar.fill(fill, inner=('out_a', 'workspace'))
        rc = hip.dexct_gn_decompose_multi(ar['g'].ptr, 1, n_pix, K, M, ar['i0'].ptr, ar['mus'].ptr, n_e, 50, None, 0.95, 0,
                                          ar['out_a'].ptr, ar['workspace'].ptr, stream_ptr())
        assert rc == ERANGE
        torch.cuda.synchronize()
        assert hip.dexct_last_hip_error() == hip_error_before
        for b in ar.buffers.values():
            b.check()
        assert np.all(ar['out_a'].get() == fill) and np.all(ar['workspace'].get() == fill)
    with pytest.raises(ValueError):
        md.gn_device_multi(torch.from_numpy(g).to('cuda'), i0, mus, 50)
