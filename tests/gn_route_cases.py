"""What the suites of the dedup route's streaming passes share (tests/test_gpu_gn_idle_launch.py, test_gpu_gn_expand_repeat.py,
test_gpu_gn_census_wide.py): one call of matdecomp.gn_device with its diagnostics, and the comparison of the route with the direct
route of the same call - a_out between guard bands, a_out and the dedup workspace pre-filled once with 0x00 and once with 0xFF,
every comparison byte for byte.  The sinograms and the pool of counts are those of tests/test_gpu_gn_dedup.py.
"""
import numpy as np
import torch

from gn_dedup_caps import device_expected
from guarded import Arena, twice
from test_gpu_gn_dedup import N_ITERS

MODES = {'one': dict(two_level='one'), 'two': dict(two_level='start'), 'pass0': dict(two_level=False)}      # gn_shortcut_kernel<1>, <2>, gn_refill_kernel<false>
MODE_NAME = {'one': 'one', 'two': 'start', 'pass0': 'single'}
STAT_WORDS = ('pixel_iterations', 'stalled_lane_steps', 'launches', 'mode', 'residual_energies')


def call(pl, t, how, mask, dedup, out=None, dedup_workspace=None):
    """gn_device on the device sinograms t [2][V][C][R] (or [2][n]: plain tiling) -> (a_out, the words last_gn_stats() reports,
    its 'dedup', the finished-pixel word)."""
    from dex_ct_sim_amd import _native, matdecomp as md
    gmax = torch.tensor(pl['air_count'], dtype=torch.float64, device='cuda') if mask else None
    out_rc = (int(t.shape[-1]), int(t.shape[-2])) if t.dim() == 4 else None
    a = md.gn_device(t[0], t[1], pl['i0'], pl['mus'], N_ITERS, 'f64', kernel=1, audit=0, out_rc=out_rc, mask_max=gmax, out=out, dedup=dedup,
                     dedup_workspace=dedup_workspace, **MODES[how])
    st = md.last_gn_stats()
    assert st['mode'] == MODE_NAME[how], st
    word = md._last_run.workspaces[-1][_native.GN_WS_PROGRESS:_native.GN_WS_PROGRESS + 8].view(torch.int64)
    # (pass 0 counts the lane-steps its waves waited for a free result slot: that depends on which wave drew which tile, not on the
    # call - the one word that may differ between two runs of the same launch.  The short cut does not count them: 0.)
    return a, {k: st[k] for k in STAT_WORDS if not (how == 'pass0' and k == 'stalled_lane_steps')}, st.get('dedup'), int(word.item())


def host_fresh(g):
    """bool [V][C][R]: the pixels whose bits differ from the row before (row 0 always) - the census on the host"""
    b = g.view(np.uint32 if g.dtype == np.float32 else np.uint64)
    fresh = np.ones(g.shape[1:], dtype=bool)
    fresh[..., 1:] = (b[:, ..., 1:] != b[:, ..., :-1]).any(axis=0)
    return fresh


def the_list(g, cap):
    """[2][n]: the pad (the count 1.0 up to the tile's start) and the fresh pixels in the order of the pixels: what the launch on
    the list solves."""
    fresh = host_fresh(g)
    n_fresh = int(fresh.sum())
    pad = (cap - n_fresh) % 64
    return np.concatenate([np.ones((2, pad), dtype=g.dtype), g[:, fresh]], axis=1)


def route_equals_direct(hip, pl, g, how, mask, use=None, t=None):
    """The route on g [2][V][C][R] (``t``: the device tensor to use for it - a view at some alignment) against dedup=False: the bytes
    of a_out, the descriptor, every word of last_gn_stats(), the finished-pixel word.  Returns the descriptor."""
    from dex_ct_sim_amd import _native
    V, C, R = g.shape[1:]
    n = V * C * R
    if t is None:
        t = torch.from_numpy(g).cuda()
    a, st_direct, none, done = call(pl, t, how, mask, False)
    assert none is None and done == n, (none, done)
    want = a.view(torch.int64).cpu().numpy()
    arena = Arena(torch.device('cuda', torch.cuda.current_device()), None)
    out = arena.alloc('out', 16 * n)
    dws = arena.alloc('dedup', _native.load().dexct_gn_dedup_workspace_bytes(n, R, int(g.dtype == np.float64)))
    before = hip.dexct_last_hip_error()
    seen = []
    got = twice(arena, lambda: seen.append(call(pl, t, how, mask, True, out=out.view(torch.float64, (V, R, C, 2)), dedup_workspace=dws.inner)[1:]),
                outputs=('out',), scratch=('dedup',))
    assert hip.dexct_last_hip_error() == before
    assert np.array_equal(got['out'].view(np.int64).reshape(V, R, C, 2), want), (g.shape, how, mask)
    want_dd = device_expected(t)
    assert seen[0] == seen[1], seen
    st, dd, done = seen[0]
    assert dd == want_dd and (use is None or dd['use'] == use), (g.shape, dd, want_dd)
    assert done == n, (done, n)
    if dd['use']:
        # the launch on the list is the one that worked: the steps of the list's entries (and of its pad), nothing from the other
        lst = torch.from_numpy(the_list(g, dd['cap'])).cuda()
        _, st_list, _, done_list = call(pl, lst, how, mask, False)
        assert done_list == lst.shape[1]
        assert st == st_list, (st, st_list)
        assert st['pixel_iterations'] <= st_direct['pixel_iterations'] + 63 * N_ITERS
    else:
        assert st == st_direct, (st, st_direct)
    return dd
