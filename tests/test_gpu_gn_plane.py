"""The Newton short cut swept over the plane of its table against an extended-precision root (tests/gn_plane_refs.py): every
4th cell of the domain, cell corners and edges to the last double, the thick end, the rim of the physical ratios and the water
line, the closed rings and the outside of the grid, the frontier between open and closed cells - in the three modes and with
the fixed count, for the bundled 140 / 80 kV pair (golden case 0) and the Kramers 140 / 80 pair.  On every pixel the
reference vouches for, per component:
    |device - root| <= 1e-12 max(|root|, 1) + slack,   slack = |float64 oracle - root|
1e-12 is the library's contract; slack is what the reference's own arithmetic accounts for (below 1e-12 wherever the
reference is usable: gn_plane_refs.reference).  No other tolerance appears; where the reference is not usable the finite /
non-finite pattern is the fixed count's.  The tests print, per set and mode, the largest |device - root| /
max(|root|, 1) and the smallest margin under the bound (run with -s)."""
import numpy as np
import pytest
import torch

import gn_plane_refs as pr
from gn_plane_refs import SEED, tables

pytestmark = pytest.mark.gpu

N_ITERS = 50
MODES = ['one', 'start', False, 'exact']
WANT_MODE = {'one': 'one', 'start': 'start', False: 'single', 'exact': 'single'}


def launch(pl, g, mode, **kw):
    """One launch of the lane kernel on the counts g [n, 2] (NumPy float64 / float32 or a pair of device tensors) -> (result as
    a device tensor, last_gn_stats())."""
    from dex_ct_sim_amd import matdecomp as md
    if isinstance(g, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(g.T)).cuda()
        g = (t[0], t[1])
    how = dict(stop_tol=0.0, two_level=False) if mode == 'exact' else dict(two_level=mode)
    a = md.gn_device(g[0], g[1], pl['i0'], pl['mus'], N_ITERS, 'f64', kernel=1, audit=0, **how, **kw)
    st = md.last_gn_stats()
    assert st['mode'] == WANT_MODE[mode], (mode, st['mode'])
    return a, st


@pytest.fixture(scope='module', params=['case0', 'kramers'])
def plane(hip, request):
    """Per table pair, once: the sets, the launch order, its counts, the reference of every point, the calibrated table."""
    from dex_ct_sim_amd import matdecomp as md, quadrature
    i0, mus = tables(request.param)
    head = quadrature.newton_start_grid(i0, mus)['head']
    sets = pr.point_sets(head, SEED, (i0, mus), pr.DOMAIN_CUT.get(request.param))
    order = pr.interleave(sets, SEED + 1)
    fxy = pr.gather(sets, order)
    g = pr.counts_of(head, fxy[:, 0], fxy[:, 1])
    root, slack, usable = pr.reference(g, i0, mus, screen=order[0] == order[2].index('border'))
    gate = md._device_tables(i0, mus, torch.device('cuda', torch.cuda.current_device()), True)[2]
    assert gate['start'] is not None and not gate['ill_posed']
    n = quadrature.GATE_CELLS
    _, c0, k0, _ = quadrature.start_layout(n)
    start = gate['start'][:k0].cpu().numpy()                              # (header, roots, cells: not the power form behind them)
    assert int(start[3]) == n and np.array_equal(start[:10], head[:10]) and start[11] > 0.0
    pl = {'pair': request.param, 'i0': i0, 'mus': mus, 'head': head, 'sets': sets, 'order': order, 'fxy': fxy, 'g': g, 'root': root,
          'slack': slack, 'usable': usable, 'n': n, 'need': start[c0:k0].reshape(n, n, 2)[:, :, 0].copy(), 'cache': {}}
    return pl


def exact_of(pl, key, g):
    """The fixed count's result on the counts g (one launch per fixture and key)."""
    if key not in pl['cache']:
        pl['cache'][key] = launch(pl, g, 'exact')[0].cpu().numpy().reshape(-1, 2)
    return pl['cache'][key]


def hold(pl, mode, dev, exact, root, slack, usable, fxy, groups, what):
    """The assertion of this module on one launch's result dev [n, 2]; ``groups``: name -> mask, for the report."""
    dev = dev.reshape(-1, 2)
    scale = np.maximum(np.abs(root), 1.0)
    with np.errstate(all='ignore'):
        bound = 1e-12 * scale + slack
        err = np.abs(dev - root)
        over = usable[:, None] & ~(err <= bound)
    for name, m in groups.items():
        mu = m & usable
        if mu.any():
            rel = (err[mu] / scale[mu]).max()
            margin = ((bound[mu] - err[mu]) / scale[mu]).min()
            print(f'{pl["pair"]} {what} mode={mode} {name}: {mu.sum()} of {m.sum()} usable, max |device - root| / max(|root|, 1) = {rel:.2e}, '
                  f'least margin {margin:.2e}')
    if over.any():
        k, c = np.argwhere(over)[np.argmax((err / bound)[over])]
        name = [s for s, m in groups.items() if m[k]]
        raise AssertionError(f'{pl["pair"]} {what} mode={mode}: {over.any(axis=1).sum()} pixels beyond the bound; worst: set {name}, cell '
                             f'({int(np.floor(fxy[k, 0]))}, {int(np.floor(fxy[k, 1]))}) at (fx, fy) = ({fxy[k, 0]!r}, {fxy[k, 1]!r}), component {c}: '
                             f'device {dev[k, c]!r}, root {root[k, c]!r}, |diff| {err[k, c]:.3e} > bound {bound[k, c]:.3e} (slack {slack[k, c]:.3e})')
    assert np.array_equal(np.isfinite(dev).all(axis=1)[~usable], np.isfinite(exact).all(axis=1)[~usable]), (what, mode)


def need_at(pl, fxy):
    """``need`` of the cell floor() puts a point in; inf outside the grid."""
    n = pl['n']
    inside = np.all((fxy >= 0.0) & (fxy < n), axis=1)
    ij = np.where(inside[:, None], np.floor(fxy), 0).astype(np.int64)
    return np.where(inside, pl['need'][ij[:, 0], ij[:, 1]], np.inf), inside


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_plane_sweep(plane, mode):
    """All the sets in one launch, border runs of every length between them."""
    pl = plane
    which, _, names = pl['order']
    assert len(which) % 2 == 1
    exact = exact_of(pl, 'sweep', pl['g'])
    dev = launch(pl, pl['g'], mode)[0].cpu().numpy()
    hold(pl, mode, dev, exact, pl['root'], pl['slack'], pl['usable'], pl['fxy'], {s: which == k for k, s in enumerate(names)}, 'sweep')


def test_sweep_exercises_what_it_claims(plane):
    """More than half of interior, thick and ratio_rim lie in cells with a finite step budget; every border point outside the
    grid or in one of the two closed rings lies in a closed cell; the three modes did three different amounts of work."""
    pl = plane
    n = pl['n']
    for name in ('interior', 'thick', 'ratio_rim', 'corners0', 'corners1', 'edges'):
        need, inside = need_at(pl, pl['sets'][name]['fxy'])
        share = np.isfinite(need).mean()
        within = (need <= N_ITERS).mean()
        print(f'{pl["pair"]} {name}: {share:.3f} of the points in cells with finite need, {within:.3f} with need <= {N_ITERS}')
        if name in ('interior', 'thick', 'ratio_rim'):
            assert inside.all() and share > 0.5, f'{name}: only {share:.3f} of the points lie in open cells'
    b = pl['sets']['border']['fxy']
    need, inside = need_at(pl, b)
    ring = ~inside | np.any((b < 2.0) | (b >= n - 2.0), axis=1)
    assert ring.sum() > 1000 and np.all(np.isinf(need[ring]))
    steps = {mode: launch(pl, pl['g'], mode)[1]['pixel_iterations'] for mode in ('one', 'start', False)}
    print(f'{pl["pair"]} pixel_iterations {steps} on {len(pl["g"])} pixels')
    assert 0 < steps['one'] < steps['start'] < steps[False]


@pytest.fixture(scope='module')
def frontier(plane):
    """The open cells with a closed 8-neighbour (from the downloaded table), strided down to at most 3 000: one random point
    and the four corners of each, and their reference."""
    pl = plane
    n = pl['n']
    closed = np.pad(~np.isfinite(pl['need']), 1, mode='constant', constant_values=True)
    near = np.any([closed[1 + di:n + 1 + di, 1 + dj:n + 1 + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj], axis=0)
    cells = np.argwhere(~closed[1:-1, 1:-1] & near)
    assert len(cells) > 100
    cells = cells[::-(-len(cells) // 3000)]
    rng = np.random.default_rng(SEED + 2)
    w = np.concatenate([rng.random((len(cells), 1, 2)), np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]]).repeat(len(cells), 0)], axis=1)
    fxy = (cells[:, None, :] + w).reshape(-1, 2)
    g = pr.counts_of(pl['head'], fxy[:, 0], fxy[:, 1])
    root, slack, usable = pr.reference(g, pl['i0'], pl['mus'], screen=np.ones(len(g), bool))
    print(f'{pl["pair"]} frontier: {len(cells)} cells, {len(g)} points, {usable.mean():.3f} usable')
    return {'fxy': fxy, 'g': g, 'root': root, 'slack': slack, 'usable': usable}


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_frontier_between_open_and_closed_cells(plane, frontier, mode):
    f = frontier
    assert len(f['g']) <= 15000
    exact = exact_of(plane, 'frontier', f['g'])
    dev = launch(plane, f['g'], mode)[0].cpu().numpy()
    corner = np.tile(np.arange(5) > 0, len(f['g']) // 5)
    hold(plane, mode, dev, exact, f['root'], f['slack'], f['usable'], f['fxy'], {'frontier inside': ~corner, 'frontier corners': corner}, 'frontier')


def test_whole_tile_stores_and_stashed_pixels(plane):
    """The interior set as a ragged [view][channel][row] sinogram, results in the reference's order written by the kernel (whole
    tiles on the fast path, stashed pixels one by one): the same bits as the plain launch, permuted."""
    pl = plane
    s = pl['sets']['interior']['fxy']
    C, R = 67, 23
    V = -(-len(s) // (C * R))
    fxy = s[np.arange(V * C * R) % len(s)]
    g = torch.from_numpy(np.ascontiguousarray(pr.counts_of(pl['head'], fxy[:, 0], fxy[:, 1]).T)).cuda().reshape(2, V, C, R)
    plain, _ = launch(pl, (g[0], g[1]), 'one')
    got, _ = launch(pl, (g[0], g[1]), 'one', out_rc=(R, C))
    assert got.shape == (V, R, C, 2)
    assert torch.equal(got.view(torch.int64), plain.permute(0, 2, 1, 3).contiguous().view(torch.int64))


def test_float32_counts(hip):
    """The interior set of case 0 as float32 counts: the points move with the rounding, so the reference is that of the
    rounded counts."""
    from dex_ct_sim_amd import quadrature
    i0, mus = tables('case0')
    head = quadrature.newton_start_grid(i0, mus)['head']
    pl = {'pair': 'case0', 'i0': i0, 'mus': mus, 'head': head, 'cache': {}}
    s = pr.point_sets(head, SEED, cut=pr.DOMAIN_CUT['case0'])['interior']['fxy']
    g32 = pr.counts_of(pl['head'], s[:, 0], s[:, 1]).astype(np.float32)
    g = g32.astype(np.float64)
    fxy = np.stack(pr.plane_of(pl['head'], g), axis=1)
    assert np.abs(fxy - s).max() > 1e-6                                   # (they did move)
    root, slack, usable = pr.reference(g, pl['i0'], pl['mus'])
    assert usable.mean() > 0.99
    exact = exact_of(pl, 'float32', g32)
    for mode in MODES:
        dev = launch(pl, g32, mode)[0].cpu().numpy()
        hold(pl, mode, dev, exact, root, slack, usable, fxy, {'interior (float32 counts)': np.ones(len(g), bool)}, 'float32')
