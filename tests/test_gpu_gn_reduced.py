"""The reduced residual rule on the device (csrc/gn.hip, gn_shortcut_kernel<1> with the block of dexct_gn_reduced_rows behind the
start array's power form; matdecomp.gn_device(reduced=...)), for the bundled 140 / 80 kV pair (golden case 0) and the Kramers
140 / 80 pair, on points of tests/gn_plane_refs.py - every 4th cell of the domain, the borders of the grid, the thick end and the
frontier between open and closed cells:

  * rule on, mode 'one': per component within the plane test's bound of the extended-precision root,
        |device - root| <= 1e-12 max(|root|, 1) + slack,   slack = |float64 oracle - root|;
  * last_gn_stats()['residual_energies'] is the rule's node count with the rule on and n_e with reduced=False;
  * reduced=False gives the bits of a start array without the block; pixels of closed cells and air pixels have the same bits
    on and off; guard bytes around the start array (the appended block is its end) and around the output stay as they were;
  * shapes: all points flat (an odd count), 64 * 3 + 5 pixels flat, [view][channel][row] sinograms written transposed with ragged
    (20 rows x 6 channels) and exact (16 x 4) tiles of 4 channels x 16 rows; float64 and float32 counts.

The largest difference between on and off is printed per launch (run with -s)."""
import numpy as np
import pytest
import torch

import gn_plane_refs as pr
from gn_plane_refs import SEED, tables
from guarded import Arena

pytestmark = pytest.mark.gpu

N_ITERS = 50
GUARD_BYTE = 0xA5


def launch(pl, g, shape=None, out_rc=None, mask=False, **kw):
    """One launch of mode 'one' on the counts g [n, 2] (host float64 / float32), given to the library as ``shape`` (default flat);
    the result lands in a guarded buffer.  -> (result [n, 2] in the order of the OUTPUT, last_gn_stats())."""
    from dex_ct_sim_amd import matdecomp as md
    t = torch.from_numpy(np.ascontiguousarray(g.T)).cuda()
    g0, g1 = (t[k].reshape(shape) if shape is not None else t[k] for k in (0, 1))
    n = g.shape[0]
    out = pl['arena'].alloc('out', 16 * n)
    out.fill(GUARD_BYTE)
    gmax = t[0].max().double() if mask else None
    a = md.gn_device(g0, g1, pl['i0'], pl['mus'], N_ITERS, 'f64', kernel=1, audit=0, two_level='one', out=out.view(torch.float64), out_rc=out_rc,
                     mask_max=gmax, **kw)
    st = md.last_gn_stats()
    assert st['mode'] == 'one'
    check_guards(pl)
    return a.cpu().numpy().reshape(-1, 2), st


def check_guards(pl):
    """The guards of the start array and of the last output are what they were, and no launch left a HIP error.  (The library's last
    HIP error is per thread and never cleared: an earlier test of the session that provoked a refusal on purpose leaves it set, so
    it is compared with the value the fixture started from, not with 0 as Arena.check would; every call is also checked by its
    return code.)"""
    pl['arena'].check()
    assert pl['lib'].dexct_last_hip_error() == pl['hip_error_before']


class start_array:
    """For the block: the gate of the pair hands out ``tensor`` as its start array."""

    def __init__(self, pl, tensor):
        self.gate, self.tensor = pl['gate'], tensor

    def __enter__(self):
        self.keep, self.gate['start'] = self.gate['start'], self.tensor

    def __exit__(self, *exc):
        self.gate['start'] = self.keep


@pytest.fixture(scope='module', params=['case0', 'kramers'])
def plane(hip, request):
    """Per table pair, once: the table with its rule (in a guarded buffer) and without, the points and their reference."""
    from dex_ct_sim_amd import matdecomp as md, quadrature
    i0, mus = tables(request.param)
    dev = torch.device('cuda', torch.cuda.current_device())
    gate = md._device_tables(i0, mus, dev, True)[2]
    info = gate['stats'].get('residual_rule')
    print(f'{request.param}: {info}')
    assert gate['start'] is not None and 'rule' in gate and info['installed'], info
    n = quadrature.GATE_CELLS
    _, c0, k0, _ = quadrature.start_layout(n)
    with_rule = gate['start']
    assert with_rule[10].item() == 3.0
    off = int(with_rule[11].item()) + quadrature.POWER_CELL * n * n
    block = with_rule[off:].cpu().numpy()
    assert int(block[0]) == info['nodes'] == len(gate['rule']['nodes']) and block.size == int(block[9]) == 16 + 14 * info['nodes']
    assert int(block[1] + block[3] + block[5]) == info['nodes']
    plain = with_rule[:off].clone()
    plain[10] = 2.0
    arena = Arena(dev, None)
    hip_error_before = hip.dexct_last_hip_error()
    arena.alloc('start', 8 * with_rule.numel()).put(with_rule)
    arena['start'].fill(GUARD_BYTE, inner=False)
    head = quadrature.newton_start_grid(i0, mus)['head']
    need = with_rule[c0:k0].cpu().numpy().reshape(n, n, 2)[:, :, 0]
    # every 4th cell (every other point of that set), the borders, the thick end, the frontier cells
    sets = pr.point_sets(head, SEED, (i0, mus), pr.DOMAIN_CUT.get(request.param))
    closed = np.pad(~np.isfinite(need), 1, mode='constant', constant_values=True)
    near = np.any([closed[1 + di:n + 1 + di, 1 + dj:n + 1 + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj], axis=0)
    cells = np.argwhere(~closed[1:-1, 1:-1] & near)
    cells = cells[::-(-len(cells) // 1000)]
    rng = np.random.default_rng(SEED + 3)
    parts = {'interior': sets['interior']['fxy'][::2], 'border': sets['border']['fxy'][::2], 'thick': sets['thick']['fxy'][::2],
             'frontier': cells + rng.random((len(cells), 2))}
    fxy = np.concatenate(list(parts.values()))
    which = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts.values())])
    if len(fxy) % 2 == 0:
        fxy, which = fxy[:-1], which[:-1]
    order = rng.permutation(len(fxy))
    fxy, which = fxy[order], which[order]
    g = pr.counts_of(head, fxy[:, 0], fxy[:, 1])
    root, slack, usable = pr.reference(g, i0, mus, screen=np.isin(which, (1, 3)))
    pl = {'pair': request.param, 'i0': i0, 'mus': mus, 'head': head, 'n': n, 'n_e': i0.shape[1], 'gate': gate, 'info': info, 'need': need,
          'plain': plain, 'guarded': arena['start'].view(torch.float64), 'arena': arena, 'names': list(parts), 'which': which, 'fxy': fxy,
          'g': g, 'root': root, 'slack': slack, 'usable': usable, 'lib': hip, 'hip_error_before': hip_error_before}
    print(f'{pl["pair"]}: {len(g)} points ' + ', '.join(f'{s} {int((which == k).sum())}' for k, s in enumerate(parts)) +
          f'; {usable.mean():.3f} usable; rule {info["nodes"]} of {pl["n_e"]} energies; last HIP error before: {hip_error_before}')
    return pl


def closed_of(pl, g):
    """Pixels whose counts (float64) fall in a closed cell or outside the grid: they never take the chord step.  (A point within
    1e-6 of a grid line counts only if the cells on both sides are closed: the device's logarithm may put it in either.)"""
    fx, fy = pr.plane_of(pl['head'], g)
    n = pl['n']
    out = np.ones(len(g), dtype=bool)
    for dx in (-1e-6, 0.0, 1e-6):
        for dy in (-1e-6, 0.0, 1e-6):
            x, y = fx + dx, fy + dy
            inside = np.isfinite(x) & np.isfinite(y) & (x >= 0.0) & (x < n) & (y >= 0.0) & (y < n)
            i, j = np.where(inside, x, 0).astype(np.int64), np.where(inside, y, 0).astype(np.int64)
            out &= ~inside | ~(pl['need'][i, j] <= N_ITERS)
    return out


def on_off_plain(pl, g, what, **kw):
    """The three launches on the same counts; the checks every shape shares.  -> (on, off)."""
    with start_array(pl, pl['guarded']):
        on, st_on = launch(pl, g, **kw)
        off, st_off = launch(pl, g, reduced=False, **kw)
    with start_array(pl, pl['plain']):
        plain, st_plain = launch(pl, g, **kw)
    print(f'{pl["pair"]} {what}: residual_energies on {st_on["residual_energies"]}, off {st_off["residual_energies"]}, without the block '
          f'{st_plain["residual_energies"]}; steps {st_on["pixel_iterations"]} / {st_off["pixel_iterations"]}')
    assert st_on['residual_energies'] == pl['info']['nodes'] < pl['n_e']
    assert st_off['residual_energies'] == pl['n_e'] == st_plain['residual_energies']
    assert np.array_equal(off.view(np.int64), plain.view(np.int64))
    with np.errstate(all='ignore'):
        d = np.abs(on - off) / np.maximum(np.abs(off), 1.0)
    both = np.isfinite(on).all(axis=1) & np.isfinite(off).all(axis=1)
    assert np.array_equal(np.isfinite(on), np.isfinite(off))
    print(f'{pl["pair"]} {what}: largest |on - off| / max(|off|, 1) = {d[both].max():.2e} over {both.sum()} of {len(g)} pixels, '
          f'{(on.view(np.int64) != off.view(np.int64)).any(axis=1).sum()} pixels differ in a bit')
    return on, off


def hold(pl, dev, root, slack, usable, what):
    scale = np.maximum(np.abs(root), 1.0)
    with np.errstate(all='ignore'):
        bound = 1e-12 * scale + slack
        err = np.abs(dev - root)
        over = usable[:, None] & ~(err <= bound)
    rel = (err[usable] / scale[usable]).max()
    margin = ((bound[usable] - err[usable]) / scale[usable]).min()
    print(f'{pl["pair"]} {what}: {usable.sum()} of {len(usable)} usable, max |device - root| / max(|root|, 1) = {rel:.2e}, least margin {margin:.2e}')
    assert not over.any(), (what, int(over.any(axis=1).sum()), float((err / bound)[over].max()))


def test_all_points_flat(plane):
    """Every point in one flat launch of an odd size: the bound with the rule on (and off), the row counts, the bits."""
    pl = plane
    assert len(pl['g']) % 2 == 1 and len(pl['g']) > 64 * 8
    on, off = on_off_plain(pl, pl['g'], 'all points')
    hold(pl, on, pl['root'], pl['slack'], pl['usable'], 'rule on')
    hold(pl, off, pl['root'], pl['slack'], pl['usable'], 'rule off')
    closed = closed_of(pl, pl['g'])
    took = (on.view(np.int64) != off.view(np.int64)).any(axis=1)
    print(f'{pl["pair"]}: {closed.sum()} pixels in closed cells, {took.sum()} pixels differ between on and off')
    assert closed.sum() > 500 and took.sum() > 500
    assert np.array_equal(on[closed].view(np.int64), off[closed].view(np.int64))
    for k, name in enumerate(pl['names']):
        m = (pl['which'] == k) & pl['usable']
        print(f'{pl["pair"]} {name}: {m.sum()} of {(pl["which"] == k).sum()} usable')
        assert m.sum() > 100 or name == 'border', name


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape,out_rc', [((64 * 3 + 5,), None), ((3, 6, 20), (20, 6)), ((3, 4, 16), (16, 4))], ids=['flat197', 'ragged20x6', 'exact16x4'])
def test_shapes_and_count_types(plane, shape, out_rc, dtype):
    """64 * 3 + 5 pixels flat, and sinograms [view][channel][row] written as [view][row][channel] by the kernel - tiles of 4 channels
    x 16 rows: ragged in both directions (6 x 20) and exact (4 x 16) - with the air mask on; float64 and float32 counts (the
    reference is that of the counts the kernel is given)."""
    pl = plane
    m = int(np.prod(shape))
    g = pl['g'][:m].astype(dtype)
    g64 = g.astype(np.float64)
    if dtype == np.float32:
        root, slack, usable = pr.reference(g64, pl['i0'], pl['mus'], screen=np.isin(pl['which'][:m], (1, 3)))
    else:
        root, slack, usable = pl['root'][:m], pl['slack'][:m], pl['usable'][:m]
    what = f'{"x".join(map(str, shape))} {np.dtype(dtype).name}'
    on, off = on_off_plain(pl, g, what, shape=shape, out_rc=out_rc, mask=True)
    if out_rc is not None:                                                # pixel (v, c, r) of the input went to [v][r][c]
        V, C, R = shape
        back = np.arange(m).reshape(V, R, C).transpose(0, 2, 1).ravel()
        on, off = on[back], off[back]
    air = g64[:, 0] >= 0.95 * g64[:, 0].max()
    closed = closed_of(pl, g64)
    print(f'{pl["pair"]} {what}: {air.sum()} air pixels, {closed.sum()} in closed cells')
    assert air.sum() >= 1 and np.all(on[air] == 0.0) and np.all(off[air] == 0.0)
    assert closed.sum() >= 10 and np.array_equal(on[closed].view(np.int64), off[closed].view(np.int64))
    hold(pl, on, root, slack, usable & ~air, f'{what} rule on')


def test_switches_of_the_rule(plane):
    """reduced=None and reduced=True are the same launch; the library refuses the flag of the full residual where there is no chord
    step and takes it with one."""
    from dex_ct_sim_amd import _native, matdecomp as md
    from dex_ct_sim_amd._device import ptr, stream_ptr
    pl = plane
    g = pl['g'][:197]
    with start_array(pl, pl['guarded']):
        a, st = launch(pl, g)
        b, st_b = launch(pl, g, reduced=True)
    assert st['residual_energies'] == st_b['residual_energies'] == pl['info']['nodes'] and np.array_equal(a.view(np.int64), b.view(np.int64))
    t = torch.from_numpy(np.ascontiguousarray(g.T)).cuda()
    i0_d, mus_d, _ = md._device_tables(pl['i0'], pl['mus'], t.device, False)
    out = torch.empty((197, 2), dtype=torch.float64, device=t.device)
    ws = torch.empty(hip_ws_bytes(pl), dtype=torch.uint8, device=t.device)
    call = lambda gn_pass, start, flags: _native.load().dexct_gn_decompose(
        ptr(t[0]), ptr(t[1]), 1, 197, ptr(i0_d), ptr(mus_d), pl['n_e'], 1, 1, N_ITERS, 0, 0, None, 0.95, ptr(out),
        _native.gn_options(1e-12, 0, 0, 1, gn_pass, None, start, flags), ptr(ws), stream_ptr())
    start = pl['guarded'].data_ptr()
    assert call(_native.GN_PASS_SHORTCUT, start, _native.GN_FLAG_FULL_RESIDUAL) == -1                       # no chord step: two-step mode
    assert call(0, None, _native.GN_FLAG_FULL_RESIDUAL) == -1
    assert call(_native.GN_PASS_SHORTCUT, start, _native.GN_FLAG_ONE_STEP | _native.GN_FLAG_FULL_RESIDUAL) == 0
    check_guards(pl)


def hip_ws_bytes(pl):
    from dex_ct_sim_amd import _native
    return _native.load().dexct_gn_workspace_bytes(pl['n_e'], 1)
