"""The passes of dexct_gn_decompose_dedup (csrc/gn_dedup.hip) past one trip of their capped grids and past the wraps of their bit
words - the shapes, constants and host model of tests/gn_dedup_caps.py, whose CPU self-test (tests/test_gn_dedup_caps.py) shows
that on these shapes a pass that stops after a trip, or runs its later trips one work item late, changes the descriptor or some
pixel's result, whether the buffers held 0x00 or 0xFF.

The oracle is that of tests/test_gpu_gn_dedup.py: a_out of gn_device(dedup=True) must be the BYTES of dedup=False (the direct
route, which the other suites pin to the CPU oracle) on the same inputs, last_gn_stats()['dedup'] must be what the rules of
include/dexct_gn_dedup.h give for the inputs, and after a list-route call the finished-pixel word of the Newton workspace is n_pix (the
expansion adds to it per column).  a_out and the dedup workspace lie between guards and are pre-filled with 0x00 and with 0xFF.

The large shapes (2.1e7 to 3.4e7 pixels) are generated and compared on the device.  Line l repeats pairs of counts of the pool's
points inside the short cut's table: pair (l + 7 run) % 457 in its run-th fresh run, g2 advanced by l // 457 ulps, so that every
line of the call has bits of its own; before the comparison the direct route's results of line l are shown to differ from those
of line l +- W for every distance W at which a wrong trip or a late work item would read (gn_dedup_caps.confused_line_offsets).

Measured on an MI355X (wall time per test: generation, the direct call, both fills and the comparisons): the first large case 1.9 s
(it builds the pool and the short cut's table), every other large case under 0.1 s, each of the small-shape tests 0.2 s.
"""
import time

import numpy as np
import pytest
import torch

import gn_dedup_caps as dc
from guarded import Arena, twice
from test_gpu_gn_dedup import LIGHT, N_ITERS, PASSES, decompose, expected, pool, sinogram  # noqa: F401  (pool: the fixture)
from test_gpu_gn_dedup_passes import lines_of_fresh_rows, same_bytes

pytestmark = pytest.mark.gpu

OFF_TABLE = 60                 # the pool's last live points: 20 thin, 20 thick, 20 photon-starved (tests/test_gpu_gn_dedup.py pool)


def inside_points(pl):
    live = pl['values'][pl['kinds']['live']]
    pts = live[:len(live) - OFF_TABLE][:dc.KEY_POOL]
    assert len(pts) == dc.KEY_POOL and float(pts.max()) < 0.5 * pl['air_count']
    return pts


def large_counts(pl, case, dtype):
    """-> (g [2][V][C][R] on the device, the fresh pixels the case asked for [L][R])"""
    V, C, R = case.shape
    l, r = dc.grid_lr(V, C, R, xp=torch, device='cuda', dtype=torch.int64)
    step = case.step(l, r) & (r >= 1)
    idx = (l + dc.KEY_STRIDE * torch.cumsum(step, dim=1)) % dc.KEY_POOL
    pts = torch.from_numpy(inside_points(pl).astype(np.float32 if dtype == torch.float32 else np.float64)).cuda()
    as_int = torch.int32 if dtype == torch.float32 else torch.int64
    g = torch.empty((2, V * C, R), dtype=dtype, device='cuda')
    g[0] = pts[:, 0].contiguous()[idx]
    g[1] = (pts[:, 1].contiguous().view(as_int)[idx] + (l // dc.KEY_POOL).to(as_int)).view(dtype)
    step[:, 0] = True
    return g.view(2, V, C, R), step


def assert_same_bytes(got, want, what):
    a, b = got.view(torch.int64), want.view(torch.int64)
    if torch.equal(a, b):
        return
    bad = (a != b).any(dim=-1)                               # [V][R][C]
    i = int(torch.nonzero(bad.reshape(-1))[0])
    (V, R, C), n = bad.shape, int(bad.sum())
    v, r, c = i // (R * C), i // C % R, i % C
    raise AssertionError(f'{what}: {n} of {bad.numel()} pixels differ from the direct route, the first at (view {v}, row {r}, channel {c}) = '
                         f'line {v * C + c}: {a[v, r, c].tolist()} for {b[v, r, c].tolist()}')


def lines_differ(want, shape, allowed):
    """The direct route's results of line l against those of line l + W, for every W a mutant confuses: (pairs, equal pairs)."""
    V, C, R = shape
    lines = want.view(torch.int64).view(V, R, C, 2).permute(0, 2, 1, 3).reshape(V * C, 2 * R)
    pairs = equal = 0
    for W in dc.confused_line_offsets(V, C, R):
        same = int((lines[W:] == lines[:-W]).all(dim=1).sum())
        assert same <= allowed * (V * C - W), f'lines {W} apart: {same} of {V * C - W} pairs have equal results'
        pairs, equal = pairs + V * C - W, equal + same
    return pairs, equal


def run_large(hip, pl, name, how, mask, dtype=torch.float32):
    from dex_ct_sim_amd import _native, matdecomp as md
    t0 = time.perf_counter()
    case = dc.LARGE[name]
    V, C, R = case.shape
    n = V * C * R
    g, asked = large_counts(pl, case, dtype)
    assert torch.equal(dc.device_fresh(g).reshape(V * C, R), asked)           # the bits are the pattern the host model was run on
    want_dd = dc.device_expected(g)
    del asked
    sample = int(dc.device_fresh(g).reshape(V * C, R)[::dc.K('kProbeStride')].sum())
    votes_yes = sample * dc.K('kUseShare') <= dc.ceil_div(V * C, dc.K('kProbeStride')) * R
    assert want_dd['use'] == case.use and votes_yes == (name not in dc.VOTES_NO), (want_dd, sample)
    if case.use:
        assert want_dd['F'] <= want_dd['cap'] and want_dd['F'] % dc.K('kTile') != 0
    if name == 'A-over':
        assert want_dd['F'] == want_dd['cap'] + 1
    gmax = torch.tensor(pl['air_count'], dtype=torch.float64, device='cuda') if mask else None
    kw = dict(kernel=1, audit=0, out_rc=(R, C), mask_max=gmax, **PASSES[how])
    want = md.gn_device(g[0], g[1], pl['i0'], pl['mus'], N_ITERS, 'f64', dedup=False, **kw)
    assert md.last_gn_stats()['dedup'] is None
    pairs, equal = lines_differ(want, case.shape, 0.0 if dtype == torch.float32 else 1e-3)
    arena = Arena(torch.device('cuda', torch.cuda.current_device()), None)
    out = arena.alloc('out', 16 * n)
    dws = arena.alloc('dedup', _native.load().dexct_gn_dedup_workspace_bytes(n, R, int(dtype == torch.float64)))
    before = hip.dexct_last_hip_error()
    for fill in (0x00, 0xFF):
        arena.fill(fill, inner=('out', 'dedup'))
        got = md.gn_device(g[0], g[1], pl['i0'], pl['mus'], N_ITERS, 'f64', out=out.view(torch.float64, (V, R, C, 2)), dedup=True,
                           dedup_workspace=dws.inner, **kw)
        st = md.last_gn_stats()
        arena.check()
        assert hip.dexct_last_hip_error() == before
        progress = int(md._last_run.workspaces[-1][_native.GN_WS_PROGRESS:_native.GN_WS_PROGRESS + 8].view(torch.int64))
        assert st['mode'] == ('one' if how == 'one' else 'single')
        assert st['dedup'] == want_dd, (name, fill, st['dedup'], want_dd)
        if want_dd['use']:
            assert progress == n, (progress, n)
        assert_same_bytes(got, want, f'{name} {how} mask={mask} fill=0x{fill:02x}')
    torch.cuda.synchronize()
    print(f'{name} {how} mask={mask} {dtype}: {V} x {C} x {R} = {n} pixels, descriptor {want_dd}, progress {progress}, trips '
          f'{dc.all_trips(V, C, R)}, {equal} of {pairs} confusable line pairs equal, {time.perf_counter() - t0:.1f} s')
    for p, kind in case.mutants():
        assert dc.trips(p, V, C, R) > 1, (name, p)


@pytest.mark.parametrize('mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('how', list(PASSES))
def test_a_every_pass_past_its_first_trip(hip, pool, how, mask):
    """1000 x 1311 x 16: the probe's trip 2 (20 485 words: some waves carry two valid unrolled items, others one and clamped ones),
    the scan's trip 2 (1 281 block sums), the gather's trip 3 (5 122 batches, the last of 24 lines), 161 trips of the census, 21 of
    the expansion (41 000 columns, the last tile of channels ragged)."""
    run_large(hip, pool, 'A', how, mask)


@pytest.mark.parametrize('name', ['A-no', 'A-edge', 'A-over'])
def test_a_votes_and_overflow_decided_beyond_the_first_trip(hip, pool, name):
    """A-no: the lines the probe's first trip samples repeat, those of its trip 2 are fresh in every row - the vote is no.  A-edge:
    the sample is one pixel over 1 / 8, and the first word of trip 2 holds more than that one.  A-over: F = cap + 1 through the
    lines whose block sums reach F only through the scan's carry.  use == 0 each time, and the direct launch's bytes."""
    run_large(hip, pool, name, 'one', False)


@pytest.mark.parametrize('name,mask', [('B', True), ('B-edge', False)])
def test_b_third_trips_of_probe_and_scan(hip, pool, name, mask):
    """1000 x 2101 x 16: the probe's trip 3 (61 words) and the scan's (4 block sums).  A vote of yes cannot depend on the probe's
    last words; in B-edge the sample is one pixel over 1 / 8 and the first word of trip 3 holds more than that one: use == 0."""
    run_large(hip, pool, name, 'one', mask)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_c_batches_of_multi_word_lines_past_the_gathers_grid(hip, pool, dtype):
    """530 x 331 x 130: the gather's trip 2 with batches of 85 lines of three words (2 064 batches, the last of 75 lines), three
    trips of the expansion (5 830 columns), 22 of the census; fresh runs across the word boundaries.  float64: lines 457 apart
    differ by ulps of their g2 alone, and at most 0.1 % of the confusable pairs may have equal results."""
    run_large(hip, pool, 'C', 'one', False, dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
@pytest.mark.parametrize('target', ['expand_reload', 'gather_chunk'])
def test_small_shapes_past_the_word_wraps(hip, pool, target, how, dtype):
    """expand_reload: R in (4096, 4097, 4160, 8193) x C in (1, 33) - the expansion reloads a line's bit words into its registers
    after word 63 and word_of_lane wraps; before[] carries across.  gather_chunk: R in (16384, 16385, 16450, 32769) x C = 3 x V in
    (1, 2) - a line is a batch by itself, in one, two (the second of one word) and three chunks of 256 words.  Fresh rows at the
    boundaries (gn_dedup_caps.reload_rows / chunk_rows) through lines_of_fresh_rows, guarded and pre-filled buffers; and the
    suites' random LIGHT sinograms of the same shapes through same_bytes."""
    from dex_ct_sim_amd import _native
    t0 = time.perf_counter()
    arena_dev = torch.device('cuda', torch.cuda.current_device())
    for name, (what, (V, C, R), rows) in dc.SMALL.items():
        if what != target:
            continue
        s = dc.small_sinogram(V, C, R, rows)
        g = lines_of_fresh_rows(pool, rows, R, dtype).reshape(2, V, C, R)
        use, F, cap = s.expected()
        want_dd = {'use': use, 'F': F, 'cap': cap, 'launches': 1}
        assert expected(g) == want_dd and use == 1
        assert same_bytes(pool, g, how, use=1) == want_dd
        arena = Arena(arena_dev, None)
        n = V * C * R
        out = arena.alloc('out', 16 * n)
        dws = arena.alloc('dedup', _native.load().dexct_gn_dedup_workspace_bytes(n, R, int(dtype == np.float64)))
        before = hip.dexct_last_hip_error()
        for mask in (False, True):
            want, _ = decompose(pool, g, how, mask, False)
            seen = []
            got = twice(arena, lambda: seen.append(decompose(pool, g, how, mask, True, out=out.view(torch.float64, (V, R, C, 2)), dedup_workspace=dws.inner)[1]),
                        outputs=('out',), scratch=('dedup',))
            assert hip.dexct_last_hip_error() == before
            assert seen[0] == seen[1] == want_dd, (name, seen)
            assert np.array_equal(got['out'].view(np.int64).reshape(V, R, C, 2), want), (name, mask)
        dd = same_bytes(pool, sinogram(pool, V, C, R, dtype, patterns=LIGHT, seed=R + C + V), how)
        print(f'{name} {how} {np.dtype(dtype).name}: descriptor {want_dd}, random lines {dd}, trips {dc.all_trips(V, C, R)}')
    print(f'{target} {how} {np.dtype(dtype).name}: {time.perf_counter() - t0:.1f} s')
