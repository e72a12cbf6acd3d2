"""dexct_gn_decompose_dedup (csrc/gn_dedup.hip; matdecomp.gn_device(dedup=True)) against the direct route of the same call
(dedup=False, which the other suites pin to the CPU oracle): the results must be the same BYTES.

Sinograms are built line by line ([view][channel][row], a line = the rows of one channel) from a pool of distinct pairs of
counts for the tables of golden case 0 - points inside the short cut's table, points outside its cells (thinner and thicker
than the grid: the stash and the general iteration), photon-starved counts, air (masked when a mask is given), +0.0, -0.0 and
NaN - in row patterns: all rows equal, all rows different, runs of random length, a repeat of g1 whose g2 differs in the last
bit, a masked run between live runs, runs of zeros of both signs and of NaN.

  * every shape of views {1, 3} x channels {1, 4, 5, 67} x rows {1, 15, 16, 17, 64, 65, 130, 512}, float32 and float64 counts, with
    and without the mask, the one-step short cut and pass 0 (the lane kernel);
  * the list exactly full (F = cap) and one over (F = cap + 1: the direct launch); a sample that votes for the list while the
    census overflows; a sample that votes against it on an input that repeats everywhere else; last_gn_stats()['dedup'] says
    which route ran;
  * guard bands around out_a and the dedup workspace, and the same bytes whether the workspace and out_a held 0x00 or 0xFF.
"""
import numpy as np
import pytest
import torch

import gn_plane_refs as pr
from guarded import Arena, twice

pytestmark = pytest.mark.gpu

N_ITERS = 50
VIEWS, CHANNELS, ROWS = (1, 3), (1, 4, 5, 67), (1, 15, 16, 17, 64, 65, 130, 512)
PROBE_STRIDE = 64             # gn_dedup_index.h kProbeStride
PASSES = {'one': dict(two_level='one'), 'pass0': dict(two_level=False)}


@pytest.fixture(scope='module')
def pool(hip):
    """The pairs of counts the lines are made of: (values [n, 2] float64, all distinct as float32 too; the air count; indices by
    kind)."""
    from dex_ct_sim_amd import quadrature
    i0, mus = pr.tables('case0')
    head = quadrature.newton_start_grid(i0, mus)['head']
    n = int(head[3])
    rng = np.random.default_rng(pr.SEED + 41)
    lo, hi, j_lo, _ = pr.domain(head, pr.DOMAIN_CUT['case0'])
    inside = pr.counts_of(head, rng.uniform(lo, min(hi, 300), 600), rng.uniform(j_lo + 1, 0.5 * n, 600))
    thin = pr.counts_of(head, rng.uniform(-6.0, -0.5, 20), rng.uniform(j_lo + 1, 0.5 * n, 20))          # left of the grid
    thick = pr.counts_of(head, rng.uniform(n + 0.5, n + 3.0, 20), rng.uniform(j_lo + 1, 0.5 * n, 20))   # right of it
    starved = np.stack([rng.uniform(1e-12, 1e-3, 20), rng.uniform(1e-12, 1e-3, 20)], axis=-1)
    live = np.concatenate([inside, thin, thick, starved])
    live = live[np.isfinite(live).all(axis=1) & (live > 0).all(axis=1)]
    _, first = np.unique(live.astype(np.float32), axis=0, return_index=True)          # distinct in either type
    live = live[np.sort(first)]
    air_count = 4.0 * float(live[:, 0].max())
    air = np.stack([air_count * rng.uniform(0.96, 1.0, 8), air_count * rng.uniform(0.5, 1.0, 8)], axis=-1)
    odd = np.array([[0.0, 0.0], [-0.0, -0.0], [0.0, -0.0], [np.nan, np.nan], [np.nan, 1.0], [1.0, np.nan]])
    values = np.concatenate([live, air, odd])
    kinds = {'live': np.arange(len(live)), 'air': len(live) + np.arange(len(air)), 'odd': len(live) + len(air) + np.arange(len(odd))}
    assert len(live) > 520
    return {'i0': i0, 'mus': mus, 'values': values, 'air_count': air_count, 'kinds': kinds, 'rng_seed': pr.SEED + 43}


def line_of(pl, pattern, R, rng):
    """Indices into the pool for the R rows of one line."""
    live, air, odd = (pl['kinds'][k] for k in ('live', 'air', 'odd'))
    if pattern == 'equal':
        return np.full(R, rng.choice(live))
    if pattern == 'different':
        return rng.permutation(live)[:R] if R <= len(live) else live[np.arange(R) % len(live)]
    if pattern == 'runs':
        out = []
        while len(out) < R:
            out += [rng.choice(live)] * int(rng.integers(1, 40))
        return np.array(out[:R])
    if pattern == 'masked':                       # live run, air run, live run
        a, b = sorted(rng.integers(0, R + 1, 2))
        out = np.full(R, rng.choice(live))
        out[a:b] = rng.choice(air)
        out[b:] = rng.choice(live)
        return out
    if pattern == 'odd':                          # runs of zeros of both signs and of NaN between live runs
        out = []
        while len(out) < R:
            out += [rng.choice(odd if rng.random() < 0.6 else live)] * int(rng.integers(1, 6))
        return np.array(out[:R])
    raise ValueError(pattern)


PATTERNS = ('equal', 'runs', 'masked', 'odd', 'equal', 'lastbit', 'different', 'runs')
LIGHT = ('equal', 'runs', 'masked', 'equal')          # few fresh pixels: the list route where the lines are long enough


def sinogram(pl, V, C, R, dtype, patterns=PATTERNS, seed=0):
    """Counts [2][V][C][R] of ``dtype``: line l follows patterns[l % len(patterns)].  'lastbit': runs whose second half repeats g1
    and has g2 one ulp (of ``dtype``) up - fresh, though g1 repeats."""
    rng = np.random.default_rng(pl['rng_seed'] + seed)
    g = np.empty((2, V * C, R), dtype=dtype)
    for l in range(V * C):
        p = patterns[l % len(patterns)]
        idx = line_of(pl, 'runs' if p == 'lastbit' else p, R, rng)
        g[:, l, :] = pl['values'][idx].T.astype(dtype)
        if p == 'lastbit':
            for r in range(1, R, 2):
                g[0, l, r] = g[0, l, r - 1]
                g[1, l, r] = np.nextafter(g[1, l, r - 1], dtype(np.inf))
    return g.reshape(2, V, C, R)


def fresh_count(g):
    """The census on the host: pixels whose bits differ from the row before (row 0 always)."""
    bits = g.view(np.uint32 if g.dtype == np.float32 else np.uint64)
    differ = (bits[:, ..., 1:] != bits[:, ..., :-1]).any(axis=0)
    return int(differ.sum()) + int(np.prod(g.shape[1:-1]))


def expected(g):
    """What the descriptor must say, from the rules of include/dexct_gn_dedup.h on the host: the probe's vote on every 64th line, then
    the census against the capacity."""
    lines = g.reshape(2, -1, g.shape[-1])
    cap = lines[0].size // 8 // 64 * 64
    sample = lines[:, ::PROBE_STRIDE]
    if fresh_count(sample) * 8 > sample[0].size:
        return {'use': 0, 'F': 0, 'cap': cap, 'launches': 1}
    n_fresh = fresh_count(lines)
    return {'use': int(n_fresh <= cap), 'F': n_fresh, 'cap': cap, 'launches': 1}


def decompose(pl, g, how, mask, dedup, out=None, dedup_workspace=None):
    """gn_device on the sinograms g [2][V][C][R] -> (bytes of a_out as int64 [V, R, C, 2], last_gn_stats()['dedup'])."""
    from dex_ct_sim_amd import matdecomp as md
    t = torch.from_numpy(g).cuda()
    V, C, R = g.shape[1:]
    gmax = torch.tensor(pl['air_count'], dtype=torch.float64, device='cuda') if mask else None
    a = md.gn_device(t[0], t[1], pl['i0'], pl['mus'], N_ITERS, 'f64', kernel=1, audit=0, out_rc=(R, C), mask_max=gmax, out=out, dedup=dedup,
                     dedup_workspace=dedup_workspace, **PASSES[how])
    st = md.last_gn_stats()
    assert st['mode'] == ('one' if how == 'one' else 'single')
    decompose.steps = st['pixel_iterations']
    return a.view(torch.int64).cpu().numpy().reshape(V, R, C, 2), st['dedup']


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
def test_every_shape_is_byte_identical(pool, how, dtype):
    routes = {'list': 0, 'direct': 0, 'none': 0}
    for V in VIEWS:
        for C in CHANNELS:
            for R in ROWS:
                g = sinogram(pool, V, C, R, dtype, patterns=PATTERNS if (V + C + R) % 3 == 0 else LIGHT, seed=1000 * V + 10 * C + R)
                for mask in (False, True):
                    want, none = decompose(pool, g, how, mask, False)
                    got, dd = decompose(pool, g, how, mask, True)
                    assert none is None
                    assert np.array_equal(got, want), (V, C, R, mask, dd)
                    if dd is None:
                        assert V * C * R // 8 < 64          # no list of even one tile: the library's plain call
                        routes['none'] += 1
                    else:
                        assert dd == expected(g), (V, C, R, dd, expected(g))
                        routes['list' if dd['use'] else 'direct'] += 1
    print(f'{how} {np.dtype(dtype).name}: {routes}')
    assert routes['list'] >= 16 and routes['direct'] >= 10 and routes['none'] >= 10


@pytest.mark.parametrize('how', list(PASSES))
def test_row_patterns(pool, how):
    """Each pattern by itself over all lines of a 3 x 5 x 130 scan (ragged in both directions), and all of them mixed; the masked
    pixels are exact zeros, the all-different lines overflow the list (the direct launch after the census)."""
    for p in ('equal', 'runs', 'masked', 'odd', 'lastbit', 'different', 'mixed'):
        g = sinogram(pool, 3, 5, 130, np.float64, patterns=PATTERNS if p == 'mixed' else (p,), seed=7)
        want, _ = decompose(pool, g, how, True, False)
        steps_direct = decompose.steps
        got, dd = decompose(pool, g, how, True, True)
        print(f'{how} {p}: {dd}; executed steps {steps_direct} direct, {decompose.steps} here')
        if p == 'runs':
            # pixels of the pool leave the one-step fast path (the stash and the general iteration: more than one step per
            # pixel on the direct route), and the list route runs the steps of every distinct pixel once - those of 97 entries
            # and at most 63 pads instead of 1950 pixels
            assert steps_direct > 3 * 5 * 130 and decompose.steps < steps_direct
        assert np.array_equal(got, want), p
        assert dd == expected(g), (p, dd, expected(g))
        assert dd['use'] == (p in ('equal', 'runs', 'masked')), (p, dd)
        if p == 'masked':
            air = np.moveaxis(g[0], 1, 2) >= 0.95 * pool['air_count']              # [V][R][C]
            assert air.sum() > 50 and not want[air].any() and want[~air].all(axis=-1).any()
        if p == 'lastbit':
            assert fresh_count(g) == 3 * 5 * 130                                   # every one of those pixels is fresh


def lines_with_fresh(pool, per_line, R, dtype=np.float32):
    """[2][1][len(per_line)][R]: line l has exactly per_line[l] fresh pixels (runs of equal length, the remainder in the last)."""
    live = pool['kinds']['live']
    g = np.empty((2, 1, len(per_line), R), dtype=dtype)
    for l, f in enumerate(per_line):
        idx = live[(np.minimum(np.arange(R) * f // R, f - 1) + 7 * l) % len(live)]
        g[:, 0, l, :] = pool['values'][idx].T.astype(dtype)
    assert fresh_count(g) == sum(per_line)
    return g


@pytest.mark.parametrize('how', list(PASSES))
def test_capacity_and_probe_boundaries(pool, how):
    cases = {
        # 4 lines of 512: cap = 256; the probe reads line 0 (64 of 512 fresh: exactly 1 / 8)
        'F = cap': (lines_with_fresh(pool, [64, 64, 64, 64], 512), 1, 256, 256),
        'F = cap + 1': (lines_with_fresh(pool, [64, 64, 65, 64], 512), 0, 257, 256),
        'F = cap - 1': (lines_with_fresh(pool, [64, 63, 64, 64], 512), 1, 255, 256),
        'F = 1 mod 64': (lines_with_fresh(pool, [64, 1, 1, 63], 512), 1, 129, 256),
        # 128 lines of 64: cap = 1024; the probe reads lines 0 and 64
        'sample says yes, census overflows': (lines_with_fresh(pool, [1 if l % 64 == 0 else 64 for l in range(128)], 64), 0, 2 + 126 * 64, 1024),
        'sample says no, the rest repeats': (lines_with_fresh(pool, [64 if l % 64 == 0 else 1 for l in range(128)], 64), 0, 0, 1024),
        'sample at the limit': (lines_with_fresh(pool, [8 if l % 64 == 0 else 1 for l in range(128)], 64), 1, 16 + 126, 1024),
        'sample one over the limit': (lines_with_fresh(pool, [9 if l == 0 else 8 if l == 64 else 1 for l in range(128)], 64), 0, 0, 1024),
    }
    for name, (g, use, n_fresh, cap) in cases.items():
        for mask in (False, True):
            want, _ = decompose(pool, g, how, mask, False)
            got, dd = decompose(pool, g, how, mask, True)
            assert dd == {'use': use, 'F': n_fresh, 'cap': cap, 'launches': 1}, (name, dd)
            assert np.array_equal(got, want), name


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
def test_guard_bands_and_previous_contents(hip, pool, how, dtype):
    """out_a and the dedup workspace between guards; the workspace and out_a pre-filled with 0x00 and with 0xFF: the same bytes,
    those of the direct route, and no guard byte touched - on the list route, on the overflow after the census and on a sample
    that says no."""
    from dex_ct_sim_amd import _native
    V, C, R = 3, 5, 130
    inputs = {'list': sinogram(pool, V, C, R, dtype, patterns=('equal', 'runs', 'masked'), seed=3),
              'overflow': sinogram(pool, V, C, R, dtype, patterns=('equal',) + ('different',) * 15, seed=4),
              'no': sinogram(pool, V, C, R, dtype, patterns=('different',), seed=5)}
    arena = Arena(torch.device('cuda', torch.cuda.current_device()), None)
    n = V * C * R
    out = arena.alloc('out', 16 * n)
    dws = arena.alloc('dedup', _native.load().dexct_gn_dedup_workspace_bytes(n, R, int(dtype == np.float64)))
    before = hip.dexct_last_hip_error()
    for name, g in inputs.items():
        want, _ = decompose(pool, g, how, True, False)
        seen = []
        got = twice(arena, lambda: seen.append(decompose(pool, g, how, True, True, out=out.view(torch.float64, (V, R, C, 2)), dedup_workspace=dws.inner)[1]),
                    outputs=('out',), scratch=('dedup',))
        assert hip.dexct_last_hip_error() == before
        assert seen[0] == seen[1] and seen[0]['use'] == (name == 'list'), (name, seen)
        assert np.array_equal(got['out'].view(np.int64).reshape(V, R, C, 2), want), name
