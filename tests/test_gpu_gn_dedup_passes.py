"""The passes around the Newton launches of dexct_gn_decompose_dedup (csrc/gn_dedup.hip) at the edges of their own tiling: the
gather's batches of lines (gn_dedup_index.h gather_batch_lines: the lines that share 256 bit words), the scan's blocks of 1024
lines, the expansion's tiles of channels x 64 rows.  As in tests/test_gpu_gn_dedup.py - whose sinograms, pool of counts and
``decompose`` these tests use - a_out must be the BYTES of the direct route (dexct_gn_decompose) of the same call, for float32
and float64 counts, with and without the mask, on the one-step short cut and on pass 0.

  * lines per batch: views {1, 3} x channels such that the line count is one below, at and one above a multiple of the batch,
    and a single line;
  * rows {1, 63, 64, 65, 130, 512} (one to eight bit words per line, the last one partial) x channels {1, 15, 16, 17, 31, 32, 33,
    67} (one below, at and one above the expansion's tile width, and the width it had before);
  * lines without a fresh pixel after row 0, a line fresh in every row within the capacity, fresh runs across a word boundary,
    more lines than a block of the scan takes, F = cap - 1, cap, cap + 1, and a sample that votes no;
  * guard bands around a_out and the dedup workspace, both pre-filled with 0x00 and with 0xFF.
"""
import numpy as np
import pytest
import torch

from guarded import Arena, twice
from test_gpu_gn_dedup import LIGHT, PASSES, decompose, expected, fresh_count, lines_with_fresh, pool, sinogram  # noqa: F401  (pool: the fixture)

pytestmark = pytest.mark.gpu

GATHER_WORDS, SCAN_BLOCK = 256, 1024          # gn_dedup_index.h kGatherWords, kScanBlock


def batch_lines(R):
    """gn_dedup_index.h gather_batch_lines"""
    return max(1, GATHER_WORDS // ((R + 63) // 64))


def same_bytes(pl, g, how, masks=(False, True), use=None):
    for mask in masks:
        want, _ = decompose(pl, g, how, mask, False)
        got, dd = decompose(pl, g, how, mask, True)
        assert dd == expected(g), (g.shape, dd, expected(g))
        if use is not None:
            assert dd['use'] == use, (g.shape, dd)
        assert np.array_equal(got, want), (g.shape, mask, dd)
    return dd


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
def test_line_counts_around_the_gathers_batch(pool, how, dtype):
    for R in (512, 130):
        b = batch_lines(R)
        assert b == {512: 32, 130: 85}[R]
        shapes = [(1, 1)] if R // 8 >= 64 else []            # a single line, where it has a list of one tile
        shapes += [(1, b - 1), (1, b), (1, b + 1)]
        shapes += [(3, C) for C in range(1, 2 * b) if (3 * C) % b in (b - 1, 0, 1)][:3]
        assert {(V * C) % b for V, C in shapes[-3:]} == {b - 1, 0, 1}
        for V, C in shapes:
            same_bytes(pool, sinogram(pool, V, C, R, dtype, patterns=LIGHT, seed=V + 10 * C + R), how, use=1)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
def test_rows_and_channels_around_the_expansions_tile(pool, how, dtype):
    used = 0
    for R in (1, 63, 64, 65, 130, 512):
        for C in (1, 15, 16, 17, 31, 32, 33, 67):
            V = 3 if (C + R) % 2 else 1
            if V * C * R // 8 < 64:
                continue                              # no list of even one tile: tests/test_gpu_gn_dedup.py has the plain call
            used += same_bytes(pool, sinogram(pool, V, C, R, dtype, patterns=LIGHT, seed=100 * C + R), how)['use']
    assert used >= 24
    # one row per line: every pixel is fresh, the census overflows the list
    assert same_bytes(pool, sinogram(pool, 3, 200, 1, dtype, patterns=LIGHT, seed=1), how)['use'] == 0


def lines_of_fresh_rows(pl, fresh_rows, R, dtype=np.float32):
    """[2][1][len(fresh_rows)][R]: line l is fresh in row 0 and in the rows fresh_rows[l], nowhere else."""
    live = pl['kinds']['live']
    g = np.empty((2, 1, len(fresh_rows), R), dtype=dtype)
    for l, rows in enumerate(fresh_rows):
        step = np.zeros(R, dtype=np.int64)
        step[np.array([r for r in rows if 0 < r < R], dtype=np.int64)] = 1
        g[:, 0, l, :] = pl['values'][live[(np.cumsum(step) + 7 * l) % len(live)]].T.astype(dtype)
    assert fresh_count(g) == sum(len({r for r in rows if 0 < r < R}) + 1 for rows in fresh_rows)
    return g


@pytest.mark.parametrize('how', list(PASSES))
def test_patterns_at_the_passes_edges(pool, how):
    every = range(512)
    cases = {
        # 16 lines of 512, cap = 1024; the sample is line 0
        'nothing fresh after row 0': (lines_of_fresh_rows(pool, [[]] * 16, 512), 1),
        'a line fresh in every row': (lines_of_fresh_rows(pool, [[], every, [], [5]] + [[]] * 12, 512), 1),
        'fresh runs across word boundaries': (lines_of_fresh_rows(pool, [[], range(60, 70), range(63, 65), [63], [64], range(120, 200), [511], range(448, 512)] + [[]] * 8, 512), 1),
        'the last word partial': (lines_of_fresh_rows(pool, [[], range(126, 130), [128], [129], [127, 128]] + [[]] * 11, 130), 1),
        # more lines than a block of the scan takes; 64 rows: 256 lines per batch of the gather
        'across the scan\'s block': (lines_of_fresh_rows(pool, [[l % 64] if l % 5 else range(1 + l % 3, 9) for l in range(SCAN_BLOCK + 7)], 64), 1),
        'F = cap - 1': (lines_with_fresh(pool, [64, 63, 64, 64], 512), 1),
        'F = cap': (lines_with_fresh(pool, [64, 64, 64, 64], 512), 1),
        'F = cap + 1': (lines_with_fresh(pool, [64, 64, 65, 64], 512), 0),
        'the sample votes no': (lines_with_fresh(pool, [64 if l % 64 == 0 else 1 for l in range(128)], 64), 0),
    }
    for name, (g, use) in cases.items():
        for dtype in (np.float32, np.float64):
            dd = same_bytes(pool, g.astype(dtype), how, use=use)
            print(f'{how} {name} {np.dtype(dtype).name}: {dd}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('how', list(PASSES))
def test_guards_and_previous_contents_across_batches(hip, pool, how, dtype):
    """3 x 33 x 130: 99 lines in batches of 85, two tiles of channels and a partial one, three bit words per line, the last partial."""
    from dex_ct_sim_amd import _native
    V, C, R = 3, 33, 130
    arena = Arena(torch.device('cuda', torch.cuda.current_device()), None)
    n = V * C * R
    out = arena.alloc('out', 16 * n)
    dws = arena.alloc('dedup', _native.load().dexct_gn_dedup_workspace_bytes(n, R, int(dtype == np.float64)))
    before = hip.dexct_last_hip_error()
    g = sinogram(pool, V, C, R, dtype, patterns=LIGHT, seed=11)
    for mask in (False, True):
        want, _ = decompose(pool, g, how, mask, False)
        seen = []
        got = twice(arena, lambda: seen.append(decompose(pool, g, how, mask, True, out=out.view(torch.float64, (V, R, C, 2)), dedup_workspace=dws.inner)[1]),
                    outputs=('out',), scratch=('dedup',))
        assert hip.dexct_last_hip_error() == before
        assert seen[0] == seen[1] == expected(g) and seen[0]['use'] == 1, seen
        assert np.array_equal(got['out'].view(np.int64).reshape(V, R, C, 2), want), mask
