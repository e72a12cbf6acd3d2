"""The census of the dedup route in its wide form (csrc/gn_dedup.hip gn_dedup_census_wide_kernel: float32 counts, rows a multiple
of 4, both sinograms aligned to 16 bytes - a lane loads four rows at once, the row before its first comes from the lane below,
the lanes' nibbles are OR-ed into the 64-bit words) and the cases that keep the loop of one row per lane.  The descriptor (use, F,
cap) must be gn_dedup_caps.device_expected's - F is the census' own count - and a_out the direct route's, byte for byte
(tests/gn_route_cases.py: guard bands, both fills, the diagnostic words):

  * rows 4 (the probe votes no: a fresh row 0 in every four), 60, 64, 68, 512 and 516 - one lane group short of a word, a word,
    a word and a nibble, two chunks of 256 rows, two chunks and a nibble - and 130 and 514, no multiples of 4: the old loop;
  * sinograms that start one float past a 16-byte boundary: the old loop, the same bytes;
  * a fresh pixel exactly at a row 4 l (it differs from the last row of the lane below only), at rows 63 | 64 (the words'
    boundary) and 255 | 256 (the chunks': the row before comes from the chunk before), and at the row after each;
  * a difference in the first sinogram only, and in the second only;
  * +0.0 next to -0.0: fresh (the comparison is of bit patterns); two equal NaN patterns: a repeat; two different ones: fresh;
  * float64 counts (the old loop), the same patterns.
"""
import numpy as np
import pytest
import torch

from gn_route_cases import host_fresh, route_equals_direct
from test_gpu_gn_dedup import LIGHT, pool, sinogram  # noqa: F401  (pool: the fixture)
from test_gpu_gn_dedup_passes import lines_of_fresh_rows

pytestmark = pytest.mark.gpu

WIDE_ROWS, OLD_ROWS = (60, 64, 68, 512, 516), (130, 514)


def shape_for(R):
    return (3, 33, R) if R >= 60 else (2, 128, R)


@pytest.mark.parametrize('R', WIDE_ROWS + OLD_ROWS + (4,))
def test_rows_around_the_wide_loads(hip, pool, R):
    V, C, _ = shape_for(R)
    for how, mask in (('one', False), ('pass0', True)):
        g = sinogram(pool, V, C, R, np.float32, patterns=LIGHT, seed=R)
        dd = route_equals_direct(hip, pool, g, how, mask)
        assert dd['use'] == (R != 4) and dd['F'] == (int(host_fresh(g).sum()) if R != 4 else 0), dd


@pytest.mark.parametrize('R', (64, 512, 516))
def test_one_float_past_a_16_byte_boundary(hip, pool, R):
    V, C, _ = shape_for(R)
    g = sinogram(pool, V, C, R, np.float32, patterns=LIGHT, seed=R + 1)
    flat = torch.empty(g.size + 8, dtype=torch.float32, device='cuda')
    assert flat.data_ptr() % 16 == 0
    t = flat[1:1 + g.size].view(g.shape)
    t.copy_(torch.from_numpy(g))
    assert t[0].data_ptr() % 16 == 4 and t[1].data_ptr() % 16 == 4
    assert route_equals_direct(hip, pool, g, 'one', False, use=1, t=t)['F'] == int(host_fresh(g).sum())


def edge_lines(pl, R, dtype):
    """[2][1][24][R]: fresh rows at the edges of the lanes' pieces, of the words and of the chunks; then the special lines."""
    sets = [[], [4], [8], [252], [256], [64], [63], [255], [3, 4], [5], [4, 5, 6, 7], [60], [63, 64], [255, 256], [256, 257], [R - 4], [R - 1], [1]]
    g = lines_of_fresh_rows(pl, sets + [[]] * 6, R, dtype)
    n = len(sets)
    other = g[:, 0, 1, 0].copy()                       # another pair of counts than line 0's
    g[0, 0, n, 256:] = other[0]                        # the first sinogram alone changes, at a chunk's first row
    g[1, 0, n + 1, 64:] = other[1]                     # the second alone, at a word's first row
    g[0, 0, n + 2, 7:] = other[0]                      # the first alone, at a lane's last row
    g[:, 0, n + 3, :] = 0.0
    g[0, 0, n + 3, 8:] = -0.0                          # +0.0 | -0.0 at a row 4 l
    g[1, 0, n + 3, 13:] = -0.0
    nan = np.array([0x7FC00000, 0x7FC00001] if dtype == np.float32 else [0x7FF8000000000000, 0x7FF8000000000001],
                   dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)
    g[:, 0, n + 4, :] = nan[0]                         # one NaN pattern all along: repeats
    g[:, 0, n + 5, :] = nan[0]
    g[1, 0, n + 5, 128:] = nan[1]                      # another pattern from row 128 on: fresh there
    fresh = host_fresh(g)[0]
    assert fresh[n].sum() == 2 and fresh[n, 256] and fresh[n + 1].sum() == 2 and fresh[n + 1, 64] and fresh[n + 2].sum() == 2 and fresh[n + 2, 7]
    assert fresh[n + 3].sum() == 3 and fresh[n + 3, 8] and fresh[n + 3, 13]
    assert fresh[n + 4].sum() == 1 and fresh[n + 5].sum() == 2 and fresh[n + 5, 128]
    return g


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_fresh_pixels_at_the_edges(hip, pool, dtype):
    for R in (512, 516):
        g = edge_lines(pool, R, dtype)
        for how, mask in (('one', False), ('pass0', False), ('one', True)):
            dd = route_equals_direct(hip, pool, g, how, mask, use=1)
            assert dd['F'] == int(host_fresh(g).sum())
