"""gn_dedup_expand_kernel (csrc/gn_dedup.hip) on tiles without a fresh pixel: a tile of 32 channels x 64 rows in which no line has
a bit set holds, in every row, the last row of the tile before it.  A form of the kernel that stores such tiles from one
register per lane - no results loads, no LDS writes, none of the tile's barriers - was built, passed these tests and was taken
out again because the pass did not get faster (profiles/gn_route_streaming.md, section 3); the tests stay for the kernel as it
is and for whoever tries again.  a_out must be the direct route's, byte for byte (tests/gn_route_cases.py: guard bands, both
fills, the descriptor, the diagnostic words), with

  * rows 64 (one tile), 128, 130 (a last tile of two rows), 192, 512 and 4160 (65 tiles: past the reload of the bit words, which
    also renews the tiles' mask), channels 1, 31, 32, 33 and 67 (a ragged last column of 1 or 3 channels);
  * columns of three kinds, taking turns over the views and the columns of a view:
      single   every other tile behind the row-0 tile holds exactly ONE fresh bit - in one line, the others none: the line moves
               through the column's channels (its last real one included), the bit is 0, 63 or 31 - so runs of all-repeat tiles
               lie between fresh ones;
      early    fresh pixels in tile 1 only, and from four tiles on in the last tile too: a run of all-repeat tiles that ends the
               line (a partial tile where the rows are no multiple of 64) or lies between two fresh tiles;
      still    nothing fresh after row 0: every tile behind the row-0 tile repeats;
  * C = 67, R = 4160 once more with every position of the single line in a column of 32 and of 3 channels, for each of the
    three bits.

Every case asserts from a census on the host that it holds all-repeat tiles and ordinary ones (where there is more than one
tile of rows), and tiles with exactly one fresh bit.
"""
import numpy as np
import pytest

from gn_route_cases import host_fresh, route_equals_direct
from test_gpu_gn_dedup import pool  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TILE_C, TILE_R = 32, 64               # csrc/gn_dedup.hip kExpandC, kExpandR
ROWS, CHANNELS = (64, 128, 130, 192, 512, 4160), (1, 31, 32, 33, 67)
BITS = (0, 63, 31)


def columns(C):
    return [(cb, min(TILE_C, C - cb * TILE_C)) for cb in range((C + TILE_C - 1) // TILE_C)]


def mixed_rows(V, C, R):
    """fresh rows (behind row 0) per line, line = v * C + c"""
    tiles = (R + TILE_R - 1) // TILE_R
    rows = [[] for _ in range(V * C)]
    for v in range(V):
        for cb, nc in columns(C):
            first = v * C + cb * TILE_C
            kind = ('single', 'early', 'still')[(v + cb) % 3]
            if kind == 'single':
                for rb in range(1, tiles, 2):
                    rows[first + (rb // 2 + v) % nc].append(TILE_R * rb + BITS[(rb // 2 + v) % 3])
            elif kind == 'early' and tiles > 1:
                rows[first].append(TILE_R + 5)
                rows[first + nc - 1].append(2 * TILE_R - 1)
                if tiles >= 4:
                    rows[first + nc // 2].append(R - 1)
    return [[r for r in rr if r < R] for rr in rows]


def sweep_rows(V, C, R):
    """view v: tile rb of every column holds the one bit BITS[v] in the column's line (rb - 1) % nc, every third tile none"""
    tiles = (R + TILE_R - 1) // TILE_R
    rows = [[] for _ in range(V * C)]
    for v in range(V):
        for cb, nc in columns(C):
            k = 0
            for rb in range(1, tiles):
                if rb % 3 == 0:
                    continue
                rows[v * C + cb * TILE_C + k % nc].append(TILE_R * rb + BITS[v])
                k += 1
            assert k >= nc                         # (every position of the column's line was taken)
    return rows


def build(pl, V, C, R, rows):
    live = pl['kinds']['live']
    g = np.empty((2, V * C, R), dtype=np.float32)
    for l, rr in enumerate(rows):
        step = np.zeros(R, dtype=np.int64)
        step[np.array(sorted(set(rr)), dtype=np.int64)] = 1
        g[:, l, :] = pl['values'][live[(np.cumsum(step) + 7 * l) % len(live)]].T.astype(np.float32)
    return g.reshape(2, V, C, R)


def tile_census(g):
    """fresh bits per tile [V][column][tile of rows]"""
    _, V, C, R = g.shape
    fresh = host_fresh(g)
    tiles, cols = (R + TILE_R - 1) // TILE_R, (C + TILE_C - 1) // TILE_C
    padded = np.zeros((V, cols * TILE_C, tiles * TILE_R), dtype=np.int64)
    padded[:, :C, :R] = fresh
    return padded.reshape(V, cols, TILE_C, tiles, TILE_R).sum(axis=(2, 4))


def check(hip, pl, V, C, R, rows, how='one', mask=False):
    g = build(pl, V, C, R, rows)
    per_tile = tile_census(g)
    assert (per_tile[:, :, 0] >= 1).all()                       # the row-0 tile never repeats
    if R > TILE_R:
        assert (per_tile == 0).any() and (per_tile[:, :, 1:] > 0).any() and (per_tile[:, :, 1:] == 1).any(), (V, C, R)
    assert route_equals_direct(hip, pl, g, how, mask, use=1)['F'] == int(per_tile.sum())
    return per_tile


@pytest.mark.parametrize('R', ROWS)
def test_all_repeat_tiles(hip, pool, R):
    for C in CHANNELS:
        V = max(3, -(-512 // (C * R)))                          # (the route needs a list of one tile: 512 pixels)
        check(hip, pool, V, C, R, mixed_rows(V, C, R))


def test_the_single_fresh_line_at_every_position(hip, pool):
    V, C, R = 3, 67, 4160
    per_tile = check(hip, pool, V, C, R, sweep_rows(V, C, R))
    assert (per_tile[:, :, 1:] <= 1).all() and (per_tile[:, 2, 1:] == 1).sum() >= 3 * 3


def test_pass_0_and_the_mask(hip, pool):
    for how, mask in (('pass0', False), ('one', True), ('two', False)):
        check(hip, pool, 3, 67, 192, mixed_rows(3, 67, 192), how, mask)
