"""rows16_kernel's narrow list rounds (csrc/dedup_index.h: round_rows; DEXCT_DET_DEDUP = 1) on the device: knob 1 (the list, its
last round two rows per lane where at most 32 entries are left) against knob 2 (the list, four rows per lane in every round)
against knob 0 (no list) byte for byte - counts, log sinogram, path lengths - on guarded buffers, through both entry points of the
packed projection (without a map, and with the air-column map forced).  Geometry, volumes and helpers are those of
tests/test_gpu_rows16_dedup.py: 32 x 32 in plane, 6 views x 10 channels; 256 / 512 / 1024 rows are 4 / 2 / 1 pairs per wave, 200
rows leave the last lane of a pair with invalid rows, 2048 rows are two z-chunks.

F = fresh quads of a wave = entries of its list.  A round of 64 entries detects four rows per lane; the last round detects two
when its remainder is at most 32 (the one-row form for at most 16 is not built: those lists take the two-row round).  Every case
counts F itself from the path lengths of the knob-0 run and asserts the width of the last round it was made for:

  levels:T      T = 16, 32, 64, 80, 96, 128, 144, 160, 192 and each plus one pair's worth (the pairs of the wave): remainders 16,
                32, 64 and the counts just past them in the first, second and third round; 192 + pairs needs four rounds, so the
                wave keeps its rounds of rows
  extruded      the smallest F a shape allows: the pairs of the wave
  air, rod      all-air lists of two entries; air pairs beside water pairs, so that a narrow round holds entries of two chords
and a table whose last row holds a NaN or an infinity (the absent-material short cut must stay off in the narrow rounds too)."""
import numpy as np
import pytest

from test_gpu_rows16_dedup import Case, N_CHANNELS, N_VIEWS, lanes_per_pair, make_volume

pytestmark = pytest.mark.gpu

TARGETS = [16, 32, 64, 80, 96, 128, 144, 160, 192]
# rows per lane of the LAST list round at F = T and at F = T + one pair's worth (1 .. 4 more); 0: no list (four rounds of rows)
WIDTH_AT = {16: 2, 32: 2, 64: 4, 80: 2, 96: 2, 128: 4, 144: 2, 160: 2, 192: 4}
WIDTH_PAST = {16: 2, 32: 4, 64: 2, 80: 2, 96: 4, 128: 2, 144: 2, 160: 4, 192: 0}
ROWS = [256, 512, 1024, 200, 2048]


def last_round_rows(f, live_rounds=4):
    """The rule, restated: 0 where the list saves no round; else 4 for a whole last round, 2 for at most 32 entries, 4 beyond."""
    rounds = -(-f // 64)
    if f < 1 or rounds >= live_rounds:
        return 0
    left = f - 64 * (rounds - 1)
    return 2 if left <= 32 else 4


def three_knobs(case, monkeypatch, what, mu=None):
    """Knob 0 without a map, then knobs 0, 2, 1 and the default through both entry points (the map forced for the second)."""
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '2')
    monkeypatch.setenv('DEXCT_DET_DEDUP', '0')
    off = case.packed(False, mu)
    for skip in (False, True):
        for knob in ('0', '2', '1', None):
            if skip is False and knob == '0':
                continue
            if knob is None:
                monkeypatch.delenv('DEXCT_DET_DEDUP')
            else:
                monkeypatch.setenv('DEXCT_DET_DEDUP', knob)
            got = case.packed(skip, mu)
            for n in off:
                assert np.array_equal(off[n], got[n]), f'{what}: {n} differs (map={skip}, DEXCT_DET_DEDUP={knob})'
    return off


LEVEL_CASES = [(rows, t, past, 3) for rows in ROWS for t in TARGETS for past in (False, True)] + \
              [(rows, t, past, ids) for ids in (2, 4) for rows in (256, 1024) for t in TARGETS for past in (False, True)]


@pytest.mark.parametrize('rows,target,past,n_ids', LEVEL_CASES)
def test_levels_reach_every_width(hip, monkeypatch, rows, target, past, n_ids):
    n_pairs = 64 // lanes_per_pair(rows)
    f_want = target + (n_pairs if past else 0)
    case = Case(hip, make_volume(f'levels:{f_want}', rows, n_ids, seed=rows + n_ids), n_ids, rows)
    off = three_knobs(case, monkeypatch, f'levels:{f_want}')
    full = [f for live, _, f in case.fresh_per_wave(off) if live == n_pairs]
    assert full and set(full) == ({f_want} if rows <= 1024 else {f_want, f_want + 1}), sorted(set(full))
    want = (WIDTH_PAST if past else WIDTH_AT)[target]
    assert all(last_round_rows(f) == want for f in full if f == f_want)
    print(f'rows {rows}, {n_ids} ids: F {sorted(set(full))}, last round {sorted(set(last_round_rows(f) for f in full))} rows per lane')


@pytest.mark.parametrize('rows,n_ids', [(rows, 3) for rows in ROWS] + [(256, 2), (1024, 2), (256, 4), (1024, 4)])
@pytest.mark.parametrize('kind', ['extruded', 'air'])
def test_smallest_lists(hip, monkeypatch, rows, n_ids, kind):
    case = Case(hip, make_volume(kind, rows, n_ids), n_ids, rows)
    off = three_knobs(case, monkeypatch, kind)
    waves = case.fresh_per_wave(off)
    assert all(f == live for live, _, f in waves)                       # one entry per pair
    assert all(last_round_rows(f) == 2 for _, _, f in waves)
    if kind == 'air':                 # neighbouring channels have equal sums and different chords: their counts differ
        c = off['counts'].view(np.float32).reshape(2, N_VIEWS, N_CHANNELS, rows)
        assert (c[:, :, 1:, 0] != c[:, :, :-1, 0]).mean() > 0.5


@pytest.mark.parametrize('rows,n_ids', [(256, 3), (512, 3), (200, 4), (1024, 4)])
@pytest.mark.parametrize('absent', ['0', '1'])
def test_entries_of_two_chords_in_one_round(hip, monkeypatch, rows, n_ids, absent):
    monkeypatch.setenv('DEXCT_DET_ABSENT', absent)
    case = Case(hip, make_volume('rod', rows, n_ids), n_ids, rows)
    off = three_knobs(case, monkeypatch, 'rod')
    pl = off['pathlen'].view(np.float32).reshape(N_VIEWS, N_CHANNELS, rows, n_ids)
    hit = (pl[..., 1] > 0).any(axis=2)
    assert hit.any() and not hit.all() and not pl[..., 2:].any()
    waves = case.fresh_per_wave(off)
    assert all(f == live for live, _, f in waves) and all(last_round_rows(f) == 2 for _, _, f in waves)
    if rows < 1024:                   # a wave of several pairs: some hold an air pair beside a water pair
        n_pairs = 64 // lanes_per_pair(rows)
        mixed = [hit[:, c0:c0 + n_pairs].any(axis=1) & ~hit[:, c0:c0 + n_pairs].all(axis=1) for c0 in range(0, N_CHANNELS, n_pairs)]
        assert np.any(mixed)


@pytest.mark.parametrize('n_ids', [3, 4])
@pytest.mark.parametrize('value', [np.nan, np.inf])
@pytest.mark.parametrize('kind', ['extruded', 'levels:32', 'levels:80'])
def test_not_finite_entry_in_the_last_table_row(hip, monkeypatch, value, n_ids, kind):
    """No ray meets the last material, so the short form would drop its row - and fma(NaN or inf, 0, pe) is NaN: the rounds of
    rows give NaN counts wherever that row is looked at, so the narrow rounds must too."""
    rows = 512
    case = Case(hip, make_volume(kind, rows, n_ids - 1), n_ids, rows)
    mu = case.mu.clone()
    mu[n_ids - 1, mu.shape[1] // 2] = value
    for absent in ('0', '1'):
        monkeypatch.setenv('DEXCT_DET_ABSENT', absent)
        off = three_knobs(case, monkeypatch, f'{value} absent={absent}', mu=mu)
        assert np.isnan(off['counts'].view(np.float32)).any()
    full = [f for live, _, f in case.fresh_per_wave(off) if live == 2]
    assert full and all(last_round_rows(f) == 2 for f in full)
