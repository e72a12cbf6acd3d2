"""CPU self-test of tests/gn_dedup_caps.py, in the manner of tests/test_grid_caps.py.

(a) The constants named in csrc/gn_dedup.hip and csrc/gn_dedup_index.h equal the table every shape of
    tests/test_gpu_gn_dedup_caps.py is derived from, and the shapes leave the trips they are meant to leave.
(b) The host model of the route's index side reproduces the rules of include/dexct_gn_dedup.h on every shape - the descriptor, and
    every pixel takes the entry of its own pair of counts - whatever the buffers held before.
(c) The 14 mutants - each of the seven passes stopped after its first trip, and with its later trips one work item late - change
    the descriptor or some pixel's result on every shape that takes their pass past one trip, with the buffers pre-filled with
    0x00 and with 0xFF: the shapes and fills leave the byte comparison on the GPU nothing to hide behind.
"""
import time

import numpy as np
import pytest

import gn_dedup_caps as dc


def test_constants_in_the_sources_equal_the_table():
    found = dc.source_constants()
    for name, (f, value) in dc.CONSTANTS.items():
        assert found.get(name) == (f, value), f'{name}: csrc has {found.get(name)}, tests/gn_dedup_caps.py has {(f, value)}'
    assert all(dc.scan_literals_present()), dc.scan_literals_present()
    assert dc.SCAN_TRIP_SUMS == 1024


def test_a_changed_constant_is_noticed(monkeypatch):
    monkeypatch.setitem(dc.CONSTANTS, 'kProbeMaxGrid', ('gn_dedup.hip', 2048))
    with pytest.raises(AssertionError):
        test_constants_in_the_sources_equal_the_table()


def test_trips_and_shapes():
    """Today's numbers, from today's constants."""
    assert [dc.trip_items(p) for p in dc.PASSES] == [16384, 8192, 1024, 2048, 256, 2048, 64]
    assert dc.trip_lines('scan', 16) == 1048576 and dc.batch_lines(16) == 256 and dc.batch_lines(130) == 85 and dc.batch_lines(16384) == 1
    shapes = {n: c.shape for n, c in dc.LARGE.items()}
    assert shapes == {'A': (1000, 1311, 16), 'A-no': (1000, 1311, 16), 'A-edge': (1000, 1311, 16), 'A-over': (1000, 1311, 16),
                      'B': (1000, 2101, 16), 'B-edge': (1000, 2101, 16), 'C': (530, 331, 130)}
    a, b, c = (dc.all_trips(*shapes[n]) for n in 'ABC')
    assert dc.items('probe', *shapes['A']) == 20485 and dc.items('scan', *shapes['A']) == 1281 and dc.items('gather', *shapes['A']) == 5122
    assert a == {'probe': 2, 'census': 161, 'scan': 2, 'gather': 3, 'gather_chunk': 1, 'expand': 21, 'expand_reload': 1}
    assert dc.items('probe', *shapes['B']) == 2 * 16384 + 61 and dc.items('scan', *shapes['B']) == 2 * 1024 + 4
    assert b['probe'] == 3 and b['scan'] == 3
    assert dc.items('gather', *shapes['C']) == 2064 and dc.items('expand', *shapes['C']) == 5830
    assert c == {'probe': 1, 'census': 22, 'scan': 1, 'gather': 2, 'gather_chunk': 1, 'expand': 3, 'expand_reload': 1}
    assert sorted({s[2] for _, s, _ in dc.SMALL.values()}) == [4096, 4097, 4160, 8193, 16384, 16385, 16450, 32769]
    assert [dc.trips('expand_reload', 1, 1, R) for R in (4096, 4097, 4160, 8193)] == [1, 2, 2, 3]
    assert [dc.trips('gather_chunk', 1, 3, R) for R in (16384, 16385, 16450, 32769)] == [1, 2, 2, 3]
    for name, case in dc.LARGE.items():                      # every pass a case targets makes more than one trip on it
        for p, kind in case.mutants():
            assert dc.trips(p, *case.shape) > (kind[1] if kind != 'late' else 1), (name, p, kind)


def check(name, s, mutants, use):
    """The model without a mutant is the route; every mutant that is one on this shape is rejected; -> those rejected."""
    use_e, F, cap = s.expected()
    print(f'{name}: {s.V} x {s.C} x {s.R}, descriptor {(use_e, F, cap)}, trips {dc.all_trips(s.V, s.C, s.R)}')
    assert use_e == use
    if use:                                                  # the pad in front of the list is live
        assert F <= cap and F % 64 != 0
    killed = []
    for fill in (0x00, 0xFF):
        desc, keys = dc.run(s, fill)
        assert desc == s.expected() and (keys is None) == (not use)
        assert keys is None or np.array_equal(keys, s.key)
        for m in mutants:
            if dc.vacuous(s, m):
                assert not dc.rejected(s, fill, m), (name, m)
                continue
            assert dc.rejected(s, fill, m), f'{name}: the mutant {m} goes unnoticed with the buffers filled with 0x{fill:02x}'
            killed.append(m)
    return killed


@pytest.mark.parametrize('name', list(dc.LARGE))
def test_large_shapes_reject_their_mutants(name):
    case = dc.LARGE[name]
    t0 = time.perf_counter()
    s = case.sinogram()
    killed = check(name, s, case.mutants(), case.use)
    print(f'{name}: {case.note}; rejected {sorted(set(map(str, killed)))} in {time.perf_counter() - t0:.1f} s')
    assert set(killed) == set(case.mutants())
    if name == 'A-over':
        assert s.expected() == (0, s.cap + 1, s.cap)
    if name in dc.VOTES_NO:
        assert s.expected() == (0, 0, s.cap)
    sample = int(np.bitwise_count(s.bits[::64]).sum())
    assert (sample * 8 <= dc.ceil_div(s.L, 64) * s.R) == (name not in dc.VOTES_NO)


@pytest.mark.parametrize('name', list(dc.SMALL))
def test_small_shapes_reject_their_mutants(name):
    target, (V, C, R), rows = dc.SMALL[name]
    s = dc.small_sinogram(V, C, R, rows)
    assert s.expected()[0] == 1
    killed = check(name, s, list(dc.MUTANTS), 1)             # all 14: those of the other passes are the route itself here
    live = [m for m in dc.MUTANTS if not dc.vacuous(s, m)]
    # (the gather's long lines take the expansion's registers round several times as well)
    assert {m[0] for m in live} <= {target, 'expand_reload'} and set(killed) == set(live)
    assert any(m[0] == target for m in live) == (dc.trips(target, V, C, R) > 1)


def test_every_mutant_is_rejected_somewhere():
    """Each of the 14 is a real change on at least one shape (and is rejected there: the tests above)."""
    live = set()
    for case in dc.LARGE.values():
        live |= {m for m in case.mutants() if m in dc.MUTANTS}
    for target, (V, C, R), rows in dc.SMALL.values():
        s = dc.small_sinogram(V, C, R, rows)
        live |= {m for m in dc.MUTANTS if m[0] == target and not dc.vacuous(s, m)}
    assert live == set(dc.MUTANTS) and len(dc.MUTANTS) == 14
