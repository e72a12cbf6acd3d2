"""CPU self-test of tests/grid_caps.py, in the manner of tests/test_bounds_refs.py.

(a) The grid caps named in csrc/*.hip equal the table every size of tests/test_gpu_grid_passes.py is derived from.
(b) For every kernel and every size, in NumPy alone: the problem is built, the reference and its bound computed (timed: each is to
    take seconds), the reference rounded to the output's type passes the comparison the GPU module uses, and two planted results
    do not: the second pass missing (its values keep the 0x00 or the 0xFF fill, or the input of an in-place call; its terms are
    left out of the sums), and the second pass reading its inputs one work item late.  No device: dexct_bhc_linearize's cap
    depends on the compute units, taken as 256 here."""
import time

import numpy as np
import pytest

import grid_caps as gc

REFERENCE_SECONDS = 60.0          # "seconds", with a wide margin for a loaded machine; measured: K = 3 on 4.2 million rays 9 - 10 s
                                  # (the 3 x 3 inverses of the generator), K = 2 under 5 s, everything else under 4 s


def test_caps_in_the_sources_equal_the_table():
    found = gc.source_constants()
    for name, (f, value) in gc.CAPS.items():
        assert found.get(name) == (f, value), f'{name}: csrc has {found.get(name)}, tests/grid_caps.py has {(f, value)}'
    assert {c for c, *_ in gc.ROWS.values()} | {'kBhcBlock'} == set(gc.CAPS)


def test_a_changed_constant_is_noticed(monkeypatch):
    monkeypatch.setitem(gc.CAPS, 'kPwlsMaxBlocks', ('pwls.hip', 2048))
    with pytest.raises(AssertionError):
        test_caps_in_the_sources_equal_the_table()


def test_passes_and_sizes():
    W = 4096 * 256
    assert gc.pass_items('dexct_cov_precision') == (W, 1) and gc.pass_items('dexct_pwls_majorizer', 'float4') == (W, 4)
    assert gc.pass_items('dexct_volume_ids') == (W, 16) and gc.pass_items('dexct_volume_remap') == (2 * W, 4)
    assert gc.pass_items('dexct_reduce_max') == (2048 * 256, 1)
    C = 2 * gc.n_cu()
    assert gc.pass_items('dexct_bhc_linearize', 'float4') == (C * 2048, 4) and gc.pass_items('dexct_bhc_linearize', 'scalar') == (C * 1024, 1)
    assert 2050 * (2052 // 4) == 1051650 > W and 1025 * 1027 == 1052675 > W and 2 * 509 * 1031 == 1049558 > W
    assert 1022 * 1027 > W and 5 * 509 * 1031 > 2 * W


def rejected(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)
    return True


@pytest.mark.parametrize('name', list(gc.CASES))
def test_comparison_rejects_a_missing_and_a_late_second_pass(name):
    t0 = time.perf_counter()
    p = gc.CASES[name]()
    took = time.perf_counter() - t0
    print(f'{name}: inputs, reference and bound in {took:.1f} s; W = {p.W} work items of {p.V}, {len(p.pos)} in all')
    assert took < REFERENCE_SECONDS
    n_pass = -(-len(p.pos) // p.W)
    assert (n_pass >= 3 if name.endswith('-B') else n_pass == 2) and 0 < len(p.pos) % p.W < p.W - 1   # ragged, in the pass it names
    if p.entry == 'dexct_volume_ids':
        p.check_counts(p.counts)
        assert rejected(p.check_counts, p.counts_missing) and rejected(p.check_counts, p.counts_late)
        return
    keeps = [p.fill(0x00), p.fill(0xFF)]
    if p.entry == 'dexct_pwls_residual':
        keeps.append(p.ax)                                           # q = ax
    elif p.entry == 'dexct_sirt_residual':
        keeps.append(p.ax[None])                                     # r = ax
    elif p.entry == 'dexct_sirt_update':
        keeps = [p.x[None]]                                          # in place
    elif p.entry == 'dexct_volume_remap':
        keeps = [p.vol[None]]
    for keep in keeps:
        p.check_values(p.good(keep), keep=keep)
        assert rejected(p.check_values, p.plant_missing(keep), keep=keep)
        assert rejected(p.check_values, p.plant_late(keep), keep=keep)
    for s, (ref, missing, late) in p.sums.items():
        p.check_sum(s, ref)
        p.check_sum(s, ref * (1 + 2.0 ** -41))                       # 4.5e-13: what 4096 partial sums may carry
        assert rejected(p.check_sum, s, missing) and rejected(p.check_sum, s, late)


@pytest.mark.parametrize('line,n_lines,step', gc.SIRT_SMALL)
def test_small_sirt_references(line, n_lines, step):
    """The float32 restatement lies inside the bound of the float64 reference; a float32 difference in norm2 does not meet 1e-12."""
    p = gc.SirtResidual(line, n_lines, step)
    keep = p.fill(0xFF)
    p.check_values(np.where(p.written, p.f32, keep), keep=keep)
    if step > 1:                                                     # a skipped line that changed
        assert rejected(p.check_values, np.where(p.written, p.f32, F32_ONE), keep=keep)
    u = gc.SirtUpdate(line * n_lines, bool(step == 3))
    u.check_values(u.f32.copy())
    assert np.array_equal(u.f32[0][u.stay], np.maximum(u.x[u.stay], 0) if u.nonneg else u.x[u.stay])


F32_ONE = np.float32(1.0)


def test_norm2_needs_the_float64_difference():
    """sum (b - ax)^2 / R with the difference rounded to float32 first misses the float64 formula by far more than 1e-12: the
    reason dexct_sirt_residual forms it in float64."""
    for shape in ((1027, 1022, 1), (257, 1, 1), (63, 1, 1)):
        p = gc.SirtResidual(*shape)
        hit = p.R > 0
        d32 = (p.b - p.ax).astype(np.float64)
        rounded = float(np.sum(d32[hit] ** 2 / p.R[hit].astype(np.float64)))
        rel = abs(rounded - p.sums['norm2'][0]) / p.sums['norm2'][0]
        print(f'{p.label}: norm2 from the float32 difference: relative {rel:.2e}')
        assert rejected(p.check_sum, 'norm2', rounded)
