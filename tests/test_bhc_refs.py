"""The beam-hardening reference, point set and bound of tests/bhc_refs.py, proven on the CPU before any GPU run.

``reference`` (SciPy's cubic Hermite spline, cell by searchsorted) agrees with ``LinearizationTable.evaluate`` (cell by frexp)
on every layout to the table's float32 rounding; ``kernel_float32``, the kernel's float32 operations without fma, meets
4e-7 M with no absolute floor on every layout and returns the table's bits at every node, so a correct float32 evaluation can
reach the bound; every mutant of it breaks the bound on some layout, so the point set and the bound see such errors; and on
the 16 bundled tables ``reference`` meets the exact inverse.

Measured (worst error / bound per layout, in the order of bhc_refs.LAYOUTS):
  evaluate() against reference:  0.006 0.125 0.111 0.094 0.146 0.148 0.148 0.147 0.148 0.148 0.146 0.138
  kernel_float32 against it:     0.324 0.370 0.351 0.327 0.357 0.335 0.353 0.381 0.435 0.435 0.349 0.323
  share of points left to the overflow exclusion: 0.16 % to 0.63 %
Every mutant is caught on at least 8 of the 12 layouts (the a_max mutant needs unequal octave counts, the fraction mutant an
octave with more than one cell); the boundary mutant ``o > n_oct`` by the 122 to 126 points of the first octave beyond each side.
On the 16 bundled tables ``reference`` is within 0.56 ... 0.68 of 1e-7 |exact| + 1e-12 (most of it the float32 rounding of the
table's values, 2^-24 = 0.6e-7), at 3 to 5 s per table for the 200 bisection steps on 23 to 29 thousand points.
"""
import numpy as np
import pytest

import bhc_refs as br
from test_bhc import DETECTORS, SPECTRA, bisect_inverse, log_signal, scanner, spectrum

IDS = [f'E{e}_K{k}_{op}_{on}' for e, k, op, on in br.LAYOUTS]


@pytest.mark.parametrize('layout,nodes', list(zip(br.LAYOUTS, br.NODES)), ids=IDS)
def test_points_cover_the_layout(layout, nodes):
    table, p, ref, M = br.layout_case(layout)
    assert table.n_nodes == nodes and table.pairs().shape == (nodes, 2)
    assert p.dtype == np.float32 and 30000 <= p.size < 100000
    bits = set(p.view(np.uint32).tolist())
    q, idx = br.node_points(table)
    assert idx.size == nodes - 1 and np.array_equal(np.sort(idx), np.delete(np.arange(nodes), table.base_neg))
    qb = q.view(np.uint32).astype(np.int64)
    mag, sign = qb & 0x7FFFFFFF, qb & 0x80000000
    for d in (-2, -1, 0, 1, 2):                      # the node and its neighbours in |p|; below zero lies the other side
        near = mag + d
        assert all(int(b) in bits for b in (sign | near)[near >= 0])
    # every exponent field with its end mantissas, on both signs; zero, the infinities and NaN
    for e in range(255):
        for m in (0, 1, 2, (1 << 23) - 2, (1 << 23) - 1):
            assert (e << 23 | m) in bits and (1 << 31 | e << 23 | m) in bits
    assert {0, 1 << 31, 0x7F800000, 0xFF800000} <= bits and np.count_nonzero(np.isnan(p)) == 1
    a = np.abs(p)
    assert np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny)) >= 126            # denormals
    # every cell of both sides holds its quarter points and midpoint; both extensions are reached
    neg, j = br.cell_of(table, p)
    for side in (False, True):
        cells = table.side_a(side).size - 1
        inside = (neg == side) & (j >= 0) & (j < cells)
        assert np.all(np.bincount(j[inside], minlength=cells) >= 3 + 2)
        assert np.count_nonzero((neg == side) & (j == cells) & np.isfinite(p)) >= 64
    # the reference returns the table's own float32 values at the nodes
    assert np.array_equal(br.reference(table, q)[0], table.pairs()[idx, 0].astype(np.float64))


@pytest.mark.parametrize('layout', br.LAYOUTS, ids=IDS)
def test_reference_matches_evaluate(layout):
    """Two ways to the cell, one spline: only the float32 rounding of the table separates them."""
    table, p, ref, M = br.layout_case(layout)
    with np.errstate(over='ignore', invalid='ignore'):
        ev = table.evaluate(p)
    worst, share = br.compare(table, p, ev, ref, M)
    print(f'{layout}: evaluate() against the reference {worst:.3f} of the bound, {share:.2%} excluded')
    assert worst < 0.5


@pytest.mark.parametrize('layout', br.LAYOUTS, ids=IDS)
def test_kernel_float32_meets_the_bound(layout):
    table, p, ref, M = br.layout_case(layout)
    got = br.kernel_float32(table, p)
    assert got.dtype == np.float32
    worst, share = br.compare(table, p, got, ref, M)
    print(f'{layout}: kernel_float32 against the reference {worst:.3f} of the bound, {share:.2%} excluded')
    q, idx = br.node_points(table)
    assert np.array_equal(br.kernel_float32(table, q).view(np.uint32), table.pairs()[idx, 0].view(np.uint32))
    zero = br.kernel_float32(table, np.array([0.0, -0.0], dtype=np.float32))
    assert np.array_equal(zero.view(np.uint32), table.pairs()[[0, 0], 0].view(np.uint32))


@pytest.mark.parametrize('mutant', br.MUTANTS)
def test_mutant_breaks_the_bound(mutant):
    caught = []
    for layout in br.LAYOUTS:
        table, p, ref, M = br.layout_case(layout)
        r = br.ratios(p, br.kernel_float32(table, p, mutant), ref, M)
        if np.max(r) > 1.0:
            caught.append((layout, int(np.count_nonzero(r > 1.0))))
    print(f'{mutant}: beyond the bound on {len(caught)} of {len(br.LAYOUTS)} layouts: {caught}')
    assert caught, f'no layout notices the mutant {mutant}'


@pytest.mark.parametrize('det,eid', DETECTORS)
@pytest.mark.parametrize('spec_id', SPECTRA)
@pytest.mark.parametrize('material', ['water', 'bone'])
def test_reference_matches_exact_inverse_on_bundled_tables(det, eid, spec_id, material):
    from dex_ct_sim_amd import bhc
    ct, spec = scanner(det, eid), spectrum(spec_id)
    t = bhc.linearization_table(ct, spec, material)
    assert t.cells_log2 in (4, 5)
    w, mu = log_signal(ct, spec, material)
    p = br.points(t, np.random.default_rng(11))
    p = p[(p >= -1) & (p <= 40)]
    ref, _ = br.reference(t, p)
    exact = t.mu_ref * bisect_inverse(w, mu, p.astype(np.float64))[0]
    err = np.abs(ref - exact) - (1e-7 * np.abs(exact) + 1e-12)
    k = int(np.argmax(err))
    print(f'{det} {spec_id} {material}: K = {t.cells_log2}, {p.size} points, worst error / bound '
          f'{np.max(np.abs(ref - exact) / (1e-7 * np.abs(exact) + 1e-12)):.3f}')
    assert err[k] <= 0, f'worst at p = {float(p[k])!r}: {ref[k]!r} vs {exact[k]!r}'
