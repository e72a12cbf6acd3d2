"""References and point sets for the beam-hardening kernel (dexct_bhc_linearize), NumPy and SciPy only.

The kernel finds its table cell by bit tricks on p (exponent -> octave, top K mantissa bits -> cell, the rest -> fraction), and
``LinearizationTable.evaluate`` restates that through ``frexp``.  ``reference`` here locates the cell by ``searchsorted`` on the
node positions and evaluates SciPy's cubic Hermite spline, so nothing is shared with either but the table itself.  ``points``
puts values where bit tricks go wrong: on every node and one and two ulp either side, inside every cell, and through every
exponent field of float32.  ``kernel_float32`` is the kernel's float32 operation sequence in NumPy; tests/test_bhc_refs.py
mutates it to show that the point set and the bound notice such errors.
"""
import functools

import numpy as np
from scipy.interpolate import CubicHermiteSpline

RTOL = 4e-7                 # the project's figure for the float32 evaluation (tests/test_gpu_bhc.py), here times the cell magnitude
OVERFLOW = 1e38             # a reference beyond this is float32 overflow of the linear extension: sign and not-NaN only
MAX_EXCLUDED = 0.01         # share of a point set that may fall to that exclusion

# (log2_min E, cells_log2 K, oct_pos, oct_neg): the layouts under test, from the smallest table to the largest the checks admit
LAYOUTS = ((-20, 0, 0, 0), (-20, 0, 26, 20), (-20, 3, 0, 5), (-20, 3, 5, 0), (-20, 6, 26, 20), (-20, 7, 26, 20),
           (-20, 7, 31, 30), (-100, 5, 100, 100), (-100, 11, 1, 0), (-100, 11, 0, 1), (60, 4, 40, 40), (100, 7, 0, 0))
NODES = (4, 50, 58, 58, 3074, 6146, 8066, 6466, 6146, 6146, 1314, 258)

MUTANTS = ('node_index', 'frac_shift', 'lin_width', 'a_max_side', 'base_neg', 'beyond_test', 'slope_sign', 'h_swap')


def synthetic_table(E, K, oct_pos, oct_neg):
    """A table of the layout (E, K, oct_pos, oct_neg) over smooth, strictly monotone, non-polynomial functions of
    x = a / 2^E, one per side, scaled by 2^E so that the slopes are O(1) at every E."""
    from dex_ct_sim_amd import bhc
    C = 1 << K
    value, slope = [], []
    for neg, n_oct in ((False, oct_pos), (True, oct_neg)):
        x = np.ldexp(bhc.node_a(np.arange(C * (1 + n_oct) + 1), K, E), -E)
        if neg:
            f, df = -(x + x * x / (2 * (1 + x))), -(1 + (x * x + 2 * x) / (2 * (1 + x) ** 2))
        else:
            f, df = np.log1p(x) + x / (4 * (1 + x)), 1 / (1 + x) + 1 / (4 * (1 + x) ** 2)
        value.append(np.ldexp(f, E))
        slope.append(df)
    return bhc.LinearizationTable('synthetic', 1.0, K, np.concatenate(value), np.concatenate(slope), log2_min=E,
                                  oct_pos=oct_pos, oct_neg=oct_neg)


def _sides(table):
    """Per side: (neg, node positions in a = |p|, float32-rounded values, float32-rounded slopes), all float64."""
    pairs = table.pairs().astype(np.float64)
    for neg in (False, True):
        xa = table.side_a(neg)
        base = table.base_neg if neg else 0
        yield neg, xa, pairs[base:base + xa.size, 0], pairs[base:base + xa.size, 1]


def cell_of(table, p):
    """(neg, j) of every p: its side and the cell [node j, node j + 1) found by searchsorted; j = cells of the side beyond
    the last node (that node included), -1 for NaN."""
    p = np.asarray(p, dtype=np.float64)
    neg = p < 0
    j = np.full(p.shape, -1, dtype=np.int64)
    for side, xa, _, _ in _sides(table):
        sel = (neg == side) & ~np.isnan(p)
        j[sel] = np.searchsorted(xa, np.abs(p[sel]), side='right') - 1
    return neg, j


def reference(table, p):
    """(value, M) in float64 on the table's float32-rounded pairs: per side SciPy's cubic Hermite spline in a = |p|, linear
    from the last node's value and slope beyond it; +-0 on the positive side, NaN -> NaN, +-inf by the end slope's sign.
    M is the magnitude of the cell, max |v| + width max |s| over its two nodes, and |v_end| + |a - a_max| |s_end| beyond."""
    p = np.asarray(p, dtype=np.float64)
    neg, j = cell_of(table, p)
    ref, M = np.full(p.shape, np.nan), np.full(p.shape, np.nan)
    with np.errstate(invalid='ignore', over='ignore'):
        for side, xa, v, s in _sides(table):
            last = xa.size - 1
            sel = (neg == side) & (j >= 0)
            a, c = np.abs(p[sel]), j[sel]
            r, m = np.empty(a.shape), np.empty(a.shape)
            ins = c < last
            ci = c[ins]
            r[ins] = CubicHermiteSpline(xa, v, s, extrapolate=False)(a[ins])
            m[ins] = np.maximum(np.abs(v[ci]), np.abs(v[ci + 1])) + (xa[ci + 1] - xa[ci]) * np.maximum(np.abs(s[ci]),
                                                                                                      np.abs(s[ci + 1]))
            d = a[~ins] - xa[last]
            r[~ins] = np.where(np.isinf(d), np.copysign(np.inf, s[last]), v[last] + d * s[last])
            m[~ins] = np.abs(v[last]) + d * np.abs(s[last])
            ref[sel], M[sel] = r, m
    return ref, M


def node_points(table):
    """(p, index): the float32 p of every node that the kernel can reach and its index in the table.  Node 0 of the
    negative side is p = -0, which belongs to the positive side, so it is not listed."""
    a_pos, a_neg = table.side_a(False), table.side_a(True)[1:]
    p = np.concatenate([a_pos, -a_neg]).astype(np.float32)
    idx = np.concatenate([np.arange(a_pos.size), table.base_neg + 1 + np.arange(a_neg.size)])
    assert np.array_equal(p.astype(np.float64), np.concatenate([a_pos, -a_neg]))           # nodes are float32 values
    return p, idx


def points(table, rng):
    """The float32 values a table is tried at: every node and its 1 and 2 ulp neighbours on both sides; the quarter points
    and the midpoint of every cell; every finite exponent field (0: zero and denormals) x both signs x the mantissas 0, 1, 2,
    2^23 - 2, 2^23 - 1 and 59 random ones; +-0, +-inf and NaN."""
    out = []
    for neg in (False, True):
        a = table.side_a(neg)
        sign = np.uint32(0x80000000 if neg else 0)
        bits = a.astype(np.float32).view(np.uint32).astype(np.int64)
        near = (bits[:, None] + np.array([-2, -1, 0, 1, 2])[None, :]).ravel()
        near = near[near >= 0]                       # below zero lies the other side, which has its own node 0
        out.append((near.astype(np.uint32) | sign).view(np.float32))
        inner = (a[:-1, None] + np.array([0.25, 0.5, 0.75])[None, :] * np.diff(a)[:, None]).ravel()
        out.append((-inner if neg else inner).astype(np.float32))
    man = np.empty((255, 2, 64), dtype=np.int64)
    man[..., :5] = [0, 1, 2, (1 << 23) - 1, (1 << 23) - 2]
    man[..., 5:] = rng.integers(0, 1 << 23, size=(255, 2, 59))
    sweep = (np.arange(255)[:, None, None] << 23) | man | (np.array([0, 1 << 31])[None, :, None])
    out.append(sweep.ravel().astype(np.uint32).view(np.float32))
    out.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32))
    return np.concatenate(out)


def positions(p, q):
    """Where the bit patterns of the float32 values q stand in the float32 array p (each must occur; the first is taken)."""
    pb, qb = np.asarray(p).view(np.uint32), np.asarray(q, dtype=np.float32).view(np.uint32)
    order = np.argsort(pb, kind='stable')
    pos = order[np.minimum(np.searchsorted(pb[order], qb), pb.size - 1)]
    assert np.array_equal(pb[pos], qb), 'a value asked for is not in the point set'
    return pos


def kernel_float32(table, p, mutant=None):
    """bhc_eval of csrc/bhc.hip as a sequence of float32 NumPy operations, without fma.  ``mutant``: one of MUTANTS, a
    deliberate error in that sequence (CPU only; indices are then kept inside the table, as no kernel would)."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    tab = table.pairs()
    K, E = table.cells_log2, table.log2_min
    C, shift = 1 << K, 23 - K
    base_neg = C * (1 + table.oct_pos) + 1 + (mutant == 'base_neg')
    lin_scale, lin_width = f(2.0 ** (K - E)), f(2.0 ** (E - K))
    cell_frac, frac_scale = f(2.0 ** -K), f(2.0 ** -shift)
    a_max_pos, a_max_neg = f(2.0 ** (E + table.oct_pos)), f(2.0 ** (E + table.oct_neg))
    p = np.ascontiguousarray(p, dtype=np.float32)
    shape, p = p.shape, p.ravel()
    nan = p != p
    neg = p < 0
    a = np.abs(p)
    bits = a.view(np.uint32).astype(np.int64)
    base = np.where(neg, base_neg, 0)
    n_oct = np.where(neg, table.oct_neg, table.oct_pos)
    o = (bits >> 23) - (127 + E)
    beyond = (o > n_oct) if mutant == 'beyond_test' else (o >= n_oct)
    lin = ~beyond & (o < 0)
    octv = ~beyond & (o >= 0)

    def fetch(i):
        if mutant is None:
            assert i.size == 0 or (i.min() >= 0 and i.max() < table.n_nodes)
        return tab[np.clip(i, 0, table.n_nodes - 1)]

    out = p.copy()
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        e = fetch((base + C * (1 + n_oct))[beyond])
        a_max = a_max_pos if mutant == 'a_max_side' else np.where(neg[beyond], a_max_neg, a_max_pos).astype(f)
        out[beyond] = e[:, 0] + (a[beyond] - a_max) * e[:, 1]
        j, t, w = np.zeros(p.shape, np.int64), np.zeros(p.shape, f), np.zeros(p.shape, f)
        u = a[lin] * lin_scale
        j[lin] = u.astype(np.int32)
        t[lin] = u - j[lin].astype(f)
        w[lin] = (bits[lin] & 0x7F800000).astype(np.uint32).view(f) * cell_frac if mutant == 'lin_width' else lin_width
        man = bits[octv] & 0x7FFFFF
        j[octv] = C * (1 + o[octv]) + (man >> shift)
        t[octv] = (man & ((1 << (shift + (mutant == 'frac_shift'))) - 1)).astype(f) * frac_scale
        w[octv] = (bits[octv] & 0x7F800000).astype(np.uint32).view(f) * cell_frac
        cell = lin | octv
        if mutant == 'node_index':
            j[cell & (t == 0)] += 1
        j, t, w = j[cell], t[cell], w[cell]
        l, r = fetch(base[cell] + j), fetch(base[cell] + j + 1)
        s = f(1) - t
        h01 = t * t * (f(3) - f(2) * t)
        h00 = f(1) - h01
        if mutant == 'h_swap':
            h00, h01 = h01, h00
        d = t * s * (s * l[:, 1] + t * r[:, 1]) if mutant == 'slope_sign' else t * s * (s * l[:, 1] - t * r[:, 1])
        res = h00 * l[:, 0] + (h01 * r[:, 0] + w * d)
        assert res.dtype == f and t.dtype == f and w.dtype == f
        out[cell] = res
    out[nan] = p[nan]
    return out.reshape(shape)


def ratios(p, got, ref, M):
    """|got - ref| / (RTOL M) per point; 0 where the bound does not apply (NaN in, |ref| > OVERFLOW), inf for a NaN that
    should be a number."""
    got = np.asarray(got, dtype=np.float64)
    held = ~(np.abs(ref) > OVERFLOW) & ~np.isnan(p)
    assert np.all(M[held] > 0)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.abs(got - ref) / (RTOL * M)
    return np.where(held, np.where(np.isnan(r), np.inf, r), 0.0)


def compare(table, p, got, ref, M, max_excluded=MAX_EXCLUDED):
    """Hold ``got`` (the float32 output for the float32 ``p``) to |got - ref| <= RTOL M with no absolute floor.  Where
    |ref| > OVERFLOW (the linear extension overflowing float32, +-inf in included with it) only the sign and not-NaN are asked; such
    points lie beyond a side's last node and stay under ``max_excluded`` of the set.  That cap belongs to the synthetic
    layouts, whose end slopes (0.25 ... 1.5) are ours to choose; a table of a real spectrum ends with the slope mu_ref / mu_min
    of its hardest beam (110 for 80 kV bone on the silicon detector, 1.24 % excluded), each doubling of which takes one more
    of the 254 exponent fields of the sweep out (128 points), so such tables pass None and only the place of the excluded
    points is asked.  NaN must come out exactly where it went in.
    Returns (worst error / bound, excluded share); the assertion names the worst p with its side and cell."""
    p, got = np.asarray(p), np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(p)), 'the NaN pattern of the output differs from the input'
    over = np.abs(ref) > OVERFLOW
    assert np.array_equal(np.sign(got[over]), np.sign(ref[over])), 'wrong sign where the linear extension overflows'
    inf = np.isinf(p)
    assert np.array_equal(got[inf], ref[inf]), '+-inf must give the signed infinity of the end slope'
    neg, j = cell_of(table, p[over])
    assert np.all(j == np.where(neg, table.side_a(True).size, table.side_a(False).size) - 1), 'overflow inside the table'
    share = float(np.count_nonzero(over & ~inf)) / p.size
    assert max_excluded is None or share < max_excluded, f'{share:.2%} of the points overflow float32'
    ratio = ratios(p, got, ref, M)
    k = int(np.argmax(ratio))
    if not ratio[k] <= 1.0:
        neg, j = cell_of(table, p[k:k + 1])
        raise AssertionError(
            f'p = {float(p[k])!r} (bits 0x{int(np.asarray(p[k:k + 1], dtype=np.float32).view(np.uint32)[0]):08x}), '
            f'{"negative" if neg[0] else "positive"} side, cell {int(j[0])} of layout E = {table.log2_min}, K = '
            f'{table.cells_log2}, octaves {table.oct_pos}/{table.oct_neg}: got {got[k]!r}, reference {ref[k]!r}, '
            f'error {abs(got[k] - ref[k]):.3e} = {ratio[k]:.3g} x the bound {RTOL * M[k]:.3e}; '
            f'{np.count_nonzero(ratio > 1)} of {p.size} points beyond the bound')
    return float(ratio[k]), share


@functools.lru_cache(maxsize=None)
def layout_case(layout):
    """(table, points, reference, M) of one synthetic layout, computed once and shared (read-only) by the tests."""
    table = synthetic_table(*layout)
    p = points(table, np.random.default_rng(100 + LAYOUTS.index(layout)))
    ref, M = reference(table, p)
    for x in (p, ref, M):
        x.setflags(write=False)
    return table, p, ref, M
