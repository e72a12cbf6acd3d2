"""tests/gn_plane_refs.py checked on the CPU: the coordinates invert each other, the point sets land where they are aimed, the
extended-precision root is one, the reference is usable on (almost) every point of every set and closer to the truth than the
1e-12 it judges.  Two table pairs: golden case 0 (the bundled 140 / 80 kV spectra) and the Kramers 140 / 80 pair of
tests/test_gpu_gn.py::test_short_cut_on_poisson_counts_of_physical_spectra."""
import numpy as np
import pytest

import gn_plane_refs as pr

SETS = ('interior', 'corners0', 'corners1', 'edges', 'thick', 'ratio_rim', 'border')
USABLE_CAP = 0.01
SEED, tables = pr.SEED, pr.tables


@pytest.fixture(scope='module', params=['case0', 'kramers'])
def plane(request):
    from dex_ct_sim_amd import quadrature
    i0, mus = tables(request.param)
    head = quadrature.newton_start_grid(i0, mus)['head']
    return {'pair': request.param, 'i0': i0, 'mus': mus, 'head': head, 'cut': pr.DOMAIN_CUT.get(request.param),
            'sets': pr.point_sets(head, SEED, (i0, mus), pr.DOMAIN_CUT.get(request.param))}


def test_coordinates_invert_each_other(plane):
    """plane_of(counts_of(.)) is the identity to 1e-12 of a cell in long double - the two are inverse functions.  In float64 the
    COUNTS are quantised (half an ulp of g = air exp(-16 u) is 2^-53 / (16 u0) of ln u0: 2.9e-12 of a cell along fx and, times
    (1 + |t|) head[7] / head[5], up to 1e-10 along fy at u0 = 1e-4 - measured: 5.2e-12 and 1.2e-10), so there the round trip
    is held to 1e-12 plus four such half-ulps: exp, the count's own rounding and the two logarithms."""
    head = plane['head']
    for name, s in plane['sets'].items():
        fx, fy = s['fxy'].T
        bx, by = pr.plane_of(head, pr.counts_of(head, fx.astype(pr.LD), fy.astype(pr.LD)))
        assert max(np.abs(bx - fx).max(), np.abs(by - fy).max()) < 1e-12, name
        bx, by = pr.plane_of(head, pr.counts_of(head, fx, fy))
        u0 = np.exp(head[4] + fx / head[5])
        q = 4.0 * 2.0 ** -53 * head[2] / u0
        t = np.abs(head[6] + fy / head[7])
        ex, ey = np.abs(bx - fx) - head[5] * q, np.abs(by - fy) - head[7] * q * (1.0 + t)
        print(f'{plane["pair"]} {name}: float64 round trip {np.abs(bx - fx).max():.2e} / {np.abs(by - fy).max():.2e} of a cell')
        assert ex.max() < 1e-12 and ey.max() < 1e-12, name


def test_sets_fall_in_the_cells_they_are_aimed_at(plane):
    head, n, sets = plane['head'], int(plane['head'][3]), plane['sets']
    i_lo, i_hi, j_lo, j_top = pr.domain(head, plane['cut'])
    j_hi = int(j_top.max())
    assert (i_lo, j_lo, j_hi) == (3, 58, 325) and np.exp(head[4] + i_hi / head[5]) <= 0.75 < np.exp(head[4] + (i_hi + 1) / head[5])
    assert np.all(j_top[:344] == 325) and np.all(np.diff(j_top) <= 0) and (np.all(j_top == 325) if plane['cut'] is None else j_top[i_hi] == 167)
    for name, s in sets.items():
        fxy, cell = s['fxy'], s['cell']
        inside = (fxy >= 0.0) & (fxy < n)
        assert np.array_equal(np.where(inside, np.floor(fxy), -1), cell), name                  # the host's floor is the aim
        # ... and so is the place of the float64 counts, within 1e-9 of a cell
        back = np.stack(pr.plane_of(head, pr.counts_of(head, fxy[:, 0], fxy[:, 1])), axis=1)
        assert np.abs(back - fxy).max() < 1e-9, name
        assert len(fxy) <= 15000, name
        if name != 'border':
            assert cell[:, 0].min() >= i_lo and cell[:, 0].max() <= i_hi, name
            lo, up = (j_lo - 1, 1) if name == 'ratio_rim' else (j_lo, 0)
            assert cell[:, 1].min() >= lo and np.all(cell[:, 1] <= j_top[cell[:, 0]] + up), name
    m = len(sets['interior']['fxy'])
    assert (5500 if plane['cut'] is None else 5300) < m < 6500 and len(np.unique(sets['interior']['cell'], axis=0)) == m
    both = np.concatenate([sets['corners0']['cell'], sets['corners1']['cell']])
    assert len(both) == 4 * m and np.array_equal(np.unique(both, axis=0), np.unique(sets['interior']['cell'], axis=0))
    w = sets['interior']['fxy'] - sets['interior']['cell']
    assert w.min() > 0.0 and w.max() < 1.0
    # corners: on the node, and the last double below the next one - on the intended side, by less than 1e-9
    c = sets['corners0']
    k = len(c['fxy']) // 4
    w = c['fxy'] - c['cell']
    assert np.all(w[:k] == 0.0) and np.all(w[k:2 * k, 0] < 1.0) and np.all(w[k:2 * k, 0] > 1.0 - 1e-9) and np.all(w[k:2 * k, 1] == 0.0)
    assert np.all(w[2 * k:3 * k, 0] == 0.0) and np.all((w[2 * k:, 1] < 1.0) & (w[2 * k:, 1] > 1.0 - 1e-9))
    assert np.all((w[3 * k:, 0] < 1.0) & (w[3 * k:, 0] > 1.0 - 1e-9))
    assert np.all(np.nextafter(c['fxy'][k:2 * k, 0], np.inf) == c['cell'][k:2 * k, 0] + 1.0)
    e = sets['edges']
    w = e['fxy'] - e['cell']
    k = len(w) // 2
    assert np.all(w[:k, 0] == 0.0) and np.all(w[:k, 1] > 0.0) and np.all(w[k:, 1] == 0.0) and np.all(w[k:, 0] > 0.0)
    # thick: every cell of four rows; ratio_rim: both columns whole, and a connected water line
    assert len(np.unique(sets['thick']['cell'], axis=0)) == sum(j_top[i] - j_lo + 1 for i in range(i_hi - 3, i_hi + 1))
    assert set(np.unique(sets['thick']['cell'][:, 0])) == {i_hi - 3, i_hi - 2, i_hi - 1, i_hi}
    rim = sets['ratio_rim']['cell']
    rows = i_hi - i_lo + 1
    assert np.all(rim[:rows, 1] == 57) and np.array_equal(rim[rows:2 * rows, 1], j_top[i_lo:i_hi + 1] + 1)
    assert np.array_equal(rim[:rows, 0], np.arange(i_lo, i_hi + 1)) and rim[rows, 1] == 326
    water = rim[2 * rows:]
    assert len(water) >= rows and set(water[:, 0]) == set(range(i_lo, i_hi + 1)) and np.abs(np.diff(water, axis=0)).max() <= 1
    # border: outside the grid on all four sides, both closed rings, the first open ring
    b = sets['border']
    for axis in (0, 1):
        f = b['fxy'][:, axis]
        assert (f < 0).any() and (f == 0).any() and (f >= n).any() and ((f > n - 1) & (f < n)).any()
        assert ((f > 1) & (f < 2)).any() and ((f > 2) & (f < 3)).any() and (f == 3).any() and (f == n - 3).any()
        assert np.all(b['cell'][(f < 0) | (f >= n), axis] == -1)
    # the launch order: every point once (border: at least once), border runs of every length 0 .. 64 after interior points
    which, idx, names = pr.interleave(sets, SEED + 1)
    assert len(which) % 2 == 1 and names == list(sets)
    bi, ii = names.index('border'), names.index('interior')
    for k, name in enumerate(names):
        got = np.sort(idx[which == k])
        if k != bi:
            assert np.array_equal(got, np.arange(len(sets[name]['fxy']))), name
        else:
            assert np.array_equal(np.unique(got), np.arange(len(sets[name]['fxy'])))
    isb = np.concatenate([[False], which == bi, [False]]).astype(np.int8)
    starts, ends = np.flatnonzero(np.diff(isb) == 1), np.flatnonzero(np.diff(isb) == -1)
    lengths = ends - starts
    assert set(range(1, 65)) <= set(lengths.tolist()) and np.all(which[starts[starts > 0] - 1] == ii)
    assert np.array_equal(pr.gather(sets, (which, idx, names))[which == ii], sets['interior']['fxy'][idx[which == ii]])


def test_exact_root_recovers_the_truth():
    """Counts formed in long double from known thicknesses (physical rays, water rays among them): the long-double Newton
    returns them.  The equations are met to 1e-17 (RESID_TOL); the root follows them through the inverse of the log-Jacobian,
    so 1e-17 of the ROOT is out of reach of a 64-bit mantissa: 1.08e-19 x sqrt(140 energies) x cond (17 - 50 on these rays) =
    2e-17 .. 6e-17.  Held to 2e-16 of max(|a|, 1) per component (measured 7.3e-17 at worst, 2.8e-17 at the 99th percentile):
    four orders below the 1e-12 this root judges.  A wrong start is forgotten."""
    i0, mus = tables('case0')
    rng = np.random.default_rng(5)
    n = 4000
    a = np.stack([rng.uniform(0, 40, n) * rng.choice([0.02, 0.3, 1.0], n), rng.uniform(0, 8, n) * rng.choice([0.0, 0.1, 1.0], n)], -1)
    a[: n // 3, 1] = -0.008 * a[: n // 3, 0]
    nu, _ = pr.model_ld(a.astype(pr.LD), i0, mus)
    assert np.finfo(pr.LD).nmant >= 63
    root, resid, cond = pr.exact_root(nu, i0, mus, a * (1.0 + 1e-9) + 1e-9)
    rel = np.abs(root - a.astype(pr.LD)) / np.maximum(np.abs(a), 1.0)
    print(f'exact_root: worst {float(rel.max()):.2e}, residual {float(resid.max()):.2e}, cond {cond.min():.0f} .. {cond.max():.0f}')
    assert np.all(resid < 1e-17 * np.maximum(np.abs(np.log(nu)), 1.0))
    assert rel.max() <= 2e-16 and cond.max() < 100
    # the float64 oracle on the rounded counts ends within 1e-12 of it, and reference() says so
    g = nu.astype(np.float64)
    r, slack, usable = pr.reference(g, i0, mus)
    assert usable.all() and (slack / np.maximum(np.abs(r), 1.0)).max() < 1e-12
    assert (np.abs(r - a) / np.maximum(np.abs(a), 1.0)).max() < 1e-12          # (the counts' rounding, through cond)
    # counts that are no counts are not usable
    bad = g[:4].copy()
    bad[0, 0], bad[1, 1], bad[2, 0], bad[3, 1] = np.nan, 0.0, -1.0, np.inf
    assert not pr.reference(bad, i0, mus)[2].any()


@pytest.mark.parametrize('name', SETS)
def test_reference_is_usable_and_tighter_than_the_contract(plane, name):
    """``usable`` - the oracle finite and arrived within 1e-12 of the extended-precision root, relative to max(|a|, 1) per
    component, the root converged and well conditioned - leaves out at most 1 % of a set's points (no cap for ``border``): the
    reference is tighter than the contract it judges on (all but 1 % of) every set, or the set's domain is shrunk
    (gn_plane_refs.DOMAIN_CUT: case 0).  Recorded (median / 99th percentile / maximum of that distance): DESIGN.md section 5."""
    s = plane['sets'][name]
    g = pr.counts_of(plane['head'], s['fxy'][:, 0], s['fxy'][:, 1])
    root, slack, usable = pr.reference(g, plane['i0'], plane['mus'], screen=np.full(len(g), name == 'border'))
    rel = (slack / np.maximum(np.abs(root), 1.0)).max(axis=1)
    print(f'{plane["pair"]} {name}: {len(g)} points, {1.0 - usable.mean():.4f} not usable; slack median '
          f'{np.median(rel[usable]):.1e}, p99 {np.percentile(rel[usable], 99):.1e}, max {rel[usable].max():.1e}')
    assert len(g) <= 15000
    if name != 'border':
        assert 1.0 - usable.mean() <= USABLE_CAP
    assert usable.sum() > 100 and rel[usable].max() < 1e-12
