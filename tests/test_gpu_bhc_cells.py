"""dexct_bhc_linearize at every cell edge and table layout, against the independent reference of tests/bhc_refs.py.

The kernel reads octave, cell and fraction from the bits of p.  The bundled spectra only ever give it two layouts (K = 4 or 5,
E = -20, 26 / 20 octaves: 770 or 1538 nodes, 6 or 12 KiB of LDS); its entry point takes K = 0 ... 12, E = -100 ... 100, any octave
counts from 0 and up to 8192 nodes (64 KiB).  Here it runs on twelve synthetic layouts that span those limits, on the 80 kV water
and bone tables built at K = 6 and 7 (which the builder may return for a harder spectrum) and on all 16 bundled tables.  The
inputs are bhc_refs.points: every node and one and two ulp either side of it, the quarter points and midpoint of every cell,
every exponent field of float32 on both signs (zero and denormals included), +-0, +-inf and NaN.  The bound is 4e-7 M with M the
magnitude of the cell and no absolute floor; tests/test_bhc_refs.py shows on the CPU that a correct float32 evaluation
reaches it and that eight kinds of indexing and basis errors do not.

Measured on an MI355X, all 41 cases passing, 11 s for the module.  Worst error / bound (4e-7 M) per synthetic layout, in the
order of bhc_refs.LAYOUTS, with the share of points left to the overflow exclusion (extension beyond 1e38):

  (E, K, octaves)      nodes   points   worst   over the denormals   excluded
  (-20,  0,   0,   0)      4   32 667   0.324   8.9e-34              0.61 %
  (-20,  0,  26,  20)     50   33 035   0.370   8.9e-34              0.49 %
  (-20,  3,   0,   5)     58   33 099   0.351   6.1e-33              0.63 %
  (-20,  3,   5,   0)     58   33 099   0.284   6.1e-33              0.47 %
  (-20,  6,  26,  20)   3074   57 227   0.277   4.7e-32              0.27 %
  (-20,  7,  26,  20)   6146   81 803   0.267   9.4e-32              0.19 %
  (-20,  7,  31,  30)   8066   97 163   0.344   9.4e-32              0.16 %
  (-100, 5, 100, 100)   6466   84 363   0.286   1.1e-7               0.18 %
  (-100, 11,  1,   0)   6146   81 803   0.325   7.6e-6               0.22 %
  (-100, 11,  0,   1)   6146   81 803   0.324   5.6e-6               0.26 %
  (60,   4,  40,  40)   1314   43 147   0.349   2.1e-49              0.38 %
  (100,  7,   0,   0)    258   34 699   0.323   1.5e-60              0.61 %

The float32 stand-in without fma (tests/test_bhc_refs.py) gives 0.32 ... 0.44 on the same points, so the kernel's fmaf only rounds
less.  The denormals are not flushed: at E = -100, K = 11 a flushed input alone would miss the bound 38 times over (the largest
denormal is 2^-15 of a cell there, against 4e-7), and the device is 7.6e-6 of the bound away, as the stand-in is.  80 kV tables
built at K = 6 / K = 7: water 0.316 / 0.316, bone 0.323 / 0.323 of 4e-7 M (0.31 ... 0.70 % excluded), and against the exact inverse
on [-1, 40] at most 0.217 of 1e-6 |exact| with no floor, denormal p included.  The 16 bundled tables: 0.296 ... 0.394 of 4e-7 M
(worst: detunedMV water on the energy-integrating detector), the denormals exact (slope 1 at p = 0), 0.42 ... 1.24 % excluded (the
most at 80 kV bone on the silicon detector, whose extension has slope 110).  Every node returned the bits of its table value, both
zeros those of node 0 of the positive side, in place equalled out of place bit for bit, and no bug was found in the kernel.
"""
import functools

import numpy as np
import pytest

import bhc_refs as br
from test_bhc import DETECTORS, SPECTRA, bisect_inverse, log_signal, scanner, spectrum
from test_bhc_refs import IDS

pytestmark = pytest.mark.gpu


def run(table, p):
    """The device output for the float32 array p, out of place, after checking that in place gives the same bits."""
    import torch
    from dex_ct_sim_amd import bhc
    d = torch.tensor(p, device='cuda')
    got = bhc.linearize_device(d, table).cpu().numpy()
    assert bhc.linearize_device(d, table, out=d) is d
    assert np.array_equal(d.cpu().numpy().view(np.uint32), got.view(np.uint32)), 'in place differs from out of place'
    return got


def check_output(table, p, got, ref, M, max_excluded=br.MAX_EXCLUDED):
    """Everything asked of one output: the bound on every point (NaN pattern, infinities, overflow exclusion: br.compare), the
    table's bits at every node, node 0 of the positive side for both zeros, and the denormals on their own for the record.
    Returns (worst error / bound, excluded share, worst error / bound over the denormals)."""
    assert got.dtype == np.float32 and got.shape == p.shape
    worst, share = br.compare(table, p, got, ref, M, max_excluded)
    q, idx = br.node_points(table)
    pairs = table.pairs()
    at = br.positions(p, q)
    bad = np.flatnonzero(got[at].view(np.uint32) != pairs[idx, 0].view(np.uint32))
    assert bad.size == 0, (f'{bad.size} nodes do not return their table value, the first p = {float(q[bad[0]])!r} '
                           f'(node {int(idx[bad[0]])}): {float(got[at][bad[0]])!r} vs {float(pairs[idx[bad[0]], 0])!r}')
    zeros = got[br.positions(p, np.array([0.0, -0.0], dtype=np.float32))]
    assert np.array_equal(zeros.view(np.uint32), pairs[[0, 0], 0].view(np.uint32)), '+-0 must give node 0 of the positive side'
    a = np.abs(p)
    den = (a > 0) & (a < np.finfo(np.float32).tiny)
    assert np.count_nonzero(den) >= 126
    den_worst = float(np.max(br.ratios(p[den], got[den], ref[den], M[den])))
    return worst, share, den_worst


@pytest.mark.parametrize('layout', br.LAYOUTS, ids=IDS)
def test_layout(hip, layout):
    table, p, ref, M = br.layout_case(layout)
    worst, share, den = check_output(table, p, run(table, p), ref, M)
    print(f'layout {layout}: {table.n_nodes} nodes, {p.size} points, worst error / bound {worst:.3f} (denormals {den:.3g}), '
          f'{share:.2%} left to the overflow exclusion')


@functools.lru_cache(maxsize=None)
def physics_table(material, K):
    """The 80 kV table of build_table for one K: the inverse at bhc.node_a, values mu_ref L, slopes sign mu_ref / P'."""
    from dex_ct_sim_amd import bhc
    P = bhc.SpectralLog(*log_signal(scanner(), spectrum('80kV'), material))
    value, slope = [], []
    for sign, n_oct in ((1.0, bhc.OCT_POS), (-1.0, bhc.OCT_NEG)):
        L = P.inverse(sign * bhc.node_a(np.arange((1 << K) * (1 + n_oct) + 1), K))
        value.append(P.mu_mean * L)
        slope.append(sign * P.mu_mean / P.slope(L))
    return bhc.LinearizationTable(material, P.mu_mean, K, np.concatenate(value), np.concatenate(slope))


@functools.lru_cache(maxsize=None)
def physics_points(material, K):
    p = br.points(physics_table(material, K), np.random.default_rng(5))
    p.setflags(write=False)
    return p


@pytest.mark.parametrize('K,nodes', [(6, 3074), (7, 6146)])
@pytest.mark.parametrize('material', ['water', 'bone'])
def test_large_tables_on_real_physics(hip, material, K, nodes):
    table, p = physics_table(material, K), physics_points(material, K)
    assert table.n_nodes == nodes
    ref, M = br.reference(table, p)
    worst, share, den = check_output(table, p, run(table, p), ref, M, None)
    print(f'80kV {material}, K = {K}: {nodes} nodes, {p.size} points, worst error / bound {worst:.3f} (denormals {den:.3g}), '
          f'{share:.2%} excluded')


PARTS = 4


@pytest.mark.parametrize('part', range(PARTS))
@pytest.mark.parametrize('material', ['water', 'bone'])
def test_large_tables_against_the_exact_inverse(hip, material, part):
    """Both large tables against 200 float64 bisection steps on [-1, 40], at the 1e-6 |exact| of tests/test_gpu_bhc.py without
    its absolute floor.  The K = 6 points are among the K = 7 points (the inner points of its cells are nodes and midpoints of
    K = 7, the exponent sweep comes from the same seed), so one inverse serves both; every fourth point per case keeps the
    bisection of a case to a few seconds, and the four cases together cover every point."""
    import torch
    from dex_ct_sim_amd import bhc
    w, mu = log_signal(scanner(), spectrum('80kV'), material)
    p7, p6 = physics_points(material, 7), physics_points(material, 6)
    assert np.all(np.isin(p6.view(np.uint32), p7.view(np.uint32)))
    p = np.unique(p7[(p7 >= -1) & (p7 <= 40)].view(np.uint32)).view(np.float32)[part::PARTS]     # by bits: both zeros stay
    exact = bisect_inverse(w, mu, p.astype(np.float64))[0]
    in6 = np.isin(p.view(np.uint32), p6.view(np.uint32))
    for K, sel in ((6, in6), (7, np.ones(p.shape, dtype=bool))):
        table = physics_table(material, K)
        q, want = p[sel], table.mu_ref * exact[sel]
        got = bhc.linearize_device(torch.tensor(q, device='cuda'), table).cpu().numpy()
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.abs(got - want) / (1e-6 * np.abs(want))
        ratio[(want == 0) & (got == 0)] = 0.0
        i = int(np.argmax(ratio))
        print(f'80kV {material}, K = {K}, part {part}: {q.size} points, worst error {ratio[i]:.3f} of 1e-6 |exact|')
        assert ratio[i] <= 1.0, f'K = {K}: worst at p = {float(q[i])!r}: {float(got[i])!r} vs {want[i]!r}'


@pytest.mark.parametrize('det,eid', DETECTORS)
@pytest.mark.parametrize('spec_id', SPECTRA)
@pytest.mark.parametrize('material', ['water', 'bone'])
def test_bundled_table(hip, det, eid, spec_id, material):
    from dex_ct_sim_amd import bhc
    table = bhc.linearization_table(scanner(det, eid), spectrum(spec_id), material)
    p = br.points(table, np.random.default_rng(11))
    ref, M = br.reference(table, p)
    worst, share, den = check_output(table, p, run(table, p), ref, M, None)
    print(f'{det} {spec_id} {material}: K = {table.cells_log2}, {p.size} points, worst error / bound {worst:.3f} '
          f'(denormals {den:.3g}), {share:.2%} excluded')


def test_accepted_edges_of_the_argument_checks(hip):
    """The last accepted and the first refused value of every range check, through the bare entry point.  The table buffer
    holds the 8194 nodes of the largest layout asked for, so a check that failed to refuse could still not read past it."""
    import torch
    lib = hip
    x = torch.tensor(np.array([0.0, 1e-30, -1e-30, 0.75, -0.75, 3.0, -3.0, 1e30, -1e30, 7e-31, 2.5e30, -2.5e30, 1e-40, -1e-40,
                               1.5, -1.5], dtype=np.float32), device='cuda')
    out = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream

    def call(E, K, op, on, table=None):
        buf = torch.zeros(8194, 2, device='cuda')
        if table is not None:
            buf[:table.n_nodes] = torch.from_numpy(table.pairs()).cuda()
        rc = lib.dexct_bhc_linearize(x.data_ptr(), x.numel(), buf.data_ptr(), E, K, op, on, out.data_ptr(), st)
        torch.cuda.synchronize()
        return rc

    def accepted(layout):
        table = br.synthetic_table(*layout)
        assert call(*layout, table=table) == 0, layout
        p = x.cpu().numpy()
        ref, M = br.reference(table, p)
        br.compare(table, p, out.cpu().numpy(), ref, M)

    accepted((-100, 5, 100, 100))                    # log2_min = -100 (-101 is refused in tests/test_gpu_bhc.py)
    accepted((60, 4, 40, 40))                        # log2_min + octaves = 100 ...
    accepted((100, 7, 0, 0))
    assert call(61, 4, 40, 40) == -1                 # ... 101, by either side or by log2_min alone
    assert call(60, 4, 41, 40) == -1
    assert call(60, 4, 40, 41) == -1
    assert call(101, 7, 0, 0) == -1
    accepted((-100, 11, 1, 0))                       # 6146 nodes at K = 11
    accepted((-100, 11, 0, 1))
    assert call(-100, 12, 0, 0) == -1                # 8194 nodes > 8192
    assert call(-20, 12, 0, 0) == -1
    accepted((-20, 7, 31, 30))                       # 8066 nodes, 64 528 B of LDS: the largest table the checks admit
    assert call(-20, 7, 31, 31) == -1                # 8194 nodes again, by the octaves
