"""The reduced residual rule of the Newton short cut's chord step (quadrature.residual_rule; csrc/gn.hip, kRedHeader), on the CPU:
for the Kramers 140 / 80 pair and the golden kV / kV case the rule is built over a gate table and judged on verification points
drawn with another seed - the criterion (its largest relative error against a long-double sum of all energies at most 4 x the full
float64 sum's own, measured in the same run on the same points) and the conditions (no cancelling weights, at most 3/4 of the
energies, what the error can move a result by) - six deliberately wrong variants each miss the criterion by an order or more, tables
the short cut does not take install nothing, and the rule's file round-trips and is rejected after a change of any one byte.

The gate tables here are made on the CPU (the library's calibration needs the device): the fixed points at the corners and centres
of a 192-cell grid by a float64 Newton iteration on ln nu_k(a) = ln g_k, assembled and validated by quadrature's own functions.
They cover the same region of the data plane as the device's 384-cell tables; the tests print every figure they assert (-s)."""
import numpy as np
import pytest

import gn_plane_refs as pr
from dex_ct_sim_amd import quadrature as q

N_CELLS = 192              # 36 864 cells: more than RULE_VERIFY_POINTS of them are open
OTHER_SEED = 20261019


def log_newton(g, i0, mus, n_steps=40):
    """Roots [n, 2] of ln nu_k(a) = ln g_k for the counts g [n, 2]: Newton in float64 from 1e-6, steps limited to 20 per component;
    non-finite where it does not arrive."""
    W = np.concatenate([i0, np.repeat(i0, 2, axis=0) * np.tile(mus, (2, 1))]).T             # [e, 6]: nu_0, nu_1, G_00, G_01, G_10, G_11
    a = np.full((len(g), 2), 1e-6)
    with np.errstate(all='ignore'):
        ln_g = np.log(g)
        for _ in range(n_steps):
            s = np.exp(np.clip(-(a @ mus), -700.0, 700.0)) @ W
            nu, G = s[:, :2], s[:, 2:].reshape(-1, 2, 2)
            r = np.log(nu) - ln_g
            J = -G / nu[:, :, None]
            det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
            d = np.stack([(J[:, 1, 1] * r[:, 0] - J[:, 0, 1] * r[:, 1]) / det, (J[:, 0, 0] * r[:, 1] - J[:, 1, 0] * r[:, 0]) / det], axis=1)
            a = a - np.clip(d, -20.0, 20.0)
    return a


def cpu_table(i0, mus, n):
    """(start array, calibration stats) of a gate table with n cells per axis, as matdecomp.calibrate_gate assembles them."""
    cells = q.GATE_CELLS
    try:
        q.GATE_CELLS = n
        p = q.newton_start_grid(i0, mus)
    finally:
        q.GATE_CELLS = cells
    roots = log_newton(p['corner_g'], p['i0'], p['mus'])
    start, _, stats = q.assemble_start(p, np.where(np.all(np.isfinite(roots), axis=1), 17, 255), roots)
    centres = log_newton(q.cell_centres(p), p['i0'], p['mus'])
    start, share, n_bad = q.validate_start(start, p, np.where(np.all(np.isfinite(centres), axis=1), 17, 255), centres)
    return start, dict(stats, grid=True, open_share=float(share), centres_failed=int(n_bad))


@pytest.fixture(scope='module', params=['kramers', 'case0'])
def fitted(request):
    """Per pair, once: the table, its rule, the pivoted QR the rule came from, and the reference on the other seed's points."""
    i0, mus = pr.tables(request.param)
    start, stats = cpu_table(i0, mus, N_CELLS)
    rule, info = q.residual_rule(start, i0, mus, stats)
    print(f'{request.param}: {info}')
    assert rule is not None and info['installed'], info
    used = np.flatnonzero(np.any(i0 > 0.0, axis=0))
    i0u, musu = i0[:, used], mus[:, used]
    R, piv = q.rule_pivots(i0u, musu, q.rule_fit_points(start))
    fit = q.rule_fit_points(start)
    ver = q.rule_verify_points(start, OTHER_SEED)
    return dict(pair=request.param, i0=i0, mus=mus, start=start, stats=stats, rule=rule, info=info, used=used, i0u=i0u, musu=musu, R=R,
                piv=piv, fit=fit, ver=ver, v=q.rule_reference(i0u, musu, ver), nodes_u=np.searchsorted(used, rule['nodes']))


def test_criterion_and_conditions_hold_on_points_of_another_seed(fitted):
    f = fitted
    info, rule, v = f['info'], f['rule'], f['v']
    m = info['nodes']
    # the sets: disjoint, large enough, with the rim of the open region and its negative components, and with a reference
    ver0 = q.rule_verify_points(f['start'], 0)
    fit_set = {tuple(x) for x in f['fit']}
    assert len(f['ver']) >= q.RULE_VERIFY_POINTS and not fit_set & {tuple(x) for x in f['ver']} and not fit_set & {tuple(x) for x in ver0}
    assert {tuple(x) for x in f['ver']} != {tuple(x) for x in ver0}
    assert f['fit'][:, 1].min() < 0.0 and f['ver'][:, 1].min() < 0.0
    unusable = 1.0 - v['usable'].mean()
    ok, fig = q.rule_meets(v, f['nodes_u'], rule['w'])
    print(f'{f["pair"]}: {m} of {f["used"].size} energies; other seed: {len(f["ver"])} points, {unusable:.4f} unusable, {fig}')
    assert unusable <= q.RULE_MAX_UNUSABLE
    assert fig['err_rule'] <= q.RULE_MARGIN * fig['err_full']
    assert fig['amplification'] <= q.RULE_MAX_AMPLIFICATION and fig['shift_rule'] <= q.RULE_MAX_SHIFT and ok
    assert m % 2 == 0 and m <= q.RULE_MAX_SHARE * f['used'].size and len(set(rule['nodes'].tolist())) == m
    # it is the pivoted QR's rule of that count, and the smallest even count that passes on the builder's own points
    J, w = q.rule_weights(f['R'], f['piv'], m, f['i0u'])
    assert np.array_equal(f['used'][J], rule['nodes']) and np.array_equal(w, rule['w'])
    v0 = q.rule_reference(f['i0u'], f['musu'], ver0)
    assert q.rule_meets(v0, J, w)[0] and not q.rule_meets(v0, *q.rule_weights(f['R'], f['piv'], m - 2, f['i0u']))[0]
    # a node the second measurement does not weight has weight exactly 0 there (the kernel's class B)
    dark = f['i0'][1][rule['nodes']] == 0.0
    print(f'{f["pair"]}: {dark.sum()} nodes without weight in measurement 1, {(rule["w"] < 0).sum()} negative weights')
    assert np.all(rule['w'][1][dark] == 0.0) and np.all(rule['w'][0][f['i0'][0][rule['nodes']] == 0.0] == 0.0)


def test_wrong_variants_miss_the_criterion_by_an_order(fitted):
    f = fitted
    v, m, J, w = f['v'], f['info']['nodes'], f['nodes_u'], f['rule']['w']
    allowed = q.RULE_MARGIN * float(v['err_full'][v['usable']].max())
    big = int(np.argmax(np.abs(w[0])))
    variants = {
        'one node dropped': (np.delete(J, big), np.delete(w, big, axis=1)),
        'weights rounded to float32': (J, w.astype(np.float32).astype(np.float64)),
        'weights of the two measurements swapped': (J, w[::-1]),
        'X without the identity part': q.rule_weights(f['R'], f['piv'], m, f['i0u'], identity=False),
        'rows not normalised': q.rule_weights(*q.rule_pivots(f['i0u'], f['musu'], f['fit'], normalise=False), m, f['i0u']),
        'fit on the thick half of the domain only': q.rule_weights(
            *q.rule_pivots(f['i0u'], f['musu'], q.rule_fit_points(f['start'], thick_half_only=True)), m, f['i0u']),
    }
    for name, (nodes, weights) in variants.items():
        err, _ = q.rule_errors(v, nodes, weights)
        worst = float(err[v['usable']].max())
        print(f'{f["pair"]} {name}: {worst:.2e} = {worst / allowed:.1f} x the error allowed ({allowed:.2e})')
        assert worst >= 10.0 * allowed, name


def test_tables_the_short_cut_does_not_take_install_nothing(golden):
    i0, mus = pr.tables('kramers')
    # three energies; fewer weighted energies than the short cut's limit
    for keep in (np.array([20, 60, 100]), np.arange(0, 2 * (q.RULE_MIN_ENERGIES - 1), 2)):
        rule, info = q.residual_rule(np.zeros(q.START_HEADER), i0[:, keep], mus[:, keep])
        assert rule is None and not info['installed'] and 'energies' in info['reason'], info
    # an ill-posed bundled pair (golden case 1: 140 kV against 6 MV)
    i0, mus = golden['gn1_i0'], golden['gn1_mus']
    start, stats = cpu_table(i0, mus, 96)
    assert q.pair_is_ill_posed(stats), stats
    rule, info = q.residual_rule(start, i0, mus, stats)
    assert rule is None and info['reason'] == 'ill-posed pair', info
    # no one-step tables
    rule, info = q.residual_rule(None, *pr.tables('kramers'))
    assert rule is None and info['reason'] == 'no one-step tables'


def test_rule_file_round_trips_and_a_changed_byte_is_rejected(fitted, tmp_path):
    f = fitted
    n_e = f['i0'].shape[1]
    path = q.rule_cache_path(str(tmp_path), f['i0'], f['mus'], f['start'])
    assert path.startswith(str(tmp_path)) and 'rule_' in path
    assert q.rule_cache_path(None, f['i0'], f['mus'], f['start']) is None and q.rule_from_disk(path, n_e) is None
    other = f['i0'].copy()
    other[0, 50] *= 1.0 + 1e-15
    assert q.rule_cache_path(str(tmp_path), other, f['mus'], f['start']) != path                # keyed by content
    q.rule_to_disk(path, f['rule'], f['info'])
    rule, info = q.rule_from_disk(path, n_e)
    assert np.array_equal(rule['nodes'], f['rule']['nodes']) and np.array_equal(rule['w'], f['rule']['w']) and info == f['info']
    assert q.rule_from_disk(path, int(f['rule']['nodes'].max())) is None                          # tables with fewer energies
    raw = open(path, 'rb').read()
    # any byte: the first, one of the stored weights, every 97th, the last of the archive, the checksum's first and last
    at = raw.find(np.ascontiguousarray(f['rule']['w']).tobytes()[:16])
    assert at > 0
    for where in sorted({0, at + 3, len(raw) - 33, len(raw) - 32, len(raw) - 1} | set(range(5, len(raw), 97))):
        bad = bytearray(raw)
        bad[where] ^= 0x01
        open(path, 'wb').write(bytes(bad))
        assert q.rule_from_disk(path, n_e) is None, where
    open(path, 'wb').write(raw)
    assert q.rule_from_disk(path, n_e) is not None
    open(path, 'wb').write(bytes(raw[:len(raw) // 2]))
    assert q.rule_from_disk(path, n_e) is None
    # the verdict "nothing installed" is kept too
    q.rule_to_disk(path, None, {'installed': False, 'version': q.RULE_VERSION, 'reason': 'ill-posed pair'})
    assert q.rule_from_disk(path, n_e) == (None, {'installed': False, 'version': q.RULE_VERSION, 'reason': 'ill-posed pair'})


def test_native_rows_of_a_rule(fitted):
    """dexct_gn_reduced_rows (pure host code): the rows of the kernel's table format - exponent columns with the bits of the full
    tables', the two weights in slots 2 and 8, zeros elsewhere - sorted into the classes both / only 0 / only 1 with the always
    clipped rows first, and the classes' own counts in the header; bad arguments are refused."""
    from dex_ct_sim_amd import _native
    f = fitted
    mus, nodes, w = f['mus'], f['rule']['nodes'], f['rule']['w'].copy()
    both = np.flatnonzero((w[0] != 0.0) & (w[1] != 0.0))
    w[0, both[2]] = 0.0                             # a node only measurement 1 weights, and one nobody weights
    w[:, both[4]] = 0.0
    block = _native.gn_reduced_rows(mus, nodes, w)
    H, T = _native.GN_REDUCED_HEADER, _native.GN_TABLE_ROW
    rows = block[H:].reshape(-1, T)
    n = int(block[0])
    assert n == len(rows) == len(nodes) - 1 and block[9] == block.size == H + T * n and np.all(block[10:H] == 0.0)
    nA, nAc, nB, nBc, nC, nCc = (int(x) for x in block[1:7])
    k_exp = float.fromhex('0x1.71547652b82fep+11')           # 2048 / ln 2 (csrc/gn.hip, kExpScale)
    z0, z1 = w[0] == 0.0, w[1] == 0.0
    cls = np.where(~z0 & ~z1, 0, np.where(~z0, 1, np.where(~z1, 2, 3)))
    big = ~(np.maximum(np.abs(mus[0][nodes]), np.abs(mus[1][nodes])) <= 4.0)
    order = [j for c in (0, 1, 2) for part in (True, False) for j in range(len(nodes)) if cls[j] == c and big[j] == part]
    assert (nA, nB, nC) == tuple(int((cls == c).sum()) for c in (0, 1, 2)) and nC >= 1 and nB >= 1
    assert (nAc, nBc, nCc) == tuple(int(((cls == c) & big).sum()) for c in (0, 1, 2))
    want = np.zeros((n, T))
    want[:, 0], want[:, 1] = -mus[0][nodes[order]] * k_exp, -mus[1][nodes[order]] * k_exp
    want[:, 2], want[:, 8] = w[0][order], w[1][order]
    assert np.array_equal(rows, want)
    free = ~big[order]
    assert block[7] == np.abs(mus[0][nodes[order]][free]).max() and block[8] == np.abs(mus[1][nodes[order]][free]).max()
    lib = _native.load()
    args = lambda nd, n_e, out: (mus.ctypes.data, n_e, nd.ctypes.data, nd.size, np.ascontiguousarray(w[0]).ctypes.data,
                                 np.ascontiguousarray(w[1]).ctypes.data, out.ctypes.data, out.size)
    nd32 = np.ascontiguousarray(nodes, dtype=np.int32)
    out = np.zeros(H + T * nd32.size)
    assert lib.dexct_gn_reduced_rows(*args(nd32, mus.shape[1], out)) == 0
    assert lib.dexct_gn_reduced_rows(*args(nd32, mus.shape[1], out[:-1])) == -1                 # a short block
    assert lib.dexct_gn_reduced_rows(*args(nd32, int(nd32.max()), out)) == -1                   # a node outside the tables
    w[1, 3] = np.inf
    assert lib.dexct_gn_reduced_rows(*args(nd32, mus.shape[1], out)) == -1
