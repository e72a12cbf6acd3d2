"""What the Newton short cut must return over the whole plane of its table, and where to ask: the coordinates of csrc/gn.hip
gn_start in both directions, an extended-precision root of the two equations, the float64 oracle's distance from it, and
named sets of points of the (fx, fy) plane that a cell-indexed sextic can get wrong; plain NumPy, no device, no library
(quadrature's host-side grid and oracle/gn_oracle.py only).  tests/test_gn_plane_refs.py shows on the CPU that the reference
is usable on these sets and tighter than the contract it judges; tests/test_gpu_gn_plane.py holds the kernel to it.

The plane.  gn_start places a pixel with the counts (g0, g1) at
    fx = (ln u0 - head[4]) head[5],  fy = (u1 / u0 - head[6]) head[7],  u_k = ln(head[k] / g_k) head[2]
(head: the twelve doubles quadrature.newton_start_grid lays out; head[3] = n cells per axis); cell (i, j) = (floor fx, floor
fy) carries the step budget `need`, and the start value is the 6 x 6 interpolant of the corners' fixed points around it.
``counts_of`` and ``plane_of`` are the two directions in the precision of their arguments (float64, or long double for the
check that they are inverses of each other).  A float64 count g = air exp(-16 u) is quantised: half an ulp of g moves u by
2^-53 / 16 absolutely, ln u0 by 2^-53 / (16 u0), so at the thin end (u0 = 1e-4) a point of the plane is only representable
to 41.7 x 6.9e-14 = 2.9e-12 of a cell along fx and to ~3e-11 along fy; from u0 = 1e-2 on to 1e-13 and better.

The root.  ``exact_root`` solves ln nu_k(a) = ln g_k, k = 0, 1, nu_k(a) = sum_e i0[k][e] exp(-a . mus[:, e]) by Newton in long
double (64-bit mantissa required, 1.08e-19), seeded with the float64 oracle's answer.  ``reference`` returns that root, the
oracle's distance from it per component (``slack``: what float64 arithmetic alone accounts for) and ``usable``: the oracle
ended finite and within 1e-12 of the root, the extended-precision iteration converged and the root is well conditioned.

The sets (``point_sets``): see there.  Everything is a function of the two tables and a seed.
"""
import os

import numpy as np

from dex_ct_sim_amd import quadrature
from oracle import gn_oracle

LD = np.longdouble
RESID_TOL = 1.0e-17            # the long-double Newton has converged: |ln nu_k - ln g_k| < RESID_TOL max(|ln g_k|, 1) (the residual of an
                               # equation in ln g; relative to |ln g_k| alone it would depend on the unit of the counts - a dose
                               # that puts ln g_k = 0 into the plane - which no root does)
FY_LO, FY_HI = 0.15, 0.85      # the physical ratios, as shares of the grid (tests/test_quadrature.py::test_gate_grid_and_start_array)
FX_LO = 3                      # first cell row of the domain: the first open ring


def _dtype(*xs):
    return LD if any(np.asarray(x).dtype == LD for x in xs) else np.float64


def counts_of(head, fx, fy):
    """The counts [.., 2] whose place in the plane is (fx, fy)."""
    dt = _dtype(fx, fy)
    h = np.asarray(head, dtype=dt)
    fx, fy = np.asarray(fx, dtype=dt), np.asarray(fy, dtype=dt)
    u0 = np.exp(h[4] + fx / h[5])
    u1 = u0 * (h[6] + fy / h[7])
    return np.stack([h[0] * np.exp(-u0 / h[2]), h[1] * np.exp(-u1 / h[2])], axis=-1)


def plane_of(head, g):
    """(fx, fy) of the counts g [.., 2]."""
    dt = _dtype(g)
    h = np.asarray(head, dtype=dt)
    g = np.asarray(g, dtype=dt)
    with np.errstate(all='ignore'):
        u0 = np.log(h[0] / g[..., 0]) * h[2]
        u1 = np.log(h[1] / g[..., 1]) * h[2]
        return (np.log(u0) - h[4]) * h[5], (u1 / u0 - h[6]) * h[7]


def model_ld(a, i0, mus):
    """nu [n, 2] and G [n, k, m] = sum_e i0_k mu_m att of the forward model at a [n, 2], in long double."""
    i0, mus = np.asarray(i0, dtype=LD), np.asarray(mus, dtype=LD)
    att = np.exp(-(a[:, 0, None] * mus[0] + a[:, 1, None] * mus[1]))                       # [n, e]
    nu = np.stack([(att * i0[k]).sum(axis=1) for k in (0, 1)], axis=1)
    G = np.stack([np.stack([(att * (i0[k] * mus[m])).sum(axis=1) for m in (0, 1)], axis=1) for k in (0, 1)], axis=1)
    return nu, G


def exact_root(g, i0, mus, a0, n_steps=6):
    """The root of ln nu_k(a) = ln g_k (k = 0, 1) next to a0 [n, 2], for counts g [n, 2] (float64 or long double): Newton in
    long double.  Returns (root [n, 2] long double, residual [n, 2] = |ln nu_k(root) - ln g_k|, cond [n] = sigma_max /
    sigma_min of the log-Jacobian d ln nu_k / d a_m at the root)."""
    if np.finfo(LD).nmant < 63:
        raise RuntimeError('exact_root needs a long double with a 64-bit mantissa (x87); this platform has '
                           f'{np.finfo(LD).nmant + 1} bits - port it to mpmath')
    g = np.asarray(g, dtype=LD).reshape(-1, 2)
    a = np.array(a0, dtype=LD).reshape(-1, 2)
    with np.errstate(all='ignore'):
        ln_g = np.log(g)
        for _ in range(n_steps):
            nu, G = model_ld(a, i0, mus)
            r = np.log(nu) - ln_g
            J = -G / nu[:, :, None]                                                         # [n, k, m]
            det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
            a = a - np.stack([(J[:, 1, 1] * r[:, 0] - J[:, 0, 1] * r[:, 1]) / det,
                              (J[:, 0, 0] * r[:, 1] - J[:, 1, 0] * r[:, 0]) / det], axis=1)
        nu, G = model_ld(a, i0, mus)
        resid = np.abs(np.log(nu) - ln_g)
        J = (-G / nu[:, :, None]).astype(np.float64)
        fro2 = (J ** 2).sum(axis=(1, 2))
        det = np.abs(J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0])
        cond = (fro2 + np.sqrt(np.maximum(fro2 * fro2 - 4.0 * det * det, 0.0))) / (2.0 * det)
    return a, resid, np.where(np.isfinite(cond), cond, np.inf)


def oracle64(g, i0, mus, n_iters=50):
    """oracle.gn_oracle.newton_solve on the counts g [n, 2]: [n, 2]."""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 2)
    with np.errstate(all='ignore'):
        return gn_oracle.newton_solve(np.ascontiguousarray(g.T)[:, :, None], np.asarray(i0, dtype=np.float64),
                                      np.asarray(mus, dtype=np.float64), n_iters).reshape(-1, 2)


def reference(g, i0, mus, screen=None):
    """(root [n, 2] float64 - the extended-precision root, rounded -, slack [n, 2] = |oracle - root| per component, usable [n])
    for the float64 counts g [n, 2].  usable: the oracle ended finite, the long-double iteration converged, the root is well
    conditioned, and the oracle's 50 steps have ARRIVED at it: slack <= 1e-12 max(|root|, 1) per component - a reference further
    from the root than the contract it judges has nothing to say (a state in the middle of a walk is no fixed point, and two
    float64 arithmetics differ on it by 1e-8 of |a|).  ``screen`` (mask or True): pixels that must also pass the oracle's twin
    screen (see below) - for points outside the domain."""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 2)
    ref64 = oracle64(g, i0, mus)
    finite = np.isfinite(ref64).all(axis=1) & np.isfinite(g).all(axis=1) & (g > 0.0).all(axis=1)
    root, resid, cond = exact_root(np.where(finite[:, None], g, 1.0), i0, mus, np.where(finite[:, None], ref64, 0.0))
    with np.errstate(all='ignore'):
        converged = (resid < RESID_TOL * np.maximum(np.abs(np.log(np.where(finite[:, None], g, 1.0).astype(LD))), 1.0)).all(axis=1)
        slack = np.abs(ref64.astype(LD) - root).astype(np.float64)
        arrived = (slack <= 1e-12 * np.maximum(np.abs(root.astype(np.float64)), 1.0)).all(axis=1)
    usable = finite & converged & np.isfinite(root).all(axis=1) & (cond < quadrature.GATE_MAX_COND) & arrived
    if screen is not None and np.any(screen & usable):
        # outside the domain (the border set, the frontier of the open cells) the reference's walk can be CHAOTIC: it passes a
        # nearly singular Hessian and where it lands is an accident of rounding (a count one ulp away ends non-finite).  The
        # oracle's own screen says so: twin trajectories kicked by each step's rounding uncertainty must end within 1e-12 too.
        m = np.flatnonzero(np.broadcast_to(screen, usable.shape) & usable)
        with np.errstate(all='ignore'):
            _, sens = gn_oracle.newton_solve(np.ascontiguousarray(g[m].T)[:, :, None], np.asarray(i0, dtype=np.float64),
                                             np.asarray(mus, dtype=np.float64), 50, return_sensitivity=True)
        usable[m] &= sens['twin'].ravel() <= 1e-12
    return root.astype(np.float64), np.where(usable[:, None], slack, np.inf), usable


# Where a table pair's domain is SHRUNK, on the evidence of the reference alone: (first row, columns lost per row, offset) - from
# that row on the last column of the domain is  floor(0.85 n) - 1 - ceil(slope (i - row)) - offset.
# case0 (the bundled 140 / 80 kV spectra, weight down to 1 keV): beyond the line  fy = 326 - 5.4 (fx - 346)  - the thick end at
# large ratios, past the line of a pure second material, where the root is at a = (-320, 335) .. (-230, 290) - the reference's
# walk from 1e-6 has not arrived after its 50 steps (the oracle is up to 0.56 of |a| from the root; 120 steps arrive): no
# 50-step reference has a root to be held to there.  The line was mapped at every 2nd row and column (first column with
# |oracle - root| > 1e-12: 326 at row 346, 312 / 348, 262 / 356, 222 / 364, 186 / 372); the cut below keeps 4 .. 19 columns
# clear of it.  The thick rows of case 0 keep the columns 58 .. 167.  The Kramers pair needs none.
DOMAIN_CUT = {'case0': (344, 5.5, 4)}
SEED = 20261018
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gn_reference.npz')
DETECTOR_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dex-ct-sim_amd', 'input', 'detector',
                             'eta_eid_mv.bin')


def tables(pair):
    """(i0 [2, nE], mus [2, nE]) of a table pair: 'case0' = golden case 0, 'kramers' = the Kramers 140 / 80 pair of
    tests/test_gpu_gn.py::test_short_cut_on_poisson_counts_of_physical_spectra at 1e5 photons."""
    if pair == 'case0':
        g = np.load(GOLDEN_FILE)
        return g['gn0_i0'], g['gn0_mus']
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md, synthetic
    ct = dx.FanBeamGeometry(N_channels=8, N_proj=8, eid=True, detector_file=DETECTOR_FILE)
    _, i0, mus = md.decomposition_tables(ct, synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80))
    return i0 * (1e5 / i0.sum(axis=1, keepdims=True)), mus


def domain(head, cut=None):
    """(i_lo, i_hi, j_lo, j_hi [n]): the cells of the domain, ends included - rows from the first open ring to the cell that
    holds GATE_U_MAX (the first row the host closes for photon starvation), columns inside the physical ratios: j_lo ..
    j_hi[i] in row i (``cut``: an entry of DOMAIN_CUT)."""
    n = int(head[3])
    i_hi = int(np.floor((np.log(quadrature.GATE_U_MAX) - head[4]) * head[5]))
    j_hi = np.full(n, int(np.floor(FY_HI * n)) - 1)
    if cut is not None:
        row, slope, offset = cut
        i = np.arange(row, n)
        j_hi[row:] -= np.ceil(slope * (i - row)).astype(np.int64) + offset
    return FX_LO, i_hi, int(np.ceil(FY_LO * n)), j_hi


def _below(x):
    """The largest double below x."""
    return np.nextafter(np.asarray(x, dtype=np.float64), -np.inf)


def _set(fx, fy, ci, cj):
    fx, fy = np.broadcast_arrays(np.asarray(fx, dtype=np.float64), np.asarray(fy, dtype=np.float64))
    return {'fxy': np.stack([fx.ravel(), fy.ravel()], axis=1),
            'cell': np.stack([np.broadcast_to(ci, fx.shape).ravel(), np.broadcast_to(cj, fx.shape).ravel()], axis=1).astype(np.int64)}


def point_sets(head, seed, tables=None, cut=None):
    """Named sets of points of the plane: name -> {'fxy' [m, 2] the points, 'cell' [m, 2] the cell (i, j) each is aimed at - the
    one floor() puts it in on the host; -1 for a coordinate outside the grid}.  ``tables`` = (i0, mus): needed for the water
    line of ``ratio_rim`` (left out without); ``cut``: see ``domain``.

    interior   one uniformly random point in every 4th cell of the domain in each direction (offset of the cells: seeded)
    corners0,  the same cells - one colour of their checkerboard each, so that a set stays below 15 000 points - at wx = wy = 0,
    corners1   and at the largest doubles below the next node in x, in y and in both: the device's logarithm may put such a point
               in either neighbour, and both answers must be right
    edges      the same cells at wx = 0 with random wy, and the transpose
    thick      every cell of the last three rows below GATE_U_MAX and of the row that holds it (closed by the host)
    ratio_rim  every cell of the column that holds 0.15 n and of the one after the domain's last (the one that holds 0.85 n where
               the domain is not cut), and one point of the water line a1 = -0.016 a0 in every cell it crosses inside the domain
    border     fx in {-1e-9, 0, 1e-9, 2 -+ 1e-9, 3, n - 3, n - 2 -+ 1e-9, n - 1e-9, n, n + 1e-9} against a strided fy, and the
               transpose: outside the grid, both closed rings, the first open ring.  The one set outside the domain."""
    n = int(head[3])
    rng = np.random.default_rng(seed)
    i_lo, i_hi, j_lo, j_top = domain(head, cut)
    j_hi = int(j_top.max())
    oi, oj = rng.integers(0, 4, size=2)
    ci, cj = np.meshgrid(np.arange(i_lo + oi, i_hi + 1, 4), np.arange(j_lo + oj, j_hi + 1, 4), indexing='ij')
    colour = (((ci - ci.min()) // 4 + (cj - cj.min()) // 4) % 2).ravel()
    ci, cj = ci.ravel(), cj.ravel()
    keep = cj <= j_top[ci]
    ci, cj, colour = ci[keep], cj[keep], colour[keep]
    # (wx, wy in (0, 1): never on a node, whatever the generator returns)
    inside = lambda m: np.clip(rng.random(m), 1e-6, 1.0 - 1e-6)
    sets = {'interior': _set(ci + inside(ci.size), cj + inside(ci.size), ci, cj)}
    for c in (0, 1):
        ki, kj = ci[colour == c], cj[colour == c]
        sets[f'corners{c}'] = _set(np.concatenate([ki, _below(ki + 1.0), ki, _below(ki + 1.0)]),
                                   np.concatenate([kj, kj, _below(kj + 1.0), _below(kj + 1.0)]), np.tile(ki, 4), np.tile(kj, 4))
    sets['edges'] = _set(np.concatenate([ci, ci + inside(ci.size)]), np.concatenate([cj + inside(ci.size), cj]),
                         np.tile(ci, 2), np.tile(cj, 2))
    ti, tj = np.meshgrid(np.arange(i_hi - 3, i_hi + 1), np.arange(j_lo, j_hi + 1), indexing='ij')
    ti, tj = ti.ravel(), tj.ravel()
    keep = tj <= j_top[ti]
    ti, tj = ti[keep], tj[keep]
    sets['thick'] = _set(ti + inside(ti.size), tj + inside(ti.size), ti, tj)
    rows = np.arange(i_lo, i_hi + 1)
    ri = np.tile(rows, 2)
    rj = np.concatenate([np.full(rows.size, int(np.floor(FY_LO * n))), j_top[rows] + 1])
    rim = _set(ri + inside(ri.size), rj + inside(ri.size), ri, rj)
    if tables is not None:
        i0, mus = (np.asarray(x, dtype=np.float64) for x in tables)
        a0 = np.geomspace(1e-4, 200.0, 200001)
        with np.errstate(all='ignore'):
            g = np.exp(-(np.stack([a0, -0.016 * a0], axis=1) @ mus)) @ i0.T
            wx_, wy_ = plane_of(head, g)
        ok = np.isfinite(wx_) & np.isfinite(wy_)
        wi, wj = np.floor(np.where(ok, wx_, -1.0)).astype(np.int64), np.floor(np.where(ok, wy_, -1.0)).astype(np.int64)
        ok &= (wi >= i_lo) & (wi <= i_hi) & (wj >= 0) & (wj < n)
        # the middle one of the samples that fall into a cell
        cells, first, count = np.unique(wi[ok] * n + wj[ok], return_index=True, return_counts=True)
        pick = np.flatnonzero(ok)[first + count // 2]
        water = _set(wx_[pick], wy_[pick], wi[pick], wj[pick])
        rim = {k: np.concatenate([rim[k], water[k]]) for k in rim}
    sets['ratio_rim'] = rim
    bx = np.array([-1e-9, 0.0, 1e-9, 2.0 - 1e-9, 2.0 + 1e-9, 3.0, n - 3.0, n - 2.0 - 1e-9, n - 2.0 + 1e-9, n - 1e-9, float(n), n + 1e-9])
    sy = np.arange(j_lo + oj, j_hi + 1, 4)
    sy = sy + inside(sy.size)
    sx = np.arange(i_lo + oi, i_hi + 1, 4)
    sx = sx + inside(sx.size)
    px, py = np.meshgrid(bx, sy, indexing='ij')
    qx, qy = np.meshgrid(sx, bx, indexing='ij')
    fx, fy = np.concatenate([px.ravel(), qx.ravel()]), np.concatenate([py.ravel(), qy.ravel()])
    cell = lambda f: np.where((f >= 0.0) & (f < n), np.floor(f), -1.0)
    sets['border'] = _set(fx, fy, cell(fx), cell(fy))
    return sets


def interleave(sets, seed):
    """One pixel order for a launch of all the sets: (set index [N], index within the set [N], names).  The points of every set
    but ``border`` in a seeded random order; runs of ``border`` points of every length 0 .. 64 (in a seeded order; the set is
    walked cyclically) are placed between them, each directly after an ``interior`` point.  Border points are stashed and
    walked by the kernel, so its waves meet the stash's drain threshold at different fills.  Every point of every set
    appears; N is odd (no multiple of the wave or of a tile)."""
    names = list(sets)
    rng = np.random.default_rng(seed)
    b = names.index('border')
    n_b = len(sets['border']['fxy'])
    rest = np.concatenate([np.stack([np.full(len(sets[s]['fxy']), k), np.arange(len(sets[s]['fxy']))], axis=1)
                           for k, s in enumerate(names) if k != b])
    rest = rest[rng.permutation(len(rest))]
    lengths = rng.permutation(65)
    if lengths.sum() < n_b:                                               # every border point at least once
        lengths = np.concatenate([lengths, np.full(-(-(n_b - lengths.sum()) // 64), 64)])
    if (len(rest) + lengths.sum()) % 2 == 0:                              # one more run of one point: N is odd
        lengths = np.concatenate([lengths, [1]])
    at_interior = np.flatnonzero(rest[:, 0] == names.index('interior'))
    after = at_interior[np.linspace(0, len(at_interior) - 1, len(lengths)).astype(np.int64)]
    pieces, pos, taken = [], 0, 0
    for where, m in zip(after, lengths):
        pieces.append(rest[pos:where + 1])
        pieces.append(np.stack([np.full(m, b), (taken + np.arange(m)) % n_b], axis=1))
        pos, taken = where + 1, taken + m
    pieces.append(rest[pos:])
    order = np.concatenate(pieces)
    return order[:, 0].astype(np.int64), order[:, 1].astype(np.int64), names


def gather(sets, order):
    """The points [N, 2] of an order of ``interleave``."""
    which, idx, names = order
    out = np.empty((len(which), 2))
    for k, s in enumerate(names):
        m = which == k
        out[m] = sets[s]['fxy'][idx[m]]
    return out
