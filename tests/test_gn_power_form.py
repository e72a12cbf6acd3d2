"""The power form of the short cut's start value (matdecomp.power_form, csrc/gn.hip gn_start<DERIV>): per cell the
coefficients of the same 6 x 6 Lagrange interpolant of the corners' fixed points.  Evaluated by Horner with the derivatives
carried along - as the kernel does - it must give the Lagrange form's value and both derivatives (hence s and B) to rounding."""
import numpy as np
import torch

from dex_ct_sim_amd import matdecomp as md, quadrature as q


def _table(n, seed=3):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing='ij')
    a0 = 3.0 + np.exp(0.7 * x) * np.cos(2.1 * y) + 0.01 * rng.standard_normal(x.shape)     # smooth plus corner-level noise
    a1 = -0.5 + 20.0 * np.sin(1.3 * x + 0.4 * y) + 0.01 * rng.standard_normal(x.shape)
    head = np.zeros(q.START_HEADER)
    head[3] = n
    roots = np.stack([a0, a1], -1)
    cells = np.ones((n, n, 2))
    start = np.concatenate([head, roots.reshape(-1), cells.reshape(-1)])
    return start, roots


def _lagrange(roots, n, i, j, wx, wy):
    """gn_start's Lagrange form (nodes -2 .. 3), with its derivatives along wx and wy."""
    nodes = np.arange(-2.0, 4.0)

    def w(t):
        val, der = np.zeros(6), np.zeros(6)
        for a in range(6):
            others = [b for b in range(6) if b != a]
            den = np.prod([nodes[a] - nodes[b] for b in others])
            val[a] = np.prod([t - nodes[b] for b in others]) / den
            der[a] = sum(np.prod([t - nodes[c] for c in others if c != b]) for b in others) / den
        return val, der
    cx, dx = w(wx)
    cy, dy = w(wy)
    bi, bj = min(max(i - 2, 0), n - 5), min(max(j - 2, 0), n - 5)
    r = roots[bi:bi + 6, bj:bj + 6]
    return (np.einsum('p,q,pqk->k', cx, cy, r), np.einsum('p,q,pqk->k', dx, cy, r), np.einsum('p,q,pqk->k', cx, dy, r))


def _horner(c, wx, wy):
    """The kernel's evaluation order: rows by Horner along wy (derivative carried), then along wx."""
    rows = []
    for a in range(6):
        p, d = c[a, 5].copy(), c[a, 5].copy()
        p = p * wy + c[a, 4]
        for b in range(3, -1, -1):
            d = d * wy + p
            p = p * wy + c[a, b]
        rows.append((p, d))
    v, vy = rows[5]
    vx = v.copy()
    v, vy = v * wx + rows[4][0], vy * wx + rows[4][1]
    for a in range(3, -1, -1):
        vx = vx * wx + v
        v = v * wx + rows[a][0]
        vy = vy * wx + rows[a][1]
    return v, vx, vy


def test_power_form_layout_leaves_the_table_alone():
    n = 12
    start, _ = _table(n)
    out = md.power_form(torch.from_numpy(start)).numpy()
    off = int(out[11])
    assert off % 2 == 0 and off >= start.size and out.size == off + n * n * 36 * 2
    keep = np.r_[0:11, 12:start.size]
    assert np.array_equal(out[keep], start[keep])


def test_power_form_matches_lagrange_to_rounding():
    n = 16
    start, roots = _table(n)
    out = md.power_form(torch.from_numpy(start)).numpy()
    coef = out[int(out[11]):].reshape(n, n, 6, 6, 2)
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(400):
        i, j = rng.integers(2, n - 2, size=2)                     # the open cells: two away from the border
        wx, wy = rng.random(2)
        want = _lagrange(roots, n, i, j, wx, wy)
        got = _horner(coef[i, j], wx, wy)
        for g, w_ in zip(got, want):
            worst = max(worst, float(np.max(np.abs(g - w_) / np.maximum(np.abs(w_), 1.0))))
    assert worst < 1e-13, worst
    # the cells at the border use the same clamped window as the Lagrange form
    for i, j in ((0, 0), (1, n - 1), (n - 1, 3)):
        want, got = _lagrange(roots, n, i, j, 0.3, 0.6), _horner(coef[i, j], 0.3, 0.6)
        assert all(np.allclose(g, w_, rtol=1e-10, atol=1e-10) for g, w_ in zip(got, want))
