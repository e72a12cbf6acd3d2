"""NumPy float64 restatement of the Newton decomposition for K >= M (matdecomp.py:114-125 of the reference, per pixel), and the
synthetic tables the goldens (tests/golden/make_goldens_multi.py) and the tests of dexct_gn_decompose_multi share.

Nothing here touches the HIP library: tests/test_gn_multi_refs.py pins this module to arrays the real reference produced
(tests/golden/ref_multi.npz), and the GPU tests (tests/test_gpu_gn_multi.py) then use it where no golden exists.
"""
import numpy as np

# (K, M) the kernel is instantiated for
SHAPES = ((2, 2), (3, 2), (4, 2), (3, 3), (4, 3))
# energy-bin edges [keV] of the synthetic photon-counting detector per number of measurements
EDGES = {2: (20.0, 60.0, 141.0), 3: (20.0, 50.0, 75.0, 141.0), 4: (20.0, 45.0, 60.0, 85.0, 141.0)}
# upper ends of the uniform line integrals [g/cm^2]: water-like, bone-like, K-edge material
A_MAX = (20.0, 3.0, 0.05)


def newton_solve_multi(sino_gg, i0, mus, n_iters):
    """sino_gg [K, ...] counts, i0 [K, nE], mus [M, nE] -> [..., M]: n_iters Newton steps from 1e-6 per pixel, each the full
    Newton step on the Poisson likelihood incl. the (g/nu - 1) second-derivative term, solved with np.linalg.solve per pixel.
    A pixel whose Hessian is singular or non-finite ends NaN; no other pixel is affected."""
    g = np.asarray(sino_gg, dtype=np.float64)
    i0 = np.asarray(i0, dtype=np.float64)
    mus = np.asarray(mus, dtype=np.float64)
    K, M, nE = g.shape[0], mus.shape[0], mus.shape[1]
    assert i0.shape == (K, nE) and K >= M
    shape = g.shape[1:]
    g = g.reshape(K, -1).T                                                   # [P, K]
    w1 = (i0[:, None, :] * mus[None, :, :]).reshape(K * M, nE)               # i0_k mu_m
    w2 = (i0[:, None, None, :] * (mus[None, :, :] * mus[:, None, :])[None]).reshape(K * M * M, nE)   # i0_k (mu_m mu_n)
    a = np.full((g.shape[0], M), 1e-6)
    with np.errstate(all='ignore'):
        for _ in range(int(n_iters)):
            at = np.exp(np.clip(-(a @ mus), -700.0, 700.0))                  # [P, nE]
            nu = at @ i0.T                                                   # [P, K]
            G = (at @ w1.T).reshape(-1, K, M)                                # = -nu_grad
            S = (at @ w2.T).reshape(-1, K, M, M)                             # = nu_hess
            c = g / nu - 1.0
            q = g / (nu * nu)
            dF = np.einsum('pk,pkm->pm', c, G)
            H = np.einsum('pk,pkm,pkn->pmn', q, G, G) - np.einsum('pk,pkmn->pmn', c, S)
            step = np.full_like(a, np.nan)
            ok = np.flatnonzero(np.all(np.isfinite(H), axis=(1, 2)) & np.all(np.isfinite(dF), axis=1))
            try:                                          # one LAPACK solve per pixel (the stacked form of np.linalg.solve)
                step[ok] = np.linalg.solve(H[ok], dF[ok][..., None])[..., 0]
            except np.linalg.LinAlgError:                 # some pixel is exactly singular: find it, keep the others
                for p in ok:
                    try:
                        step[p] = np.linalg.solve(H[p], dF[p])
                    except np.linalg.LinAlgError:
                        pass
            a = a - step
    return a.reshape(shape + (M,))


def synthetic_tables(n_energies=60):
    """(E, mus [3, nE], S [nE]): a water-like, a bone-like and a K-edge (33.2 keV) material on linspace(20, 140, nE), and a
    tungsten-like spectrum.  The K-edge is what makes a third basis identifiable."""
    E = np.linspace(20.0, 140.0, int(n_energies))
    pe = (30.0 / E) ** 3
    kn = 1.0 / (1.0 + E / 250.0)
    mu_w = 0.02 * pe + 0.18 * kn
    mu_b = 0.25 * pe + 0.17 * kn
    mu_i = np.where(E >= 33.2, 6.0, 1.2) * (33.2 / E) ** 2.7 + 0.15 * kn
    S = 1e3 * np.maximum(140.0 - E, 0.0) * np.exp(-0.9 * pe)
    return E, np.stack([mu_w, mu_b, mu_i]), S


def synthetic_bins(E, S, edges):
    """i0 [K, nE]: the spectrum seen through K soft-edged energy windows (3 keV tanh edges)."""
    return np.stack([S * (np.tanh((E - lo) / 3.0) - np.tanh((E - hi) / 3.0)) / 2.0 for lo, hi in zip(edges[:-1], edges[1:])])


def forward_counts(a, i0, mus):
    """counts [K, ...] = sum_e i0[k, e] exp(-sum_m a[..., m] mus[m, e])"""
    ex = np.exp(-np.tensordot(np.asarray(a, dtype=np.float64), mus, axes=([-1], [0])))
    return np.stack([np.sum(i0[k] * ex, axis=-1) for k in range(i0.shape[0])])


def noisy(g, rng):
    """g + sqrt(g) z, clipped at 1e-3"""
    return np.maximum(g + np.sqrt(g) * rng.standard_normal(g.shape), 1e-3)


def sweep_case(K, M, n_energies, n_pix=1000, seed=7):
    """(counts [K, n_pix] float64, i0 [K, nE], mus [M, nE]) of the GPU shape sweep: the synthetic tables resampled to
    n_energies at the same total flux, line integrals uniform in [0, A_MAX], quantum noise.  tests/test_gn_multi_refs.py shows that these inputs
    are well conditioned (reversing the energies moves the restatement's result by less than 1e-12)."""
    E, mus3, S = synthetic_tables(n_energies)
    i0 = synthetic_bins(E, S * (60.0 / n_energies), EDGES[K])      # the flux of the 60-energy tables on any grid
    mus = np.ascontiguousarray(mus3[:M])
    rng = np.random.default_rng([seed, K, M, n_energies])
    a_true = rng.uniform(0.0, 1.0, (n_pix, M)) * np.array(A_MAX[:M])
    return noisy(forward_counts(a_true, i0, mus), rng), i0, mus


def rel_err(a, ref):
    """max over pixels and components of |a - ref| / max(|ref|, 1); NaN anywhere gives NaN"""
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref), 1.0))) if np.size(ref) else 0.0


def load_goldens(path):
    """The cases of tests/golden/ref_multi.npz (make_goldens_multi.py) as a list of dicts: name, g [K, 4, 16], i0, mus and the
    real reference's results a[30], a[50] ([4, 16, M])."""
    out = []
    with np.load(path) as z:
        for name, tables, k in zip(z['cases'], z['tables'], z['index']):
            a30 = z[f'{tables}_a30'][k]
            out.append({'name': str(name), 'g': z[f'{tables}_g'][k], 'i0': z[f'{tables}_i0'], 'mus': z[f'{tables}_mus'],
                        'a': {30: a30, 50: a30 + z[f'{tables}_d50'][k]}})
    return out
