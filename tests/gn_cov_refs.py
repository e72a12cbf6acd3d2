"""NumPy restatement of the per-pixel noise covariance of the decomposition (include/dexct.h, dexct_gn_covariance), in float64
and in np.longdouble, and the inputs its tests share.  Nothing here touches the HIP library.

For a state a [M], spectra i0 [K, nE], variance weights i0v [K, nE] and basis attenuation mus [M, nE]:
    t = exp(clip(-a . mus, +-700));  nu = i0 t;  v = i0v t;  G_km = sum_e i0_k mu_m t
    estimator:  C = H^-1 (G^T diag(v / nu^2) G) H^-1,  H = G^T diag(1 / nu) G
    crlb:       C = (G^T diag(1 / v) G)^-1
with the inverse written out (2 x 2, 3 x 3 adjugate), so that the same code runs in either precision.  The synthetic tables,
bins, edges and ranges are those of tests/gn_multi_refs.py.
"""
import numpy as np

from gn_multi_refs import A_MAX, EDGES, SHAPES, synthetic_bins, synthetic_tables  # noqa: F401  (shared with the tests)

KINDS = ('estimator', 'crlb')
EPS = 2.0 ** -53
LD = np.longdouble


def tri_index(M):
    """[(i, j)] of the row-major upper triangle"""
    return [(i, j) for i in range(M) for j in range(i, M)]


def variance_weights(i0, E, eid):
    """i0v: i0 x E/60 for the energy-integrating variant of the synthetic detector (its signal per photon is E/60), i0 for the
    counting one"""
    return i0 * (E / 60.0) if eid else i0.copy()


def tables(K, M, n_energies=60, eid=False, flux=1.0):
    """(i0, i0v, mus) of the synthetic K-bin detector on n_energies, at the total flux of the 60-energy tables times ``flux``"""
    E, mus3, S = synthetic_tables(n_energies)
    i0 = synthetic_bins(E, S * (60.0 / n_energies) * flux, EDGES[K])
    return i0, variance_weights(i0, E, eid), np.ascontiguousarray(mus3[:M])


def sums(a, i0, i0v, mus, dtype=np.float64):
    """nu [P, K], v [P, K], G [P, K, M] at the states a [P, M], in ``dtype``"""
    a, i0, i0v, mus = (np.asarray(x, dtype=dtype) for x in (a, i0, i0v, mus))
    lim = dtype(700.0)
    with np.errstate(all='ignore'):
        t = np.exp(np.clip(-(a @ mus), -lim, lim))                            # [P, nE]
        nu = t @ i0.T
        v = t @ i0v.T
        K, M = i0.shape[0], mus.shape[0]
        G = (t @ (i0[:, None, :] * mus[None, :, :]).reshape(K * M, -1).T).reshape(-1, K, M)
    return nu, v, G


def sym_inverse(h):
    """inverse of the symmetric matrices h [P, M, M], M = 2 or 3, by the adjugate (any float dtype); singular -> inf / NaN"""
    M = h.shape[-1]
    out = np.empty_like(h)
    with np.errstate(all='ignore'):
        if M == 2:
            h00, h01, h11 = h[:, 0, 0], h[:, 0, 1], h[:, 1, 1]
            det = h00 * h11 - h01 * h01
            out[:, 0, 0], out[:, 0, 1], out[:, 1, 1] = h11 / det, -h01 / det, h00 / det
            out[:, 1, 0] = out[:, 0, 1]
            return out
        assert M == 3
        h00, h01, h02, h11, h12, h22 = h[:, 0, 0], h[:, 0, 1], h[:, 0, 2], h[:, 1, 1], h[:, 1, 2], h[:, 2, 2]
        c00, c01, c02 = h11 * h22 - h12 * h12, h02 * h12 - h01 * h22, h01 * h12 - h02 * h11
        c11, c12, c22 = h00 * h22 - h02 * h02, h01 * h02 - h00 * h12, h00 * h11 - h01 * h01
        det = (h00 * c00 + h01 * c01) + h02 * c02
        for (i, j), c in zip(tri_index(3), (c00, c01, c02, c11, c12, c22)):
            out[:, i, j] = out[:, j, i] = c / det
    return out


def covariance_full(a, i0, i0v, mus, kind='estimator', dtype=np.float64):
    """C [P, M, M] at the states a [P, M]"""
    assert kind in KINDS
    nu, v, G = sums(np.atleast_2d(a), i0, i0v, mus, dtype)
    with np.errstate(all='ignore'):
        if kind == 'crlb':
            return sym_inverse(np.einsum('pk,pkm,pkn->pmn', 1.0 / v, G, G))
        Hi = sym_inverse(np.einsum('pk,pkm,pkn->pmn', 1.0 / nu, G, G))
        B = np.einsum('pk,pkm,pkn->pmn', v / (nu * nu), G, G)
        return Hi @ B @ Hi


def pack(C):
    """[P, M, M] -> [P, T], the row-major upper triangle"""
    return np.stack([C[:, i, j] for i, j in tri_index(C.shape[-1])], axis=-1)


def covariance(a, i0, i0v, mus, kind='estimator', dtype=np.float64):
    """C [P, T] packed like out_cov of dexct_gn_covariance"""
    return pack(covariance_full(a, i0, i0v, mus, kind, dtype))


def corr_cond(C_full):
    """2-norm condition number per pixel of the correlation matrix of C [P, M, M] (float64 is enough for a factor)"""
    C = np.asarray(C_full, dtype=np.float64)
    d = np.sqrt(np.einsum('pii->pi', C))
    return np.linalg.cond(C / (d[:, :, None] * d[:, None, :]))


def error_ratio(C_packed, C_ld_full):
    """max over pixels and elements of |C - C_ld|_ij / (cond(corr_p) 2^-53 sqrt(C_ii C_jj)): the ``c`` a result needs in the
    bound |C - C_ld|_ij <= c cond(corr_p) 2^-53 sqrt(C_ii C_jj).  C_ld_full [P, M, M] long double; NaN anywhere gives NaN."""
    M = C_ld_full.shape[-1]
    d = np.sqrt(np.einsum('pii->pi', C_ld_full))
    cond = corr_cond(C_ld_full).astype(LD)
    worst = 0.0
    for t, (i, j) in enumerate(tri_index(M)):
        r = np.abs(np.asarray(C_packed[:, t], dtype=LD) - C_ld_full[:, i, j]) / (cond * LD(EPS) * d[:, i] * d[:, j])
        if not np.all(np.isfinite(r)):
            return float('nan')
        worst = max(worst, float(np.max(r)))
    return worst


SWEEP_ENERGIES = (8, 60, 239)
SWEEP_PIXELS = (1, 63, 64, 65, 257, 1000)
_sweep = {}


def sweep_case(K, M, n_energies, eid=True, n_pix=1000, seed=11):
    """(a [n_pix, M], i0, i0v, mus): the GPU sweep's inputs - states uniform in [0, A_MAX] on the synthetic tables.  Pixels are
    independent, so every smaller size is a prefix.  Energy-integrating by default, so that the two kinds differ for K > M."""
    key = (K, M, n_energies, eid, n_pix, seed)
    if key not in _sweep:
        i0, i0v, mus = tables(K, M, n_energies, eid)
        rng = np.random.default_rng([seed, K, M, n_energies])
        _sweep[key] = (rng.uniform(0.0, 1.0, (n_pix, M)) * np.array(A_MAX[:M]), i0, i0v, mus)
    return _sweep[key]


def sweep_ratio_f64():
    """{(K, M, nE, kind): error_ratio of the FLOAT64 restatement against the long-double one} over the whole sweep - shapes x
    SWEEP_ENERGIES x 1000 pixels x both kinds.  Its maximum (4.91 on x86-64 with 80-bit long double) is the yardstick of the
    device test: the kernel is allowed 4 x that (another summation order, a refined hardware reciprocal, a table exponential)."""
    out = {}
    for K, M in SHAPES:
        for n_e in SWEEP_ENERGIES:
            a, i0, i0v, mus = sweep_case(K, M, n_e)
            for kind in KINDS:
                out[(K, M, n_e, kind)] = error_ratio(covariance(a, i0, i0v, mus, kind), covariance_full(a, i0, i0v, mus, kind, LD))
    return out
