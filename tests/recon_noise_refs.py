"""NumPy float64 references of the noise propagation through the FBP (include/dexct.h, dexct_fbp_var_filter and its two
back-projections; back_project.get_recon_covariance), no HIP.

The FBP is linear, image = M sino.  For independent sinogram pixels with (co)variance s the (co)variance of an image pixel is
(M o M) s, the element-wise square of the FBP matrix applied to s.  Two independent routes to it:

  variance_recon, variance_fdk   the closed forms: with the filter q[n] = dg sum_m p[m] W_m g[n - m] and the interpolation
                                 (1 - w) q[k] + w q[k + 1] of oracle/fbp_oracle.py,
                                     A[n] = dg^2 sum_m s[m] W_m^2 P_m^2 g[n - m]^2              var(q[n])
                                     B[n] = dg^2 sum_m s[m] W_m^2 P_m^2 g[n - m] g[n + 1 - m]   cov(q[n], q[n + 1])
                                     K s  = dbeta^2 sum_views [(1 - w)^2 A[k] + w^2 A[k + 1] + 2 w (1 - w) B[k]] / L^4
                                 (P = 2 w_Parker of a short scan, else 1), written with the oracle's ramp_taps, parker_weights
                                 and pixel geometry; Feldkamp adds the row interpolation, whose two rows are independent.
  operator_matrix                M itself, column by column, from unit impulses through fbp_oracle.get_recon / fdk_recon -
                                 nothing of the closed form enters.
tests/test_recon_noise_refs.py holds one against the other; the GPU tests hold the kernels against the closed forms.
"""
import numpy as np

from oracle import fbp_oracle as fo


def fan(n_views, n_channels, gamma_fan, theta_tot=2 * np.pi):
    """(thetas, gammas) of FanBeamGeometry(N_channels, N_proj, gamma_fan, theta_tot=...)."""
    dg = gamma_fan / n_channels
    return np.arange(n_views) * (theta_tot / n_views), (np.arange(n_channels) - 0.5 * (n_channels - 1)) * dg


def _planes(s, lead):
    """s [lead axes..., extra axes...] -> ([lead..., P], extra shape)"""
    s = np.asarray(s, dtype=np.float64)
    extra = s.shape[lead:]
    return s.reshape(s.shape[:lead] + (-1,)), extra


def filter_variance(s, thetas, gammas, sid, ramp=1.0, window='rect', theta_tot=None):
    """s [n_views, ..., n_channels, P] -> (A, B) of the same shape: variance of the filtered samples and covariance of
    neighbouring ones (B of the last channel is 0)."""
    n = s.shape[-2]
    dg = float(gammas[1] - gammas[0])
    g = fo.ramp_taps(n, dg, ramp, window)
    G = g[np.arange(n)[:, None] - np.arange(n)[None, :] + (n - 1)]                 # G[n, m] = g[n - m]
    GG = np.zeros_like(G)
    GG[:-1] = G[:-1] * G[1:]                                                        # g[n - m] g[n + 1 - m]
    p = np.ones((len(thetas), n))
    if theta_tot is not None and theta_tot < 2 * np.pi - 1e-9:
        p = 2.0 * fo.parker_weights(thetas, gammas, theta_tot)
    p = p.reshape((len(thetas),) + (1,) * (s.ndim - 3) + (n, 1))
    wl = s * ((sid * np.cos(gammas)) ** 2)[:, None] * p ** 2
    return dg * dg * np.einsum('...mp,nm->...np', wl, G * G), dg * dg * np.einsum('...mp,nm->...np', wl, GG)


def _views(thetas, gammas, sid, n_matrix, fov, n_ch):
    """per view: (kk, w, ok, l2) of every pixel, the arithmetic of fbp_oracle.back_project"""
    dg = float(gammas[1] - gammas[0])
    c = (np.arange(n_matrix) - n_matrix / 2 + 0.5) * (fov / n_matrix)
    x, y = np.meshgrid(c, c)
    for th in thetas:
        cb, sb = np.cos(th), np.sin(th)
        dx, dy = x - sid * cb, y - sid * sb
        gam = np.arctan2(-cb * dy + sb * dx, -(cb * dx + sb * dy))
        pos = gam / dg + 0.5 * (n_ch - 1)
        k = np.floor(pos).astype(np.int64)
        yield np.clip(k, 0, n_ch - 2), pos - k, (k >= 0) & (k < n_ch - 1), dx * dx + dy * dy


def _dbeta(thetas):
    return float(thetas[1] - thetas[0]) if len(thetas) > 1 else 2 * np.pi


def variance_recon(s, thetas, gammas, sid, n_matrix, fov, ramp=1.0, window='rect', theta_tot=None):
    """s [n_views, n_channels, ...] (trailing axes: planes) -> [n_matrix, n_matrix, ...]: the closed form of a fan-beam FBP."""
    s, extra = _planes(s, 2)
    A, B = filter_variance(s, thetas, gammas, sid, ramp, window, theta_tot)
    out = np.zeros((n_matrix, n_matrix, s.shape[-1]))
    for i, (kk, w, ok, l2) in enumerate(_views(thetas, gammas, sid, n_matrix, fov, s.shape[1])):
        w = w[..., None]
        val = (1 - w) ** 2 * A[i, kk] + w ** 2 * A[i, kk + 1] + 2 * w * (1 - w) * B[i, kk]
        out += np.where(ok[..., None], val / (l2 * l2)[..., None], 0.0)
    return (out * _dbeta(thetas) ** 2).reshape((n_matrix, n_matrix) + extra)


def variance_stack(s, *args, **kw):
    """s [n_views, n_rows, n_channels, T] -> [n_rows, n_matrix, n_matrix, T]: variance_recon row by row (a stacked fan)."""
    return np.stack([variance_recon(s[:, r], *args, **kw) for r in range(s.shape[1])])


def variance_fdk(s, thetas, gammas, sid, sdd, row_z, src_z, n_matrix, fov, ramp, slices_z, window='rect'):
    """s [n_views, n_rows, n_channels, ...] -> [len(slices_z), n_matrix, n_matrix, ...]: the closed form of fbp_oracle.fdk_recon."""
    s, extra = _planes(s, 3)
    n_views, n_rows, n_ch, _ = s.shape
    row_z = np.asarray(row_z, dtype=np.float64)
    A, B = filter_variance(s, thetas, gammas, sid, ramp, window)
    c2 = ((sdd / np.sqrt(sdd ** 2 + (row_z - src_z) ** 2)) ** 2)[:, None]           # squared cone weights
    dzr = float(row_z[1] - row_z[0])
    out = np.zeros((len(slices_z), n_matrix, n_matrix, s.shape[-1]))
    for i, (kk, w, ok, l2) in enumerate(_views(thetas, gammas, sid, n_matrix, fov, n_ch)):
        w = w[..., None]
        for s_i, z in enumerate(slices_z):
            rpos = (src_z + (z - src_z) * sdd / np.sqrt(l2) - row_z[0]) / dzr
            r0 = np.floor(rpos).astype(np.int64)
            wr = (rpos - r0)[..., None]
            okr = ok & (r0 >= 0) & (r0 < n_rows - 1)
            rr = np.clip(r0, 0, n_rows - 2)
            V = [(1 - w) ** 2 * A[i, r, kk] + w ** 2 * A[i, r, kk + 1] + 2 * w * (1 - w) * B[i, r, kk] for r in (rr, rr + 1)]
            val = (1 - wr) ** 2 * c2[rr] * V[0] + wr ** 2 * c2[rr + 1] * V[1]
            out[s_i] += np.where(okr[..., None], val / (l2 * l2)[..., None], 0.0)
    return (out * _dbeta(thetas) ** 2).reshape((len(slices_z), n_matrix, n_matrix) + extra)


def fdk_inside(thetas, gammas, sid, sdd, row_z, src_z, n_matrix, fov, slices_z):
    """[slices, views, n_matrix, n_matrix] bool: the (voxel, view) pairs that contribute - inside the fan and between two rows"""
    row_z = np.asarray(row_z, dtype=np.float64)
    out = np.zeros((len(slices_z), len(thetas), n_matrix, n_matrix), bool)
    for i, (_, _, ok, l2) in enumerate(_views(thetas, gammas, sid, n_matrix, fov, len(gammas))):
        for k, z in enumerate(slices_z):
            r0 = np.floor((src_z + (z - src_z) * sdd / np.sqrt(l2) - row_z[0]) / float(row_z[1] - row_z[0]))
            out[k, i] = ok & (r0 >= 0) & (r0 < len(row_z) - 1)
    return out


def operator_matrix(thetas, gammas, sid, n_matrix, fov, ramp=1.0, window='rect', theta_tot=None, fdk=None):
    """The FBP matrix M [image pixels, sinogram pixels] (both raveled in C order) from unit impulses through the oracle.
    ``fdk``: dict(sdd, row_z, src_z, slices_z) - the sinogram is then [n_views, n_rows, n_channels] and the image the volume."""
    n_views, n_ch = len(thetas), len(gammas)
    shape = (n_views, n_ch) if fdk is None else (n_views, len(fdk['row_z']), n_ch)
    cols = []
    for j in range(int(np.prod(shape))):
        e = np.zeros(shape)
        e.flat[j] = 1.0
        if fdk is None:
            img = fo.get_recon(e, thetas, gammas, sid, n_matrix, fov, ramp, window=window, theta_tot=theta_tot)[0]
        else:
            img = fo.fdk_recon(e, thetas, gammas, sid, fdk['sdd'], fdk['row_z'], fdk['src_z'], n_matrix, fov, ramp,
                               fdk['slices_z'], window=window)
        cols.append(img.ravel())
    return np.stack(cols, axis=1)


def squared_operator(M, s):
    """(M o M) s for s [sinogram shape..., P] -> [image pixels, P]"""
    s = np.asarray(s, dtype=np.float64)
    return (M * M) @ s.reshape(M.shape[1], -1)


# ---- the statistical case (CPU test 2 and GPU test 5 share it) ---------------------------------------------------------------------
STAT = dict(n_views=24, n_channels=48, gamma_fan=0.8230337, sid=60.0, n_matrix=32, fov=30.0, realisations=512)


def stat_problem():
    """(s, noise): the variance sinogram, uniform in (0.5, 4) 1e-4, and 512 Gaussian realisations [512, views, channels] with it."""
    rng = np.random.default_rng(20240607)
    s = rng.uniform(0.5e-4, 4e-4, (STAT['n_views'], STAT['n_channels']))
    noise = np.random.default_rng(977).standard_normal((STAT['realisations'],) + s.shape) * np.sqrt(s)
    return s, noise


def stat_check(images, predicted):
    """images [R, N, N]: reconstructions of the realisations.  (R - 1) ratio is chi^2 with R - 1 degrees of freedom per pixel:
    relative sd sqrt(2 / 511) = 6.26 %.  Returns (mean ratio, min, max) after asserting |mean - 1| <= 0.03 and every pixel within
    1 +- 0.375 (6 sigma)."""
    ratio = np.var(np.asarray(images, dtype=np.float64), axis=0, ddof=1) / predicted
    print(f'variance ratio: mean {ratio.mean():.4f}, range {ratio.min():.3f} .. {ratio.max():.3f}, sd {ratio.std():.4f}')
    assert abs(ratio.mean() - 1.0) <= 0.03, ratio.mean()
    assert np.all(np.abs(ratio - 1.0) <= 0.375), (ratio.min(), ratio.max())
    return ratio.mean(), ratio.min(), ratio.max()
