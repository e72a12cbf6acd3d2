"""Fan-beam filtered back-projection: drop-in for the reference's ``xtomosim.back_project.get_recon``.

``recon_raw, recon_HU = get_recon(sino, ct, spec, N_matrix, FOV, ramp)`` is called at main.py:134 (log
sinogram of one spectrum) and main.py:168 (basis-material sinograms, ``spec`` a filler there).  The
reference source is in the un-vendored x-tomo-sim submodule; README.md:30-31 describes it as fan-beam
FBP with a windowed ramp filter.  This build implements Kak & Slaney 3.4.1 for the equiangular fan of
``FanBeamGeometry`` (see oracle/fbp_oracle.py for the formulas): ``ramp`` is the cutoff of the
band-limited ramp as a fraction of the Nyquist frequency (``ramp_filter_percent_Nyquist``,
input/params.txt:35), ``recon_raw`` is in 1/cm on an ``N_matrix`` x ``N_matrix`` grid over ``FOV`` cm,
``recon_HU = 1000 (raw - mu_w) / mu_w`` with the spectrum- and detector-weighted water attenuation.
The convolution and the back-projection run in the HIP library (dexct_fbp_filter, dexct_fbp_backproject).  Rotations shorter than 2 pi (``rotation_angle_total``,
input/params.txt:24) down to pi + the fan angle are reconstructed with Parker's short-scan weights (dexct_fbp_parker).
"""
import numpy as np
import torch

from . import _device, _native, iterative, xcompy
from ._device import dense_input, device, gpu_of, ptr, stream_ptr, to_dev, to_host
from .forward_project import effective_weights

WATER = 'H(11.2)O(88.8)'       # the composition plots.py:140 uses for HU


WINDOWS = {                      # apodisation W(x), x = f / f_cutoff in [0, 1], applied to the ramp |f|
    'rect': None,                                                        # band-limited ramp (Ram-Lak)
    'sinc': lambda x: np.sinc(0.5 * x),                                  # Shepp-Logan: sin(pi x / 2) / (pi x / 2)
    'cosine': lambda x: np.cos(0.5 * np.pi * x),
    'hann': lambda x: 0.5 * (1.0 + np.cos(np.pi * x)),
    'hamming': lambda x: 0.54 + 0.46 * np.cos(np.pi * x),
}


def default_window():
    """The reference's README (README.md:30-31) speaks of "a sinc window filter"; its source is not available, so
    the plain band-limited ramp stays the default and the window is a choice (``DEXCT_FBP_WINDOW``)."""
    import os
    return os.environ.get('DEXCT_FBP_WINDOW', 'rect')


def _window(window, default=True):
    """The name of the ramp's window: ``default_window()`` where the caller named none (unless ``default`` is off), a ValueError
    for a name WINDOWS does not have."""
    if default:
        window = window or default_window()
    if window not in WINDOWS:
        raise ValueError(f'unknown filter window {window!r}; choose from {sorted(WINDOWS)}')
    return window


def _windowed_ramp(t, fc, window):
    """h(t) = 2 int_0^fc f W(f / fc) cos(2 pi f t) df for an array of lags t, by Gauss-Legendre panels shorter
    than half a period of the fastest cosine (float64, error ~1e-15 of h(0))."""
    t = np.asarray(t, dtype=np.float64)
    n_panels = int(np.ceil(4.0 * fc * np.max(np.abs(t)))) + 2
    x, w = np.polynomial.legendre.leggauss(12)
    edges = np.linspace(0.0, fc, n_panels + 1)
    half = 0.5 * (edges[1:] - edges[:-1])
    f = (0.5 * (edges[1:] + edges[:-1])[:, None] + half[:, None] * x[None, :]).ravel()       # nodes
    wf = (half[:, None] * w[None, :]).ravel() * f * window(f / fc)
    out = np.empty(t.shape)
    step = max(1, int(4e6 // f.size))
    for i in range(0, t.size, step):
        out[i:i + step] = 2.0 * (np.cos(2.0 * np.pi * t[i:i + step, None] * f[None, :]) @ wf)
    return out


def ramp_taps(n_channels, dgamma, ramp=1.0, window='rect'):
    """Equiangular filter taps g(n dgamma), n = -(N-1)..(N-1), cutoff ``ramp`` x Nyquist (float64);
    ``window`` apodises the ramp below the cutoff (WINDOWS)."""
    window = _window(window, default=False)
    n = np.arange(-(n_channels - 1), n_channels, dtype=np.float64)
    c = float(ramp)
    t = n * dgamma
    if WINDOWS[window] is None:
        h = (c * c / (2 * dgamma ** 2)) * np.sinc(c * n) - (c * c / (4 * dgamma ** 2)) * np.sinc(c * n / 2) ** 2
    else:
        pos = _windowed_ramp(t[n_channels - 1:], c / (2.0 * dgamma), WINDOWS[window])      # h is even in t
        h = np.concatenate([pos[:0:-1], pos])
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(n == 0, 1.0, t / np.sin(t))
    return 0.5 * ratio ** 2 * h


def water_mu(ct, spec):
    """Effective water attenuation [1/cm] seen by (spectrum, detector): weighted mean over the spectrum."""
    w = effective_weights(ct, spec)
    return float(np.sum(w * xcompy.mixatten(WATER, spec.E)) / np.sum(w))


def default_slices(ct):
    """Slice grid of a cone-beam reconstruction when none is given: one slice per detector row, spaced by the row
    height at the isocentre, centred on z = 0 (the centre of the phantom grid)."""
    return ct.N_rows, -0.5 * (ct.N_rows - 1) * ct.h_iso, ct.h_iso


def _short_scan(ct):
    """Is the rotation (``rotation_angle_total``, input/params.txt:24) a short scan: one for Parker's weights, which make every
    ray count once?  Refuses what the FBP does not reconstruct."""
    if ct.theta_tot > 2 * np.pi + 1e-4:
        raise ValueError(f'rotation_angle_total = {ct.theta_tot:.6g} exceeds 2 pi: more than one rotation is not reconstructed')
    if ct.theta_tot >= 2 * np.pi - 1e-4:
        return False
    need = np.pi + (ct.N_channels - 1) * ct.dgamma
    if ct.theta_tot < need * (1 - 1e-12):
        raise ValueError(f'rotation_angle_total = {ct.theta_tot:.6g} rad is less than a short scan (pi + fan angle = '
                         f'{need:.6g} rad): projections are missing')
    return True


def _check_sino_shape(shape, ct, what='sinogram', tail=0):
    """[N_proj, N_channels] or [N_proj, N_rows, N_channels] of the scanner, and ``tail`` more axes (the planes of a covariance)."""
    shape = tuple(shape)
    if len(shape) - tail not in (2, 3) or shape[0] != ct.N_proj or shape[-1 - tail] != ct.N_channels:
        raise ValueError(f'{what} {shape} does not match the scanner ({ct.N_proj} x {ct.N_channels})')


def _single_process(caller):
    from . import _shard
    if _shard.world()[1] > 1:
        raise NotImplementedError(f'{caller} runs on a single process')


def _stack(t, tail=0):
    """The lift of [views, channels(, T)] to the stack [views, 1, channels(, T)] the kernels take; a stack stays as it is.
    Returns it contiguous, and ``back``: what takes the lift off an image stack again (img -> img[0], or nothing)."""
    if t.dim() - tail == 3:
        return t.contiguous(), lambda img: img
    return t[(slice(None), None) + (slice(None),) * (1 + tail)].contiguous(), lambda img: img[0]          # t[:, None, :(, :)]


def _zero_nonfinite(t, caller, what):
    """The non-finite rule of every reconstruction entry point: count, warn (``caller: n non-finite <what>``), set to 0.
    Returns the cleaned tensor and the mask of the finite values - None where every value is finite."""
    finite = torch.isfinite(t)
    bad = int((~finite).sum().item())
    if not bad:
        return t, None
    # one NaN (a photon-starved ray whose decomposition diverged, ln of a zero count) would spread over its whole
    # detector line in the filter and over the whole image in the back-projection
    import warnings
    warnings.warn(f'{caller}: {bad} non-finite {what}', RuntimeWarning, stacklevel=2)
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0), finite


def _cone(ct, n_rows, what='sinogram'):
    """Does a stack of ``n_rows`` rows go through Feldkamp's algorithm: a cone-beam scanner and more than one row - which
    then must be the scanner's rows."""
    cone = bool(getattr(ct, 'cone', False)) and n_rows > 1
    if cone and n_rows != ct.N_rows:
        raise ValueError(f'{what} has {n_rows} rows, the scanner {ct.N_rows}')
    return cone


def _fbp_inputs(s, ct, what, N_matrix, FOV, ramp, window, slices):
    """What the filter and the back-projection read besides the stack ``s``, on its device: the taps and the channel weight
    SID cos(gamma) in its dtype (float32 for the image, float64 for its covariance), (cos, sin) of the views in float64, the row
    weights of a cone in its dtype (None for a fan: _cone decides, ``what`` names ``s`` if it refuses), the number of images, and
    the scanner geometry: the arguments that follow the counts in the call of the fan or the Feldkamp back-projection."""
    n_rows, dtype, dev = s.shape[1], s.dtype, s.device
    cone = _cone(ct, n_rows, what)
    taps = to_dev(ramp_taps(ct.N_channels, ct.dgamma, ramp, _window(window)), dtype, dev)
    weight = to_dev(ct.SID * np.cos(ct.gammas), dtype, dev)
    view_cs = to_dev(ct.view_cs(), torch.float64, dev)
    dtheta, grid = ct.theta_tot / ct.N_proj, (int(N_matrix), float(FOV))
    if not cone:
        return taps, weight, view_cs, None, n_rows, (ct.SID, ct.dgamma, dtheta) + grid
    n_slices, z0, dz = slices if slices is not None else default_slices(ct)
    row_z = ct.row_z()
    row_w = to_dev(ct.SDD / np.sqrt(ct.SDD ** 2 + (row_z - ct.src_z) ** 2), dtype, dev)
    return taps, weight, view_cs, row_w, int(n_slices), (ct.SID, ct.SDD, ct.dgamma, dtheta, float(row_z[0]), float(ct.h),
                                                         float(ct.src_z)) + grid + (int(n_slices), float(z0), float(dz))


def recon_device(sino_d, ct, N_matrix, FOV, ramp, window=None, slices=None, bhc=None, method='fbp', n_iters=20, n_subsets=1,
                 relax=1.0, init='fbp', nonneg=True, history=None):
    """sino_d: device float32 [N_proj, N_channels] or [N_proj, N_rows, N_channels] -> image tensor
    [N_matrix, N_matrix] or [N_rows, N_matrix, N_matrix] (float32, 1/cm).  A cone-beam scanner (``ct.cone``) is
    reconstructed with Feldkamp's algorithm onto ``slices = (n_slices, z_first [cm], dz [cm])``.  ``bhc``: a
    ``bhc.LinearizationTable`` - the sinogram is linearised first (into a new buffer; sino_d is left as it is), before
    Parker's weights, which a nonlinear map must not follow.  ``method`` and the keywords after it: see get_recon.
    Tensor contract: any view or dtype of ``sino_d`` is made dense float32 first; a host tensor is refused."""
    n_subsets = iterative.check_options(method, ct, n_iters, n_subsets, relax, init)
    # the tensor contract (_device.py): the kernels read dense float32 - a view is made dense, another dtype (the float64
    # stride-2 views get_basismat_sinos hands out) is cast as get_recon casts host arrays, a host tensor is refused
    sino_d = dense_input(sino_d, 'sino_d', gpu_of(sino_d, 'sino_d'), keep=(torch.float32,), cast=torch.float32)
    _check_sino_shape(sino_d.shape, ct)
    if method != 'fbp':
        return _recon_sirt(sino_d, ct, N_matrix, FOV, ramp, window, bhc, n_iters, n_subsets, relax, init, nonneg, history)
    lib = _native.load()
    s, back = _stack(sino_d)
    if bhc is not None:
        from .bhc import linearize_device
        s = linearize_device(s, bhc)
    n_views, n_rows, n_ch = s.shape
    st = stream_ptr()
    if _short_scan(ct):
        sw = torch.empty_like(s)
        _native.check(lib.dexct_fbp_parker(ptr(s), n_views, n_rows, n_ch, float(ct.theta_tot), float(ct.dgamma), 0, n_views,
                                           ptr(sw), st), 'dexct_fbp_parker')
        s = sw
    taps, weight, view_cs, row_w, n_images, geometry = _fbp_inputs(s, ct, 'sinogram', N_matrix, FOV, ramp, window, slices)
    q = torch.empty_like(s)
    _native.check(lib.dexct_fbp_filter(ptr(s), ptr(taps), ptr(weight), n_views * n_rows, n_ch, ct.dgamma, ptr(q), st),
                  'dexct_fbp_filter')
    img = torch.empty((n_images, N_matrix, N_matrix), dtype=torch.float32, device=s.device)
    if row_w is not None:
        _native.check(lib.dexct_fdk_backproject(ptr(q), ptr(view_cs), ptr(row_w), n_views, n_ch, n_rows, *geometry, ptr(img), st),
                      'dexct_fdk_backproject')
        return img
    _native.check(lib.dexct_fbp_backproject(ptr(q), ptr(view_cs), n_views, n_ch, n_rows, *geometry, ptr(img), st),
                  'dexct_fbp_backproject')
    return back(img)


def _recon_sirt(sino_d, ct, N_matrix, FOV, ramp, window, bhc, n_iters, n_subsets, relax, init, nonneg, history):
    """SIRT / OS-SART of a fan or stacked-fan sinogram (iterative.sirt), from the FBP image or from zero; the options have
    passed iterative.check_options.  ``bhc`` as for recon_device: a table, applied into a new buffer."""
    s, back = _stack(sino_d)
    n_views, n_rows, n_ch = s.shape
    _check_sino_shape(sino_d.shape, ct)
    proj = iterative.ImageProjector(ct, N_matrix, FOV, n_slices=n_rows)
    if bhc is not None:
        from .bhc import linearize_device
        s = linearize_device(s, bhc)
    x0 = recon_device(s, ct, N_matrix, FOV, ramp, window) if init == 'fbp' else None
    return back(iterative.sirt(s, proj, n_iters, n_subsets, relax, x0=x0, nonneg=nonneg, history=history))


def get_recon(sino, ct, spec, N_matrix, FOV, ramp, window=None, slices=None, bhc=None, method='fbp', n_iters=20, n_subsets=1,
              relax=1.0, init='fbp', nonneg=True, history=None, weights=None, beta=0.0, delta=1e-3):
    """Drop-in for ``recon_raw, recon_HU = get_recon(sino, ct, spec, N_matrix, FOV, ramp)`` (main.py:134).
    ``window``: apodisation of the ramp (WINDOWS; default ``DEXCT_FBP_WINDOW`` or the plain band-limited ramp).
    Cone-beam sinograms ([N_proj, N_rows, N_channels] of a ``cone=True`` scanner) are reconstructed with Feldkamp's
    algorithm into ``slices = (n_slices, z_first, dz)`` (default: default_slices).
    ``bhc``: beam-hardening correction of the log sinogram before the reconstruction (bhc.py) - a material ('water',
    'bone', a Material or (formula, density)) linearised for ``spec`` and the scanner's detector, or a prebuilt
    ``bhc.LinearizationTable``.  recon_HU stays 1000 (raw - water_mu) / water_mu: water reads 0 HU after water BHC.
    ``method``: 'fbp' (the default: everything above), 'sirt' or 'os-sart' - ``n_iters`` iterations of iterative.sirt on the
    matched projector pair of the same grid, over ``n_subsets`` ordered subsets of the views (1: SIRT; more: OS-SART;
    'os-sart' with the default of 1 means 10), relaxation ``relax`` in (0, 2), started from the FBP image (``init='fbp'``) or
    from zero (``'zero'``), clamped at 0 after every update if ``nonneg``; ``history``: a list that receives the weighted
    residual norm before each iteration.  Fan and stacked fan only.  The warning about non-finite values, ``bhc`` and the HU
    formula are those of the FBP path.  A short scan needs no Parker weights here: the iteration solves A x = b for the views
    there are, and a ray measured twice simply enters twice (the weights only serve init='fbp').
    ``method='pwls'``: penalised weighted least squares, the single-channel case of get_basismat_recon - ``weights`` (needed) is
    the inverse variance of every sinogram value, of the sinogram's shape and >= 0 (0: the ray is ignored), ``beta`` and
    ``delta`` the strength and the threshold of the Huber penalty; ``n_iters``, ``n_subsets``, ``init``, ``nonneg`` and
    ``history`` (here: the objective before each iteration) as above, ``relax`` is not used.  Non-finite sinogram values get
    the weight 0.  Like ``sino``, ``weights`` is a host array (device tensors: iterative.pwls); ``slices`` belongs to the cone
    branch and is refused here; single process, as get_basismat_recon."""
    # host checks: nothing here touches the device
    if method == 'pwls':
        n_subsets, beta, delta = iterative.check_pwls_options(ct, 1, n_iters, n_subsets, beta, delta, init, FOV)
        if weights is None:
            raise ValueError("method='pwls' needs weights: the inverse variance of every sinogram value")
        if slices is not None:
            raise ValueError("slices belong to the cone-beam FBP: method='pwls' reconstructs the rows of the sinogram")
        if getattr(weights, 'is_cuda', False) or getattr(sino, 'is_cuda', False):
            raise ValueError('get_recon takes host arrays: device tensors go to get_basismat_recon or iterative.pwls')
        if tuple(np.shape(weights)) != tuple(np.shape(sino)):
            raise ValueError(f'weights {tuple(np.shape(weights))} do not have the shape of the sinogram {tuple(np.shape(sino))}')
        _check_sino_shape(np.shape(sino), ct)
        _single_process("get_recon(method='pwls')")
    elif weights is not None:
        raise ValueError(f"weights belong to method='pwls', not to {method!r}")
    else:
        n_subsets = iterative.check_options(method, ct, n_iters, n_subsets, relax, init, FOV)
    sino_d = to_dev(np.asarray(sino, dtype=np.float32), torch.float32, device())
    sino_d, finite = _zero_nonfinite(sino_d, 'get_recon', 'sinogram value(s) set to 0 before filtering')
    if bhc is not None:
        from . import bhc as bhc_mod
        table = bhc if isinstance(bhc, bhc_mod.LinearizationTable) else bhc_mod.linearization_table(ct, spec, bhc)
        bhc_mod.linearize_device(sino_d, table, out=sino_d)         # sino_d is this call's own copy
    if method == 'pwls':
        weights_d = to_dev(np.asarray(weights, dtype=np.float32), torch.float32, sino_d.device)
        if not bool((torch.isfinite(weights_d) & (weights_d >= 0)).all().item()):
            raise ValueError('weights must be finite and >= 0')
        if finite is not None:
            weights_d[~finite] = 0.0
        s, back = _stack(sino_d)
        img = back(_recon_pwls(s[None], weights_d.reshape((1,) + s.shape), ct, N_matrix, FOV, ramp, window, beta, delta, n_iters,
                               n_subsets, init, nonneg, history)[0])
    elif method == 'fbp':
        img = recon_device(sino_d, ct, N_matrix, FOV, ramp, window=window, slices=slices)
    else:
        img = _recon_sirt(sino_d, ct, N_matrix, FOV, ramp, window, bhc=None, n_iters=n_iters, n_subsets=n_subsets, relax=relax,
                          init=init, nonneg=nonneg, history=history)
    raw = img.cpu().numpy()
    mu_w = water_mu(ct, spec)
    return raw, (1000.0 * (raw - mu_w) / mu_w).astype(np.float32)


def _recon_pwls(sinos_d, weights_d, ct, N_matrix, FOV, ramp, window, beta, delta, n_iters, n_subsets, init, nonneg, history):
    """iterative.pwls of sinograms [K, N_proj, n_rows, N_channels] with the packed weights [T, N_proj, n_rows, N_channels]
    (device float32), every channel started from its FBP image (``init='fbp'``) or from zero -> images [K, n_rows, N, N]."""
    K, _, n_rows, _ = sinos_d.shape
    proj = iterative.ImageProjector(ct, N_matrix, FOV, n_slices=n_rows)
    x0 = torch.stack([recon_device(sinos_d[k], ct, N_matrix, FOV, ramp, window) for k in range(K)]) if init == 'fbp' else None
    return iterative.pwls(sinos_d, weights_d, proj, n_iters, n_subsets, beta, delta, x0=x0, nonneg=nonneg, history=history)


def get_basismat_recon(basis_sinos, cov_sino, ct, N_matrix, FOV, ramp, beta, delta, n_iters=20, n_subsets=1, init='fbp',
                       nonneg=False, w_fill=0.0, history=None, window=None):
    """Joint statistical reconstruction of the K = 1 .. 3 basis-material images from the basis sinograms and their per-ray noise
    covariance: penalised weighted least squares with the inverse covariance as the weight and a Huber penalty (iterative.pwls,
    which states the objective and the iteration).

    basis_sinos: K sinograms, each [N_proj, N_channels] or [N_proj, N_rows, N_channels] - what get_basismat_sinos returns;
    cov_sino: exactly what matdecomp.get_basismat_covariance returns for them, [N_proj, (N_rows,) N_channels, T] with T =
    K (K + 1) / 2 (var(m1), cov(m1, m2), var(m2) for two).  ``beta``, ``delta``: strength and threshold [the images' unit] of the
    Huber penalty, a scalar or one value per channel; ``n_iters`` iterations over ``n_subsets`` ordered subsets of the views,
    started from the FBP image of every channel (``init='fbp'``, with ``ramp`` and ``window``) or from zero; ``nonneg`` clamps at 0
    (off: basis images may be negative).  A ray whose covariance is not finite and positive definite - the exact zeros of an
    air-masked pixel, a diverged decomposition - weighs ``w_fill`` on the diagonal and 0 off it (0: the ray is ignored).
    Non-finite sinogram values are set to 0 with a RuntimeWarning, as in get_recon, and their rays get ``w_fill`` too.
    ``history``: a list that receives the objective before each iteration.  Returns a tuple of K images [N_matrix, N_matrix]
    or [N_rows, N_matrix, N_matrix], float32: NumPy arrays, or device tensors if the sinograms were device tensors.  Fan and
    stacked fan only; single process."""
    sinos = list(basis_sinos)
    K = len(sinos)
    n_subsets, beta, delta = iterative.check_pwls_options(ct, K, n_iters, n_subsets, beta, delta, init, FOV)
    shapes = [tuple(t.shape) if isinstance(t, torch.Tensor) else np.shape(t) for t in sinos]
    shape = shapes[0]
    if any(sh != shape for sh in shapes):
        raise ValueError(f'the basis sinograms differ in shape: {shapes}')
    _check_sino_shape(shape, ct)
    T = K * (K + 1) // 2
    cov_shape = tuple(cov_sino.shape) if isinstance(cov_sino, torch.Tensor) else np.shape(cov_sino)
    if cov_shape != shape + (T,):
        raise ValueError(f'covariance sinogram {cov_shape}: {shape + (T,)} wanted for {K} sinogram(s) of shape {shape}')
    iterative.check_w_fill(w_fill)
    window = _window(window)
    _short_scan(ct)
    _single_process('get_basismat_recon')
    tensors_in = all(isinstance(t, torch.Tensor) for t in sinos)
    dev = device()
    stacks = [_stack(to_dev(t if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32), torch.float32, dev)) for t in sinos]
    s, back = torch.stack([st for st, _ in stacks]), stacks[0][1]
    cov_d = to_dev(cov_sino if isinstance(cov_sino, torch.Tensor) else np.asarray(cov_sino, dtype=np.float64), torch.float64, dev)
    cov_d = _stack(cov_d, tail=1)[0]
    s, finite = _zero_nonfinite(s, 'get_basismat_recon', 'sinogram value(s) set to 0 before the reconstruction')
    if finite is not None:
        # their rays are unusable: a NaN covariance makes dexct_cov_precision write w_fill (into a copy: cov_sino is the caller's)
        cov_d = torch.where(finite.all(0)[..., None], cov_d, torch.full_like(cov_d, float('nan')))
    w = iterative.precision_weights(cov_d, w_fill)
    imgs = _recon_pwls(s, w, ct, N_matrix, FOV, ramp, window, beta, delta, n_iters, n_subsets, init, nonneg, history)
    out = tuple(back(imgs[k]) for k in range(K))
    return out if tensors_in else tuple(t.cpu().numpy() for t in out)


def _check_cov_sino(shape, ct, window):
    """The host checks of a covariance sinogram [N_proj, (N_rows,) N_channels, T] against ``ct``: everything that can be
    refused before the device is touched.  Returns the window's name."""
    shape = tuple(shape)
    if len(shape) == 2:
        raise ValueError(f'covariance sinogram {shape} has no plane axis: pass a single variance sinogram as var[..., None]')
    if len(shape) not in (3, 4):
        raise ValueError(f'covariance sinogram must be [N_proj, N_channels, T] or [N_proj, N_rows, N_channels, T], got {shape}')
    _check_sino_shape(shape, ct, 'covariance sinogram', tail=1)
    if shape[-1] < 1:
        raise ValueError('covariance sinogram has no planes')
    window = _window(window)
    _short_scan(ct)
    _cone(ct, shape[1] if len(shape) == 4 else 1, 'covariance sinogram')
    if ct.N_channels > _native.FBP_VAR_MAX_CHANNELS:
        raise ValueError(f'{ct.N_channels} channels: the variance filter takes at most {_native.FBP_VAR_MAX_CHANNELS}')
    return window


def recon_covariance_device(cov_d, ct, N_matrix, FOV, ramp, window=None, slices=None):
    """Noise propagation through the FBP of recon_device: cov_d, device float64 [N_proj, N_channels, T] or [N_proj, N_rows,
    N_channels, T] - T planes of per-pixel (co)variance of independent sinogram pixels, e.g. the packed triangle of
    matdecomp.gn_covariance_device - -> the (co)variance of every image pixel, [N_matrix, N_matrix, T] or [rows or slices,
    N_matrix, N_matrix, T] (float64).  Exact for the discrete operator recon_device applies with the same ``ct``, ``ramp``,
    ``window`` and ``slices`` (Parker weights of a short scan and Feldkamp's cone branch included): the element-wise square of
    the FBP matrix applied to every plane (dexct_fbp_var_filter, dexct_fbp_var_backproject, dexct_fdk_var_backproject).  The
    result is pixel-wise: neighbouring image pixels are correlated, the variance of an ROI mean is not its average."""
    if not _device.on_gpu(cov_d) or cov_d.dtype != torch.float64:
        raise ValueError('cov_d must be a float64 device tensor')
    window = _check_cov_sino(cov_d.shape, ct, window)
    cov_d = dense_input(cov_d, 'cov_d', cov_d.device, keep=(torch.float64,))
    lib = _native.load()
    s, back = _stack(cov_d, tail=1)
    n_views, n_rows, n_ch, n_planes = s.shape
    st = stream_ptr()
    taps, weight, view_cs, row_w, n_images, geometry = _fbp_inputs(s, ct, 'covariance sinogram', N_matrix, FOV, ramp, window, slices)
    qa, qb = torch.empty_like(s), torch.empty_like(s)
    _native.check(lib.dexct_fbp_var_filter(ptr(s), n_views, n_rows, n_ch, n_planes, ptr(taps), ptr(weight), float(ct.dgamma),
                                           float(ct.theta_tot) if _short_scan(ct) else 2 * np.pi, 0, n_views, ptr(qa), ptr(qb), st),
                  'dexct_fbp_var_filter')
    img = torch.empty((n_images, N_matrix, N_matrix, n_planes), dtype=torch.float64, device=s.device)
    if row_w is not None:
        _native.check(lib.dexct_fdk_var_backproject(ptr(qa), ptr(qb), ptr(view_cs), ptr(row_w), n_views, n_ch, n_rows, n_planes,
                                                    *geometry, ptr(img), st), 'dexct_fdk_var_backproject')
        return img
    _native.check(lib.dexct_fbp_var_backproject(ptr(qa), ptr(qb), ptr(view_cs), n_views, n_ch, n_rows, n_planes, *geometry, ptr(img),
                                                st), 'dexct_fbp_var_backproject')
    return back(img)


def get_recon_covariance(cov_sino, ct, N_matrix, FOV, ramp, window=None, slices=None):
    """The predicted noise (co)variance of the images get_recon makes from sinograms whose per-pixel (co)variance is
    ``cov_sino``: [N_proj, N_channels, T] or [N_proj, N_rows, N_channels, T], e.g. what matdecomp.get_basismat_covariance
    returns (T = 3: var(m1), cov(m1, m2), var(m2)); a single variance sinogram is passed as ``var[..., None]``.  Returns
    [N_matrix, N_matrix, T] or [rows or slices, N_matrix, N_matrix, T], float64, the layout plots.vmi_noise_map and
    plots.vmi_variance read.  ``window`` and ``slices`` as for get_recon.  Non-finite entries (a diverged pixel of the
    decomposition) are set to 0 with a RuntimeWarning - get_recon's rule: they must not smear over the image.  Sinogram
    pixels are taken as independent; the result is the pixel-wise (co)variance of the FBP image (recon_covariance_device).
    NumPy in -> NumPy out; a device tensor in -> a device tensor out.  Single process only."""
    tensor_in = isinstance(cov_sino, torch.Tensor)
    window = _check_cov_sino(cov_sino.shape if tensor_in else np.shape(cov_sino), ct, window)
    _single_process('get_recon_covariance')
    cov_d = to_dev(cov_sino if tensor_in else np.asarray(cov_sino, dtype=np.float64), torch.float64, device())
    cov_d, _ = _zero_nonfinite(cov_d, 'get_recon_covariance', 'covariance value(s) set to 0 before filtering')
    out = recon_covariance_device(cov_d, ct, N_matrix, FOV, ramp, window, slices)
    return out if tensor_in else to_host(out)


def make_vmi(E0, M1, M2, HU=True, matcomp1=None, matcomp2=None):
    """Virtual monoenergetic image at E0 [keV] from the two basis-material images - the reference's
    ``make_vmi`` (plots.py:136-144): ``u_p_1 * M1 + u_p_2 * M2`` with the basis mass attenuations at E0, in HU
    against water ('H(11.2)O(88.8)', plots.py:140) unless ``HU=False``.  float32 out, like the reference."""
    from . import matdecomp as md
    lib = _native.load()
    dev = device()
    E = np.array([float(E0)])
    u1 = float(xcompy.mixatten(matcomp1 or md.matcomp1, E)[0])
    u2 = float(xcompy.mixatten(matcomp2 or md.matcomp2, E)[0])
    uw = float(xcompy.mixatten(WATER, E)[0])
    m1 = to_dev(np.asarray(M1, dtype=np.float32), torch.float32, dev)
    m2 = to_dev(np.asarray(M2, dtype=np.float32), torch.float32, dev)
    if m1.shape != m2.shape:
        raise ValueError('basis images differ in shape')
    out = torch.empty_like(m1)
    _native.check(lib.dexct_vmi(ptr(m1), ptr(m2), m1.numel(), u1, u2, uw, int(bool(HU)), ptr(out), stream_ptr()),
                  'dexct_vmi')
    return out.cpu().numpy()
