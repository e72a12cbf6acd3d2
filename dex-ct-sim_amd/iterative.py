"""Iterative reconstruction (SIRT / OS-SART) on a matched projector pair (csrc/iterative.hip; an extension: the reference
reconstructs with filtered back-projection only).

``ImageProjector`` applies the system matrix A of the label projector to a float32 image (``forward``) and its transpose to a
sinogram (``adjoint``): dexct_image_project and dexct_image_backproject on the fixed-point plan of dexct_fan_plan, with the
image grid of ``get_recon`` (``N_matrix`` pixels over ``FOV`` cm, centred on the isocentre) in the place of the phantom grid.
Row i of A holds the intersection lengths [cm] of ray i with the pixels (include/dexct.h states the coefficients); both
kernels form them with one device function, so <A x, y> = <x, A^T y> up to float32 rounding.

``sirt`` iterates, for the ordered subsets s = 0 .. S - 1 of the views (subset s = the views congruent to s modulo S):

    r_i = (b_i - (A x)_i) / R_i          R_i = sum_j a_ij      (0 for a ray that misses the grid)
    x_j <- x_j + relax * (sum_{i in s} a_ij r_i) / C^s_j       C^s_j = sum_{i in s} a_ij   (pixels with C = 0 stay)
    x_j <- max(x_j, 0)                                         if nonneg

S = 1 is SIRT (Gilbert 1972; for relax in (0, 2) the R-weighted residual norm never increases), S > 1 is OS-SART (Andersen &
Kak 1984 with ordered subsets).  Every step is a HIP kernel (dexct_sirt_residual, dexct_sirt_update); torch tensors are the
device containers.

``pwls`` is the statistical iteration on the same pair: K = 1 .. 3 channels (sinograms b_k, images x_k) coupled by a symmetric
K x K weight matrix W_i per ray - the inverse of the covariance of the basis line integrals (``precision_weights``) - and an
edge-preserving Huber penalty on the in-plane 4-neighbourhood of every image:

    Phi(x) = 1/2 sum_i r_i^T W_i r_i + sum_k beta_k sum_pairs psi_(delta_k)(x_kj - x_kn)       r_i = ((A x_k)_i - b_ki)_k

minimised with ordered-subsets separable quadratic surrogates (Erdogan & Fessler 1999); the steps are stated at ``pwls`` and
are the kernels of csrc/pwls.hip (dexct_pwls_majorizer, dexct_pwls_residual, dexct_pwls_update).
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _device, _native
from ._device import dense_input, device, ptr, stream_ptr, to_dev

METHODS = ('fbp', 'sirt', 'os-sart')
OS_SART_SUBSETS = 10


def _check_iteration(ct, FOV, init, n_iters):
    """What check_options and check_pwls_options ask alike, up to the iteration count; _check_subsets closes both."""
    if bool(getattr(ct, 'cone', False)):
        raise ValueError('iterative reconstruction is fan and stacked-fan only: a cone-beam scanner has no matched pair here')
    if FOV is not None and 0.5 * np.sqrt(2.0) * float(FOV) >= ct.SID:
        raise ValueError(f'FOV = {FOV} cm: the image grid does not lie strictly inside the source circle (SID = {ct.SID} cm)')
    if init not in ('fbp', 'zero'):
        raise ValueError(f"init must be 'fbp' or 'zero', not {init!r}")
    if int(n_iters) < 1:
        raise ValueError(f'n_iters = {n_iters}: at least one iteration')


def _check_subsets(n_subsets, ct):
    """``n_subsets`` is named in the message as the caller passes it here.  Returns the count."""
    if not 1 <= int(n_subsets) <= ct.N_proj:
        raise ValueError(f'n_subsets = {n_subsets} lies outside 1 .. N_proj = {ct.N_proj}')
    return int(n_subsets)


def check_options(method, ct, n_iters, n_subsets, relax, init='fbp', FOV=None):
    """The argument checks of ``get_recon(..., method=)``, before any device access.  Returns the subset count."""
    if method not in METHODS:
        raise ValueError(f'unknown reconstruction method {method!r}; choose from {METHODS}')
    if method == 'fbp':
        return 1
    _check_iteration(ct, FOV, init, n_iters)
    if not 0.0 < float(relax) < 2.0:
        raise ValueError(f'relax = {relax} lies outside (0, 2)')
    n_subsets = int(n_subsets)
    if method == 'os-sart' and n_subsets == 1:
        n_subsets = min(OS_SART_SUBSETS, ct.N_proj)
    return _check_subsets(n_subsets, ct)


class ImageProjector:
    """The pair (A, A^T) of one scanner and one image grid; the plan of all views is built once, on first use.

    ``ImageProjector(ct, N_matrix, FOV, n_slices=1)``: the grid of ``get_recon``; ``n_slices`` stacked slices share the plan
    (row r of the sinogram images slice r).  ``transposed=False`` makes both kernels work on the image alone, without the
    in-plane transposed copy that the x-dominant rays otherwise use (tools/probes/iter_recon.py measures the two)."""

    def __init__(self, ct, N_matrix, FOV, n_slices=1, transposed=True):
        if bool(getattr(ct, 'cone', False)):
            raise ValueError('ImageProjector is fan and stacked-fan only: a cone-beam scanner has no matched pair here')
        n, fov = int(N_matrix), float(FOV)
        if n < 1 or not fov > 0 or int(n_slices) < 1:
            raise ValueError(f'N_matrix = {N_matrix}, FOV = {FOV}, n_slices = {n_slices}: positive values wanted')
        self._setup(nx=n, ny=n, nz=int(n_slices), dx=fov / n, dy=fov / n, n_views=ct.N_proj, n_channels=ct.N_channels,
                    n_rows=int(n_slices), z_first=0, sid=ct.SID, sdd=ct.SDD, view_cs=ct.view_cs(), chan_cs=ct.chan_cs(),
                    transposed=transposed)

    @classmethod
    def from_grid(cls, nx, ny, nz, dx, dy, n_views, n_channels, n_rows, z_first, sid, sdd, view_cs, chan_cs, transposed=True):
        """Any grid (nx != ny, dx != dy) and any window of slices: row r images slice ``z_first + r`` of ``nz``."""
        self = cls.__new__(cls)
        self._setup(nx=int(nx), ny=int(ny), nz=int(nz), dx=float(dx), dy=float(dy), n_views=int(n_views),
                    n_channels=int(n_channels), n_rows=int(n_rows), z_first=int(z_first), sid=float(sid), sdd=float(sdd),
                    view_cs=view_cs, chan_cs=chan_cs, transposed=transposed)
        return self

    def _setup(self, nx, ny, nz, dx, dy, n_views, n_channels, n_rows, z_first, sid, sdd, view_cs, chan_cs, transposed):
        # the plan clips every ray against the grid from a source OUTSIDE it
        if 0.5 * np.hypot(nx * dx, ny * dy) >= sid:
            raise ValueError(f'the image grid ({nx * dx:.6g} x {ny * dy:.6g} cm, half diagonal {0.5 * np.hypot(nx * dx, ny * dy):.6g} '
                             f'cm) does not lie strictly inside the source circle (SID = {sid:.6g} cm)')
        if z_first < 0 or n_rows < 1 or z_first + n_rows > nz:
            raise ValueError(f'rows {z_first} .. {z_first + n_rows - 1} lie outside the {nz} slices')
        self.nx, self.ny, self.nz, self.n_views, self.n_channels, self.n_rows, self.z_first = nx, ny, nz, n_views, n_channels, n_rows, z_first
        self.geom = _native.FanGeom(n_views, n_channels, n_rows, z_first, nx, ny, nz, 0, dx, dy, 1.0, sid, sdd)
        self._view_cs, self._chan_cs = np.ascontiguousarray(view_cs, np.float64), np.ascontiguousarray(chan_cs, np.float64)
        self.transposed = bool(transposed)
        self.plan = None
        self._row_sums, self._col_sums = None, {}
        self._pwls_d = None

    # ---- device state ---------------------------------------------------------------------------------------------------------
    def _ready(self):
        if self.plan is not None:
            return
        self.lib = _native.load()
        self.dev = device()
        vcs, ccs = to_dev(self._view_cs, torch.float64, self.dev), to_dev(self._chan_cs, torch.float64, self.dev)
        plan = torch.empty(self.n_views * self.n_channels * _native.PLAN_BYTES, dtype=torch.uint8, device=self.dev)
        _native.check(self.lib.dexct_fan_plan(C.byref(self.geom), ptr(vcs), ptr(ccs), 0, self.n_views, ptr(plan), stream_ptr()),
                      'dexct_fan_plan')
        torch.cuda.current_stream().synchronize()          # vcs and ccs may go once the plan is written
        self.scratch = torch.empty(self.image_shape, dtype=torch.float32, device=self.dev) if self.transposed else None
        self.plan = plan

    @property
    def image_shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def sino_shape(self):
        return (self.n_views, self.n_rows, self.n_channels)

    def _views(self, views):
        begin, end, step = (0, self.n_views, 1) if views is None else (int(v) for v in views)
        if not (0 <= begin < end <= self.n_views and step >= 1):
            raise ValueError(f'views = {views}: (begin, end, step) with 0 <= begin < end <= {self.n_views} and step >= 1 wanted')
        return begin, end, step

    def _tensor(self, t, shape, what):
        """The tensor contract of this module (_device.py): strict - nothing is normalised; every argument is checked on the
        host before the projector's device state is built."""
        if not (_device.on_gpu(t) and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f'{what}: a contiguous float32 device tensor wanted')
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f'{what}: shape {tuple(t.shape)} does not match {shape}')
        return t

    def forward(self, img_d, views=None, out=None):
        """A x: image [nz, ny, nx] ([ny, nx] for one slice) -> sinogram [n_views, n_rows, n_channels].  ``views = (begin, end,
        step)``: only those views are computed; the other lines of ``out`` stay (zeros in a new tensor)."""
        begin, end, step = self._views(views)
        img = self._tensor(img_d, self.image_shape, 'image')
        if out is not None:
            self._tensor(out, self.sino_shape, 'out')
        self._ready()
        if out is None:
            out = torch.zeros(self.sino_shape, dtype=torch.float32, device=self.dev)
        sino = out
        st = stream_ptr()
        if self.transposed:
            _native.check(self.lib.dexct_transpose_batched(ptr(img), ptr(self.scratch), self.nz, self.ny, self.nx, 4, st),
                          'dexct_transpose_batched')
        line = self.n_rows * self.n_channels
        _native.check(self.lib.dexct_image_project(
            C.byref(self.geom), self.plan.data_ptr() + begin * self.n_channels * _native.PLAN_BYTES, begin, end, step, ptr(img),
            ptr(self.scratch), sino.data_ptr() + 4 * begin * line, st), 'dexct_image_project')
        return out

    def adjoint(self, sino_d, views=None, out=None, accumulate=False):
        """A^T y over the views -> image [nz, ny, nx]; ``out`` is overwritten unless ``accumulate``."""
        begin, end, step = self._views(views)
        sino = self._tensor(sino_d, self.sino_shape, 'sinogram')
        if out is not None:
            self._tensor(out, self.image_shape, 'out')
        self._ready()
        if out is None:
            out = torch.empty(self.image_shape, dtype=torch.float32, device=self.dev)
            accumulate = False
        img = out
        line = self.n_rows * self.n_channels
        _native.check(self.lib.dexct_image_backproject(
            C.byref(self.geom), self.plan.data_ptr() + begin * self.n_channels * _native.PLAN_BYTES, begin, end, step,
            sino.data_ptr() + 4 * begin * line, ptr(img), ptr(self.scratch), int(bool(accumulate)), stream_ptr()),
            'dexct_image_backproject')
        return out

    def forget_weights(self):
        """Drop the majoriser ``pwls`` keeps for its last weight tensor (it is made again on the next call): needed only after
        that tensor was overwritten through its raw pointer, which torch does not see."""
        self._pwls_d = None

    def row_sums(self):
        """R = A 1 (the forward kernel applied to an image of ones), cached."""
        if self._row_sums is None:
            self._ready()
            self._row_sums = self.forward(torch.ones(self.image_shape, dtype=torch.float32, device=self.dev))
        return self._row_sums

    def col_sums(self, subset=0, n_subsets=1):
        """C^s = A_s^T 1 over the views congruent to ``subset`` modulo ``n_subsets`` (the adjoint kernel applied to a sinogram
        of ones), cached."""
        key = (int(subset), int(n_subsets))
        if key not in self._col_sums:
            self._ready()
            ones = torch.ones(self.sino_shape, dtype=torch.float32, device=self.dev)
            self._col_sums[key] = self.adjoint(ones, views=(key[0], self.n_views, key[1]))
        return self._col_sums[key]


def sirt(sino_d, proj, n_iters, n_subsets=1, relax=1.0, x0=None, nonneg=True, history=None):
    """``n_iters`` passes over the ``n_subsets`` ordered subsets (module docstring); sino_d: device float32 [n_views, n_rows,
    n_channels]; x0: start image (default zeros; not modified).  ``history``: a list that receives the R-weighted residual
    norm sqrt(sum (b - A x)_i^2 / R_i) of the image BEFORE each iteration (computed on the device; one host
    synchronisation per iteration).  Returns the image [nz, ny, nx]."""
    n_iters, S, relax = int(n_iters), int(n_subsets), float(relax)
    if n_iters < 1 or not 1 <= S <= proj.n_views or not 0.0 < relax < 2.0:
        raise ValueError(f'n_iters = {n_iters}, n_subsets = {S}, relax = {relax}: n_iters >= 1, 1 <= n_subsets <= '
                         f'{proj.n_views} and 0 < relax < 2 wanted')
    b = proj._tensor(sino_d, proj.sino_shape, 'sinogram')
    if x0 is not None:
        proj._tensor(x0, proj.image_shape, 'x0')
    proj._ready()
    lib, dev = proj.lib, proj.dev
    x = torch.zeros(proj.image_shape, dtype=torch.float32, device=dev) if x0 is None else x0.clone()
    R = proj.row_sums()
    ax = torch.zeros(proj.sino_shape, dtype=torch.float32, device=dev)
    g = torch.empty(proj.image_shape, dtype=torch.float32, device=dev)
    norm2 = torch.zeros(1, dtype=torch.float64, device=dev) if history is not None else None
    line = proj.n_rows * proj.n_channels
    n_views = proj.n_views

    def residual(s, step, r, n2):
        off = 4 * s * line
        _native.check(lib.dexct_sirt_residual(b.data_ptr() + off, ax.data_ptr() + off, R.data_ptr() + off, n_views - s, step,
                                              line, None if r is None else r.data_ptr() + off, ptr(n2), stream_ptr()),
                      'dexct_sirt_residual')

    for _ in range(n_iters):
        if history is not None and S > 1:                  # (with one subset the iteration's own residual is the one wanted)
            proj.forward(x, out=ax)
            residual(0, 1, None, norm2)
            history.append(float(np.sqrt(norm2.item())))
        for s in range(S):
            views = (s, n_views, S)
            proj.forward(x, views=views, out=ax)
            residual(s, S, ax, norm2 if S == 1 else None)
            proj.adjoint(ax, views=views, out=g)
            _native.check(lib.dexct_sirt_update(ptr(x), ptr(g), ptr(proj.col_sums(s, S)), x.numel(), relax, int(bool(nonneg)),
                                                stream_ptr()), 'dexct_sirt_update')
        if history is not None and S == 1:
            history.append(float(np.sqrt(norm2.item())))
    return x


# ---- joint penalised weighted least squares (OS-SQS, Huber) -----------------------------------------------------------------------

PWLS_MAX_CHANNELS = 3


def per_channel(value, K, what, positive=False):
    """A scalar or one value per channel -> K floats; beta >= 0, delta > 0 (``positive``), finite."""
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    if v.size == 1:
        v = np.repeat(v, K)
    if v.size != K:
        raise ValueError(f'{what} = {value!r}: a scalar or one value per channel ({K}) wanted')
    if not np.all(np.isfinite(v)) or (positive and not np.all(v > 0)) or not np.all(v >= 0):
        raise ValueError(f'{what} = {value!r}: {"positive" if positive else "non-negative"} finite values wanted')
    return [float(t) for t in v]


def check_pwls_options(ct, K, n_iters, n_subsets, beta, delta, init='fbp', FOV=None):
    """The argument checks of ``get_basismat_recon`` and ``get_recon(..., method='pwls')`` that need no device.  Returns
    (n_subsets, beta per channel, delta per channel)."""
    if not 1 <= int(K) <= PWLS_MAX_CHANNELS:
        raise ValueError(f'{K} channels: the joint reconstruction takes 1 .. {PWLS_MAX_CHANNELS}')
    _check_iteration(ct, FOV, init, n_iters)
    return _check_subsets(n_subsets, ct), per_channel(beta, K, 'beta'), per_channel(delta, K, 'delta', positive=True)


def channels_of(n_planes):
    """K of a packed triangle of T = K (K + 1) / 2 planes (ValueError for any other T)."""
    for K in range(1, PWLS_MAX_CHANNELS + 1):
        if K * (K + 1) // 2 == int(n_planes):
            return K
    raise ValueError(f'{n_planes} planes are no packed triangle of 1 .. {PWLS_MAX_CHANNELS} channels (1, 3 or 6 wanted)')


def check_w_fill(w_fill):
    if not (float(w_fill) >= 0.0 and np.isfinite(float(w_fill))):
        raise ValueError(f'w_fill = {w_fill}: a finite value >= 0 wanted')


def precision_weights(cov_d, w_fill=0.0):
    """The per-ray precision matrices of a packed covariance: cov_d, device float64 [..., T] (the layout of
    matdecomp.gn_covariance_device) -> float32 [T, ...], plane-major, each plane a sinogram (dexct_cov_precision: the float64
    closed-form inverse rounded once; a ray whose matrix is not finite and positive definite gets ``w_fill`` on the diagonal
    planes and 0 elsewhere)."""
    if not (_device.on_gpu(cov_d) and cov_d.dtype == torch.float64):
        raise ValueError('cov_d must be a float64 device tensor')
    T = cov_d.shape[-1]
    K = channels_of(T)
    check_w_fill(w_fill)
    c = dense_input(cov_d, 'cov_d', cov_d.device, keep=(torch.float64,))
    w = torch.empty((T,) + tuple(c.shape[:-1]), dtype=torch.float32, device=c.device)
    _native.check(_native.load().dexct_cov_precision(ptr(c), c.numel() // T, K, float(w_fill), ptr(w), stream_ptr()),
                  'dexct_cov_precision')
    return w


def _pwls_majoriser(proj, w, K):
    """d_k = A^T((sum_l |W_kl|) R) over ALL views, [K, nz, ny, nx]; kept on the projector for the weight tensor it was made
    from: the same object, unchanged since by torch's count of in-place operations.  A write through the raw pointer (a
    library call given ``w.data_ptr()``) is invisible to that count: after one, call ``proj.forget_weights()``."""
    hit = proj._pwls_d
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    m = torch.empty((K,) + proj.sino_shape, dtype=torch.float32, device=proj.dev)
    _native.check(proj.lib.dexct_pwls_majorizer(ptr(w), ptr(proj.row_sums()), m[0].numel(), K, ptr(m), stream_ptr()),
                  'dexct_pwls_majorizer')
    d = torch.empty((K,) + proj.image_shape, dtype=torch.float32, device=proj.dev)
    for k in range(K):
        proj.adjoint(m[k], out=d[k])
    proj._pwls_d = (weakref.ref(w), w._version, d)
    return d


def pwls(sinos_d, weights_d, proj, n_iters, n_subsets=1, beta=0.0, delta=1e-3, x0=None, nonneg=False, history=None):
    """Joint penalised weighted least squares of K = 1 .. 3 channels, ``n_iters`` passes over the ``n_subsets`` ordered
    subsets (subset s = the views congruent to s modulo S, as in ``sirt``).

    sinos_d: device float32 [K, n_views, n_rows, n_channels] (or a sequence of K sinograms); weights_d: device float32
    [T, n_views, n_rows, n_channels], the packed upper triangle of the symmetric positive semi-definite W_i
    (``precision_weights``); ``beta``, ``delta``: a scalar or one value per channel; x0: start images [K, nz, ny, nx] (default
    zeros; not modified).  Per subset, with R = A 1:

        q_k  = sum_l W_kl (A_s x_l - b_l)                  on the lines of the subset, 0 where R = 0
        g_k  = S A_s^T q_k
        d_k  = A^T((sum_l |W_kl|) R)                       once, over ALL views
        p_kj = beta_k sum_(n in N(j)) clip(x_kj - x_kn, +-delta_k)
        c_kj = 2 beta_k sum_(n in N(j)) min(1, delta_k / |x_kj - x_kn|)
        x_kj <- x_kj - (g_kj + p_kj) / (d_kj + c_kj)       where the denominator > 0 (other pixels stay); max(., 0) if nonneg

    a Jacobi step between two image buffers.  d majorises the data Hessian for every symmetric positive semi-definite W because
    a_ij >= 0 (row (k, j) of |H| 1 is d_kj), so with one subset Phi never increases.  The K channels go through the
    projector pair one call each.  ``history``: a list that receives Phi of the images BEFORE each iteration, data term (over
    the rays with R > 0) plus penalty, summed in float64 on the device (one host synchronisation per iteration; with more than
    one subset also one full forward projection per iteration, as ``sirt``).  Returns the images [K, nz, ny, nx]."""
    n_iters, S = int(n_iters), int(n_subsets)
    if n_iters < 1 or not 1 <= S <= proj.n_views:
        raise ValueError(f'n_iters = {n_iters}, n_subsets = {S}: n_iters >= 1 and 1 <= n_subsets <= {proj.n_views} wanted')
    if not isinstance(sinos_d, torch.Tensor):
        sinos_d = torch.stack([t.reshape(proj.sino_shape) for t in sinos_d])
    K = int(sinos_d.shape[0]) if sinos_d.dim() == len(proj.sino_shape) + 1 else 0
    if not 1 <= K <= PWLS_MAX_CHANNELS:
        raise ValueError(f'sinograms {tuple(sinos_d.shape)}: [K, n_views, n_rows, n_channels] with K = 1 .. {PWLS_MAX_CHANNELS} wanted')
    T = K * (K + 1) // 2
    betas, deltas = per_channel(beta, K, 'beta'), per_channel(delta, K, 'delta', positive=True)
    b = proj._tensor(sinos_d, (K,) + proj.sino_shape, 'sinograms')
    w = proj._tensor(weights_d, (T,) + proj.sino_shape, 'weights')
    if x0 is not None:
        proj._tensor(x0, (K,) + proj.image_shape, 'x0')
    proj._ready()
    lib, dev = proj.lib, proj.dev
    x = torch.zeros((K,) + proj.image_shape, dtype=torch.float32, device=dev) if x0 is None else x0.clone()
    y = torch.empty_like(x)
    R = proj.row_sums()
    d = _pwls_majoriser(proj, w, K)
    ax = torch.zeros((K,) + proj.sino_shape, dtype=torch.float32, device=dev)
    g = torch.empty((K,) + proj.image_shape, dtype=torch.float32, device=dev)
    phi = torch.zeros(2, dtype=torch.float64, device=dev) if history is not None else None      # data term, penalty
    line = proj.n_rows * proj.n_channels
    n_views, plane = proj.n_views, proj.n_views * line
    beta_c, delta_c = (C.c_double * K)(*betas), (C.c_double * K)(*deltas)
    data_ptr = None if phi is None else phi.data_ptr()
    pen_ptr = None if phi is None else phi.data_ptr() + 8

    def residual(s, step, q, objective):
        off = 4 * s * line
        _native.check(lib.dexct_pwls_residual(b.data_ptr() + off, ax.data_ptr() + off, w.data_ptr() + off, R.data_ptr() + off, plane,
                                              K, n_views - s, step, line, None if q is None else q.data_ptr() + off, objective,
                                              stream_ptr()), 'dexct_pwls_residual')

    for _ in range(n_iters):
        if history is not None and S > 1:                  # (with one subset the iteration's own residual is the one wanted)
            for k in range(K):
                proj.forward(x[k], out=ax[k])
            residual(0, 1, None, data_ptr)
        for s in range(S):
            views = (s, n_views, S)
            for k in range(K):
                proj.forward(x[k], views=views, out=ax[k])
            residual(s, S, ax, data_ptr if S == 1 else None)
            for k in range(K):
                proj.adjoint(ax[k], views=views, out=g[k])
            _native.check(lib.dexct_pwls_update(ptr(x), ptr(g), ptr(d), K, proj.nz, proj.ny, proj.nx, float(S), beta_c, delta_c,
                                                int(bool(nonneg)), ptr(y), pen_ptr if s == 0 else None, stream_ptr()),
                          'dexct_pwls_update')
            x, y = y, x
            if history is not None and s == 0:
                data, penalty = phi.tolist()
                history.append(data + penalty)
    return x
