"""Every call the reconstruction's Python layer refuses without a device, as one table: get_recon (FBP, SIRT, OS-SART, PWLS),
get_basismat_recon, get_recon_covariance, recon_covariance_device (its host-side type check), ramp_taps, check_options,
check_pwls_options, ImageProjector and the argument tests of sirt and pwls that fire before the projector's device state is built.

Each row holds the keywords that depart from a call that would pass, the exception's type and its FULL message.  A row MUST be a
refused call: without a device, one that passed its checks would fail further on for want of one, which pins nothing.  Every
check has a row that trips it alone; the last rows of each block trip two or three at once, so that the message that comes out
tells which check runs first.  Types and messages are literals recorded from the package as it was before the reconstruction
calls got their shared helpers (back_project.py, iterative.py); nothing is computed from the code under test.

Not reachable without a device, hence not here: what get_recon(method='fbp' / 'sirt') and recon_device refuse after the upload
(the sinogram's shape, the window, the rotation, the rows of a cone), the weights that are not finite and non-negative, and
ImageProjector's tensor and view checks (tests/test_gpu_recon_layer.py).  ``world=2`` stands for a process group of two."""
import numpy as np
import pytest
import torch

import dex_ct_sim_amd as dx
from dex_ct_sim_amd import _shard, back_project as bp, iterative as it

inf, nan = float('inf'), float('nan')


def scanner(name):
    """12 views by 16 channels unless the name says otherwise"""
    kw = dict(N_channels=16, N_proj=12)
    kw.update({'fan': {}, 'cone': dict(N_rows=4, cone=True),
               'less-than-short': dict(theta_tot=np.pi),
               'two-turns': dict(theta_tot=4 * np.pi),
               'cone-less-than-short': dict(N_rows=4, cone=True, theta_tot=np.pi),
               'wide': dict(N_channels=4096)}[name])
    return dx.FanBeamGeometry(**kw)


class OnDevice(np.ndarray):
    """What get_recon takes for a device tensor without a device: an array that says it is one."""
    is_cuda = True


def array(spec, dtype=np.float32):
    if isinstance(spec, tuple) and spec and spec[0] == 'device':
        return np.ones(spec[1], dtype).view(OnDevice)
    return None if spec is None else np.ones(spec, dtype)


def get_recon(ct='fan', sino=(12, 16), FOV=20.0, weights=None, **kw):
    return bp.get_recon(array(sino), scanner(ct), None, 16, FOV, 1.0, weights=array(weights), **kw)


def get_basismat_recon(ct='fan', sinos=((12, 16), (12, 16)), cov=(12, 16, 3), FOV=20.0, beta=0.1, delta=0.01, **kw):
    return bp.get_basismat_recon([array(s) for s in sinos], array(cov, np.float64), scanner(ct), 16, FOV, 1.0, beta, delta, **kw)


def get_recon_covariance(ct='fan', cov=(12, 16, 3), **kw):
    return bp.get_recon_covariance(array(cov, np.float64), scanner(ct), 16, 20.0, 1.0, **kw)


def recon_covariance_device(cov='numpy'):
    x = {'numpy': np.ones((12, 16, 1)), 'host-float64': torch.ones(12, 16, 1, dtype=torch.float64), 'none': None}[cov]
    return bp.recon_covariance_device(x, scanner('fan'), 16, 20.0, 1.0)


def check_options(method='sirt', ct='fan', n_iters=20, n_subsets=1, relax=1.0, **kw):
    return it.check_options(method, scanner(ct), n_iters, n_subsets, relax, **kw)


def check_pwls_options(ct='fan', K=2, n_iters=20, n_subsets=1, beta=0.1, delta=0.01, **kw):
    return it.check_pwls_options(scanner(ct), K, n_iters, n_subsets, beta, delta, **kw)


def image_projector(ct='fan', N_matrix=16, FOV=20.0, **kw):
    return it.ImageProjector(scanner(ct), N_matrix, FOV, **kw)


def from_grid(nz=4, n_rows=2, z_first=0, dx_=1.0):
    ct = scanner('fan')
    return it.ImageProjector.from_grid(16, 16, nz, dx_, 1.0, 12, 16, n_rows, z_first, ct.SID, ct.SDD, ct.view_cs(), ct.chan_cs())


def sirt(n_iters=5, **kw):
    """the sinogram is host memory: a call that got past the argument tests would fail in _ready() for want of a device"""
    return it.sirt(torch.zeros(12, 1, 16), it.ImageProjector(scanner('fan'), 16, 20.0), n_iters, **kw)


def pwls(sinos=(2, 12, 1, 16), n_iters=5, **kw):
    return it.pwls(torch.zeros(sinos), torch.zeros((3, 12, 1, 16)), it.ImageProjector(scanner('fan'), 16, 20.0), n_iters, **kw)


def ramp_taps(**kw):
    return bp.ramp_taps(16, 0.05, **kw)


# the messages that many rows share
NO_PAIR = 'iterative reconstruction is fan and stacked-fan only: a cone-beam scanner has no matched pair here'
OUTSIDE = 'FOV = 84.86 cm: the image grid does not lie strictly inside the source circle (SID = 60.0 cm)'
WINDOW = "unknown filter window 'boxcar'; choose from ['cosine', 'hamming', 'hann', 'rect', 'sinc']"
TOO_SHORT = 'rotation_angle_total = 3.14159 rad is less than a short scan (pi + fan angle = 3.91319 rad): projections are missing'
TWO_TURNS = 'rotation_angle_total = 12.5664 exceeds 2 pi: more than one rotation is not reconstructed'
HOST_ARRAYS = 'get_recon takes host arrays: device tensors go to get_basismat_recon or iterative.pwls'
NO_SLICES = "slices belong to the cone-beam FBP: method='pwls' reconstructs the rows of the sinogram"
NO_WEIGHTS = "method='pwls' needs weights: the inverse variance of every sinogram value"
NO_PLANE_AXIS = ' has no plane axis: pass a single variance sinogram as var[..., None]'
COV_DIMS = 'covariance sinogram must be [N_proj, N_channels, T] or [N_proj, N_rows, N_channels, T], got '
SIRT_WANTS = ': n_iters >= 1, 1 <= n_subsets <= 12 and 0 < relax < 2 wanted'
GRID_OUTSIDE = ' does not lie strictly inside the source circle (SID = 60 cm)'
PWLS_SINOS = ': [K, n_views, n_rows, n_channels] with K = 1 .. 3 wanted'

CASES = {
    get_recon: [
        (dict(method='art'), ValueError, "unknown reconstruction method 'art'; choose from ('fbp', 'sirt', 'os-sart')"),
        (dict(method='fbp', weights=(12, 16)), ValueError, "weights belong to method='pwls', not to 'fbp'"),
        (dict(method='sirt', weights=(12, 16)), ValueError, "weights belong to method='pwls', not to 'sirt'"),
        (dict(method='art', weights=(12, 16)), ValueError, "weights belong to method='pwls', not to 'art'"),
        (dict(method='sirt', ct='cone', sino=(12, 4, 16)), ValueError, NO_PAIR),
        (dict(method='os-sart', ct='cone', sino=(12, 4, 16)), ValueError, NO_PAIR),
        (dict(method='sirt', FOV=84.86), ValueError, OUTSIDE),
        (dict(method='sirt', init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(method='os-sart', init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(method='sirt', n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(method='sirt', relax=0.0), ValueError, 'relax = 0.0 lies outside (0, 2)'),
        (dict(method='sirt', relax=2.0), ValueError, 'relax = 2.0 lies outside (0, 2)'),
        (dict(method='sirt', relax=nan), ValueError, 'relax = nan lies outside (0, 2)'),
        (dict(method='sirt', n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(method='sirt', n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(method='os-sart', n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(method='os-sart', n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(method='sirt', n_iters=0, relax=2.0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(method='sirt', relax=2.0, n_subsets=0), ValueError, 'relax = 2.0 lies outside (0, 2)'),
        (dict(method='sirt', ct='cone', sino=(12, 4, 16), init='ones'), ValueError, NO_PAIR),
        (dict(method='sirt', FOV=84.86, init='ones'), ValueError, OUTSIDE),
        (dict(method='sirt', init='ones', n_iters=0), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(method='sirt', ct='cone', FOV=84.86), ValueError, NO_PAIR),
        (dict(method='pwls', weights=(12, 16), ct='cone'), ValueError, NO_PAIR),
        (dict(method='pwls', weights=(12, 16), FOV=84.86), ValueError, OUTSIDE),
        (dict(method='pwls', weights=(12, 16), init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(method='pwls', weights=(12, 16), n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(method='pwls', weights=(12, 16), n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(method='pwls', weights=(12, 16), n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(method='pwls', weights=(12, 16), beta=-0.1), ValueError, 'beta = -0.1: non-negative finite values wanted'),
        (dict(method='pwls', weights=(12, 16), beta=(0.1, 0.2)), ValueError, 'beta = (0.1, 0.2): a scalar or one value per channel (1) wanted'),
        (dict(method='pwls', weights=(12, 16), beta=inf), ValueError, 'beta = inf: non-negative finite values wanted'),
        (dict(method='pwls', weights=(12, 16), delta=0.0), ValueError, 'delta = 0.0: positive finite values wanted'),
        (dict(method='pwls', weights=(12, 16), delta=nan), ValueError, 'delta = nan: positive finite values wanted'),
        (dict(method='pwls', weights=(12, 16), delta=(0.1, 0.1)), ValueError, 'delta = (0.1, 0.1): a scalar or one value per channel (1) wanted'),
        (dict(method='pwls'), ValueError, NO_WEIGHTS),
        (dict(method='pwls', weights=(12, 16), slices=(1, 0.0, 0.1)), ValueError, NO_SLICES),
        (dict(method='pwls', weights=('device', (12, 16))), ValueError, HOST_ARRAYS),
        (dict(method='pwls', weights=(12, 16), sino=('device', (12, 16))), ValueError, HOST_ARRAYS),
        (dict(method='pwls', weights=(12, 15)), ValueError, 'weights (12, 15) do not have the shape of the sinogram (12, 16)'),
        (dict(method='pwls', weights=(12, 1, 16)), ValueError, 'weights (12, 1, 16) do not have the shape of the sinogram (12, 16)'),
        (dict(method='pwls', weights=(11, 16), sino=(11, 16)), ValueError, 'sinogram (11, 16) does not match the scanner (12 x 16)'),
        (dict(method='pwls', weights=(12, 15), sino=(12, 15)), ValueError, 'sinogram (12, 15) does not match the scanner (12 x 16)'),
        (dict(method='pwls', weights=(12,), sino=(12,)), ValueError, 'sinogram (12,) does not match the scanner (12 x 16)'),
        (dict(method='pwls', weights=(12, 1, 16, 1), sino=(12, 1, 16, 1)), ValueError, 'sinogram (12, 1, 16, 1) does not match the scanner (12 x 16)'),
        (dict(method='pwls', weights=(12, 16), world=2), NotImplementedError, "get_recon(method='pwls') runs on a single process"),
        (dict(method='pwls', n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(method='pwls', weights=(12, 15), sino=(11, 16)), ValueError, 'weights (12, 15) do not have the shape of the sinogram (11, 16)'),
        (dict(method='pwls', weights=('device', (12, 16)), slices=(1, 0.0, 0.1)), ValueError, NO_SLICES),
        (dict(method='pwls', weights=(12, 16), delta=0.0, n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(method='pwls', slices=(1, 0.0, 0.1)), ValueError, NO_WEIGHTS),
        (dict(method='pwls', weights=('device', (12, 15))), ValueError, HOST_ARRAYS),
        (dict(method='pwls', weights=(12, 16), beta=-0.1, delta=0.0), ValueError, 'beta = -0.1: non-negative finite values wanted'),
        (dict(method='pwls', weights=(11, 16), sino=(11, 16), world=2), ValueError, 'sinogram (11, 16) does not match the scanner (12 x 16)'),
        (dict(method='pwls', weights=(12, 16), ct='cone', init='ones'), ValueError, NO_PAIR),
    ],
    get_basismat_recon: [
        (dict(sinos=(), cov=(12, 16, 0)), ValueError, '0 channels: the joint reconstruction takes 1 .. 3'),
        (dict(sinos=((12, 16), (12, 16), (12, 16), (12, 16)), cov=(12, 16, 10)), ValueError, '4 channels: the joint reconstruction takes 1 .. 3'),
        (dict(ct='cone'), ValueError, NO_PAIR),
        (dict(FOV=84.86), ValueError, OUTSIDE),
        (dict(init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(beta=-0.1), ValueError, 'beta = -0.1: non-negative finite values wanted'),
        (dict(beta=(0.1, 0.1, 0.1)), ValueError, 'beta = (0.1, 0.1, 0.1): a scalar or one value per channel (2) wanted'),
        (dict(delta=0.0), ValueError, 'delta = 0.0: positive finite values wanted'),
        (dict(delta=(0.1, nan)), ValueError, 'delta = (0.1, nan): positive finite values wanted'),
        (dict(sinos=((12, 16), (12, 15))), ValueError, 'the basis sinograms differ in shape: [(12, 16), (12, 15)]'),
        (dict(sinos=((11, 16), (11, 16)), cov=(11, 16, 3)), ValueError, 'sinogram (11, 16) does not match the scanner (12 x 16)'),
        (dict(sinos=((12, 15), (12, 15)), cov=(12, 15, 3)), ValueError, 'sinogram (12, 15) does not match the scanner (12 x 16)'),
        (dict(sinos=((12,), (12,)), cov=(12, 3)), ValueError, 'sinogram (12,) does not match the scanner (12 x 16)'),
        (dict(sinos=((12, 1, 16, 1), (12, 1, 16, 1)), cov=(12, 1, 16, 1, 3)), ValueError, 'sinogram (12, 1, 16, 1) does not match the scanner (12 x 16)'),
        (dict(cov=(12, 16, 6)), ValueError, 'covariance sinogram (12, 16, 6): (12, 16, 3) wanted for 2 sinogram(s) of shape (12, 16)'),
        (dict(cov=(12, 16)), ValueError, 'covariance sinogram (12, 16): (12, 16, 3) wanted for 2 sinogram(s) of shape (12, 16)'),
        (dict(cov=(12, 1, 16, 3)), ValueError, 'covariance sinogram (12, 1, 16, 3): (12, 16, 3) wanted for 2 sinogram(s) of shape (12, 16)'),
        (dict(w_fill=-1.0), ValueError, 'w_fill = -1.0: a finite value >= 0 wanted'),
        (dict(w_fill=inf), ValueError, 'w_fill = inf: a finite value >= 0 wanted'),
        (dict(w_fill=nan), ValueError, 'w_fill = nan: a finite value >= 0 wanted'),
        (dict(window='boxcar'), ValueError, WINDOW),
        (dict(ct='less-than-short'), ValueError, TOO_SHORT),
        (dict(ct='two-turns'), ValueError, TWO_TURNS),
        (dict(world=2), NotImplementedError, 'get_basismat_recon runs on a single process'),
        (dict(sinos=((11, 16), (11, 16)), w_fill=-1.0), ValueError, 'sinogram (11, 16) does not match the scanner (12 x 16)'),
        (dict(w_fill=-1.0, window='boxcar'), ValueError, 'w_fill = -1.0: a finite value >= 0 wanted'),
        (dict(window='boxcar', ct='less-than-short'), ValueError, WINDOW),
        (dict(n_subsets=13, sinos=((12, 16), (12, 15))), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(sinos=((12, 16), (11, 16)), cov=(12, 16, 6)), ValueError, 'the basis sinograms differ in shape: [(12, 16), (11, 16)]'),
        (dict(cov=(12, 16, 6), w_fill=-1.0), ValueError, 'covariance sinogram (12, 16, 6): (12, 16, 3) wanted for 2 sinogram(s) of shape (12, 16)'),
        (dict(ct='less-than-short', world=2), ValueError, TOO_SHORT),
        (dict(delta=0.0, sinos=((11, 16), (11, 16))), ValueError, 'delta = 0.0: positive finite values wanted'),
        (dict(sinos=((12, 16), (12, 16), (12, 16), (12, 16)), ct='cone'), ValueError, '4 channels: the joint reconstruction takes 1 .. 3'),
    ],
    get_recon_covariance: [
        (dict(cov=(12, 16)), ValueError, 'covariance sinogram (12, 16)' + NO_PLANE_AXIS),
        (dict(cov=(12,)), ValueError, COV_DIMS + '(12,)'),
        (dict(cov=(12, 16, 3, 1, 1)), ValueError, COV_DIMS + '(12, 16, 3, 1, 1)'),
        (dict(cov=(11, 16, 3)), ValueError, 'covariance sinogram (11, 16, 3) does not match the scanner (12 x 16)'),
        (dict(cov=(12, 15, 3)), ValueError, 'covariance sinogram (12, 15, 3) does not match the scanner (12 x 16)'),
        (dict(cov=(12, 2, 15, 3)), ValueError, 'covariance sinogram (12, 2, 15, 3) does not match the scanner (12 x 16)'),
        (dict(cov=(12, 16, 0)), ValueError, 'covariance sinogram has no planes'),
        (dict(window='boxcar'), ValueError, WINDOW),
        (dict(ct='less-than-short', cov=(12, 16, 1)), ValueError, TOO_SHORT),
        (dict(ct='two-turns'), ValueError, TWO_TURNS),
        (dict(ct='cone', cov=(12, 3, 16, 1)), ValueError, 'covariance sinogram has 3 rows, the scanner 4'),
        (dict(ct='wide', cov=(12, 4096, 1)), ValueError, '4096 channels: the variance filter takes at most 2730'),
        (dict(world=2), NotImplementedError, 'get_recon_covariance runs on a single process'),
        (dict(cov=(12, 16), window='boxcar'), ValueError, 'covariance sinogram (12, 16)' + NO_PLANE_AXIS),
        (dict(cov=(11, 16, 0)), ValueError, 'covariance sinogram (11, 16, 0) does not match the scanner (12 x 16)'),
        (dict(cov=(12, 16, 0), window='boxcar'), ValueError, 'covariance sinogram has no planes'),
        (dict(window='boxcar', ct='cone-less-than-short', cov=(12, 3, 16, 1)), ValueError, WINDOW),
        (dict(ct='cone-less-than-short', cov=(12, 3, 16, 1)), ValueError, TOO_SHORT),
        (dict(ct='cone', cov=(12, 3, 16, 1), world=2), ValueError, 'covariance sinogram has 3 rows, the scanner 4'),
        (dict(ct='wide', cov=(12, 4096, 1), world=2), ValueError, '4096 channels: the variance filter takes at most 2730'),
        (dict(cov=(12, 15), ct='two-turns'), ValueError, 'covariance sinogram (12, 15)' + NO_PLANE_AXIS),
    ],
    ramp_taps: [
        (dict(window='boxcar'), ValueError, WINDOW),
        (dict(window=None), ValueError, "unknown filter window None; choose from ['cosine', 'hamming', 'hann', 'rect', 'sinc']"),
    ],
    recon_covariance_device: [
        (dict(cov='numpy'), ValueError, 'cov_d must be a float64 device tensor'),
        (dict(cov='host-float64'), ValueError, 'cov_d must be a float64 device tensor'),
        (dict(cov='none'), ValueError, 'cov_d must be a float64 device tensor'),
    ],
    check_options: [
        (dict(method='art'), ValueError, "unknown reconstruction method 'art'; choose from ('fbp', 'sirt', 'os-sart')"),
        (dict(method='pwls'), ValueError, "unknown reconstruction method 'pwls'; choose from ('fbp', 'sirt', 'os-sart')"),
        (dict(ct='cone'), ValueError, NO_PAIR),
        (dict(FOV=84.86), ValueError, OUTSIDE),
        (dict(init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(relax=0.0), ValueError, 'relax = 0.0 lies outside (0, 2)'),
        (dict(relax=2.0), ValueError, 'relax = 2.0 lies outside (0, 2)'),
        (dict(n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(method='os-sart', n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(method='art', ct='cone'), ValueError, "unknown reconstruction method 'art'; choose from ('fbp', 'sirt', 'os-sart')"),
        (dict(ct='cone', FOV=84.86), ValueError, NO_PAIR),
        (dict(FOV=84.86, init='ones'), ValueError, OUTSIDE),
        (dict(init='ones', n_iters=0), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(n_iters=0, relax=2.0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(relax=2.0, n_subsets=0), ValueError, 'relax = 2.0 lies outside (0, 2)'),
    ],
    check_pwls_options: [
        (dict(K=0), ValueError, '0 channels: the joint reconstruction takes 1 .. 3'),
        (dict(K=4), ValueError, '4 channels: the joint reconstruction takes 1 .. 3'),
        (dict(ct='cone'), ValueError, NO_PAIR),
        (dict(FOV=84.86), ValueError, OUTSIDE),
        (dict(init='ones'), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(n_iters=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(n_subsets=0), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(n_subsets=13), ValueError, 'n_subsets = 13 lies outside 1 .. N_proj = 12'),
        (dict(n_subsets=0.5), ValueError, 'n_subsets = 0.5 lies outside 1 .. N_proj = 12'),
        (dict(beta=-0.1), ValueError, 'beta = -0.1: non-negative finite values wanted'),
        (dict(beta=(0.1, 0.1, 0.1)), ValueError, 'beta = (0.1, 0.1, 0.1): a scalar or one value per channel (2) wanted'),
        (dict(beta=nan), ValueError, 'beta = nan: non-negative finite values wanted'),
        (dict(delta=0.0), ValueError, 'delta = 0.0: positive finite values wanted'),
        (dict(delta=(0.1, nan)), ValueError, 'delta = (0.1, nan): positive finite values wanted'),
        (dict(delta=(0.1, 0.1, 0.1)), ValueError, 'delta = (0.1, 0.1, 0.1): a scalar or one value per channel (2) wanted'),
        (dict(K=4, ct='cone'), ValueError, '4 channels: the joint reconstruction takes 1 .. 3'),
        (dict(ct='cone', FOV=84.86), ValueError, NO_PAIR),
        (dict(FOV=84.86, init='ones'), ValueError, OUTSIDE),
        (dict(init='ones', n_iters=0), ValueError, "init must be 'fbp' or 'zero', not 'ones'"),
        (dict(n_iters=0, n_subsets=0), ValueError, 'n_iters = 0: at least one iteration'),
        (dict(n_subsets=0, beta=-0.1), ValueError, 'n_subsets = 0 lies outside 1 .. N_proj = 12'),
        (dict(beta=-0.1, delta=0.0), ValueError, 'beta = -0.1: non-negative finite values wanted'),
    ],
    image_projector: [
        (dict(ct='cone'), ValueError, 'ImageProjector is fan and stacked-fan only: a cone-beam scanner has no matched pair here'),
        (dict(N_matrix=0), ValueError, 'N_matrix = 0, FOV = 20.0, n_slices = 1: positive values wanted'),
        (dict(FOV=0.0), ValueError, 'N_matrix = 16, FOV = 0.0, n_slices = 1: positive values wanted'),
        (dict(FOV=nan), ValueError, 'N_matrix = 16, FOV = nan, n_slices = 1: positive values wanted'),
        (dict(n_slices=0), ValueError, 'N_matrix = 16, FOV = 20.0, n_slices = 0: positive values wanted'),
        (dict(FOV=84.86), ValueError, 'the image grid (84.86 x 84.86 cm, half diagonal 60.0051 cm)' + GRID_OUTSIDE),
        (dict(FOV=90.0), ValueError, 'the image grid (90 x 90 cm, half diagonal 63.6396 cm)' + GRID_OUTSIDE),
        (dict(ct='cone', N_matrix=0), ValueError, 'ImageProjector is fan and stacked-fan only: a cone-beam scanner has no matched pair here'),
        (dict(N_matrix=0, FOV=90.0), ValueError, 'N_matrix = 0, FOV = 90.0, n_slices = 1: positive values wanted'),
    ],
    from_grid: [
        (dict(z_first=-1), ValueError, 'rows -1 .. 0 lie outside the 4 slices'),
        (dict(n_rows=0), ValueError, 'rows 0 .. -1 lie outside the 4 slices'),
        (dict(z_first=3), ValueError, 'rows 3 .. 4 lie outside the 4 slices'),
        (dict(dx_=10.0), ValueError, 'the image grid (160 x 16 cm, half diagonal 80.399 cm)' + GRID_OUTSIDE),
        (dict(dx_=10.0, n_rows=0), ValueError, 'the image grid (160 x 16 cm, half diagonal 80.399 cm)' + GRID_OUTSIDE),
    ],
    sirt: [
        (dict(n_iters=0), ValueError, 'n_iters = 0, n_subsets = 1, relax = 1.0' + SIRT_WANTS),
        (dict(n_subsets=0), ValueError, 'n_iters = 5, n_subsets = 0, relax = 1.0' + SIRT_WANTS),
        (dict(n_subsets=13), ValueError, 'n_iters = 5, n_subsets = 13, relax = 1.0' + SIRT_WANTS),
        (dict(relax=0.0), ValueError, 'n_iters = 5, n_subsets = 1, relax = 0.0' + SIRT_WANTS),
        (dict(relax=2.0), ValueError, 'n_iters = 5, n_subsets = 1, relax = 2.0' + SIRT_WANTS),
        (dict(n_iters=0, n_subsets=13, relax=2.5), ValueError, 'n_iters = 0, n_subsets = 13, relax = 2.5' + SIRT_WANTS),
    ],
    pwls: [
        (dict(n_iters=0), ValueError, 'n_iters = 0, n_subsets = 1: n_iters >= 1 and 1 <= n_subsets <= 12 wanted'),
        (dict(n_subsets=0), ValueError, 'n_iters = 5, n_subsets = 0: n_iters >= 1 and 1 <= n_subsets <= 12 wanted'),
        (dict(n_subsets=13), ValueError, 'n_iters = 5, n_subsets = 13: n_iters >= 1 and 1 <= n_subsets <= 12 wanted'),
        (dict(n_iters=0, n_subsets=13), ValueError, 'n_iters = 0, n_subsets = 13: n_iters >= 1 and 1 <= n_subsets <= 12 wanted'),
        (dict(sinos=(12, 1, 16)), ValueError, 'sinograms (12, 1, 16)' + PWLS_SINOS),
        (dict(sinos=(4, 12, 1, 16)), ValueError, 'sinograms (4, 12, 1, 16)' + PWLS_SINOS),
        (dict(sinos=(0, 12, 1, 16)), ValueError, 'sinograms (0, 12, 1, 16)' + PWLS_SINOS),
        (dict(beta=-0.1), ValueError, 'beta = -0.1: non-negative finite values wanted'),
        (dict(beta=(0.1, 0.1, 0.1)), ValueError, 'beta = (0.1, 0.1, 0.1): a scalar or one value per channel (2) wanted'),
        (dict(delta=0.0), ValueError, 'delta = 0.0: positive finite values wanted'),
        (dict(delta=(0.1, nan)), ValueError, 'delta = (0.1, nan): positive finite values wanted'),
        (dict(n_iters=0, sinos=(12, 1, 16)), ValueError, 'n_iters = 0, n_subsets = 1: n_iters >= 1 and 1 <= n_subsets <= 12 wanted'),
        (dict(sinos=(4, 12, 1, 16), beta=-0.1), ValueError, 'sinograms (4, 12, 1, 16)' + PWLS_SINOS),
        (dict(beta=-0.1, delta=0.0), ValueError, 'beta = -0.1: non-negative finite values wanted'),
    ],
}

TABLE = [pytest.param(fn, kw, exc, msg, id=f'{fn.__name__}-{i:02d}-' + '-'.join(f'{k}={v}' for k, v in kw.items()))
         for fn, cases in CASES.items() for i, (kw, exc, msg) in enumerate(cases)]


@pytest.mark.parametrize('fn,kw,exc,msg', TABLE)
def test_refused_call_raises_the_recorded_message(monkeypatch, fn, kw, exc, msg):
    kw = dict(kw)
    world = kw.pop('world', 1)
    monkeypatch.setattr(_shard, 'world', lambda: (0, world))
    with pytest.raises(exc) as info:
        fn(**kw)
    assert type(info.value) is exc and str(info.value) == msg
