"""The tensor contract of the device entry points, as far as it can be checked without a GPU ("tensor
contract"; dex-ct-sim_amd/_device.py: dense_input, written, device_scalar, gpu_of).

1. The helpers' own rules on CPU tensors: identity for conforming tensors, densifying, each cast, each refusal with its full
   message.
2. The in-bounds rule of tests/tensor_views.py for every recipe at every shape tests/test_gpu_tensor_contract.py uses.
3. For every entry point: the calls it must refuse - a host tensor where a device tensor is documented, an ``out`` of the wrong
   dtype, one element short, one element long or not dense, a two-element ``mask_max`` - raise ValueError BEFORE the native
   library is asked for anything: ``_native.load`` is replaced by a stub that fails the test when it is called, as is every
   attribute of a projector's ``lib``.  The stand-in for device memory is torch's 'meta' device (shapes, strides and dtypes
   without storage): ``_device.GPU`` is set to it, so that the arguments that are NOT under test pass.
   As in tests/test_recon_args.py every row must be a refused call.
4. For conforming tensors every entry point hands on the very object it was given (``is``): the benchmark's step neither copies
   nor synchronises more than before.

The functions documented "NumPy in -> NumPy out, tensor in -> tensor out" (get_basismat_sinos, get_basismat_sinos_multi,
do_matdecomp_gn, get_basismat_covariance, get_basismat_recon, get_recon_covariance, plots.vmi_*) upload whatever they are
given (to_dev, _as_device_counts) and refuse no tensor: they have no rows here; the GPU module checks that they normalise."""
import types

import numpy as np
import pytest
import torch

import dex_ct_sim_amd as dx
import tensor_views as tv
from dex_ct_sim_amd import _device, _native, back_project as bp, bhc, forward_project as fp, iterative as it, matdecomp as md

CPU, FAKE = torch.device('cpu'), torch.device('meta')
F32, F64, U8 = torch.float32, torch.float64, torch.uint8


# ---- 1. the helpers ----------------------------------------------------------------------------------------------------------------

def test_conforming_tensors_come_back_as_the_same_object():
    for dt in (F32, F64):
        t = torch.arange(24, dtype=dt).reshape(2, 3, 4)
        assert _device.dense_input(t, 'x', CPU, **_device.COUNTS) is t
        off = torch.zeros(30, dtype=dt)[3:27].view(2, 3, 4)                 # dense at an offset: conforms
        assert _device.dense_input(off, 'x', CPU, **_device.COUNTS) is off
        assert _device.written(t, 'out', CPU, dt, 24) is t and _device.written(t, 'ws', CPU, dt, 20, at_least=True) is t
    s = torch.tensor(5.0, dtype=F64)
    assert _device.device_scalar(s, 'mask_max', CPU) is s
    one = torch.ones(1, 1, dtype=F64)
    assert _device.device_scalar(one, 'mask_max', CPU) is one


@pytest.mark.parametrize('shape', [(6,), (3, 4), (2, 3, 4)])
def test_views_are_made_dense_and_dtypes_cast(shape):
    x = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
    for r in tv.variants(x):
        t = r.build(CPU)
        got = _device.dense_input(t, 'x', CPU, **_device.COUNTS)
        assert got.is_contiguous() and np.array_equal(got.double().numpy(), x.astype(np.float64)), r
        want = t.dtype if t.dtype in (F32, F64) else F64                    # counts: float32 and float64 stay, the rest -> float64
        assert got.dtype == want, r
        assert (got is t) == r.conforms or r.name == 'float64', r           # (float64 counts conform too)
        got = _device.dense_input(t, 'x', CPU, keep=(F32,), cast=F32)       # recon_device's rule
        assert got.dtype == F32 and got.is_contiguous() and np.array_equal(got.numpy(), x), r
    b = np.broadcast_to(np.arange(4, dtype=np.float64), (3, 4))
    t = [r for r in tv.variants(b) if r.name == 'broadcast'][0].build(CPU)
    assert t.stride(0) == 0 and np.array_equal(_device.dense_input(t, 'x', CPU, **_device.COUNTS).numpy(), b)
    s32 = torch.tensor(7.0, dtype=F32)
    got = _device.device_scalar(s32, 'mask_max', CPU)
    assert got.dtype == F64 and got.item() == 7.0


def test_refusals_and_their_messages():
    def refused(message, fn, *a, **kw):
        with pytest.raises(ValueError) as info:
            fn(*a, **kw)
        assert str(info.value) == message

    t = torch.zeros(2, 3, dtype=F32)
    refused('g1 must be a device tensor (got a tensor on cpu)', _device.gpu_of, t, 'g1')
    refused('g1 must be a device tensor (got ndarray)', _device.gpu_of, np.zeros(3), 'g1')
    refused('x must be a tensor on meta (got a tensor on cpu)', _device.dense_input, t, 'x', FAKE)
    refused('x must be a tensor on cpu (got ndarray)', _device.dense_input, np.zeros(3), 'x', CPU)
    refused('x must be a tensor on cpu (got NoneType)', _device.dense_input, None, 'x', CPU)
    refused('x must be float64 (got float32)', _device.dense_input, t, 'x', CPU, keep=(F64,))
    refused('x must be float32 or float64 (got int32)', _device.dense_input, t.int(), 'x', CPU, keep=(F32, F64))
    refused('out must be a tensor on meta (got a tensor on cpu)', _device.written, t, 'out', FAKE, F32, 6)
    refused('out must be a tensor on cpu (got ndarray)', _device.written, np.zeros(6), 'out', CPU, F32, 6)
    refused('out must be float64 (got float32)', _device.written, t, 'out', CPU, F64, 6)
    refused('out must hold 7 float32 elements (got 6)', _device.written, t, 'out', CPU, F32, 7)
    refused('out must hold 5 float32 elements (got 6)', _device.written, t, 'out', CPU, F32, 5)
    refused('ws must hold at least 7 float32 elements (got 6)', _device.written, t, 'ws', CPU, F32, 7, at_least=True)
    refused('out must be contiguous (got shape (3, 2) with strides (1, 3))', _device.written, t.t(), 'out', CPU, F32, 6)
    refused('out must be contiguous (got shape (2, 2) with strides (3, 2))', _device.written, t[:, ::2], 'out', CPU, F32, 4)
    d = torch.zeros(16, dtype=F64)
    assert d.data_ptr() % 16 == 0 and _device.written(d[2:8], 'out', CPU, F64, 6, align=16) is not None
    refused('out must start on a 16-byte boundary (its data starts 8 bytes past one)', _device.written, d[1:7], 'out', CPU, F64, 6, align=16)
    refused('mask_max must be a one-element float64 tensor on meta (got a tensor on cpu)', _device.device_scalar, t, 'mask_max', FAKE)
    refused('mask_max must be a one-element float64 tensor on cpu (got float)', _device.device_scalar, 3.0, 'mask_max', CPU)
    refused('mask_max must hold one element (got 2)', _device.device_scalar, torch.zeros(2, dtype=F64), 'mask_max', CPU)
    refused('mask_max must hold one element (got 0)', _device.device_scalar, torch.zeros(0, dtype=F64), 'mask_max', CPU)
    refused('mask_max must be float64 (got int64)', _device.device_scalar, torch.tensor(3), 'mask_max', CPU)
    refused('mask_max must be float64 (got float16)', _device.device_scalar, torch.tensor(3.0, dtype=torch.float16), 'mask_max', CPU)


# ---- 2. the in-bounds rule -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', tv.GPU_SHAPES, ids=str)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_every_recipe_stays_inside_its_parent(shape, dtype):
    """Restated here, independently of tensor_views.in_bounds: a reader that ignores strides and dtype and takes numel elements of
    8 bytes from the data pointer ends inside the parent's storage, and so does the view's own extent."""
    x = np.broadcast_to(np.arange(int(np.prod(shape[1:])), dtype=dtype).reshape(shape[1:]) % 7 + 1, shape) if len(shape) > 1 else \
        np.arange(int(np.prod(shape)), dtype=dtype).reshape(shape) % 7 + 1
    names = set()
    for r in tv.variants(x):
        t = r.build(CPU)
        first = t.storage_offset() * t.element_size()
        end = t.untyped_storage().nbytes()
        assert first + 8 * t.numel() <= end, r
        assert first + (1 + sum((d - 1) * s for d, s in zip(t.shape, t.stride()))) * t.element_size() <= end, r
        assert np.array_equal(t.double().numpy(), x.astype(np.float64)), r
        names.add(r.name)
    assert {'offset1', 'offset3', 'float16', 'int32'} <= names and (x.size < 2 or 'plane_of_pair' in names)
    assert (len(shape) < 2 or shape[0] < 2) or 'broadcast' in names
    for kind, make in tv.written_variants(shape, torch.float64 if dtype == np.float64 else torch.float32).items():
        t = make(CPU)
        assert t.storage_offset() == 0 and 8 * t.numel() <= t.untyped_storage().nbytes() and tuple(t.shape) == tuple(shape), kind


# ---- 3. refused before the library is touched ------------------------------------------------------------------------------------------

class Forbidden:
    """stands where the native library would: any use of it fails the test"""

    def __getattr__(self, name):
        pytest.fail(f'the native library was asked for {name}: the call was not refused on the host')


LIB = {0: Forbidden}            # what a projector of this module gets for its library


def no_load():
    pytest.fail('_native.load() was called: the call was not refused on the host')


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, 'load', no_load)
    monkeypatch.setattr(_device, 'GPU', FAKE)


MADE = []                    # every tensor T() made, in order (the identity test looks at those a call's builder made)


def T(shape, dtype=F32, device=FAKE):
    MADE.append(torch.empty(shape, dtype=dtype, device=device))
    return MADE[-1]


def host(shape, dtype=F32):
    return T(shape, dtype, CPU)


def outs(shape, dtype):
    """the four written tensors a call must refuse, by name"""
    n = int(np.prod(shape))
    wrong = F32 if dtype == F64 else F64
    return {'wrong-dtype': T(shape, wrong), 'short': T((n - 1,), dtype), 'long': T((n + 1,), dtype),
            'non-dense': T((2 * n,), dtype)[::2].view(shape) if len(shape) == 1 else T(tuple(shape[:-1]) + (2 * shape[-1],), dtype)[..., ::2],
            'host': host(shape, dtype)}


I0, MUS = np.ones((2, 48)), np.ones((2, 48))


def gn_device(**kw):
    a = dict(g1=T((4, 16, 8)), g2=T((4, 16, 8)), mask_max=T((), F64), out=T((4, 8, 16, 2), F64), dedup_workspace=T((1 << 20,), U8))
    a.update(kw)
    return md.gn_device(a.pop('g1'), a.pop('g2'), I0, MUS, 5, stop_tol=0.0, two_level=False, out_rc=(8, 16), dedup=True, **a)


def gn_device_multi(**kw):
    a = dict(g=T((3, 5, 7), F64), mask_max=T((), F64), out=T((5, 7, 2), F64))
    a.update(kw)
    return md.gn_device_multi(a.pop('g'), np.ones((3, 48)), MUS, 5, **a)


def gn_covariance_device(**kw):
    a = dict(a=T((5, 7, 2), F64), mask_g=T((5, 7)), mask_max=T((), F64), out=T((5, 7, 3), F64))
    a.update(kw)
    return md.gn_covariance_device(a.pop('a'), I0, I0, MUS, **a)


def scanner(**kw):
    return dx.FanBeamGeometry(**dict(dict(N_channels=16, N_proj=12), **kw))


def recon_device(sino=None, ct=None, **kw):
    return bp.recon_device(host((12, 16)) if sino is None else sino, ct or scanner(), 16, 20.0, 1.0, **kw)


def recon_covariance_device(cov):
    return bp.recon_covariance_device(cov, scanner(), 16, 20.0, 1.0)


def image_projector():
    return it.ImageProjector(scanner(), 16, 20.0)


def forward(**kw):
    a = dict(img_d=T((1, 16, 16)), out=T((12, 1, 16)))
    a.update(kw)
    return image_projector().forward(**a)


def adjoint(**kw):
    a = dict(sino_d=T((12, 1, 16)), out=T((1, 16, 16)))
    a.update(kw)
    return image_projector().adjoint(**a)


def sirt(**kw):
    a = dict(sino_d=T((12, 1, 16)), x0=T((1, 16, 16)))
    a.update(kw)
    return it.sirt(a.pop('sino_d'), image_projector(), 3, **a)


def pwls(**kw):
    a = dict(sinos_d=T((2, 12, 1, 16)), weights_d=T((3, 12, 1, 16)), x0=T((2, 1, 16, 16)))
    a.update(kw)
    return it.pwls(a.pop('sinos_d'), a.pop('weights_d'), image_projector(), 3, **a)


def precision_weights(cov_d):
    return it.precision_weights(cov_d)


def linearize_device(**kw):
    a = dict(sino_d=T((12, 16)), out=T((12, 16)))
    a.update(kw)
    return bhc.linearize_device(a.pop('sino_d'), object(), **a)


S, NV, NR, NC, NE, NMAT = 2, 6, 4, 5, 9, 3


def projector(native_layout=0):
    """a Projector without its device state: what project_tables, sino_log and transpose_log look at before the first launch"""
    pj = fp.Projector.__new__(fp.Projector)
    pj.lib, pj.dev, pj.n_mat, pj.view_begin, pj.view_end, pj.native_layout = LIB[0](), FAKE, NMAT, 0, NV, native_layout
    pj.plan, pj.geom, pj.use_packed, pj._groups, pj.cone, pj.kernel = torch.empty(8, dtype=U8, device=FAKE), _native.FanGeom(), False, False, False, 1
    pj.vol_yx = pj.vol_xy = pj.vol_zf = None
    pj.ct = types.SimpleNamespace(N_rows=NR, N_channels=NC)
    pj.phantom = types.SimpleNamespace(n_materials=NMAT)
    pj.mat_rows = list(range(NMAT))
    return pj


def project_tables(layout=0, native=0, **kw):
    a = dict(mu_d=T((NMAT, NE)), w_d=T((S, NE)), air=[1.0, 1.0])
    a.update(kw)
    return projector(native).project_tables(a.pop('mu_d'), a.pop('w_d'), layout=layout, **a)


def sino_log(**kw):
    a = dict(counts=T((S, NV, NR, NC)), out=T((S, NV, NR, NC)))
    a.update(kw)
    return projector().sino_log(a.pop('counts'), [1.0, 1.0], **a)


def transpose_log(**kw):
    a = dict(src=T((S, NV, NR, NC)), dst=T((S, NV, NC, NR)), log_dst=T((S, NV, NC, NR)))
    a.update(kw)
    return projector().transpose_log(a['src'], a['dst'], a['log_dst'], [1.0, 1.0], NR, NC)


def _written(fn, arg, shape, dtype, **fixed):
    return [(fn, dict(fixed, **{arg: t}), arg, f'{arg}-{kind}') for kind, t in outs(shape, dtype).items()]


def _hosts(fn, shapes, **fixed):
    return [(fn, dict(fixed, **{arg: host(*sd) if isinstance(sd[0], tuple) else host(sd)}), arg, f'{arg}-host') for arg, sd in shapes.items()]


TWO = T((2,), F64)
ROWS = (
    _hosts(gn_device, dict(g1=(4, 16, 8), g2=(4, 16, 8), mask_max=((), F64)))
    + _written(gn_device, 'out', (4, 8, 16, 2), F64)
    + [(gn_device, dict(mask_max=TWO), 'mask_max', 'mask_max-two'), (gn_device, dict(mask_max=T((), torch.int64)), 'mask_max', 'mask_max-int'),
       (gn_device, dict(dedup_workspace=host((1 << 20,), U8)), 'dedup_workspace', 'dedup_workspace-host'),
       (gn_device, dict(dedup_workspace=T((1 << 18,), F32)), 'dedup_workspace', 'dedup_workspace-wrong-dtype'),
       (gn_device, dict(dedup_workspace=T((1 << 21,), U8)[::2]), 'dedup_workspace', 'dedup_workspace-non-dense'),
       (gn_device, dict(g2=T((4, 16, 8), F64)), 'agree', 'g2-other-dtype'), (gn_device, dict(g2=np.ones((4, 16, 8))), 'g2', 'g2-numpy')]
    + _hosts(gn_device_multi, dict(g=((3, 5, 7), F64), mask_max=((), F64)))
    + _written(gn_device_multi, 'out', (5, 7, 2), F64)
    + [(gn_device_multi, dict(mask_max=TWO), 'mask_max', 'mask_max-two')]
    + _hosts(gn_covariance_device, dict(a=((5, 7, 2), F64), mask_g=(5, 7), mask_max=((), F64)))
    + _written(gn_covariance_device, 'out', (5, 7, 3), F64)
    + [(gn_covariance_device, dict(mask_max=TWO), 'mask_max', 'mask_max-two')]
    + [(recon_device, dict(), 'sino_d', 'sino_d-host-fbp'), (recon_device, dict(method='sirt'), 'sino_d', 'sino_d-host-sirt'),
       (recon_device, dict(method='os-sart'), 'sino_d', 'sino_d-host-os-sart'), (recon_device, dict(bhc=object()), 'sino_d', 'sino_d-host-bhc'),
       (recon_device, dict(sino=host((12, 4, 16)), ct=scanner(N_rows=4, cone=True)), 'sino_d', 'sino_d-host-cone'),
       (recon_device, dict(sino=np.ones((12, 16), np.float32)), 'sino_d', 'sino_d-numpy'),
       (recon_covariance_device, dict(cov=host((12, 16, 3), F64)), 'cov_d', 'cov_d-host'),
       (recon_covariance_device, dict(cov=T((12, 16, 3), F32)), 'cov_d', 'cov_d-float32'),
       (precision_weights, dict(cov_d=host((12, 16, 3), F64)), 'cov_d', 'cov_d-host'),
       (precision_weights, dict(cov_d=T((12, 16, 3), F32)), 'cov_d', 'cov_d-float32')]
    + _hosts(forward, dict(img_d=(1, 16, 16))) + _written(forward, 'out', (12, 1, 16), F32)
    + [(forward, dict(img_d=T((1, 16, 16), F64)), 'image', 'img_d-float64'), (forward, dict(img_d=T((1, 16, 32))[..., ::2]), 'image', 'img_d-non-dense')]
    + _hosts(adjoint, dict(sino_d=(12, 1, 16))) + _written(adjoint, 'out', (1, 16, 16), F32)
    + _hosts(sirt, dict(sino_d=(12, 1, 16), x0=(1, 16, 16))) + [(sirt, dict(x0=T((1, 16, 15))), 'x0', 'x0-short')]
    + _hosts(pwls, dict(sinos_d=(2, 12, 1, 16), weights_d=(3, 12, 1, 16), x0=(2, 1, 16, 16)))
    + [(pwls, dict(weights_d=T((3, 12, 1, 16), F64)), 'weights', 'weights_d-float64')]
    + _hosts(linearize_device, dict(sino_d=(12, 16))) + _written(linearize_device, 'out', (12, 16), F32)
    + [(linearize_device, dict(sino_d=T((12, 32))[:, ::2]), 'contiguous float32 device tensor', 'sino_d-non-dense')]
    + _hosts(project_tables, dict(mu_d=(NMAT, NE), w_d=(S, NE), w2_d=(S, NE)))
    + [row for lay, nat in ((0, 0), (1, 0), (0, 1), (1, 1)) for arg in ('out', 'log_out')
       for row in _written(project_tables, arg, (S, NV, NR, NC) if lay == 0 else (S, NV, NC, NR), F32, layout=lay, native=nat)]
    + _hosts(sino_log, dict(counts=(S, NV, NR, NC))) + _written(sino_log, 'out', (S, NV, NR, NC), F32)
    + _hosts(transpose_log, dict(src=(S, NV, NR, NC))) + _written(transpose_log, 'dst', (S, NV, NC, NR), F32)
    + _written(transpose_log, 'log_dst', (S, NV, NC, NR), F32)
    + [(transpose_log, dict(src=T((S, NV, NC, NR))), 'src', 'src-other-shape')]
)
NAMES = {'img_d': 'image', 'sino_d': {adjoint: 'sinogram', sirt: 'sinogram', linearize_device: 'contiguous float32 device tensor'},
         'sinos_d': 'sinograms', 'weights_d': 'weights'}


def _named(fn, arg):
    n = NAMES.get(arg, arg)
    n = n.get(fn, arg) if isinstance(n, dict) else n
    return 'out' if (fn is linearize_device and arg == 'out') else n


@pytest.mark.parametrize('fn,kw,arg,case', [pytest.param(*r, id=f'{r[0].__name__}-{r[3]}') for r in ROWS])
def test_refused_on_the_host(no_device, fn, kw, arg, case):
    with pytest.raises(ValueError) as info:
        fn(**kw)
    name = _named(fn, arg)                                               # the message names the argument
    text = str(info.value)                                               # (short names: at the head of the message, not anywhere in it)
    assert text.startswith((f'{name} must', f'{name}: ')) if len(name) < 3 else name in text, text


# ---- 4. conforming tensors are handed on as they are ----------------------------------------------------------------------------------

class Reached(Exception):
    """the call passed its host checks and asked for the library"""


class Ends:
    def __getattr__(self, name):
        raise Reached(name)


class CallEnds:
    """a library whose every function can be looked up and ends the call when it is CALLED (its arguments have been built by then)"""

    def __getattr__(self, name):
        def function(*args):
            raise Reached(name)
        return function


IDENTITY = [gn_device, gn_device_multi, gn_covariance_device, project_tables, sino_log, transpose_log, recon_device,
            recon_covariance_device, precision_weights, forward, adjoint, sirt, pwls, linearize_device]


@pytest.mark.parametrize('fn', IDENTITY, ids=lambda f: f.__name__)
def test_conforming_tensors_are_passed_on_by_identity(monkeypatch, fn):
    """Every tensor a conforming call is given goes through the module's check and comes out as the same object, up to the point
    where the call asks for the library (which ends the call here).  Recorded where each module decides: the helpers of
    _device.py, ImageProjector._tensor for the strict calls, and - linearize_device keeps no helper between its check and the
    library - the very objects whose pointers it hands to dexct_bhc_linearize."""
    def ends():
        raise Reached('load')
    monkeypatch.setattr(_native, 'load', ends)
    monkeypatch.setattr(_device, 'GPU', FAKE)
    monkeypatch.setitem(LIB, 0, Ends)
    seen = []

    def recording(helper):
        def wrapped(t, *a, **kw):
            got = helper(t, *a, **kw)
            seen.append((t, got))
            return got
        return wrapped
    for mod in (md, bp, it, fp):
        for name in ('dense_input', 'device_scalar', 'written'):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, recording(getattr(_device, name)))
    real_tensor = it.ImageProjector._tensor
    monkeypatch.setattr(it.ImageProjector, '_tensor', lambda self, t, *a: seen.append((t, real_tensor(self, t, *a))) or t)
    kw = {}
    if fn is recon_device:
        kw = dict(sino=T((12, 16)))
    elif fn is recon_covariance_device:
        kw = dict(cov=T((12, 16, 3), F64))
    elif fn is precision_weights:
        kw = dict(cov_d=T((12, 16, 3), F64))
    elif fn is linearize_device:
        monkeypatch.setattr(_native, 'load', CallEnds)
        monkeypatch.setattr(bhc, 'ptr', lambda t: seen.append((t, t)) or 0)
        monkeypatch.setattr(bhc, 'stream_ptr', lambda: 0)
        table = types.SimpleNamespace(device=lambda dev: torch.zeros(4), log2_min=-20, cells_log2=3, oct_pos=26, oct_neg=20)
        monkeypatch.setattr(bhc, 'linearize_device', (lambda real: lambda s, _, **k: real(s, table, **k))(bhc.linearize_device))
    before = len(MADE)
    with pytest.raises(Reached):
        fn(**kw)
    given = list(kw.values()) + [t for t in MADE[before:] if t.device.type == 'meta']
    assert given and all(got is t for t, got in seen)
    assert all(any(t is a for a, _ in seen) for t in given), fn.__name__      # every tensor of the call went through a check
