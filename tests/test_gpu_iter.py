"""The matched projector pair (csrc/iterative.hip) and SIRT / OS-SART on it, on the GPU, against tests/iter_refs.py.

Bounds (u = 2^-24): a float32 sum of n products whose factors carry a rounding each is within (n + 4) u sum |a| |x| of the
exact sum - n - 1 additions, the product and the coefficient's own rounding, one more addition where a transposed accumulator
is merged and one where the call accumulates; 1.01 covers the second-order terms.  The same per ray (forward, n_i non-zeros
of the row) and per pixel (adjoint, n_j non-zeros of the column over the views of the call).

Measured on an MI355X, worst error / bound: forward 0.21, adjoint 0.24, adjoint identity 2e-4; test_sirt_matches_reference
0.92 - 2.68 of d32 against the 8 allowed (per case in DESIGN.md section 4.6).  The module takes about 3 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iter_refs as ir
from guarded import Arena, twice
from iter_refs import F32, F64, U

pytestmark = pytest.mark.gpu

SCANS = ['c53', 'c65', 'one']


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = ir.system_matrix(ir.small(name))
    A.setflags(write=False)
    return A


def projector(name, transposed=True):
    from dex_ct_sim_amd.iterative import ImageProjector
    s = ir.small(name)
    return ImageProjector.from_grid(s.nx, s.ny, s.nz, s.dx, s.dy, s.n_views, s.n_ch, s.n_rows, s.z_first, s.sid, s.sdd, s.view_cs,
                                    s.chan_cs, transposed=transposed)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def view_rows(scan, begin, step):
    """mask over the rows of A of the views begin + k step"""
    v = np.arange(scan.n_views)
    on = (v >= begin) & ((v - begin) % step == 0)
    return np.repeat(on, scan.n_rows * scan.n_ch)


def check(got, ref, bound, what):
    got = np.asarray(got, F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf))
    print(f'{what}: worst error / bound {ratio.max():.3f}')
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound), (what, float(ratio.max()))


# ---- 1: forward ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('transposed', [True, False])
@pytest.mark.parametrize('begin,step', [(0, 1), (0, 3), (1, 3)])
def test_forward_against_system_matrix(hip, name, transposed, begin, step):
    scan, A = ir.small(name), matrix(name)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, (scan.nz, scan.ny, scan.nx)).astype(F32)
    ref, bound = ir.forward_bound(A, x.reshape(-1).astype(F64))
    p = projector(name, transposed)
    out = torch.full(p.sino_shape, 7.5, dtype=torch.float32, device='cuda')
    got = p.forward(dev(x), views=(begin, scan.n_views, step), out=out).cpu().numpy().reshape(-1)
    on = view_rows(scan, begin, step)
    check(got[on], ref[on], bound[on], f'forward {name} t={transposed} {begin}:{step}')
    assert np.all(got[~on] == F32(7.5))                              # the lines of the other views keep their sentinel
    assert np.any(ref[on] != 0) and np.any(bound[on] == 0)           # rays that hit and rays that miss


# ---- 2: adjoint ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('transposed', [True, False])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('begin,step', [(0, 1), (1, 3)])
def test_adjoint_against_transpose(hip, name, transposed, accumulate, begin, step):
    scan, A = ir.small(name), matrix(name)
    rng = np.random.default_rng(12)
    y = rng.uniform(-1.0, 1.0, (scan.n_views, scan.n_rows, scan.n_ch)).astype(F32)
    z0 = rng.uniform(-2.0, 2.0, (scan.nz, scan.ny, scan.nx)).astype(F32)
    on = view_rows(scan, begin, step)
    As = A[on]
    yy = y.reshape(-1).astype(F64)[on]
    start = z0.reshape(-1).astype(F64) if accumulate else 0.0
    ref = start + As.T @ yy
    bound = (np.count_nonzero(As, axis=0) + 4.0) * U * (np.abs(start) + np.abs(As).T @ np.abs(yy)) * 1.01
    p = projector(name, transposed)
    out = dev(z0)
    got = p.adjoint(dev(y), views=(begin, scan.n_views, step), out=out, accumulate=accumulate).cpu().numpy().reshape(-1)
    check(got, ref, bound, f'adjoint {name} t={transposed} acc={accumulate} {begin}:{step}')
    untouched = np.count_nonzero(As, axis=0) == 0                    # slices no row images, pixels no ray crosses
    assert untouched.any() or name == 'one'
    assert np.array_equal(got[untouched], z0.reshape(-1)[untouched] if accumulate else np.zeros(untouched.sum(), F32))


# ---- 3: adjoint identity -------------------------------------------------------------------------------------------------------

def test_adjoint_identity(hip):
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd.iterative import ImageProjector
    n, fov, n_views, n_ch = 64, 25.0, 90, 96
    ct = dx.FanBeamGeometry(N_channels=n_ch, N_proj=n_views)
    rng = np.random.default_rng(13)
    x = rng.uniform(0.0, 1.0, (1, n, n)).astype(F32)
    y = rng.uniform(0.0, 1.0, (n_views, 1, n_ch)).astype(F32)
    pix = fov / n
    per_view = int(np.ceil(pix * np.sqrt(2.0) / ((ct.SID - 0.5 * fov * np.sqrt(2.0)) * ct.dgamma))) + 1
    n_max = max(2 * n, n_views * per_view)
    for transposed in (True, False):
        p = ImageProjector(ct, n, fov, transposed=transposed)
        ax = p.forward(dev(x)).cpu().numpy().astype(F64)
        aty = p.adjoint(dev(y)).cpu().numpy().astype(F64)
        lhs, rhs = float(np.sum(ax * y.astype(F64))), float(np.sum(x.astype(F64) * aty))
        print(f'adjoint identity t={transposed}: <Ax,y> = {lhs!r}, <x,ATy> = {rhs!r}, |diff| / bound = '
              f'{abs(lhs - rhs) / (2 * (n_max + 4) * U * lhs):.4f}')
        assert lhs > 0 and abs(lhs - rhs) <= 2 * (n_max + 4) * U * lhs


# ---- 4: determinism of the forward ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['c65'])
def test_forward_is_deterministic(hip, name):
    scan = ir.small(name)
    x = dev(np.random.default_rng(14).uniform(-1.0, 1.0, (scan.nz, scan.ny, scan.nx)))
    p = projector(name)
    a, b = p.forward(x).cpu().numpy(), p.forward(x).cpu().numpy()
    assert np.array_equal(a, b) and np.any(a != 0)


# ---- 5: SIRT / OS-SART against the reference -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sirt_problem(name):
    scan, A = ir.small(name), matrix(name)
    rng = np.random.default_rng(15)
    x_true = rng.uniform(0.0, 1.0, A.shape[1])
    b = (A @ x_true) * rng.uniform(0.7, 1.3, A.shape[0]) - 0.05          # inconsistent data, some of it negative
    x0 = rng.uniform(0.0, 1.0, (scan.nz, scan.ny, scan.nx)).astype(F32)
    return b.reshape(scan.n_views, scan.n_rows, scan.n_ch).astype(F32), x0


@functools.lru_cache(maxsize=None)
def sirt_refs(name, n_subsets, nonneg, given):
    b, x0 = sirt_problem(name)
    args = (matrix(name), b, 5, n_subsets, 1.0, nonneg, x0 if given else None)
    return ir.sirt_ref(*args, dtype=F64), ir.sirt_ref(*args, dtype=F32)


@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('n_subsets', [1, 3])
@pytest.mark.parametrize('nonneg', [True, False])
@pytest.mark.parametrize('given', [False, True])
def test_sirt_matches_reference(hip, name, n_subsets, nonneg, given):
    """5 iterations; d32 = max |float32 reference - float64 reference| measures how far float32 rounding carries through the
    iterations of THIS problem; the device result lies within 8 d32 of the float64 reference (the margin covers the other
    summation order of the atomics)."""
    from dex_ct_sim_amd.iterative import sirt
    b, x0 = sirt_problem(name)
    ref64, ref32 = sirt_refs(name, n_subsets, nonneg, given)
    d32 = float(np.max(np.abs(ref32.astype(F64) - ref64)))
    p = projector(name)
    x0_d = dev(x0) if given else None
    got = sirt(dev(b), p, 5, n_subsets, 1.0, x0=x0_d, nonneg=nonneg).cpu().numpy().reshape(-1).astype(F64)
    err = float(np.max(np.abs(got - ref64)))
    print(f'sirt {name} S={n_subsets} nonneg={nonneg} x0={given}: err {err:.3e}, d32 {d32:.3e}, ratio {err / d32 if d32 else np.inf:.3f}')
    assert np.all(np.isfinite(got)) and err <= 8.0 * d32
    if given:
        assert np.array_equal(x0_d.cpu().numpy(), x0)                 # the start image is the caller's
    if nonneg:
        assert got.min() >= 0.0


# ---- 6: fixed point ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['c65', 'one'])
@pytest.mark.parametrize('n_subsets', [1, 3])
def test_fixed_point_is_bit_identical(hip, name, n_subsets):
    from dex_ct_sim_amd.iterative import sirt
    scan = ir.small(name)
    x_true = dev(np.random.default_rng(16).uniform(0.0, 1.0, (scan.nz, scan.ny, scan.nx)))
    p = projector(name)
    b = p.forward(x_true)
    hist = []
    x = sirt(b, p, 1, n_subsets, 1.0, x0=x_true, nonneg=True, history=hist)
    assert np.array_equal(x.cpu().numpy(), x_true.cpu().numpy()) and hist == [0.0]


# ---- 7: the public path --------------------------------------------------------------------------------------------------------

def two_discs(n):
    yy, xx = np.mgrid[0:n, 0:n] - 0.5 * (n - 1)
    img = np.zeros((n, n), F32)
    img[(xx + 0.15 * n) ** 2 + yy ** 2 < (0.22 * n) ** 2] = 0.2
    img[(xx - 0.2 * n) ** 2 + (yy - 0.1 * n) ** 2 < (0.1 * n) ** 2] = 0.45
    return img


def non_increasing(h, slack):
    return all(b <= a * (1 + slack) for a, b in zip(h[:-1], h[1:]))


def test_public_path(hip):
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import synthetic
    from dex_ct_sim_amd.back_project import get_recon, recon_device, water_mu
    from dex_ct_sim_amd.iterative import ImageProjector
    n, fov = 32, 20.0
    ct = dx.FanBeamGeometry(N_channels=64, N_proj=48)
    spec = synthetic.kramers_spectrum(80)
    x_true = two_discs(n)
    p = ImageProjector(ct, n, fov)
    b_d = p.forward(dev(x_true[None]))
    b = b_d.cpu().numpy()[:, 0, :]
    hist = []
    raw, hu = get_recon(b, ct, spec, n, fov, 1.0, method='sirt', n_iters=10, init='zero', nonneg=False, history=hist)
    print('sirt history', hist)
    assert raw.shape == hu.shape == (n, n) and raw.dtype == np.float32
    assert len(hist) == 10 and hist[-1] < hist[0] and non_increasing(hist, 1e-5)
    mu_w = water_mu(ct, spec)
    assert np.array_equal(hu, (1000.0 * (raw - mu_w) / mu_w).astype(F32))
    # 'fbp' is the call without the keyword
    f0, h0 = get_recon(b, ct, spec, n, fov, 1.0)
    f1, h1 = get_recon(b, ct, spec, n, fov, 1.0, method='fbp')
    assert np.array_equal(f0, f1) and np.array_equal(h0, h1)
    # init='fbp' starts from the FBP image: the first residual norm is the FBP image's
    R = p.row_sums().cpu().numpy().astype(F64)[:, 0, :]
    d = b.astype(F64) - p.forward(dev(f0[None])).cpu().numpy().astype(F64)[:, 0, :]
    norm_fbp = float(np.sqrt(np.sum(np.where(R > 0, d * d / np.where(R > 0, R, 1.0), 0.0))))
    hist_f = []
    get_recon(b, ct, spec, n, fov, 1.0, method='sirt', n_iters=2, nonneg=False, history=hist_f)
    assert abs(hist_f[0] - norm_fbp) <= 1e-5 * norm_fbp and hist_f[1] < hist_f[0]
    # a stacked fan, through the alias (10 subsets)
    ct3 = dx.FanBeamGeometry(N_channels=64, N_proj=48, N_rows=3)
    raw3, hu3 = get_recon(np.stack([b, 0.5 * b, b], 1), ct3, spec, n, fov, 1.0, method='os-sart', n_iters=2)
    assert raw3.shape == hu3.shape == (3, n, n) and np.all(raw3 >= 0)
    assert np.array_equal(raw3[0], raw3[2]) or np.allclose(raw3[0], raw3[2], rtol=0, atol=1e-5)
    # the device entry point takes the same keywords
    img = recon_device(b_d[:, 0, :].contiguous(), ct, n, fov, 1.0, method='sirt', n_iters=3, n_subsets=4, init='zero')
    assert tuple(img.shape) == (n, n)
    # a short scan: no Parker weights, the residual decreases
    cts = dx.FanBeamGeometry(N_channels=64, N_proj=48, theta_tot=np.pi + ct.gamma_fan + 0.2)
    bs = ImageProjector(cts, n, fov).forward(dev(x_true[None])).cpu().numpy()[:, 0, :]
    hist_s = []
    get_recon(bs, cts, spec, n, fov, 1.0, method='sirt', n_iters=6, init='zero', nonneg=False, history=hist_s)
    print('short-scan history', hist_s)
    assert hist_s[-1] < hist_s[0] and non_increasing(hist_s, 1e-5)


# ---- 8: guard bands, through the bare C ABI ------------------------------------------------------------------------------------

def arena_for(hip, scan, with_t):
    from dex_ct_sim_amd import _native
    g, plan = ir.plan_of(scan)
    n_img = 4 * scan.nz * scan.ny * scan.nx
    # (the library's last HIP error is per thread and is never cleared: an earlier test of the session that provoked a refusal
    # on purpose leaves it set.  Every call here is checked by its return code, and the tests compare the value with the one
    # they started from instead of with 0, which Arena.check would do.)
    ar = Arena('cuda', None)
    ar.hip_error_before = hip.dexct_last_hip_error()
    ar.alloc('plan', plan.nbytes).put(plan)
    ar.alloc('image', n_img)
    ar.alloc('sino', 4 * scan.n_views * scan.n_rows * scan.n_ch)
    if with_t:
        ar.alloc('image_t', n_img)
    return ar, scan.geom(lambda *a: _native.FanGeom(*a[:7], 0, *a[7:]))


@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('with_t', [False, True])
def test_guard_bands_project(hip, name, with_t):
    scan, A = ir.small(name), matrix(name)
    ar, geom = arena_for(hip, scan, with_t)
    x = np.random.default_rng(17).uniform(-1.0, 1.0, (scan.nz, scan.ny, scan.nx)).astype(F32)
    ref, bound = ir.forward_bound(A, x.reshape(-1).astype(F64))
    t_ptr = lambda: ar['image_t'].ptr if with_t else None

    def launch(step):
        ar['image'].put(x)
        if with_t:
            ar['image_t'].put(np.ascontiguousarray(x.transpose(0, 2, 1)))
        rc = hip.dexct_image_project(C.byref(geom), ar['plan'].ptr, 0, scan.n_views, step, ar['image'].ptr, t_ptr(), ar['sino'].ptr, sp())
        assert rc == 0, rc

    got = twice(ar, lambda: launch(1), ['sino'])['sino'].view(F32)
    check(got, ref, bound, f'guarded forward {name} t={with_t}')
    for byte in (0x00, 0xFF):                                         # ragged subsets: the skipped lines keep the fill
        ar.fill(byte, inner=('sino',))
        launch(3)
        ar.check()
        on = view_rows(scan, 0, 3)
        raw = ar['sino'].get()
        check(raw.view(F32)[on], ref[on], bound[on], f'guarded forward {name} step 3')
        assert np.all(raw.reshape(-1, 4)[~on] == byte)
    # argument errors come back without a launch
    from dex_ct_sim_amd import _native
    big = scan.geom(lambda *a: _native.FanGeom(*a[:4], 8193, *a[5:7], 0, *a[7:]))
    for byte in (0x00, 0xFF):
        ar.fill(byte, inner=('sino',))
        args = (ar['plan'].ptr, 0, scan.n_views)
        assert hip.dexct_image_project(C.byref(geom), *args, 0, ar['image'].ptr, t_ptr(), ar['sino'].ptr, sp()) == -1
        assert hip.dexct_image_project(C.byref(geom), *args, 1, None, t_ptr(), ar['sino'].ptr, sp()) == -1
        assert hip.dexct_image_project(C.byref(geom), *args, 1, ar['image'].ptr, t_ptr(), None, sp()) == -1
        assert hip.dexct_image_project(C.byref(geom), ar['plan'].ptr, 0, scan.n_views + 1, 1, ar['image'].ptr, t_ptr(), ar['sino'].ptr, sp()) == -1
        assert hip.dexct_image_project(C.byref(big), *args, 1, ar['image'].ptr, t_ptr(), ar['sino'].ptr, sp()) == -2
        ar.check()
        assert np.all(ar['sino'].get() == byte)
    assert hip.dexct_last_hip_error() == ar.hip_error_before


@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('with_t', [False, True])
def test_guard_bands_backproject(hip, name, with_t):
    scan, A = ir.small(name), matrix(name)
    ar, geom = arena_for(hip, scan, with_t)
    y = np.random.default_rng(18).uniform(-1.0, 1.0, (scan.n_views, scan.n_rows, scan.n_ch)).astype(F32)
    t_ptr = lambda: ar['image_t'].ptr if with_t else None
    for begin, step in ((0, 1), (0, 3)):
        on = view_rows(scan, begin, step)
        As, yy = A[on], y.reshape(-1).astype(F64)[on]
        ref = As.T @ yy
        bound = (np.count_nonzero(As, axis=0) + 4.0) * U * (np.abs(As).T @ np.abs(yy)) * 1.01

        def launch():
            ar['sino'].put(y)
            rc = hip.dexct_image_backproject(C.byref(geom), ar['plan'].ptr, begin, scan.n_views, step, ar['sino'].ptr, ar['image'].ptr,
                                             t_ptr(), 0, sp())
            assert rc == 0, rc

        for byte in (0x00, 0xFF):             # (float atomics in unspecified order: the two fills may differ in the last bits)
            got = twice(ar, launch, ['image'], scratch=['image_t'] if with_t else [], fills=(byte,))['image'].view(F32)
            check(got, ref, bound, f'guarded adjoint {name} t={with_t} {begin}:{step} fill {byte:#x}')
    from dex_ct_sim_amd import _native
    big = scan.geom(lambda *a: _native.FanGeom(*a[:5], 8193, a[6], 0, *a[7:]))
    for byte in (0x00, 0xFF):
        ar.fill(byte, inner=('image',) + (('image_t',) if with_t else ()))
        args = (ar['plan'].ptr, 0, scan.n_views)
        assert hip.dexct_image_backproject(C.byref(geom), *args, 0, ar['sino'].ptr, ar['image'].ptr, t_ptr(), 0, sp()) == -1
        assert hip.dexct_image_backproject(C.byref(geom), *args, 1, None, ar['image'].ptr, t_ptr(), 0, sp()) == -1
        assert hip.dexct_image_backproject(C.byref(geom), *args, 1, ar['sino'].ptr, None, t_ptr(), 0, sp()) == -1
        assert hip.dexct_image_backproject(C.byref(geom), None, 0, scan.n_views, 1, ar['sino'].ptr, ar['image'].ptr, t_ptr(), 0, sp()) == -1
        assert hip.dexct_image_backproject(C.byref(big), *args, 1, ar['sino'].ptr, ar['image'].ptr, t_ptr(), 0, sp()) == -2
        ar.check()
        assert np.all(ar['image'].get() == byte)
        if with_t:
            assert np.all(ar['image_t'].get() == byte)
    assert hip.dexct_last_hip_error() == ar.hip_error_before
