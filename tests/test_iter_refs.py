"""CPU pins of the references of the iterative reconstruction (tests/iter_refs.py) and of what the feature promises without
a GPU: the exported entry points and the argument errors of get_recon(..., method=) and ImageProjector."""
import ctypes
import re
import os

import numpy as np
import pytest

import iter_refs as ir
from conftest import ROOT


@pytest.fixture(scope='module', params=['c53', 'one'])
def matrices(request):
    scan = ir.small(request.param)
    return scan, ir.system_matrix(scan)


def test_small_scans_take_every_branch():
    for name in ('c53', 'c65'):
        scan = ir.small(name)
        _, plan = ir.plan_of(scan)
        hit = plan['n_slabs'] > 0
        assert set(plan['flags'][hit] & 1) == {0, 1} and set(plan['flags'][hit] & 2) == {0, 2}
        assert (~hit).any()                                                        # rays that miss the grid
        nu = np.where(plan['flags'] & 1, scan.ny, scan.nx)
        assert (hit & (plan['n_slabs'] < nu)).any()                                # rays through a side face
        assert scan.dx != scan.dy and scan.nx != scan.ny and scan.z_first == 1 and scan.n_rows < scan.nz
    _, plan = ir.plan_of(ir.small('one'))
    assert (plan['n_slabs'] == 1).any() and (plan['n_slabs'] == 0).any()


def test_dda_matrix_agrees_with_classic_matrix(matrices):
    """Entry by entry to 3e-7 cm, row sums against the plan's chord to 2e-5 cm: the tolerances tests/test_siddon_oracle.py
    applies to the two formulations; rays along a grid plane (the one genuine tie) are left out and are few."""
    scan, A = matrices
    Ac = ir.classic_matrix(scan)
    tie = ir.on_plane_rays(scan)
    assert tie.mean() <= 0.02
    assert np.max(np.abs(A - Ac)[~tie]) < 3e-7
    assert np.max(np.abs(A.sum(1) - Ac.sum(1))[~tie]) < 2e-5
    assert np.count_nonzero(A) > 0 and np.all(A >= 0)
    # every coefficient is a float32 number
    assert np.array_equal(A, A.astype(np.float32).astype(np.float64))


def test_sirt_ref_residual_never_increases(matrices):
    scan, A = matrices
    rng = np.random.default_rng(3)
    b = rng.uniform(0.0, 2.0, (scan.n_views, scan.n_rows, scan.n_ch))
    hist = []
    ir.sirt_ref(A, b, 10, 1, 1.0, False, None, history=hist)
    assert len(hist) == 10 and hist[0] > 0
    assert all(b_ <= a_ * (1 + 1e-12) for a_, b_ in zip(hist[:-1], hist[1:])), hist


@pytest.mark.parametrize('n_subsets', [1, 3])
def test_sirt_ref_fixed_point(matrices, n_subsets):
    scan, A = matrices
    n_subsets = min(n_subsets, scan.n_views)
    rng = np.random.default_rng(4)
    x_true = rng.uniform(0.0, 1.0, A.shape[1])
    b = (A @ x_true).reshape(scan.n_views, scan.n_rows, scan.n_ch)
    x = ir.sirt_ref(A, b, 2, n_subsets, 1.0, True, x_true)
    assert np.max(np.abs(x - x_true)) <= 1e-13


def test_library_exports_the_pair():
    from dex_ct_sim_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    for name in ('dexct_image_project', 'dexct_image_backproject', 'dexct_sirt_residual', 'dexct_sirt_update'):
        assert hasattr(lib, name) and name in _native.SYMBOLS and re.search(name + r'\s*\(', hdr), name
    lib.dexct_abi_version.restype = ctypes.c_int
    assert lib.dexct_abi_version() == 6 == _native.ABI_VERSION


def test_pair_rejects_bad_arguments_without_a_launch():
    import ctypes as C
    from dex_ct_sim_amd import _native
    lib = _native.load()
    one = C.c_void_p(8)
    g = _native.FanGeom(10, 16, 2, 1, 8, 8, 3, 0, 0.1, 0.1, 0.1, 60.0, 100.0)
    EINVAL, ERANGE = -1, -2
    fwd = lambda geom=g, plan=one, vb=0, ve=10, step=1, img=one, sino=one: \
        lib.dexct_image_project(C.byref(geom) if geom else None, plan, vb, ve, step, img, None, sino, None)
    bwd = lambda geom=g, plan=one, vb=0, ve=10, step=1, img=one, sino=one: \
        lib.dexct_image_backproject(C.byref(geom) if geom else None, plan, vb, ve, step, sino, img, None, 0, None)
    for f in (fwd, bwd):
        assert f(geom=None) == EINVAL and f(plan=None) == EINVAL and f(img=None) == EINVAL and f(sino=None) == EINVAL
        assert f(step=0) == EINVAL and f(vb=5, ve=5) == EINVAL and f(ve=11) == EINVAL and f(vb=-1) == EINVAL
        assert f(geom=_native.FanGeom(10, 0, 2, 1, 8, 8, 3, 0, 0.1, 0.1, 0.1, 60.0, 100.0)) == EINVAL
        assert f(geom=_native.FanGeom(10, 16, 3, 1, 8, 8, 3, 0, 0.1, 0.1, 0.1, 60.0, 100.0)) == EINVAL       # slices past nz
        assert f(geom=_native.FanGeom(10, 16, 2, 1, 9000, 8, 3, 0, 0.1, 0.1, 0.1, 60.0, 100.0)) == ERANGE
        assert f(geom=_native.FanGeom(70000, 16, 2, 1, 8, 8, 3, 0, 0.1, 0.1, 0.1, 60.0, 100.0), ve=70000) == ERANGE
    assert lib.dexct_sirt_residual(one, one, one, 4, 0, 16, one, None, None) == EINVAL
    assert lib.dexct_sirt_residual(one, one, one, 4, 1, 16, None, None, None) == EINVAL
    assert lib.dexct_sirt_update(one, one, one, 0, 1.0, 1, None) == EINVAL
    assert lib.dexct_sirt_update(one, one, one, 16, 0.0, 1, None) == EINVAL


def test_value_errors_come_before_any_device_access():
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd.back_project import get_recon
    from dex_ct_sim_amd.iterative import ImageProjector
    ct = dx.FanBeamGeometry(N_channels=32, N_proj=12)
    cone = dx.FanBeamGeometry(N_channels=32, N_proj=12, N_rows=4, cone=True)
    sino = np.zeros((12, 32), np.float32)
    spec = None                                             # never reached
    for kw in (dict(method='art'), dict(method='sirt', relax=2.0), dict(method='sirt', relax=0.0), dict(method='sirt', n_subsets=0),
               dict(method='sirt', n_subsets=13), dict(method='sirt', n_iters=0), dict(method='os-sart', init='ones')):
        with pytest.raises(ValueError):
            get_recon(sino, ct, spec, 16, 20.0, 1.0, **kw)
    with pytest.raises(ValueError):
        get_recon(np.zeros((12, 4, 32), np.float32), cone, spec, 16, 20.0, 1.0, method='sirt')
    with pytest.raises(ValueError):
        get_recon(sino, ct, spec, 16, ct.SID * np.sqrt(2.0), 1.0, method='sirt')      # the grid's corner on the source circle
    with pytest.raises(ValueError):
        ImageProjector(cone, 16, 20.0)
    with pytest.raises(ValueError):
        ImageProjector(ct, 16, ct.SID * np.sqrt(2.0))
    p = ImageProjector(ct, 16, 20.0, n_slices=3)            # no device needed to describe the pair
    assert p.image_shape == (3, 16, 16) and p.sino_shape == (12, 3, 32)
