"""The status code of every call the seven projection entry points refuse, as a table: dexct_siddon_project, _grouped, _packed,
_grouped_packed, dexct_cone_project, _rows and _grouped.

The pointers are non-null dummies that a refused call never follows, so every case here MUST be a refused call - one that
passed its checks would go on to launch (and without a device would merely come back with DEXCT_EHIP, which pins nothing).
Each `return DEXCT_EINVAL / DEXCT_ERANGE` of an entry point or of a helper it calls before its first launch has a case that
trips it alone; the two-fault cases at the end of each block pin the ORDER of the checks (an EINVAL fault mixed with an ERANGE
fault: the code that comes back tells which check runs first).  The expected codes are literals recorded from the library as it
was before the entry points got their shared host layer (csrc/proj_host.h); nothing is computed from the code under test.

Not reachable without a device, hence not here: the grid limit of the detection pass (launch_detect_any runs after the group
traversals were launched) and the 160 KB bound of DEXCT_ALLOW_LDS (256 materials need 128 KB)."""
import ctypes as C

import pytest

from dex_ct_sim_amd import _native

EINVAL, ERANGE = -1, -2
P = C.c_void_p(16)          # a non-null dummy pointer

GEOM = dict(n_views=10, n_channels=8, n_rows=16, z_first=0, nx=8, ny=8, nz=16, pad_=0, dx=0.1, dy=0.1, dz=0.1, sid=60.0, sdd=100.0)
# a grid of more than 2^31 - 1 workgroups for every kernel that has a one-dimensional grid
HUGE = dict(n_views=65535, n_channels=200000, ve=65535)
SAMPLE = 'sample'           # stands for a dexct_noise that asks for the sample
LOG = 'log'                 # stands for a dexct_log_out with a sinogram pointer


def _common(kw):
    geom = dict(GEOM)
    geom.update({k: kw.pop(k) for k in list(kw) if k in GEOM})
    null = kw.pop('null', ())
    null = (null,) if isinstance(null, str) else null
    a = dict(vb=0, ve=10, nE=10, S=2, layout=1, kernel=2, dz_max=0.0, w2=None, var=None, noise=None, lo=None)
    a.update(kw)
    a['geom'] = None if 'geom' in null else C.byref(_native.FanGeom(*[geom[k] for k, _ in _native.FanGeom._fields_]))
    a['noise'] = _native.noise(3) if a['noise'] == SAMPLE else (_native.noise(3, sample=False) if a['noise'] == 'nosample' else None)
    a['lo'] = _native.log_out(16, [1.0, 1.0]) if a['lo'] == LOG else (_native.log_out(0, [1.0]) if a['lo'] == 'nolog' else None)
    a['w2'] = P if a['w2'] else None
    a['var'] = P if a['var'] else None
    a['p'] = lambda name: None if name in null else P
    return a


def siddon_project(lib, M=3, **kw):
    a = _common(kw)
    p = a['p']
    return lib.dexct_siddon_project(a['geom'], p('plan'), a['vb'], a['ve'], p('vol_yx'), p('vol_xy'), p('vol_zf'), M, a['nE'], a['S'],
                                    p('mu'), p('weights'), p('counts'), None, a['kernel'], a['layout'], a['w2'], a['var'], a['lo'], None)


def _grouped(fn, M, kw):
    a = _common(kw)
    p = a['p']
    return fn(a['geom'], p('plan'), a['vb'], a['ve'], p('codes'), M, a['nE'], a['S'], p('mu'), p('weights'), p('counts'), None,
              p('acc_scratch'), a['layout'], a['w2'], a['var'], a['lo'], a['noise'], None)


def siddon_grouped(lib, M=5, **kw):
    return _grouped(lib.dexct_siddon_project_grouped, M, kw)


def siddon_grouped_packed(lib, M=5, **kw):
    return _grouped(lib.dexct_siddon_project_grouped_packed, M, kw)


def siddon_packed(lib, M=3, **kw):
    a = _common(kw)
    p = a['p']
    return lib.dexct_siddon_project_packed(a['geom'], p('plan'), a['vb'], a['ve'], p('vol_z2'), M, a['nE'], a['S'], p('mu'), p('weights'),
                                           p('counts'), None, a['layout'], a['lo'], a['w2'], a['var'], a['noise'], None)


def cone_project(lib, M=3, **kw):
    a = _common(kw)
    p = a['p']
    return lib.dexct_cone_project(a['geom'], p('plan'), p('view_cs'), p('chan_cs'), p('row_z'), 0.0, a['dz_max'], a['vb'], a['ve'],
                                  p('vol_yx'), p('vol_xy'), M, a['nE'], a['S'], p('mu'), p('weights'), p('counts'), None, a['lo'],
                                  a['w2'], a['var'], a['noise'], None)


def cone_rows(lib, M=3, **kw):
    a = _common(kw)
    p = a['p']
    return lib.dexct_cone_project_rows(a['geom'], p('plan'), p('view_cs'), p('chan_cs'), p('row_z'), 0.0, a['dz_max'], a['vb'], a['ve'],
                                       p('vol_zc'), M, a['nE'], a['S'], p('mu'), p('weights'), p('counts'), None, a['lo'], a['w2'],
                                       a['var'], a['noise'], None)


def cone_grouped(lib, M=5, **kw):
    a = _common(kw)
    p = a['p']
    return lib.dexct_cone_project_grouped(a['geom'], p('plan'), p('view_cs'), p('chan_cs'), p('row_z'), 0.0, a['dz_max'], a['vb'],
                                          a['ve'], p('vol_zcg'), M, a['nE'], a['S'], p('mu'), p('weights'), p('counts'), None,
                                          p('acc_scratch'), a['lo'], a['w2'], a['var'], a['noise'], None)


# what every entry point checks in the same words: (arguments, code)
VIEWS = [(dict(vb=-1), EINVAL), (dict(ve=11), EINVAL), (dict(vb=5, ve=5), EINVAL)]
SIXTEEN_BIT = [(dict(n_rows=65536, nz=65536), ERANGE), (dict(n_views=65536, ve=65536), ERANGE)]
NOISE_EINVAL = [(dict(w2=1), EINVAL), (dict(var=1), EINVAL), (dict(noise=SAMPLE), EINVAL)]
SLOPE = [(dict(dz_max=1e4), ERANGE), (dict(dz_max=-1.0), ERANGE), (dict(dz_max=float('nan')), ERANGE)]
VOXELS = dict(nx=2048, ny=2048, nz=1024)                 # 2^32 voxels: past the 32-bit offsets
CONE_BYTES = dict(nx=2048, ny=2048, nz=1024)             # the guarded layout past 2^32 - 2 bytes
PACKED_BYTES = dict(nx=2047, ny=2047, nz=3856)           # 2047^2 x 964 packed bytes: past the offsets below kOob
# the noise limits of the detection pass of the material groups, and its log rule
GROUP_NOISE = NOISE_EINVAL + [
    (dict(w2=1, noise=SAMPLE, S=3), ERANGE), (dict(w2=1, noise=SAMPLE, M=49), ERANGE),
    (dict(w2=1, var=1, lo=LOG), EINVAL), (dict(w2=1, var=1, noise='nosample', lo=LOG), EINVAL)]

CASES = {
    siddon_project: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'mu', 'weights', 'counts')] + VIEWS + SIXTEEN_BIT + [
        (dict(M=0), EINVAL), (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(n_rows=0), EINVAL),
        (dict(M=257), ERANGE), (dict(S=5), ERANGE),
        (dict(z_first=-1), EINVAL), (dict(nz=24, n_rows=32), EINVAL), (dict(z_first=4), EINVAL),
        (VOXELS, ERANGE),
        (dict(kernel=1, null='vol_yx'), EINVAL), (dict(kernel=1, null='vol_xy'), EINVAL), (dict(kernel=0, null='vol_yx'), EINVAL),
        (dict(kernel=2, null='vol_zf'), EINVAL),
        (dict(kernel=3, null='vol_zf'), EINVAL), (dict(kernel=3, M=5), EINVAL), (dict(kernel=3, M=1), EINVAL),
        (dict(kernel=5, nz=18), EINVAL), (dict(kernel=5, z_first=2, n_rows=8), EINVAL),
        (dict(kernel=7), EINVAL), (dict(kernel=4), EINVAL), (dict(kernel=-1), EINVAL),
        (dict(kernel=6, null='vol_xy'), EINVAL), (dict(kernel=6, M=5), EINVAL), (dict(kernel=6, w2=1, var=1), EINVAL),
        (dict(layout=2), EINVAL), (dict(layout=-1), EINVAL),
        (dict(w2=1), EINVAL), (dict(var=1), EINVAL),
        (dict(w2=1, var=1, lo=LOG), EINVAL),
        # the launch functions: one-dimensional grids, the tables of the wave-per-ray kernel in LDS
        (dict(kernel=2, **HUGE), ERANGE), (dict(kernel=2, M=60, **HUGE), ERANGE), (dict(kernel=3, **HUGE), ERANGE),
        # (49+ materials run 64 rows per workgroup: 128 rows are one chunk of 128 lanes - 1.31e9 workgroups - but two of 64)
        (dict(kernel=2, M=60, n_rows=128, nz=128, n_views=65535, ve=65535, n_channels=20000), ERANGE),
        (dict(kernel=5, **dict(HUGE, n_channels=2000000)), ERANGE), (dict(kernel=0, n_rows=64, nz=64, **HUGE), ERANGE),
        (dict(kernel=6, nE=5000, S=3, M=1), ERANGE),
        # two faults
        (dict(ve=11, M=257), EINVAL), (dict(M=0, S=5), EINVAL), (dict(M=257, z_first=-1), ERANGE),
        (dict(z_first=-1, **VOXELS), EINVAL), (dict(kernel=7, **VOXELS), ERANGE), (dict(layout=2, n_rows=65536, nz=65536), EINVAL),
        (dict(w2=1, n_rows=65536, nz=65536), EINVAL), (dict(w2=1, var=1, lo=LOG, n_rows=65536, nz=65536), ERANGE),
        (dict(kernel=2, layout=2, **HUGE), EINVAL), (dict(kernel=2, w2=1, var=1, lo=LOG, **HUGE), EINVAL),
    ],
    siddon_grouped: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'codes', 'mu', 'weights', 'counts', 'acc_scratch')]
    + VIEWS + SIXTEEN_BIT + GROUP_NOISE + [
        (dict(M=1), EINVAL), (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(n_rows=0), EINVAL),
        (dict(M=257), ERANGE), (dict(S=5), ERANGE),
        (dict(z_first=-4), EINVAL), (dict(nz=24, n_rows=32), EINVAL), (dict(z_first=4), EINVAL),
        (dict(nz=18), EINVAL), (dict(z_first=2, n_rows=8), EINVAL),
        (VOXELS, ERANGE), (dict(layout=2), EINVAL),
        (HUGE, ERANGE),
        # two faults
        (dict(M=1, S=5), EINVAL), (dict(M=257, ve=11), EINVAL), (dict(M=257, nz=18), ERANGE), (dict(z_first=2, n_rows=8, **VOXELS), EINVAL),
        (dict(layout=2, **VOXELS), ERANGE), (dict(w2=1, n_rows=65536, nz=65536), ERANGE), (dict(w2=1, noise=SAMPLE, S=5), ERANGE),
        (dict(w2=1, noise=SAMPLE, S=3, layout=2), EINVAL), (dict(var=1, **HUGE), EINVAL),
        (dict(w2=1, var=1, lo=LOG, **HUGE), EINVAL), (dict(noise=SAMPLE, S=3), EINVAL),
    ],
    siddon_packed: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'vol_z2', 'mu', 'weights', 'counts')]
    + VIEWS + SIXTEEN_BIT + NOISE_EINVAL + [
        (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(M=1), ERANGE), (dict(M=5), ERANGE), (dict(S=5), ERANGE),
        (dict(w2=1, var=1, S=3), ERANGE), (dict(w2=1, noise=SAMPLE, S=3), ERANGE),
        (dict(n_rows=0), EINVAL), (dict(z_first=-16), EINVAL), (dict(nz=24, n_rows=32), EINVAL), (dict(z_first=16), EINVAL),
        (dict(nz=24), EINVAL), (dict(nz=32, z_first=4, n_rows=8), EINVAL),
        (PACKED_BYTES, ERANGE), (dict(nx=2048), ERANGE), (dict(ny=2048), ERANGE),
        (dict(layout=2), EINVAL), (HUGE, ERANGE),
        (dict(w2=1, var=1, lo=LOG), EINVAL), (dict(w2=1, var=1, noise='nosample', lo=LOG), EINVAL),
        # two faults
        (dict(M=1, nE=0), EINVAL), (dict(M=5, ve=11), ERANGE), (dict(w2=1, M=5), ERANGE), (dict(w2=1, nx=2048), EINVAL),
        (dict(w2=1, var=1, S=3, ve=11), ERANGE), (dict(nz=24, nx=2048), EINVAL), (dict(layout=2, nx=2048), ERANGE),
        (dict(layout=2, **HUGE), EINVAL), (dict(w2=1, var=1, lo=LOG, **HUGE), ERANGE), (dict(w2=1, var=1, lo=LOG, nx=2048), ERANGE),
        (dict(ve=11, **PACKED_BYTES), EINVAL),
    ],
    siddon_grouped_packed: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'codes', 'mu', 'weights', 'counts', 'acc_scratch')]
    + VIEWS + SIXTEEN_BIT + GROUP_NOISE + [
        (dict(M=1), EINVAL), (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(M=257), ERANGE), (dict(S=5), ERANGE),
        (dict(n_rows=0), EINVAL), (dict(z_first=-16), EINVAL), (dict(nz=24, n_rows=32), EINVAL), (dict(z_first=16), EINVAL),
        (dict(nz=24), EINVAL), (dict(nz=32, z_first=4, n_rows=8), EINVAL),
        (PACKED_BYTES, ERANGE), (dict(nx=2048), ERANGE), (dict(ny=2048), ERANGE),
        (dict(layout=2), EINVAL), (HUGE, ERANGE),
        # two faults
        (dict(M=1, S=5), EINVAL), (dict(M=257, ve=11), ERANGE), (dict(M=257, nE=0), EINVAL), (dict(nz=24, nx=2048), EINVAL),
        (dict(layout=2, nx=2048), ERANGE), (dict(w2=1, nx=2048), ERANGE), (dict(w2=1, **HUGE), ERANGE),
        (dict(w2=1, noise=SAMPLE, S=3, layout=2), EINVAL), (dict(w2=1, noise=SAMPLE, S=5), ERANGE), (dict(noise=SAMPLE, S=3), EINVAL),
    ],
    cone_project: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'view_cs', 'chan_cs', 'row_z', 'vol_yx', 'vol_xy', 'mu', 'weights',
                                                   'counts')]
    + VIEWS + SIXTEEN_BIT + NOISE_EINVAL + SLOPE + [
        (dict(w2=1, var=1, lo=LOG), EINVAL), (dict(w2=1, var=1, noise='nosample', lo=LOG), EINVAL),
        (dict(M=0), EINVAL), (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(n_rows=0), EINVAL),
        (dict(M=257), ERANGE), (dict(S=5), ERANGE), (VOXELS, ERANGE),
        # two faults
        (dict(w2=1, M=257), EINVAL), (dict(w2=1, var=1, lo=LOG, S=5), EINVAL), (dict(ve=11, M=257), EINVAL), (dict(M=0, S=5), EINVAL),
        (dict(M=257, n_rows=0), EINVAL), (dict(var=1, dz_max=1e4), EINVAL), (dict(ve=11, dz_max=1e4), EINVAL),
        (dict(nE=0, **VOXELS), EINVAL), (dict(w2=1, n_rows=65536), EINVAL),
    ],
    cone_rows: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'view_cs', 'chan_cs', 'row_z', 'vol_zc', 'mu', 'weights', 'counts')]
    + VIEWS + SIXTEEN_BIT + NOISE_EINVAL + SLOPE + [
        (dict(w2=1, var=1, lo=LOG), EINVAL), (dict(w2=1, var=1, noise='nosample', lo=LOG), EINVAL),
        (dict(M=0), EINVAL), (dict(M=4), ERANGE),
        (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(n_rows=0), EINVAL), (dict(S=5), ERANGE),
        (CONE_BYTES, ERANGE), (HUGE, ERANGE),
        # two faults
        (dict(w2=1, M=4), EINVAL), (dict(M=4, ve=11), ERANGE), (dict(M=4, nE=0), ERANGE), (dict(M=0, S=5), EINVAL),
        (dict(ve=11, S=5), EINVAL), (dict(nE=0, dz_max=1e4), EINVAL), (dict(S=5, n_rows=0), EINVAL), (dict(var=1, **HUGE), EINVAL),
        (dict(ve=11, **CONE_BYTES), EINVAL),
    ],
    cone_grouped: [(dict(null=n), EINVAL) for n in ('geom', 'plan', 'view_cs', 'chan_cs', 'row_z', 'vol_zcg', 'mu', 'weights', 'counts',
                                                   'acc_scratch')]
    + VIEWS + SIXTEEN_BIT + GROUP_NOISE + SLOPE + [
        (dict(M=0), EINVAL), (dict(M=257), ERANGE),
        (dict(nE=0), EINVAL), (dict(S=0), EINVAL), (dict(n_rows=0), EINVAL), (dict(S=5), ERANGE),
        (CONE_BYTES, ERANGE), (HUGE, ERANGE),
        (dict(w2=1, noise=SAMPLE, M=1), ERANGE),          # one material goes to the general detection, which draws no sample
        # two faults
        (dict(M=257, ve=11), ERANGE), (dict(M=0, S=5), EINVAL), (dict(ve=11, S=5), EINVAL), (dict(w2=1, dz_max=1e4), ERANGE),
        (dict(w2=1, S=5), ERANGE), (dict(w2=1, **HUGE), EINVAL), (dict(w2=1, var=1, lo=LOG, **HUGE), EINVAL),
        (dict(w2=1, noise=SAMPLE, M=1, **HUGE), ERANGE), (dict(noise=SAMPLE, S=3), EINVAL), (dict(nE=0, **CONE_BYTES), EINVAL),
    ],
}

TABLE = [pytest.param(fn, kw, code, id=f'{fn.__name__}-{i:02d}-' + '-'.join(f'{k}={v}' for k, v in kw.items()))
         for fn, cases in CASES.items() for i, (kw, code) in enumerate(cases)]


@pytest.fixture(scope='module')
def lib():
    return _native.load()


@pytest.mark.parametrize('fn,kw,code', TABLE)
def test_refused_call_returns_the_recorded_code(lib, fn, kw, code):
    assert fn(lib, **dict(kw)) == code
