"""Every capped-grid kernel past its cap, and the two SIRT steps directly, through the bare C ABI on guarded buffers.

Ten entry points launch a bounded number of workgroups and walk the rest of their input in a grid-stride loop; the per-kernel
modules stay inside the first pass of that loop.  Here every one of them gets inputs that make the loop run a second time (size
A: a handful of work items into pass 2, ragged) and a third (size B, one K only).  tests/grid_caps.py derives the sizes from the
``constexpr`` caps in csrc/*.hip and builds the problems from the generators, references and bounds of the per-kernel modules;
tests/test_grid_caps.py shows on the CPU that the comparisons used here reject a missing and a late second pass.  With W = 4096 x
256 = 1 048 576 work items (volume_remap: 8192 x 256; bhc: C = 2 n_cu workgroups of 1024):

  entry point (kernel)                        test                   sizes
  dexct_cov_precision (cov_precision<K>)      test_precision         K = 1, 2, 3: n = W + 1 and W + 9 (every unusable kind again at
                                                                     rays W + 2 .. W + 7); K = 2: 2 W + 259
  dexct_pwls_majorizer (<K,4> / <K,1>)        test_majorizer         K = 1, 2, 3: n = 4 W + 4 (float4), W + 1 (scalar); K = 2: W + 4
                                                                     with every buffer 4 bytes off (scalar)
  dexct_pwls_residual (<K,4> / <K,1>)         test_residual          K = 1, 2, 3: 2050 lines of 2052, step 1 (float4, 1 051 650
                                                                     items); 3075 lines of 1027, step 3 (scalar, 1 052 675 items: a
                                                                     pass boundary inside a line, skipped lines between); q apart
                                                                     and q = ax; q with objective, q alone, objective alone
  dexct_pwls_update (pwls_update<K>)          test_update            K = 1, 2, 3: (2, 509, 1031) = 1 049 558 pixels, pixel W in the
                                                                     last row of a slice at ix = 49; K = 2: (5, 509, 1031); nonneg
                                                                     both ways, g_scale 3
  dexct_sirt_residual                         test_sirt_residual     lines of 1, 63, 64, 65, 257 at steps 1 and 3; 3075 lines of
                                                                     1027 at step 3, 1022 lines of 1027 at step 1; r = NULL with
                                                                     norm2, r = ax with norm2, r apart without
  dexct_sirt_update                           test_sirt_update       n = 1, 63, 64, 65, 257, W + 1, 2 W + 259; nonneg both ways
  dexct_volume_ids                            test_volume_ids        W' + 4099, 2 W' + 16 x 257 + 5 bytes (W' = 16 W)
  dexct_volume_remap                          test_volume_remap      W' + 4099, 2 W' + 4 x 257 + 3 bytes (W' = 8192 x 256 x 4)
  dexct_bhc_linearize, float4 / scalar        test_bhc               C 8192 + 8197, 2 C 8192 + 12 301 (p and out 4 bytes off) /
                                                                     C 1024 + 1, 3 C 1024 + 77 (p at 0, out 4 bytes off)

Every case runs with guards, outputs and scratch filled with 0x00 and then with 0xFF, must leave the guards and the library's last
HIP error alone and give bit-identical outputs; buffers have exactly the size include/dexct.h promises.  Bounds: those of the
per-kernel tests (tests/test_gpu_pwls.py, tests/test_gpu_bounds.py); objective, penalty and norm2 at relative 1e-12 - every term
is non-negative, so the 4096 block partials and the per-thread chains of a few passes carry at most about (4096 + 16) 2^-53 =
4.6e-13; the SIRT steps against the float64 formula on the float32 inputs, with u = 2^-24 and no contraction in the build:
|r - ref| <= 2.02 u |ref| and |x' - ref| <= 1.01 u (|ref| + 2 |relax g / C|).

Found while writing this module: dexct_sirt_residual formed norm2 from the float32 difference b - ax, whose rounding (2^-24 per
term) left the sum 1.3e-11 (a million rays) to 6e-9 (a few hundred) from the float64 formula (tests/test_grid_caps.py::test_norm2_needs_the_float64_difference); the
kernel now forms that difference in float64, as pwls_residual_kernel does for its objective.  r is unchanged.

Measured on an MI355X (256 CUs, so C = 512), all 62 cases passing.  Worst error / bound: precision 0.50, majoriser 0.53, residual
0.68, update 0.94, sirt residual 0.98 (of 2.02 u |ref|), sirt update 0.99; bhc 0.42 of 4e-7 |ref| + 1e-9, NaN pattern and the
in-place result identical; volume ids and remap exact.  Relative errors of the sums: objective up to 4.1e-15, penalty 1.6e-15,
norm2 1.6e-15 past the cap and 1.9e-16 at the small sizes, against the 1e-12 allowed.  The float32 NumPy restatements of both SIRT
steps were reproduced bit for bit in all 26 runs (reported, not asserted: nothing states that the device division rounds
correctly).  Wall time: 28 s for the module; the float4 residual cases 1.6 / 4.0 / 6.1 s for K = 1 / 2 / 3 and the float4 majoriser
of K = 3 2.6 s - most of it the NumPy reference - every other case at most 1.4 s, so no size B had to go.  With each of the ten
loops cut down to its first pass the 42 past-cap cases here all fail, while tests/test_gpu_pwls.py, test_gpu_iter.py,
test_gpu_bhc.py and the three test_gpu_bounds* modules lose one case of 936, the 4096 x 256 x 16 + 16 bytes of
test_volume_ids_and_remap (its 8192 x 256 x 4 + 3 bytes of dexct_volume_remap end exactly on the first pass and still pass).
"""
import ctypes as C
import time

import numpy as np
import pytest

import grid_caps as gc
from guarded import Arena, GuardError, twice
from pwls_refs import F32, F64

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF)


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


def ok(rc):
    assert rc == 0, rc


class SinceStart:
    """dexct_last_hip_error is sticky, and argument-check tests of other modules leave it set on purpose: Arena.check, which
    wants 0 after every launch, gets 0 while the error is the one the case started with (tests/test_gpu_pwls.py compares the
    same two values once per case)."""

    def __init__(self, hip):
        self.hip, self.before = hip, hip.dexct_last_hip_error()

    def dexct_last_hip_error(self):
        now = self.hip.dexct_last_hip_error()
        return 0 if now == self.before else now


def arena(hip):
    return Arena('cuda', SinceStart(hip))


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f'wall time of {request.node.name}: {time.perf_counter() - t0:.1f} s')


def twice_on(ar, launch, out, scratch, written, idle=()):
    """guarded.twice for a call that leaves part of its output alone: only the ``written`` values [P] of every plane must agree
    bit for bit between the fills; the ``idle`` buffers must keep the fill.  Returns [(fill, host copy of ``out`` as float32
    [planes, P])]."""
    runs = []
    for byte in FILLS:
        ar.fill(byte, inner=(out,) + tuple(scratch))
        launch()
        ar.check()
        runs.append((byte, ar[out].get(F32).reshape(-1, written.size)))
        for name in idle:
            assert np.all(ar[name].get() == byte), f'{name} was written'
    a, b = runs[0][1][:, written].view(np.uint32), runs[1][1][:, written].view(np.uint32)
    if not np.array_equal(a, b):
        raise GuardError(f'output {out!r} depends on bytes outside the inputs')
    return runs


def untouched(ar, name, byte):
    assert np.all(ar[name].get() == byte), f'{name} was written'


# ---- PWLS ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', gc.cases('precision'))
def test_precision(hip, name):
    p = gc.CASES[name]()
    ar = arena(hip)
    ar.alloc('cov', p.cov.nbytes).put(p.cov)
    ar.alloc('w', 4 * p.ref.size)
    got = twice(ar, lambda: ok(hip.dexct_cov_precision(ar['cov'].ptr, p.n, p.K, p.w_fill, ar['w'].ptr, sp())), ['w'])['w'].view(F32)
    p.check_values(got)


@pytest.mark.parametrize('name', gc.cases('majorizer'))
def test_majorizer(hip, name):
    p = gc.CASES[name]()
    ar = arena(hip)
    ar.alloc('w', p.Wt.nbytes, p.offset).put(p.Wt)
    ar.alloc('R', p.R.nbytes, p.offset).put(p.R)
    ar.alloc('m', 4 * p.ref.size, p.offset)
    got = twice(ar, lambda: ok(hip.dexct_pwls_majorizer(ar['w'].ptr, ar['R'].ptr, p.n, p.K, ar['m'].ptr, sp())), ['m'])['m'].view(F32)
    p.check_values(got)
    assert np.all(got.reshape(p.K, -1)[:, p.R == 0] == 0)


@pytest.mark.parametrize('name', gc.cases('residual'))
def test_residual(hip, name):
    p = gc.CASES[name]()
    ar = arena(hip)
    for n, a in (('b', p.b), ('ax', p.ax), ('w', p.Wt), ('R', p.R)):
        ar.alloc(n, a.nbytes).put(a)
    ar.alloc('q', p.ax.nbytes)
    ar.alloc('obj', 8)

    def call(out, with_obj):
        def launch():
            ar['ax'].put(p.ax)
            ok(hip.dexct_pwls_residual(ar['b'].ptr, ar['ax'].ptr, ar['w'].ptr, ar['R'].ptr, p.plane, p.K, p.n_lines, p.step, p.line,
                                       ar[out].ptr if out else None, ar['obj'].ptr if with_obj else None, sp()))
            if with_obj:
                p.check_sum('objective', ar['obj'].get(F64)[0])
        return launch

    for out, with_obj in (('q', True), ('ax', True), ('q', False)):
        others = [n for n in ('q', 'obj') if n != out]
        idle = [n for n in others if n != 'obj' or not with_obj]
        for byte, got in twice_on(ar, call(out, with_obj), out, others, p.written, idle):
            p.check_values(got, keep=p.ax if out == 'ax' else p.fill(byte), what=f'q={out} objective={with_obj}')
            assert np.all(got[:, p.written][:, p.R[p.written] == 0] == 0)
    for byte in FILLS:                                                # the objective alone
        ar.fill(byte, inner=('q', 'obj'))
        call(None, True)()
        ar.check()
        untouched(ar, 'q', byte)
        assert np.array_equal(ar['ax'].get(F32), p.ax.reshape(-1))


@pytest.mark.parametrize('name', gc.cases('update'))
def test_update(hip, name):
    p = gc.CASES[name]()
    ar = arena(hip)
    for n, a in (('x', p.x), ('g', p.g), ('d', p.d)):
        ar.alloc(n, a.nbytes).put(a)
    ar.alloc('y', p.x.nbytes)
    ar.alloc('pen', 8)
    beta, delta = (C.c_double * p.K)(*p.beta), (C.c_double * p.K)(*p.delta)

    def launch():
        ok(hip.dexct_pwls_update(ar['x'].ptr, ar['g'].ptr, ar['d'].ptr, p.K, *p.grid, p.g_scale, beta, delta, int(p.nonneg),
                                 ar['y'].ptr, ar['pen'].ptr, sp()))
        p.check_sum('penalty', ar['pen'].get(F64)[0])

    got = twice(ar, launch, ['y'], scratch=['pen'])['y'].view(F32)
    p.check_values(got)
    assert np.array_equal(ar['x'].get(F32), p.x.reshape(-1))
    if p.nonneg:
        assert got.min() >= 0 and (p.ref == 0).any()


# ---- the SIRT steps ------------------------------------------------------------------------------------------------------------

def sirt_residual(hip, p):
    ar = arena(hip)
    for n, a in (('b', p.b), ('ax', p.ax), ('R', p.R)):
        ar.alloc(n, a.nbytes).put(a)
    ar.alloc('r', p.ax.nbytes)
    ar.alloc('norm2', 8)

    def call(out, with_norm):
        def launch():
            ar['ax'].put(p.ax)
            ok(hip.dexct_sirt_residual(ar['b'].ptr, ar['ax'].ptr, ar['R'].ptr, p.n_lines, p.step, p.line, ar[out].ptr if out else None,
                                       ar['norm2'].ptr if with_norm else None, sp()))
            if with_norm:
                p.check_sum('norm2', ar['norm2'].get(F64)[0])
        return launch

    exact = []
    for out, with_norm in (('ax', True), ('r', False)):
        others = [n for n in ('r', 'norm2') if n != out]
        idle = [n for n in others if n != 'norm2' or not with_norm]
        for byte, got in twice_on(ar, call(out, with_norm), out, others, p.written, idle):
            p.check_values(got, keep=p.ax[None] if out == 'ax' else p.fill(byte), what=f'r={out} norm2={with_norm}')
            assert np.all(got[0, p.written & (p.R == 0)] == 0)          # exactly 0 (and out of norm2: check_sum)
            exact.append(np.array_equal(got[:, p.written].view(np.uint32), p.f32[:, p.written].view(np.uint32)))
    for byte in FILLS:                                                # norm2 alone
        ar.fill(byte, inner=('r', 'norm2'))
        call(None, True)()
        ar.check()
        untouched(ar, 'r', byte)
        assert np.array_equal(ar['ax'].get(F32), p.ax)
    print(f'{p.label}: the float32 NumPy restatement is {"" if all(exact) else "NOT "}reproduced bit for bit')


@pytest.mark.parametrize('line,n_lines,step', gc.SIRT_SMALL)
def test_sirt_residual_small(hip, line, n_lines, step):
    sirt_residual(hip, gc.SirtResidual(line, n_lines, step))


@pytest.mark.parametrize('name', gc.cases('sirt_residual'))
def test_sirt_residual(hip, name):
    sirt_residual(hip, gc.CASES[name]())


def sirt_update(hip, p):
    ar = arena(hip)
    ar.alloc('x', p.x.nbytes)
    ar.alloc('g', p.g.nbytes).put(p.g)
    ar.alloc('C', p.C.nbytes).put(p.C)

    def launch():
        ar['x'].put(p.x)
        ok(hip.dexct_sirt_update(ar['x'].ptr, ar['g'].ptr, ar['C'].ptr, p.n, p.relax, int(p.nonneg), sp()))

    got = twice(ar, launch, ['x'])['x'].view(F32)
    p.check_values(got)
    assert np.array_equal(got[p.stay].view(np.uint32), (np.maximum(p.x[p.stay], 0) if p.nonneg else p.x[p.stay]).view(np.uint32))
    same = np.array_equal(got.view(np.uint32), p.f32[0].view(np.uint32))
    print(f'{p.label}: the float32 NumPy restatement is {"" if same else "NOT "}reproduced bit for bit')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('nonneg', [False, True])
def test_sirt_update_small(hip, n, nonneg):
    sirt_update(hip, gc.SirtUpdate(n, nonneg))


@pytest.mark.parametrize('name', gc.cases('sirt_update'))
def test_sirt_update(hip, name):
    sirt_update(hip, gc.CASES[name]())


# ---- volume ids ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', gc.cases('volume_ids'))
def test_volume_ids(hip, name):
    p = gc.CASES[name]()
    ar = arena(hip)
    ar.alloc('vol', p.n).put(p.vol)
    ar.alloc('counts256', 2048)
    got = twice(ar, lambda: ok(hip.dexct_volume_ids(ar['vol'].ptr, p.n, ar['counts256'].ptr, sp())), ['counts256'])
    p.check_counts(got['counts256'].view(np.uint64))


@pytest.mark.parametrize('name', gc.cases('volume_remap'))
def test_volume_remap(hip, name):
    p = gc.CASES[name]()
    lut = (C.c_uint8 * 256)(*gc.REMAP_LUT.tolist())
    ar = arena(hip)
    ar.alloc('vol', p.n)

    def remap():
        ar['vol'].put(p.vol)
        ok(hip.dexct_volume_remap(ar['vol'].ptr, p.n, lut, sp()))

    p.check_values(twice(ar, remap, ['vol'])['vol'])


# ---- beam hardening ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', gc.cases('bhc'))
def test_bhc(hip, name):
    p = gc.CASES[name]()
    t, (po, oo) = p.table, p.OFFSETS[p.path]
    tab = t.pairs()
    args = (t.log2_min, t.cells_log2, t.oct_pos, t.oct_neg)
    ar = arena(hip)
    ar.alloc('table', tab.nbytes).put(tab)
    ar.alloc('p', 4 * p.n, po).put(p.p)
    ar.alloc('out', 4 * p.n, oo)
    got = twice(ar, lambda: ok(hip.dexct_bhc_linearize(ar['p'].ptr, p.n, ar['table'].ptr, *args, ar['out'].ptr, sp())), ['out'])['out'].view(F32)
    p.check_values(got)

    def in_place():
        ar['p'].put(p.p)
        ok(hip.dexct_bhc_linearize(ar['p'].ptr, p.n, ar['table'].ptr, *args, ar['p'].ptr, sp()))

    same = twice(ar, in_place, ['p'], scratch=['out'])['p'].view(F32)
    assert np.array_equal(same.view(np.int32), got.view(np.int32))
