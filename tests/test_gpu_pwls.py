"""The joint PWLS reconstruction on the GPU (csrc/pwls.hip, iterative.pwls, back_project.get_basismat_recon) against
tests/pwls_refs.py on the small scans of tests/iter_refs.py.

Bounds (u = 2^-24):
  precision   one float32 rounding of the float64 inverse, whose own error at |rho| <= 0.999 (condition ~ 2e3) is orders
              below it: 2^-23 |ref| per element.
  majoriser,  (K + 2) u sum_l |w_kl| |r_l| per element: the rounding of r_l, of the product, of the K - 1 additions, one spare
  residual    (the majoriser: R in the place of r_l, and the final product).  Objectives: 1e-12 of the float64 sum.
  update      pwls_refs.update_bound, derived there.
  pwls        d32 = max |float32 reference - float64 reference| measures how far float32 rounding carries through 5 iterations
              of THIS problem; the device result lies within 8 d32 of the float64 reference (the factor of
              test_sirt_matches_reference for the same atomics).  CHANGED for the one-pixel grid ('one'), whose cases measure
              above 8 whenever the atomics fall in another order: there d32 is a single rounding sample of K numbers, not a
              measure - the float32 reference can land on the float64 value by luck (K = 2, S = 3, x0 = 0: d32 = 1.0e-9 =
              0.03 u |x|, so ONE ulp of the result, 6e-8, is a ratio of 58) - and the worst ratio is not something a few runs
              measure.  On that grid d32 is floored at u max |reference|, half an ulp of the largest result: no float32
              computation of these numbers can be expected to land closer, and 8 of it is 4 ulps (``rounding_scale``).  The
              13 x 9 scans keep the plain d32 and the 8; test_diagonal_weights_decouple uses the same scale.

Measured on an MI355X, worst error / bound: precision 0.50, majoriser 0.48, residual 0.62, update 0.60; test_pwls_matches_reference
on the 13 x 9 scans 0.55 - 2.49 of d32 against the 8 allowed over three runs (per case in DESIGN.md section 4.10); on the
one-pixel grid up to 1.54 of the plain d32 in those runs, above 8 in a later one (which failed), and a computed 58 for one ulp.  The module takes about 8 s, 4 s of
them the one run of main.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iter_refs as ir
import pwls_refs as pr
from guarded import Arena, twice
from pwls_refs import F32, F64, U

pytestmark = pytest.mark.gpu

SCANS = ['c53', 'c65', 'one']
BETA, DELTA = [0.5, 2.0, 1.0], [0.1, 0.05, 0.2]


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = ir.system_matrix(ir.small(name))
    A.setflags(write=False)
    return A


def projector(name):
    from dex_ct_sim_amd.iterative import ImageProjector
    s = ir.small(name)
    return ImageProjector.from_grid(s.nx, s.ny, s.nz, s.dx, s.dy, s.n_views, s.n_ch, s.n_rows, s.z_first, s.sid, s.sdd, s.view_cs,
                                    s.chan_cs)


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def worst(got, ref, bound, what):
    got = np.asarray(got, F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf))
    print(f'{what}: worst error / bound {ratio.max():.3f}')
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound), (what, float(ratio.max()))


def rel_close(got, ref, what, tol=1e-12):
    print(f'{what}: {got!r} against {ref!r}, relative {abs(got - ref) / abs(ref) if ref else abs(got):.2e}')
    assert abs(got - ref) <= tol * abs(ref), what


# ---- 1: precision --------------------------------------------------------------------------------------------------------------

def covariances(n, K, seed):
    """[n, T]: standard deviations over two decades; K = 2: rho up to +-0.999; K = 3: rho_01, rho_02 up to +-0.9 and a partial
    correlation t of channels 1 and 2 up to +-0.999, rho_12 = rho_01 rho_02 + t sqrt((1 - rho_01^2)(1 - rho_02^2)) - positive
    definite for every |t| < 1, without the structural zero an AR(1) matrix has in its inverse.  The first two rays sit at the
    ends of the range."""
    rng = np.random.default_rng(seed)
    sd = 10.0 ** rng.uniform(-2.0, 0.0, (n, K))
    t = rng.uniform(-0.999, 0.999, n)
    t[:2] = (-0.999, 0.999)[:min(n, 2)]
    r = np.ones((n, K, K))
    if K == 2:
        r[:, 0, 1] = t
    elif K == 3:
        r01, r02 = rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n)
        r[:, 0, 1], r[:, 0, 2], r[:, 1, 2] = r01, r02, r01 * r02 + t * np.sqrt((1 - r01 ** 2) * (1 - r02 ** 2))
    cov = np.empty((n, K * (K + 1) // 2))
    for k in range(K):
        for l in range(k, K):
            cov[:, pr.tri(K, k, l)] = sd[:, k] * sd[:, l] * r[:, k, l]
    return cov


def spoil(cov, K):
    """every unusable kind, at rays 2 .. 6 (7 for K > 1): zeros, NaN, inf, -inf, a negative diagonal, an indefinite matrix"""
    cov[2] = 0.0
    cov[3, 0] = np.nan
    cov[4, -1] = np.inf
    cov[5, 0] = -np.inf
    cov[6, -1] = -cov[6, -1]
    bad = [2, 3, 4, 5, 6]
    if K > 1:
        cov[7, 1] = 3.0 * np.sqrt(cov[7, 0] * cov[7, K])          # |rho| = 3
        bad.append(7)
    return bad


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 7 * 2 * 53])
def test_precision_against_reference(hip, K, n):
    from dex_ct_sim_amd.iterative import precision_weights
    cov = covariances(n, K, 31 + n)
    bad = spoil(cov, K) if n > 8 else []
    ref, ok = pr.precision_ref(cov, K, 0.75)
    assert list(np.flatnonzero(~ok)) == bad
    got = precision_weights(dev(cov, F64), 0.75).cpu().numpy()
    assert got.dtype == F32 and got.shape == ref.shape
    worst(got[:, ok], ref[:, ok], 2.0 ** -23 * np.abs(ref[:, ok]), f'precision K={K} n={n}')
    assert np.array_equal(got[:, ~ok], ref[:, ~ok].astype(F32))                # exactly w_fill / 0


@pytest.mark.parametrize('K', [1, 2, 3])
def test_precision_of_every_unusable_kind(hip, K):
    from dex_ct_sim_amd.iterative import precision_weights
    cov = covariances(10, K, 32)
    bad = spoil(cov, K) + [9]
    cov[9] *= 1e-42                      # positive definite in float64, but every weight is beyond the float32 range
    assert list(np.flatnonzero(~pr.precision_ref(cov, K)[1])) == bad
    for w_fill in (0.0, 2.5):
        got = precision_weights(dev(cov, F64), w_fill).cpu().numpy()
        for t in range(got.shape[0]):
            diag = t in [pr.tri(K, k, k) for k in range(K)]
            assert np.all(got[t, bad] == F32(w_fill if diag else 0.0)), (t, got[t])
        assert np.all(got[0, [0, 1, 8]] > 0) and np.all(np.isfinite(got))


# ---- 2: majoriser and residual -------------------------------------------------------------------------------------------------

def sino_inputs(shape, K, seed):
    rng = np.random.default_rng(seed)
    T = K * (K + 1) // 2
    b = rng.uniform(-1.0, 1.0, (K,) + shape).astype(F32)
    ax = rng.uniform(-1.0, 1.0, (K,) + shape).astype(F32)
    _, W = pr.correlated_weights(rng, shape, K, -0.9, 0.1)
    R = np.where(rng.uniform(size=shape) < 0.15, 0.0, rng.uniform(0.5, 3.0, shape)).astype(F32)
    return b, ax, W.astype(F32), R, T


SHAPES = {'c53': (7, 2, 53), 'c65': (7, 2, 65), 'wide': (7, 1, 64), 'one': (1, 1, 1)}


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_majorizer_against_numpy(hip, K, shape):
    shape = SHAPES[shape]
    _, _, W, R, T = sino_inputs(shape, K, 41)
    n = int(np.prod(shape))
    m = torch.full((K,) + shape, 7.5, dtype=torch.float32, device='cuda')
    w_d, R_d = dev(W), dev(R)
    assert hip.dexct_pwls_majorizer(w_d.data_ptr(), R_d.data_ptr(), n, K, m.data_ptr(), sp()) == 0
    W2, R1 = W.reshape(T, -1), R.reshape(-1)
    ref = pr.majorizer_ref(W2, R1, K, F64)
    bound = np.stack([(K + 2) * U * sum(np.abs(W2[pr.tri(K, k, l)].astype(F64)) for l in range(K)) * R1 for k in range(K)])
    worst(m.cpu().numpy().reshape(K, -1), ref, bound, f'majoriser K={K} {shape}')
    assert np.all(m.cpu().numpy().reshape(K, -1)[:, R1 == 0] == 0)


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('shape', ['c53', 'c65', 'wide'])
@pytest.mark.parametrize('begin,step', [(0, 1), (1, 3)])
@pytest.mark.parametrize('alias', [False, True])
def test_residual_against_numpy(hip, K, shape, begin, step, alias):
    shape = SHAPES[shape]
    b, ax, W, R, T = sino_inputs(shape, K, 42)
    n_views, line = shape[0], shape[1] * shape[2]
    plane = n_views * line
    on = np.repeat((np.arange(n_views) >= begin) & ((np.arange(n_views) - begin) % step == 0), line)
    b_d, ax_d, w_d, R_d = dev(b), dev(ax), dev(W), dev(R)
    q_d = ax_d if alias else torch.full((K,) + shape, 7.5, dtype=torch.float32, device='cuda')
    obj = torch.full((1,), 123.0, dtype=torch.float64, device='cuda')
    off = 4 * begin * line
    rc = hip.dexct_pwls_residual(b_d.data_ptr() + off, ax_d.data_ptr() + off, w_d.data_ptr() + off, R_d.data_ptr() + off, plane, K,
                                 n_views - begin, step, line, q_d.data_ptr() + off, obj.data_ptr(), sp())
    assert rc == 0, rc
    b2, ax2, W2, R1 = b.reshape(K, -1), ax.reshape(K, -1), W.reshape(T, -1), R.reshape(-1)
    ref, ref_obj = pr.residual_ref(b2[:, on], ax2[:, on], W2[:, on], R1[on], K, F64)
    got = q_d.cpu().numpy().reshape(K, -1)
    hit = R1[on] > 0
    worst(got[:, on], ref, np.where(hit, pr.residual_bound(b2[:, on], ax2[:, on], W2[:, on], K), 0.0),
          f'residual K={K} {shape} {begin}:{step} alias={alias}')
    assert np.any(ref != 0) and np.any(~hit) and np.all(got[:, on][:, ~hit] == 0)
    assert np.array_equal(got[:, ~on], ax2[:, ~on] if alias else np.full_like(got[:, ~on], 7.5))     # the other lines stay
    rel_close(float(obj.item()), ref_obj, 'data objective')
    # the objective alone, without q
    obj.fill_(5.0)
    ax_d = dev(ax)
    rc = hip.dexct_pwls_residual(b_d.data_ptr() + off, ax_d.data_ptr() + off, w_d.data_ptr() + off, R_d.data_ptr() + off, plane,
                                 K, n_views - begin, step, line, None, obj.data_ptr(), sp())
    assert rc == 0
    rel_close(float(obj.item()), ref_obj, 'data objective alone')


# ---- 3: the update kernel alone ------------------------------------------------------------------------------------------------

def update_inputs(K, grid, seed):
    """differences of exactly 0, delta / 2, delta, 3 delta / 2 and more along every row or column of channel 0 (delta = 1 / 8,
    multiples of 1 / 16 are exact), random ones in the others; beta = 0 in the last channel of K > 1, whose d has zeros: pixels with d + c = 0"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (K,) + grid).astype(F32)
    x[0] = np.resize(np.array([0, 0, 1, 3, 6, 5, 3, 0, -4]) / 16.0, grid)
    g = rng.uniform(-1.0, 1.0, (K,) + grid).astype(F32)
    d = np.where(rng.uniform(size=(K,) + grid) < 0.3, 0.0, rng.uniform(0.5, 4.0, (K,) + grid)).astype(F32)
    beta, delta = [0.7, 1.3, 0.0][:K], [0.125, 0.05, 0.2][:K]
    if K > 1:
        beta[-1] = 0.0
    return x, g, d, beta, delta


GRIDS = {'13x9': (3, 9, 13), '1x1': (1, 1, 1), '1x9': (2, 9, 1), '13x1': (2, 1, 13)}


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('nonneg', [False, True])
@pytest.mark.parametrize('g_scale', [1.0, 3.0])
def test_update_against_formula(hip, K, grid, nonneg, g_scale):
    grid = GRIDS[grid]
    x, g, d, beta, delta = update_inputs(K, grid, 51)
    if K == 1 and grid[1] * grid[2] > 1:
        beta = [0.7]
    elif K == 1:
        beta = [0.0]                                                  # a pixel without a neighbour and with d = 0 stays
        d[0, 0, 0, 0] = 0.0
    x_d, y_d = dev(x), torch.full((K,) + grid, 7.5, dtype=torch.float32, device='cuda')
    g_d, d_d = dev(g), dev(d)
    pen = torch.full((1,), 9.0, dtype=torch.float64, device='cuda')
    rc = hip.dexct_pwls_update(x_d.data_ptr(), g_d.data_ptr(), d_d.data_ptr(), K, *grid, g_scale, (C.c_double * K)(*beta),
                               (C.c_double * K)(*delta), int(nonneg), y_d.data_ptr(), pen.data_ptr(), sp())
    assert rc == 0, rc
    got = y_d.cpu().numpy()
    ref = pr.update_ref(x, g, d, beta, delta, nonneg, g_scale, F64)
    worst(got, ref, pr.update_bound(x, g, d, beta, delta, g_scale), f'update K={K} {grid} nonneg={nonneg}')
    assert np.array_equal(x_d.cpu().numpy(), x)
    for k in range(K):
        _, c = pr.penalty_terms(x[k].astype(F64), beta[k], delta[k], F64)
        stay = d[k].astype(F64) + c == 0
        if beta[k] == 0.0 and (x[k].size > 1 or K == 1):
            assert stay.any()
        assert np.array_equal(got[k][stay], np.maximum(x[k][stay], 0) if nonneg else x[k][stay])
    if nonneg:
        assert got.min() >= 0 and ((ref == 0).any() or x[0].size == 1)
    if grid[1] * grid[2] > 1:
        t = np.abs(np.diff(x[0], axis=-1 if grid[2] > 1 else -2))
        assert (t < delta[0]).any() and (t == F32(delta[0])).any() and (t > delta[0]).any() and (t == 0).any()
    ref_pen = pr.penalty_ref(x, beta, delta)
    rel_close(float(pen.item()), ref_pen, 'penalty')
    assert (ref_pen > 0) == (grid[1] * grid[2] > 1 and beta[0] > 0)


# ---- 4: pwls against the reference ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pwls_problem(name, K):
    scan, A = ir.small(name), matrix(name)
    rng = np.random.default_rng(61)
    shape = (scan.n_views, scan.n_rows, scan.n_ch)
    x_true = rng.uniform(0.0, 1.0, (K, A.shape[1]))
    b = np.stack([(A @ x_true[k]) * rng.uniform(0.7, 1.3, A.shape[0]) - 0.05 for k in range(K)]).reshape((K,) + shape)
    _, W = pr.correlated_weights(rng, shape, K, -0.9, 0.1)
    x0 = rng.uniform(0.0, 1.0, (K, scan.nz, scan.ny, scan.nx)).astype(F32)
    return b.astype(F32), W.astype(F32), x0


@functools.lru_cache(maxsize=None)
def pwls_refs(name, K, n_subsets, nonneg, given):
    scan = ir.small(name)
    b, W, x0 = pwls_problem(name, K)
    args = (matrix(name), b, W, 5, n_subsets, BETA[:K], DELTA[:K], nonneg, x0 if given else None, (scan.nz, scan.ny, scan.nx))
    return pr.pwls_ref(*args, dtype=F64), pr.pwls_ref(*args, dtype=F32)


def rounding_scale(name, ref64, ref32):
    """d32 = max |float32 reference - float64 reference|; on the one-pixel grid floored at u max |reference| (module
    docstring).  Returns (scale, plain d32)."""
    d32 = float(np.max(np.abs(ref32.astype(F64) - ref64)))
    return (max(d32, U * float(np.max(np.abs(ref64)))) if name == 'one' else d32), d32


@pytest.mark.parametrize('name', SCANS)
@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('n_subsets', [1, 3])
@pytest.mark.parametrize('nonneg', [False, True])
@pytest.mark.parametrize('given', [False, True])
def test_pwls_matches_reference(hip, name, K, n_subsets, nonneg, given):
    """5 iterations; the device images lie within 8 d32 of the float64 reference; on the one-pixel grid d32 is floored at half an
    ulp of the result (module docstring: the plain d32 there is a rounding sample that one ulp exceeds 58 times)."""
    from dex_ct_sim_amd.iterative import pwls
    b, W, x0 = pwls_problem(name, K)
    ref64, ref32 = pwls_refs(name, K, n_subsets, nonneg, given)
    scale, d32 = rounding_scale(name, ref64, ref32)
    x0_d = dev(x0) if given else None
    got = pwls(dev(b), dev(W), projector(name), 5, n_subsets, BETA[:K], DELTA[:K], x0=x0_d, nonneg=nonneg).cpu().numpy().astype(F64)
    err = float(np.max(np.abs(got - ref64)))
    print(f'pwls {name} K={K} S={n_subsets} nonneg={nonneg} x0={given}: err {err:.3e}, d32 {d32:.3e}, scale {scale:.3e}, '
          f'of plain d32 {err / d32 if d32 else np.inf:.3f}, ratio {err / scale:.3f}')
    assert got.shape == ref64.shape and np.all(np.isfinite(got))
    assert err <= 8.0 * scale
    if given:
        assert np.array_equal(x0_d.cpu().numpy(), x0)                 # the start images are the caller's
    if nonneg:
        assert got.min() >= 0.0


def test_pwls_history_is_the_objective(hip):
    from dex_ct_sim_amd.iterative import pwls
    for name, K, S in (('c53', 2, 1), ('c65', 3, 3)):
        scan = ir.small(name)
        b, W, x0 = pwls_problem(name, K)
        hist, ref_hist = [], []
        pwls(dev(b), dev(W), projector(name), 3, S, BETA[:K], DELTA[:K], x0=dev(x0), history=hist)
        pr.pwls_ref(matrix(name), b, W, 3, S, BETA[:K], DELTA[:K], False, x0, (scan.nz, scan.ny, scan.nx), F64, ref_hist)
        print('history', hist, ref_hist)
        rel_close(hist[0], ref_hist[0], 'objective of x0', 1e-5)      # one float32 forward projection away
        assert len(hist) == 3 and np.allclose(hist, ref_hist, rtol=1e-4, atol=0)


def test_majoriser_is_kept_per_weight_tensor(hip):
    from dex_ct_sim_amd.iterative import pwls
    b, W, _ = pwls_problem('c53', 2)
    p, w_d = projector('c53'), dev(W)
    pwls(dev(b), w_d, p, 1)
    first = p._pwls_d[2]
    pwls(dev(b), w_d, p, 1)
    assert p._pwls_d[2] is first
    w_d.mul_(2.0)                                                     # changed in place: made again
    pwls(dev(b), w_d, p, 1)
    assert p._pwls_d[2] is not first
    pwls(dev(b), dev(W), p, 1)                                        # another tensor
    assert p._pwls_d[0]() is not w_d
    p.forget_weights()                                                # after a write through the raw pointer
    assert p._pwls_d is None


# ---- 5: fixed point ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['c65', 'one'])
@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('n_subsets', [1, 3])
@pytest.mark.parametrize('beta', [0.0, 0.8])
def test_fixed_point_is_bit_identical(hip, name, K, n_subsets, beta):
    from dex_ct_sim_amd.iterative import pwls
    scan = ir.small(name)
    rng = np.random.default_rng(71)
    grid = (K, scan.nz, scan.ny, scan.nx)
    x_true = rng.uniform(0.0, 1.0, grid) if beta == 0.0 else np.broadcast_to(rng.uniform(0.2, 1.0, (K, 1, 1, 1)), grid)
    x_true = dev(x_true)
    p = projector(name)
    b = torch.stack([p.forward(x_true[k]) for k in range(K)])
    _, W, _ = pwls_problem(name, K)
    hist = []
    x = pwls(b, dev(W), p, 1, n_subsets, beta, 0.1, x0=x_true, history=hist)
    assert np.array_equal(x.cpu().numpy(), x_true.cpu().numpy()) and hist == [0.0]


# ---- 6: a diagonal W decouples the channels ------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['c53', 'one'])
@pytest.mark.parametrize('n_subsets', [1, 3])
def test_diagonal_weights_decouple(hip, name, n_subsets):
    from dex_ct_sim_amd.iterative import pwls
    scan = ir.small(name)
    b, W, x0 = pwls_problem(name, 2)
    W = W.copy()
    W[1] = 0.0
    args = (matrix(name), b, W, 5, n_subsets, BETA[:2], DELTA[:2], False, x0, (scan.nz, scan.ny, scan.nx))
    scale, d32 = rounding_scale(name, pr.pwls_ref(*args, dtype=F64), pr.pwls_ref(*args, dtype=F32))
    p = projector(name)
    joint = pwls(dev(b), dev(W), p, 5, n_subsets, BETA[:2], DELTA[:2], x0=dev(x0)).cpu().numpy().astype(F64)
    for k in range(2):
        single = pwls(dev(b[k:k + 1]), dev(W[2 * k:2 * k + 1]), p, 5, n_subsets, BETA[k], DELTA[k], x0=dev(x0[k:k + 1]))
        err = float(np.max(np.abs(single.cpu().numpy()[0].astype(F64) - joint[k])))
        print(f'diagonal {name} S={n_subsets} channel {k}: |joint - single| {err:.3e}, d32 {d32:.3e}, scale {scale:.3e}')
        assert err <= 8.0 * scale


# ---- 7: the public path --------------------------------------------------------------------------------------------------------

def two_discs(n):
    yy, xx = np.mgrid[0:n, 0:n] - 0.5 * (n - 1)
    a, c = np.zeros((n, n), F32), np.zeros((n, n), F32)
    a[(xx + 0.15 * n) ** 2 + yy ** 2 < (0.22 * n) ** 2] = 0.2
    c[(xx - 0.2 * n) ** 2 + (yy - 0.1 * n) ** 2 < (0.1 * n) ** 2] = 0.45
    return np.stack([a, c])


def non_increasing(h, slack):
    return all(b <= a * (1 + slack) for a, b in zip(h[:-1], h[1:]))


def test_public_path(hip):
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import synthetic
    from dex_ct_sim_amd.back_project import get_basismat_recon, get_recon
    from dex_ct_sim_amd.iterative import ImageProjector, precision_weights
    n, fov = 32, 20.0
    ct = dx.FanBeamGeometry(N_channels=64, N_proj=48)
    spec = synthetic.kramers_spectrum(80)
    x_true = two_discs(n)
    p = ImageProjector(ct, n, fov)
    clean = np.stack([p.forward(dev(x_true[k][None])).cpu().numpy()[:, 0, :] for k in range(2)])
    # noise of a per-ray covariance with rho = -0.9, drawn in NumPy
    rng = np.random.default_rng(81)
    sd = rng.uniform(0.02, 0.06, (2,) + clean.shape[1:])
    cov = np.stack([sd[0] ** 2, -0.9 * sd[0] * sd[1], sd[1] ** 2], axis=-1)
    z = rng.standard_normal((2,) + clean.shape[1:])
    noisy = np.stack([clean[0] + sd[0] * z[0], clean[1] + sd[1] * (-0.9 * z[0] + np.sqrt(1 - 0.81) * z[1])]).astype(F32)
    beta, delta = 2.0, 0.02
    hist = []
    imgs = get_basismat_recon(noisy, cov, ct, n, fov, 1.0, beta, delta, n_iters=12, init='zero', history=hist)
    print('pwls history', hist)
    assert len(imgs) == 2 and all(im.shape == (n, n) and im.dtype == np.float32 for im in imgs)
    assert len(hist) == 12 and hist[-1] < hist[0] and non_increasing(hist, 1e-5)
    # init='fbp' starts at the objective of the FBP images
    fbp = np.stack([get_recon(noisy[k], ct, spec, n, fov, 1.0)[0] for k in range(2)])
    W = precision_weights(dev(cov, F64)).cpu().numpy().astype(F64)
    R = p.row_sums().cpu().numpy().astype(F64)[:, 0, :]
    ax = np.stack([p.forward(dev(fbp[k][None])).cpu().numpy()[:, 0, :] for k in range(2)])
    _, data = pr.residual_ref(noisy.reshape(2, -1), ax.reshape(2, -1), W.reshape(3, -1), R.reshape(-1), 2, F64)
    phi_fbp = data + pr.penalty_ref(fbp[:, None], [beta] * 2, [delta] * 2)
    hist_f = []
    imgs_f = get_basismat_recon(noisy, cov, ct, n, fov, 1.0, beta, delta, n_iters=3, history=hist_f)
    rel_close(hist_f[0], phi_fbp, 'objective of the FBP images', 1e-9)
    assert hist_f[-1] < hist_f[0] and non_increasing(hist_f, 1e-5)
    # the noise goes down: standard deviation inside the large disc of channel 0, FBP against PWLS
    roi = x_true[0] > 0
    roi &= np.roll(roi, 2, 0) & np.roll(roi, -2, 0) & np.roll(roi, 2, 1) & np.roll(roi, -2, 1)
    print(f'ROI standard deviation: fbp {fbp[0][roi].std():.4f}, pwls {imgs_f[0][roi].std():.4f}')
    # device tensors in, device tensors out; ordered subsets; a per-channel penalty; a non-finite value
    bad = noisy.copy()
    bad[1, 5, 7] = np.nan
    with pytest.warns(RuntimeWarning, match='non-finite'):
        t = get_basismat_recon([dev(bad[0]), dev(bad[1])], dev(cov, F64), ct, n, fov, 1.0, (beta, 0.5), (delta, 0.01), n_iters=2,
                               n_subsets=4, w_fill=0.0)
    assert all(isinstance(im, torch.Tensor) and im.is_cuda and bool(torch.isfinite(im).all()) for im in t)
    # get_recon(method='pwls') is the K = 1 case.  The two calls run the same kernels on the same values; only the order of
    # the adjoint's float atomics differs from run to run.  A pixel sums about 2 x 48 products per adjoint, d32-like growth
    # over 3 iterations stays below 3 * 100 u = 2e-5 of the largest value; 1e-4 leaves a factor of 5.
    w1 = (1.0 / sd[0] ** 2).astype(F32)
    h1, hk = [], []
    raw, hu = get_recon(noisy[0], ct, spec, n, fov, 1.0, method='pwls', weights=w1, beta=beta, delta=delta, n_iters=3, nonneg=False,
                        history=h1)
    one, = get_basismat_recon([noisy[0]], (1.0 / w1.astype(F64))[..., None], ct, n, fov, 1.0, beta, delta, n_iters=3, history=hk)
    assert raw.shape == hu.shape == (n, n) and np.max(np.abs(raw - one)) <= 1e-4 * np.max(np.abs(one))
    assert len(h1) == 3 and abs(h1[0] - hk[0]) <= 1e-12 * hk[0]
    with pytest.warns(RuntimeWarning, match='non-finite'):          # a non-finite value: set to 0, its ray weighs nothing
        raw_b, _ = get_recon(bad[1], ct, spec, n, fov, 1.0, method='pwls', weights=(1.0 / sd[1] ** 2).astype(F32), n_iters=2)
    assert np.all(np.isfinite(raw_b))
    # get_recon without the keyword is what it was
    f0, h0 = get_recon(noisy[0], ct, spec, n, fov, 1.0)
    f1, hh1 = get_recon(noisy[0], ct, spec, n, fov, 1.0, method='fbp')
    assert np.array_equal(f0, f1) and np.array_equal(h0, hh1) and np.array_equal(f0, fbp[0])


# ---- 8: guard bands, through the bare C ABI ------------------------------------------------------------------------------------

def arena(hip):
    ar = Arena('cuda', None)
    ar.hip_error_before = hip.dexct_last_hip_error()
    return ar


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 7 * 2 * 53])
def test_guard_bands_precision(hip, K, n):
    cov = covariances(n, K, 91)
    if n > 8:
        spoil(cov, K)
    T = K * (K + 1) // 2
    ar = arena(hip)
    ar.alloc('cov', 8 * n * T).put(cov)
    ar.alloc('w', 4 * n * T)

    def launch():
        assert hip.dexct_cov_precision(ar['cov'].ptr, n, K, 0.5, ar['w'].ptr, sp()) == 0

    got = twice(ar, launch, ['w'])['w'].view(F32).reshape(T, n)
    ref, ok = pr.precision_ref(cov, K, 0.5)
    worst(got[:, ok], ref[:, ok], 2.0 ** -23 * np.abs(ref[:, ok]), f'guarded precision K={K} n={n}')
    assert np.array_equal(got[:, ~ok], ref[:, ~ok].astype(F32))
    assert hip.dexct_last_hip_error() == ar.hip_error_before


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('shape', ['c53', 'c65', 'wide', 'one'])
@pytest.mark.parametrize('offset', [0, 4])
def test_guard_bands_majorizer_and_residual(hip, K, shape, offset):
    """offset 4: every buffer starts 4 bytes past a 256-byte boundary - the single-element path also where the sizes allow
    16-byte accesses"""
    shape = SHAPES[shape]
    b, ax, W, R, T = sino_inputs(shape, K, 92)
    n_views, line = shape[0], shape[1] * shape[2]
    n = n_views * line
    ar = arena(hip)
    for name, a in (('b', b), ('ax', ax), ('w', W), ('R', R)):
        ar.alloc(name, a.nbytes, offset).put(a)
    ar.alloc('m', 4 * K * n, offset)
    ar.alloc('q', 4 * K * n, offset)
    ar.alloc('obj', 8)
    W2, R1, b2, ax2 = W.reshape(T, -1), R.reshape(-1), b.reshape(K, -1), ax.reshape(K, -1)

    def majorizer():
        assert hip.dexct_pwls_majorizer(ar['w'].ptr, ar['R'].ptr, n, K, ar['m'].ptr, sp()) == 0

    got = twice(ar, majorizer, ['m'], scratch=['q', 'obj'])['m'].view(F32).reshape(K, n)
    ref = pr.majorizer_ref(W2, R1, K, F64)
    worst(got, ref, np.stack([(K + 2) * U * sum(np.abs(W2[pr.tri(K, k, l)].astype(F64)) for l in range(K)) * R1 for k in range(K)]),
          f'guarded majoriser K={K} {shape} +{offset}')

    def residual():
        rc = hip.dexct_pwls_residual(ar['b'].ptr, ar['ax'].ptr, ar['w'].ptr, ar['R'].ptr, n, K, n_views, 1, line, ar['q'].ptr,
                                     ar['obj'].ptr, sp())
        assert rc == 0, rc

    got = twice(ar, residual, ['q'], scratch=['m', 'obj'])['q'].view(F32).reshape(K, n)
    ref, ref_obj = pr.residual_ref(b2, ax2, W2, R1, K, F64)
    worst(got, ref, np.where(R1 > 0, pr.residual_bound(b2, ax2, W2, K), 0.0), f'guarded residual K={K} {shape} +{offset}')
    rel_close(float(ar['obj'].get(F64)[0]), ref_obj, 'guarded objective')
    if n_views >= 3:                                                  # a ragged subset: the skipped lines keep the fill
        for byte in (0x00, 0xFF):
            ar.fill(byte, inner=('q', 'obj'))
            rc = hip.dexct_pwls_residual(ar['b'].ptr, ar['ax'].ptr, ar['w'].ptr, ar['R'].ptr, n, K, n_views, 3, line, ar['q'].ptr,
                                         ar['obj'].ptr, sp())
            assert rc == 0
            ar.check()
            on = np.repeat(np.arange(n_views) % 3 == 0, line)
            raw = ar['q'].get().reshape(K, n, 4)
            assert np.all(raw[:, ~on] == byte)
            worst(raw.view(F32).reshape(K, n)[:, on], ref[:, on], np.where(R1 > 0, pr.residual_bound(b2, ax2, W2, K), 0.0)[:, on],
                  'guarded residual step 3')
    assert hip.dexct_last_hip_error() == ar.hip_error_before


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_guard_bands_update(hip, K, grid):
    grid = GRIDS[grid]
    x, g, d, beta, delta = update_inputs(K, grid, 93)
    ar = arena(hip)
    for name, a in (('x', x), ('g', g), ('d', d)):
        ar.alloc(name, a.nbytes).put(a)
    ar.alloc('y', x.nbytes)
    ar.alloc('pen', 8)

    def launch():
        rc = hip.dexct_pwls_update(ar['x'].ptr, ar['g'].ptr, ar['d'].ptr, K, *grid, 1.0, (C.c_double * K)(*beta),
                                   (C.c_double * K)(*delta), 0, ar['y'].ptr, ar['pen'].ptr, sp())
        assert rc == 0, rc

    got = twice(ar, launch, ['y'], scratch=['pen'])['y'].view(F32).reshape(x.shape)
    worst(got, pr.update_ref(x, g, d, beta, delta, False, 1.0, F64), pr.update_bound(x, g, d, beta, delta), f'guarded update K={K} {grid}')
    rel_close(float(ar['pen'].get(F64)[0]), pr.penalty_ref(x, beta, delta), 'guarded penalty')
    # an alias is refused and nothing is written
    for byte in (0x00, 0xFF):
        ar.fill(byte, inner=('y', 'pen'))
        rc = hip.dexct_pwls_update(ar['x'].ptr, ar['g'].ptr, ar['d'].ptr, K, *grid, 1.0, (C.c_double * K)(*beta),
                                   (C.c_double * K)(*delta), 0, ar['x'].ptr, ar['pen'].ptr, sp())
        assert rc == -1
        ar.check()
        assert np.all(ar['y'].get() == byte) and np.all(ar['pen'].get() == byte) and np.array_equal(ar['x'].get(F32), x.reshape(-1))
    assert hip.dexct_last_hip_error() == ar.hip_error_before


# ---- 9: main.py --recon pwls ---------------------------------------------------------------------------------------------------

def test_main_reconstructs_the_basis_images_jointly(hip, tmp_path):
    """One run of main.py on a tiny scan of the bundled pair.  mat{1,2}_recon are the joint reconstruction of the basis sinograms
    with the covariance of the run; recomputed here from the WRITTEN files, which are float32: the weights move by up to
    2^-24 cond(corr) <= ~500 x 6e-8 = 3e-5 relative and the sinograms by 6e-8, and two iterations from the same FBP images pass
    at most that on - 1e-3 of the largest pixel is what the comparison can ask.  The single-energy images stay FBP."""
    import json
    import os
    import subprocess
    import sys
    from conftest import INPUT, ROOT
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd.back_project import get_basismat_recon, get_recon
    params = json.load(open(os.path.join(INPUT, 'params.txt')))
    params.update({'RUN_ID': 'tiny', 'Nx': 48, 'Ny': 48, 'dx': 0.4, 'dy': 0.4, 'N_channels': 96, 'N_projections': 60,
                   'back_project': True, 'N_recon_matrix': 32, 'FOV_recon': 20.0})
    pf = tmp_path / 'params.txt'
    pf.write_text(json.dumps(params))
    main = os.path.join(ROOT, 'dex-ct-sim_amd', 'main.py')
    subprocess.run([sys.executable, main, '--params', str(pf), '--input-dir', INPUT, '--pairs', '140kV:80kV:5:5', '--n-iters', '30',
                    '--out', str(tmp_path / 'o'), '--covariance', '--recon', 'pwls', '--recon-iters', '2', '--recon-subsets', '2',
                    '--recon-beta', '1e7', '--recon-delta', '0.01'], check=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    run = dx.read_parameter_file(str(pf), base_dir=os.path.dirname(INPUT))[0]
    ct, (n, fov, ramp) = run[3], run[6:9]
    d = tmp_path / 'o' / 'tiny' / 'matdecomp_140kV_80kV_5000uGy_5000uGy'
    shape = (ct.N_proj, ct.N_channels)
    a = [np.fromfile(d / f'mat{m}_sino_float32.bin', dtype=F32).reshape(shape) for m in (1, 2)]
    cov = np.stack([np.fromfile(d / f'cov{t}_sino_float32.bin', dtype=F32).reshape(shape) for t in ('11', '12', '22')], -1)
    got = [np.fromfile(d / f'mat{m}_recon_float32.bin', dtype=F32).reshape(n, n) for m in (1, 2)]
    ref = get_basismat_recon(a, cov.astype(F64), ct, n, fov, ramp, 1e7, 0.01, n_iters=2, n_subsets=2)
    import dex_ct_sim_amd.main as m
    spec = m.load_spectrum(ct, '140kV', 5.0, INPUT)
    for k in range(2):
        err, top = float(np.max(np.abs(got[k] - ref[k]))), float(np.max(np.abs(ref[k])))
        print(f'basis image {k + 1}: |main.py - get_basismat_recon| {err:.3e} of {top:.3e}')
        assert err <= 1e-3 * top
        assert not np.array_equal(got[k], get_recon(a[k], ct, spec, n, fov, ramp)[0])        # not the FBP image
    s = tmp_path / 'o' / 'tiny' / '140kV_5000uGy'
    log = np.fromfile(s / 'sino_log_float32.bin', dtype=F32).reshape(shape)
    assert np.array_equal(np.fromfile(s / 'recon_raw_float32.bin', dtype=F32).reshape(n, n), get_recon(log, ct, spec, n, fov, ramp)[0])
