"""The capped grids of the element-wise kernels, and the problems that run them past their caps.

Ten entry points launch a bounded number of workgroups and cover the rest of their input in a grid-stride loop.  ``CAPS`` names the
``constexpr`` of every cap in csrc/*.hip with its value (tests/test_grid_caps.py reads the sources and compares), ``ROWS`` derives
the work items of one pass from it, and every test size below is derived from that: a later change of a cap fails on the CPU
instead of silently taking the GPU tests (tests/test_gpu_grid_passes.py) back inside one pass.

A work item is what one thread handles per pass: V neighbouring values (V = 4 on the float4 paths, 16 bytes in dexct_volume_ids,
4 bytes in dexct_volume_remap).  One pass is W = blocks x lanes work items (x 2 on the float4 path of dexct_bhc_linearize, whose
loop body holds two loads ``i`` and ``i + stride``).  Sizes: A lands a handful of work items in pass 2, ragged; B lands in pass 3.

Every problem is built from the generators, references and bounds the per-kernel modules already use (tests/test_gpu_pwls.py,
tests/pwls_refs.py, LinearizationTable.evaluate); only the two SIRT steps, which had no value test, get their reference here.
A ``Problem`` holds the inputs, the float64 reference with its bound, the reference of every reduction and ``pos``, the offset of
each work item's first value in launch order.  ``check_values`` / ``check_sum`` are the comparisons of the GPU module;
``plant_missing`` and ``plant_late`` make the two wrong results those comparisons must reject (tests/test_grid_caps.py):
the second pass missing - values from work item W onwards keep what the buffer held, their terms are left out of the sums - and
the second pass reading its inputs one work item late.
"""
import functools
import os
import re

import numpy as np

import pwls_refs as pr
from pwls_refs import F32, F64, U
from test_gpu_pwls import covariances, rel_close, sino_inputs, spoil, update_inputs, worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc')

# constant -> (source file, value)
CAPS = {
    'kPwlsMaxBlocks': ('pwls.hip', 4096),
    'kElementwiseMaxBlocks': ('iterative.hip', 4096),
    'kVolumeIdsMaxBlocks': ('plan.hip', 4096),
    'kVolumeRemapMaxBlocks': ('plan.hip', 8192),
    'kBhcGroupsPerCu': ('bhc.hip', 2),
    'kBhcBlock': ('bhc.hip', 1024),
    'kReduceMaxBlocks': ('gn.hip', 2048),
}
NOMINAL_CUS = 256          # an MI355X, and what the library assumes when the query fails: used where no device is present

# (entry point, path) -> (constant, lanes per workgroup, work items per lane and pass, values per work item, per CU?)
ROWS = {
    ('dexct_cov_precision', ''): ('kPwlsMaxBlocks', 256, 1, 1, False),
    ('dexct_pwls_majorizer', 'float4'): ('kPwlsMaxBlocks', 256, 1, 4, False),
    ('dexct_pwls_majorizer', 'scalar'): ('kPwlsMaxBlocks', 256, 1, 1, False),
    ('dexct_pwls_residual', 'float4'): ('kPwlsMaxBlocks', 256, 1, 4, False),
    ('dexct_pwls_residual', 'scalar'): ('kPwlsMaxBlocks', 256, 1, 1, False),
    ('dexct_pwls_update', ''): ('kPwlsMaxBlocks', 256, 1, 1, False),
    ('dexct_sirt_residual', ''): ('kElementwiseMaxBlocks', 256, 1, 1, False),
    ('dexct_sirt_update', ''): ('kElementwiseMaxBlocks', 256, 1, 1, False),
    ('dexct_volume_ids', ''): ('kVolumeIdsMaxBlocks', 256, 1, 16, False),
    ('dexct_volume_remap', ''): ('kVolumeRemapMaxBlocks', 256, 1, 4, False),
    ('dexct_bhc_linearize', 'float4'): ('kBhcGroupsPerCu', 1024, 2, 4, True),
    ('dexct_bhc_linearize', 'scalar'): ('kBhcGroupsPerCu', 1024, 1, 1, True),
    ('dexct_reduce_max', ''): ('kReduceMaxBlocks', 256, 1, 1, False),      # tests/test_gpu_bounds.py runs it at 2048 * 256 + 1
}


def source_constants():
    """{name: value} of every ``constexpr int kName = VALUE;`` line of the files CAPS names."""
    found = {}
    for f in sorted({f for f, _ in CAPS.values()}):
        for m in re.finditer(r'^\s*constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;', open(os.path.join(CSRC, f)).read(), re.M):
            found[m.group(1)] = (f, int(m.group(2)))
    return found


def n_cu():
    """The compute units of the device the library runs on (it queries the same attribute); NOMINAL_CUS without one."""
    import torch
    if torch.cuda.is_available():
        return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    return NOMINAL_CUS


def pass_items(entry, path=''):
    """(W, V): the work items of one pass and the values of one work item."""
    const, lanes, per_lane, width, per_cu = ROWS[(entry, path)]
    blocks = CAPS[const][1] * (n_cu() if per_cu else 1)
    if entry == 'dexct_bhc_linearize':
        assert lanes == CAPS['kBhcBlock'][1]
    return blocks * lanes * per_lane, width


# ---- problems ------------------------------------------------------------------------------------------------------------------

class Problem:
    """One call past its cap.  ref, bound: [planes, P] float64 (bound None: exact); written: [P] mask of the values the call
    writes (None: all); pos: [items] offset inside a plane of each work item's first value, in launch order; sums: name ->
    (reference, without the terms of work items >= W, with the terms of work items > W in the place of those >= W)."""
    dtype = F32
    written = None
    bound = None
    sums = {}

    def good(self, keep=None):
        """the reference rounded once to the output's type; the values outside ``written`` are those of ``keep``"""
        got = self.ref.astype(self.dtype)
        if self.written is not None and keep is not None:
            got[:, ~self.written] = keep.reshape(self.ref.shape)[:, ~self.written]
        return got

    def fill(self, byte):
        """a buffer of the output's shape as the fill leaves it"""
        return np.full(self.ref.shape, byte, np.uint8).repeat(np.dtype(self.dtype).itemsize, -1).view(self.dtype)

    def compare(self, got, ref, bound, what):
        if bound is None:
            assert np.array_equal(got, ref.astype(self.dtype)), what
        else:
            worst(got, ref, bound, what)

    def check_values(self, got, keep=None, what=''):
        """got: the output buffer, any shape; keep: what the values outside ``written`` must still hold, byte for byte"""
        got = got.reshape(self.ref.shape)
        w = self.written
        if w is None:
            return self.compare(got, self.ref, self.bound, f'{self.label} {what}')
        self.compare(got[:, w], self.ref[:, w], None if self.bound is None else self.bound[:, w], f'{self.label} {what}')
        bits = np.dtype(f'u{np.dtype(self.dtype).itemsize}')
        assert np.array_equal(got[:, ~w].view(bits), keep.reshape(self.ref.shape)[:, ~w].view(bits)), f'{self.label}: other values changed'

    def check_sum(self, name, got):
        rel_close(float(got), self.sums[name][0], f'{self.label} {name}')

    def elements(self, items):
        return (items[:, None] + np.arange(self.V)).reshape(-1)

    def plant_missing(self, keep):
        got = self.good(keep)
        e = self.elements(self.pos[self.W:])
        got[:, e] = keep.reshape(self.ref.shape)[:, e]
        return got

    def plant_late(self, keep):
        """work item i >= W holds the result of item i + 1; the last one, whose inputs would lie past the end, what the buffer held"""
        good, got = self.good(keep), self.good(keep)
        dst, src = self.pos[self.W:-1], self.pos[self.W + 1:]
        for e in range(self.V):
            got[:, dst + e] = good[:, src + e]
        last = self.elements(self.pos[-1:])
        got[:, last] = keep.reshape(self.ref.shape)[:, last]
        return got


SINO_CHUNK = 1 << 19


@functools.lru_cache(maxsize=1)
def big_sino_inputs(K, n):
    """sino_inputs for n rays as chunks of 2^19 (the 3 x 3 inverses of one chunk fit any machine): b, ax [K, n], W [T, n], R [n]"""
    parts = [sino_inputs((min(SINO_CHUNK, n - o),), K, 1000 + o // SINO_CHUNK) for o in range(0, n, SINO_CHUNK)]
    b, ax, W, R = (np.concatenate([p[i] for p in parts], axis=-1) for i in range(4))
    for a in (b, ax, W, R):
        a.setflags(write=False)
    return b, ax, W, R


SINO_RAYS = 2050 * 2052        # the largest sinogram below; the others are its first n rays


def sino_slice(K, n, live):
    """The first n rays of big_sino_inputs.  The generator gives one ray in seven R = 0 and one in ten W = 0; ray ``live``, the
    first of pass 2, must be neither (a result of 0 there could not tell a missing pass from the 0x00 fill): it gets R = 1.5
    and the weights of the first ray that has any."""
    assert live < n <= SINO_RAYS
    b, ax, Wt, R = (a[..., :n].copy() for a in big_sino_inputs(K, SINO_RAYS))
    R[live] = 1.5
    Wt[:, live] = Wt[:, np.flatnonzero(Wt[0] != 0)[0]]
    return b, ax, Wt, R


class Precision(Problem):
    entry, path, w_fill = 'dexct_cov_precision', '', 0.5

    def __init__(self, K, n_of):
        self.W, self.V = pass_items(self.entry)
        self.K, self.n = K, n_of(self.W)
        self.label = f'precision K={K} n={self.n}'
        n, W = self.n, self.W
        self.cov = covariances(n, K, 31 + K)
        bad = spoil(self.cov, K)
        if n >= W + 8:                                                # every unusable kind again, in pass 2
            bad += [W + i for i in spoil(self.cov[W:], K)]
        ref, self.ok = pr.precision_ref(self.cov, K, self.w_fill)
        assert list(np.flatnonzero(~self.ok)) == bad
        self.ref, self.bound = ref, np.where(self.ok, 2.0 ** -23 * np.abs(ref), 0.0)   # unusable rays: exactly w_fill / 0
        self.pos = np.arange(n, dtype=np.int64)


class Majorizer(Problem):
    entry = 'dexct_pwls_majorizer'

    def __init__(self, K, path, n_of, offset=0):
        self.path, self.K, self.offset = path, K, offset
        self.W, self.V = pass_items(self.entry, path)
        self.n = n = n_of(self.W)
        assert (n % 4 == 0 and offset == 0) == (path == 'float4')
        self.label = f'majoriser K={K} n={n} +{offset}'
        self.pos = np.arange(n // self.V, dtype=np.int64) * self.V
        _, _, self.Wt, self.R = sino_slice(K, n, self.pos[self.W])
        self.ref = pr.majorizer_ref(self.Wt, self.R, K, F64)
        self.bound = np.stack([(K + 2) * U * sum(np.abs(self.Wt[pr.tri(K, k, l)].astype(F64)) for l in range(K)) * self.R for k in range(K)])
        assert np.all(self.ref[:, self.pos[self.W]] > 0)


class Residual(Problem):
    entry = 'dexct_pwls_residual'
    SHAPES = {'float4': (2052, 2050, 1), 'scalar': (1027, 3075, 3)}      # line, n_lines, step

    def __init__(self, K, path):
        self.path, self.K = path, K
        self.W, self.V = pass_items(self.entry, path)
        self.line, self.n_lines, self.step = line, n_lines, step = self.SHAPES[path]
        assert (line % 4 == 0) == (path == 'float4')
        self.plane = plane = n_lines * line
        self.label = f'residual K={K} {path}'
        self.written = on = np.repeat(np.arange(n_lines) % step == 0, line)
        lv, n_sub = line // self.V, (n_lines + step - 1) // step
        i = np.arange(n_sub * lv, dtype=np.int64)
        self.pos = (i // lv) * step * line + (i % lv) * self.V
        assert len(self.pos) > self.W and np.array_equal(np.sort(self.elements(self.pos)), np.flatnonzero(on))
        assert self.pos[self.W] % line not in (0, line - self.V)     # the pass boundary lies inside a line
        self.b, self.ax, self.Wt, self.R = b, ax, Wt, R = sino_slice(K, plane, self.pos[self.W])
        self.ref, self.bound = np.zeros((K, plane)), np.zeros((K, plane))
        self.ref[:, on], obj = pr.residual_ref(b[:, on], ax[:, on], Wt[:, on], R[on], K, F64)
        self.bound[:, on] = np.where(R[on] > 0, pr.residual_bound(b[:, on], ax[:, on], Wt[:, on], K), 0.0)
        first = self.elements(self.pos[:self.W])
        late = np.concatenate([first, self.elements(self.pos[self.W + 1:])])
        self.sums = {'objective': (obj,) + tuple(pr.residual_ref(b[:, s], ax[:, s], Wt[:, s], R[s], K, F64)[1] for s in (first, late))}
        assert np.any(R[on] == 0) and np.any(self.ref != 0)


class Update(Problem):
    entry, path, g_scale = 'dexct_pwls_update', '', 3.0

    def __init__(self, K, nz, nonneg):
        self.W, self.V = pass_items(self.entry)
        self.K, self.nonneg = K, nonneg
        self.grid = grid = (nz, 509, 1031)
        self.n = n = int(np.prod(grid))
        self.label = f'update K={K} {grid} nonneg={nonneg}'
        self.x, self.g, self.d, self.beta, self.delta = x, g, d, beta, delta = update_inputs(K, grid, 51 + K)
        z, y, x0 = np.unravel_index(self.W, grid)
        assert n > self.W and y == grid[1] - 1 and 0 < x0 < grid[2] - 1       # the pass boundary: inside the last row of a slice
        self.ref = pr.update_ref(x, g, d, beta, delta, nonneg, self.g_scale, F64).reshape(K, n)
        self.bound = pr.update_bound(x, g, d, beta, delta, self.g_scale).reshape(K, n)
        self.stay = np.stack([d[k].astype(F64) + pr.penalty_terms(x[k].astype(F64), beta[k], delta[k], F64)[1] == 0 for k in range(K)])
        self.stay = self.stay.reshape(K, n)
        self.bound[self.stay] = 0.0                                   # pixels with d + c = 0 stay exactly
        assert self.stay[-1].any() or K == 1
        self.pos = np.arange(n, dtype=np.int64)
        # the penalty of the pixels from W on: the rest of that last row (pairs to the right only) and the slices after it; of
        # pixel W alone: its pair to the right
        pen = pr.penalty_ref(x, beta, delta)
        tail = pr.penalty_ref(x[:, z:z + 1, y:y + 1, x0:], beta, delta) + (pr.penalty_ref(x[:, z + 1:], beta, delta) if z + 1 < nz else 0.0)
        one = pr.penalty_ref(x[:, z:z + 1, y:y + 1, x0:x0 + 2], beta, delta)
        assert tail > 0 and one > 0
        self.sums = {'penalty': (pen, pen - tail, pen - one)}


class SirtResidual(Problem):
    """r = (b - ax) / R where R > 0, else 0, and norm2 = sum (b - ax)^2 / R over those: the float64 formula on the float32
    inputs.  |r - ref| <= 2.02 u |ref|: the subtraction and the division round once each (-ffp-contract=off)."""
    entry, path = 'dexct_sirt_residual', ''

    def __init__(self, line, n_lines, step):
        self.W, self.V = pass_items(self.entry)
        self.line, self.n_lines, self.step = line, n_lines, step
        self.plane = plane = n_lines * line
        self.label = f'sirt residual {line} x {n_lines} : {step}'
        rng = np.random.default_rng(line + 7 * n_lines + step)
        self.b, self.ax = rng.uniform(-1.0, 1.0, plane).astype(F32), rng.uniform(-1.0, 1.0, plane).astype(F32)
        self.R = np.where(rng.uniform(size=plane) < 0.15, 0.0, rng.uniform(0.5, 3.0, plane)).astype(F32)
        self.written = on = np.repeat(np.arange(n_lines) % step == 0, line)
        i = np.arange(int(on.sum()), dtype=np.int64)
        self.pos = (i // line) * step * line + i % line
        if plane > 1:
            self.R[1] = 0.0
        if len(self.pos) > self.W:
            self.R[self.pos[self.W]] = 2.0                            # the ray whose term ``late`` drops is there
        hit = on & (self.R > 0)
        d = self.b.astype(F64) - self.ax.astype(F64)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.ref = np.where(hit, d / self.R.astype(F64), 0.0)[None]
            term = np.where(hit, d * d / self.R.astype(F64), 0.0)
            self.f32 = np.where(hit, (self.b - self.ax) / self.R, F32(0))[None]      # the kernel's order in float32 NumPy
        self.bound = 2.02 * U * np.abs(self.ref)
        first, late = self.pos[:self.W], np.concatenate([self.pos[:self.W], self.pos[self.W + 1:]])
        self.sums = {'norm2': (float(term.sum()), float(term[first].sum()), float(term[late].sum()))}


class SirtUpdate(Problem):
    """x' = x + relax (g / C) where C > 0, else x; max(x', 0) if nonneg.  |x' - ref| <= 1.01 u (|ref| + 2 |relax g / C|): the
    division, the product and the addition round once each.  relax = 0.75 is a float32 number."""
    entry, path, relax = 'dexct_sirt_update', '', 0.75

    def __init__(self, n, nonneg):
        self.W, self.V = pass_items(self.entry)
        self.n, self.nonneg = n, nonneg
        self.label = f'sirt update n={n} nonneg={nonneg}'
        rng = np.random.default_rng(n)
        self.x, self.g = rng.uniform(-0.5, 1.0, n).astype(F32), rng.uniform(-1.0, 1.0, n).astype(F32)
        self.C = np.where(rng.uniform(size=n) < 0.2, 0.0, rng.uniform(0.5, 40.0, n)).astype(F32)
        self.C[0], self.C[-1] = 0.0, 1.5                              # (n = 1: no pixel stays)
        self.stay = self.C == 0
        with np.errstate(divide='ignore', invalid='ignore'):
            step = np.where(self.stay, 0.0, self.relax * (self.g.astype(F64) / self.C.astype(F64)))
            f32 = np.where(self.stay, self.x, self.x + F32(self.relax) * (self.g / self.C))
        ref = self.x.astype(F64) + step
        self.ref = (np.maximum(ref, 0.0) if nonneg else ref)[None]
        self.f32 = (np.maximum(f32, F32(0)) if nonneg else f32)[None]
        self.bound = np.where(self.stay, 0.0, 1.01 * U * (np.abs(ref) + 2.0 * np.abs(step)))[None]   # pixels with C = 0 stay exactly
        self.pos = np.arange(n, dtype=np.int64)


REMAP_LUT = ((np.arange(256) * 5 + 3) % 256).astype(np.uint8)          # a permutation without a fixed point


class Volume(Problem):
    """dexct_volume_ids (a histogram: ``counts`` and its two planted versions) and dexct_volume_remap (in place) on one volume
    with all 256 ids: 250 .. 252 only in the first work item of pass 2, 253 .. 255 only in the scalar tail."""
    dtype, path = np.uint8, ''

    def __init__(self, entry, n_of):
        self.entry = entry
        self.W, self.V = pass_items(entry)
        self.n = n = n_of(self.W * self.V)
        self.label = f'{entry} n={n}'
        V, body = self.V, n // self.V * self.V
        rng = np.random.default_rng(n)
        self.vol = vol = rng.integers(0, 250, n, dtype=np.uint8)
        assert n - body >= 3 and body > (self.W + 1) * V
        vol[self.W * V:self.W * V + 3] = (250, 251, 252)
        vol[body:body + 3] = (253, 254, 255)
        self.pos = np.arange(n // V, dtype=np.int64) * V
        self.ref = REMAP_LUT[vol][None]
        count = lambda a: np.bincount(a, minlength=256).astype(np.uint64)
        self.counts = count(vol)
        self.counts_missing = count(np.concatenate([vol[:self.W * V], vol[body:]]))
        self.counts_late = count(np.concatenate([vol[:self.W * V], vol[(self.W + 1) * V:]]))
        assert np.all(self.counts > 0) and np.all(self.counts_missing[250:253] == 0)

    def check_counts(self, got):
        assert np.array_equal(got, self.counts), self.label


@functools.lru_cache(maxsize=None)
def bhc_table():
    """the table of tests/test_gpu_bounds.py's dexct_bhc_linearize test"""
    from dex_ct_sim_amd import bhc
    E = np.linspace(10.0, 140.0, 131)
    w = np.exp(-((E - 60.0) / 30.0) ** 2)
    mu = 0.2 + 3.0 * (E / 20.0) ** -3
    return bhc.build_table(w, mu, 'water')


class Bhc(Problem):
    """Tolerance and NaN pattern of tests/test_gpu_bounds.py::test_bhc_linearize.  NaN, +-0 and values beyond the last node of
    both sides stand at the start and again from the first value of pass 2."""
    entry = 'dexct_bhc_linearize'
    OFFSETS = {'float4': (4, 4), 'scalar': (0, 4)}                     # bytes added to p and to out

    def __init__(self, path, n_of):
        self.path = path
        self.W, self.V = pass_items(self.entry, path)
        self.table = t = bhc_table()
        self.n = n = n_of(self.W * self.V)
        self.label = f'bhc {path} n={n}'
        self.head = head = (16 - self.OFFSETS[path][0]) % 16 // 4 if path == 'float4' else 0
        rng = np.random.default_rng(n)
        self.p = p = (rng.standard_normal(n) * 3.0).astype(F32)
        lo, hi = t.p_range
        special = np.array([-0.5, np.nan, 0.0, -0.0, 1.5 * hi, 1.5 * lo], F32)
        for at in (1, head + self.W * self.V):
            m = min(len(special), n - at)
            p[at:at + m] = special[:m]
        self.ref = t.evaluate(p)[None]
        self.pos = head + np.arange((n - head) // self.V, dtype=np.int64) * self.V
        assert len(self.pos) > self.W

    def compare(self, got, ref, bound, what):
        fin = np.isfinite(ref)
        with np.errstate(invalid='ignore'):
            over = np.max(np.abs(got[fin] - ref[fin]) - 4e-7 * np.abs(ref[fin]), initial=0.0)
            print(f'{what}: worst |error| - 4e-7 |ref| = {over:.3e} (allowed 1e-9), '
                  f'worst error / (4e-7 |ref| + 1e-9) {np.max(np.abs(got[fin] - ref[fin]) / (4e-7 * np.abs(ref[fin]) + 1e-9)):.3f}')
        assert over <= 1e-9 and np.array_equal(np.isnan(got), np.isnan(ref)), what


# ---- the cases: (id, constructor) ------------------------------------------------------------------------------------------------

def _cases():
    c = {}
    for K in (1, 2, 3):
        c[f'precision-K{K}-A'] = functools.partial(Precision, K, lambda W: W + 1)                      # n = W + 1
        c[f'precision-K{K}-A9'] = functools.partial(Precision, K, lambda W: W + 9)                     # W + 9: the unusable kinds in pass 2
    c['precision-K2-B'] = functools.partial(Precision, 2, lambda W: 2 * W + 259)                          # 2 W + 259
    for K in (1, 2, 3):                                                                 # grouped by K: one set of inputs per K
        c[f'majorizer-K{K}-float4-A'] = functools.partial(Majorizer, K, 'float4', lambda W: 4 * W + 4)
        c[f'majorizer-K{K}-scalar-A'] = functools.partial(Majorizer, K, 'scalar', lambda W: W + 1)
        if K == 2:
            c['majorizer-K2-scalar-offset4-A'] = functools.partial(Majorizer, 2, 'scalar', lambda W: W + 4, 4)
        c[f'residual-K{K}-float4-A'] = functools.partial(Residual, K, 'float4')
        c[f'residual-K{K}-scalar-A'] = functools.partial(Residual, K, 'scalar')
    for nonneg in (False, True):
        for K in (1, 2, 3):
            c[f'update-K{K}-nonneg{int(nonneg)}-A'] = functools.partial(Update, K, 2, nonneg)
        c[f'update-K2-nonneg{int(nonneg)}-B'] = functools.partial(Update, 2, 5, nonneg)
    c['sirt_residual-step3-A'] = functools.partial(SirtResidual, 1027, 3075, 3)
    c['sirt_residual-step1-A'] = functools.partial(SirtResidual, 1027, 1022, 1)
    for nonneg in (False, True):
        c[f'sirt_update-nonneg{int(nonneg)}-A'] = functools.partial(SirtUpdate, pass_items('dexct_sirt_update')[0] + 1, nonneg)
        c[f'sirt_update-nonneg{int(nonneg)}-B'] = functools.partial(SirtUpdate, 2 * pass_items('dexct_sirt_update')[0] + 259, nonneg)
    c['volume_ids-A'] = functools.partial(Volume, 'dexct_volume_ids', lambda W: W + 4099)
    c['volume_ids-B'] = functools.partial(Volume, 'dexct_volume_ids', lambda W: 2 * W + 16 * 257 + 5)
    c['volume_remap-A'] = functools.partial(Volume, 'dexct_volume_remap', lambda W: W + 4099)
    c['volume_remap-B'] = functools.partial(Volume, 'dexct_volume_remap', lambda W: 2 * W + 4 * 257 + 3)
    c['bhc-float4-A'] = functools.partial(Bhc, 'float4', lambda W: W + 8197)             # W values: C * 8192
    c['bhc-float4-B'] = functools.partial(Bhc, 'float4', lambda W: 2 * W + 12301)
    c['bhc-scalar-A'] = functools.partial(Bhc, 'scalar', lambda W: W + 1)                # C * 1024
    c['bhc-scalar-B'] = functools.partial(Bhc, 'scalar', lambda W: 3 * W + 77)
    return c


CASES = _cases()


def cases(prefix):
    return [k for k in CASES if k.startswith(prefix + '-')]


# the small direct cases of the two SIRT steps: (line, n_lines, step); step 3 takes lines 0, 3 and 6
SIRT_SMALL = [(line, 1 if step == 1 else 7, step) for line in (1, 63, 64, 65, 257) for step in (1, 3)]
