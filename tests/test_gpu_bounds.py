"""Guard-banded bounds tests of the Newton family and the element-wise kernels through the bare C ABI (tests/guarded.py).

Every buffer a launch is given sits between two 64 KiB guards.  Each case runs twice - guards, outputs and workspace filled with
0x00, then with 0xFF (NaN in float32 and float64) - and must leave every guard unchanged, end without a HIP error and give
bit-identical outputs: a write past a buffer, a read past an input, a read of workspace that was not written first or an
output byte left unwritten would each show.  Values are checked as well, against a NumPy reference of the same operation.

Outcome when this module was written: no guard and no read check fired, on any launch form of dexct_gn_decompose
(gn_refill_kernel<false> / <true>, gn_coop_kernel, gn_kernel<false, true> and <true, false>, gn_shortcut_kernel<1> / <2>, the
gn_tile_key / scan / scatter hand-out), on the model sums, the mask, the maximum, or the element-wise and transpose kernels.
The gate calibration (matdecomp.calibrate_gate, replayed on guarded buffers through its ``alloc`` argument) gives the same gate
bit for bit.  Each launch of matdecomp._walk on a table of n_e energies and n counts (n = 385^2 = 148 225 grid corners, then
384^2 = 147 456 cell centres) is given, and stays inside:
  g: 16 n bytes (two float64 rows), a: 16 n, iterations: n, workspace: dexct_gn_workspace_bytes(n_e, 1) =
  16 * ceil((128 + 172 n_e) / 16) + 8192 + 196 608 bytes, i.e. 205 104 / 205 280 / 205 456 bytes for n_e = 1 / 2 / 3 (the
  128-byte header, the 14-double and 14-float tables and the permutation per energy, then the tile-order region of the sort,
  which the counting pass does not use).
So the intermittent aborts of round 6 during gate calibration on 1 - 3 energy tables are not explained by an overrun of these
launches.  The next suspect is the host heap: dexct_host_touch as it was before commit c3f0e6e, which this module does not test.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from guarded import Arena, twice

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


def ok(rc):
    assert rc == 0, rc


def err(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))


# ---- problems ----------------------------------------------------------------------------------------------------------------

def tables(n_e, seed, n_bins=1, empty=False, clipped=False):
    """Random well-posed tables (the recipe of test_gpu_gn.test_random_tables_against_numpy_oracle): i0 [2, n_bins, n_e],
    mus [2, n_e].  ``empty``: energies only one spectrum weights and one nobody weights; ``clipped``: some mu far above 4."""
    rng = np.random.default_rng(seed)
    E = np.linspace(15.0, 150.0, n_e) if n_e > 1 else np.array([60.0])
    pa, pb = rng.uniform(0.1, 0.4, 2), rng.uniform(0.1, 0.2, 2)
    pp = np.array([rng.uniform(0.2, 1.0), rng.uniform(2.0, 3.2)])
    mus = pa[:, None] * (E[None, :] / 60.0) ** (-pp[:, None]) + pb[:, None]
    if clipped:
        mus[:, : n_e // 8 + 1] *= 30.0
    i0 = rng.uniform(0.2, 1.0, (2, n_bins, n_e)) * rng.uniform(1e3, 1e6)
    if empty and n_e > 6:
        lo, hi = sorted(rng.integers(1, n_e - 1, 2))
        i0[0, :, lo:hi // 2 + 1] = 0.0                                      # only spectrum 1 weights these
        i0[1, :, hi:] = 0.0                                                 # only spectrum 0
        i0[:, :, n_e // 2] = 0.0                                            # nobody
        i0[:, :, -1] = np.maximum(i0[:, :, -1], 1.0)
        i0[:, :, 0] = np.maximum(i0[:, :, 0], 1.0)
    return i0, mus


def pixel_i0(i0, n_pix, bin_div):
    """[2, n_pix, n_e]: the spectrum row each pixel uses, (p / bin_div) % n_bins."""
    return i0[:, (np.arange(n_pix) // bin_div) % i0.shape[1], :]


def counts(i0, mus, n_pix, seed, bin_div=1, noise=1e-3):
    rng = np.random.default_rng(seed + 7)
    a = np.stack([rng.uniform(0, 30, n_pix), rng.uniform(0, 5, n_pix)], -1)
    ip = pixel_i0(i0, n_pix, bin_div)
    att = np.exp(-(a[:, :1] * mus[0] + a[:, 1:] * mus[1]))                  # [p, e]
    return np.einsum('kpe,pe->kp', ip, att) * (1 + noise * rng.standard_normal((2, n_pix)))


def oracle_check(got, g, i0, mus, n_iters, bin_div=1, sample=None, tol=1e-7):
    """got [n_pix, 2] against gn_oracle.newton_solve, with the perturbation screen of test_random_tables_against_numpy_oracle;
    ``sample``: pixel indices to compare (the oracle stays cheap on the 2-million-pixel cases)."""
    from oracle import gn_oracle
    idx = np.arange(g.shape[1]) if sample is None else sample
    ip = pixel_i0(i0, g.shape[1], bin_div)[:, idx]
    gs = g[:, idx][:, None, :]
    with np.errstate(all='ignore'):
        ref = gn_oracle.newton_solve(gs, ip, mus, n_iters)[0]
        ref_p = gn_oracle.newton_solve(gs * (1 + 1e-13), ip, mus, n_iters)[0]
    stable = np.isfinite(ref).all(-1) & (np.abs(ref).max(-1) < 1e6)
    with np.errstate(all='ignore'):
        stable &= np.abs(ref - ref_p).max(-1) <= 1e-10 * np.maximum(np.abs(ref).max(-1), 1.0)
    if i0.shape[-1] >= 3:
        assert stable.mean() > 0.5, stable.mean()
    if stable.any():
        assert err(got[idx][stable], ref[stable]) < tol, err(got[idx][stable], ref[stable])
    return stable


# ---- dexct_gn_decompose on guarded buffers -----------------------------------------------------------------------------------

def gn_guarded(lib, g, i0, mus, n_iters, *, f32=False, mask_max=None, mask_frac=0.95, bin_div=1, precision=0, n_polish=3,
               stop_tol=None, out_rc=(0, 0), kernel=1, gn_pass=0, start=None, flags=0):
    """One dexct_gn_decompose with every buffer guarded (g1, g2, i0, mus, mask_max, out_a, iterations, start, workspace of
    exactly dexct_gn_workspace_bytes(n_e, n_bins)), run with both fills.  Returns (out_a [n_pix, 2], iterations or None)."""
    from dex_ct_sim_amd import _native
    from dex_ct_sim_amd._device import stream_ptr
    n_bins, n_e = i0.shape[1], i0.shape[2]
    n_pix = g.shape[1]
    gh = np.ascontiguousarray(g, dtype=F32 if f32 else F64)
    ar = Arena('cuda', lib)
    for k in range(2):
        ar.alloc(f'g{k + 1}', gh[k].nbytes).put(gh[k])
    ar.alloc('i0', i0.nbytes).put(np.ascontiguousarray(i0, dtype=F64))
    ar.alloc('mus', mus.nbytes).put(np.ascontiguousarray(mus, dtype=F64))
    ar.alloc('out_a', 16 * n_pix)
    ar.alloc('workspace', lib.dexct_gn_workspace_bytes(n_e, n_bins))
    outs = ['out_a']
    if mask_max is not None:
        ar.alloc('mask_max', 8).put(np.array([mask_max], dtype=F64))
    if gn_pass == _native.GN_PASS_COUNT:
        ar.alloc('iterations', n_pix)
        outs.append('iterations')
    if start is not None:
        ar.alloc('start', start.numel() * 8).put(start)

    def launch():
        opts = _native.gn_options(stop_tol, out_rc[0], out_rc[1], kernel, gn_pass,
                                  ar['iterations'].ptr if 'iterations' in outs else None,
                                  ar['start'].ptr if start is not None else None, flags)
        rc = lib.dexct_gn_decompose(ar['g1'].ptr, ar['g2'].ptr, int(not f32), n_pix, ar['i0'].ptr, ar['mus'].ptr, n_e, n_bins,
                                    bin_div, n_iters, precision, n_polish, ar['mask_max'].ptr if mask_max is not None else None,
                                    mask_frac, ar['out_a'].ptr, opts, ar['workspace'].ptr, stream_ptr())
        assert rc == 0, rc

    got = twice(ar, launch, outs, scratch=['workspace'])
    a = got['out_a'].view(F64).reshape(n_pix, 2)
    return a, (got['iterations'] if 'iterations' in outs else None)


# (n_e, n_pix, f32, masked, empty classes, clipped, natural order)
PLAIN = [(1, 63, False, False, False, False, False), (2, 64, True, False, False, False, False),
         (3, 65, False, True, False, False, True), (4, 257, True, False, False, False, False),
         (47, 4097, False, False, True, False, False), (48, 1, False, False, False, False, False),
         (49, 4097, True, True, True, True, False), (140, 257, False, False, True, True, True),
         (239, 63, True, True, False, False, False), (4096, 65, False, False, True, True, False)]


@pytest.mark.parametrize('n_e,n_pix,f32,masked,empty,clipped,natural', PLAIN)
def test_refill_kernel_plain_and_cooperative(hip, n_e, n_pix, f32, masked, empty, clipped, natural):
    """gn_refill_kernel<false> (kernel 1, sorted or natural hand-out) and gn_coop_kernel (kernel 2) on ragged sizes, every energy
    class, the clipped class and the largest table the ABI takes: inside their buffers, independent of the fills, equal to each
    other's bits where the exact count is asked, and to the NumPy oracle."""
    from dex_ct_sim_amd import _native
    i0, mus = tables(n_e, n_e * 31 + n_pix, empty=empty, clipped=clipped)
    g = counts(i0, mus, n_pix, n_pix)
    gmax = float(g[0].max()) if masked else None
    if masked:
        g[0, ::5] = 2.0 * gmax                                                   # air: above 0.95 * max
        gmax = float(g[0].astype(F32 if f32 else F64).max())
    flags = _native.GN_FLAG_NATURAL_ORDER if natural else 0
    a, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, kernel=1, flags=flags)
    gg = g.astype(F32).astype(F64) if f32 else g
    live = np.ones(n_pix, bool)
    if masked:
        live = gg[0] < 0.95 * gmax
        assert np.all(a[~live] == 0.0)
    oracle_check(a[live], gg[:, live], i0, mus, 30)
    coop, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, kernel=2, flags=flags)
    if masked:
        assert np.all(coop[~live] == 0.0)
    oracle_check(coop[live], gg[:, live], i0, mus, 30)
    # the exact count (stop_tol = 0): the lane kernel's bits do not depend on the order of the hand-out
    e1, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, kernel=1, stop_tol=0.0)
    e2, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, kernel=1, stop_tol=0.0, flags=_native.GN_FLAG_NATURAL_ORDER)
    assert np.array_equal(e1.view(np.int64), e2.view(np.int64))


@pytest.mark.parametrize('n_pix', [64, 128, 2097152, 2097153])
def test_tile_counts_of_the_sorted_hand_out(hip, n_pix):
    """1, 2, 32768 (= kMaxSortTiles, the largest sorted hand-out: gn_tile_key / scan / scatter fill the tile-order region to its
    end) and 32769 tiles (natural order): a seeded sample of pixels, the first and last tile and any non-finite result
    included, against the oracle."""
    i0, mus = tables(48, 5)
    g = counts(i0, mus, n_pix, 11)
    a, _ = gn_guarded(hip, g, i0, mus, 30, kernel=1)
    rng = np.random.default_rng(n_pix)
    bad = np.flatnonzero(~np.isfinite(a).all(-1))                  # (the oracle must not answer those stably either)
    assert bad.size < 1e-3 * n_pix + 1
    sample = np.unique(np.concatenate([np.arange(min(64, n_pix)), np.arange(max(0, n_pix - 64), n_pix),
                                       rng.integers(0, n_pix, 3000), bad[:200]]))
    oracle_check(a, g, i0, mus, 30, sample=sample)


@pytest.mark.parametrize('V,R,Ch,f32', [(3, 1, 65, False), (7, 3, 5, True), (4, 17, 1, False), (2, 17, 65, True), (1, 3, 1, False)])
def test_transposed_results(hip, V, R, Ch, f32):
    """out_rows / out_channels (4 x 16 tiles collected in LDS, ragged both ways): inside out_a, and the plain order's bits
    transposed - lane kernel, cooperative kernel and the mixed-precision kernel's scattered stores."""
    i0, mus = tables(49, V * R * Ch, empty=True)
    n = V * R * Ch
    g = counts(i0, mus, n, n)
    gmax = float(g[0].astype(F32 if f32 else F64).max())
    for kw in (dict(kernel=1, stop_tol=0.0), dict(kernel=2, stop_tol=0.0), dict(precision=1)):
        plain, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, **kw)
        tr, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, mask_max=gmax, out_rc=(R, Ch), **kw)
        want = plain.reshape(V, Ch, R, 2).transpose(0, 2, 1, 3).reshape(n, 2)
        assert np.array_equal(tr.view(np.int64), want.view(np.int64)), kw


@pytest.mark.parametrize('n_e,n_bins,bin_div,n_pix,f32', [(3, 3, 1, 65, True), (49, 5, 3, 257, False), (140, 2, 7, 4097, False)])
def test_per_bin_kernel(hip, n_e, n_bins, bin_div, n_pix, f32):
    """gn_kernel<false, true>: a spectrum per bin, pixel p on row (p / bin_div) % n_bins; the workspace holds n_bins tables."""
    i0, mus = tables(n_e, n_e + n_bins, n_bins=n_bins, empty=True)
    g = counts(i0, mus, n_pix, 3, bin_div=bin_div)
    a, _ = gn_guarded(hip, g, i0, mus, 30, f32=f32, bin_div=bin_div)
    gg = g.astype(F32).astype(F64) if f32 else g
    oracle_check(a, gg, i0, mus, 30, bin_div=bin_div)


@pytest.mark.parametrize('n_pix,f32,masked', [(65, False, False), (4097, True, True)])
def test_mixed_precision(hip, golden, n_pix, f32, masked):
    """gn_kernel<true, false>: float32 bulk, float64 polish, per-pixel redo; within the north-star 1e-5 of the oracle."""
    i0, mus = golden['gn0_i0'][:, None, :], golden['gn0_mus']
    g = counts(i0, mus, n_pix, 9, noise=3e-3)
    gmax = float(g[0].astype(F32 if f32 else F64).max()) if masked else None
    a, _ = gn_guarded(hip, g, i0, mus, 50, f32=f32, mask_max=gmax, precision=1)
    gg = g.astype(F32).astype(F64) if f32 else g
    live = gg[0] < 0.95 * gmax if masked else np.ones(n_pix, bool)
    oracle_check(a[live], gg[:, live], i0, mus, 50, tol=1e-5)


@pytest.mark.parametrize('n_e,n_pix', [(1, 65), (2, 4097), (3, 63), (140, 4097), (4096, 64)])
def test_counting_pass(hip, n_e, n_pix):
    """gn_refill_kernel<true> with exactly the arguments matdecomp._walk passes (float64 counts, 254 steps, stop_tol 1e-12, lane
    kernel, no mask): step counts in 1..254 or 255, the same bytes under both fills, and results bit-identical to a plain
    launch with the same tolerance (csrc/gn.hip: the same iteration, counting steps)."""
    from dex_ct_sim_amd import _native
    i0, mus = tables(n_e, n_e, empty=True)
    g = counts(i0, mus, n_pix, n_e + 1)
    a, it = gn_guarded(hip, g, i0, mus, 254, stop_tol=1e-12, kernel=1, gn_pass=_native.GN_PASS_COUNT)
    assert it.min() >= 1 and it.max() <= 255
    plain, _ = gn_guarded(hip, g, i0, mus, 254, stop_tol=1e-12, kernel=1)
    assert np.array_equal(a.view(np.int64), plain.view(np.int64))


def _short_cut_problem(golden, n, seed):
    rng = np.random.default_rng(seed)
    i0, mus = golden['gn0_i0'], golden['gn0_mus']
    a_true = np.stack([rng.uniform(0, 40, n) * rng.choice([0.02, 0.3, 1.0], n), rng.uniform(0, 8, n) * rng.choice([0.0, 0.1, 1.0], n)], -1)
    ex = np.exp(-a_true @ mus)
    g = np.stack([(i0[k] * ex).sum(-1) for k in range(2)]) * (1 + 0.002 * rng.standard_normal((2, n)))
    g[:, ::97] = np.nan
    return g, i0[:, None, :], mus


@pytest.mark.parametrize('n,out_rc', [(65, (0, 0)), (4097, (0, 0)), (3 * 17 * 65, (17, 65))])
def test_short_cut_kernels(hip, golden, n, out_rc):
    """gn_shortcut_kernel<2> and <1> (DEXCT_GN_FLAG_ONE_STEP) on the start array of the real gate (power form appended):
    inside their buffers, within 1e-12 of the exact count on every pixel where that is finite, identical where it is not."""
    from dex_ct_sim_amd import _native, matdecomp as md
    g, i0, mus = _short_cut_problem(golden, n, n)
    start = md._device_tables(i0[:, 0], mus, torch.device('cuda'), True)[2]['start']
    assert start is not None
    exact, _ = gn_guarded(hip, g, i0, mus, 50, stop_tol=0.0, kernel=1, out_rc=out_rc)
    ok = np.isfinite(exact).all(-1)
    for flags in (0, _native.GN_FLAG_ONE_STEP):
        a, _ = gn_guarded(hip, g, i0, mus, 50, kernel=1, gn_pass=_native.GN_PASS_SHORTCUT, start=start, flags=flags, out_rc=out_rc)
        assert err(a[ok], exact[ok]) < 1e-12, flags
        assert np.array_equal(a[~ok].view(np.int64), exact[~ok].view(np.int64))


# ---- the gate calibration ----------------------------------------------------------------------------------------------------

def _guarded_alloc(arenas, lib):
    """An ``alloc`` for matdecomp._walk: every buffer a fresh arena's guarded buffer (guards filled with the arena's byte)."""
    def alloc(name, shape, dtype):
        ar = Arena('cuda', lib)
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        b = ar.alloc(name, n)
        ar.fill(arenas['byte'], inner=(name,))
        arenas['list'].append((ar, name, n))
        return b.view(dtype, shape)
    return alloc


def _gate_cases():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from soak_cases import draw
    cases = [(f'soak seed {s}', draw(s)['i0'], draw(s)['mus']) for s in (319, 525, 468, 1179, 4, 29, 126, 397, 1795)]
    for n_e in (1, 2, 3):
        i0, mus = tables(n_e, 40 + n_e)
        cases.append((f'{n_e} energies', i0[:, 0], mus))
    return cases


def test_gate_calibration_replayed_on_guarded_buffers(hip):
    """matdecomp.calibrate_gate - newton_start_grid corners, the counting pass, assemble_start, the centre pass of cell_centres,
    validate_start with the model sums on the device - with the buffers of both counting launches guarded (fills 0x00 and 0xFF,
    workspace and outputs included): no guard changes, and the gate is bit for bit the one calibrate_gate computes on plain
    buffers.  The nine flagged soak seeds and tables of 1, 2 and 3 energies (the round-6 aborts)."""
    from dex_ct_sim_amd import matdecomp as md
    dev = torch.device('cuda')
    extents = {}
    for what, i0, mus in _gate_cases():
        i0_h = np.ascontiguousarray(np.asarray(i0, dtype=F64).reshape(2, -1))
        mus_h = np.ascontiguousarray(mus, dtype=F64)
        i0_d = torch.tensor(i0_h[:, None, :], device=dev).contiguous()
        mus_d = torch.tensor(mus_h, device=dev)
        want = md.calibrate_gate(i0_h, mus_h, i0_d, mus_d, dev, 1e-12)
        for byte in (0x00, 0xFF):
            arenas = {'byte': byte, 'list': []}
            got = md.calibrate_gate(i0_h, mus_h, i0_d, mus_d, dev, 1e-12, alloc=_guarded_alloc(arenas, hip))
            for ar, name, n in arenas['list']:
                ar.check()
            extents[what] = [(name, n) for _, name, n in arenas['list']]
            assert json.dumps(got[1], sort_keys=True) == json.dumps(want[1], sort_keys=True), what
            if want[0] is None:
                assert got[0] is None, what
            else:
                assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)), what
        if want[0] is not None:
            assert len(extents[what]) == 8                                     # two launches of four buffers
    n_e_ws = {n_e: hip.dexct_gn_workspace_bytes(n_e, 1) for n_e in (1, 2, 3)}
    assert n_e_ws == {1: 205104, 2: 205280, 3: 205456}                         # (the module docstring)


# ---- model sums, mask, maximum -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_e', [1, 2, 3, 140])
@pytest.mark.parametrize('n', [1, 255, 256, 5003])
def test_model_sums(hip, n_e, n):
    from dex_ct_sim_amd import quadrature as q
    from dex_ct_sim_amd._device import stream_ptr
    rng = np.random.default_rng(n_e * 7 + n)
    i0, mus = tables(n_e, n_e, clipped=n_e > 4)
    i0 = i0[:, 0]
    a = np.stack([rng.uniform(-5.0, 45.0, n), rng.uniform(-3.0, 8.0, n)], 1)
    a[7::211] *= 100.0
    for third in (False, True):
        ar = Arena('cuda', hip)
        ar.alloc('a', a.nbytes).put(a)
        ar.alloc('i0', i0.nbytes).put(i0)
        ar.alloc('mus', mus.nbytes).put(mus)
        ar.alloc('nu', 16 * n)
        ar.alloc('g', 32 * n)
        outs = ['nu', 'g'] + (['s'] if third else [])
        if third:
            ar.alloc('s', 64 * n)

        def launch():
            assert hip.dexct_gn_model_sums(ar['a'].ptr, n, ar['i0'].ptr, ar['mus'].ptr, n_e, ar['nu'].ptr, ar['g'].ptr,
                                           ar['s'].ptr if third else None, stream_ptr()) == 0

        got = twice(ar, launch, outs)
        want = q._model_sums(dict(i0=i0, mus=mus), a, third=third)
        for name, w in zip(outs, want):
            np.testing.assert_allclose(got[name].view(F64).reshape(w.shape), w, rtol=5e-12, atol=0.0)


MASK_SIZES = [1, 255, 256, 2048 * 256 + 1]


@pytest.mark.parametrize('n', MASK_SIZES)
@pytest.mark.parametrize('f64', [False, True])
def test_apply_mask_and_reduce_max(hip, n, f64):
    """dexct_gn_apply_mask (in place on out_a) and dexct_reduce_max (grid capped at 2048 blocks: the last size is one pixel past
    it) against NumPy; a NaN anywhere, the last pixel included, propagates like np.max."""
    from dex_ct_sim_amd._device import stream_ptr
    rng = np.random.default_rng(n)
    g = rng.uniform(1.0, 100.0, n).astype(F64 if f64 else F32)
    a = rng.standard_normal((n, 2))
    thresh = 0.9 * float(g.max())
    ar = Arena('cuda', hip)
    ar.alloc('g1', g.nbytes)
    ar.alloc('out_a', a.nbytes)
    ar.alloc('max', 8)

    def mask():
        ar['g1'].put(g)
        ar['out_a'].put(a)
        assert hip.dexct_gn_apply_mask(ar['g1'].ptr, int(f64), n, thresh, ar['out_a'].ptr, stream_ptr()) == 0

    got = twice(ar, mask, ['out_a'])['out_a'].view(F64).reshape(n, 2)
    want = np.where((g >= thresh)[:, None], 0.0, a)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    for nan_at in (None, 0, n - 1):
        gx = g.copy()
        if nan_at is not None:
            gx[nan_at] = np.nan

        def reduce():
            ar['g1'].put(gx)
            assert hip.dexct_reduce_max(ar['g1'].ptr, int(f64), n, ar['max'].ptr, stream_ptr()) == 0

        m = twice(ar, reduce, ['max'])['max'].view(F64)[0]
        w = float(np.max(gx))
        assert (np.isnan(m) and np.isnan(w)) or m == w, (nan_at, m, w)


# ---- element-wise and transpose kernels --------------------------------------------------------------------------------------

OFFSETS = [0, 4, 8, 12]


@pytest.fixture(scope='module')
def bhc_table():
    import grid_caps
    return grid_caps.bhc_table()                  # shared with tests/test_gpu_grid_passes.py


@pytest.mark.parametrize('n', list(range(10)) + [4099, 100003])
def test_bhc_linearize(hip, bhc_table, n):
    """dexct_bhc_linearize: float4 body and scalar head / tail at every pair of input / output offsets, in place and out of place,
    against LinearizationTable.evaluate at the tolerance of test_gpu_bhc."""
    from dex_ct_sim_amd._device import stream_ptr
    t = bhc_table
    rng = np.random.default_rng(n)
    p = (rng.standard_normal(n) * 3.0).astype(F32)
    if n > 3:
        p[1], p[2], p[3] = np.nan, 0.0, -0.5
    tab = t.pairs()
    ref = t.evaluate(p)
    fin = np.isfinite(ref)
    lo = Arena('cuda', hip)
    lo.alloc('table', tab.nbytes).put(tab)
    args = (t.log2_min, t.cells_log2, t.oct_pos, t.oct_neg)
    first = None
    for po in OFFSETS:
        for oo in OFFSETS:
            ar = Arena('cuda', hip)
            ar.buffers['table'] = lo['table']
            ar.alloc('p', 4 * n, po).put(p)
            ar.alloc('out', 4 * n, oo)
            got = twice(ar, lambda: ok(hip.dexct_bhc_linearize(ar['p'].ptr, n, ar['table'].ptr, *args, ar['out'].ptr, stream_ptr())),
                        ['out'])['out'].view(F32)
            assert np.max(np.abs(got[fin] - ref[fin]) - 4e-7 * np.abs(ref[fin]), initial=0.0) <= 1e-9
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            if first is None:
                first = got
            assert np.array_equal(got.view(np.int32), first.view(np.int32)), (po, oo)
        ar = Arena('cuda', hip)
        ar.buffers['table'] = lo['table']
        ar.alloc('p', 4 * n, po)

        def in_place():
            ar['p'].put(p)
            assert hip.dexct_bhc_linearize(ar['p'].ptr, n, ar['table'].ptr, *args, ar['p'].ptr, stream_ptr()) == 0

        got = twice(ar, in_place, ['p'])['p'].view(F32)
        assert np.array_equal(got.view(np.int32), first.view(np.int32)), po


def np_log(air, c):
    with np.errstate(divide='ignore'):
        return np.log(np.float32(air)[:, None] / c.astype(F32)).astype(F32)


@pytest.mark.parametrize('n_spectra', [1, 2, 3, 4])
@pytest.mark.parametrize('n_rays', [1, 5, 1023, 4099])
def test_sino_log(hip, n_spectra, n_rays):
    from dex_ct_sim_amd._device import stream_ptr
    rng = np.random.default_rng(n_rays + n_spectra)
    c = (rng.uniform(1e-3, 1e5, (n_spectra, n_rays))).astype(F32)
    air = (C.c_float * n_spectra)(*[3.0e5 / (s + 1) for s in range(n_spectra)])
    want = np_log(np.array(list(air)), c)
    for co, oo in ((0, 0), (4, 4), (8, 0), (0, 12)):
        ar = Arena('cuda', hip)
        ar.alloc('counts', c.nbytes, co).put(c)
        ar.alloc('log', c.nbytes, oo)
        got = twice(ar, lambda: ok(hip.dexct_sino_log(ar['counts'].ptr, air, n_spectra, n_rays, ar['log'].ptr, stream_ptr())),
                    ['log'])['log'].view(F32).reshape(n_spectra, n_rays)
        assert np.allclose(got, want, rtol=5e-6, atol=5e-7), np.abs(got - want).max()


TRANSPOSE = [(1, 1, 2), (3, 4, 3), (4, 4, 2), (63, 65, 1), (65, 129, 2), (129, 3, 1), (4, 64, 3), (128, 64, 1), (4, 3, 65537), (4, 4, 65537)]


@pytest.mark.parametrize('rows,cols,batch', TRANSPOSE)
def test_transposes(hip, rows, cols, batch):
    """dexct_transpose_batched (4, 8, 16-byte elements) and dexct_transpose_log (16-byte path and its generic fall-back; a batch
    of 65537 crosses the 65535 slice of gridDim.z): exact transposes, logs as dexct_sino_log's tolerance."""
    from dex_ct_sim_amd._device import stream_ptr
    rng = np.random.default_rng(rows * cols + batch)
    for eb in (4, 8, 16):
        src = rng.integers(0, 2 ** 31, (batch, rows, cols * eb // 4)).astype(np.int32)
        ar = Arena('cuda', hip)
        ar.alloc('src', src.nbytes).put(src)
        ar.alloc('dst', src.nbytes)
        got = twice(ar, lambda: ok(hip.dexct_transpose_batched(ar['src'].ptr, ar['dst'].ptr, batch, rows, cols, eb, stream_ptr())),
                    ['dst'])['dst']
        want = src.view(np.uint8).reshape(batch, rows, cols, eb).transpose(0, 2, 1, 3)
        assert np.array_equal(got.reshape(batch, cols, rows, eb), want), eb
    S = 2 if batch % 2 == 0 else 1
    per = batch // S
    c = rng.uniform(1e-2, 1e5, (batch, rows, cols)).astype(F32)
    air_v = [3.0e5, 1.5e5][:S]
    air = (C.c_float * S)(*air_v)
    want = c.transpose(0, 2, 1)
    want_log = np_log(np.array(air_v, dtype=F32), want.reshape(S, -1)).reshape(want.shape)
    for off in (0, 4):
        ar = Arena('cuda', hip)
        ar.alloc('src', c.nbytes, off).put(c)
        ar.alloc('dst', c.nbytes)
        ar.alloc('log', c.nbytes)
        got = twice(ar, lambda: ok(hip.dexct_transpose_log(ar['src'].ptr, ar['dst'].ptr, ar['log'].ptr, air, S, per, rows, cols,
                                                            stream_ptr())), ['dst', 'log'])
        assert np.array_equal(got['dst'].view(F32).reshape(want.shape), want)
        lg = got['log'].view(F32).reshape(want.shape)
        assert np.allclose(lg, want_log, rtol=5e-6, atol=5e-7), np.abs(lg - want_log).max()


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 1, 1, 1), (3, 9, 4, 13)])
def test_add_noise(hip, layout, shape):
    """dexct_add_noise in place, n not a multiple of 256, view_offset > 0: inside its buffers and equal to the same call on plain
    tensors."""
    from dex_ct_sim_amd._device import stream_ptr
    S, V, R, Ch = shape
    rng = np.random.default_rng(V * R * Ch)
    cnt = rng.uniform(10.0, 1e4, (S, V * R * Ch)).astype(F32)
    var = (cnt * rng.uniform(0.5, 2.0, cnt.shape)).astype(F32)
    ar = Arena('cuda', hip)
    ar.alloc('counts', cnt.nbytes, 4)
    ar.alloc('variance', var.nbytes, 8).put(var)

    def launch():
        ar['counts'].put(cnt)
        assert hip.dexct_add_noise(ar['counts'].ptr, ar['variance'].ptr, S, V, R, Ch, layout, 17, 1234, stream_ptr()) == 0

    got = twice(ar, launch, ['counts'])['counts'].view(F32)
    plain = torch.tensor(cnt, device='cuda')
    pv = torch.tensor(var, device='cuda')
    assert hip.dexct_add_noise(plain.data_ptr(), pv.data_ptr(), S, V, R, Ch, layout, 17, 1234, stream_ptr()) == 0
    assert np.array_equal(got.view(np.int32), plain.cpu().numpy().reshape(-1).view(np.int32))
    assert not np.array_equal(got, cnt.reshape(-1))


@pytest.mark.parametrize('n_mat', [4, 5, 16, 17, 48, 49])
def test_poisson_detect(hip, n_mat):
    """dexct_poisson_detect across every register-array template (4 / 16 / 48 / 256 materials) with pathlen = 0: lambda equals
    photons, so counts are whole Poisson samples of known mean and variance, and identical under both fills."""
    from dex_ct_sim_amd._device import stream_ptr
    S, n_e, V, R, Ch = 2, 1, 37, 3, 181                                   # 20 091 rays: not a multiple of 256
    lam = np.array([[12.0], [400.0]], dtype=F32)                          # inversion, rounded normal
    n_rays = V * R * Ch
    ar = Arena('cuda', hip)
    ar.alloc('pathlen', 4 * n_rays * n_mat).put(np.zeros(n_rays * n_mat, F32))
    ar.alloc('mu', 4 * n_mat * n_e).put(np.full(n_mat * n_e, 0.3, F32))
    ar.alloc('photons', lam.nbytes).put(lam)
    ar.alloc('gain', 4 * n_e).put(np.ones(n_e, F32))
    ar.alloc('counts', 4 * S * n_rays, 4)
    got = twice(ar, lambda: ok(hip.dexct_poisson_detect(ar['pathlen'].ptr, ar['mu'].ptr, ar['photons'].ptr, ar['gain'].ptr, n_mat,
                                                         n_e, S, V, R, Ch, 1, 5, 99, ar['counts'].ptr, stream_ptr())),
                ['counts'])['counts'].view(F32).reshape(S, n_rays).astype(F64)
    assert np.array_equal(got, np.round(got))
    for s in range(S):
        m, v = got[s].mean(), got[s].var()
        L = float(lam[s, 0])
        assert abs(m - L) < 5.0 * np.sqrt(L / n_rays), (s, m)
        assert abs(v / L - 1.0) < 0.06, (s, v)
