"""The tensor contract of the device entry points on the device ("tensor contract"): whatever view or dtype a
caller hands in, a call computes what it computes from the plain dense tensor - byte for byte, NaN for NaN - or raises
ValueError.  A different result fails.  The dense views at a storage offset of 1 and 3 elements (tensor_views: ``conforms``)
must compute; refusal is not accepted for them.  They also drive the kernels' fall-backs for pointers that are not on a 16-byte
boundary through the public calls (the wide census of csrc/gn_dedup.hip, dexct_transpose_log's 16-byte path, the float4 loads).

Every variant comes from tests/tensor_views.py and obeys its in-bounds rule: a wrapper that ignored strides or dtype would read
the parent's filler, never memory this module does not own (tests/test_tensor_views.py checks the arithmetic for every shape
used here).  Host tensors and outputs of the wrong size cannot meet that rule; they are refused on the CPU, in
tests/test_tensor_views.py, and never reach a device here.

Each baseline is compared once with the float64 reference its module already uses, at that test's tolerance (named where it is
applied); no tolerance is new.  Everything else is equality - with one exception that the kernels force: ImageProjector.adjoint
scatters with float atomics (csrc/iterative.hip), so two runs of adjoint, sirt or pwls on the same bytes need not agree to the
bit.  Their offset variants are held to the module's own reference bound instead (8 d32, tests/test_gpu_iter.py and
tests/test_gpu_pwls.py); every other variant of theirs must be refused, which is what that strict module promises."""
import functools
import types

import numpy as np
import pytest
import torch

import bounds_refs as br
import gn_cov_refs as cr
import gn_multi_refs as mr
import tensor_views as tv

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DEV = 'cuda'


def check_variants(call, x, base, what, dtypes=True, must_refuse=False):
    """``call(tensor)`` for every variant of the host array ``x`` against the baseline ``base`` (a tensor or a tuple of them)."""
    assert tuple(x.shape) in tv.GPU_SHAPES, x.shape                          # (the CPU module checks the in-bounds rule there)
    base = base if isinstance(base, tuple) else (base,)
    wrong, seen = [], []
    for r in tv.variants(x, dtypes):
        t = r.build(DEV)
        try:
            got = call(t)
        except ValueError as e:
            seen.append(f'{r.name}: refused')
            if r.conforms:
                wrong.append(f'{r.name}: refused ({e})')
            continue
        seen.append(f'{r.name}: computed')
        if must_refuse and not r.conforms:
            wrong.append(f'{r.name}: neither refused nor conforming')
            continue
        got = got if isinstance(got, tuple) else (got,)
        if len(got) != len(base) or not all(tv.same_bytes(g, b) for g, b in zip(got, base)):
            wrong.append(f'{r.name}: another result')
    print(f'{what}: ' + ', '.join(seen))
    assert not wrong, (what, wrong)


def refused(call, what):
    with pytest.raises(ValueError):
        call()


# ---- Newton: gn_device ---------------------------------------------------------------------------------------------------------------

N_E = 48


@functools.lru_cache(maxsize=None)
def gn_tables():
    """one pair of spectra on 48 energies; air counts of about 1900: integer counts stay exact in float16 and int32"""
    rng = np.random.default_rng(7)
    E = np.linspace(20.0, 140.0, N_E)
    mus = np.array([[0.25], [0.18]]) * (E[None, :] / 60.0) ** -np.array([[0.6], [2.6]]) + np.array([[0.15], [0.12]])
    i0 = rng.uniform(0.5, 1.0, (2, N_E))
    i0[0, N_E // 2:] *= 0.1                                                     # a low and a high spectrum
    i0[1, :N_E // 4] *= 0.1
    i0 *= 1900.0 / i0.sum(axis=1, keepdims=True)
    return i0, mus


@functools.lru_cache(maxsize=None)
def gn_problem(shape, f32):
    """integer counts of random thicknesses, [2] + shape, and the oracle's 30 iterations on them"""
    from oracle import gn_oracle
    i0, mus = gn_tables()
    rng = np.random.default_rng(100 + len(shape) + shape[0])
    n = int(np.prod(shape))
    a = np.stack([rng.uniform(0.0, 6.0, n), rng.uniform(0.0, 1.5, n)], -1)
    a[:n // 5] = 0.0                                                            # air: masked pixels
    att = np.exp(-(a[:, :1] * mus[0] + a[:, 1:] * mus[1]))
    g = np.maximum(np.rint(np.einsum('ke,pe->kp', i0, att)), 2.0).reshape((2,) + shape)
    g = g.astype(F32) if f32 else g
    with np.errstate(all='ignore'):
        g2d = g.astype(F64).reshape(2, 1, n)
        ref = gn_oracle.newton_solve(g2d, i0, mus, 30)[0]
        ref_p = gn_oracle.newton_solve(g2d * (1 + 1e-13), i0, mus, 30)[0]
    for arr in (g, ref, ref_p):
        arr.setflags(write=False)
    return g, ref, ref_p


GN_SHAPES = {'v4c16r8': ((4, 16, 8), (8, 16)), 'v4c15r6': ((4, 15, 6), (6, 15)), 'flat197': ((197,), None)}


def gn_call(shape, out_rc, **fixed):
    from dex_ct_sim_amd import matdecomp as md
    i0, mus = gn_tables()

    def call(g1, g2, i0=i0, mus=mus, **kw):
        return md.gn_device(g1, g2, i0, mus, 30, stop_tol=0.0, two_level=False, out_rc=out_rc, dedup=True if out_rc else None,
                            mask_frac=0.9, **dict(fixed, **kw))
    return call


@pytest.mark.parametrize('f32', [True, False], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', list(GN_SHAPES))
def test_gn_device(hip, name, f32):
    from dex_ct_sim_amd import matdecomp as md
    shape, out_rc = GN_SHAPES[name]
    g, ref, ref_p = gn_problem(shape, f32)
    i0, mus = gn_tables()
    gmax = np.array(float(g[0].max()))
    assert gmax < 2048.0
    g1, g2, mm = tv.plain(g[0], DEV), tv.plain(g[1], DEV), tv.plain(gmax, DEV)
    call = gn_call(shape, out_rc)
    base = call(g1, g2, mask_max=mm).clone()
    if name == 'v4c16r8' and not f32:
        assert md.last_gn_stats()['dedup'] is not None                          # the dedup route and its wide census took this one
    # the baseline against oracle/gn_oracle.py, as tests/test_gpu_gn.py::test_random_tables_against_numpy_oracle: 1e-7 of
    # max(|a|, 1) where the oracle is finite and insensitive to a 1e-13 perturbation of its input; masked pixels are exact zeros
    got = base.cpu().numpy()
    if out_rc is not None:
        got = np.swapaxes(got, -3, -2)                                          # [v][r][c][2] -> the input's [v][c][r][2]
    got = got.reshape(-1, 2)
    air = g[0].astype(F64).reshape(-1) >= 0.9 * float(gmax)
    assert air.any() and not air.all() and np.all(got[air] == 0.0)
    ok = np.isfinite(ref).all(-1) & (np.abs(ref - ref_p).max(-1) <= 1e-10 * np.maximum(np.abs(ref).max(-1), 1.0)) & ~air
    assert ok.sum() > 0.5 * (~air).sum()
    assert np.max(np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1.0)) < 1e-7
    # every argument in every variant
    check_variants(lambda t: call(t, g2, mask_max=mm), g[0], base, f'gn_device {name} g1')
    check_variants(lambda t: call(g1, t, mask_max=mm), g[1], base, f'gn_device {name} g2')
    for r in tv.variants(g[0]):                                                 # both sinograms in the same variant
        a = call(r.build(DEV), [q for q in tv.variants(g[1]) if q.name == r.name][0].build(DEV), mask_max=mm)
        assert tv.same_bytes(a, base), (name, r)
    check_variants(lambda t: call(g1, g2, mask_max=t), gmax, base, f'gn_device {name} mask_max')
    tables = torch.from_numpy(np.stack([i0, mus])).to(DEV)                      # tables given as device tensors
    assert tv.same_bytes(call(g1, g2, i0=tables[0], mus=tables[1], mask_max=mm), base)
    check_variants(lambda t: call(g1, g2, i0=t, mus=tables[1], mask_max=mm), i0, base, f'gn_device {name} i0', dtypes=False)
    check_variants(lambda t: call(g1, g2, i0=tables[0], mus=t, mask_max=mm), mus, base, f'gn_device {name} mus', dtypes=False)
    # out: a dense tensor at any offset is written and returned; anything else is refused
    # (this kernel stores a pixel's two doubles as one 16-byte piece and the library refuses an ``out`` off that boundary: 1 and 3
    # doubles into an allocation are refused here, by name, and 2 doubles in takes the place of the offset variants)
    out_shape = tuple(base.shape)
    zeros = np.zeros(out_shape)
    for r in tv.variants(zeros, dtypes=False) + [tv.Recipe('offset2', zeros, torch.float64, tv._dense_strides(out_shape), 2, conforms=True)]:
        out = r.build(DEV)
        if r.name == 'offset2':
            assert out.data_ptr() % 16 == 0 and call(g1, g2, mask_max=mm, out=out) is out and tv.same_bytes(out, base), r
        else:
            assert not r.conforms or out.data_ptr() % 16 == 8
            with pytest.raises(ValueError, match='out must'):
                call(g1, g2, mask_max=mm, out=out)
    for kind, make in tv.written_variants(out_shape, torch.float64).items():
        refused(lambda: call(g1, g2, mask_max=mm, out=make(DEV)), kind)
    if out_rc is not None:
        refused(lambda: call(g1, g2, mask_max=mm, dedup_workspace=torch.zeros(1 << 16, dtype=torch.float32, device=DEV)), 'workspace dtype')


# ---- Newton: gn_device_multi ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(4, 16, 8), (197,)], ids=str)
@pytest.mark.parametrize('f32', [True, False], ids=['f32', 'f64'])
def test_gn_device_multi(hip, shape, f32):
    from dex_ct_sim_amd import matdecomp as md
    n = int(np.prod(shape))
    g, i0, mus = mr.sweep_case(3, 2, N_E)
    scale = 2000.0 / g.max()                                                    # the same problem with counts below 2048 ...
    g, i0 = np.maximum(np.rint(g[:, :n] * scale), 1.0), i0 * scale            # ... rounded to integers
    ref = mr.newton_solve_multi(g, i0, mus, 30)
    g = (g.astype(F32) if f32 else g).reshape((3,) + shape)
    gmax = np.array(float(g[0].max()))
    g_d, mm = tv.plain(g, DEV), tv.plain(gmax, DEV)
    call = lambda t, i0=i0, mus=mus, **kw: md.gn_device_multi(t, i0, mus, 30, **kw)
    plain = call(g_d).clone()
    # tests/test_gpu_gn_multi.py::test_shape_sweep_against_the_restatement: 1e-9 of max(|a|, 1)
    assert mr.rel_err(plain.cpu().numpy().reshape(n, 2), ref) <= 1e-9
    base = call(g_d, mask_max=mm, mask_frac=0.5).clone()
    masked = (base == 0).all(-1)
    assert masked.any() and not masked.all() and tv.same_bytes(base[~masked], plain[~masked])
    check_variants(lambda t: call(t, mask_max=mm, mask_frac=0.5), g, base, f'gn_device_multi {shape} g')
    check_variants(lambda t: call(g_d, mask_max=t, mask_frac=0.5), gmax, base, f'gn_device_multi {shape} mask_max')
    check_variants(lambda t: call(g_d, i0=t), i0, plain, f'gn_device_multi {shape} i0', dtypes=False)
    check_variants(lambda t: call(g_d, mus=t), mus, plain, f'gn_device_multi {shape} mus', dtypes=False)
    for r in tv.variants(np.zeros(tuple(plain.shape)), dtypes=False):
        out = r.build(DEV)
        if r.conforms:
            assert call(g_d, out=out) is out and tv.same_bytes(out, plain), r
        else:
            refused(lambda: call(g_d, out=out), r)
    for kind, make in tv.written_variants(tuple(plain.shape), torch.float64).items():
        refused(lambda: call(g_d, out=make(DEV)), kind)


# ---- the covariance ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['estimator', 'crlb'])
def test_gn_covariance_device(hip, kind):
    from dex_ct_sim_amd import matdecomp as md
    shape = (4, 16, 8)
    n = int(np.prod(shape))
    a, i0, i0v, mus = cr.sweep_case(2, 2, 60)
    a = np.maximum(np.rint(a[:n]), 1.0)                                         # integer states: exact in every dtype variant
    ld = cr.covariance_full(a, i0, i0v, mus, kind, np.longdouble)
    a = a.reshape(shape + (2,))
    mask_g = (np.arange(n) % 11 + 1.0).astype(F32).reshape(shape)
    gmax = np.array(11.0)
    a_d, mg, mm = tv.plain(a, DEV), tv.plain(mask_g, DEV), tv.plain(gmax, DEV)
    call = lambda t, **kw: md.gn_covariance_device(t, i0, i0v, mus, kind, **kw)
    plain = call(a_d).clone()
    # tests/test_gpu_gn_cov.py::test_kernel_against_the_long_double_restatement: error ratio <= 4 x the float64 restatement's worst
    assert cr.error_ratio(plain.cpu().numpy().reshape(n, 3), ld) <= 4.0 * max(cr.sweep_ratio_f64().values())
    kw = dict(mask_g=mg, mask_max=mm, mask_frac=0.6)
    base = call(a_d, **kw).clone()
    masked = (base == 0).all(-1)
    assert masked.any() and not masked.all() and tv.same_bytes(base[~masked], plain[~masked])
    check_variants(lambda t: call(t, **kw), a, base, f'gn_covariance_device {kind} a')
    check_variants(lambda t: call(a_d, **dict(kw, mask_g=t)), mask_g, base, f'gn_covariance_device {kind} mask_g')
    check_variants(lambda t: call(a_d, **dict(kw, mask_max=t)), gmax, base, f'gn_covariance_device {kind} mask_max')
    for tab, x in (('i0', i0), ('i0v', i0v), ('mus', mus)):
        args = dict(i0=i0, i0v=i0v, mus=mus)
        check_variants(lambda t: md.gn_covariance_device(a_d, **dict(args, **{tab: t}), kind=kind), x, plain,
                       f'gn_covariance_device {kind} {tab}', dtypes=False)
    for r in tv.variants(np.zeros(tuple(plain.shape)), dtypes=False):
        out = r.build(DEV)
        if r.conforms:
            assert call(a_d, out=out) is out and tv.same_bytes(out, plain), r
        else:
            refused(lambda: call(a_d, out=out), r)


# ---- FBP ---------------------------------------------------------------------------------------------------------------------------

FBP = {'fan': (dict(), (12, 16), 5e-5), 'stack9': (dict(N_rows=9), (12, 9, 16), 5e-5),
       'cone4': (dict(N_rows=4, cone=True, h_iso=0.4), (12, 4, 16), 5e-5), 'short': (dict(theta_tot=4.4), (12, 16), 3e-5)}
N_MATRIX, FOV, RAMP = 16, 20.0, 0.9


def fbp_scanner(name):
    import dex_ct_sim_amd as dx
    return dx.FanBeamGeometry(N_channels=16, N_proj=12, **FBP[name][0])


@pytest.mark.parametrize('name', list(FBP))
def test_recon_device(hip, name):
    from dex_ct_sim_amd import back_project as bp
    from oracle import fbp_oracle as fo
    ct, (_, shape, tol) = fbp_scanner(name), FBP[name]
    s = np.random.default_rng(5).integers(0, 9, shape).astype(F32)
    call = lambda t: bp.recon_device(t, ct, N_MATRIX, FOV, RAMP)
    base = call(tv.plain(s, DEV)).clone()
    got = base.cpu().numpy()
    # the tolerances of tests/test_gpu_fbp.py: test_random_reconstructions_match_oracle (fan, stack: 5e-5 of max |ref|),
    # test_fdk_matches_oracle_on_random_data (cone: 5e-5), test_short_scan_parker_matches_oracle (short: 3e-5)
    if name == 'cone4':
        n_sl, z0, dz = bp.default_slices(ct)
        ref = fo.fdk_recon(s, ct.thetas, ct.gammas, ct.SID, ct.SDD, ct.row_z(), ct.src_z, N_MATRIX, FOV, RAMP, z0 + dz * np.arange(n_sl))
        assert got.shape == ref.shape and np.max(np.abs(got - ref)) < tol * np.abs(ref).max()
    else:
        rows = s.reshape(12, -1, 16)
        for r in range(rows.shape[1]):
            ref, _ = fo.get_recon(np.ascontiguousarray(rows[:, r]), ct.thetas, ct.gammas, ct.SID, N_MATRIX, FOV, RAMP,
                                  theta_tot=4.4 if name == 'short' else None)
            assert np.max(np.abs(got.reshape(-1, N_MATRIX, N_MATRIX)[r] - ref)) < tol * np.abs(ref).max(), r
    check_variants(call, s, base, f'recon_device {name}')


def test_recon_device_bhc_branch_and_linearize_device(hip):
    """bhc= takes the sinogram through the same rule: the float64 stride-2 plane is cast and made dense; linearize_device itself
    is strict."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import back_project as bp, bhc, synthetic
    ct = fbp_scanner('fan')
    table = bhc.linearization_table(ct, synthetic.kramers_spectrum(120), 'water')
    s = np.random.default_rng(6).integers(0, 5, (12, 16)).astype(F32)
    call = lambda t: bp.recon_device(t, ct, N_MATRIX, FOV, RAMP, bhc=table)
    base = call(tv.plain(s, DEV)).clone()
    assert not tv.same_bytes(base, bp.recon_device(tv.plain(s, DEV), ct, N_MATRIX, FOV, RAMP))
    check_variants(call, s, base, 'recon_device bhc')
    lin = lambda t, **kw: bhc.linearize_device(t, table, **kw)
    base = lin(tv.plain(s, DEV)).clone()
    check_variants(lin, s, base, 'linearize_device sino_d', must_refuse=True)
    for r in tv.variants(np.zeros((12, 16), F32), dtypes=False):
        out = r.build(DEV)
        if r.conforms:
            assert lin(tv.plain(s, DEV), out=out) is out and tv.same_bytes(out, base), r
        else:
            refused(lambda: lin(tv.plain(s, DEV), out=out), r)


@functools.lru_cache(maxsize=None)
def recon_matrix():
    """the system matrix of ImageProjector(fbp_scanner('fan'), N_MATRIX, FOV), as tests/iter_refs.py builds it for its scans"""
    import iter_refs as ir
    ct = fbp_scanner('fan')
    scan = br.Scan(nx=N_MATRIX, ny=N_MATRIX, nz=1, n_views=12, n_ch=16, n_rows=1, z_first=0, dx=FOV / N_MATRIX, dy=FOV / N_MATRIX, dz=1.0,
                   sid=ct.SID, sdd=ct.SDD)
    scan.view_cs, scan.chan_cs = np.ascontiguousarray(ct.view_cs(), F64), np.ascontiguousarray(ct.chan_cs(), F64)
    A = ir.system_matrix(scan)
    A.setflags(write=False)
    return A


def test_recon_device_sirt_branch(hip):
    """recon_device(method='sirt') from zero: the plain tensor and every variant within 8 d32 of the float64 restatement, the bound
    of tests/test_gpu_iter.py::test_sirt_matches_reference (the adjoint's float atomics rule out equal bytes).  A sinogram read
    as other bytes - the parent's filler of 3.0 among values of 0 .. 8 - misses that bound by orders of magnitude."""
    import iter_refs as ir
    from dex_ct_sim_amd import back_project as bp
    ct, A = fbp_scanner('fan'), recon_matrix()
    s = np.random.default_rng(16).integers(0, 9, (12, 16)).astype(F32)
    args = (A, s.reshape(12, 1, 16), 5, 1, 1.0, True, None)
    ref64, ref32 = ir.sirt_ref(*args, dtype=F64), ir.sirt_ref(*args, dtype=F32)
    d32 = float(np.max(np.abs(ref32.astype(F64) - ref64)))
    assert d32 > 0 and np.abs(ref64).max() > 1e4 * d32
    assert tuple(s.shape) in tv.GPU_SHAPES
    for r in [None] + tv.variants(s):
        t = tv.plain(s, DEV) if r is None else r.build(DEV)
        img = bp.recon_device(t, ct, N_MATRIX, FOV, RAMP, method='sirt', n_iters=5, n_subsets=1, relax=1.0, init='zero', nonneg=True)
        err = float(np.max(np.abs(img.cpu().numpy().reshape(-1).astype(F64) - ref64)))
        print(f'recon_device sirt {r}: err {err:.3e}, d32 {d32:.3e}')
        assert img.shape == (N_MATRIX, N_MATRIX) and err <= 8.0 * d32, (r, err / d32)


def test_recon_covariance_device_and_precision_weights(hip):
    from dex_ct_sim_amd import back_project as bp, iterative as it
    ct = fbp_scanner('fan')
    cov = np.random.default_rng(8).integers(1, 9, (12, 16, 3)).astype(F64)
    cov[..., 1] = 0.0                                                           # positive definite: a diagonal covariance
    call = lambda t: bp.recon_covariance_device(t, ct, N_MATRIX, FOV, RAMP)
    check_variants(call, cov, call(tv.plain(cov, DEV)).clone(), 'recon_covariance_device cov_d')
    ctn = fbp_scanner('stack9')
    cov9 = np.random.default_rng(9).integers(1, 9, (12, 9, 16, 3)).astype(F64)
    call9 = lambda t: bp.recon_covariance_device(t, ctn, N_MATRIX, FOV, RAMP)
    check_variants(call9, cov9, call9(tv.plain(cov9, DEV)).clone(), 'recon_covariance_device cov_d stack')
    check_variants(it.precision_weights, cov, it.precision_weights(tv.plain(cov, DEV)).clone(), 'precision_weights cov_d')


# ---- projection ----------------------------------------------------------------------------------------------------------------------

def projector_of(name):
    """a Projector on a scan of tests/bounds_refs.py: the scanner and the phantom as the objects Projector reads"""
    from dex_ct_sim_amd import forward_project as fp
    s = br.scan(name)
    ct = types.SimpleNamespace(N_proj=s.n_views, N_channels=s.n_ch, N_rows=s.n_rows, SID=s.sid, SDD=s.sdd, cone=s.cone, src_z=s.src_z,
                               view_cs=lambda: s.view_cs, chan_cs=lambda: s.chan_cs, row_z=lambda: s.row_z)
    mats = [types.SimpleNamespace(density=1.0 + k, matcomp=f'm{k}') for k in range(s.n_mat)]
    ph = types.SimpleNamespace(volume=s.vol, Nx=s.nx, Ny=s.ny, Nz=s.nz, dx=s.dx, dy=s.dy, dz=s.dz, z_index=s.z_first, materials=mats,
                               n_materials=s.n_mat)
    return s, fp.Projector(ct, ph)


@pytest.mark.parametrize('name', ['r16', 'cone'])
def test_project_tables(hip, name):
    from oracle import c_oracle as co
    from test_gpu_siddon import REL_TOL
    s, pj = projector_of(name)
    assert pj.n_mat == s.n_mat
    air = s.w.sum(axis=1)
    mu_d, w_d = tv.plain(s.mu, DEV), tv.plain(s.w, DEV)
    base = {lay: tuple(t.clone() for t in pj.project_tables(mu_d, w_d, layout=lay, air=air)) for lay in (0, 1)}
    # tests/test_gpu_bounds_projection.py: counts within REL_TOL of c_oracle.project_classic / project_cone(dda=False), tie rays left out
    g = s.geom(co.make_geom)
    if s.cone:
        ref, _ = co.project_cone(g, s.view_cs, s.chan_cs, 0, s.n_views, s.row_z, s.src_z, s.vol, s.mu, s.w, dda=False, n_threads=8)
    else:
        ref = co.project_classic(g, s.view_cs, s.chan_cs, 0, s.n_views, s.vol, s.mu, s.w, n_threads=8)
    ref = np.asarray(ref, F64).reshape(s.n_spec, s.n_views, s.n_rows, s.n_ch)
    assert br.counts_rel(base[0][0].cpu().numpy(), ref, br.tie_rays(s, 0, s.n_views)) < REL_TOL
    assert tv.same_bytes(base[1][0], base[0][0].permute(0, 1, 3, 2)) and tv.same_bytes(base[1][1], base[0][1].permute(0, 1, 3, 2))
    for lay in (0, 1):
        call = lambda mu, w: pj.project_tables(mu, w, layout=lay, air=air)
        check_variants(lambda t: call(t, w_d), s.mu, base[lay], f'project_tables {name} layout {lay} mu_d', dtypes='exact')
        check_variants(lambda t: call(mu_d, t), s.w, base[lay], f'project_tables {name} layout {lay} w_d', dtypes='exact')
        shape = tuple(base[lay][0].shape)
        for r in tv.variants(np.zeros(shape, F32), dtypes=False):
            out, log_out = r.build(DEV), r.build(DEV)
            if r.conforms:
                c, lg = pj.project_tables(mu_d, w_d, layout=lay, air=air, out=out, log_out=log_out)
                assert c is out and lg is log_out and tv.same_bytes(c, base[lay][0]) and tv.same_bytes(lg, base[lay][1]), (lay, r)
            else:
                refused(lambda: pj.project_tables(mu_d, w_d, layout=lay, air=air, out=out), r)
                refused(lambda: pj.project_tables(mu_d, w_d, layout=lay, air=air, log_out=log_out), r)
        for kind, make in tv.written_variants(shape, torch.float32).items():
            refused(lambda: pj.project_tables(mu_d, w_d, layout=lay, air=air, out=make(DEV)), kind)
            refused(lambda: pj.project_tables(mu_d, w_d, layout=lay, air=air, log_out=make(DEV)), kind)
    if not s.cone:                                                              # quantum noise: the variance weights as a third table
        w2_d = tv.plain(s.w2, DEV)
        noisy = tuple(t.clone() for t in pj.project_tables(mu_d, w_d, w2_d=w2_d, seed=5, air=air))
        assert not tv.same_bytes(noisy[0], base[0][0])
        check_variants(lambda t: pj.project_tables(mu_d, w_d, w2_d=t, seed=5, air=air), s.w2, noisy, f'project_tables {name} w2_d', dtypes='exact')
    # the log pass of its own
    counts = base[0][0].cpu().numpy()
    log0 = pj.sino_log(base[0][0], air).clone()
    assert tv.same_bytes(log0, base[0][1]) or name == 'cone'
    check_variants(lambda t: pj.sino_log(t, air), counts, log0, f'sino_log {name} counts', dtypes='exact')
    for r in tv.variants(np.zeros(counts.shape, F32), dtypes=False):
        out = r.build(DEV)
        if r.conforms:
            assert pj.sino_log(base[0][0], air, out) is out and tv.same_bytes(out, log0), r
        else:
            refused(lambda: pj.sino_log(base[0][0], air, out), r)


@pytest.mark.parametrize('n', [52, 37])
def test_transpose_log(hip, n):
    _, pj = projector_of('r16')
    rows, cols = 16, 2
    src = np.random.default_rng(n).integers(1, 2000, (2, n, rows, cols)).astype(F32)
    air = [2000.0, 1500.0]
    src_d = tv.plain(src, DEV)
    dst, lg = torch.empty((2, n, cols, rows), device=DEV), torch.empty((2, n, cols, rows), device=DEV)
    pj.transpose_log(src_d, dst, lg, air, rows, cols)
    assert tv.same_bytes(dst, src_d.permute(0, 1, 3, 2)) and tv.same_bytes(lg, pj.sino_log(dst, air))

    def call(t, dst=None, log_dst=None):
        d = torch.empty((2, n, cols, rows), device=DEV) if dst is None else dst
        l = torch.empty((2, n, cols, rows), device=DEV) if log_dst is None else log_dst
        pj.transpose_log(t, d, l, air, rows, cols)
        return d, l
    check_variants(call, src, (dst, lg), f'transpose_log {n} src')
    for r in tv.variants(np.zeros((2, n, cols, rows), F32), dtypes=False):
        d, l = r.build(DEV), r.build(DEV)
        if r.conforms:                                                          # (pointers off the 16-byte boundary: the narrow path)
            got = call(src_d, d, l)
            assert tv.same_bytes(got[0], dst) and tv.same_bytes(got[1], lg), r
        else:
            refused(lambda: call(src_d, dst=d), r)
            refused(lambda: call(src_d, log_dst=l), r)


# ---- the matched pair, SIRT and PWLS (strict: everything that does not conform is refused) -------------------------------------------------

def test_image_projector_sirt_and_pwls(hip):
    from dex_ct_sim_amd.iterative import pwls, sirt
    import iter_refs as ir
    from test_gpu_iter import projector, sirt_problem, sirt_refs
    from test_gpu_pwls import BETA, DELTA, pwls_problem, pwls_refs, rounding_scale
    name = 'c53'
    scan, p = ir.small(name), projector(name)
    x = np.random.default_rng(3).integers(0, 5, (scan.nz, scan.ny, scan.nx)).astype(F32)
    fwd = p.forward(tv.plain(x, DEV)).clone()                                   # a gather: bit-reproducible
    check_variants(lambda t: p.forward(t), x, fwd, 'forward image', must_refuse=True)
    for r in tv.variants(np.zeros(p.sino_shape, F32), dtypes=False):
        out = r.build(DEV)
        if r.conforms:
            assert p.forward(tv.plain(x, DEV), out=out) is out and tv.same_bytes(out, fwd), r
        else:
            refused(lambda: p.forward(tv.plain(x, DEV), out=out), r)
    # sirt, tests/test_gpu_iter.py::test_sirt_matches_reference: within 8 d32 of the float64 reference
    b, x0 = sirt_problem(name)
    ref64, ref32 = sirt_refs(name, 1, True, True)
    d32 = float(np.max(np.abs(ref32.astype(F64) - ref64)))
    x0_d = tv.plain(x0, DEV)
    for r in [None] + tv.variants(b):
        try:
            got = sirt(tv.plain(b, DEV) if r is None else r.build(DEV), p, 5, 1, 1.0, x0=x0_d, nonneg=True)
        except ValueError:
            assert r is not None and not r.conforms, r
            continue
        assert r is None or r.conforms, (r, 'neither refused nor conforming')
        assert float(np.max(np.abs(got.cpu().numpy().reshape(-1).astype(F64) - ref64))) <= 8.0 * d32, r
    for r in tv.variants(x0):
        if not r.conforms:
            refused(lambda: sirt(tv.plain(b, DEV), p, 5, 1, 1.0, x0=r.build(DEV)), r)
            refused(lambda: p.adjoint(tv.plain(b, DEV), out=r.build(DEV)), r)
    # pwls, tests/test_gpu_pwls.py::test_pwls_matches_reference: within 8 d32 of the float64 reference
    K = 2
    bk, W, xk = pwls_problem(name, K)
    r64, r32 = pwls_refs(name, K, 1, False, True)
    scale, _ = rounding_scale(name, r64, r32)
    for arg, arr in (('sinograms', bk), ('weights', W)):
        for r in [None] + tv.variants(arr):
            t = {'sinograms': tv.plain(bk, DEV), 'weights': tv.plain(W, DEV)}
            if r is not None:
                t[arg] = r.build(DEV)
            try:
                got = pwls(t['sinograms'], t['weights'], p, 5, 1, BETA[:K], DELTA[:K], x0=tv.plain(xk, DEV), nonneg=False)
            except ValueError:
                assert r is not None and not r.conforms, (arg, r)
                continue
            assert r is None or r.conforms, (arg, r, 'neither refused nor conforming')
            assert float(np.max(np.abs(got.cpu().numpy().astype(F64) - r64))) <= 8.0 * scale, (arg, r)


# ---- the chain: decomposition -> reconstruction and covariance ------------------------------------------------------------------------

def test_views_of_get_basismat_sinos_go_straight_into_the_next_step(hip):
    """get_basismat_sinos hands device callers a[..., 0], a[..., 1]: float64 views of stride 2.  Fed as they are into recon_device
    and get_basismat_covariance they must give the bytes of their dense float32 / float64 copies, and the image get_recon makes
    of the host copies."""
    import os
    import dex_ct_sim_amd as dx
    from conftest import INPUT
    from dex_ct_sim_amd import back_project as bp, matdecomp as md, synthetic
    ct = dx.FanBeamGeometry(N_channels=16, N_proj=12, eid=True, detector_file=os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'))
    specs = [synthetic.kramers_spectrum(80), synthetic.kramers_spectrum(140)]
    _, i0, mus = md.decomposition_tables(ct, *specs)
    rng = np.random.default_rng(12)
    a = np.stack([rng.uniform(0.0, 20.0, (12, 16)), rng.uniform(0.0, 3.0, (12, 16))], -1)
    a[:, :3] = 0.0                                                              # air at the fan's edge
    g = np.einsum('ke,vce->kvc', i0, np.exp(-(a[..., :1] * mus[0] + a[..., 1:] * mus[1])))
    g1, g2 = tv.plain(g[0].astype(F32), DEV), tv.plain(g[1].astype(F32), DEV)
    m1, m2 = md.get_basismat_sinos(ct, g1, g2, specs[0], specs[1], n_iters=30, stop_tol=0.0, two_level=False)
    assert m1.dtype == torch.float64 and m1.stride() == (32, 2) and m2.storage_offset() == 1 and bool(torch.isfinite(m1).all())
    for m in (m1, m2):
        img = bp.recon_device(m, ct, N_MATRIX, FOV, RAMP)
        assert tv.same_bytes(img, bp.recon_device(m.contiguous().float(), ct, N_MATRIX, FOV, RAMP))
        host, _ = bp.get_recon(m.cpu().numpy(), ct, specs[0], N_MATRIX, FOV, RAMP)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), host.view(np.uint32)) and np.any(host != 0)
    cov = md.get_basismat_covariance(ct, (m1, m2), specs, mask_from=g1)
    dense = md.get_basismat_covariance(ct, (m1.contiguous(), m2.contiguous()), specs, mask_from=g1.clone())
    assert tv.same_bytes(cov, dense) and bool((cov != 0).any())
    # the tensor-in drop-ins normalise whatever they are given
    for r in tv.variants(g[0].astype(F32), dtypes=False):
        q = [v for v in tv.variants(g[1].astype(F32), dtypes=False) if v.name == r.name][0]
        n1, n2 = md.get_basismat_sinos(ct, r.build(DEV), q.build(DEV), specs[0], specs[1], n_iters=30, stop_tol=0.0, two_level=False)
        assert tv.same_bytes(n1, m1) and tv.same_bytes(n2, m2), r


# ---- the "tensor in, tensor out" functions: whatever they are given is uploaded, cast and made dense -------------------------------

def kramers(*kvp):
    from dex_ct_sim_amd import synthetic
    return [synthetic.kramers_spectrum(k) for k in kvp]


def eid_scanner(**kw):
    import os
    import dex_ct_sim_amd as dx
    from conftest import INPUT
    return dx.FanBeamGeometry(N_channels=16, N_proj=12, eid=True, detector_file=os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'), **kw)


def counts_of(ct, specs, seed):
    """float32 counts [K][12][16] of random thicknesses for the spectra (air at the fan's edge)"""
    from dex_ct_sim_amd import matdecomp as md
    _, i0, mus = md.decomposition_tables_multi(ct, specs)
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(0.0, 20.0, (12, 16)), rng.uniform(0.0, 3.0, (12, 16))], -1)
    a[:, :3] = 0.0
    return np.einsum('ke,vce->kvc', i0, np.exp(-(a[..., :1] * mus[0] + a[..., 1:] * mus[1]))).astype(F32)


def each_argument(call, arrays, base, what, dtypes=False):
    """check_variants on every array of ``arrays`` in turn, the others plain: ``call(list of tensors)``"""
    plains = [tv.plain(x, DEV) for x in arrays]
    for k, x in enumerate(arrays):
        check_variants(lambda t: call(plains[:k] + [t] + plains[k + 1:]), x, base, f'{what} [{k}]', dtypes=dtypes)


def test_decomposition_functions_with_tensors_in(hip):
    from dex_ct_sim_amd import matdecomp as md
    ct = eid_scanner()
    two, three = kramers(80, 140), kramers(80, 110, 140)
    g2, g3 = counts_of(ct, two, 21), counts_of(ct, three, 22)
    tup = lambda res: tuple(t.clone() for t in res)
    fixed = dict(n_iters=30, stop_tol=0.0, two_level=False)
    sinos = lambda ts: tup(md.get_basismat_sinos(ct, ts[0], ts[1], two[0], two[1], **fixed))
    base = sinos([tv.plain(g2[0], DEV), tv.plain(g2[1], DEV)])
    assert bool(torch.isfinite(base[0]).all()) and bool((base[0] != 0).any())
    each_argument(sinos, [g2[0], g2[1]], base, 'get_basismat_sinos')
    gn = lambda ts: md.do_matdecomp_gn(ct, ts[0], ts[1], two[0], two[1], 30, stop_tol=0.0, two_level=False)
    base_gn = gn([tv.plain(g2[0], DEV), tv.plain(g2[1], DEV)]).clone()
    live = (base[0] != 0)                                                       # do_matdecomp_gn masks nothing: the same solve elsewhere
    assert tv.same_bytes(base_gn[..., 0][live], base[0][live]) and tv.same_bytes(base_gn[..., 1][live], base[1][live])
    each_argument(gn, [g2[0], g2[1]], base_gn, 'do_matdecomp_gn')
    multi = lambda ts: tup(md.get_basismat_sinos_multi(ct, ts, three, n_iters=30))
    base_m = multi([tv.plain(g, DEV) for g in g3])
    assert len(base_m) == 2 and bool(torch.isfinite(base_m[0]).all()) and bool((base_m[0] != 0).any())
    each_argument(multi, list(g3), base_m, 'get_basismat_sinos_multi')
    # the covariance of integer-valued basis sinograms: every dtype variant reproduces them exactly
    rng = np.random.default_rng(23)
    m = [rng.integers(1, 20, (12, 16)).astype(F64), rng.integers(1, 4, (12, 16)).astype(F64)]
    mask_from = (rng.integers(1, 12, (12, 16))).astype(F32)
    cov = lambda ts: md.get_basismat_covariance(ct, (ts[0], ts[1]), two, mask_from=ts[2])
    base_c = cov([tv.plain(x, DEV) for x in m + [mask_from]]).clone()
    host = md.get_basismat_covariance(ct, tuple(m), two, mask_from=mask_from)   # NumPy in: the same bytes
    assert np.array_equal(base_c.cpu().numpy().view(np.uint64), host.view(np.uint64)) and (host != 0).any() and not host.all()
    each_argument(cov, m + [mask_from], base_c, 'get_basismat_covariance', dtypes=True)


def test_plots_and_get_recon_covariance_with_tensors_in(hip):
    from dex_ct_sim_amd import back_project as bp, matdecomp as md, plots, xcompy
    ct = fbp_scanner('fan')
    cov = np.random.default_rng(31).integers(1, 9, (12, 16, 3)).astype(F64)
    cov[..., 1] = np.minimum(cov[..., 1], 2.0) - 1.0                            # a covariance below the geometric mean of the variances
    c_d = tv.plain(cov, DEV)
    base = plots.vmi_variance(c_d, 70.0).clone()
    # u^T C u on the host, as tests/test_gpu_gn_cov.py::test_public_function: within 4 ulp of the sum of the terms' magnitudes
    u = np.array([xcompy.mixatten(md.matcomp1, np.array([70.0]))[0], xcompy.mixatten(md.matcomp2, np.array([70.0]))[0]])
    terms = np.stack([u[0] * u[0] * cov[..., 0], 2.0 * u[0] * u[1] * cov[..., 1], u[1] * u[1] * cov[..., 2]])
    assert np.all(np.abs(base.cpu().numpy() - terms.sum(0)) <= 4.0 * np.spacing(np.abs(terms).sum(0)))
    check_variants(lambda t: plots.vmi_variance(t, 70.0), cov, base, 'vmi_variance cov')
    for hu in (True, False):
        sd = plots.vmi_noise_map(c_d, 70.0, HU=hu).clone()
        check_variants(lambda t: plots.vmi_noise_map(t, 70.0, HU=hu), cov, sd, f'vmi_noise_map cov HU={hu}')
    Evals = np.arange(40.0, 141.0, 20.0)
    var, e_min = plots.vmi_noise_sweep(Evals, c_d)
    var_h, e_min_h = plots.vmi_noise_sweep(Evals, cov)                          # NumPy in (test_public_function: rtol 1e-12 between the two)
    assert e_min == e_min_h and np.allclose(var, var_h, rtol=1e-12, atol=0.0)
    for r in tv.variants(cov):
        v, e = plots.vmi_noise_sweep(Evals, r.build(DEV))
        assert e == e_min and np.array_equal(v.view(np.uint64), var.view(np.uint64)), r
    rc = lambda t: bp.get_recon_covariance(t, ct, N_MATRIX, FOV, RAMP)
    base_rc = rc(c_d).clone()
    assert tv.same_bytes(base_rc, bp.recon_covariance_device(c_d, ct, N_MATRIX, FOV, RAMP))
    check_variants(rc, cov, base_rc, 'get_recon_covariance cov')


def test_get_basismat_recon_with_tensors_in(hip):
    """Two basis sinograms and their covariance as device tensors in every variant: the images within 8 d32 of the float64
    restatement of the iteration (tests/test_gpu_pwls.py::test_pwls_matches_reference; float atomics in the adjoint rule out
    equal bytes), from zero so that the restatement needs no FBP."""
    import pwls_refs as pr
    from dex_ct_sim_amd import back_project as bp
    ct, A = fbp_scanner('fan'), recon_matrix()
    rng = np.random.default_rng(41)
    b = rng.integers(0, 9, (2, 12, 16)).astype(F32)
    cov = rng.integers(1, 9, (12, 16, 3)).astype(F64)
    cov[..., 1] = 0.0
    W = pr.precision_ref(cov.reshape(-1, 3), 2)[0].reshape(3, 12, 1, 16).astype(F32)
    beta, delta = [0.05, 0.02], [0.5, 0.2]
    args = (A, b.reshape(2, 12, 1, 16), W, 5, 1, beta, delta, False, None, (1, N_MATRIX, N_MATRIX))
    ref64, ref32 = pr.pwls_ref(*args, dtype=F64), pr.pwls_ref(*args, dtype=F32)
    d32 = float(np.max(np.abs(ref32.astype(F64) - ref64)))
    assert d32 > 0 and np.abs(ref64).max() > 1e3 * d32

    def run(b0, b1, c):
        imgs = bp.get_basismat_recon((b0, b1), c, ct, N_MATRIX, FOV, RAMP, beta, delta, n_iters=5, n_subsets=1, init='zero')
        assert all(isinstance(i, torch.Tensor) and i.shape == (N_MATRIX, N_MATRIX) for i in imgs)
        return float(np.max(np.abs(torch.stack(imgs).cpu().numpy().reshape(ref64.shape).astype(F64) - ref64)))
    plains = [tv.plain(b[0], DEV), tv.plain(b[1], DEV), tv.plain(cov, DEV)]
    err = run(*plains)
    print(f'get_basismat_recon plain: err {err:.3e}, d32 {d32:.3e}')
    assert err <= 8.0 * d32
    for k, x in enumerate([b[0], b[1], cov]):
        assert tuple(x.shape) in tv.GPU_SHAPES
        for r in tv.variants(x):
            e = run(*(plains[:k] + [r.build(DEV)] + plains[k + 1:]))
            assert e <= 8.0 * d32, (k, r, e / d32)
