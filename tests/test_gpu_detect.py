"""Every form of the polychromatic detection against the float64 reference of tests/detect_refs.py over the dynamic range: counts,
variance and log sinogram of every ray of every launch, from all-zero attenuation through the underflow of v_exp_f32 to rays
that lose every energy, through Projector.project_tables.  The reference is fed the launch's own float32 path lengths (equal,
bit for bit, to the C oracle's - asserted here too), so the comparison isolates the detection.

Bounds (derived in the docstring of tests/detect_refs.py, which also holds the tables, the scans and the matrix of cases;
tests/test_detect_refs.py shows on the CPU that they hold for float32 emulations of the four summation orders and reject sixteen
kinds of subtly wrong detection), u = 2^-24:
  counts, variance   |got - exact| <= u sum_e |w_e| t_e ((M + 3.5) P_e + 2 + n_e) + 2^-125 sum_e |w_e|; finite, not negative
  log                |got - ln(air / counts)| <= 2^-22 (1 + |ln(air / counts)|) where the float32 quotient is finite, +inf
                     exactly where it is not (counts == 0: a ray that lost every energy), never NaN
  noisy launches     the sample of noise_refs.add_noise_ref from the same launch's clean counts and variance within its bound,
                     at least 1e-20, the log finite
Measured on the MI355X (the code under test - the bounds above are not taken from these): worst |got - exact| / bound over all
rays, tables and cases of a form
  form                    counts   variance  log
  detect_store1           0.339    0.267     0.613      (kernels 1 and 2, up to 4 table rows)
  detect_store_lds        0.313    0.301     0.629      (kernels 1 and 2, 5 .. 60 table rows)
  detect_store4           0.339    0.326     0.629      (kernels 3 and 5: detect_store<NM, 4>, masks, the air shortcut)
  wave_ray_kernel         0.329    -         0.559      (kernel 6; it has no variance)
  rows16_kernel           0.339    0.326     0.643      (kernel 7, staged and per-round stores, the air cache)
  detect_kernel           0.431    0.380     0.640      (kernels 4 and 8, 5 .. 48 table rows, 4 / 2 / 1 rays per thread)
  detect_kernel_chunked   0.354    0.356     0.647      (kernels 4 and 8, 49 and 60 table rows)
  detect_energy_pairs     0.331    0.323     0.630      (cone kernels 1 and 2, one and two spectra)
  cone_scalar_loop        0.199    0.198     0.643      (cone kernels 1 and 2, three and four spectra)
  cone_groups             0.342    0.329     0.644      (cone kernel 2, 4, 7 and 50 table rows)
Every bit-identity claim of siddon_detect.h and detect.hip held on every table.  One finding, fixed in csrc/common.h: log_ratio
gave +inf for a denormal count whose quotient float32 still holds (v_rcp_f32 takes a denormal for zero) - on the step-120 table
of the three-energy cases and on the hand-made counts of test_log_of_tiny_and_zero_counts with an air signal below 4.
"""
import numpy as np
import pytest
import torch

import detect_refs as dr
import noise_refs as nr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = nr.SEEDS[1]
_measured = {}


def dev(*arrays):
    return [torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda') for a in arrays]


def projector(key, n_mat, kernel):
    from dex_ct_sim_amd import forward_project as fp
    ct, ph = dr.scan(key, n_mat)
    pj = fp.Projector(ct, ph, kernel=kernel)
    assert pj.n_mat == n_mat                                                 # every id present, no two rows merged
    return pj


def assert_form(pj, form, kernel, n_mat, n_s):
    """The projector's own flags say that the case runs the form it is named for."""
    groups = pj.grouped or pj.grouped_packed or pj.cone_groups
    if form in ('detect_store1', 'detect_store_lds'):
        assert not pj.cone and kernel in (1, 2) and not pj.use_packed and not groups and pj.native_layout == kernel - 1
        assert (n_mat <= 4) == (form == 'detect_store1')
    elif form == 'detect_store4':
        assert not pj.cone and kernel in (3, 5) and not pj.use_packed and not groups and pj.native_layout == 1 and n_mat <= 4
    elif form == 'wave_ray_kernel':
        assert not pj.cone and kernel == 6 and not pj.use_packed and not groups and pj.native_layout == 0 and n_mat <= 4
    elif form == 'rows16_kernel':
        assert pj.use_packed and pj.vol_z2 is not None and not groups and pj.native_layout == 1
    elif form in ('detect_kernel', 'detect_kernel_chunked'):
        assert not pj.cone and not pj.use_packed and pj.native_layout == 1
        assert (pj.grouped and kernel == 4) or (pj.grouped_packed and kernel == 8)
        assert (n_mat <= 48) == (form == 'detect_kernel')
    elif form in ('detect_energy_pairs', 'cone_scalar_loop'):
        assert pj.cone and not pj.cone_groups and pj.cone_rows == (kernel == 2) and n_mat <= 3
        assert (n_s <= 2) == (form == 'detect_energy_pairs')
    elif form == 'cone_groups':
        assert pj.cone and pj.cone_rows and pj.cone_groups and n_mat > 3
    else:
        raise AssertionError(form)


def record(form, quantity, q):
    _measured[form, quantity] = max(_measured.get((form, quantity), 0.0), q)


def noisy_ok(got, ref, bound, raw):
    """Within add_noise_ref's bound of its reference; a value clipped to the float32 1e-20 where the reference, within its bound,
    is clipped too."""
    g32 = np.asarray(got, F32).reshape(ref.shape)
    g = g32.astype(F64)
    clipped = (g32 == F32(nr.FLOOR)) & (raw - bound <= nr.FLOOR)
    return bool(np.all(np.isfinite(g)) and np.all((np.abs(g - ref) <= bound) | clipped))


def check_launches(pj, form, pl0, mu, w, w2, step, variance=True):
    """One table of the sweep through one projector: every assertion of the module docstring on every ray."""
    M, n_e = mu.shape
    n_s = w.shape[0]
    ct = pj.ct
    native = pj.native_layout
    air = w.astype(F64).sum(axis=1)
    mu_d, w_d, w2_d = dev(mu, w, w2)
    counts, pathlen, log = pj.project_tables(mu_d, w_d, want_pathlen=True, air=air, layout=None)
    pl = pathlen.cpu().numpy().reshape(-1, M)
    assert np.array_equal(pl, pl0), 'path lengths differ from the oracle (or between launches)'
    c = counts.cpu().numpy().reshape(n_s, -1)
    exact, bound = dr.detect_ref(pl, mu, w)
    q = dr.worst(c, exact, bound)
    print(f'  table {step}: counts {q:.3f}', end='')
    record(form, 'counts', q)
    assert dr.within(c, exact, bound), (step, 'counts', q)
    P, _ = dr.exponents(pl, mu)
    lost = P.min(axis=1) > 88.0                                              # every exponential below 2^-126 with room to spare
    assert np.all(c[:, lost] == 0.0)
    if step == 120:
        assert lost.mean() >= 0.01
    # the log: from the detection store, as a pass of its own, and through the transpose in the reference's order
    lexact, lbound = dr.log_ref(air, c)
    for name, lg in (('store', log), ('sino_log', pj.sino_log(counts, air))):
        lg = lg.cpu().numpy().reshape(n_s, -1)
        record(form, 'log', dr.log_worst(lg, lexact, lbound))
        assert dr.log_within(lg, lexact, lbound), (step, name, dr.log_worst(lg, lexact, lbound))
        assert np.all(np.isinf(lg[:, lost]))
    c0, l0 = pj.project_tables(mu_d, w_d, air=air, layout=0)
    assert torch.equal(c0, counts.permute(0, 1, 3, 2) if native == 1 else counts)
    l0exact, l0bound = dr.log_ref(air, c0.cpu().numpy().reshape(n_s, -1))
    l0 = l0.cpu().numpy().reshape(n_s, -1)
    record(form, 'log', dr.log_worst(l0, l0exact, l0bound))
    assert dr.log_within(l0, l0exact, l0bound), (step, 'layout 0', dr.log_worst(l0, l0exact, l0bound))
    print(f', log {_measured[form, "log"]:.3f} (so far)', end='')
    if not variance:
        print()
        return c, None
    # the variance, and the sample drawn from the counts and the variance of the same launch
    noisy, nlog, var = pj.project_tables(mu_d, w_d, layout=None, w2_d=w2_d, seed=SEED, air=air, want_variance=True)
    v = var.cpu().numpy().reshape(n_s, -1)
    vexact, vbound = dr.detect_ref(pl, mu, w2)
    q = dr.worst(v, vexact, vbound)
    print(f', variance {q:.3f}')
    record(form, 'variance', q)
    assert dr.within(v, vexact, vbound), (step, 'variance', q)
    n = noisy.cpu().numpy().reshape(n_s, -1)
    nl = nlog.cpu().numpy().reshape(n_s, -1)
    assert np.all(n >= F32(nr.FLOOR)) and np.all(np.isfinite(n)) and np.all(np.isfinite(nl)), step
    ref, nbound, raw = nr.add_noise_ref(c, v, (ct.N_proj, ct.N_rows, ct.N_channels), native, 0, SEED, raw=True)
    assert noisy_ok(n, ref, nbound, raw), (step, 'sample')
    assert not np.array_equal(n[:, ~lost], c[:, ~lost])
    nlexact, nlbound = dr.log_ref(air, n)
    assert dr.log_within(nl, nlexact, nlbound), (step, 'log of the sample', dr.log_worst(nl, nlexact, nlbound))
    return c, v


@pytest.mark.parametrize('case', dr.CASES, ids=dr.case_id)
def test_form_meets_the_bound_on_every_ray(hip, case, monkeypatch):
    form, key, kernel, n_mat, n_e, n_s, _, _ = case
    pj = projector(key, n_mat, kernel)
    assert_form(pj, form, kernel, n_mat, n_s)
    pl0 = dr.oracle_pathlen(key, n_mat, layout=pj.native_layout)
    print()
    for staged in (('1', '0') if kernel == 7 else (None,)):
        if staged is not None:
            monkeypatch.setenv('DEXCT_P16_STAGED', staged)
        for step, mu, w, w2 in dr.case_tables(case, pl0):
            check_launches(pj, form, pl0, mu, w, w2, step, variance=form != 'wave_ray_kernel')
    print('MEASURED ' + '; '.join(f'{f} {k} {v:.3f}' for (f, k), v in sorted(_measured.items()) if f == form))


# ---- identical bits where the source promises them ---------------------------------------------------------------------------------

def launch(pj, mu, w, w2=None):
    """Counts (and, with w2, the sample and the variance) in the reference's order."""
    mu_d, w_d = dev(mu, w)
    if w2 is None:
        return pj.project_tables(mu_d, w_d, layout=0)
    return pj.project_tables(mu_d, w_d, layout=0, w2_d=dev(w2)[0], seed=SEED, want_variance=True)


@pytest.mark.parametrize('key,n_mat,n_e', [('rows64', 2, 139), ('rows64', 3, 300), ('rows66', 4, 139), ('rows64', 4, 7)])
def test_row_parallel_kernels_give_the_bits_of_the_ray_kernel(hip, key, n_mat, n_e):
    """siddon_detect.h: pairs of rays through v_pk_fma_f32, skipped zero-weight blocks, the air shortcut with its cache and the
    fused variance change no bit - kernels 3, 5 and 7 against kernel 1, the fused variance of kernel 7 against the separate loop of
    kernel 3, and the two-spectrum launch (masks and shortcut) against the first two of three spectra (neither), on every table."""
    pjs = {k: projector(key, n_mat, k) for k in (1, 3, 5, 7)}
    pl0 = dr.oracle_pathlen(key, n_mat)
    pu = dr.p_unit(pl0, n_mat)
    for step in dr.STEPS:
        mu, w, w2 = dr.sweep_tables(n_mat, n_e, 2, step, pu)
        ref = launch(pjs[1], mu, w)
        for k in (3, 5, 7):
            assert torch.equal(launch(pjs[k], mu, w), ref), (step, k)
        n7, v7 = launch(pjs[7], mu, w, w2)
        n3, v3 = launch(pjs[3], mu, w, w2)
        assert torch.equal(v7, v3) and torch.equal(n7, n3), step
        assert torch.equal(v3, launch(pjs[1], mu, w2)), step                 # and the variance is the sum with w2 as weights
        w3 = np.concatenate([w, dr.weights(n_e, 3)[2:]])
        for k in (3, 7):
            assert torch.equal(launch(pjs[k], mu, w3)[:2], ref), (step, k)


@pytest.mark.parametrize('n_mat,n_e', [(5, 139), (17, 7), (33, 64), (49, 64), (60, 7), (49, 300)])
def test_group_detection_gives_the_same_bits(hip, n_mat, n_e):
    """Kernel 8 (packed group codes) against kernel 4; beyond 48 table rows kernel 4 against kernel 1 (detect.hip:
    detect_kernel_chunked performs the operations of detect_store_lds in the same order), on every table."""
    key = 'rows64'
    pj4, pj8 = projector(key, n_mat, 4), projector(key, n_mat, 8)
    pj1 = projector(key, n_mat, 1) if n_mat > 48 else None
    pl0 = dr.oracle_pathlen(key, n_mat)
    pu = dr.p_unit(pl0, n_mat)
    for step in dr.STEPS:
        mu, w, w2 = dr.sweep_tables(n_mat, n_e, 2, step, pu)
        c4 = launch(pj4, mu, w)
        assert torch.equal(launch(pj8, mu, w), c4), step
        n4, v4 = launch(pj4, mu, w, w2)
        n8, v8 = launch(pj8, mu, w, w2)
        assert torch.equal(n8, n4) and torch.equal(v8, v4), step
        if pj1 is not None:
            assert torch.equal(launch(pj1, mu, w), c4), step


# ---- the log of counts at the edge of the float32 range ----------------------------------------------------------------------------

@pytest.mark.parametrize('air', [0.7, 3.0, 3.9, 150.0, 1e6])
def test_log_of_tiny_and_zero_counts(hip, air):
    """air * rcp(c) for hand-made counts from 0 through the denormals to 1e30, by dexct_sino_log and by dexct_transpose_log: +inf
    exactly where np.float32(air) / c is not finite, within the bound elsewhere."""
    pj = projector('row1', 2, 1)
    rng = np.random.default_rng(3)
    edge = np.array([0.0, 1e-45, 1e-40, 8.9e-39, 1.0e-38, 1.17e-38, 1.1754944e-38, 2e-38, 1e-30, 1e-20, 1e-3, 1.0, 3.0, 1e6, 1e30], F32)
    rows, cols = 64, 65
    c = (10.0 ** rng.uniform(-44.0, 8.0, (2, 1, rows, cols))).astype(F32)
    c[:, 0, :edge.size, 0] = edge
    c[:, 0, 0, :edge.size] = edge
    exact, bound = dr.log_ref([air, air], c)
    c_d = dev(c)[0]
    got = pj.sino_log(c_d, [air, air]).cpu().numpy().reshape(2, -1)
    assert dr.log_within(got, exact, bound), dr.log_worst(got, exact, bound)
    dst, lg = torch.empty((2, 1, cols, rows), device='cuda'), torch.empty((2, 1, cols, rows), device='cuda')
    pj.transpose_log(c_d, dst, lg, [air, air], rows, cols)
    assert torch.equal(dst, c_d.permute(0, 1, 3, 2))
    te, tb = dr.log_ref([air, air], dst.cpu().numpy())
    assert dr.log_within(lg.cpu().numpy().reshape(2, -1), te, tb)
    assert np.isinf(exact).any() and np.isfinite(exact).any()
