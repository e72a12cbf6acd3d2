"""The quantum-noise samplers against the per-pixel float64 reference of tests/noise_refs.py: dexct_add_noise and
dexct_poisson_detect through the bare C ABI on plain torch tensors, and the samples a user receives through
Projector.project_tables / Projector.project.  Every kernel that is bit-compared with dexct_add_noise elsewhere in the suite
(the in-kernel samplers of the packed stacked fan, the cone beam and the material groups) is pinned through it.

Bounds (derived in the docstring of tests/noise_refs.py, which also holds the inputs; tests/test_noise_refs.py shows on the CPU
that each comparison used here rejects eleven kinds of subtly wrong sampler):
  Gaussian   |z_gpu - z_ref| <= 1e-3 (chosen for what it separates: the hardware's log, sqrt, sin and cos have no accuracy
             figure); through noisy_count sqrt(var) 1e-3 + 4 u (|mean| + sqrt(var) |z|), u = 2^-24
  Poisson    lambda_gpu = lambda_ref (1 +- eps), eps = 1.001 u (5 + sum_m (M - m + 2) mu_m pathlen_m), 0 where no material is
             crossed: 3.0e-7 .. 2.9e-5 on the attenuated inputs here (1.6e-5 where lambda > 1); the argument of the rounded
             normal's floor within delta = 1.001 u (24 sqrt(lambda) |z| + 2 (|lambda + sqrt(lambda) z| + 0.5)), at most 9.4e-4
             at lambda = 3e3; the float32 sum over the energies n_e u hi
Measured on the MI355X (the code under test - the bounds above are not taken from these):
  worst |z_gpu - z_ref| over every pixel of test_recover_z:  1.31e-6 (shape (5, 4, 67), spectrum 2, z = 2.82, u1 = 0.0173,
      u2 = 0.0239 revolutions - nowhere special; far below the 1e-4 that would be a finding)
  share of ambiguous bins (a window of more than one integer) over the attenuated inputs:  9.7e-4 at most (49 materials),
      2.7e-4 .. 4.0e-4 for 1 - 17 materials; 5.3e-5 on the projected small scan
"""
import functools

import numpy as np
import pytest
import torch

import noise_refs as nr
from conftest import small_scan

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def add_noise(lib, cnt, var, shape, layout, view_offset, seed):
    """dexct_add_noise in place on a copy of ``cnt`` [S][n_rays]; the float32 result."""
    from dex_ct_sim_amd._device import stream_ptr
    c, v = torch.tensor(cnt, device='cuda'), torch.tensor(var, device='cuda')
    rc = lib.dexct_add_noise(c.data_ptr(), v.data_ptr(), cnt.shape[0], shape[0], shape[1], shape[2], layout, view_offset, seed,
                             stream_ptr())
    assert rc == 0, rc
    return c.cpu().numpy()


def poisson_detect(lib, p):
    """dexct_poisson_detect on the problem ``p`` (the keyword arguments of noise_refs.poisson_detect_ref); [S][n_rays]."""
    from dex_ct_sim_amd._device import stream_ptr
    dev = {k: torch.tensor(p[k], device='cuda').contiguous() for k in ('pathlen', 'mu', 'photons', 'gain')}
    n_rays = p['n_views'] * p['n_rows'] * p['n_channels']
    out = torch.full((p['n_spectra'], n_rays), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.dexct_poisson_detect(dev['pathlen'].data_ptr(), dev['mu'].data_ptr(), dev['photons'].data_ptr(), dev['gain'].data_ptr(),
                                  p['n_materials'], p['n_energies'], p['n_spectra'], p['n_views'], p['n_rows'], p['n_channels'],
                                  p['layout'], p['view_offset'], p['seed'], out.data_ptr(), stream_ptr())
    assert rc == 0, rc
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def normals(shape, layout, view_offset, seed):
    v, r, c = nr.decode(shape, layout)
    return nr.pixel_normals_ref(v + view_offset, r, c, seed)


# ---- dexct_add_noise -----------------------------------------------------------------------------------------------------------

_z = dict(worst=0.0, where=None)


@pytest.mark.parametrize('shape', nr.SHAPES)
def test_recover_z(hip, shape):
    """mean = 16, variance = 1: the output minus 16 is the normal itself (float32 step 2e-6 there), every pixel of every spectrum
    within 1e-3 of pixel_normals_ref."""
    for S, layout, off, seed in nr.add_noise_cases(shape):
        cnt, var = nr.constant_inputs(S, shape, 16.0, 1.0)
        z = add_noise(hip, cnt, var, shape, layout, off, seed).astype(F64) - 16.0
        z_ref = normals(shape, layout, off, seed)[:S]
        d = np.abs(z - z_ref)
        if d.max() > _z['worst']:
            s, ray = np.unravel_index(np.argmax(d), d.shape)
            v, r, c = (a[ray] for a in nr.decode(shape, layout))
            w = nr.philox4x32_10(v + off, r, c, 0, *nr.seed_words(seed))
            _z.update(worst=float(d.max()), where=dict(shape=shape, spectrum=int(s), z_ref=float(z_ref[s, ray]),
                                                       u1_u2=[float(x) for x in nr.unit_pair(w[2 * (s // 2)], w[2 * (s // 2) + 1])]))
        assert nr.z_within(z, z_ref), (S, layout, off, seed, d.max())
    print(f'worst |z_gpu - z_ref| so far: {_z["worst"]:.3e} at {_z["where"]}')


@pytest.mark.parametrize('shape', nr.SHAPES)
def test_physical_values(hip, shape):
    worst = 0.0
    for S, layout, off, seed in nr.add_noise_cases(shape):
        cnt, var = nr.physical_inputs(S, shape)
        got = add_noise(hip, cnt, var, shape, layout, off, seed)
        ref, bound = nr.add_noise_ref(cnt, var, shape, layout, off, seed)
        worst = max(worst, nr.worst(got, ref, bound))
        assert nr.within(got, ref, bound), (S, layout, off, seed, nr.worst(got, ref, bound))
        assert not np.array_equal(got, cnt)
    print(f'{shape}: worst |got - ref| / bound = {worst:.3e}')


@pytest.mark.parametrize('shape', nr.SHAPES)
def test_clipping(hip, shape):
    """mean = 1, variance = 25: exactly 1e-20 where the reference is below minus its bound, within the bound above it, one of
    the two for the pixels in between (at most 0.1 % of all: tests/test_noise_refs.py::test_clipping_cap)."""
    clipped = 0
    for S, layout, off, seed in nr.add_noise_cases(shape):
        cnt, var = nr.constant_inputs(S, shape, 1.0, 25.0)
        got = add_noise(hip, cnt, var, shape, layout, off, seed)
        _, bound, raw = nr.add_noise_ref(cnt, var, shape, layout, off, seed, raw=True)
        assert nr.clip_ok(got, raw, bound), (S, layout, off, seed)
        clipped += int(np.count_nonzero(got == F32(nr.FLOOR)))
    assert clipped > 0 or shape == (1, 1, 1)


@pytest.mark.parametrize('shape', nr.SHAPES)
def test_degenerate_variances_and_nan_mean(hip, shape):
    """Variance 0, -1 and NaN return the mean bit for bit; a NaN mean becomes 1e-20 (include/dexct.h: fmaxf drops the NaN, the
    clip keeps every output finite and positive)."""
    for S, layout, off, seed in nr.add_noise_cases(shape):
        cnt, var = nr.physical_inputs(S, shape)
        for bad in (0.0, -1.0, np.nan):
            got = add_noise(hip, cnt, np.full(cnt.shape, bad, F32), shape, layout, off, seed)
            assert np.array_equal(got.view(np.int32), cnt.view(np.int32)), (S, layout, off, seed, bad)
        got = add_noise(hip, np.full(cnt.shape, np.nan, F32), var, shape, layout, off, seed)
        assert np.all(got == F32(nr.FLOOR)), (S, layout, off, seed)


def test_spectra_are_independent_on_the_device(hip):
    """The recovered normals of the (9, 4, 131) shape: every pair of spectra correlates below 0.05 (4 716 pixels: 3.4 standard
    deviations; the reference's own stay below 0.045 there), and no two spectra are equal."""
    shape = nr.SHAPES[-1]
    for _, layout, off, seed in [k for k in nr.add_noise_cases(shape) if k[0] == 4]:
        cnt, var = nr.constant_inputs(4, shape, 16.0, 1.0)
        z = add_noise(hip, cnt, var, shape, layout, off, seed).astype(F64) - 16.0
        corr = np.corrcoef(z)
        assert np.all(np.abs(corr[~np.eye(4, dtype=bool)]) < 0.05), (layout, off, seed, corr)
        for a in range(4):
            for b in range(a + 1, 4):
                assert not np.array_equal(z[a], z[b]) and np.abs(z[a] - z[b]).mean() > 0.5, (a, b)


def spectra(scale):
    from dex_ct_sim_amd import synthetic
    sp = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
    for s in sp:
        s.rescale_counts(scale)
    return sp


def test_project_tables_draws_the_reference_sample(hip):
    """What get_sino(noise=True) hands out, on a shard that starts at view 2: the packed stacked fan draws the sample in its
    registers, the 4-rows-per-lane kernel writes the variance and goes through dexct_add_noise.  Both noisy results are within the
    bound of add_noise_ref applied to the same projector's clean counts and the same call's variance."""
    from dex_ct_sim_amd import forward_project as fp
    ct, ph = small_scan(n=40, nz=16, n_views=7, n_channels=23, n_rows=16)
    sp = spectra(1.0)                                                        # ~1e6 photons per ray: the Gaussian regime
    _, mu, w, w2 = fp.merged_tables(ct, ph, sp, with_variance=True)
    seed = nr.SEEDS[1]
    for kernel, packed in ((7, True), (3, False)):
        pj = fp.Projector(ct, ph, kernel=kernel, view_range=(2, 7))
        assert pj.use_packed == packed
        mu_d, w_d, w2_d = (torch.tensor(x, dtype=torch.float32, device='cuda').contiguous() for x in (pj.compact(mu), w, w2))
        for layout in (0, 1):
            noisy, var = pj.project_tables(mu_d, w_d, layout=layout, w2_d=w2_d, seed=seed, want_variance=True)
            clean = pj.project_tables(mu_d, w_d, layout=layout)
            assert noisy.shape == ((2, 5, 16, 23) if layout == 0 else (2, 5, 23, 16))
            ref, bound = nr.add_noise_ref(clean.cpu().numpy(), var.cpu().numpy(), (5, 16, 23), layout, 2, seed)
            got = noisy.cpu().numpy().reshape(2, -1)
            print(f'kernel {kernel}, layout {layout}: worst |got - ref| / bound = {nr.worst(got, ref, bound):.3e}')
            assert nr.within(got, ref, bound), (kernel, layout, nr.worst(got, ref, bound))
            assert (var > 0).all() and not torch.equal(noisy, clean)


# ---- dexct_poisson_detect ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table', [0, 1])
@pytest.mark.parametrize('layout', [0, 1])
def test_per_bin_decode(hip, table, layout):
    """n_e = 3, gain = (1, 2^8, 2^16), pathlen = 0 (lambda = photons exactly), two spectra, photons 0.05 .. 60: every bin's draw is
    read off the signal and equals the reference's; only a rounded-normal bin within delta of a half may take either neighbour.
    Over the two tables every (spectrum, energy) takes both branches."""
    p = nr.unattenuated_problem(nr.DECODE_TABLES[table], layout=layout, view_offset=17, seed=nr.SEEDS[1])
    sig = poisson_detect(hip, p)
    lo, hi, ambiguous, detail = nr.poisson_detect_ref(**p)
    draws = nr.decode_draws(sig, p['gain'])
    assert draws is not None
    assert np.array_equal(draws[~detail['normal']], detail['k_lo'][~detail['normal']])          # inversion: the draw itself
    assert nr.decode_ok(sig, detail, p['gain']) and nr.poisson_within(sig, lo, hi, 3)
    assert ambiguous <= nr.AMBIGUOUS_CAP
    for s in range(2):
        for e in range(3):
            assert draws[s, :, e].std() > 0.0                                                     # (a bin that is always drawn)


def test_branch_boundary(hip):
    """photons = 30.0 takes the rounded normal, the float32 just below it the inversion, bin by bin."""
    p = nr.unattenuated_problem(nr.BOUNDARY_TABLE, layout=1, view_offset=17, seed=nr.SEEDS[1])
    sig = poisson_detect(hip, p)
    lo, hi, _, detail = nr.poisson_detect_ref(**p)
    assert nr.decode_ok(sig, detail, p['gain']) and nr.poisson_within(sig, lo, hi, 3)
    draws = nr.decode_draws(sig, p['gain'])
    assert np.array_equal(draws[~detail['normal']], detail['k_lo'][~detail['normal']])


def test_dark_bins(hip):
    """Zero and negative photons: no draw, the 1e-20 floor."""
    sig = poisson_detect(hip, nr.unattenuated_problem(nr.DARK_TABLE, view_offset=3))
    assert np.all(sig == F32(nr.FLOOR))


_ambiguous = []


@pytest.mark.parametrize('n_mat', nr.ATTENUATED_MATERIALS)
@pytest.mark.parametrize('layout', [0, 1])
def test_attenuated(hip, n_mat, layout):
    """48 energies, 3 spectra, (5, 4, 67), view_offset 17, an energy-integrating gain, lambda from 3e3 down to below 1e-3, through
    every register-array template: every (ray, spectrum) signal lies in the reference's interval."""
    p = nr.attenuated_problem(n_mat, layout)
    sig = poisson_detect(hip, p)
    lo, hi, ambiguous, _ = nr.poisson_detect_ref(**p)
    _ambiguous.append(ambiguous)
    print(f'{n_mat} materials, layout {layout}: ambiguous bins {ambiguous:.3e} (largest so far {max(_ambiguous):.3e}), '
          f'mean relative width of the intervals {np.mean((hi - lo) / hi):.3e}')
    assert ambiguous <= nr.AMBIGUOUS_CAP
    assert nr.poisson_within(sig, lo, hi, p['n_energies']), (n_mat, layout)
    assert len(np.unique(sig)) > 1000


def test_project_poisson_draws_the_reference_sample(hip):
    """Projector.project(noise='poisson') on a shard that starts at view 1, against poisson_detect_ref fed with the path lengths
    the same call returns and the tables the host hands the kernel."""
    from dex_ct_sim_amd import forward_project as fp
    ct, ph = small_scan(n=32, nz=4, n_views=6, n_channels=23, n_rows=4)
    sp = spectra(1e-2)                                                       # <= 300 photons per bin: both branches
    seed = nr.SEEDS[1]
    for kernel, layout in ((1, 0), (3, 1)):
        pj = fp.Projector(ct, ph, kernel=kernel, view_range=(1, 6))
        (counts, pathlen), _ = pj.project(sp, want_pathlen=True, layout=layout, noise='poisson', seed=seed)
        E, mu, w = fp.merged_tables(ct, ph, sp)
        mu_c = pj.compact(mu)
        lo, hi, ambiguous, detail = nr.poisson_detect_ref(
            pathlen.cpu().numpy(), mu_c.astype(F32), (w / E).astype(F32), E.astype(F32), mu_c.shape[0], E.size, 2, 5, 4, 23, layout,
            1, seed)
        lam = detail['lam'][detail['live']]
        print(f'kernel {kernel}: ambiguous bins {ambiguous:.3e}, lambda {lam.min():.2e} .. {lam.max():.2e}')
        assert ambiguous <= nr.AMBIGUOUS_CAP and lam.min() < 30.0 < lam.max()
        assert nr.poisson_within(counts.cpu().numpy().reshape(2, -1), lo, hi, E.size), kernel
