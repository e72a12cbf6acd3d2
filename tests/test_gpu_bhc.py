"""HIP beam-hardening correction (dexct_bhc_linearize) against the host table, and get_recon / main.py with ``bhc``."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import INPUT, ROOT
from oracle import fbp_oracle as fo
from test_bhc import bisect_inverse, log_signal, scanner, spectrum
from test_fbp_oracle import disc_sino

pytestmark = pytest.mark.gpu


def special_values(rng, n):
    p = rng.uniform(-1.5, 45.0, n).astype(np.float32)
    p[::7] = rng.uniform(-1e-3, 1e-3, p[::7].size)
    p[::11] = rng.uniform(50.0, 200.0, p[::11].size)          # beyond the table
    p[::13] = rng.uniform(-5.0, -1.0, p[::13].size)
    p[3::17] = 0.0
    p[5::19] = np.inf
    p[6::23] = -np.inf
    p[8::29] = np.nan
    return p


@pytest.mark.parametrize('spec_id,material', [('80kV', 'water'), ('140kV', 'bone'), ('detunedMV', 'water')])
def test_kernel_matches_host_table(hip, spec_id, material):
    import torch
    from dex_ct_sim_amd import bhc
    ct, spec = scanner(), spectrum(spec_id)
    t = bhc.linearization_table(ct, spec, material)
    w, mu = log_signal(ct, spec, material)
    rng = np.random.default_rng(3)
    for shape in [(100003,), (360, 257), (90, 3, 129), (1,), (5,)]:
        p = special_values(rng, int(np.prod(shape))).reshape(shape)
        ref = t.evaluate(p)
        d = torch.tensor(p, device='cuda')
        got = bhc.linearize_device(d, t).cpu().numpy()
        fin = np.isfinite(p)
        assert np.array_equal(np.isnan(got), np.isnan(p))
        assert np.array_equal(got[np.isinf(p)], p[np.isinf(p)])
        assert np.all(np.isfinite(got[fin]))
        assert np.max(np.abs(got[fin] - ref[fin]) - 4e-7 * np.abs(ref[fin]), initial=0.0) <= 1e-9
        inside = fin & (p >= -1) & (p <= 40)
        exact = t.mu_ref * bisect_inverse(w, mu, p[inside].astype(np.float64))[0]
        assert np.max(np.abs(got[inside] - exact) - 1e-6 * np.abs(exact), initial=0.0) <= 1e-9
        # in place equals out of place bit for bit
        bhc.linearize_device(d, t, out=d)
        assert np.array_equal(d.cpu().numpy().view(np.uint32), got.view(np.uint32))
    # a view at element offset 1 (unaligned start, n not a multiple of 4), in place and out of place
    base = torch.tensor(special_values(rng, 4099), device='cuda')
    v = base[1:]
    ref = t.evaluate(v.cpu().numpy())
    out = bhc.linearize_device(v, t).cpu().numpy()
    fin = np.isfinite(ref)
    assert np.max(np.abs(out[fin] - ref[fin]) - 4e-7 * np.abs(ref[fin]), initial=0.0) <= 1e-9
    bhc.linearize_device(v, t, out=v)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), out.view(np.uint32))


def test_argument_checks(hip):
    import torch
    from dex_ct_sim_amd import _native, bhc
    lib = hip
    t = bhc.linearization_table(scanner(), spectrum('80kV'), 'water')
    tab = t.device(torch.device('cuda'))
    x = torch.zeros(16, device='cuda')
    P, T = x.data_ptr(), tab.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    E, K, OP, ON = t.log2_min, t.cells_log2, t.oct_pos, t.oct_neg
    ok = lib.dexct_bhc_linearize(P, 16, T, E, K, OP, ON, P, st)
    assert ok == 0
    assert lib.dexct_bhc_linearize(P, 0, T, E, K, OP, ON, P, st) == 0
    bad = [(None, 16, T, E, K, OP, ON, P), (P, 16, None, E, K, OP, ON, P), (P, 16, T, E, K, OP, ON, None),
           (P, -1, T, E, K, OP, ON, P), (P, 16, T, E, -1, OP, ON, P), (P, 16, T, E, 13, OP, ON, P),
           (P, 16, T, E, K, -1, ON, P), (P, 16, T, E, K, OP, -1, P), (P, 16, T, -101, K, OP, ON, P),
           (P, 16, T, 90, K, 20, ON, P), (P, 16, T, E, 8, OP, ON, P)]        # the last: 12290 nodes > 8192
    for args in bad:
        assert lib.dexct_bhc_linearize(*args, st) == -1, args
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        bhc.linearize_device(torch.zeros(4, 4, device='cuda').t(), t)
    assert _native.SYMBOLS.count('dexct_bhc_linearize') == 1


@pytest.mark.parametrize('case', ['full', 'short', 'stack'])
def test_get_recon_bhc_matches_oracle(hip, case):
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import back_project as bp, bhc
    if case == 'short':
        n_views, theta = 240, np.pi + 0.8230337 + 0.05
    else:
        n_views, theta = 360, 2 * np.pi
    ct = scanner(N_channels=257, N_proj=n_views, gamma_fan=0.8230337, SID=60.0, SDD=100.0, theta_tot=theta,
                 N_rows=3 if case == 'stack' else 1)
    spec = spectrum('80kV')
    w, mu = log_signal(ct, spec, 'water')
    _, P = bisect_inverse(w, mu, np.zeros(1))
    L = disc_sino(ct.thetas, ct.gammas, [(0.0, 0.0, 10.0, 1.0), (4.0, -2.0, 2.0, 1.5)])
    s = P(L.ravel()).reshape(L.shape).astype(np.float32)
    if case == 'stack':
        s = np.stack([s, 0.5 * s, 1.5 * s], axis=1)
    raw, hu = dx.get_recon(s, ct, spec, 128, 30.0, 0.8, bhc='water')
    lin = bhc.linearize(s, ct, spec, 'water')
    mu_w = bp.water_mu(ct, spec)
    rows = [lin[:, r, :] for r in range(lin.shape[1])] if case == 'stack' else [lin]      # the oracle is 2-D
    ref = np.stack([fo.get_recon(x, ct.thetas, ct.gammas, 60.0, 128, 30.0, 0.8, mu_water=mu_w,
                                 theta_tot=None if case != 'short' else ct.theta_tot)[0] for x in rows])
    ref = ref if case == 'stack' else ref[0]
    assert raw.shape == ref.shape
    assert np.max(np.abs(raw - ref)) < 2e-5 * np.abs(ref).max()
    assert np.allclose(hu, 1000.0 * (raw - mu_w) / mu_w, atol=1e-3)
    # a prebuilt table gives the same image; bhc=None is bit-identical to no keyword
    raw_t, _ = dx.get_recon(s, ct, spec, 128, 30.0, 0.8, bhc=bhc.linearization_table(ct, spec, 'water'))
    assert np.array_equal(raw_t, raw)
    a, ah = dx.get_recon(s, ct, spec, 128, 30.0, 0.8, bhc=None)
    b, bh = dx.get_recon(s, ct, spec, 128, 30.0, 0.8)
    assert np.array_equal(a, b) and np.array_equal(ah, bh)


def test_project_then_reconstruct_with_water_bhc(hip):
    """Water cylinder with a bone insert, projected with the bundled 80 kV spectrum and reconstructed with water BHC:
    the water around the centre reads 0 HU (measured on the MI355X: -0.70 HU; -715.8 HU without BHC)."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import system
    n = 128
    c = (np.arange(n) - n / 2 + 0.5) * 0.2
    x, y = np.meshgrid(c, c)
    vol = np.zeros((1, n, n), dtype=np.uint8)
    vol[0][x ** 2 + y ** 2 < 10.0 ** 2] = 1
    vol[0][(x - 5.0) ** 2 + (y - 2.0) ** 2 < 1.5 ** 2] = 2
    ph = dx.VoxelPhantom.from_array('water_bone', vol, [system.AIR, system.WATER, system.BONE], dx=0.2)
    ct = scanner(N_channels=300, N_proj=400, gamma_fan=0.8230337, SID=60.0, SDD=100.0)
    spec = spectrum('80kV')
    spec.rescale_counts(1e8)
    _, log = dx.get_sino(ct, ph, spec)
    _, hu = dx.get_recon(log, ct, spec, n, 25.6, 1.0, bhc='water')
    _, hu0 = dx.get_recon(log, ct, spec, n, 25.6, 1.0)
    roi = (np.abs(x + 2.0) < 2.0) & (np.abs(y + 2.0) < 2.0)
    got, got0 = float(hu[roi].mean()), float(hu0[roi].mean())
    print(f'central water ROI: {got:.2f} HU with water BHC, {got0:.1f} HU without')
    assert abs(got) < 5.0
    assert abs(got0) > 100.0
    _, noisy = dx.get_sino(ct, ph, spec, noise=True, seed=5)
    _, hun = dx.get_recon(noisy, ct, spec, n, 25.6, 1.0, bhc='water')
    assert np.all(np.isfinite(hun))


def test_main_writes_bhc_images(hip, tmp_path):
    import json
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd.back_project import get_recon
    params = json.load(open(os.path.join(INPUT, 'params.txt')))
    params.update({'RUN_ID': 'tiny', 'Nx': 48, 'Ny': 48, 'dx': 0.4, 'dy': 0.4, 'N_channels': 96, 'N_projections': 60,
                   'N_recon_matrix': 48, 'FOV_recon': 20.0})
    pf = tmp_path / 'params.txt'
    pf.write_text(json.dumps(params))
    main = os.path.join(ROOT, 'dex-ct-sim_amd', 'main.py')
    base = [sys.executable, main, '--params', str(pf), '--input-dir', INPUT, '--pairs', 'detunedMV:80kV:9:1',
            '--n-iters', '5']
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ['--out', str(tmp_path / 'a'), '--bhc', 'water', 'bone'], check=True, env=env, timeout=600)
    subprocess.run(base + ['--out', str(tmp_path / 'b')], check=True, env=env, timeout=600)
    files_a = sorted(str(p.relative_to(tmp_path / 'a')) for p in (tmp_path / 'a').rglob('*') if p.is_file())
    files_b = sorted(str(p.relative_to(tmp_path / 'b')) for p in (tmp_path / 'b').rglob('*') if p.is_file())
    extra = sorted(set(files_a) - set(files_b))
    assert set(files_b) <= set(files_a)
    assert not any('BHC' in f for f in files_b)
    for spec_dir in ('detunedMV_9000uGy', '80kV_1000uGy'):
        for m in ('water', 'bone'):
            for u in ('raw', 'HU'):
                assert os.path.join('tiny', spec_dir, f'recon_{m}BHC_{u}_float32.bin') in extra
    assert len(extra) == 8
    # the images are get_recon(bhc=...) of the written log sinogram; the plain files are unchanged by --bhc
    all_params = dx.read_parameter_file(str(pf), base_dir=os.path.dirname(INPUT))
    ct = all_params[0][3]
    from dex_ct_sim_amd import plots
    for spec_id, dose in (('detunedMV', 9.0), ('80kV', 1.0)):
        d = tmp_path / 'a' / 'tiny' / f'{spec_id}_{int(dose * 1000):04}uGy'
        spec = dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{spec_id}_1mGy_float32.bin'), spec_id)
        spec.rescale_counts(ct.A_iso * dose / ct.N_proj)
        log = np.fromfile(d / 'sino_log_float32.bin', dtype=np.float32).reshape(ct.N_proj, ct.N_channels)
        for m in ('water', 'bone'):
            raw, hu = get_recon(log, ct, spec, 48, 20.0, params['ramp_filter_percent_Nyquist'], bhc=m)
            assert np.array_equal(np.fromfile(d / f'recon_{m}BHC_raw_float32.bin', dtype=np.float32), raw.ravel())
            assert np.array_equal(np.fromfile(d / f'recon_{m}BHC_HU_float32.bin', dtype=np.float32), hu.ravel())
            img = plots.get_img_ct_BHC('', spec_id, dose, units='HU', N_matrix=48, out_dir=str(tmp_path / 'a'),
                                       run_prefix='tiny', bhc=m)
            assert np.array_equal(img, hu)
        for f in ('sino_log_float32.bin', 'recon_raw_float32.bin', 'recon_HU_float32.bin'):
            b = tmp_path / 'b' / 'tiny' / f'{spec_id}_{int(dose * 1000):04}uGy' / f
            assert (d / f).read_bytes() == b.read_bytes(), f
