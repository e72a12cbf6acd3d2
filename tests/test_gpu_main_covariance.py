"""``main.py --covariance``: the predicted noise covariance of a decomposed pair, written next to its basis sinograms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import INPUT, ROOT

pytestmark = pytest.mark.gpu


def test_main_writes_the_covariance_sinograms(hip, tmp_path):
    """One run of main.py on a tiny scan of the bundled 140 / 80 kV pair, no reconstruction.  The three files are the covariance
    get_basismat_covariance returns for the written basis sinograms: those are float32, so each state is off by up to 2^-24
    relative, every exponent a.mu(e) <= ~20 of an energy that counts by 1.2e-6, and the covariance by up to cond(corr) <= ~500
    times that: 1e-3 of sqrt(C_ii C_jj) is what the comparison can ask.  Air pixels hold 0."""
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import matdecomp as md
    params = json.load(open(os.path.join(INPUT, 'params.txt')))
    params.update({'RUN_ID': 'tiny', 'Nx': 48, 'Ny': 48, 'dx': 0.4, 'dy': 0.4, 'N_channels': 96, 'N_projections': 60,
                   'back_project': False})
    pf = tmp_path / 'params.txt'
    pf.write_text(json.dumps(params))
    main = os.path.join(ROOT, 'dex-ct-sim_amd', 'main.py')
    subprocess.run([sys.executable, main, '--params', str(pf), '--input-dir', INPUT, '--pairs', '140kV:80kV:5:5', '--n-iters', '30',
                    '--out', str(tmp_path / 'o'), '--covariance'], check=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    d = tmp_path / 'o' / 'tiny' / 'matdecomp_140kV_80kV_5000uGy_5000uGy'
    ct = dx.read_parameter_file(str(pf), base_dir=os.path.dirname(INPUT))[0][3]
    shape = (ct.N_proj, ct.N_channels)
    a1, a2 = (np.fromfile(d / f'mat{m}_sino_float32.bin', dtype=np.float32).reshape(shape) for m in (1, 2))
    c11, c12, c22 = (np.fromfile(d / f'cov{t}_sino_float32.bin', dtype=np.float32).reshape(shape).astype(np.float64)
                     for t in ('11', '12', '22'))
    raw0 = np.fromfile(tmp_path / 'o' / 'tiny' / '140kV_5000uGy' / 'sino_raw_float32.bin', dtype=np.float32).reshape(shape)
    air = raw0.astype(np.float64) >= 0.95 * float(raw0.max())
    assert air.any() and not air.all()
    assert not c11[air].any() and not c12[air].any() and not c22[air].any() and not a1[air].any()
    assert np.all(c11[~air] > 0.0) and np.all(c22[~air] > 0.0) and np.all(c12[~air] ** 2 < c11[~air] * c22[~air])
    specs = []
    for kv in (140, 80):
        sp = dx.xRaySpectrum(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV')
        sp.rescale_counts(ct.A_iso * 5.0 / ct.N_proj)
        specs.append(sp)
    cov = md.get_basismat_covariance(ct, (a1, a2), specs, mask_from=raw0)
    s1, s2 = np.sqrt(cov[..., 0][~air]), np.sqrt(cov[..., 2][~air])
    for got, t, scale in ((c11, 0, s1 * s1), (c12, 1, s1 * s2), (c22, 2, s2 * s2)):
        err = np.max(np.abs(got[~air] - cov[..., t][~air]) / scale)
        print(f'element {t}: {err:.2e} of sqrt(C_ii C_jj)')
        assert err <= 1e-3
