"""A/B of rows16_kernel's air-column map and absent-material detection (profiles/rows16_air_skip.md): the projection launch of
the benchmark scan (512^3, 1000 x 800 x 512, dual spectrum, log sinogram from the same store) under the knobs
DEXCT_P16_AIR_SKIP (0 / 2 / default) and DEXCT_DET_ABSENT (0 / 1), on three volumes: the benchmark
phantom, the same with its air turned to water (no air column) and the same with its bone turned to water (two table rows).
Every result is compared bit for bit with the first of its volume.  DEXCT_ROOT names the tree whose package is loaded (default:
this one), so that a build without the knobs - where they do nothing - is timed by the same script.

    python tools/probes/p16_air_skip.py [rounds]"""
import os
import sys

import torch

ROOT = os.environ.get('DEXCT_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import dex_ct_sim_amd as dx
from dex_ct_sim_amd import forward_project as fp, synthetic
from dex_ct_sim_amd.system import AIR, BONE, WATER

det = os.path.join(ROOT, 'dex-ct-sim_amd/input/detector/eta_eid_mv.bin')
n, views, chans = int(os.environ.get('N', 512)), int(os.environ.get('VIEWS', 1000)), int(os.environ.get('CHANS', 800))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ct = dx.FanBeamGeometry(N_channels=chans, N_proj=views, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True, detector_file=det, N_rows=n)
specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
log = torch.empty_like(out)
SETTINGS = [('0', '0'), ('2', '0'), ('0', '1'), ('2', '1'), (None, '1')]


def run(pj, mu_d, w_d, air, setting, reps=5):
    for name, v in zip(('DEXCT_P16_AIR_SKIP', 'DEXCT_DET_ABSENT'), setting):
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = v
    pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def study(name, ph):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    n_air = getattr(pj, 'n_air_columns', None)
    print(f'== {name}: {pj.n_mat} table rows, air columns {n_air} of {ph.Nx * ph.Ny}', flush=True)
    ref = None
    for rep in range(rounds):
        for s in SETTINGS:
            ms = run(pj, mu_d, w_d, air, s)
            if ref is None:
                ref = (out.clone(), log.clone())
            same = bool(torch.equal(out, ref[0]) and torch.equal(log.view(torch.int32), ref[1].view(torch.int32)))
            print(f'{name} round {rep} air_skip={s[0]} det_absent={s[1]}: {ms:.3f} ms  bit-identical: {same}', flush=True)
            assert same


ph = synthetic.make_phantom(n, n, extent=51.2, seed=1234)
which = os.environ.get('VOLUMES', 'benchmark,no-air,two-rows').split(',')
if 'benchmark' in which:
    study('benchmark phantom', ph)
if 'no-air' in which:
    vol = ph.volume.copy()
    vol[vol == 0] = 1
    study('no air columns', dx.VoxelPhantom.from_array('water-box', vol, [AIR, WATER, BONE], dx=ph.dx, dy=ph.dy, dz=ph.dz))
if 'two-rows' in which:
    vol = ph.volume.copy()
    vol[vol == 2] = 1
    study('two table rows', dx.VoxelPhantom.from_array('water-only', vol, [AIR, WATER], dx=ph.dx, dy=ph.dy, dz=ph.dz))
