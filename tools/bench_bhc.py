#!/usr/bin/env python3
"""Beam-hardening correction on the MI355X: dexct_bhc_linearize on a configs[2]-sized stack (1000 views x 512 rows x 800
channels = 4.1e8 values) and on configs[0]'s 1200 x 800 sinogram - kernel time by device events and the effective
rate (8 B moved per value: 4 read, 4 written) - and get_recon at configs[0] (512^2, FOV 50 cm) with and without
``bhc='water'``.  One JSON line on stdout.

    python tools/bench_bhc.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import torch
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import bhc
    assert torch.cuda.is_available(), 'bench_bhc needs a HIP device'
    inp = os.path.join(ROOT, 'dex-ct-sim_amd', 'input')
    ct = dx.FanBeamGeometry(N_channels=800, N_proj=1200, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True,
                            detector_file=os.path.join(inp, 'detector', 'eta_eid_mv.bin'))
    spec = dx.xRaySpectrum(os.path.join(inp, 'spectrum', '80kV_1mGy_float32.bin'), '80kV')
    t0 = time.perf_counter()
    table = bhc.linearization_table(ct, spec, 'water')
    t_table = time.perf_counter() - t0
    res = {'table_nodes': table.n_nodes, 'table_build_s': round(t_table, 3)}
    g = torch.Generator(device='cuda').manual_seed(0)
    for name, shape in (('stack_1000x512x800', (1000, 512, 800)), ('sino_1200x800', (1200, 800))):
        p = torch.rand(shape, device='cuda', generator=g) * 12.0 - 0.5
        out = torch.empty_like(p)
        ms = kernel_time(lambda: bhc.linearize_device(p, table, out=out), args.reps)
        res[name] = {'n': p.numel(), 'ms': round(ms, 4), 'TB_per_s': round(8.0 * p.numel() / (ms * 1e-3) / 1e12, 3)}
        ms_ip = kernel_time(lambda: bhc.linearize_device(p, table, out=p), args.reps)
        res[name]['in_place_ms'] = round(ms_ip, 4)
        del p, out
        torch.cuda.empty_cache()
    # get_recon at configs[0]: host to host, as main.py calls it
    from dex_ct_sim_amd.back_project import get_recon
    rng = np.random.default_rng(1)
    sino = rng.uniform(0.0, 8.0, (ct.N_proj, ct.N_channels)).astype(np.float32)
    for key, kw in (('get_recon_ms', {}), ('get_recon_bhc_water_ms', {'bhc': 'water'})):
        get_recon(sino, ct, spec, 512, 50.0, 0.8, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            get_recon(sino, ct, spec, 512, 50.0, 0.8, **kw)
        torch.cuda.synchronize()
        res[key] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
