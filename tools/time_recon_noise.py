#!/usr/bin/env python3
"""Times of the noise propagation through the FBP (csrc/fbp_var.hip) next to the FBP itself, kernel by kernel, on one shape in one
process: device events around each entry point, warm, the median of ``--runs`` runs.

    python tools/time_recon_noise.py                                # 1000 views x 800 channels -> 512^2, T = 3, 1 row and 64 rows
    python tools/time_recon_noise.py --rows 8 --planes 6 --out t.json

Prints one JSON line per row count: milliseconds of dexct_fbp_var_filter / dexct_fbp_var_backproject and of dexct_fbp_filter /
dexct_fbp_backproject, and their ratios.  The geometry of a (pixel, view) pair is shared by the T planes: a variance back-projection
that costs more than T x the FBP's is not sharing it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, runs, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--views', type=int, default=1000)
    ap.add_argument('--channels', type=int, default=800)
    ap.add_argument('--matrix', type=int, default=512)
    ap.add_argument('--planes', type=int, default=3)
    ap.add_argument('--rows', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--runs', type=int, default=21)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args(argv)
    import torch
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import _native, back_project as bp
    from dex_ct_sim_amd._device import device, ptr, stream_ptr, to_dev
    lib, dev = _native.load(), device()
    ct = dx.FanBeamGeometry(N_channels=args.channels, N_proj=args.views)
    N, fov, T = args.matrix, 50.0, args.planes
    taps = bp.ramp_taps(ct.N_channels, ct.dgamma, 0.8)
    weight = ct.SID * np.cos(ct.gammas)
    taps64, weight64 = to_dev(taps, torch.float64, dev), to_dev(weight, torch.float64, dev)
    taps32, weight32 = to_dev(taps, torch.float32, dev), to_dev(weight, torch.float32, dev)
    view_cs = to_dev(ct.view_cs(), torch.float64, dev)
    dbeta = ct.theta_tot / ct.N_proj
    for rows in args.rows:
        gen = torch.Generator(device=dev).manual_seed(rows)
        cov = torch.rand((ct.N_proj, rows, ct.N_channels, T), dtype=torch.float64, device=dev, generator=gen) + 0.5
        qa, qb = torch.empty_like(cov), torch.empty_like(cov)
        img64 = torch.empty((rows, N, N, T), dtype=torch.float64, device=dev)
        sino = cov[..., 0].to(torch.float32).contiguous()
        q = torch.empty_like(sino)
        img32 = torch.empty((rows, N, N), dtype=torch.float32, device=dev)
        st = stream_ptr()

        def chk(rc, what):
            _native.check(rc, what)

        steps = {
            'var_filter': lambda: chk(lib.dexct_fbp_var_filter(ptr(cov), ct.N_proj, rows, ct.N_channels, T, ptr(taps64), ptr(weight64),
                                                               ct.dgamma, 2 * np.pi, 0, ct.N_proj, ptr(qa), ptr(qb), st), 'var_filter'),
            'var_backproject': lambda: chk(lib.dexct_fbp_var_backproject(ptr(qa), ptr(qb), ptr(view_cs), ct.N_proj, ct.N_channels, rows,
                                                                         T, ct.SID, ct.dgamma, dbeta, N, fov, ptr(img64), st),
                                           'var_backproject'),
            'fbp_filter': lambda: chk(lib.dexct_fbp_filter(ptr(sino), ptr(taps32), ptr(weight32), ct.N_proj * rows, ct.N_channels,
                                                           ct.dgamma, ptr(q), st), 'fbp_filter'),
            'fbp_backproject': lambda: chk(lib.dexct_fbp_backproject(ptr(q), ptr(view_cs), ct.N_proj, ct.N_channels, rows, ct.SID,
                                                                     ct.dgamma, dbeta, N, fov, ptr(img32), st), 'fbp_backproject'),
        }
        res = {'views': ct.N_proj, 'channels': ct.N_channels, 'matrix': N, 'planes': T, 'rows': rows, 'runs': args.runs}
        for name, fn in steps.items():
            med, lo, hi = median_ms(fn, args.runs, args.warmup)
            res[name + '_ms'] = round(med, 4)
            res[name + '_range_ms'] = [round(lo, 4), round(hi, 4)]
        res['filter_ratio'] = round(res['var_filter_ms'] / res['fbp_filter_ms'], 2)
        res['backproject_ratio'] = round(res['var_backproject_ms'] / res['fbp_backproject_ms'], 2)
        res['total_ratio'] = round((res['var_filter_ms'] + res['var_backproject_ms']) / (res['fbp_filter_ms'] + res['fbp_backproject_ms']), 2)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        del cov, qa, qb, img64, sino, q, img32
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
