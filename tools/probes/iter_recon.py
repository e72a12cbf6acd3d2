#!/usr/bin/env python3
"""The matched projector pair and one SIRT iteration on the MI355X, by device events: 512^2 pixels over 50 cm, 1200 views x
800 channels, one slice and 64 stacked slices, with and without the in-plane transposed buffers (``layout``), against
filtered back-projection of the same shape.  The adjoint's added bytes are counted from the plan (4 B per non-zero
coefficient and slice).  One JSON line per case on stdout; profiles/iter_recon.md keeps the numbers.

    python tools/probes/iter_recon.py [--reps 5] [--slices 1 64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def event_ms(fn, reps):
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


def coefficients(proj):
    """Non-zero coefficients of one slice, counted from the device plan (fields of dexct_ray_plan, include/dexct.h)."""
    import torch
    plan = proj.plan.view(torch.int64).view(-1, 5)
    V0, SV = plan[:, 0], plan[:, 1]
    i_first, n_slabs = plan[:, 2] & 0xFFFFFFFF, plan[:, 2] >> 32
    axis = (plan[:, 4] >> 32) & 1
    nv = torch.where(axis == 0, proj.ny, proj.nx)
    total = 0
    for s in range(int(n_slabs.max())):
        live = s < n_slabs
        Va = V0 + (i_first + s) * SV
        ja, jb = Va >> 40, (Va + SV) >> 40
        a = live & (ja != jb) & (ja >= 0) & (ja < nv)
        b = live & (jb >= 0) & (jb < nv)
        total += int(a.sum()) + int(b.sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slices', type=int, nargs='+', default=[1, 64])
    args = ap.parse_args()
    import torch
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd.back_project import recon_device
    from dex_ct_sim_amd.iterative import ImageProjector, sirt
    assert torch.cuda.is_available(), 'iter_recon needs a HIP device'
    n, fov = 512, 50.0
    ct = dx.FanBeamGeometry(N_channels=800, N_proj=1200, gamma_fan=0.8230337, SID=60.0, SDD=100.0)
    g = torch.Generator(device='cuda').manual_seed(0)
    n_coef = None
    for n_slices in args.slices:
        x = torch.rand((n_slices, n, n), device='cuda', generator=g)
        fbp_ms = None
        for transposed in (True, False):
            p = ImageProjector(ct, n, fov, n_slices=n_slices, transposed=transposed)
            b = p.forward(x)
            if n_coef is None:
                n_coef = coefficients(p)
            if fbp_ms is None:
                fbp_ms = event_ms(lambda: recon_device(b, ct, n, fov, 1.0), args.reps)
            out_s, out_i = torch.empty_like(b), torch.empty_like(x)
            fwd = event_ms(lambda: p.forward(x, out=out_s), args.reps)
            adj = event_ms(lambda: p.adjoint(b, out=out_i), args.reps)
            p.row_sums(), p.col_sums()
            it = event_ms(lambda: sirt(b, p, 1, x0=x), args.reps)
            added = 4.0 * n_coef * n_slices
            print(json.dumps({'slices': n_slices, 'layout': 'transposed buffers' if transposed else 'image only',
                              'forward_ms': round(fwd, 3), 'adjoint_ms': round(adj, 3), 'sirt_iteration_ms': round(it, 3),
                              'fbp_ms': round(fbp_ms, 3), 'coefficients_per_slice': n_coef,
                              'adjoint_added_GB': round(added / 1e9, 3),
                              'adjoint_added_TB_per_s': round(added / (adj * 1e-3) / 1e12, 4)}), flush=True)
            del p, b, out_s, out_i
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
