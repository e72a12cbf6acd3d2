"""How long does the general Newton kernel (csrc/gn_multi.hip, dexct_gn_decompose_multi) take at the reference's own scan size?
(K, M) = (3, 2) and (4, 3) on 1200 x 800 pixels, 136 energies, n_iters = 50: device events around the call, warmed up, the
default (a pixel ends when its update returns its own input) and the full loop (every iteration executed, so the work is known
exactly), beside the FP64 issue estimate: per pixel-iteration-energy one table exponential (M + 9 FP64 instructions) plus
K (1 + M + M (M + 1) / 2) FMAs, at 614.4 G wave-instructions per second (256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per FP64
instruction of a 64-lane wave).  Prints one line per configuration; profiles/gn_multi.md records them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import gn_multi_refs as mr
from dex_ct_sim_amd import matdecomp as md

VIEWS, CHANNELS, N_E, N_ITERS, REPS = 1200, 800, 136, 50, 7
ISSUE_RATE = 256 * 4 * 2.4e9 / 4 * 64          # FP64 lane-instructions per second

n_pix = VIEWS * CHANNELS
for K, M in ((3, 2), (4, 3)):
    g, i0, mus = mr.sweep_case(K, M, N_E, n_pix=n_pix)
    gd = torch.from_numpy(g.astype(np.float32).reshape(K, VIEWS, CHANNELS)).to('cuda')
    out = torch.empty((VIEWS, CHANNELS, M), dtype=torch.float64, device='cuda')
    n_used = int(np.count_nonzero(np.any(i0 != 0.0, axis=0)))
    per_energy = (M + 9) + K * (1 + M + M * (M + 1) // 2)
    floor_ms = 1e3 * n_pix * N_ITERS * n_used * per_energy / ISSUE_RATE
    results = {}
    for full in (False, True):
        ts = []
        for rep in range(2 + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            md.gn_device_multi(gd, i0, mus, N_ITERS, full_loop=full, out=out)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ts.append(e0.elapsed_time(e1))
        results[full] = (out.clone(), sorted(ts))
    same = torch.equal(results[False][0].view(torch.int64), results[True][0].view(torch.int64))
    finite = bool(torch.isfinite(results[True][0]).all())
    for full in (False, True):
        ts = results[full][1]
        line = (f'K={K} M={M} {n_pix} pixels {n_used} of {N_E} energies n_iters={N_ITERS} {"full loop" if full else "default  "}: '
                f'median {ts[len(ts) // 2]:.2f} ms (min {ts[0]:.2f}, max {ts[-1]:.2f}, {REPS} runs)')
        if full:
            line += f'; FP64 issue estimate {floor_ms:.2f} ms = {floor_ms / ts[len(ts) // 2]:.2f} of the measured time'
        print(line, flush=True)
    print(f'K={K} M={M}: default and full loop bit-identical: {same}; all finite: {finite}', flush=True)
