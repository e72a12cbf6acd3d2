"""How long does the covariance kernel (csrc/gn_cov.hip, dexct_gn_covariance) take at the reference's own scan size?
(K, M) = (2, 2) and (4, 3) on 1200 x 800 pixels, 136 energies, both kinds: device events around the call (table kernel +
covariance kernel), warmed up, beside the FP64 issue estimate - per pixel and energy one table exponential (M + 9 FP64
instructions) plus K (M + 2) FMAs, at 614.4 G wave-instructions per second (256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per FP64
instruction of a 64-lane wave), the yardstick of profiles/gn_multi.md - and dexct_cov_quadform on the result.
Writes the table to profiles/gn_cov.md (or the path given as the first argument) and prints it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import gn_cov_refs as cr
from dex_ct_sim_amd import _native, matdecomp as md
from dex_ct_sim_amd._device import ptr, stream_ptr

VIEWS, CHANNELS, N_E, REPS = 1200, 800, 136, 9
ISSUE_RATE = 256 * 4 * 2.4e9 / 4 * 64          # FP64 lane-instructions per second


def timed(fn):
    ts = []
    for rep in range(2 + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gn_cov.md')
    lib = _native.load()
    n_pix = VIEWS * CHANNELS
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    rows, quad_rows = [], []
    for K, M in ((2, 2), (4, 3)):
        a, i0, i0v, mus = cr.sweep_case(K, M, N_E, n_pix=n_pix)
        n_used = int(np.count_nonzero(np.any(i0 != 0.0, axis=0) | np.any(i0v != 0.0, axis=0)))
        ad = torch.from_numpy(a.reshape(VIEWS, CHANNELS, M)).to('cuda')
        tabs = [torch.from_numpy(np.ascontiguousarray(x)).to('cuda') for x in (i0, i0v, mus)]
        T = M * (M + 1) // 2
        out = torch.empty((VIEWS, CHANNELS, T), dtype=torch.float64, device='cuda')
        per_energy = (M + 9) + K * (M + 2)
        floor_ms = 1e3 * n_pix * n_used * per_energy / ISSUE_RATE
        traffic_mb = n_pix * 8 * (M + T) / 1e6
        for kind in cr.KINDS:
            med, lo, hi = timed(lambda: md.gn_covariance_device(ad, tabs[0], tabs[1], tabs[2], kind, out=out))
            finite = bool(torch.isfinite(out).all())
            rows.append(f'| ({K}, {M}) | {kind} | {n_used} of {N_E} | {med:.3f} | {lo:.3f} | {hi:.3f} | {per_energy} | {floor_ms:.3f} | '
                        f'{med / floor_ms:.2f} | {traffic_mb:.1f} | {finite} |')
        var = torch.empty((VIEWS, CHANNELS), dtype=torch.float64, device='cuda')
        u = np.ascontiguousarray(mus[:, N_E // 2])
        med, lo, hi = timed(lambda: _native.check(lib.dexct_cov_quadform(ptr(out), n_pix, M, u.ctypes.data, ptr(var), stream_ptr()),
                                                  'dexct_cov_quadform'))
        quad_rows.append(f'| {M} | {med:.3f} | {lo:.3f} | {hi:.3f} | {n_pix * 8 * (T + 1) / 1e6:.1f} | {n_pix * 8 * (T + 1) / med / 1e6:.0f} |')
    text = '\n'.join([
        '# The covariance kernel (`gn_cov.hip`): first timings beside the FP64 issue estimate', '',
        f'Written by `tools/probes/gn_cov.py` on one {arch} device (the runtime names it "{torch.cuda.get_device_name(0)}"):',
        f'{VIEWS} x {CHANNELS} = {n_pix} pixels, the synthetic',
        f'spectral tables of `tests/gn_cov_refs.py` on {N_E} energies (energy-integrating variance weights), states uniform in',
        f'[0, A_MAX], no mask.  Device events around `gn_covariance_device` with a preallocated output (table kernel + covariance',
        f'kernel + the workspace allocation of the Python layer), 2 warm-up calls, {REPS} timed calls per line, one session.', '',
        'The estimate: per pixel and energy one table exponential (M + 9 FP64 instructions) and K (M + 2) FMAs, at 614.4 G',
        'wave-instructions/s (`profiles/gn_multi.md`, section 2).  Memory traffic: the states read and the triangle written.', '',
        '| (K, M) | kind | energies kept | median ms | min | max | FP64 instructions per energy | estimate ms | measured / estimate | traffic MB | all finite |',
        '|---|---|---|---|---|---|---|---|---|---|---|', *rows, '',
        '`dexct_cov_quadform` on the result (reads the triangle, writes one double per pixel):', '',
        '| M | median ms | min | max | traffic MB | GB/s |', '|---|---|---|---|---|---|', *quad_rows, '',
        'Not measured: hardware counters, the kernel with a mask, float32 mask counts, other sizes.', ''])
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
