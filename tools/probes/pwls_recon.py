#!/usr/bin/env python3
"""One iteration of the joint PWLS reconstruction on the MI355X, by device events: 512^2 pixels over 50 cm, 1000 views x 800
channels, K = 2 channels, one subset and ten, and the share of the four kernels of csrc/pwls.hip in it against the projector
pair.  Every figure is the median of ``--reps`` timed runs after one warm-up, each run bracketed by its own pair of events; the
parts are timed alone, back to back, on the buffers of the iteration.  One JSON line per subset count on stdout; DESIGN.md
section 4.10 keeps the numbers.

    python tools/probes/pwls_recon.py [--reps 7] [--subsets 1 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def event_ms(fn, reps, inner=1):
    """ms per call: the median over ``reps`` runs, one event pair around ``inner`` calls each (a kernel of microseconds is
    called often enough that the window is not the launch alone)"""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--subsets', type=int, nargs='+', default=[1, 10])
    args = ap.parse_args()
    import torch
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import _native
    from dex_ct_sim_amd._device import stream_ptr
    from dex_ct_sim_amd.iterative import ImageProjector, precision_weights, pwls
    assert torch.cuda.is_available(), 'pwls_recon needs a HIP device'
    n, fov, K = 512, 50.0, 2
    ct = dx.FanBeamGeometry(N_channels=800, N_proj=1000, gamma_fan=0.8230337, SID=60.0, SDD=100.0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    p = ImageProjector(ct, n, fov)
    x = torch.rand((K, 1, n, n), device='cuda', generator=gen)
    b = torch.stack([p.forward(x[k]) for k in range(K)])
    sd = 0.02 + 0.04 * torch.rand((2,) + tuple(p.sino_shape), device='cuda', generator=gen, dtype=torch.float64)
    cov = torch.stack([sd[0] ** 2, -0.9 * sd[0] * sd[1], sd[1] ** 2], dim=-1).contiguous()
    lib = _native.load()
    w = precision_weights(cov)
    n_rays = b[0].numel()
    R = p.row_sums()
    m = torch.empty_like(b)
    y, g, d = torch.empty_like(x), torch.rand_like(x), torch.rand_like(x)
    ax = b.clone()
    beta, delta = (C.c_double * K)(0.5, 0.5), (C.c_double * K)(0.01, 0.01)
    line = p.n_rows * p.n_channels

    prec = event_ms(lambda: lib.dexct_cov_precision(cov.data_ptr(), n_rays, K, 0.0, w.data_ptr(), stream_ptr()), args.reps, 50)
    maj = event_ms(lambda: lib.dexct_pwls_majorizer(w.data_ptr(), R.data_ptr(), n_rays, K, m.data_ptr(), stream_ptr()), args.reps, 50)
    upd = event_ms(lambda: lib.dexct_pwls_update(x.data_ptr(), g.data_ptr(), d.data_ptr(), K, 1, n, n, 1.0, beta, delta, 0,
                                                 y.data_ptr(), None, stream_ptr()), args.reps, 50)
    for S in args.subsets:
        def residuals():
            for s in range(S):
                off = 4 * s * line
                lib.dexct_pwls_residual(b.data_ptr() + off, ax.data_ptr() + off, w.data_ptr() + off, R.data_ptr() + off, n_rays, K,
                                        p.n_views - s, S, line, ax.data_ptr() + off, None, stream_ptr())

        def pair():
            for s in range(S):
                for k in range(K):
                    p.forward(x[k], views=(s, p.n_views, S), out=ax[k])
                for k in range(K):
                    p.adjoint(ax[k], views=(s, p.n_views, S), out=g[k])

        p.forget_weights()                 # w was rewritten through its pointer above (with the same values, but say so)
        pwls(b, w, p, 1, S, 0.5, 0.01, x0=x)                                   # the majoriser of w is cached from here on
        it = event_ms(lambda: pwls(b, w, p, 1, S, 0.5, 0.01, x0=x), args.reps)
        res, pr_ms = event_ms(residuals, args.reps, 10), event_ms(pair, args.reps)
        new = res + S * upd
        print(json.dumps({'subsets': S, 'iteration_ms': round(it, 3), 'projector_pair_ms': round(pr_ms, 3),
                          'residual_ms': round(res, 3), 'update_ms': round(S * upd, 3),
                          'new_kernels_share_of_iteration': round(new / it, 4),
                          'once_per_weights_ms': {'precision': round(prec, 3), 'majorizer': round(maj, 3)},
                          'rays': n_rays, 'pixels': n * n, 'channels': K, 'reps': args.reps}), flush=True)


if __name__ == '__main__':
    main()
