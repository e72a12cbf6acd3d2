#!/usr/bin/env python3
"""How noisy is a virtual monoenergetic sinogram, and at which energy is it least noisy?  Predicted against measured, for one
noisy scan of the bundled 140 / 80 kV pair.

The prediction is the per-pixel covariance of the decomposed line integrals (matdecomp.get_basismat_covariance, the delta
method on the Newton solve) at the noise-free decomposition, turned into the variance of ``u1(E) a1 + u2(E) a2`` per energy
(plots.vmi_noise_sweep).  The measurement is the sample variance of (noisy - noise-free) VMI line integrals over the pixels
behind the phantom, from ONE noisy scan.

    python examples/decomposition_noise.py [--n 128] [--views 360] [--channels 256] [--dose-hi 5] [--dose-lo 5] [--kind estimator]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dex_ct_sim_amd as dx                                   # noqa: E402
from dex_ct_sim_amd import matdecomp as md, plots, synthetic, xcompy   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128, help='phantom slice is n x n voxels over 25.6 cm')
    ap.add_argument('--views', type=int, default=360)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--dose-hi', type=float, default=5.0, help='dose of the 140 kV scan [mGy]')
    ap.add_argument('--dose-lo', type=float, default=5.0, help='dose of the 80 kV scan [mGy]')
    ap.add_argument('--kind', default='estimator', choices=['estimator', 'crlb'])
    args = ap.parse_args(argv)

    inp = os.path.join(ROOT, 'dex-ct-sim_amd', 'input')
    ct = dx.FanBeamGeometry(N_channels=args.channels, N_proj=args.views, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True,
                            detector_file=os.path.join(inp, 'detector', 'eta_eid_mv.bin'))
    phantom = synthetic.make_phantom(args.n, 1, extent=25.6)
    specs = []
    for kv, dose in ((140, args.dose_hi), (80, args.dose_lo)):
        sp = dx.xRaySpectrum(os.path.join(inp, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV')
        sp.rescale_counts(ct.A_iso * dose / ct.N_proj)         # photons per detector pixel and view (main.py:64-69)
        specs.append(sp)

    clean = [raw for raw, _ in dx.get_sinos(ct, phantom, specs)]
    noisy = [raw for raw, _ in dx.get_sinos(ct, phantom, specs, noise=True, seed=7)]
    a_clean = md.get_basismat_sinos(ct, clean[0], clean[1], specs[0], specs[1], n_iters=50)
    a_noisy = md.get_basismat_sinos(ct, noisy[0], noisy[1], specs[0], specs[1], n_iters=50)
    cov = md.get_basismat_covariance(ct, a_clean, specs, kind=args.kind, mask_from=clean[0])
    # the pixels behind the phantom in both scans (the air mask of either decomposition holds exact zeros)
    inside = (a_clean[0] != 0) & (a_noisy[0] != 0) & np.all(np.isfinite(cov), axis=-1)

    energies = np.arange(40.0, 141.0, 10.0)
    predicted, e_min = plots.vmi_noise_sweep(energies, cov, mask=inside)
    u1, u2 = xcompy.mixatten(md.matcomp1, energies), xcompy.mixatten(md.matcomp2, energies)
    d1, d2 = (a_noisy[0] - a_clean[0])[inside], (a_noisy[1] - a_clean[1])[inside]
    measured = np.array([np.var(u1[k] * d1 + u2[k] * d2) for k in range(energies.size)])
    print(f'{int(inside.sum())} pixels behind the phantom; kind = {args.kind}')
    print(' keV   predicted sd   measured sd   measured / predicted')
    for k, e in enumerate(energies):
        print(f'{e:4.0f}  {np.sqrt(predicted[k]):12.5f}  {np.sqrt(measured[k]):12.5f}  {np.sqrt(measured[k] / predicted[k]):10.3f}')
    print(f'least predicted noise at {e_min:.0f} keV, least measured noise at {energies[int(np.argmin(measured))]:.0f} keV')
    return predicted, measured


if __name__ == '__main__':
    main()
