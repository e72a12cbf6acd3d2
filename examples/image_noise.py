#!/usr/bin/env python3
"""How noisy is a virtual monoenergetic IMAGE, pixel by pixel?  Predicted without a single noisy scan, next to the sample
standard deviation over a few hundred noisy scans, for the bundled 140 / 80 kV pair.

The prediction: the scan is decomposed noise-free, matdecomp.get_basismat_covariance gives the covariance of the two
basis-material line integrals per detector pixel (delta method), back_project.get_recon_covariance propagates it through the
FBP - exactly, the FBP is linear - and plots.vmi_noise_map turns the image-domain covariance into the standard deviation of the
VMI at one energy, in HU.  The measurement: ``--scans`` noisy scans (get_sinos(noise=True, seed=k)), each decomposed and
reconstructed, the sample standard deviation of their VMIs per pixel.  Their ratio is printed for the water pixels of the
phantom.  The delta method is first-order: the agreement is within the sampling error (1 / sqrt(2 scans) per pixel) at the
default dose and degrades as the dose goes down.  The map is pixel-wise: neighbouring pixels are correlated, so it does not give
the noise of an ROI mean.

    python examples/image_noise.py [--scans 200] [--energy 70] [--n 64] [--views 180] [--channels 128] [--matrix 64] [--dose 5]
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
    ap.add_argument('--scans', type=int, default=200, help='noisy scans for the sample standard deviation')
    ap.add_argument('--energy', type=float, default=70.0, help='energy of the VMI [keV]')
    ap.add_argument('--n', type=int, default=64, help='phantom slice is n x n voxels over 25.6 cm')
    ap.add_argument('--views', type=int, default=180)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--matrix', type=int, default=64, help='reconstruction matrix over 26 cm')
    ap.add_argument('--dose', type=float, default=5.0, help='dose of each of the two scans [mGy]')
    args = ap.parse_args(argv)

    inp = os.path.join(ROOT, 'dex-ct-sim_amd', 'input')
    ct = dx.FanBeamGeometry(N_channels=args.channels, N_proj=args.views, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True,
                            detector_file=os.path.join(inp, 'detector', 'eta_eid_mv.bin'))
    phantom = synthetic.make_phantom(args.n, 1, extent=25.6)
    specs = []
    for kv in (140, 80):
        sp = dx.xRaySpectrum(os.path.join(inp, 'spectrum', f'{kv}kV_1mGy_float32.bin'), f'{kv}kV')
        sp.rescale_counts(ct.A_iso * args.dose / ct.N_proj)    # photons per detector pixel and view (main.py:64-69)
        specs.append(sp)
    N, fov, ramp = args.matrix, 26.0, 0.8
    E = np.array([args.energy])
    u1, u2 = float(xcompy.mixatten(md.matcomp1, E)[0]), float(xcompy.mixatten(md.matcomp2, E)[0])
    uw = float(xcompy.mixatten(plots.WATER, E)[0])

    def vmi_hu(sinos):
        a1, a2 = md.get_basismat_sinos(ct, sinos[0][0], sinos[1][0], specs[0], specs[1], n_iters=50)
        m1, m2 = (dx.get_recon(a, ct, specs[0], N, fov, ramp)[0].astype(np.float64) for a in (a1, a2))
        return (a1, a2), 1000.0 * (u1 * m1 + u2 * m2 - uw) / uw

    clean = dx.get_sinos(ct, phantom, specs)
    a_clean, vmi_clean = vmi_hu(clean)
    cov = md.get_basismat_covariance(ct, a_clean, specs, mask_from=clean[0][0])
    cov_img = dx.get_recon_covariance(cov, ct, N, fov, ramp)
    predicted = plots.vmi_noise_map(cov_img, args.energy)                  # HU

    mean, m2 = np.zeros((N, N)), np.zeros((N, N))                          # Welford, per pixel
    for k in range(args.scans):
        _, v = vmi_hu(dx.get_sinos(ct, phantom, specs, noise=True, seed=k + 1))
        d = v - mean
        mean += d / (k + 1)
        m2 += d * (v - mean)
    measured = np.sqrt(m2 / (args.scans - 1))

    water = np.abs(vmi_clean) < 30.0                                       # the water pixels of the noise-free VMI
    ratio = measured[water] / predicted[water]
    print(f'{args.energy:.0f} keV VMI, {args.scans} noisy scans, {int(water.sum())} water pixels of {N} x {N}')
    print(f'predicted sd [HU]: median {np.median(predicted[water]):.2f}, range {predicted[water].min():.2f} .. {predicted[water].max():.2f}')
    print(f'measured  sd [HU]: median {np.median(measured[water]):.2f}')
    print(f'measured / predicted over the water pixels: mean {ratio.mean():.3f}, sd {ratio.std():.3f} '
          f'(sampling alone: sd {1.0 / np.sqrt(2.0 * (args.scans - 1)):.3f})')
    print(f'bias of the noisy VMIs against the noise-free one in water: {np.mean((mean - vmi_clean)[water]):+.2f} HU')
    return predicted, measured


if __name__ == '__main__':
    main()
