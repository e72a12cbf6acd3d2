#!/usr/bin/env python3
"""Does the covariance of the decomposition buy a better image?  One noisy dual-energy scan of the synthetic phantom (the
bundled 140 / 80 kV pair) is decomposed into the two basis-material sinograms, matdecomp.get_basismat_covariance predicts their
covariance per ray - the two are strongly anti-correlated - and the basis images are reconstructed twice: by filtered
back-projection, which treats every ray and both channels alike, and jointly by penalised weighted least squares
(back_project.get_basismat_recon) with the inverse covariance as the weight and a Huber penalty.

Printed: the standard deviation of both basis images and of the 70 keV virtual monoenergetic image over the water pixels
(found on a noise-free FBP), for both reconstructions, and the objective before each PWLS iteration.

What to expect (DESIGN.md section 4.10 has the measured figures).  The weights are inverse variances: they are of the order of
1e7 .. 1e10 here, and ``--beta`` lives on that scale - a penalty below about 1e7 does nothing.  The iteration is the plain
separable surrogate, without preconditioning: its diagonal majoriser follows the stiff direction of W (the sum of the two line
integrals, whose noise cancels), so the soft direction (their difference, which carries the noise of the basis images)
converges (1 + |rho|) / (1 - |rho|) times more slowly - a few hundred times at rho = -0.99.  After the default 30 x 6 updates
the basis images are somewhat less noisy than FBP while the 70 keV image, where FBP already enjoys the cancellation and its own
ramp cut-off, is noisier; the objective is still falling.  The subsets must stay few for a scan like this one: the weights of
rays that graze the object are hundreds of times those of rays through its centre, a pixel is crossed by few views, and with
ten subsets of 18 views the scaled subset Hessian exceeds twice the majoriser - the objective then grows (one subset never
does).

    python examples/statistical_recon.py [--n 64] [--views 180] [--channels 128] [--matrix 64] [--fov 25.6] [--dose 5] [--iters 30]
                                         [--subsets 6] [--beta 1e8] [--delta 0.01] [--energy 70]
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
    ap.add_argument('--n', type=int, default=64, help='phantom slice is n x n voxels over 25.6 cm')
    ap.add_argument('--views', type=int, default=180)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--matrix', type=int, default=64, help='reconstruction matrix')
    ap.add_argument('--fov', type=float, default=25.6, help='its field of view [cm]; the defaults are the grid of the phantom')
    ap.add_argument('--dose', type=float, default=5.0, help='dose of each of the two scans [mGy]')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--subsets', type=int, default=6, help='ordered subsets (see the note on their number above)')
    ap.add_argument('--beta', type=float, default=1e8, help='strength of the Huber penalty, on the scale of the weights')
    ap.add_argument('--delta', type=float, default=0.01, help='threshold of the Huber penalty [g/cm^3]')
    ap.add_argument('--energy', type=float, default=70.0, help='energy of the VMI [keV]')
    ap.add_argument('--seed', type=int, default=1)
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
    N, fov, ramp = args.matrix, args.fov, 0.8
    E = np.array([args.energy])
    u = [float(xcompy.mixatten(m, E)[0]) for m in (md.matcomp1, md.matcomp2)]
    uw = float(xcompy.mixatten(plots.WATER, E)[0])

    def decompose(sinos):
        return md.get_basismat_sinos(ct, sinos[0][0], sinos[1][0], specs[0], specs[1], n_iters=50)

    def vmi_hu(m1, m2):
        return 1000.0 * (u[0] * m1.astype(np.float64) + u[1] * m2.astype(np.float64) - uw) / uw

    clean = dx.get_sinos(ct, phantom, specs)
    fbp_clean = [dx.get_recon(a, ct, specs[0], N, fov, ramp)[0] for a in decompose(clean)]
    water = np.abs(vmi_hu(*fbp_clean)) < 30.0                  # the water pixels of the noise-free VMI

    noisy = dx.get_sinos(ct, phantom, specs, noise=True, seed=args.seed)
    a = decompose(noisy)
    cov = md.get_basismat_covariance(ct, a, specs, mask_from=noisy[0][0])
    var = cov[..., 0] * cov[..., 2]
    rho = np.divide(cov[..., 1], np.sqrt(var), out=np.zeros_like(var), where=var > 0)
    print(f'correlation of the two basis line integrals over the rays that see the object: median {np.median(rho[var > 0]):.3f}')

    fbp = [dx.get_recon(s, ct, specs[0], N, fov, ramp)[0] for s in a]
    history = []
    pwls = dx.get_basismat_recon(a, cov, ct, N, fov, ramp, args.beta, args.delta, n_iters=args.iters, n_subsets=args.subsets,
                                 history=history)

    print(f'{int(water.sum())} water pixels of {N} x {N}; joint PWLS: {args.iters} iterations x {args.subsets} subsets, '
          f'beta {args.beta:g}, delta {args.delta:g}')
    print(f'{"":24s}{"FBP":>12s}{"joint PWLS":>12s}{"ratio":>8s}')
    for name, f, p in (('basis image 1 sd [g/cm3]', fbp[0], pwls[0]), ('basis image 2 sd [g/cm3]', fbp[1], pwls[1]),
                       (f'{args.energy:.0f} keV VMI sd [HU]', vmi_hu(*fbp), vmi_hu(*pwls))):
        sf, sp_ = float(np.std((f - 0.0)[water])), float(np.std((p - 0.0)[water]))
        print(f'{name:24s}{sf:12.4f}{sp_:12.4f}{sp_ / sf:8.3f}')
    bias = [float(np.mean((p.astype(np.float64) - c)[water])) for p, c in zip(pwls, fbp_clean)]
    print(f'mean of the PWLS basis images against the noise-free FBP in water: {bias[0]:+.4f}, {bias[1]:+.4f} g/cm3')
    print('objective before each iteration:', ' '.join(f'{h:.6g}' for h in history))
    return fbp, pwls, history


if __name__ == '__main__':
    main()
