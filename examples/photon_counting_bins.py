#!/usr/bin/env python3
"""Spectral CT with a photon-counting detector on the MI355X engine: scan three energy bins of one spectrum in ONE traversal,
decompose them into two and into three basis materials, and compare with the true line integrals.

The phantom is a water cylinder with bone spheres, one of them replaced by a dilute iodine solution.  Water and bone alone
cannot describe the iodine's K-edge (33.2 keV); with a third basis and the lowest bin ending near that edge they can.

    python examples/photon_counting_bins.py [--n 128] [--views 90] [--channels 192] [--edges 20 34 60 121] [--noise]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dex_ct_sim_amd as dx                                   # noqa: E402
from dex_ct_sim_amd import matdecomp as md, synthetic         # noqa: E402
from dex_ct_sim_amd.forward_project import Projector          # noqa: E402

# 1.96 % iodine by mass in the phantom's water (H 11.1894, O 88.8106): about 20 mg/ml
IODINE = dx.Material('iodine solution', 1.02, 'H(10.9701)O(87.0699)I(1.96)')


def true_line_integrals(ct, phantom):
    """[view, channel, material id] g/cm^2 along every ray: path length per material (the projector's own) x density"""
    pj = Projector(ct, phantom)
    (_, pathlen), _ = pj.project([synthetic.kramers_spectrum(120)], want_pathlen=True)
    pl = pathlen.cpu().numpy().astype(np.float64)[:, 0]        # [view, channel, compact id] in cm (one detector row)
    out = np.zeros(pl.shape[:2] + (len(phantom.materials),))
    for k, row in enumerate(pj.mat_rows):                      # compact id k is served by the table row of phantom id `row`
        out[..., int(row)] += pl[..., k] * phantom.materials[int(row)].density
    return out


def iodine_with_k_edge():
    """The bundled attenuation surrogate is smooth (no absorption edges), and three smooth materials are not three independent
    bases.  Register an iodine table that has the K-edge at 33.17 keV: the surrogate above the edge, a 5.5th of it below
    (illustrative values, not NIST; install real tables with DEXCT_XCOM_DIR)."""
    from dex_ct_sim_amd import xcompy
    E = np.unique(np.concatenate([np.arange(1.0, 151.0, 0.5), [33.169, 33.171]]))
    mu = xcompy.mixatten('I(100)', E) * np.where(E >= 33.17, 1.0, 1.0 / 5.5)
    xcompy.register_table('I', E, mu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128, help='phantom slice is n x n voxels over 25.6 cm')
    ap.add_argument('--views', type=int, default=90)
    ap.add_argument('--channels', type=int, default=192)
    ap.add_argument('--edges', type=float, nargs=4, default=[20.0, 34.0, 60.0, 121.0], help='bin thresholds [keV]')
    ap.add_argument('--dose', type=float, default=1e7, help='photons per detector pixel and view, unattenuated')
    ap.add_argument('--noise', action='store_true', help='quantum noise for that dose (a third basis amplifies it strongly: raise --dose)')
    args = ap.parse_args()

    iodine_with_k_edge()
    det = os.path.join(ROOT, 'dex-ct-sim_amd', 'input', 'detector', 'eta_pcd_Si_30mm.bin')
    ct = dx.FanBeamGeometry(N_channels=args.channels, N_proj=args.views, eid=False, detector_file=det)
    phantom = synthetic.make_phantom(args.n, 1, extent=25.6)   # 0 air, 1 water, 2 bone
    vol = phantom.volume.copy()
    ys, xs = np.nonzero(vol[0] == 2)
    if ys.size:                                                # the bone voxels left of the centre become iodine solution
        left = xs < args.n // 2
        vol[0, ys[left], xs[left]] = 3
    phantom = dx.VoxelPhantom.from_array('water + bone + iodine', vol, list(phantom.materials) + [IODINE], dx=phantom.dx,
                                         dy=phantom.dy, dz=phantom.dz)

    spec = synthetic.kramers_spectrum(120)
    spec.rescale_counts(args.dose / spec.I0.sum())
    bins = dx.energy_bins(spec, args.edges)                    # threshold bins are just spectra
    sinos = [raw for raw, _ in dx.get_sinos(ct, phantom, bins, noise=args.noise, seed=1)]     # one traversal
    print('counts per bin in air:', ', '.join(f'{s.max():.3g}' for s in sinos))

    truth = true_line_integrals(ct, phantom)                   # [view, channel, (air, water, bone, iodine solution)]
    air = sinos[0] >= 0.95 * sinos[0].max()                    # the pixels the decomposition zeroes
    # the iodine solution is 98 % water by mass: express the truth in the bases water / bone / iodine
    w_i = 0.0196
    t_water = truth[..., 1] + (1.0 - w_i) * truth[..., 3]
    t_bone = truth[..., 2]
    t_iodine = w_i * truth[..., 3]

    water, bone = phantom.materials[1].matcomp, phantom.materials[2].matcomp
    two = md.get_basismat_sinos_multi(ct, sinos, bins, materials=(water, bone), n_iters=50)
    three = md.get_basismat_sinos_multi(ct, sinos, bins, materials=(water, bone, 'I(100)'), n_iters=50)

    def rmse(a, b):
        ok = ~air & np.isfinite(a)
        return float(np.sqrt(np.mean((a[ok] - b[ok]) ** 2)))

    print('RMSE of the density line integrals against the truth [g/cm^2]')
    print(f'  two bases:    water {rmse(two[0], t_water):.4f}   bone {rmse(two[1], t_bone):.4f}   (the iodine has nowhere to go)')
    print(f'  three bases:  water {rmse(three[0], t_water):.4f}   bone {rmse(three[1], t_bone):.4f}   '
          f'iodine {rmse(three[2], t_iodine):.5f}  (of up to {t_iodine.max():.4f})')
    return two, three


if __name__ == '__main__':
    main()
