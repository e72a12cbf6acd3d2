#!/usr/bin/env python3
"""Entry point with the reference's run sequence (main.py:74-178 of gjadick/dex-ct-sim):

for every run in the parameter file, for every dual-energy spectrum pair:
  1. per spectrum: load + dose-scale the spectrum (:64-69), forward project (:120), write
     ``<spec>_<dose>uGy/sino_raw_float32.bin`` and ``sino_log_float32.bin`` (:121-122);
  2. decompose the two raw sinograms into basis-material sinograms with 50 Newton iterations
     (:153) and write ``matdecomp_<s1>_<s2>_<d1>uGy_<d2>uGy/mat{1,2}_sino_float32.bin`` (:154-155).
  3. when ``back_project`` is set: reconstruct every log sinogram (:134 -> recon_raw/recon_HU .bin, :135-136)
     and both basis-material sinograms (:168 -> mat{1,2}_recon_float32.bin, :169); with ``--bhc water bone`` also the
     beam-hardening-corrected images of every log sinogram, ``recon_{water,bone}BHC_{raw,HU}_float32.bin`` (the files
     the reference's plots.py:184-195 reads; basis-material sinograms are linear in thickness already and get none);
     ``--recon sirt`` reconstructs all of them iteratively (SIRT / OS-SART, iterative.py) instead of by FBP.
     ``--recon pwls`` (needs ``--covariance``) reconstructs the two basis-material sinograms JOINTLY, weighted with the
     inverse of their predicted covariance and with a Huber penalty (back_project.get_basismat_recon; ``--recon-beta``,
     ``--recon-delta``), into the same ``mat{1,2}_recon_float32.bin``; the single-energy images stay FBP.
  4. with ``--covariance``: the predicted noise covariance of the two basis-material sinograms per detector pixel
     (matdecomp.get_basismat_covariance at the decomposed line integrals, for the doses of the pair), written next to them as
     ``cov11_sino_float32.bin``, ``cov12_sino_float32.bin``, ``cov22_sino_float32.bin``; air pixels hold 0 like the sinograms.
  5. with ``--noise-maps`` (needs ``--covariance`` and ``back_project``): that covariance propagated through the FBP
     (back_project.get_recon_covariance) - the predicted noise (co)variance of the two basis-material images per pixel, written as
     ``cov11_recon_float32.bin``, ``cov12_recon_float32.bin``, ``cov22_recon_float32.bin`` next to ``mat{1,2}_recon_float32.bin``
     (computed from the float32 values of the ``cov*_sino`` files, so the two sets of files agree exactly).

Differences from the reference script, all on purpose: inputs are command-line options instead of
edited source lines (:80-82, :101-103); figures are off unless --show; both spectra of a pair are
projected in ONE traversal (path lengths do not depend on energy); run with
``python -m torch.distributed.run --nproc-per-node N main.py`` to shard the projection angles.
"""
import argparse
import os
import shutil
import sys
from time import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dex_ct_sim_amd as dx  # noqa: E402
from dex_ct_sim_amd.back_project import get_basismat_recon, get_recon, get_recon_covariance  # noqa: E402
from dex_ct_sim_amd.forward_project import get_sinos  # noqa: E402
from dex_ct_sim_amd.matdecomp import get_basismat_covariance, get_basismat_sinos  # noqa: E402


def load_spectrum(ct, spec_id, dose, input_dir):
    """Spectrum at 1 mGy scaled to the target dose per view (main.py:64-69)."""
    spec = dx.xRaySpectrum(os.path.join(input_dir, 'spectrum', f'{spec_id}_1mGy_float32.bin'), spec_id)
    spec.rescale_counts(ct.A_iso * dose / ct.N_proj)
    return spec


def parse_pairs(items):
    pairs = []
    for it in items:
        s1, s2, d1, d2 = it.split(':')
        pairs.append((s1, s2, float(d1), float(d2)))
    return pairs


def show(title_a, a, title_b, b):
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(1, 2, figsize=[7, 3])
    for axi, img, ttl in ((ax[0], a, title_a), (ax[1], b, title_b)):
        m = axi.imshow(img, cmap='gray', aspect='auto')
        axi.set_title(ttl)
        fig.colorbar(m, ax=axi)
    fig.tight_layout()
    plt.show()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--params', default=os.path.join(HERE, 'input', 'params.txt'))
    ap.add_argument('--out', default='./output/')
    ap.add_argument('--input-dir', default=os.path.join(HERE, 'input'))
    ap.add_argument('--pairs', nargs='+', default=['detunedMV:80kV:9:1'],
                    help='spec1:spec2:dose1_mGy:dose2_mGy (reference default, main.py:101)')
    ap.add_argument('--n-iters', type=int, default=50)
    ap.add_argument('--gn-exact', action='store_true',
                    help='run the fixed iteration count of matdecomp.py:114 bit for bit (stop_tol = 0) instead of ending a '
                         'pixel once the distance it still has to go is below 1e-12 relative (the default)')
    ap.add_argument('--gn-audit', default='100', metavar='PPM[,strict]',
                    help='sampled audit of the Newton short cut: that many pixels per million are solved again with the fixed '
                         'iteration count in the same call and compared (<= 1e-12, same NaN pattern); a difference warns, or '
                         'raises with ",strict"; 0 = off (the library default; this script switches it on)')
    ap.add_argument('--show', action='store_true')
    ap.add_argument('--noise', default='off', choices=['off', 'gaussian', 'poisson'],
                    help='quantum noise for the dose of each spectrum (default off: the noise-free expectation); '
                         'gaussian: compound-Poisson variance, normal sample; poisson: per-energy-bin photon counts')
    ap.add_argument('--seed', type=int, default=0, help='seed of the counter-based noise generator')
    ap.add_argument('--window', default=None, choices=['rect', 'sinc', 'cosine', 'hann', 'hamming'],
                    help='apodisation of the reconstruction ramp (default: DEXCT_FBP_WINDOW or rect)')
    ap.add_argument('--bhc', nargs='*', default=[], choices=['water', 'bone'],
                    help='also write beam-hardening-corrected reconstructions of every log sinogram, linearised for '
                         'these reference materials (recon_<m>BHC_{raw,HU}_float32.bin beside recon_raw)')
    ap.add_argument('--recon', default='fbp', choices=['fbp', 'sirt', 'pwls'],
                    help='reconstruction method: filtered back-projection (default), SIRT / OS-SART on the matched projector '
                         'pair, started from the FBP image, or pwls: the basis-material images jointly by penalised weighted '
                         'least squares with the --covariance of the decomposition as the weight (the single-energy images stay '
                         'FBP); the output file names stay the reference\'s')
    ap.add_argument('--recon-iters', type=int, default=20, help='iterations of --recon sirt / pwls')
    ap.add_argument('--recon-subsets', type=int, default=1,
                    help='ordered subsets of --recon sirt (1: SIRT, more: OS-SART) / pwls')
    ap.add_argument('--recon-beta', type=float, default=0.0, help='strength of the Huber penalty of --recon pwls (0: none)')
    ap.add_argument('--recon-delta', type=float, default=1e-3,
                    help='threshold of the Huber penalty of --recon pwls, in the unit of the basis images')
    ap.add_argument('--covariance', nargs='?', const='estimator', default=None, choices=['estimator', 'crlb'],
                    help='also write the predicted noise covariance of each decomposed pair (cov11 / cov12 / cov22 _sino_float32.bin '
                         'beside mat1_sino): of what the Newton solve returns (estimator, the default) or the Cramer-Rao bound '
                         '(crlb); single process only')
    ap.add_argument('--noise-maps', action='store_true',
                    help='also write the predicted noise covariance of the basis-material IMAGES (cov11 / cov12 / cov22 '
                         '_recon_float32.bin beside mat1_recon): the --covariance sinograms propagated through the FBP; needs '
                         '--covariance, back_project in the parameter file and --recon fbp; single process only')
    args = ap.parse_args(argv)
    if args.noise_maps and not args.covariance:
        ap.error('--noise-maps needs --covariance')
    if args.noise_maps and args.recon != 'fbp':
        ap.error('--noise-maps propagates the covariance through the FBP: it needs --recon fbp')
    if args.covariance and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        ap.error('--covariance runs on a single process')
    if args.recon == 'pwls' and not args.covariance:
        ap.error('--recon pwls weights the reconstruction with the covariance of the decomposition: it needs --covariance')
    if args.recon == 'pwls' and (args.recon_beta < 0 or not args.recon_delta > 0):
        ap.error('--recon-beta must be >= 0 and --recon-delta > 0')
    recon_kw = {} if args.recon in ('fbp', 'pwls') else dict(method=args.recon, n_iters=args.recon_iters,
                                                             n_subsets=args.recon_subsets)

    import torch.distributed as dist
    if int(os.environ.get('WORLD_SIZE', '1')) > 1 and not dist.is_initialized():
        # RCCL; DEXCT_DIST_BACKEND=gloo rehearses the sharded flow on a box with fewer GPUs than ranks
        dist.init_process_group(os.environ.get('DEXCT_DIST_BACKEND', 'nccl'))
    rank = dist.get_rank() if dist.is_initialized() else 0

    # './input/...' paths of the params file resolve against the folder that holds the input directory; the
    # working directory stays where it is (relative --params / --input-dir / --out keep their meaning)
    args.params = os.path.abspath(args.params)
    args.input_dir = os.path.abspath(args.input_dir)
    all_params = dx.read_parameter_file(args.params, base_dir=os.path.dirname(args.input_dir))
    if args.noise_maps and not all(params[2] for params in all_params):
        ap.error('--noise-maps needs runs that back-project: back_project is off in the parameter file')
    for params in all_params:
        run_id, do_fp, do_bp = params[:3]
        ct, phantom, _ = params[3:6]            # the spectrum entry is ignored, as in main.py:92
        out_dir = os.path.join(args.out, run_id)
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
            shutil.copy(args.params, os.path.join(out_dir, 'params.txt'))
        if do_bp:
            N_matrix, FOV, ramp = params[6:9]
        for s1, s2, d1, d2 in parse_pairs(args.pairs):
            t0 = time()
            specs = [load_spectrum(ct, s1, d1, args.input_dir), load_spectrum(ct, s2, d2, args.input_dir)]
            print('Forward projecting!')
            sinos = get_sinos(ct, phantom, specs, noise={'off': False, 'gaussian': True, 'poisson': 'poisson'}[args.noise],
                              seed=args.seed)
            for (spec_id, dose), (sino_raw, sino_log) in zip(((s1, d1), (s2, d2)), sinos):
                sub_dir = os.path.join(out_dir, f'{spec_id}_{int(dose * 1000):04}uGy/')
                if rank == 0:
                    os.makedirs(sub_dir, exist_ok=True)
                    print(f'\n*** {sub_dir} ***')
                    sino_raw.astype(np.float32).tofile(sub_dir + 'sino_raw_float32.bin')
                    sino_log.astype(np.float32).tofile(sub_dir + 'sino_log_float32.bin')
                    if args.show:
                        show('Raw line integrals', sino_raw, 'Log sinogram', sino_log)
                    if do_bp:
                        print('Back projecting!')
                        spec = specs[0] if spec_id == s1 else specs[1]
                        recon_raw, recon_HU = get_recon(sino_log, ct, spec, N_matrix, FOV, ramp, window=args.window, **recon_kw)
                        recon_raw.astype(np.float32).tofile(sub_dir + 'recon_raw_float32.bin')
                        recon_HU.astype(np.float32).tofile(sub_dir + 'recon_HU_float32.bin')
                        for m in dict.fromkeys(args.bhc):
                            bhc_raw, bhc_HU = get_recon(sino_log, ct, spec, N_matrix, FOV, ramp, window=args.window, bhc=m, **recon_kw)
                            bhc_raw.astype(np.float32).tofile(sub_dir + f'recon_{m}BHC_raw_float32.bin')
                            bhc_HU.astype(np.float32).tofile(sub_dir + f'recon_{m}BHC_HU_float32.bin')
                        if args.show:
                            show('Raw reconstruction [1/cm]', recon_raw, 'Hounsfield Units', recon_HU)
            sub_dir = os.path.join(out_dir, f'matdecomp_{s1}_{s2}_{int(d1 * 1000):04}uGy_{int(d2 * 1000):04}uGy/')
            print('Decomposing into basis material sinograms!')
            matsino1, matsino2 = get_basismat_sinos(ct, sinos[0][0], sinos[1][0], specs[0], specs[1],
                                                    n_iters=args.n_iters, verbose=True,     # progress lines of :111-112
                                                    stop_tol=0.0 if args.gn_exact else None,
                                                    audit=float(args.gn_audit.split(',')[0]),
                                                    audit_strict=args.gn_audit.endswith(',strict'))
            if rank == 0:
                os.makedirs(sub_dir, exist_ok=True)
                print(f'\n*** {sub_dir} ***')
                matsino1.astype(np.float32).tofile(sub_dir + 'mat1_sino_float32.bin')
                matsino2.astype(np.float32).tofile(sub_dir + 'mat2_sino_float32.bin')
                if args.show:
                    show('Basis material 1', matsino1, 'Basis material 2', matsino2)
                if args.covariance:
                    print(f'Predicting the noise covariance of the basis material sinograms ({args.covariance})!')
                    cov = get_basismat_covariance(ct, (matsino1, matsino2), specs, kind=args.covariance, mask_from=sinos[0][0])
                    for t, name in enumerate(('cov11', 'cov12', 'cov22')):
                        cov[..., t].astype(np.float32).tofile(sub_dir + f'{name}_sino_float32.bin')
                if do_bp:
                    print('Back projecting basis material sinograms!')
                    if args.recon == 'pwls':
                        mat_recons = get_basismat_recon((matsino1, matsino2), cov, ct, N_matrix, FOV, ramp, args.recon_beta,
                                                        args.recon_delta, n_iters=args.recon_iters, n_subsets=args.recon_subsets,
                                                        window=args.window)
                    else:
                        # spec is filler (:168); basis-material line integrals may be negative: no clamp at 0
                        mat_kw = dict(recon_kw, nonneg=False) if recon_kw else {}
                        mat_recons = [get_recon(matsino, ct, specs[0], N_matrix, FOV, ramp, window=args.window, **mat_kw)[0]
                                      for matsino in (matsino1, matsino2)]
                    for i, recon_raw in enumerate(mat_recons):
                        recon_raw.astype(np.float32).tofile(sub_dir + f'mat{i + 1}_recon_float32.bin')
                    if args.noise_maps:
                        print('Propagating the noise covariance through the reconstruction!')
                        # of the covariance as written (float32): the files of a run agree with each other exactly
                        cov_img = get_recon_covariance(cov.astype(np.float32), ct, N_matrix, FOV, ramp, window=args.window)
                        for t, name in enumerate(('cov11', 'cov12', 'cov22')):
                            cov_img[..., t].astype(np.float32).tofile(sub_dir + f'{name}_recon_float32.bin')
                print(f'matdecomp finished for {s1}-{s2} : t={time() - t0:.2f}s')


if __name__ == '__main__':
    main()
