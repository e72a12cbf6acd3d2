#!/usr/bin/env python3
"""Generate golden vectors for K = 3, 4 measurements and M = 2, 3 basis materials from the REAL reference routine.

Runs only where the reference's sources are available (REF in make_goldens.py).  Like make_goldens.py it imports the reference's
``matdecomp.py`` with two stub modules (``cupy`` is not installed, ``xcompy`` lives in an absent submodule), calls
``optimize_sino_cpu`` (matdecomp.py:87-127) - which is general in nMeas and nMats - on small seeded inputs and stores inputs
and outputs as arrays in ``ref_multi.npz`` next to this file.  Nothing of the reference's source is stored.

    python tests/golden/make_goldens_multi.py

Layout of the file: ``cases`` lists the case names; parallel to it, ``tables`` names each case's tables and ``index`` is its
place among the cases of those tables.  ``<tables>_i0`` [K, nE], ``<tables>_mus`` [M, nE]; then, stacked over the n cases of
the tables (few arrays: every member of the archive costs a header), ``<tables>_g`` [n, K, 4, 16] counts, ``<tables>_a30``
[n, 4, 16, M] = the reference after 30 iterations and ``<tables>_d50`` = (50 iterations) - (30 iterations): the two agree to a
few ulp, the difference of two such doubles is exact, and it compresses to almost nothing, which keeps the file small;
``a30 + d50`` IS the reference after 50 iterations, bit for bit (asserted here).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gn_multi_refs as mr                       # noqa: E402
from make_goldens import half_split, load_pkg_module, load_reference   # noqa: E402

N_VIEWS, N_BINS = 4, 16
INPUT = os.path.join(ROOT, 'dex-ct-sim_amd', 'input')


def run_reference(ref, g, i0, mus, n_iters):
    """optimize_sino_cpu with the spectrum tiled over the channels, the layout do_matdecomp_gn gives it (matdecomp.py:151)"""
    i0_tiled = np.ascontiguousarray(np.broadcast_to(i0[:, None, :], (i0.shape[0], g.shape[2], i0.shape[1])))
    return ref.optimize_sino_cpu(g, None, i0_tiled, mus, n_iters, verbose=False)


def add_case(out, names, ref, name, tables, g):
    i0, mus = out[f'{tables}_i0'], out[f'{tables}_mus']
    a30 = run_reference(ref, g, i0, mus, 30)
    a50 = run_reference(ref, g, i0, mus, 50)
    assert np.all(np.isfinite(a30)) and np.all(np.isfinite(a50)), name
    d50 = a50 - a30
    assert np.array_equal(a30 + d50, a50), name
    # what the tests rely on: converged, and insensitive to the order of the energies
    rev = run_reference(ref, g, np.ascontiguousarray(i0[:, ::-1]), np.ascontiguousarray(mus[:, ::-1]), 50)
    moved = mr.rel_err(a30, a50)
    order = mr.rel_err(rev, a50)
    print(f'{name}: 30 vs 50 iterations {moved:.2e}, reversed energies {order:.2e}')
    for key, arr in (('g', g), ('a30', a30), ('d50', d50)):
        out.setdefault(f'{tables}_{key}', []).append(arr)
    names.append((name, tables, len(out[f'{tables}_g']) - 1))
    return moved, order


def main():
    ref = load_reference()
    xc = load_pkg_module('xcompy')
    rng = np.random.default_rng(20240611)
    out, names = {}, []
    worst_moved = worst_order = 0.0

    # ---- (a) synthetic tables: 3 or 4 soft-edged energy bins, 2 or 3 materials (the third with a K-edge)
    E, mus3, S = mr.synthetic_tables(60)
    for K, M in ((3, 2), (4, 2), (3, 3), (4, 3)):
        i0 = mr.synthetic_bins(E, S, mr.EDGES[K])
        mus = np.ascontiguousarray(mus3[:M])
        out[f'syn_k{K}m{M}_i0'], out[f'syn_k{K}m{M}_mus'] = i0, mus
        base = rng.uniform(0.0, 1.0, (N_VIEWS, N_BINS, M)) * np.array(mr.A_MAX[:M])
        for scale, tag in ((1.0, 'a'), (1.6, 'b')):
            g = mr.forward_counts(scale * base, i0, mus)
            for counts, kind in ((g, 'exact'), (mr.noisy(g, rng), 'noisy')):
                m, o = add_case(out, names, ref, f'syn_k{K}m{M}{tag}_{kind}', f'syn_k{K}m{M}', counts)
                worst_moved, worst_order = max(worst_moved, m), max(worst_order, o)

    # ---- (b) the bundled 80 / 120 / 140 kV spectra on the energy-integrating detector, tissue and bone
    det_E, det_eta = half_split(os.path.join(INPUT, 'detector', 'eta_eid_mv.bin'))
    specs = [half_split(os.path.join(INPUT, 'spectrum', f'{kv}kV_1mGy_float32.bin')) for kv in (80, 120, 140)]
    ee = np.array(sorted(set(np.concatenate([s[0] for s in specs]))))
    dE = np.append([ee[0]], ee[1:] - ee[:-1])
    resp = np.interp(ee, det_E, det_eta) * ee
    i0 = np.stack([np.interp(ee, s[0], s[1] * 5.0e-4) * resp * dE for s in specs])
    mus = np.stack([xc.mixatten(ref.matcomp1, ee), xc.mixatten(ref.matcomp2, ee)])
    a_true = rng.uniform(0.0, 1.0, (N_VIEWS, N_BINS, 2)) * np.array([30.0, 5.0])
    g = mr.forward_counts(a_true, i0, mus)
    out['kvp_ee'], out['kvp_k3m2_i0'], out['kvp_k3m2_mus'] = ee, i0, mus
    for counts, kind in ((g, 'exact'), (mr.noisy(g, rng), 'noisy')):
        add_case(out, names, ref, f'kvp_k3m2_{kind}', 'kvp_k3m2', counts)

    out = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
    out['cases'] = np.array([n for n, _, _ in names])
    out['tables'] = np.array([t for _, t, _ in names])
    out['index'] = np.array([i for _, _, i in names])
    print(f'synthetic cases: worst 30-vs-50 {worst_moved:.2e}, worst energy order {worst_order:.2e}')
    path = os.path.join(HERE, 'ref_multi.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(names), 'cases')


if __name__ == '__main__':
    main()
