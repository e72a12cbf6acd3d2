"""dexct_gn_decompose_dedup: solve repeated rows once, expand the results (profiles/gn_dedup.md).  The Newton launch of the
benchmark scan (512^3, 1000 x 800 x 512, dual spectrum, the default mode) on the three volumes of tools/probes/p16_dedup.py: the
benchmark phantom, the same phantom with the voxels of every z slice shuffled independently (no two rows alike) and a volume of
random blobs.  DEXCT_ROOT names the tree whose package is loaded (default: this one): a tree from before the route - where
gn_device has no ``dedup`` - is measured by the same script, as its only launch.

    python tools/probes/gn_dedup.py ab [rounds]    # per volume: ms per launch with dedup=False / None (auto), alternated;
                                                   # a_out compared byte for byte; the descriptor (use, F, cap) and F / n_pix
    python tools/probes/gn_dedup.py once           # per volume one launch of each, for rocprofv3 --kernel-trace --stats

VOLUMES=benchmark,shuffled,blobs chooses the volumes; N, VIEWS, CHANS the size."""
import inspect
import os
import sys

import torch

ROOT = os.environ.get('DEXCT_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('DEXCT_ROOT', ROOT)
import p16_dedup as vols        # noqa: E402  (its volumes, geometry and spectra)
from dex_ct_sim_amd import forward_project as fp, matdecomp as md      # noqa: E402
from dex_ct_sim_amd._device import ptr, stream_ptr      # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else 'ab'
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n, views, chans, ct, specs = vols.n, vols.views, vols.chans, vols.ct, vols.specs
HAS_ROUTE = 'dedup' in inspect.signature(md.gn_device).parameters
N_ITERS = 50


def timed(call, reps=3):
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(name, ph):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, _ = pj.upload_tables(specs)
    counts = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    pj.project_tables(mu_d, w_d, out=counts, layout=None)
    del pj
    _, i0, mus = md.decomposition_tables(ct, specs[0], specs[1])
    gmax = torch.empty((), dtype=torch.float64, device='cuda')
    assert md._native.load().dexct_reduce_max(ptr(counts[0]), 0, counts[0].numel(), ptr(gmax), stream_ptr()) == 0
    a = torch.empty((views, n, chans, 2), dtype=torch.float64, device='cuda')
    knobs = [('dedup=False', dict(dedup=False)), ('dedup=None', dict(dedup=None))] if HAS_ROUTE else [('no route in this tree', {})]
    call = lambda kw: md.gn_device(counts[0], counts[1], i0, mus, N_ITERS, 'f64', out=a, out_rc=(n, chans), mask_max=gmax, mask_frac=0.95, **kw)
    if mode == 'once':
        for label, kw in knobs:
            call(kw)
            torch.cuda.synchronize()
            print(f'{name}: one launch with {label}', flush=True)
        return
    ref = None
    for rep in range(rounds):
        for label, kw in knobs:
            ms = timed(lambda: call(kw))
            st = md.last_gn_stats()
            if ref is None:
                ref = a.clone()
            same = bool(torch.equal(a.view(torch.int64), ref.view(torch.int64)))
            dd = st.get('dedup')
            share = f', F / n_pix = {100.0 * dd["F"] / counts[0].numel():.2f} %' if dd and dd['F'] else ''
            print(f'{name} round {rep} {label}: {ms:.3f} ms  byte-identical: {same}  steps {st["pixel_iterations"]}  dedup {dd}{share}', flush=True)
            assert same


for name, ph in vols.volumes():
    measure(name, ph)
