"""--dump-outputs DIR: what the timed step computed in its LAST step, as a caller of the hot path receives it, written after the
timed loop as DIR/<name>.npy:

    sino_raw, sino_log   float32 [2 spectra, ...]   get_sino's two outputs (140 kVp, then 80 kVp), [view][row][channel] order
    basismat1, basismat2 float64 [...]              get_basismat_sinos' two basis-material sinograms, same order

At most MAX_BYTES in all.  A larger scan is sampled at a fixed, seeded set of rays - the same rays in every array, in
increasing order, their flat [view][row][channel] indices in sample_index.npy (float64, exact) - so that two builds run with
the same arguments compare output for output.  N = 1 only (launch.parse refuses it with more ranks)."""
import os

import numpy as np
import torch

MAX_BYTES = 64 << 20
SAMPLE_RAYS = 1 << 20              # 40 B per ray (2 x 4 + 2 x 4 + 8 + 8 + the index's 8): 40 MiB
SEED = 20240611


def write(wl, out_dir):
    """Returns {name: shape} of what was written."""
    counts, log, a = wl.counts, wl.log_ref, wl.a_out          # [2, nV, rows, channels] f32 x 2, [nV, rows, channels, 2] f64
    n = counts[0].numel()
    arrays = {}
    if n * 32 <= MAX_BYTES:                                  # the whole scan
        arrays['sino_raw'], arrays['sino_log'] = counts, log
        arrays['basismat1'], arrays['basismat2'] = a[..., 0], a[..., 1]
    else:
        idx = np.sort(np.random.default_rng(SEED).choice(n, size=SAMPLE_RAYS, replace=False))
        idx_d = torch.from_numpy(idx).to(wl.dev)
        arrays['sino_raw'] = counts.reshape(2, n).index_select(1, idx_d)
        arrays['sino_log'] = log.reshape(2, n).index_select(1, idx_d)
        flat = a.reshape(n, 2).index_select(0, idx_d)
        arrays['basismat1'], arrays['basismat2'] = flat[:, 0], flat[:, 1]
        arrays['sample_index'] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    shapes = {}
    for name, x in arrays.items():
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x.dtype in (np.float32, np.float64), (name, x.dtype)
        np.save(os.path.join(out_dir, name + '.npy'), np.ascontiguousarray(x))
        shapes[name] = list(x.shape)
    return shapes
