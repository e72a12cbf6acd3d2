"""References of the matched projector pair and of SIRT / OS-SART (tests/test_iter_refs.py, tests/test_gpu_iter.py); plain
NumPy and the CPU oracle, no device.

The system matrix is dense and small: rows in layout 0 of the sinogram, ((view * n_rows) + row) * n_channels + channel,
columns (slice * ny + iy) * nx + ix.  ``system_matrix`` holds exactly the float32 coefficients include/dexct.h states for
dexct_image_project: the (voxel, length) rows of the oracle's fixed-point trace, t * len_per_u and (1 - t) * len_per_u as
float32 products, and the single coefficient len_per_u where both pieces of a slab lie in one pixel (the trace lists them one
after the other under the same voxel; a pixel belongs to one slab of a ray, so two entries with one voxel are such a pair).
"""
import numpy as np

from bounds_refs import Scan
from oracle import c_oracle as co

U = 2.0 ** -24
F32, F64 = np.float32, np.float64

# the "small" scans: 13 x 9 pixels of 0.31 x 0.27 cm, 3 slices of which rows 0, 1 image slices 1, 2; 7 views from 0.3 rad on
# (both dominant axes, both signs of the slope); a fan of 0.16 rad against a grid that subtends 0.08: the outer channels miss
# it, others enter through a side face; 53 channels and 65 (a second wave); and a grid of one pixel
SMALL = {
    'c53': dict(nx=13, ny=9, nz=3, n_views=7, n_ch=53, n_rows=2, z_first=1, theta0=0.3),
    'c65': dict(nx=13, ny=9, nz=3, n_views=7, n_ch=65, n_rows=2, z_first=1, theta0=0.3),
    'one': dict(nx=1, ny=1, nz=1, n_views=5, n_ch=53, n_rows=1, z_first=0, theta0=0.3, fan=0.03),
}
_small = {}


def small(name):
    if name not in _small:
        _small[name] = Scan(**SMALL[name])
    return _small[name]


def plan_of(scan):
    g = scan.geom(co.make_geom)
    return g, co.plan(g, scan.view_cs, scan.chan_cs, 0, scan.n_views)


def _dda_row(g, p, z):
    """{voxel: float32 coefficient} of one ray in slice z."""
    vox, ln = co.dda_ray(g, p, z)
    lpu = F32(p['len_per_u'])
    row, k = {}, 0
    while k < len(vox):
        if k + 1 < len(vox) and vox[k + 1] == vox[k]:
            row[int(vox[k])] = lpu                        # ja == jb
            k += 2
        else:
            row[int(vox[k])] = F32(ln[k]) * lpu           # one float32 product
            k += 1
    return row


def system_matrix(scan):
    g, plan = plan_of(scan)
    A = np.zeros((scan.n_views, scan.n_rows, scan.n_ch, scan.nz * scan.ny * scan.nx), F64)
    for v in range(scan.n_views):
        for c in range(scan.n_ch):
            p = plan[v * scan.n_ch + c]
            for r in range(scan.n_rows):
                for j, a in _dda_row(g, p, scan.z_first + r).items():
                    A[v, r, c, j] = F64(a)
    return A.reshape(-1, A.shape[-1])


def classic_matrix(scan):
    """The same matrix from the float64 textbook Siddon trace, which knows nothing of the plan."""
    g = scan.geom(co.make_geom)
    plane = scan.ny * scan.nx
    A = np.zeros((scan.n_views, scan.n_rows, scan.n_ch, scan.nz * plane), F64)
    for v in range(scan.n_views):
        for c in range(scan.n_ch):
            vox, ln = co.classic_ray(g, scan.view_cs, scan.chan_cs, v, c)
            for r in range(scan.n_rows):
                np.add.at(A[v, r, c], (scan.z_first + r) * plane + vox, ln)
    return A.reshape(-1, A.shape[-1])


def on_plane_rays(scan):
    """[views * rows * channels] mask of the rays that run along a grid plane (tests/test_siddon_oracle.py: the one genuine tie
    between float64 and 40-bit fixed point)."""
    _, plan = plan_of(scan)
    v0 = plan['V0'].astype(F64) / 2.0 ** 40
    tie = (np.abs(plan['SV'].astype(F64)) < 2.0 ** 10) & (np.abs(v0 - np.round(v0)) < 1e-9)
    return np.repeat(tie.reshape(scan.n_views, 1, scan.n_ch), scan.n_rows, 1).reshape(-1)


def forward_bound(A, x):
    """(A x, bound): |y - (A x)_i| <= (n_i + 4) u (|A| |x|)_i 1.01 for a float32 sum of n_i products of three roundings each."""
    n = np.count_nonzero(A, axis=1)
    return A @ x, (n + 4.0) * U * (np.abs(A) @ np.abs(x)) * 1.01


def sirt_ref(A, b, n_iters, n_subsets, relax, nonneg, x0, dtype=F64, history=None):
    """The update rule of dex_ct_sim_amd.iterative, literally, in ``dtype``.  b: [n_views, ...] (the first axis tells the rays
    of a view apart); subset s = the views congruent to s modulo n_subsets, visited in ascending order."""
    n_views = b.shape[0]
    per_view = A.shape[0] // n_views
    A = A.astype(dtype)
    bb = b.reshape(-1).astype(dtype)
    x = np.zeros(A.shape[1], dtype) if x0 is None else x0.reshape(-1).astype(dtype)
    relax = dtype(relax)
    R = A.sum(1, dtype=dtype)
    hit = R > 0
    Rs = np.where(hit, R, dtype(1))
    view_of = np.arange(A.shape[0]) // per_view
    for _ in range(n_iters):
        if history is not None:
            d = bb - A @ x
            history.append(float(np.sqrt(np.sum(np.where(hit, d.astype(F64) ** 2 / Rs.astype(F64), 0.0)))))
        for s in range(n_subsets):
            rows = view_of % n_subsets == s
            As = A[rows]
            r = np.where(hit[rows], (bb[rows] - As @ x) / Rs[rows], dtype(0)).astype(dtype)
            g = As.T @ r
            C = As.sum(0, dtype=dtype)
            upd = C > 0
            x = np.where(upd, x + relax * (g / np.where(upd, C, dtype(1))), x).astype(dtype)
            if nonneg:
                x = np.maximum(x, dtype(0))
    return x
