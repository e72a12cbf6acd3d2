"""References, error bounds and the chosen geometries of the guard-banded projection and reconstruction tests
(tests/test_gpu_bounds_projection.py, tests/test_gpu_bounds_recon.py); plain NumPy, no device.

Everything the GPU modules compare a kernel against lives here, so that tests/test_bounds_refs.py can show on the CPU that
(a) each comparison rejects a slightly wrong result (a dropped view, a channel shifted by one, one tap scaled by 1 + 4 n_ch u)
and (b) the exclusion caps (2 % tie rays, 1 % edge pixels) hold for every geometry the GPU modules use.

The reconstruction references take the SAME float32 arrays the kernel is given and evaluate in float64.  The bounds follow
the arithmetic of csrc/fbp.hip, per output element, from float64 absolute sums, with u = 2^-24 (float32 unit round-off):

  Parker      out = (float)(2 w sino), w and the product in float64: one rounding (<= u |ref|); the device's sin may differ from
              the host's in the last float64 place, far below the second u:                    |err| <= 2 u |ref|
  filter      line[m] = sino[m] * weight[m] (1 rounding); two fmaf chains over the even and the odd m, ceil(n / 2) terms at
              most, every term of a chain sees at most that many roundings; their sum (1); the product with (float)dgamma (1)
              and the rounding of dgamma itself (1): n / 2 + 4.5 roundings at most, second order below 0.5 for n <= 5000:
                                       |err| <= (n / 2 + 6) u dgamma sum_m |sino[m] weight[m] taps[k - m + n - 1]|
  back-proj.  per contributing view, on the path of q0: w = (float)(pos - floor(pos)) carries u w, 1 - w the rest of u (so the
              two roundings together cost u |q0|, and likewise on the path of q1), the product (1), the sum (1), the rounding of
              L^2 (1), the division (1): 5 u (|q0| + |q1|) / L^2; the running sum adds at most one rounding per view; the
              product with (float)dbeta and its rounding (2):
                                       |err| <= (n_views + 8) u dbeta sum_v (|q0| + |q1|) / L^2
  FDK         the same with both channel interpolations (2 each), the row weight (1), the row interpolation (w_r as w: 1,
              product 1, sum 1), 1 / L^2 rounded and multiplied (2): 9 per view:
                                       |err| <= (n_views + 12) u dbeta sum_v (|qa0| + |qa1|) rw[r0] + (|qb0| + |qb1|) rw[r0 + 1]) / L^2
A pixel whose detector position (channel, or row for FDK) lies within 1e-9 of the first or last sample for some view is left
out: a whole contribution switches on or off there and atan2 may differ in the last place between device and host.
"""
import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
EDGE = 1e-9


def within(got, ref, bound):
    """True when |got - ref| <= bound everywhere (NaN or inf anywhere in ``got`` fails)."""
    got = np.asarray(got, F64)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound))


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound (for the messages of failing assertions)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, np.abs(np.asarray(got, F64) - ref) / bound, np.where(np.asarray(got, F64) == ref, 0.0, np.inf))
    return float(np.max(r))


# ---- Parker ------------------------------------------------------------------------------------------------------------------

def parker_ref(sino, theta_tot, dgamma, view_offset, n_views_total):
    """sino float32 [n_views][n_rows][n_channels] -> (ref float64, bound)."""
    from oracle import fbp_oracle as fo
    n_views, _, n_ch = sino.shape
    thetas = theta_tot * (view_offset + np.arange(n_views, dtype=F64)) / float(n_views_total)
    gammas = (np.arange(n_ch, dtype=F64) - 0.5 * (n_ch - 1)) * dgamma
    w = fo.parker_weights(thetas, gammas, theta_tot)
    ref = 2.0 * w[:, None, :] * sino.astype(F64)
    return ref, 2.0 * U * np.abs(ref)


# ---- filter ------------------------------------------------------------------------------------------------------------------

def filter_ref(sino, taps, weight, dgamma):
    """sino float32 [lines][n], taps float32 [2n - 1], weight float32 [n] -> (ref, bound), float64 [lines][n]."""
    n = sino.shape[-1]
    rp = sino.astype(F64) * weight.astype(F64)
    r = taps.astype(F64)[::-1]
    T = np.lib.stride_tricks.sliding_window_view(r, n)[::-1]           # T[k][m] = taps[k - m + n - 1]
    ref = dgamma * (rp @ T.T)
    bound = (0.5 * n + 6.0) * U * dgamma * (np.abs(rp) @ np.abs(T).T)
    return ref, bound


# ---- back-projection ---------------------------------------------------------------------------------------------------------

def _pixels(n_matrix, fov):
    c = (np.arange(n_matrix, dtype=F64) - 0.5 * n_matrix + 0.5) * (fov / n_matrix)
    return np.meshgrid(c, c)                                             # x along the last axis: image[iy][ix]


def _channel_pos(x, y, cb, sb, sid, dgamma, n_ch):
    dx, dy = x - sid * cb, y - sid * sb
    dot, cross = -(cb * dx + sb * dy), -(cb * dy - sb * dx)
    pos = np.arctan2(cross, dot) * (1.0 / dgamma) + 0.5 * (n_ch - 1)
    return pos, dx * dx + dy * dy


def backproject_ref(q, view_cs, sid, dgamma, dbeta, n_matrix, fov):
    """q float32 [n_views][n_rows][n_ch], view_cs float64 [n_views][2] -> (ref, bound, keep): float64 / bool
    [n_rows][n_matrix][n_matrix]; ``keep`` False for the pixels at a detector edge (module docstring)."""
    n_views, n_rows, n_ch = q.shape
    qd = q.astype(F64)
    x, y = _pixels(n_matrix, fov)
    ref = np.zeros((n_rows, n_matrix, n_matrix))
    mag = np.zeros_like(ref)
    keep = np.ones((n_matrix, n_matrix), bool)
    for v in range(n_views):
        pos, l2 = _channel_pos(x, y, view_cs[v, 0], view_cs[v, 1], sid, dgamma, n_ch)
        keep &= (np.abs(pos) > EDGE) & (np.abs(pos - (n_ch - 1)) > EDGE)
        fl = np.floor(pos)
        k = fl.astype(np.int64)
        ok = (k >= 0) & (k < n_ch - 1)
        kk = np.clip(k, 0, n_ch - 2)
        w = pos - fl
        q0, q1 = qd[v][:, kk], qd[v][:, kk + 1]                          # [rows][N][N]
        ref += np.where(ok, ((1.0 - w) * q0 + w * q1) / l2, 0.0)
        mag += np.where(ok, (np.abs(q0) + np.abs(q1)) / l2, 0.0)
    return ref * dbeta, (n_views + 8.0) * U * abs(dbeta) * mag, np.broadcast_to(keep, ref.shape)


def fdk_ref(q, view_cs, row_weight, sid, sdd, dgamma, dbeta, row_z0, row_dz, src_z, n_matrix, fov, n_slices, z0, dz):
    """q float32 [n_views][n_rows][n_ch], row_weight float32 [n_rows] -> (ref, bound, keep) [n_slices][n_matrix][n_matrix]."""
    n_views, n_rows, n_ch = q.shape
    qd, rw = q.astype(F64), row_weight.astype(F64)
    x, y = _pixels(n_matrix, fov)
    ref = np.zeros((n_slices, n_matrix, n_matrix))
    mag = np.zeros_like(ref)
    keep = np.ones_like(ref, dtype=bool)
    for v in range(n_views):
        pos, l2 = _channel_pos(x, y, view_cs[v, 0], view_cs[v, 1], sid, dgamma, n_ch)
        keep &= ((np.abs(pos) > EDGE) & (np.abs(pos - (n_ch - 1)) > EDGE))[None]
        fl = np.floor(pos)
        k = fl.astype(np.int64)
        ok = (k >= 0) & (k < n_ch - 1)
        kk = np.clip(k, 0, n_ch - 2)
        w = pos - fl
        m = sdd / np.sqrt(l2)
        for s in range(n_slices):
            z = z0 + s * dz
            rpos = (src_z + (z - src_z) * m - row_z0) * (1.0 / row_dz)
            keep[s] &= (np.abs(rpos) > EDGE) & (np.abs(rpos - (n_rows - 1)) > EDGE)
            rfl = np.floor(rpos)
            r0 = rfl.astype(np.int64)
            okr = ok & (r0 >= 0) & (r0 < n_rows - 1)
            rr = np.clip(r0, 0, n_rows - 2)
            wr = rpos - rfl
            a0, a1, b0, b1 = qd[v, rr, kk], qd[v, rr, kk + 1], qd[v, rr + 1, kk], qd[v, rr + 1, kk + 1]
            va = ((1.0 - w) * a0 + w * a1) * rw[rr]
            vb = ((1.0 - w) * b0 + w * b1) * rw[rr + 1]
            ref[s] += np.where(okr, ((1.0 - wr) * va + wr * vb) / l2, 0.0)
            mag[s] += np.where(okr, ((np.abs(a0) + np.abs(a1)) * rw[rr] + (np.abs(b0) + np.abs(b1)) * rw[rr + 1]) / l2, 0.0)
    return ref * dbeta, (n_views + 12.0) * U * abs(dbeta) * mag, keep


def vmi_ref(m1, m2, u1, u2, u_water, hu):
    v = u1 * m1.astype(F64) + u2 * m2.astype(F64)
    if hu:
        v = 1000.0 * (v - u_water) / u_water
    return v.astype(F32)


def moments_ref(m1, m2, labels, n_labels):
    """[n_labels][6] in longdouble: count, S m1, S m2, S m1^2, S m1 m2, S m2^2 over the pixels of each label."""
    L = np.longdouble
    a = m1.astype(L)
    b = np.zeros_like(a) if m2 is None else m2.astype(L)
    lab = np.zeros(a.size, np.int64) if labels is None else labels.astype(np.int64)
    out = np.zeros((n_labels, 6), L)
    for l in range(n_labels):
        s = lab == l
        out[l] = [s.sum(), a[s].sum(), b[s].sum(), (a[s] * a[s]).sum(), (a[s] * b[s]).sum(), (b[s] * b[s]).sum()]
    return out


# ---- the geometries of the reconstruction cases --------------------------------------------------------------------------------

FAN = 0.8230337
SID, SDD = 60.0, 100.0


def view_table(n_views, theta0=0.013):
    th = theta0 + 2.0 * np.pi * np.arange(n_views) / n_views
    return np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], 1))


# dexct_fbp_backproject: (n_views, n_channels, n_rows, n_matrix, fov); rows 1 and 7 take fbp_backproject_kernel<1>, 8, 9 and 17
# <8> (a whole group, one row and one row past whole groups); n_matrix around the 64 x 4 pixel blocks
BACKPROJECT = [(12, 2, 1, 1, 20.0), (9, 3, 7, 3, 30.0), (16, 255, 8, 63, 36.0), (11, 256, 9, 64, 44.0), (7, 257, 17, 65, 40.0),
               (13, 53, 1, 70, 52.0)]
# dexct_fdk_backproject: (n_views, n_channels, n_rows, n_matrix, fov, n_slices); fdk_backproject_kernel<4>: slices 1, 3, 4, 5
FDK = [(10, 3, 2, 3, 30.0, 1), (12, 255, 3, 63, 36.0, 3), (9, 256, 9, 64, 40.0, 4), (8, 257, 9, 65, 40.0, 5), (7, 2, 2, 70, 20.0, 4),
       (6, 64, 3, 1, 10.0, 5)]


def backproject_problem(case, seed=0):
    n_views, n_ch, n_rows, n_matrix, fov = case
    rng = np.random.default_rng(seed + n_ch * 31 + n_matrix)
    q = (rng.standard_normal((n_views, n_rows, n_ch)) * 3.0).astype(F32)
    return dict(q=q, view_cs=view_table(n_views), sid=SID, dgamma=FAN / n_ch, dbeta=2.0 * np.pi / n_views, n_matrix=n_matrix, fov=fov)


def fdk_problem(case, seed=0):
    n_views, n_ch, n_rows, n_matrix, fov, n_slices = case
    rng = np.random.default_rng(seed + n_ch * 17 + n_matrix)
    q = (rng.standard_normal((n_views, n_rows, n_ch)) * 3.0).astype(F32)
    row_dz, src_z = 0.37, 0.11
    row_z0 = -0.5 * (n_rows - 1) * row_dz + 0.023
    row_z = row_z0 + row_dz * np.arange(n_rows)
    rw = (SDD / np.sqrt(SDD ** 2 + (row_z - src_z) ** 2)).astype(F32)
    dz = 0.05
    return dict(q=q, view_cs=view_table(n_views), row_weight=rw, sid=SID, sdd=SDD, dgamma=FAN / n_ch, dbeta=2.0 * np.pi / n_views,
                row_z0=row_z0, row_dz=row_dz, src_z=src_z, n_matrix=n_matrix, fov=fov, n_slices=n_slices,
                z0=-0.5 * (n_slices - 1) * dz + 0.017, dz=dz)


# ---- the scans of the projection cases -----------------------------------------------------------------------------------------

class Scan:
    """A fan or cone scan for the bare C ABI: geometry numbers, the float64 angle tables every implementation starts from, a
    uint8 volume [nz][ny][nx] of ids 0 .. n_mat - 1 and the float32 tables mu [M][n_e], w / w2 [S][n_e]."""

    def __init__(self, nx, ny, nz, n_views, n_ch, n_rows, z_first=0, n_mat=3, n_e=5, n_spec=2, fan=0.16, seed=0, air=False,
                 dx=0.31, dy=0.27, dz=0.4, sid=SID, sdd=SDD, cone_h=None, src_z=0.0, theta0=0.0, row_centre=None):
        rng = np.random.default_rng(seed * 1000 + nx * 7 + ny * 3 + nz + n_mat)
        self.nx, self.ny, self.nz, self.n_views, self.n_ch, self.n_rows, self.z_first = nx, ny, nz, n_views, n_ch, n_rows, z_first
        self.n_mat, self.n_e, self.n_spec = n_mat, n_e, n_spec
        self.dx, self.dy, self.dz, self.sid, self.sdd = dx, dy, dz, sid, sdd
        th = theta0 + 2.0 * np.pi * np.arange(n_views) / n_views
        gam = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * (fan / n_ch)
        self.view_cs = np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], 1))
        self.chan_cs = np.ascontiguousarray(np.stack([np.cos(gam), np.sin(gam)], 1))
        yy, xx = np.mgrid[0:ny, 0:nx]
        disc = ((xx - 0.5 * nx + 0.5) / (0.45 * nx)) ** 2 + ((yy - 0.5 * ny + 0.5) / (0.45 * ny)) ** 2 < 1.0
        ids = rng.integers(1, n_mat, (nz, ny, nx), dtype=np.int64) if n_mat > 1 else np.zeros((nz, ny, nx), np.int64)
        self.vol = np.zeros((nz, ny, nx), np.uint8) if air else np.where(disc[None], ids, 0).astype(np.uint8)
        E = np.linspace(30.0, 120.0, n_e) if n_e > 1 else np.array([60.0])
        mu = rng.uniform(0.05, 0.5, (n_mat, 1)) * (E[None, :] / 60.0) ** -rng.uniform(0.3, 2.5, (n_mat, 1))
        mu[0] = 2e-4
        self.mu = mu.astype(F32)
        w = rng.uniform(1e3, 1e4, (n_spec, n_e))
        if n_e >= 8 and n_spec >= 2:
            w[1, n_e // 2:] = 0.0                                        # a spectrum that weights no energy of the upper half
        self.w = w.astype(F32)
        self.w2 = (self.w * (E / 60.0).astype(F32)[None, :]).astype(F32)
        self.cone = cone_h is not None
        self.src_z = src_z
        self.row_z = (np.arange(n_rows) - 0.5 * (n_rows - 1)) * cone_h if self.cone else None
        if row_centre is not None:                                       # the rows centred on another height than 0
            self.row_z = self.row_z + row_centre

    def geom(self, make):
        """``make``: c_oracle.make_geom or a constructor of _native.FanGeom with the same twelve numbers."""
        return make(self.n_views, self.n_ch, self.n_rows, self.z_first, self.nx, self.ny, self.nz, self.dx, self.dy, self.dz,
                    self.sid, self.sdd)

    @property
    def max_abs_dz(self):
        return float(np.max(np.abs(self.row_z - self.src_z)))


class _Tables:
    """What on_plane_rays asks of a scanner object: the two angle tables."""

    def __init__(self, scan):
        self.view_cs, self.chan_cs = (lambda: scan.view_cs), (lambda: scan.chan_cs)


def tie_rays(scan, view_begin, view_end):
    """[local views][channels] mask of the rays that run exactly along a grid plane (on_plane_rays of tests/test_gpu_siddon.py)."""
    from oracle import c_oracle as co
    from test_gpu_siddon import on_plane_rays
    return on_plane_rays(scan.geom(co.make_geom), _Tables(scan), scan.n_views)[view_begin:view_end]


def counts_rel(got, ref, tie):
    """got, ref [S][views][rows][channels]; ``tie`` [views][channels] rays left out: the largest relative difference (inf when
    ``got`` holds a NaN or an inf anywhere, a tie ray included)."""
    live = ~np.broadcast_to(tie[None, :, None, :], ref.shape)
    got = np.asarray(got, F64)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(np.abs(got - ref)[live] / ref[live], initial=0.0))


def counts_close(got, ref, tie, rel_tol):
    return counts_rel(got, ref, tie) < rel_tol


# The scans of tests/test_gpu_bounds_projection.py by name (tests/test_bounds_refs.py checks the tie-ray cap of each on the CPU).
# Small on purpose: the CPU oracle answers each in seconds.
def _rows(n_rows):
    return dict(nx=24, ny=20, nz=32, n_views=6, n_ch=53, n_rows=n_rows, z_first=16 if n_rows <= 16 else 0)


SCANS = {f'r{n}': _rows(n) for n in (1, 3, 4, 5, 15, 16, 17)}
SCANS.update({
    'r66': dict(nx=24, ny=20, nz=96, n_views=6, n_ch=53, n_rows=66, z_first=16),     # aligned volume (nz 96), ragged last lane
    'r255': dict(nx=12, ny=10, nz=272, n_views=3, n_ch=5, n_rows=255, theta0=0.2, fan=0.06),
    'r256': dict(nx=12, ny=10, nz=272, n_views=3, n_ch=5, n_rows=256, theta0=0.2, fan=0.06),
    'r257': dict(nx=12, ny=10, nz=272, n_views=3, n_ch=5, n_rows=257, theta0=0.2, fan=0.06),
    'r1100': dict(nx=10, ny=8, nz=1104, n_views=2, n_ch=3, n_rows=1100, theta0=0.2, fan=0.06),  # the packed kernel's second z-chunk
    'c1': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=1, n_rows=8, theta0=0.1),
    'c2': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=2, n_rows=8, theta0=0.1),
    'v1': dict(nx=24, ny=20, nz=16, n_views=1, n_ch=53, n_rows=8, theta0=0.3),
    's3': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=53, n_rows=8, n_spec=3),
    's4': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=53, n_rows=8, n_spec=4, n_e=9),
    's1': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=53, n_rows=8, n_spec=1, n_e=9),
    'wide': dict(nx=16, ny=16, nz=16, n_views=4, n_ch=32, n_rows=8, fan=0.6, theta0=0.05),       # some rays miss the grid
    'air': dict(nx=24, ny=20, nz=16, n_views=6, n_ch=53, n_rows=8, air=True),
    'slabs': dict(nx=560, ny=24, nz=16, n_views=4, n_ch=9, n_rows=8, dx=0.05, dy=0.3, fan=0.1, theta0=0.01),   # > 512 slabs per ray
    'cone': dict(nx=24, ny=20, nz=24, n_views=6, n_ch=53, n_rows=10, cone_h=0.8, src_z=0.3),
    'cone256': dict(nx=10, ny=8, nz=250, n_views=3, n_ch=5, n_rows=70, dz=0.05, cone_h=0.2, src_z=0.3, theta0=0.2, fan=0.06),
    'cone512': dict(nx=10, ny=8, nz=500, n_views=3, n_ch=5, n_rows=70, dz=0.05, cone_h=0.2, src_z=0.3, theta0=0.2, fan=0.06),
    'cone1024': dict(nx=10, ny=8, nz=1000, n_views=3, n_ch=5, n_rows=70, dz=0.05, cone_h=0.2, src_z=0.3, theta0=0.2, fan=0.06),
    'cone1040': dict(nx=10, ny=8, nz=1040, n_views=3, n_ch=5, n_rows=70, dz=0.05, cone_h=0.2, src_z=0.3, theta0=0.2, fan=0.06),
})
MATERIALS = [1, 2, 3, 4, 5, 7, 16, 17, 32, 33, 48, 49, 200]
SCANS.update({f'm{m}': dict(nx=24, ny=20, nz=16, n_views=4, n_ch=21, n_rows=8, n_mat=m, n_e=3 if m > 40 else 5, theta0=0.07)
              for m in MATERIALS})
SCANS.update({f'cm{m}': dict(nx=16, ny=12, nz=24, n_views=3, n_ch=11, n_rows=10, n_mat=m, n_e=3, cone_h=0.8, src_z=0.3, theta0=0.07)
              for m in MATERIALS})
# cone scans of two materials for the <2, ...> instantiations of the row kernels
# cone scans of 1, 3 and 4 spectra; of air only; with a fan wider than the grid (rays that miss it in the plane); with detector
# rows far above and below the volume (rays that leave it through its top and bottom faces, the outer rows missing it altogether)
SCANS['cs1'] = dict(SCANS['cone'], n_spec=1, n_e=9)
SCANS['cs3'] = dict(SCANS['cone'], n_spec=3)
SCANS['cs4'] = dict(SCANS['cone'], n_spec=4, n_e=9)
SCANS['cone_air'] = dict(SCANS['cone'], air=True)
SCANS['cone_wide'] = dict(SCANS['cone'], fan=0.6, theta0=0.05)
SCANS['cone_tall'] = dict(SCANS['cone'], cone_h=3.0, theta0=0.05)
SCANS['cone_m2'] = dict(SCANS['cone'], n_mat=2)
SCANS['cone1040_m2'] = dict(SCANS['cone1040'], n_mat=2)
SCANS['cone1040_m1'] = dict(SCANS['cone1040'], n_mat=1)


# ---- cone scans at the edge of the slope contract -------------------------------------------------------------------------------
# proj::cone_slope_ok (csrc/proj_host.h) accepts a cone scan when f = max_abs_dz / sdd / dz * max(dx, dy) * sqrt(2) <= 1: no ray
# climbs more than one slice per dominant-axis slab.  The scans above have f <= 0.15; those below have max_abs_dz EQUAL to the
# largest float64 the predicate accepts (edge90: 0.9 of it).  In slices per slab a ray climbs |sw| = f hypot(dx, dy) /
# (sqrt(2) max(dx, dy)) at the most, at the dominant-axis switch, so only dx = dy reaches one slice per slab: edge_aniso keeps
# dy within 1 % of dx (|sw| <= 0.995) and takes its anisotropy from dz.  Odd nx, ny and channel counts: the central ray of an
# axis-aligned view runs through the middle of a voxel row, not along a grid plane.

SQRT2 = 1.4142135623730951


def slope_ok(max_abs_dz, dx, dy, dz, sdd):
    """proj::cone_slope_ok restated: the same float64 operations in the same order."""
    dmax = dx if dx > dy else dy
    return max_abs_dz >= 0 and not (max_abs_dz / sdd / dz * dmax * SQRT2 > 1.0)


def slope_limit(dx, dy, dz, sdd):
    """The largest float64 max_abs_dz that slope_ok accepts."""
    m = sdd * dz / (max(dx, dy) * SQRT2)
    while not slope_ok(m, dx, dy, dz, sdd):
        m = float(np.nextafter(m, -np.inf))
    while slope_ok(float(np.nextafter(m, np.inf)), dx, dy, dz, sdd):
        m = float(np.nextafter(m, np.inf))
    return m


def _row_reach(n_rows, cone_h, src_z, row_centre):
    """max_abs_dz of a Scan with these rows (the operations of Scan.__init__ and Scan.max_abs_dz)."""
    row_z = (np.arange(n_rows) - 0.5 * (n_rows - 1)) * cone_h
    if row_centre is not None:
        row_z = row_z + row_centre
    return float(np.max(np.abs(row_z - src_z)))


def _edge(share=1.0, **kw):
    """Scan arguments whose row pitch makes max_abs_dz exactly ``share`` of the slope limit (share 1: the limit itself, to the
    last bit: the pitch next to limit / half_rows whose rounded row heights give it)."""
    kw = dict(dict(nx=21, ny=17, nz=96, n_views=8, n_ch=15, n_rows=17, dx=0.2, dy=0.2, dz=0.2, sid=9.0, sdd=16.0, theta0=np.pi / 4), **kw)
    limit = slope_limit(kw['dx'], kw['dy'], kw['dz'], kw['sdd'])
    src_z, centre, n_rows = kw.get('src_z', 0.0), kw.get('row_centre'), kw['n_rows']
    h = share * limit / (0.5 * (n_rows - 1))
    if share == 1.0:
        lo = hi = h
        for _ in range(256):
            if _row_reach(n_rows, lo, src_z, centre) == limit or _row_reach(n_rows, hi, src_z, centre) == limit:
                break
            lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))
        h = lo if _row_reach(n_rows, lo, src_z, centre) == limit else hi
        assert _row_reach(n_rows, h, src_z, centre) == limit, kw
    return dict(kw, cone_h=h)


_TALL = dict(nx=11, ny=9, n_ch=5, n_rows=33, dz=0.05, src_z=0.3, row_centre=0.3)        # as cone256 .. cone1040, steep
EDGE_SCANS = {
    # diagonal views with |ex| == |ey| and axis-aligned ones; the outermost rows stay inside the 96 slices
    'edge': _edge(),
    'edge_m2': _edge(n_mat=2), 'edge_m1': _edge(n_mat=1), 'edge_m5': _edge(n_mat=5), 'edge_m7': _edge(n_mat=7),
    # 16 slices: rays enter and leave through the z faces; the steep rows pass far above and below the volume
    'edge_thin': _edge(nz=16),
    # the source above the top face (1.6 cm) of that volume, at the height from which the steepest row runs down through its
    # centre; the rows centred on the source
    'edge_above': _edge(nz=16, src_z=6.5, row_centre=6.5),
    # views from atan2(dy, dx): the central ray sits on the dominant-axis switch of a grid with dx != dy != dz
    'edge_aniso': _edge(dy=0.198, dz=0.25, nz=80, theta0=float(np.arctan2(0.198, 0.2))),
    # every staged-column width of cone_cols_kernel (288, 544, 1056 bytes) and cone_rows_kernel (more than 1024 slices)
    'edge288': _edge(nz=250, **_TALL), 'edge544': _edge(nz=500, **_TALL), 'edge1056': _edge(nz=1000, **_TALL),
    'edge1040': _edge(nz=1040, **_TALL),
    # a second chunk of 256 lanes with one live lane
    'edge_r257': _edge(nx=11, ny=9, nz=64, n_views=4, n_ch=5, n_rows=257),
    # 131 slabs on a diagonal of 0.05 cm voxels (the byte counters flush after 128); the source at the height from which the
    # steepest row runs down through the centre of the volume
    'edge_slabs': _edge(nx=131, ny=131, nz=144, n_ch=5, n_rows=9, dx=0.05, dy=0.05, dz=0.05, src_z=6.375, row_centre=6.375),
    # inside the range no other scan reaches, off the rounding edge
    'edge90': _edge(share=0.9),
}
SCANS.update(EDGE_SCANS)


def cone_rays_f64(s):
    """Per-ray figures of a cone scan in float64 / in the mirror's integers, [views][rows][channels] each: 'SW' (the slice
    step per slab in 2^-40, as orc_cone_pathlen rounds it), 'past' (how many slices the ray's slice coordinate w0 + i sw runs
    past the nearer z face over the plan's slab range; <= 0 inside, -inf for a ray without slabs) and 'ties' (slabs whose two
    crossing fractions tv and tw, restated in float32 as dda_slab and orc_cone_pathlen form them, are equal and below 1)."""
    from oracle import c_oracle as co
    plan = co.plan(s.geom(co.make_geom), s.view_cs, s.chan_cs, 0, s.n_views).reshape(s.n_views, 1, s.n_ch)
    cb, sb = s.view_cs[:, 0][:, None, None], s.view_cs[:, 1][:, None, None]
    cg, sg = s.chan_cs[:, 0][None, None, :], s.chan_cs[:, 1][None, None, :]
    sx, sy = s.sid * cb, s.sid * sb
    ex, ey = -(cb * cg - sb * sg), -(sb * cg + cb * sg)
    axis = (plan['flags'] & 1).astype(np.int64)
    su = np.where(axis == 0, sx / s.dx + 0.5 * s.nx, sy / s.dy + 0.5 * s.ny)
    eu = np.where(axis == 0, ex / s.dx, ey / s.dy)
    ws = s.src_z / s.dz + 0.5 * s.nz
    sw = ((s.row_z[None, :, None] - s.src_z) / s.dz) / (s.sdd * eu)
    w0 = ws - su * sw
    one = 2.0 ** 40
    SW, W0 = np.rint(sw * one).astype(np.int64), np.rint(w0 * one).astype(np.int64)
    i0, n = plan['i_first'].astype(np.int64), plan['n_slabs'].astype(np.int64)
    wa, wb = w0 + i0 * sw, w0 + (i0 + n) * sw
    past = np.maximum(np.maximum(-wa, -wb), np.maximum(wa, wb) - s.nz)
    past = np.where(n > 0, past, -np.inf)
    # the two crossing fractions of every slab (float32, operation for operation as the mirror)
    with np.errstate(divide='ignore'):
        kfw = (np.minimum(np.where(SW != 0, one / np.abs(SW.astype(F64)), 2.0 ** 24), 2.0 ** 24) * 2.0 ** -32).astype(F32)
    wpos = np.where(SW > 0, 0xFFFFFFFF, 0).astype(np.uint32)
    smask = np.where(plan['flags'] & 2, 0xFFFFFFFF, 0).astype(np.uint32)
    ties = np.zeros(SW.shape, np.int64)
    frac = lambda X, mask, k: np.minimum(((((X >> 8) & 0xFFFFFFFF).astype(np.uint32)) ^ mask).astype(F32) * k, F32(1.0))
    for k in range(int(n.max(initial=0))):
        i = i0 + k
        tv = frac(plan['V0'] + i * plan['SV'], smask, plan['kf'])
        tw = frac(W0 + i * SW, wpos, kfw)
        ties += (k < n) & (tv == tw) & (tv < 1.0)
    return dict(SW=SW, past=past, ties=ties)


_scans = {}


def scan(name):
    if name not in _scans:
        _scans[name] = Scan(**SCANS[name])
    return _scans[name]
