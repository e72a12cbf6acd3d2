"""First-order beam-hardening correction (BHC): the reference's ``recon_{water,bone}BHC`` images (plots.py:184-195).

A polychromatic log sinogram is not linear in path length: for a ray through L cm of a material m, ``get_sino``'s
``ln(air / counts)`` holds

    P_m(L) = -ln( sum_e w_e exp(-mu_m(e) L) / sum_e w_e ),

with ``w_e = forward_project.effective_weights(ct, spec)`` (full energy grid, zero-weight bins dropped) and
``mu_m(e) = density_m * xcompy.mixatten(formula_m, spec.E)`` (the recipe of ``VoxelPhantom.mu_table``, so a
``DEXCT_XCOM_DIR`` table is used when set).  P_m is strictly increasing and concave - its slope is the mean
attenuation of the hardened spectrum - so it has a unique inverse, also for p < 0 (L < 0: noisy counts above air).
Linearisation replaces every value by

    p' = mu_ref * P_m^{-1}(p),    mu_ref = P_m'(0) = sum w mu_m / sum w  by default,

the thickness of m that gives p, as an attenuation.  For water, mu_ref equals ``back_project.water_mu(ct, spec)``, the
HU reference of ``get_recon``: after water BHC, water reads 0 HU.  After bone BHC bone is linear instead, and water
reads whatever bone's linearisation makes of it (not 0 HU).

The inverse is tabulated once per (weights, material, mu_ref), in float64 on the host, and cached.  Each node holds
``mu_ref * L_k`` and ``mu_ref / P_m'(L_k)`` (value and slope of cubic Hermite cells), L_k solved to 1e-14 relative.
The nodes are not uniform in p: the bundled kV spectra reach down to 2 keV, where water's mu is ~700 /cm, so the
inverse changes at every scale of p towards 0 (a uniform grid of 8160 nodes over [-1, 40] misses it by 1e-2).  They
follow the float32 format instead, in a = |p| and separately for each sign: a linear run of C cells over
[0, 2^-20], then C cells per octave up to 2^6 = 64 (p >= 0; 4e-28 x air) and up to 2^0 = 1 (p < 0; e x air).  The
kernel reads cell and fraction straight from the exponent and mantissa bits of p.  The builder takes the smallest C
(8 ... 128) whose cells all agree with the float64 inverse to 1e-7 relative (1e-12 absolute near p = 0; the builder
asks 5e-8) at their quarter points and midpoints, and raises if none within the kernel's 8192 nodes does.  Beyond the last node of a
side the table extends linearly from that node; non-finite values pass through.  The device evaluation is the HIP
kernel ``dexct_bhc_linearize`` (include/dexct.h).

Materials: 'water' (``back_project.WATER`` at 1 g/cm^3), 'bone' (ICRU bone, ``matdecomp.matcomp2`` at
``matdecomp.density2``, the reference's own basis material), any ``system.Material`` or a ``(formula, density)`` tuple.
"""
import os

import numpy as np
import torch

from . import _device, _native, xcompy
from ._device import ptr, stream_ptr
from .forward_project import effective_weights

LOG2_MIN = -20                           # the linear run of cells covers |p| <= 2^-20
OCT_POS, OCT_NEG = 26, 20                # octaves: p < 2^6 = 64 and p >= -2^0 = -1
CELLS_LOG2 = (3, 4, 5, 6, 7)             # candidate cells per octave (2^7: 6146 nodes)
MAX_NODES = 8192                         # DEXCT_BHC_MAX_NODES
TOL = 1e-7                               # relative error of the Hermite table against the float64 inverse ...
BUILD_TOL = 0.5 * TOL                    # ... which the builder meets at its check points with a factor 2 to spare
ABS_TOL = 1e-12                          # absolute floor of that check near p = 0


def material_of(material):
    """(name, formula, density) of 'water', 'bone', a system.Material or a (formula, density) tuple."""
    if isinstance(material, str):
        if material == 'water':
            from .back_project import WATER
            return 'water', WATER, 1.0
        if material == 'bone':
            from . import matdecomp as md
            return 'bone', md.matcomp2, float(md.density2)
        raise ValueError(f"unknown BHC material {material!r}: 'water', 'bone', a Material or (formula, density)")
    if hasattr(material, 'matcomp') and hasattr(material, 'density'):
        return getattr(material, 'name', material.matcomp), material.matcomp, float(material.density)
    formula, density = material
    return str(formula), str(formula), float(density)


class SpectralLog:
    """P(L) of one (weights, attenuation) pair in float64, with its slope and inverse."""

    def __init__(self, w, mu):
        w, mu = np.asarray(w, dtype=np.float64), np.asarray(mu, dtype=np.float64)
        keep = w != 0.0
        if not np.any(keep):
            raise ValueError('the spectrum has no detected weight')
        if np.any(w[keep] < 0) or np.any(mu[keep] <= 0) or not np.all(np.isfinite(mu[keep])):
            raise ValueError('BHC needs non-negative weights and positive, finite attenuation')
        self.q = w[keep] / np.sum(w[keep])                   # normalised weights
        self.lw = np.log(self.q)
        self.mu = mu[keep]
        self.mu_mean = float(np.sum(w * np.where(keep, mu, 0.0)) / np.sum(w))    # P'(0), summed as back_project.water_mu
        self.mu_min, self.mu_max = float(self.mu.min()), float(self.mu.max())

    def __call__(self, L):
        """P(L) for an array of L: log1p of a sum of expm1 terms near 0 (full relative precision), log-sum-exp beyond."""
        L = np.asarray(L, dtype=np.float64)
        out = np.empty(L.shape)
        small = np.abs(L) * self.mu_max < 0.5
        out[small] = -np.log1p(np.sum(self.q * np.expm1(-self.mu * L[small][:, None]), axis=1))
        a = self.lw - self.mu * L[~small][:, None]
        m = a.max(axis=1)
        out[~small] = -(m + np.log(np.sum(np.exp(a - m[:, None]), axis=1)))
        return out

    def slope(self, L):
        """P'(L) = mean attenuation of the spectrum hardened by L: sum w mu exp(-mu L) / sum w exp(-mu L)."""
        a = self.lw - self.mu * np.asarray(L, dtype=np.float64)[..., None]
        e = np.exp(a - a.max(axis=-1, keepdims=True))
        return np.sum(e * self.mu, axis=-1) / np.sum(e, axis=-1)

    def inverse(self, p, rtol=1e-14):
        """L with P(L) = p (float64 array): Newton steps kept inside a bracket that shrinks with every evaluation.
        The bracket follows from concavity: P(L) <= mu_mean L, and mu_min <= P' <= mu_max."""
        p = np.asarray(p, dtype=np.float64)
        a, b = p / self.mu_mean, np.where(p > 0, p / self.mu_min, p / self.mu_max)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        L = a
        for _ in range(200):
            f = self(L) - p
            lo = np.where(f < 0, L, lo)
            hi = np.where(f > 0, L, hi)
            Ln = L - f / self.slope(L)
            Ln = np.where((Ln > lo) & (Ln < hi), Ln, 0.5 * (lo + hi))
            done = (np.abs(Ln - L) <= rtol * np.abs(Ln)) | (hi - lo <= rtol * np.abs(Ln))
            L = Ln
            if np.all(done):
                break
        else:
            raise RuntimeError('BHC: the inverse of P did not converge')
        return np.where(p == 0, 0.0, L)


def node_a(j, cells_log2, log2_min=LOG2_MIN):
    """|p| of node j of one side: a linear run of C = 2^cells_log2 cells over [0, 2^log2_min], then C per octave."""
    j = np.asarray(j, dtype=np.int64)
    C = 1 << cells_log2
    o = np.maximum(j // C - 1, 0)
    return np.where(j <= C, np.ldexp(j.astype(np.float64), log2_min - cells_log2),
                    np.ldexp(1.0 + (j - C * (1 + o)) / C, log2_min + o))


class LinearizationTable:
    """The tabulated inverse of one (spectrum, detector, material, mu_ref) in float64: per node {value, d value / d|p|},
    the p >= 0 side first (``oct_pos`` octaves), then the p < 0 side (``oct_neg`` octaves) - the layout of
    dexct_bhc_linearize (include/dexct.h).  ``device(dev)`` gives the float32 pairs the kernel stages."""

    def __init__(self, material, mu_ref, cells_log2, value, slope, log2_min=LOG2_MIN, oct_pos=OCT_POS, oct_neg=OCT_NEG):
        self.material, self.mu_ref = material, float(mu_ref)
        self.cells_log2, self.log2_min, self.oct_pos, self.oct_neg = int(cells_log2), int(log2_min), int(oct_pos), int(oct_neg)
        C = 1 << self.cells_log2
        self.base_neg = C * (1 + self.oct_pos) + 1
        self.n_nodes = self.base_neg + C * (1 + self.oct_neg) + 1
        self.value, self.slope = np.asarray(value, dtype=np.float64), np.asarray(slope, dtype=np.float64)
        if self.value.shape != (self.n_nodes,) or self.slope.shape != (self.n_nodes,):
            raise ValueError('table size does not match its grid')
        self._dev = {}

    def side_a(self, neg):
        """|p| of the nodes of one side, ascending."""
        C = 1 << self.cells_log2
        return node_a(np.arange(C * (1 + (self.oct_neg if neg else self.oct_pos)) + 1), self.cells_log2, self.log2_min)

    @property
    def nodes(self):
        """p of every node, ascending (p = 0 once)."""
        return np.concatenate([-self.side_a(True)[:0:-1], self.side_a(False)])

    @property
    def p_range(self):
        """(first, last) node: linear extrapolation beyond."""
        return -2.0 ** (self.log2_min + self.oct_neg), 2.0 ** (self.log2_min + self.oct_pos)

    def pairs(self):
        """[n_nodes, 2] float32 {value, slope}: the table the kernel stages."""
        return np.stack([self.value, self.slope], axis=1).astype(np.float32)

    def device(self, dev):
        t = self._dev.get(str(dev))
        if t is None:
            t = self._dev[str(dev)] = torch.from_numpy(self.pairs()).to(dev)
        return t

    def evaluate(self, p):
        """The kernel's formula in float64 on the float64 table (NumPy): any shape, float64 out."""
        p = np.asarray(p, dtype=np.float64)
        out = p.copy()
        C, K, E = 1 << self.cells_log2, self.cells_log2, self.log2_min
        with np.errstate(invalid='ignore', over='ignore'):
            for neg in (False, True):
                sel = (p < 0) if neg else (p >= 0)
                a = np.abs(p[sel])
                base, n_oct = (self.base_neg, self.oct_neg) if neg else (0, self.oct_pos)
                v, s = self.value[base:], self.slope[base:]
                _, ex = np.frexp(a)
                o = np.where(a == 0, -1, ex - 1 - E)
                beyond = (o >= n_oct) | np.isinf(a)
                o = np.where(beyond, 0, o)
                res = np.empty(a.shape)
                end = C * (1 + n_oct)
                res[beyond] = v[end] + (a[beyond] - 2.0 ** (E + n_oct)) * s[end]
                lin = ~beyond & (o < 0)
                u = a[lin] * 2.0 ** (K - E)
                j = np.floor(u).astype(np.int64)
                res[lin] = _cell(v, s, j, u - j, 2.0 ** (E - K))
                octv = ~beyond & (o >= 0)
                oo = o[octv]
                start = np.ldexp(1.0, E + oo)
                w = start / C
                u = (a[octv] - start) / w
                c = np.floor(u).astype(np.int64)
                res[octv] = _cell(v, s, C * (1 + oo) + c, u - c, w)
                out[sel] = res
        return out


def _cell(v, s, j, t, w):
    """Cubic Hermite between nodes j and j + 1 of a cell of width w (the kernel's basis form)."""
    r = 1.0 - t
    h01 = t * t * (3.0 - 2.0 * t)
    return (1.0 - h01) * v[j] + h01 * v[j + 1] + w * (t * r * (r * s[j] - t * s[j + 1]))


def build_table(w, mu, material='material', mu_ref=None):
    """Tabulate mu_ref * P^{-1} for weights ``w`` and attenuation ``mu`` on one energy grid (see the module docstring)."""
    P = SpectralLog(w, mu)
    mu_ref = P.mu_mean if mu_ref is None else float(mu_ref)
    if not mu_ref > 0:
        raise ValueError('mu_ref must be positive')
    worst = None
    for k in CELLS_LOG2:
        C = 1 << k
        if C * (2 + OCT_POS + OCT_NEG) + 2 > MAX_NODES:
            break
        value, slope, q = [], [], []
        for sign, n_oct in ((1.0, OCT_POS), (-1.0, OCT_NEG)):
            a = node_a(np.arange(C * (1 + n_oct) + 1), k)
            L = P.inverse(sign * a)
            value.append(mu_ref * L)
            slope.append(sign * mu_ref / P.slope(L))
            # quarter points and midpoints of every cell
            q.append(sign * (a[:-1, None] + np.array([0.25, 0.5, 0.75])[None, :] * np.diff(a)[:, None]).ravel())
        t = LinearizationTable(material, mu_ref, k, np.concatenate(value), np.concatenate(slope))
        q = np.concatenate(q)
        exact = mu_ref * P.inverse(q)
        err = float(np.max(np.abs(t.evaluate(q) - exact) / (np.abs(exact) + ABS_TOL / TOL)))
        if err <= BUILD_TOL:
            t.check_error = err
            return t
        worst = (t.n_nodes, err)
    raise RuntimeError(f'BHC table for {material}: {worst[0]} nodes still miss the float64 inverse by {worst[1]:.2e} relative '
                       f'(> {BUILD_TOL:g}); the spectrum cannot be tabulated within {MAX_NODES} nodes')


_cache = {}


def linearization_table(ct, spec, material='water', mu_ref=None):
    """The cached LinearizationTable of (spectrum, detector, material, mu_ref); ``material`` as in material_of,
    ``mu_ref`` None for P_m'(0)."""
    name, formula, density = material_of(material)
    w = np.asarray(effective_weights(ct, spec), dtype=np.float64)
    E = np.asarray(spec.E, dtype=np.float64)
    key = (w.tobytes(), E.tobytes(), formula, density, None if mu_ref is None else float(mu_ref),
           os.environ.get('DEXCT_XCOM_DIR'))
    t = _cache.get(key)
    if t is None:
        t = _cache[key] = build_table(w, density * xcompy.mixatten(formula, E), name, mu_ref)
    return t


def linearize(sino_log, ct, spec, material='water', mu_ref=None):
    """Beam-hardening-corrected copy of a log sinogram (NumPy, any shape, float32 out), evaluated on the host."""
    t = linearization_table(ct, spec, material, mu_ref)
    return t.evaluate(np.asarray(sino_log, dtype=np.float32)).astype(np.float32)


def linearize_device(sino_d, table, out=None):
    """dexct_bhc_linearize on a float32 device tensor of any shape (contiguous; a view at any offset is fine).
    ``out``: a contiguous float32 tensor of the same shape, ``sino_d`` itself for in place, or None for a new one."""
    if not _device.on_gpu(sino_d) or sino_d.dtype != torch.float32 or not sino_d.is_contiguous():
        raise ValueError('linearize_device needs a contiguous float32 device tensor')
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != sino_d.shape
                            or not out.is_contiguous() or out.device != sino_d.device):
        raise ValueError("out must be a contiguous float32 tensor of the input's shape and device")
    if out is None:
        out = torch.empty_like(sino_d, memory_format=torch.contiguous_format)
    lib = _native.load()
    tab = table.device(sino_d.device)
    _native.check(lib.dexct_bhc_linearize(ptr(sino_d), sino_d.numel(), ptr(tab), table.log2_min, table.cells_log2,
                                          table.oct_pos, table.oct_neg, ptr(out), stream_ptr()), 'dexct_bhc_linearize')
    return out
