"""Forward projection: drop-in for the reference's ``xtomosim.forward_project.get_sino``.

``get_sino(ct, phantom, spec) -> (sino_raw, sino_log)`` is called at main.py:120 of the reference;
its source (x-tomo-sim) is not in the reference checkout, so the contract is reconstructed from the
callers: two ``[N_proj, N_channels]`` arrays, ``sino_raw`` in detected counts (matdecomp.py:30,179)
and ``sino_log`` the log-normalised sinogram fed to reconstruction (main.py:134).  Detection uses
the weighting that the reference's decomposition assumes (matdecomp.py:146-150):
``counts = sum_E I0(E) eta(E) [E if EID] dE exp(-sum_m mu_m(E) L_m)``, noise-free.

All work runs in the HIP library (dexct_fan_plan, dexct_volume_layouts, dexct_siddon_project).
"""
import collections
import ctypes as C
import os as _os

import numpy as np
import torch

from . import _native, _shard
from ._device import LazyPinnedResult, dense_input, device, pinned_empty, pool_wanted, ptr, side_streams, stream_ptr, to_dev, written


def effective_weights(ct, spec):
    """I0 * detector response * dE on the spectrum's own grid (matdecomp.py:142,146-150)."""
    return spec.I0 * ct.detector_response(spec.E) * spec.bin_widths()


def merged_tables(ct, phantom, specs, with_variance=False):
    """One energy grid for a fused multi-spectrum traversal.

    Each spectrum keeps its own quadrature: on the merged grid its weight is non-zero only at its
    own energies (no interpolation), bins that no spectrum weights are dropped.
    Returns E [nE], mu [M, nE] (float64, 1/cm), w [S, nE] (float64) and, with ``with_variance``,
    w2 = w * (detector signal per photon: E for an energy-integrating detector, 1 for a counting one).
    """
    E = np.unique(np.concatenate([s.E for s in specs]))
    w = np.zeros((len(specs), E.size))
    for k, s in enumerate(specs):
        w[k, np.searchsorted(E, s.E)] = effective_weights(ct, s)
    keep = np.any(w != 0.0, axis=0)
    E, w = E[keep], w[:, keep]
    if with_variance:
        return E, phantom.mu_table(E), w, w * (E if ct.eid else 1.0)
    return E, phantom.mu_table(E), w


def compact_ids(present, materials):
    """Which table rows a projection needs, and the renumbering of the ids: ``present[i]`` says whether id i occurs in the
    scanned voxels.  Ids with the same (density, composition) share a row (their rows of density x mixatten(E) are equal at
    every energy), absent ids get none, row 0 stays id 0 (its path length comes from the chord); at least two rows are kept
    when the table has them (the kernels' smallest table).  Returns (mat_rows, lut): mat_rows[k] = the id whose table row
    serves compact id k; lut[i] = compact id of id i (256 uint8 values; 0 for absent ids)."""
    mat_rows, lut, seen = [0], np.zeros(256, dtype=np.uint8), {}
    key = lambda m: (float(m.density), str(m.matcomp))
    seen[key(materials[0])] = 0
    for i in range(1, len(materials)):
        if present[i]:
            k = key(materials[i])
            if k not in seen:
                seen[k] = len(mat_rows)
                mat_rows.append(i)
            lut[i] = seen[k]
    if len(mat_rows) < 2 <= len(materials):
        mat_rows.append(1)
    return mat_rows, lut


# Where a projection kernel draws the noise sample itself: the limits proj::noise_log_args (csrc/proj_host.h) enforces
# (Projector._samples_in_kernel is their one reader on this side)
_NOISE_MAX_SPECTRA = 2          # the two slots of the packed stacked fan and of the groups' detection pass
_NOISE_MAX_GROUP_ROWS = 48      # table rows up to which the groups' detection pass samples (kManyMaterials)

# What Projector._launch needs of one project_tables call: the plan of its first view and that view's global number, the
# tables (device pointers), the unattenuated signals of the log, the kernel's noise (None: it draws none), the layout it
# writes, and whether the packed stacked fan serves this call
_Call = collections.namedtuple('_Call', 'plan_ptr vb S nE mu w w2 air nz run_layout packed')


def _in_view_chunks(launch, n_chunk, counts, pathlen, variance, log):
    """``launch(v0, v1, counts, pathlen, variance, log)`` over all views of the outputs, ``n_chunk`` views at a time (the
    view is dimension 1 of counts, variance and log, dimension 0 of pathlen; an output that is None stays None).  One chunk
    that covers every view writes into the outputs themselves; otherwise each chunk gets outputs of its own size, which
    are copied into place."""
    full = ((counts, 1), (pathlen, 0), (variance, 1), (log, 1))
    nV = counts.shape[1]
    if n_chunk >= nV:
        return launch(0, nV, counts, pathlen, variance, log)
    for v0 in range(0, nV, n_chunk):
        v1 = min(nV, v0 + n_chunk)
        part = [None if t is None else t.new_empty(t.shape[:d] + (v1 - v0,) + t.shape[d + 1:]) for t, d in full]
        launch(v0, v1, *part)
        for (t, d), p in zip(full, part):
            if t is not None:
                t.narrow(d, v0, v1 - v0).copy_(p)


class Projector:
    """Device-resident state of one (scanner, phantom) pair: volume layouts and ray plans.

    ``view_range`` restricts the instance to a contiguous shard of projection angles (one per
    rank in a multi-GPU run).  ``kernel``: 0 choose, 1 ray-parallel, 2 row-parallel (1 row per lane),
    3 row-parallel with 4 rows per lane (<= 4 materials, Nz and z_index multiples of 4), 4 the same kernel
    run once per group of three materials (5..256 materials), 5 the 4-rows-per-lane kernel with a tile of
    neighbouring (view, channel) pairs per workgroup walking the volume in step (rows4t_kernel: opt-in, kept for A/B
    runs - kernel 0 never picks it; same bits as kernel 3), 6 one wavefront per ray (lanes over
    dominant-axis slabs, shuffle reductions, tables in LDS: the mapping BASELINE.json's north star names; <= 4
    materials), 7 the stacked fan on a 2-bit packed volume with bit-sliced counters (rows16_kernel: 16 rows per
    lane; <= 4 materials; what kernel 0 picks from 192 rows on when a pair fills 3/4 of its lane group), 8 the same
    kernel run once per group of three materials on packed group codes (2..256 materials; what kernel 0 picks for more
    than 4 materials under the same conditions).
    """

    def __init__(self, ct, phantom, view_range=None, kernel=0, dev=None):
        self.lib = _native.load()
        self.dev = dev or device()
        self.ct, self.phantom = ct, phantom
        self.kernel = kernel
        vb, ve = view_range if view_range is not None else (0, ct.N_proj)
        if not (0 <= vb < ve <= ct.N_proj):
            raise ValueError(f'bad view range {view_range}')
        self.view_begin, self.view_end = int(vb), int(ve)
        self._bounds, self.quadrature_info = None, None
        self.cone = bool(getattr(ct, 'cone', False))
        z_first = 0 if self.cone else phantom.z_index
        if not self.cone and (z_first < 0 or z_first + ct.N_rows > phantom.Nz):
            raise ValueError(f'rows {ct.N_rows} from slice {z_first} do not fit Nz={phantom.Nz}')
        half_diag = 0.5 * np.hypot(phantom.Nx * phantom.dx, phantom.Ny * phantom.dy)
        if ct.SID <= half_diag or ct.SDD - ct.SID < half_diag:
            # line integrals run through the whole grid: a source or a detector inside it would silently see
            # material "behind" itself
            raise ValueError('source and detector must lie outside the phantom grid: SID > half diagonal and '
                             'SDD - SID >= half diagonal')
        volume, nz = phantom.volume, phantom.Nz
        if not self.cone and ct.N_rows < nz:
            # a stacked fan only ever reads its own slices: upload those (one slice of a 512^3 phantom for the
            # reference's single-row scan instead of 128 MiB)
            volume, nz, z_first = volume[z_first:z_first + ct.N_rows], ct.N_rows, 0
        st = stream_ptr()
        # ---- 1. the volume on the device, renumbered to compact ids (mat_rows, id_lut, n_mat)
        vol_raw = self._upload_compact_ids(volume, st)
        M = self.n_mat
        # ---- 2. the routes.  A row-parallel kernel (the rows of a (view, channel) pair as lanes) will run on a stacked fan
        # for kernels 2-5, 7, 8 and for kernel 0 from 64 rows on: it reads the z-fastest layout (vol_zf) and writes the
        # sinogram row fastest (native_layout 1).  A cone beam has neither (its row kernels read vol_zc, channel fastest).
        row_parallel = not self.cone and (kernel in (2, 3, 4, 5, 7, 8) or (kernel == 0 and ct.N_rows >= 64))
        self.native_layout = int(row_parallel)      # 1: [view][channel][row], 0: [view][row][channel]
        # the 2-bit packed volume with bit-sliced counters (rows16_kernel): what kernel 0 picks where it applies
        lanes16 = -(-ct.N_rows // 16)
        group16 = 64 * (-(-lanes16 // 64)) if lanes16 > 32 else (32 if lanes16 > 16 else 16)     # lanes the pair occupies
        shape2_ok = not self.cone and max(phantom.Nx, phantom.Ny) <= 2047
        # kernel 0 picks it when at least 3/4 of the pair's lane group carry rows (>= 192 rows)
        fills = ct.N_rows >= 192 and 4 * lanes16 >= 3 * group16
        packed2_ok = shape2_ok and 2 <= M <= 4                     # one fused pass: ids 0..3
        self.use_packed = (kernel == 7 and packed2_ok) or (kernel == 0 and packed2_ok and fills)
        if kernel == 7 and not packed2_ok:
            raise ValueError('kernel 7 (2-bit packed volume) needs a stacked fan, 2..4 materials and nx, ny <= 2047')
        # material groups (5..256 materials) on packed group codes: kernel 8 forces it, kernel 0 picks it like kernel 7
        self.grouped_packed = (kernel == 8 and shape2_ok and 2 <= M <= 256) or (kernel == 0 and shape2_ok and 4 < M <= 256 and fills)
        if kernel == 8 and not self.grouped_packed:
            raise ValueError('kernel 8 (material groups on the 2-bit packed volume) needs a stacked fan, 2..256 materials '
                             'and nx, ny <= 2047')
        # ---- 3. z padding.  Every row-parallel kernel but kernel 2 (one row per lane, byte loads) reads aligned dwords
        # along z - the packed volumes 16 slices at a time: pad the uploaded copy with empty slices so that the first
        # imaged slice and the slice count are multiples of that (stacked fans only see their own slices, the in-plane
        # geometry does not change).
        align = 16 if (self.use_packed or self.grouped_packed) else 4
        if row_parallel and kernel != 2 and (nz % align or z_first % align):
            lead = (-z_first) % align
            tail = (-(nz + lead)) % align
            vol_raw = torch.nn.functional.pad(vol_raw, (0, 0, 0, 0, lead, tail))      # empty slices (id 0)
            z_first, nz = z_first + lead, nz + lead + tail
        # ---- 4. geometry and ray plans
        self.geom = _native.FanGeom(ct.N_proj, ct.N_channels, ct.N_rows, z_first, phantom.Nx, phantom.Ny,
                                    nz, 0, phantom.dx, phantom.dy, phantom.dz, ct.SID, ct.SDD)
        self.view_cs = to_dev(ct.view_cs(), torch.float64, self.dev)
        self.chan_cs = to_dev(ct.chan_cs(), torch.float64, self.dev)
        self.plan = torch.empty(self.n_local_views * ct.N_channels * _native.PLAN_BYTES, dtype=torch.uint8, device=self.dev)
        _native.check(self.lib.dexct_fan_plan(C.byref(self.geom), ptr(self.view_cs), ptr(self.chan_cs),
                                              self.view_begin, self.view_end, ptr(self.plan), st), 'dexct_fan_plan')
        # ---- 5. the volume layouts: y-x and x-y for the ray-parallel kernels, z fastest (and its 2-bit packing) for the
        # row-parallel ones, the cone beam's own
        self.vol_yx = vol_raw.contiguous()
        self.vol_xy = torch.empty_like(self.vol_yx)
        self.vol_zc = None
        self.cone_groups = False
        if self.cone:
            # cone beam: kernel 1 = one thread per ray (dexct_cone_project, any number of materials), 2 = the rows of a
            # (view, channel) pair as lanes (dexct_cone_project_rows for <= 3 materials; round 6: one pass per group of three
            # materials + one detection pass beyond that, dexct_cone_project_grouped); 0 picks 2 from 32 rows on
            self.cone_rows = kernel == 2 or (kernel == 0 and ct.N_rows >= 32)
            self.cone_groups = self.cone_rows and M > 3
            kernel = self.kernel = 1
            self.row_z = to_dev(ct.row_z(), torch.float64, self.dev)
            if self.cone_rows:
                self._cone_layout(nz, st)
        self.vol_zf = torch.empty_like(self.vol_yx) if row_parallel else None
        _native.check(self.lib.dexct_volume_layouts(ptr(self.vol_yx), phantom.Nx, phantom.Ny, nz,
                                                    ptr(self.vol_xy), ptr(self.vol_zf), st), 'dexct_volume_layouts')
        self.vol_z2, self.col_air, self.n_air_columns = None, None, 0
        self.col_class, self.n_uniform_columns = None, [0, 0, 0, 0]
        self.tile_map, self.n_uniform_tiles = None, [0, 0, 0, 0]
        if self.use_packed:
            self.vol_z2 = torch.empty(self.vol_zf.numel() // 4, dtype=torch.uint8, device=self.dev)
            _native.check(self.lib.dexct_volume_pack2(ptr(self.vol_zf), self.vol_zf.numel(), ptr(self.vol_z2), st),
                          'dexct_volume_pack2')
            # its air-column map (one bit per (x, y) column that is air over all z) and the number of such columns: the
            # packed kernel enters no slab that lies in them; the library decides per call whether looking them up pays
            self.col_air = torch.empty((phantom.Nx * phantom.Ny + 31) // 32, dtype=torch.int32, device=self.dev)
            n_air = torch.empty(1, dtype=torch.int64, device=self.dev)
            _native.check(self.lib.dexct_volume_air_columns(ptr(self.vol_z2), phantom.Nx, phantom.Ny, nz, ptr(self.col_air),
                                                            ptr(n_air), st), 'dexct_volume_air_columns')
            self.n_air_columns = int(n_air.item())
            # its column-class map (four bits per column: mixed, or one id over all z) and the uniform columns per id: the
            # noise-free packed kernel counts the slabs in uniform columns once per (view, channel) pair instead of per row
            self.col_class = torch.empty((phantom.Nx * phantom.Ny + 7) // 8, dtype=torch.int32, device=self.dev)
            n_uniform = torch.empty(4, dtype=torch.int64, device=self.dev)
            _native.check(self.lib.dexct_volume_column_classes(ptr(self.vol_z2), phantom.Nx, phantom.Ny, nz, ptr(self.col_class),
                                                               ptr(n_uniform), st), 'dexct_volume_column_classes')
            self.n_uniform_columns = [int(k) for k in n_uniform.tolist()]
            # the tile map of that class map (four bits per 8 x 8 columns) and the uniform tiles per id: the kernel dismisses
            # the runs of slabs that stay inside uniform tiles before it classifies slabs one by one
            self.tile_map = torch.empty(self.lib.dexct_volume_tile_map_words(phantom.Nx, phantom.Ny), dtype=torch.int32, device=self.dev)
            _native.check(self.lib.dexct_volume_tile_classes(ptr(self.col_class), phantom.Nx, phantom.Ny, ptr(self.tile_map),
                                                             ptr(n_uniform), st), 'dexct_volume_tile_classes')
            self.n_uniform_tiles = [int(k) for k in n_uniform.tolist()]
        # ---- 6. group codes of the material-group passes
        aligned = nz % 4 == 0 and z_first % 4 == 0
        self.grouped = not self.grouped_packed and (kernel == 4 or (kernel == 0 and row_parallel and M > 4 and aligned))
        if self.grouped and not (2 <= M <= 256 and aligned):
            raise ValueError('kernel 4 needs 2..256 materials')
        self.codes = None
        if self.grouped_packed or self.grouped:
            n_groups = (M - 1 + 2) // 3
            shape, fn = (((self.vol_zf.numel() // 4,), 'dexct_volume_groups_pack2') if self.grouped_packed
                         else (tuple(self.vol_zf.shape), 'dexct_volume_groups'))
            self.codes = torch.empty((n_groups,) + shape, dtype=torch.uint8, device=self.dev)
            _native.check(getattr(self.lib, fn)(ptr(self.vol_zf), self.vol_zf.numel(), M, ptr(self.codes), st), fn)
        # the material-group passes of either geometry: they go through in view chunks (_in_view_chunks)
        self._groups = self.cone_groups or self.grouped or self.grouped_packed

    def _upload_compact_ids(self, volume, st):
        """The volume on the device, renumbered to the table rows the kernels need; sets mat_rows, id_lut and n_mat."""
        # A uint8 label map may use any of 256 ids (XCAT: input/params.txt:8-9, plots.py:124) of which many share a
        # composition and some do not occur in the slices scanned: count the ids on the device, merge ids with the same
        # (density, composition) - their rows of density x mixatten(E) are equal at every energy - drop the absent ones, and
        # renumber the uploaded copy.  Row 0 stays id 0 (its path length comes from the chord).  mat_rows[k] = the phantom id
        # whose table row serves compact id k.
        vol_raw = to_dev(volume, torch.uint8, self.dev)
        cnt = torch.empty(256, dtype=torch.int64, device=self.dev)
        _native.check(self.lib.dexct_volume_ids(ptr(vol_raw), vol_raw.numel(), ptr(cnt), st), 'dexct_volume_ids')
        present = cnt.cpu().numpy() > 0
        if present[self.phantom.n_materials:].any():
            raise ValueError('the volume holds a material id without a table entry')
        self.mat_rows, lut = compact_ids(present, self.phantom.materials)
        if any(lut[i] != i for i in np.flatnonzero(present)):
            _native.check(self.lib.dexct_volume_remap(ptr(vol_raw), vol_raw.numel(), lut.ctypes.data_as(C.POINTER(C.c_uint8)), st),
                          'dexct_volume_remap')
        self.id_lut, self.n_mat = lut, len(self.mat_rows)
        return vol_raw

    def _cone_layout(self, nz, st):
        """vol_zc: what the cone beam's row kernels read - one layout, or one per group of three materials."""
        ph, M = self.phantom, self.n_mat
        nb = self.lib.dexct_cone_layout_bytes(ph.Nx, ph.Ny, nz)
        if self.cone_groups:
            self.vol_zc = torch.empty(((M + 2) // 3) * nb, dtype=torch.uint8, device=self.dev)
            _native.check(self.lib.dexct_cone_layout_groups(ptr(self.vol_yx), ph.Nx, ph.Ny, nz, M, ptr(self.vol_zc), st),
                          'dexct_cone_layout_groups')
        else:
            self.vol_zc = torch.empty(nb, dtype=torch.uint8, device=self.dev)
            _native.check(self.lib.dexct_cone_layout(ptr(self.vol_yx), ph.Nx, ph.Ny, nz, ptr(self.vol_zc), st),
                          'dexct_cone_layout')

    @property
    def n_local_views(self):
        return self.view_end - self.view_begin

    def compact(self, mu):
        """The table rows of the compact ids the kernels see (one row per distinct composition that occurs in the scanned
        slices) out of a table with one row per phantom id."""
        return mu[self.mat_rows]

    def path_bounds(self):
        """(l_max [n_mat], c_max) in cm: no ray of this scan crosses more than l_max[k] of compact id k - the diagonal of the
        bounding box of its voxels (in the slice plane for a stacked fan, whose rays stay in their slice; in space for a cone
        beam); the grid's own diagonal for id 0 - nor more than c_max in total.  Computed once, on the device, from the
        uploaded volume (the domain quadrature.reduce_tables guarantees its error bound on)."""
        if self._bounds is None:
            ph = self.phantom
            v = self.vol_yx.view(-1, ph.Ny, ph.Nx)
            d = (ph.dz, ph.dy, ph.dx)
            axes = (0, 1, 2) if self.cone else (1, 2)
            c_max = float(np.sqrt(sum((v.shape[a] * d[a]) ** 2 for a in axes)))
            l_max = [c_max]
            for k in range(1, self.n_mat):
                m = v == k
                ext2 = 0.0
                for a in axes:
                    idx = torch.nonzero(m.any(dim=[b for b in (0, 1, 2) if b != a])).flatten()
                    if idx.numel():
                        ext2 += (float(idx[-1] - idx[0] + 1) * d[a]) ** 2
                l_max.append(min(c_max, float(np.sqrt(ext2))))
            self._bounds = (l_max, c_max)
        return self._bounds

    def upload_tables(self, specs, quadrature=None, noise=False):
        """E, mu [n_mat, nE] and w [S, nE] on the device (float32) and the S unattenuated signals.  ``quadrature='reduced'``
        (or DEXCT_QUADRATURE=reduced) swaps the energy grid for the shorter one of quadrature.reduce_tables where it applies
        (<= 4 table rows, bound verified); ``self.quadrature_info`` then says what was used (None: the full grid).
        ``noise`` (as Projector.project takes it) appends the [S, nE] device table of its noise model - True / 'gaussian': the
        variance weights (project_tables' ``w2_d``); 'poisson': the photons per bin, w / (signal per photon) - and keeps the full
        grid, whose bins the variance and the photon counts are defined on (``quadrature`` plays no part)."""
        dev32 = lambda x: to_dev(x, torch.float32, self.dev)
        E, mu, w, w2 = merged_tables(self.ct, self.phantom, specs, with_variance=True)
        mu_c, air = self.compact(mu), w.sum(axis=1)
        if noise:
            extra = w / (E if self.ct.eid else np.ones_like(E)) if noise == 'poisson' else w2
            return E, dev32(mu_c), dev32(w), air, dev32(extra)
        self.quadrature_info = None
        if _want_reduced(quadrature):
            from . import quadrature as _q
            red = _q.reduce_tables(mu_c, w, *self.path_bounds()) if self.n_mat <= _q.MAX_MATERIALS else None
            if red is not None:
                cols, w, self.quadrature_info = red
                E, mu_c = E[cols], mu_c[:, cols]
        return E, dev32(mu_c), dev32(w), air

    def project_tables(self, mu_d, w_d, want_pathlen=False, out=None, layout=0, w2_d=None, seed=0, air=None,
                       log_out=None, views=None, want_variance=False):
        """Device-side call: mu_d [M, nE], w_d [S, nE] float32 tensors -> counts.

        ``air`` (S unattenuated signals, sum_e w[s][e]) asks for get_sino's second output as well, the log sinogram
        ln(air / counts) (main.py:120-122), written by the projection kernel's own detection store (dexct_log_out) into
        ``log_out`` or a new tensor of the counts' shape; the call then returns (counts[, pathlen], log).

        layout 0: counts [S, nV, rows, channels] (the reference's order); layout 1: [S, nV, channels, rows]
        (what the row-parallel kernels produce natively); ``layout=None`` returns the native one.  When
        the requested layout is not the kernel's own, the kernel writes its own layout and
        dexct_transpose_batched converts (cheaper than scattered 4-byte stores).
        ``w2_d`` (variance weights, merged_tables(with_variance=True)) switches quantum noise on (Philox, keyed by ``seed``
        and by the GLOBAL (view, row, channel), so shards reproduce the unsharded sinogram).  The default kernels - the
        packed stacked fan (<= 2 spectra) and the cone beam - sum the variance in the detection's own energy loop and draw
        the sample in registers (struct dexct_noise): no variance array, no extra pass, and the log sinogram comes from the
        same store.  The other kernels write the variance and dexct_add_noise draws the same sample from it.
        ``want_variance``: the variance of the detected signal as a further result (appended last; tests).
        ``views=(a, b)``: only the local views [a, b) of this projector's range (outputs sized for b - a views): a step that
        hands its sinogram on in chunks projects chunk by chunk (bench.py, the sharded step).
        Tensor contract: the tables in any layout on the projector's device (made dense float32); ``out`` and
        ``log_out`` dense float32 device tensors of the layout's element count, else ValueError."""
        # ---- 1. the tables and the view range
        mu_d, w_d, w2_d, sl0, sl1 = self._check_tables(mu_d, w_d, w2_d, views)
        S, nE = w_d.shape
        M, nV, nR, nC = self.n_mat, sl1 - sl0, self.ct.N_rows, self.ct.N_channels
        # ---- 2. outputs and layouts: the kernel writes ``run_layout``; where that is not the layout wanted, a transpose follows
        new = lambda shape: torch.empty(shape, dtype=torch.float32, device=self.dev)
        native = self.native_layout
        want = native if layout is None else layout
        shape = {0: (S, nV, nR, nC), 1: (S, nV, nC, nR)}
        direct = want == native or nR == 1
        run_layout = want if direct else native
        # written tensors are never normalised (_device.written): right device, float32, dense and of the layout's size, or refused
        for name, t in (('out', out), ('log_out', log_out)):
            if t is not None:
                written(t, name, self.dev, torch.float32, S * nV * nR * nC)
        # the log sinogram: written by the detection store when the kernel's layout is the one wanted; else together with the
        # transpose at the end (dexct_transpose_log: the counts are read once for both outputs)
        fuse_log = air is not None and not direct
        counts = out if (out is not None and direct) else new(shape[run_layout])
        pathlen = new((nV, nR, nC, M) if run_layout == 0 else (nV, nC, nR, M)) if want_pathlen else None
        # ---- 3. who draws the noise: the kernel in its detection, or dexct_add_noise from the variance the kernel writes
        noisy = w2_d is not None
        in_kernel = noisy and self._samples_in_kernel(S)
        variance = torch.empty_like(counts) if (noisy and (want_variance or not in_kernel)) else None
        log = None
        if air is not None and not fuse_log:
            log = log_out if log_out is not None else new(shape[run_layout])
        # ---- 4. the launch.  The log is fused into the detection store, except where the noisy counts only exist after
        # dexct_add_noise
        call = _Call(plan_ptr=self.plan.data_ptr() + sl0 * nC * _native.PLAN_BYTES, vb=self.view_begin + sl0, S=S, nE=nE,
                     mu=ptr(mu_d), w=ptr(w_d), w2=ptr(w2_d), air=air, nz=_native.noise(seed) if in_kernel else None,
                     run_layout=run_layout, packed=self.use_packed and (not noisy or in_kernel))
        self._launch(call, counts, pathlen, variance, log if (not noisy or in_kernel) else None)
        # ---- 5. the post passes
        if noisy and not in_kernel:
            _native.check(self.lib.dexct_add_noise(ptr(counts), ptr(variance), S, nV, nR, nC, run_layout,
                                                   call.vb, int(seed) & (2 ** 64 - 1), stream_ptr()),
                          'dexct_add_noise')
            if log is not None:
                self.sino_log(counts, air, log)
        if not direct:
            dst = out if out is not None else new(shape[want])
            r, c = (nC, nR) if run_layout == 1 else (nR, nC)
            if fuse_log:
                log = log_out if log_out is not None else new(shape[want])
            self.transpose_log(counts, dst, log, air, r, c)
            counts = dst
            if pathlen is not None:
                pathlen = pathlen.permute(0, 2, 1, 3).contiguous()      # test-only output
            if variance is not None and want_variance:
                variance = variance.permute(0, 1, 3, 2).contiguous()    # test-only output
        res = (counts, pathlen) if want_pathlen else (counts,)
        if log is not None:
            res = res + (log,)
        if want_variance:
            res = res + (variance,)
        return res if len(res) > 1 else res[0]

    def _check_tables(self, mu_d, w_d, w2_d, views):
        """project_tables' tables as the kernels read them, mu with the rows of the compact ids, and the local view range."""
        # the kernels read the tables through raw pointers: dense float32 on the projector's device, whatever view the caller
        # built (torch.tensor(w[:, keep]) keeps NumPy's column-major result of the advanced index); a host tensor is refused
        f32 = dict(keep=(torch.float32,), cast=torch.float32)
        mu_d, w_d = dense_input(mu_d, 'mu_d', self.dev, **f32), dense_input(w_d, 'w_d', self.dev, **f32)
        w2_d = None if w2_d is None else dense_input(w2_d, 'w2_d', self.dev, **f32)
        if mu_d.dim() != 2 or w_d.dim() != 2:
            raise ValueError(f'tables must be [rows, nE]: mu {tuple(mu_d.shape)}, w {tuple(w_d.shape)}')
        S, nE = w_d.shape
        if mu_d.shape[1] != nE or (w2_d is not None and tuple(w2_d.shape) != (S, nE)):
            raise ValueError(f'tables disagree: mu {tuple(mu_d.shape)}, w {tuple(w_d.shape)}' + ('' if w2_d is None else f', w2 {tuple(w2_d.shape)}'))
        sl0, sl1 = (0, self.n_local_views) if views is None else (int(views[0]), int(views[1]))
        if not 0 <= sl0 < sl1 <= self.n_local_views:
            raise ValueError(f'views={views}: a non-empty range within the {self.n_local_views} local views')
        if mu_d.shape[0] != self.n_mat:
            if mu_d.shape[0] != self.phantom.n_materials:
                raise ValueError(f'mu has {mu_d.shape[0]} rows; expected {self.n_mat} (compact ids, Projector.compact) or '
                                 f'{self.phantom.n_materials} (one per phantom id)')
            mu_d = mu_d[torch.as_tensor(self.mat_rows, device=mu_d.device)].contiguous()
        return mu_d, w_d, w2_d, sl0, sl1

    def _samples_in_kernel(self, S):
        """Whether the kernel that will run draws the noise sample of ``S`` spectra itself (ABI 6: struct dexct_noise), in its
        detection; otherwise it writes the variance and dexct_add_noise draws the same sample from it.  The host-side mirror
        of proj::noise_log_args (csrc/proj_host.h), which refuses a sample where this says no: the detection pass of the
        material groups and the packed stacked fan hold two spectra, the group pass up to _NOISE_MAX_GROUP_ROWS table rows;
        the cone beam without groups always samples; the byte-volume stacked fan never does."""
        if self._groups:
            return S <= _NOISE_MAX_SPECTRA and self.n_mat <= _NOISE_MAX_GROUP_ROWS
        return self.cone or (self.use_packed and S <= _NOISE_MAX_SPECTRA)

    def _launch(self, c, counts, pathlen, variance, log):
        """The projection launch of one project_tables call ``c`` (_Call) on the route __init__ settled: one library call, or
        one per view chunk for the material groups.  ``log``: where the detection store writes the log sinogram (None: it
        writes none)."""
        if self._groups:
            # one traversal per group of three materials into M planes of path lengths (the scratch), one detection pass
            # over them
            n_chunk, scratch = self._group_scratch(counts.shape[1])
            return _in_view_chunks(lambda *chunk: self._launch_groups(c, scratch, *chunk), n_chunk, counts, pathlen, variance, log)
        lib, geom, M, ve = self.lib, C.byref(self.geom), self.n_mat, c.vb + counts.shape[1]
        lo = _native.log_out(ptr(log), c.air)
        if self.cone and self.cone_rows:
            # (quantum noise: the variance of the detected signal comes out of the same launch and the kernel draws the sample)
            _native.check(lib.dexct_cone_project_rows(
                geom, c.plan_ptr, *self._cone_rays(), c.vb, ve, ptr(self.vol_zc), M, c.nE, c.S, c.mu, c.w, ptr(counts),
                ptr(pathlen), lo, c.w2, ptr(variance), c.nz, stream_ptr()), 'dexct_cone_project_rows')
        elif self.cone:
            _native.check(lib.dexct_cone_project(
                geom, c.plan_ptr, *self._cone_rays(), c.vb, ve, ptr(self.vol_yx), ptr(self.vol_xy), M, c.nE, c.S, c.mu, c.w,
                ptr(counts), ptr(pathlen), lo, c.w2, ptr(variance), c.nz, stream_ptr()), 'dexct_cone_project')
        elif c.packed:                                          # (noise on > 2 spectra: the byte-volume kernel below)
            _native.check(lib.dexct_siddon_project_packed_tiles(
                geom, c.plan_ptr, c.vb, ve, ptr(self.vol_z2), M, c.nE, c.S, c.mu, c.w, ptr(counts), ptr(pathlen), c.run_layout, lo,
                c.w2, ptr(variance), c.nz, ptr(self.col_air), self.n_air_columns, ptr(self.col_class),
                (C.c_int64 * 4)(*self.n_uniform_columns), ptr(self.tile_map), (C.c_int64 * 4)(*self.n_uniform_tiles),
                stream_ptr()), 'dexct_siddon_project_packed_tiles')
        else:
            _native.check(lib.dexct_siddon_project(
                geom, c.plan_ptr, c.vb, ve, ptr(self.vol_yx), ptr(self.vol_xy), ptr(self.vol_zf), M, c.nE, c.S, c.mu, c.w,
                ptr(counts), ptr(pathlen), 3 if self.kernel in (7, 8) else self.kernel, c.run_layout, c.w2, ptr(variance), lo,
                stream_ptr()), 'dexct_siddon_project')

    def _cone_rays(self):
        """What every cone entry point takes after the plan: the view and channel directions, the rows' heights, the
        source's height and the largest |row height - source height|."""
        max_dz = float(np.max(np.abs(self.ct.row_z() - self.ct.src_z)))
        return ptr(self.view_cs), ptr(self.chan_cs), ptr(self.row_z), self.ct.src_z, max_dz

    def _group_scratch(self, nV):
        """The per-material accumulators of the group passes: M x rays floats.  Many materials on a large scan go through in
        view chunks so that this scratch stays below _GROUP_SCRATCH_BYTES.  Returns (views per chunk, scratch)."""
        rays = self.ct.N_rows * self.ct.N_channels
        n_chunk = max(1, min(nV, _GROUP_SCRATCH_BYTES // (self.n_mat * rays * 4)))
        return n_chunk, torch.empty((self.n_mat, n_chunk * rays), dtype=torch.float32, device=self.dev)

    def _launch_groups(self, c, scratch, v0, v1, counts, pathlen, variance, log):
        """The material-group passes over the views [v0, v1) of call ``c`` into outputs of that many views.  (The cone and the
        fan entry points order scratch / run_layout / log_out / weights2 / variance / noise differently.)"""
        geom, M, lo = C.byref(self.geom), self.n_mat, _native.log_out(ptr(log), c.air)
        plan_ptr = c.plan_ptr + v0 * self.ct.N_channels * _native.PLAN_BYTES
        if self.cone:
            _native.check(self.lib.dexct_cone_project_grouped(
                geom, plan_ptr, *self._cone_rays(), c.vb + v0, c.vb + v1, ptr(self.vol_zc), M, c.nE, c.S, c.mu, c.w, ptr(counts),
                ptr(pathlen), ptr(scratch), lo, c.w2, ptr(variance), c.nz, stream_ptr()), 'dexct_cone_project_grouped')
        else:
            what = 'dexct_siddon_project_grouped_packed' if self.grouped_packed else 'dexct_siddon_project_grouped'
            _native.check(getattr(self.lib, what)(
                geom, plan_ptr, c.vb + v0, c.vb + v1, ptr(self.codes), M, c.nE, c.S, c.mu, c.w, ptr(counts), ptr(pathlen),
                ptr(scratch), c.run_layout, c.w2, ptr(variance), lo, c.nz, stream_ptr()), what)

    @staticmethod
    def _air_array(air, S):
        """The S unattenuated signals as the float array the log passes take."""
        return (C.c_float * S)(*[float(x) for x in air[:S]])

    def transpose_log(self, src, dst, log_dst, air, rows, cols):
        """src [S, n, rows, cols] -> dst [S, n, cols, rows] and (``log_dst`` not None) ln(air[s] / dst[s]) in the same pass
        (dexct_transpose_log).  ``src`` in any layout; ``dst`` and ``log_dst`` dense float32 of src's element count, else ValueError."""
        src = dense_input(src, 'src', self.dev, keep=(torch.float32,), cast=torch.float32)
        if src.dim() != 4 or tuple(src.shape[2:]) != (int(rows), int(cols)):
            raise ValueError(f'src must be [S, n, {rows}, {cols}], got {tuple(src.shape)}')
        S, n = int(src.shape[0]), int(src.shape[1])
        written(dst, 'dst', self.dev, torch.float32, src.numel())
        if log_dst is not None:
            written(log_dst, 'log_dst', self.dev, torch.float32, src.numel())
        arr = self._air_array(air, S) if log_dst is not None else None
        _native.check(self.lib.dexct_transpose_log(ptr(src), ptr(dst), ptr(log_dst), arr, S, n, rows, cols, stream_ptr()),
                      'dexct_transpose_log')

    def sino_log(self, counts, air, out=None):
        """ln(air[s] / counts[s]) as a pass of its own (dexct_sino_log): noisy and gathered sinograms.  ``counts`` in any layout;
        ``out`` a dense float32 device tensor of its element count, else ValueError."""
        counts = dense_input(counts, 'counts', self.dev, keep=(torch.float32,), cast=torch.float32)
        S = counts.shape[0]
        out = torch.empty_like(counts) if out is None else written(out, 'out', self.dev, torch.float32, counts.numel())
        _native.check(self.lib.dexct_sino_log(ptr(counts), self._air_array(air, S), S, counts[0].numel(), ptr(out), stream_ptr()),
                      'dexct_sino_log')
        return out

    def project(self, specs, want_pathlen=False, layout=0, noise=False, seed=0, want_log=False, quadrature=None):
        """noise: False (expectation), True / 'gaussian' (compound-Poisson variance, normal sample) or 'poisson'
        (per-energy-bin Poisson photon counts: exact for photon-starved rays, ~5x the projection time).
        ``want_log``: also the log sinogram ln(air / counts), from the device (appended to the projection's result).
        ``quadrature``: see upload_tables (noise-free projections only: the noisy ones keep the full grid, whose bins the
        variance and the photon counts are defined on)."""
        if not noise:
            _, mu_d, w_d, air = self.upload_tables(specs, quadrature)
            return self.project_tables(mu_d, w_d, want_pathlen, layout=layout, air=air if want_log else None), air
        if noise == 'poisson':
            res, air = self._project_poisson(specs, want_pathlen, layout, seed)
            if want_log:
                res = (res if isinstance(res, tuple) else (res,))
                res = res + (self.sino_log(res[0], air),)
            return res, air
        _, mu_d, w_d, air, w2_d = self.upload_tables(specs, noise=True)
        return self.project_tables(mu_d, w_d, want_pathlen, layout=layout, w2_d=w2_d, seed=seed,
                                   air=air if want_log else None), air

    def _project_poisson(self, specs, want_pathlen, layout, seed):
        E, mu_d, w_d, air, ph_d = self.upload_tables(specs, noise='poisson')
        gain_d = to_dev(E if self.ct.eid else np.ones_like(E), torch.float32, self.dev)
        # path lengths from whichever traversal kernel applies (its noise-free counts are discarded)
        want = self.native_layout if layout is None else layout
        counts, pathlen = self.project_tables(mu_d, w_d, want_pathlen=True, layout=want)
        S, nE = w_d.shape
        nV, nR, nC = self.n_local_views, self.ct.N_rows, self.ct.N_channels
        _native.check(self.lib.dexct_poisson_detect(
            ptr(pathlen), ptr(mu_d), ptr(ph_d), ptr(gain_d), mu_d.shape[0], nE, S, nV, nR, nC, want, self.view_begin,
            int(seed) & (2 ** 64 - 1), ptr(counts), stream_ptr()), 'dexct_poisson_detect')
        return ((counts, pathlen) if want_pathlen else counts), air

    def trace(self, rays_vrc, max_seg=None):
        """Voxel-index sequence and float32 piece lengths of selected rays (views relative to the shard)."""
        rays = to_dev(np.asarray(rays_vrc, dtype=np.int32).reshape(-1, 3), torch.int32, self.dev)
        n = rays.shape[0]
        max_seg = max_seg or 2 * max(self.phantom.Nx, self.phantom.Ny) + 4
        vox = torch.zeros((n, max_seg), dtype=torch.int32, device=self.dev)
        ln = torch.zeros((n, max_seg), dtype=torch.float32, device=self.dev)
        ns = torch.zeros(n, dtype=torch.int32, device=self.dev)
        _native.check(self.lib.dexct_siddon_trace(C.byref(self.geom), ptr(self.plan), ptr(rays), n, max_seg,
                                                  ptr(vox), ptr(ln), ptr(ns), stream_ptr()), 'dexct_siddon_trace')
        return vox.cpu().numpy(), ln.cpu().numpy(), ns.cpu().numpy()

    def plan_host(self):
        """The plan table as a NumPy structured array (for parity tests)."""
        dt = np.dtype([('V0', '<i8'), ('SV', '<i8'), ('i_first', '<i4'), ('n_slabs', '<i4'), ('kf', '<f4'),
                       ('len_per_u', '<f4'), ('chord_u', '<f4'), ('flags', '<u4')])
        return self.plan.cpu().numpy().view(dt)


def _want_reduced(quadrature):
    """None: what DEXCT_QUADRATURE says (default 'full')."""
    q = quadrature if quadrature is not None else _os.environ.get('DEXCT_QUADRATURE', 'full')
    if q not in ('full', 'reduced'):
        raise ValueError(f"quadrature must be 'full' or 'reduced', not {q!r}")
    return q == 'reduced'


# scratch of the material-group passes above which a projection goes through in view chunks (DEXCT_GROUP_SCRATCH_GB)
_GROUP_SCRATCH_BYTES = int(float(_os.environ.get('DEXCT_GROUP_SCRATCH_GB', '16')) * 2 ** 30)

_cache = {}

# True (the default): every get_sino call checksums the WHOLE volume (xxh3, 64 bits; 15 ms per 128 MiB) and compares it with
# the checksum of the bytes the device-resident state was built from - the reference rebuilds its state on every call, so
# an in-place edit of ``phantom.volume`` must never return a stale sinogram.  The checksum is computed by the calling thread
# AFTER it has queued the projection kernel and the device-to-host copies and BEFORE it waits for them (everything it queued
# is asynchronous), so it costs the call no time as long as hashing is faster than the GPU work (512^3: 15 against 75 ms;
# one 512^2 slice: 0.03 against 0.5 ms); on a mismatch the state is rebuilt and the projection redone.
# False / DEXCT_VERIFY_VOLUME=0 opts out: the O(1) key below alone (version counter + a strided sample).
verify_volume = True


def _verify_enabled():
    return verify_volume and _os.environ.get('DEXCT_VERIFY_VOLUME', '1') != '0'


def _hash64(a):
    """64-bit hash of an array's bytes: xxh3 where the xxhash module is present, else blake2b."""
    a = np.ascontiguousarray(a)
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(a.data)
    except ImportError:
        import hashlib
        return int.from_bytes(hashlib.blake2b(a.data, digest_size=8).digest(), 'little')


def _sample_step(shape, n_samples=4096):
    """Stride of the O(1) sample: about size / n_samples and coprime to every dimension, so that the samples spread over
    all rows, columns and slices (a stride that is a multiple of Nx - what size / 4096 is for every power-of-two volume -
    only ever visits the x = 0 face, which is air for any centred phantom)."""
    from math import gcd
    size = int(np.prod(shape))
    step = max(1, -(-size // n_samples)) | 1
    while any(d > 1 and gcd(step, int(d)) != 1 for d in shape):
        step += 2
    return step


def _volume_key(phantom):
    """What identifies the bytes of ``phantom.volume`` without reading them all: the phantom's version counter (bumped
    whenever ``volume`` is assigned and by ``phantom.touch()``), the identity and shape of the array, and a hash of ~4096
    voxels at a stride coprime to the dimensions.  This key only decides whether the cached state is a CANDIDATE; whether
    its bytes are still the volume's is settled by the whole-volume checksum (``verify_volume``, on by default)."""
    v = phantom.volume
    flat = v.reshape(-1)
    return (getattr(phantom, 'version', 0), id(v), v.shape, _hash64(flat[::_sample_step(v.shape)]))


def _fingerprint(ct, phantom, view_range):
    """Everything the device-resident state (volume layouts, ray plans) depends on.  The reference rebuilds its
    state on every get_sino call; here the state is reused only while the scanner numbers, the voxel sizes and
    the volume (see _volume_key and verify_volume) are what they were when it was built."""
    return (id(ct), id(phantom), view_range, ct.N_proj, ct.N_channels, ct.N_rows, ct.SID, ct.SDD,
            _hash64(ct.thetas), _hash64(ct.gammas),
            ct.h_iso, bool(getattr(ct, 'cone', False)), float(getattr(ct, 'src_z', 0.0)),
            phantom.z_index, phantom.Nx, phantom.Ny, phantom.Nz, phantom.dx, phantom.dy, phantom.dz,
            tuple((float(m.density), str(m.matcomp)) for m in phantom.materials)) + _volume_key(phantom)


def invalidate():
    """Drop the cached device state (the next get_sino call rebuilds it)."""
    _cache.clear()


def _projector(ct, phantom, view_range):
    """The device-resident state for this (scanner, phantom, shard), and whether the caller has to verify it: True when
    it was found in the cache and verification is on - the caller then compares ``_hash64(phantom.volume)`` with
    ``pj.volume_hash`` before it hands results out (False for a state built just now: its checksum is of the bytes it was
    built from)."""
    key = _fingerprint(ct, phantom, view_range)
    pj = _cache.get(key)
    if pj is None or pj.ct is not ct or pj.phantom is not phantom:
        _cache.clear()                      # keep one (scanner, phantom) pair resident
        pj = _cache[key] = Projector(ct, phantom, view_range)
        pj.volume_hash = _hash64(phantom.volume) if _verify_enabled() else None      # (the layouts are still being written)
        return pj, False
    return pj, bool(_verify_enabled() and pj.volume_hash is not None)


def _stale(pj, check, phantom):
    """Whether ``phantom.volume`` is no longer the bytes the cached state ``pj`` was built from (``check``: _projector asks
    for the comparison).  Called between queueing the GPU work and waiting for it: the checksum costs the call no time."""
    return check and _hash64(phantom.volume) != pj.volume_hash


def _checked(out, stale, ct, phantom, specs, noise, seed, quadrature):
    """The tail of get_sinos: ``out``, the per-spectrum (raw, log) pairs [N_proj, N_rows, N_channels] that the caller holds
    through this list alone, with the single row squeezed - or, if they are ``stale``, the projection done again."""
    if stale:
        # phantom.volume was edited in place since the device state was built (no touch()): what was just computed is of
        # the old bytes.  Release it, rebuild from the current bytes and project again - the result is what the reference,
        # which builds its state on every call, returns.  (Under torch.distributed every rank holds the same phantom and
        # takes the same branch.)
        out.clear()
        invalidate()
        return get_sinos(ct, phantom, specs, noise=noise, seed=seed, quadrature=quadrature)
    if ct.N_rows == 1:
        return [(r[:, 0, :], l[:, 0, :]) for r, l in out]
    return out


_SINO_CHUNKS = 8                # view chunks of a large noise-free projection on one process: chunk k + 1 is projected while chunk k
                                # crosses PCIe (3.3 GB of results take 58 ms, their kernels 12)


def _get_sinos_pipelined(pj, check, ct, phantom, specs, seed, quadrature, noise=False):
    """get_sinos for a large scan on one process: the views are projected in _SINO_CHUNKS chunks (Projector.project_tables,
    views=) and every chunk's two outputs leave for host memory on a download stream while the next chunk is projected.  The same
    kernels on the same rays as the single launch: the same bits - with quantum noise too (``noise`` True: the Philox counter is
    the global view).  One host block per spectrum and output (_device.LazyPinnedResult: touched and locked chunk by chunk in
    front of the copies, unlocked before it is returned)."""
    _, mu_d, w_d, air, w2_d = pj.upload_tables(specs, noise=True) if noise else pj.upload_tables(specs, quadrature) + (None,)
    S, nV, nR, nC = len(specs), pj.n_local_views, ct.N_rows, ct.N_channels
    bounds = [_shard.split(nV, k, _SINO_CHUNKS) for k in range(_SINO_CHUNKS)]
    row = nR * nC * 4
    cuts = [b * row for b, _ in bounds] + [nV * row]
    holders = [[LazyPinnedResult(pj.lib, (nV, nR, nC), np.float32, cuts, pj.dev.index or 0) for _ in range(2)] for _ in range(S)]
    main, _, down = side_streams(pj.dev)      # (kernels and downloads on queues of their own, _device.side_streams)
    main.wait_stream(torch.cuda.current_stream())
    keep = []                                  # (the chunks' device tensors live until their copies are done)
    with torch.cuda.stream(main):
        for k, (b, e) in enumerate(bounds):
            c_k, l_k = pj.project_tables(mu_d, w_d, layout=0, air=air, views=(b, e), w2_d=w2_d, seed=seed)
            keep.append((c_k, l_k))
            done = torch.cuda.Event()
            done.record(main)
            down.wait_event(done)
            for s_i in range(S):
                holders[s_i][0].download(k, c_k[s_i].data_ptr(), down)
                holders[s_i][1].download(k, l_k[s_i].data_ptr(), down)
    stale = _stale(pj, check, phantom)        # (computed while the GPU works, as in get_sinos)
    down.synchronize()
    out = [(h[0].finish(), h[1].finish()) for h in holders]
    del keep
    return _checked(out, stale, ct, phantom, specs, noise, seed, quadrature)


_DOWNLOAD_PIECE = 128 << 20     # bytes of a large result per copy (and per step of the page-locking in front of it)


def get_sinos(ct, phantom, specs, noise=False, seed=0, quadrature=None):
    """Several spectra from ONE traversal (path lengths are energy independent).

    ``noise=True`` adds quantum noise for the dose the spectra are scaled to (compound-Poisson variance,
    Gaussian sample; ``noise='poisson'`` draws per-energy-bin Poisson photon counts instead, exact for
    photon-starved rays), counter-based Philox RNG keyed by ``seed`` (csrc/noise.hip); the default is the
    noise-free expectation, which is what every parity test uses.

    Returns a list of (sino_raw, sino_log) float32 NumPy pairs, shaped [N_proj, N_channels]
    (or [N_proj, N_rows, N_channels] for N_rows > 1).  Both come from the device (the log sinogram is written by
    the projection kernel's detection store) through page-locked host memory: the arrays returned are views of a
    pinned buffer that belongs to them alone (torch's caching host allocator hands it out again once they are
    garbage).  ``quadrature='reduced'`` (opt-in; quadrature.py) evaluates the noise-free detection on a shorter energy grid
    whose relative error is verified <= 1e-6 over every path length the phantom allows.  Under torch.distributed the projection angles are sharded over the ranks and every rank returns the
    full gathered sinograms.
    """
    vb, ve = _shard.my_views(ct.N_proj)
    pj, check = _projector(ct, phantom, (vb, ve))
    sharded = _shard.world()[1] > 1
    per_array = ct.N_proj * ct.N_rows * ct.N_channels * 4
    if not sharded and noise != 'poisson' and pool_wanted(per_array) and ct.N_proj >= 4 * _SINO_CHUNKS:
        return _get_sinos_pipelined(pj, check, ct, phantom, specs, seed, quadrature, noise=bool(noise))
    res, air = pj.project(specs, noise=noise, seed=seed, want_log=not sharded, quadrature=quadrature)
    if sharded:
        counts = _shard.gather_views(res, ct.N_proj, view_dim=1, tag='get_sinos', mode=_shard.dropin_mode())
        log = pj.sino_log(counts, air)              # of the gathered sinogram: one collective instead of two
    else:
        counts, log = res
    # both results start towards page-locked host memory; the checksum of the volume is computed while the kernels and the
    # copies run; one wait for everything
    n_bytes = counts.numel() * 4
    if pool_wanted(n_bytes):
        # large results: blocks of the host pool - locked already, or (a process's first projections) locked piece by piece while
        # the copies of the pieces before run (_device.LazyPinnedResult) - instead of two page-locked allocations in front of them
        cuts = list(range(0, n_bytes, _DOWNLOAD_PIECE)) + [n_bytes]
        lz = [LazyPinnedResult(pj.lib, tuple(t.shape), np.float32, cuts, pj.dev.index or 0) for t in (counts, log)]
        cur = torch.cuda.current_stream()
        for k in range(len(cuts) - 1):
            for holder, t in zip(lz, (counts, log)):
                holder.download(k, t.data_ptr() + cuts[k], cur)
        stale = _stale(pj, check, phantom)
        cur.synchronize()
        raw, lg = lz[0].finish(), lz[1].finish()
        h_raw = h_lg = None
    else:
        h_raw, h_lg = pinned_empty(counts.shape, counts.dtype), pinned_empty(log.shape, log.dtype)
        h_raw.copy_(counts, non_blocking=True)
        h_lg.copy_(log, non_blocking=True)
        stale = _stale(pj, check, phantom)
        torch.cuda.current_stream().synchronize()
        raw, lg = h_raw.numpy(), h_lg.numpy()
    out = [(raw[k], lg[k]) for k in range(len(specs))]
    del raw, lg, h_raw, h_lg, counts, log, res          # (``out`` alone holds the results: _checked can release them)
    return _checked(out, stale, ct, phantom, specs, noise, seed, quadrature)


def get_sino(ct, phantom, spec, noise=False, seed=0, quadrature=None):
    """Drop-in for the reference call ``sino_raw, sino_log = get_sino(ct, phantom, spec)`` (main.py:120)."""
    return get_sinos(ct, phantom, [spec], noise=noise, seed=seed, quadrature=quadrature)[0]
