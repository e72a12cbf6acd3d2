"""Guard-banded bounds tests of the volume preparation, the plan and every projection entry point through the bare C ABI.

Method of tests/test_gpu_bounds.py (tests/guarded.py): every buffer of a launch sits between two 64 KiB guards and has EXACTLY
the size include/dexct.h promises, each case runs under a 0x00 and a 0xFF fill of the guards, the outputs and the scratch, and
must leave every guard unchanged, dexct_last_hip_error() == 0 and bit-identical outputs - a store past an output, a buffer
descriptor longer than its buffer, a read past an input or an output element never written would each show.  Nothing goes
through forward_project.Projector: volumes are not padded by a host, tensors have no neighbours from a caching allocator.

Byte extents given (n_rays = n_local_views n_rows n_channels, M materials, S spectra, n_e energies):
  plan 40 n_local_views n_channels; view_cs 16 geom.n_views; chan_cs 16 n_channels; row_z 8 n_rows
  vol (= vol_yx), vol_xy, vol_zf nx ny nz; vol_z2 nx ny nz / 4; codes ceil((M - 1) / 3) nx ny nz; codes2 a quarter of that
  vol_zc dexct_cone_layout_bytes(nx, ny, nz); vol_zcg ceil(M / 3) times that; counts256 2048
  mu 4 M n_e; weights, weights2 4 S n_e; counts, variance, sino_log 4 S n_rays; pathlen, acc_scratch 4 n_rays M
  trace: ray_vrc 12 n; seg_voxel, seg_len 4 n max_seg; n_seg 4 n
acc_scratch is scratch: filled, not compared.

Values: per-material path lengths array_equal to c_oracle.project_dda / project_cone(dda=True) on every ray; counts within
REL_TOL = 1e-5 (tests/test_gpu_siddon.py) of project_classic / project_cone(dda=False) except on rays that run exactly along
a grid plane (on_plane_rays; at most 2 % of a case's rays, asserted here and in tests/test_bounds_refs.py on the CPU); the
variance the same way with weights2 as weights; sino_log against np_log of the counts at the tolerance of
test_log_sinogram_from_the_detection_store; sampled counts bit-equal to the noise-free call + dexct_add_noise on its variance.
Layouts, codes, id counts: array_equal to the NumPy restatement of the header's definition; the plan field by field against
c_oracle.plan.

Kernel (__global__) -> test that launches it
  plan.hip       fan_plan_kernel                          test_fan_plan
                 volume_ids_kernel, volume_remap_kernel   test_volume_ids_and_remap (one size past each capped grid)
                 transpose_xy_kernel, transpose_z_kernel  test_volume_layouts (with / without vol_zf)
                 transpose_batched_kernel                 tests/test_gpu_bounds.py::test_transposes (not repeated)
  siddon.hip
                 group_codes_kernel                       test_volume_groups (4099 voxels, 3 groups: planes off a dword boundary)
                 rays_kernel<1..4, 64, 4> and <0> (LDS)    test_siddon_project[kernel 1], test_material_counts[project-1];
                                                          <.., 256>, <.., 64, 8>, <.., 64, 16>: test_switches (DEXCT_RAYS_BATCH)
                 rows_kernel<1..4> and <0>                test_siddon_project[kernel 2], test_material_counts[project-2]
                 rows4_kernel<NM, B, false>               test_siddon_project[kernel 3] (B = 64; 128 and 256 lanes: r257 / r1100 rows)
                 rows4_kernel<NM, B, true>                test_material_counts[grouped], test_grouped_options
                 rows4t_kernel<NM, 8, 64, false>          test_siddon_project[kernel 5]
                 rows4t_kernel<.., true>                  not instantiated: no entry point passes acc_out to kernel 5, and
                                                          launch_rows4t has no group branch any more
                 wave_ray_kernel<1..4>                    test_siddon_project[kernel 6]
                 trace_kernel                             test_siddon_trace
  siddon_packed.hip  pack2_kernel, group_codes_pack2_kernel   test_volume_pack2, test_volume_groups_pack2
                 rows16_kernel<2|3|4, W, false, STAGED, NOISY>   test_packed (2, 3, 4 materials; staged and unstaged; noisy and not;
                                                          16 / 32 / 64-lane groups: 255 / 256 / 257 rows; second z-chunk: 1100 rows)
                 rows16_kernel<3, 5|6|8>                  test_switches (DEXCT_P16_MINW)
                 rows16_kernel, 3 / 4 spectra (no staged store, four-slot detection); NOISY with one spectrum:
                                                          test_three_and_four_spectra, test_sample_with_one_spectrum
                 rows16_kernel<.., true> (group passes)   test_material_counts[grouped_packed], test_grouped_options
  siddon_cone.hip  cone_kernel (one thread per ray)       test_cone[cone], test_material_counts[cone]
                 every cone kernel: 1 / 3 / 4 spectra (energy pairs with an idle slot; the general loop), air, rays that miss the grid
                 or leave it through a z face: test_three_and_four_spectra, test_sample_with_one_spectrum, test_cone_rays_that_miss
                 cone_layout_kernel, cone_layout_groups_kernel   test_cone_layouts
                 cone_cols_kernel<1|2|3, 4, 288|544|1056>  test_cone[rows] (nz 250, 500, 1000), test_material_counts[cone_grouped]
                 cone_cols_kernel<.., 8, ..>              test_switches (DEXCT_CONE_KB=8)
                 cone_rows_kernel<1>, <2>, <3, 4>         test_cone[rows, nz 1040], test_switches (DEXCT_CONE_COLS=0)
                 cone_rows_kernel<3, 2>, <3, 8>, <3, 4, false>   test_switches (DEXCT_CONE_BATCH, DEXCT_CONE_LDSC)
                 every cone kernel with max_abs_dz the LAST float64 cone_slope_ok accepts (bounds_refs.EDGE_SCANS; the next one is
                 refused: test_refused_calls_launch_nothing) - one slice per slab on the diagonals of isotropic voxels:
                 cone_kernel<1|2|3> and <0> (5 ids)       test_cone_at_the_slope_limit[cone-edge, edge_m1, edge_m2, edge_m5, ..]
                 cone_cols_kernel<1|2|3, 4, 288>          [cone_rows-edge_m1, edge_m2, edge, edge_thin, edge_above (slices clamped
                                                          up to 66 past a z face), edge_aniso, edge288, edge_r257 (2 chunks of lanes),
                                                          edge_slabs (131 slabs: a flush of the byte counters), edge90]
                 cone_cols_kernel<3, 4, 544|1056>         [cone_rows-edge544, edge1056]
                 cone_rows_kernel<3, 4>                   [cone_rows-edge1040]
                 the group passes of all of these         [cone_grouped-*]: edge_m5 and edge_m7 take two and three passes
                 with the sample                          test_sample_at_the_slope_limit
                 cone_rows_kernel<3, 2|4|8, LDSC or not>, cone_cols_kernel<3, 8, 288|544>, a view tile of 3:
                                                          test_switches_at_the_slope_limit (the bits of the default form)
  detect.hip     detect_kernel<2..48, RMAX> / <.., 1>     test_material_counts (layout 1 with 8 rows: RMAX rays per thread; layout 0: one)
                 detect_kernel_chunked                    test_material_counts (49, 200; 1 through dexct_cone_project_grouped)
                 detect_kernel with 1, 3, 4 spectra, the sample of a view sub-range: test_three_and_four_spectra,
                                                          test_sample_with_one_spectrum, test_sample_of_a_view_sub_range
  noise.hip      add_noise_kernel                         the sampled cases (reference of the in-kernel sample)
                 add_noise_kernel, poisson_detect_kernel, sino_log_kernel, transpose_log_kernel: their bounds cases are in
                                                          tests/test_gpu_bounds.py (not repeated)

Outcome.  Reading for these tests found, and test_refused_calls_launch_nothing now pins:
  * dexct_cone_project_grouped validated its noise / log arguments after it had queued every group traversal: a call that
    returned DEXCT_EINVAL / DEXCT_ERANGE had already written acc_scratch.  Fixed (siddon_cone.hip): the detection pass's
    arguments are built and checked before the first launch_cone_rows.
  * n_materials == 1 with noise->sample on dexct_cone_project_grouped (the only group entry point that admits one material)
    returned noise-free counts and DEXCT_OK, because detect_kernel_chunked draws no sample.  Decided: refused with DEXCT_ERANGE
    (noise_log_args in csrc/proj_host.h; include/dexct.h says so); the variance output + dexct_add_noise remains.
Record of the run on an MI355X: the 466 cases of the two modules take 6.4 s; the -m gpu suite without them (the parent's
tests, run in the same visit on this library, not on a build of the parent commit) takes 252.6 s.  No guard changed, no
output depended on a fill, dexct_last_hip_error() stayed 0 on every launch form listed above, every output element was written
(rays that miss, idle lanes, ragged rows included), and every value check held: path lengths bit-equal on all rays, counts
within 2.7e-7 of the float64 Siddon (bound 1e-5).  Reconstruction, worst |err| / bound: Parker 0.50 (the one rounding),
filter 0.14, back-projection 0.13, FDK 0.05 - the derivations of tests/bounds_refs.py stand as written.  The refused-call
cases of dexct_cone_project_grouped pass with the fix above (the defect was found by reading; the unfixed library was not
run).  The issue's "66 rows of nz 80 from z_first 16" cannot be run (16 + 66 > 80: DEXCT_EINVAL); scan r66 has nz = 96.

The edge of the slope contract (test_cone_at_the_slope_limit, test_sample_at_the_slope_limit, test_switches_at_the_slope_limit,
the three max_dz = nextafter cases of test_refused_calls_launch_nothing).  Record of the run on an MI355X: these 73 cases take
2.5 s run alone, interpreter and library start included (this module's 470 cases 6.0 s; the 9 new cases of
tests/test_gpu_siddon.py 2.1 s alone; the whole -m gpu suite 332 s).  Nothing failed on the way and no kernel changed.  Per entry
point, over all its edge scans:
  dexct_cone_project          path lengths bit-equal to the mirror on all rays; counts within 2.15e-7 of the float64 Siddon (edge_m2)
  dexct_cone_project_rows     path lengths bit-equal on all rays; counts within 2.15e-7 (edge_m2); every A/B form the bits of the default
  dexct_cone_project_grouped  path lengths bit-equal on all rays; counts within 2.18e-7 (edge_m2)
No guard changed, no output depended on a fill, dexct_last_hip_error() stayed 0, every output element was written - with slice
indices up to 66 slices past a z face (edge_above), 248 past on rays that miss (edge_slabs) - and the library refuses exactly the
float64 after the one scan edge runs at.  Through Projector (test_random_cone_beam_scans_near_the_slope_limit, 0.906 - 0.998 of
the limit): path lengths bit-equal, counts within 7.4e-7.
"""
import ctypes as C

import numpy as np
import pytest

import bounds_refs as br
from bounds_refs import F32, F64, scan
from guarded import Arena, twice
from oracle import c_oracle as co
from test_gpu_bounds import np_log, ok
from test_gpu_siddon import REL_TOL

pytestmark = pytest.mark.gpu


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


def native_geom(s, **over):
    from dex_ct_sim_amd import _native
    g = s.geom(lambda *a: _native.FanGeom(*a[:7], 0, *a[7:]))
    for k, v in over.items():
        setattr(g, k, v)
    return g


# ---- NumPy restatements of include/dexct.h ------------------------------------------------------------------------------------

def np_pack2(b):
    b = b.reshape(-1, 4).astype(np.uint32) & 3
    return (b[:, 0] | (b[:, 1] << 2) | (b[:, 2] << 4) | (b[:, 3] << 6)).astype(np.uint8)


def np_groups(zf, n_mat):
    """codes[g][voxel]: ids 3g + 1 .. 3g + 3 -> 1 .. 3, every other id -> 0."""
    out = []
    for g in range((n_mat - 1 + 2) // 3):
        c = zf.astype(np.int64) - 3 * g
        out.append(np.where((c >= 1) & (c <= 3), c, 0).astype(np.uint8))
    return np.stack(out)


def np_cone_layout(vol, base=0):
    """A column is zs = ((nz + 15) & ~15) + 32 bytes, vol_zc[(y nx + x) zs + 16 + z] = 8 (id - base) for ids base .. base + 2,
    24 for every other id, every guard byte and one extra column."""
    nz, ny, nx = vol.shape
    zs = ((nz + 15) & ~15) + 32
    out = np.full((ny * nx + 1, zs), 24, np.uint8)
    c = vol.astype(np.int64).transpose(1, 2, 0).reshape(ny * nx, nz) - base
    out[:-1, 16:16 + nz] = np.where((c >= 0) & (c <= 2), 8 * c, 24)
    return out.reshape(-1)


# ---- 1. volume preparation and plan -------------------------------------------------------------------------------------------

SIZES = [1, 15, 16, 17, 255, 256, 257, 4099]


def guarded_call(hip, inputs, outputs, call, scratch=()):
    """inputs: name -> array; outputs: name -> bytes.  Returns name -> uint8 array of each output."""
    ar = Arena('cuda', hip)
    for n, a in inputs.items():
        ar.alloc(n, a.nbytes).put(a)
    for n, b in list(outputs.items()) + [(n, b) for n, b in scratch]:
        ar.alloc(n, b)
    return twice(ar, lambda: ok(call(ar)), list(outputs), scratch=[n for n, _ in scratch])


@pytest.mark.parametrize('n', SIZES + [4096 * 256 * 16 + 16, 8192 * 256 * 4 + 3])
def test_volume_ids_and_remap(hip, n):
    """dexct_volume_ids (16-byte vector body, grid capped at 4096 blocks) and dexct_volume_remap (in place, grid capped at 8192
    blocks of 4 bytes per thread), one size past each capped grid included."""
    rng = np.random.default_rng(n)
    vol = rng.integers(0, 256, n, dtype=np.uint8)
    got = guarded_call(hip, dict(vol=vol), dict(counts256=2048),
                       lambda ar: hip.dexct_volume_ids(ar['vol'].ptr, n, ar['counts256'].ptr, sp()))
    assert np.array_equal(got['counts256'].view(np.uint64), np.bincount(vol, minlength=256).astype(np.uint64))
    lut = rng.permutation(256).astype(np.uint8)
    lut_c = (C.c_uint8 * 256)(*lut.tolist())
    ar = Arena('cuda', hip)
    ar.alloc('vol', n)

    def remap():
        ar['vol'].put(vol)
        ok(hip.dexct_volume_remap(ar['vol'].ptr, n, lut_c, sp()))

    assert np.array_equal(twice(ar, remap, ['vol'])['vol'], lut[vol])


@pytest.mark.parametrize('nx,ny,nz', [(1, 1, 1), (5, 3, 1), (3, 5, 4), (17, 15, 16), (16, 17, 17), (7, 9, 48), (4099, 1, 1), (1, 257, 4),
                                      (15, 1, 1), (16, 1, 1), (1, 17, 1), (255, 1, 1), (1, 256, 1), (1, 1, 256), (257, 1, 1), (1, 1, 4099)])
@pytest.mark.parametrize('with_zf', [False, True])
def test_volume_layouts(hip, nx, ny, nz, with_zf):
    vol = np.random.default_rng(nx * ny + nz).integers(0, 256, (nz, ny, nx), dtype=np.uint8)
    outs = dict(vol_xy=vol.size, **(dict(vol_zf=vol.size) if with_zf else {}))
    got = guarded_call(hip, dict(vol=vol), outs, lambda ar: hip.dexct_volume_layouts(
        ar['vol'].ptr, nx, ny, nz, ar['vol_xy'].ptr, ar['vol_zf'].ptr if with_zf else None, sp()))
    assert np.array_equal(got['vol_xy'].reshape(nz, nx, ny), vol.transpose(0, 2, 1))
    if with_zf:
        assert np.array_equal(got['vol_zf'].reshape(ny, nx, nz), vol.transpose(1, 2, 0))


@pytest.mark.parametrize('n', [4, 16, 20, 256, 260, 1020, 1024, 1028, 4100])
def test_volume_pack2(hip, n):
    """pack2_kernel reads a uint32 per output byte: n / 4 of them, every size a multiple of 4 around the block edges."""
    zf = np.random.default_rng(n).integers(0, 4, n, dtype=np.uint8)
    got = guarded_call(hip, dict(vol_zf=zf), dict(vol_z2=n // 4), lambda ar: hip.dexct_volume_pack2(ar['vol_zf'].ptr, n, ar['vol_z2'].ptr, sp()))
    assert np.array_equal(got['vol_z2'], np_pack2(zf))


@pytest.mark.parametrize('n,n_mat', [(n, 5) for n in SIZES] + [(4099, 8), (4099, 10), (17, 2), (257, 256)])
def test_volume_groups(hip, n, n_mat):
    """group_codes_kernel: dword body and byte tail per group plane; 4099 voxels with three groups (8 and 10 materials) start the
    planes after the first off a dword boundary."""
    zf = np.random.default_rng(n + n_mat).integers(0, n_mat, n, dtype=np.uint8)
    n_groups = (n_mat - 1 + 2) // 3
    got = guarded_call(hip, dict(vol_zf=zf), dict(codes=n_groups * n), lambda ar: hip.dexct_volume_groups(ar['vol_zf'].ptr, n, n_mat, ar['codes'].ptr, sp()))
    assert np.array_equal(got['codes'].reshape(n_groups, n), np_groups(zf, n_mat))


@pytest.mark.parametrize('n,n_mat', [(4, 5), (16, 5), (20, 7), (256, 8), (260, 10), (1028, 5), (4100, 10), (4100, 256)])
def test_volume_groups_pack2(hip, n, n_mat):
    zf = np.random.default_rng(n + n_mat).integers(0, n_mat, n, dtype=np.uint8)
    n_groups = (n_mat - 1 + 2) // 3
    got = guarded_call(hip, dict(vol_zf=zf), dict(codes2=n_groups * n // 4),
                       lambda ar: hip.dexct_volume_groups_pack2(ar['vol_zf'].ptr, n, n_mat, ar['codes2'].ptr, sp()))
    want = np.stack([np_pack2(c) for c in np_groups(zf, n_mat)])
    assert np.array_equal(got['codes2'].reshape(n_groups, n // 4), want)


@pytest.mark.parametrize('nx,ny,nz', [(1, 1, 1), (5, 3, 4), (3, 5, 16), (4, 3, 17), (6, 2, 48), (2, 3, 257)])
def test_cone_layouts(hip, nx, ny, nz):
    """dexct_cone_layout and dexct_cone_layout_groups (1, 3, 4, 7 materials): the guard bytes of every column and the one extra
    column are written as well - all of dexct_cone_layout_bytes, and nothing beyond."""
    rng = np.random.default_rng(nx * ny * nz)
    nb = hip.dexct_cone_layout_bytes(nx, ny, nz)
    assert nb == (nx * ny + 1) * (((nz + 15) & ~15) + 32)
    vol = rng.integers(0, 3, (nz, ny, nx), dtype=np.uint8)
    got = guarded_call(hip, dict(vol=vol), dict(vol_zc=nb), lambda ar: hip.dexct_cone_layout(ar['vol'].ptr, nx, ny, nz, ar['vol_zc'].ptr, sp()))
    assert np.array_equal(got['vol_zc'], np_cone_layout(vol))
    for n_mat in (1, 3, 4, 7):
        vol = rng.integers(0, n_mat, (nz, ny, nx), dtype=np.uint8)
        n_groups = (n_mat + 2) // 3
        got = guarded_call(hip, dict(vol=vol), dict(vol_zcg=n_groups * nb),
                           lambda ar: hip.dexct_cone_layout_groups(ar['vol'].ptr, nx, ny, nz, n_mat, ar['vol_zcg'].ptr, sp()))
        want = np.concatenate([np_cone_layout(vol, 3 * g) for g in range(n_groups)])
        assert np.array_equal(got['vol_zcg'], want), n_mat


@pytest.mark.parametrize('name,vb,ve', [('r1', 0, 6), ('r1', 2, 5), ('c1', 1, 6), ('c2', 3, 4), ('wide', 1, 4), ('slabs', 0, 4), ('v1', 0, 1)])
def test_fan_plan(hip, name, vb, ve):
    """view_begin > 0 and channel counts (53, 1, 2, 32, 9) that leave a ragged last block: field by field against c_oracle.plan."""
    s = scan(name)
    g = native_geom(s)
    got = guarded_call(hip, dict(view_cs=s.view_cs, chan_cs=s.chan_cs), dict(plan=40 * (ve - vb) * s.n_ch),
                       lambda ar: hip.dexct_fan_plan(C.byref(g), ar['view_cs'].ptr, ar['chan_cs'].ptr, vb, ve, ar['plan'].ptr, sp()))
    ref = co.plan(s.geom(co.make_geom), s.view_cs, s.chan_cs, vb, ve)
    plan = got['plan'].view(co.PLAN_DTYPE)
    for f in ref.dtype.names:
        assert np.array_equal(plan[f], ref[f]), f


# ---- 2. projection ------------------------------------------------------------------------------------------------------------

EINVAL, ERANGE = -1, -2
FAN_ENTRIES = ('project', 'grouped', 'packed', 'grouped_packed')
CONE_ENTRIES = ('cone', 'cone_rows', 'cone_grouped')


_references = {}


def references(name, vb, ve):
    """(path lengths float32 [V][rows][ch][M], counts float64 [S][V][rows][ch], variance likewise) from the CPU oracle, cached."""
    if (name, vb, ve) not in _references:
        s = scan(name)
        g = s.geom(co.make_geom)
        if s.cone:
            cone = lambda w, dda: co.project_cone(g, s.view_cs, s.chan_cs, vb, ve, s.row_z, s.src_z, s.vol, s.mu, w, dda=dda, n_threads=8)
            pl, cnt, var = cone(s.w, True)[1], cone(s.w, False)[0], cone(s.w2, False)[0]
        else:
            _, pl = co.project_dda(g, s.view_cs, s.chan_cs, vb, ve, s.vol, s.mu, s.w, True, n_threads=8)
            cnt = co.project_classic(g, s.view_cs, s.chan_cs, vb, ve, s.vol, s.mu, s.w, n_threads=8)
            var = co.project_classic(g, s.view_cs, s.chan_cs, vb, ve, s.vol, s.mu, s.w2, n_threads=8)
        _references[(name, vb, ve)] = (pl, cnt, var)
    return _references[(name, vb, ve)]


def prepare(hip, s, entry, vb, ve, n_mat):
    """The inputs of one projection call in a fresh arena, each written by the library's own preparation call on guarded buffers
    of exact size (checked once here; their values are the subject of section 1)."""
    ar = Arena('cuda', hip)
    g = native_geom(s)
    nvox = s.vol.size
    for n, a in dict(vol=s.vol, view_cs=s.view_cs, chan_cs=s.chan_cs, mu=s.mu, w=s.w, w2=s.w2).items():
        ar.alloc(n, a.nbytes).put(a)
    if s.cone:
        ar.alloc('row_z', 8 * s.n_rows).put(s.row_z)
    ar.alloc('plan', 40 * (ve - vb) * s.n_ch)
    made = ['plan']
    calls = [lambda: hip.dexct_fan_plan(C.byref(g), ar['view_cs'].ptr, ar['chan_cs'].ptr, vb, ve, ar['plan'].ptr, sp())]
    if entry in FAN_ENTRIES or entry == 'cone':
        zf = entry != 'cone'                                             # (dexct_cone_project reads vol_yx and vol_xy only)
        ar.alloc('vol_xy', nvox)
        made.append('vol_xy')
        if zf:
            ar.alloc('vol_zf', nvox)
            made.append('vol_zf')
        calls.append(lambda: hip.dexct_volume_layouts(ar['vol'].ptr, s.nx, s.ny, s.nz, ar['vol_xy'].ptr, ar['vol_zf'].ptr if zf else None, sp()))
        n_groups = (n_mat - 1 + 2) // 3
        if entry == 'packed':
            ar.alloc('vol_z2', nvox // 4)
            calls.append(lambda: hip.dexct_volume_pack2(ar['vol_zf'].ptr, nvox, ar['vol_z2'].ptr, sp()))
            made.append('vol_z2')
        elif entry == 'grouped':
            ar.alloc('codes', n_groups * nvox)
            calls.append(lambda: hip.dexct_volume_groups(ar['vol_zf'].ptr, nvox, n_mat, ar['codes'].ptr, sp()))
            made.append('codes')
        elif entry == 'grouped_packed':
            ar.alloc('codes2', n_groups * nvox // 4)
            calls.append(lambda: hip.dexct_volume_groups_pack2(ar['vol_zf'].ptr, nvox, n_mat, ar['codes2'].ptr, sp()))
            made.append('codes2')
    elif entry == 'cone_rows':
        ar.alloc('vol_zc', hip.dexct_cone_layout_bytes(s.nx, s.ny, s.nz))
        calls.append(lambda: hip.dexct_cone_layout(ar['vol'].ptr, s.nx, s.ny, s.nz, ar['vol_zc'].ptr, sp()))
        made.append('vol_zc')
    else:
        ar.alloc('vol_zcg', ((n_mat + 2) // 3) * hip.dexct_cone_layout_bytes(s.nx, s.ny, s.nz))
        calls.append(lambda: hip.dexct_cone_layout_groups(ar['vol'].ptr, s.nx, s.ny, s.nz, n_mat, ar['vol_zcg'].ptr, sp()))
        made.append('vol_zcg')
    ar.fill(0xA5, inner=tuple(made))
    for c in calls:
        ok(c())
    ar.check()
    return ar


def project(hip, name, entry, *, vb=0, ve=None, kernel=1, layout=0, pathlen=True, log=False, var=False, sample=None, w2=None,
            M=None, S=None, geom_over=None, max_dz=None, expect=0, values=True):
    """One call of a projection entry point on guarded buffers under both fills.  ``M`` / ``S`` / ``geom_over`` / ``max_dz`` /
    ``w2``: arguments that differ from the scan's (the refused calls); every buffer is sized by the arguments the call is GIVEN.
    expect == 0: returns dict of outputs (float32 views) after the value checks (``values``); expect < 0: the call must return
    that code and leave outputs and scratch at their fill."""
    from dex_ct_sim_amd import _native
    s = scan(name)
    ve = s.n_views if ve is None else ve
    nV = ve - vb
    Mg, Sg = (s.n_mat if M is None else M), (s.n_spec if S is None else S)
    g = native_geom(s, **(geom_over or {}))
    n_rays = nV * g.n_rows * s.n_ch
    ar = prepare(hip, s, entry, vb, ve, max(s.n_mat, 2) if entry in FAN_ENTRIES else s.n_mat)
    if Mg != s.n_mat or Sg != s.n_spec:                                # tables as long as the arguments say
        ar.alloc('mu', 4 * Mg * s.n_e).put(np.resize(s.mu, (Mg, s.n_e)))
        ar.alloc('w', 4 * Sg * s.n_e).put(np.resize(s.w, (Sg, s.n_e)))
        ar.alloc('w2', 4 * Sg * s.n_e).put(np.resize(s.w2, (Sg, s.n_e)))
    w2 = (var or sample is not None) if w2 is None else w2
    outs = ['counts']
    ar.alloc('counts', 4 * Sg * n_rays)
    for flag, n, b in ((pathlen, 'pathlen', 4 * n_rays * Mg), (var, 'variance', 4 * Sg * n_rays), (log, 'sino_log', 4 * Sg * n_rays)):
        if flag:
            ar.alloc(n, b)
            outs.append(n)
    scratch = []
    if entry in ('grouped', 'grouped_packed', 'cone_grouped'):
        ar.alloc('acc_scratch', 4 * n_rays * Mg)
        scratch = ['acc_scratch']
    air = s.w.astype(F64).sum(1).astype(F32)
    P = lambda n: ar[n].ptr if n in ar.buffers else None
    mdz = s.max_abs_dz if (s.cone and max_dz is None) else max_dz

    def call():
        lo = _native.log_out(P('sino_log'), list(air)) if log else None
        nz = _native.noise(sample) if sample is not None else None
        pw2 = P('w2') if w2 else None
        if entry == 'project':
            return hip.dexct_siddon_project(C.byref(g), P('plan'), vb, ve, P('vol'), P('vol_xy'), P('vol_zf'), Mg, s.n_e, Sg, P('mu'), P('w'),
                                            P('counts'), P('pathlen'), kernel, layout, pw2, P('variance'), lo, sp())
        if entry in ('grouped', 'grouped_packed'):
            fn = hip.dexct_siddon_project_grouped if entry == 'grouped' else hip.dexct_siddon_project_grouped_packed
            return fn(C.byref(g), P('plan'), vb, ve, P('codes' if entry == 'grouped' else 'codes2'), Mg, s.n_e, Sg, P('mu'), P('w'),
                      P('counts'), P('pathlen'), P('acc_scratch'), layout, pw2, P('variance'), lo, nz, sp())
        if entry == 'packed':
            return hip.dexct_siddon_project_packed(C.byref(g), P('plan'), vb, ve, P('vol_z2'), Mg, s.n_e, Sg, P('mu'), P('w'), P('counts'),
                                                   P('pathlen'), layout, lo, pw2, P('variance'), nz, sp())
        head = (C.byref(g), P('plan'), P('view_cs'), P('chan_cs'), P('row_z'), s.src_z, mdz, vb, ve)
        if entry == 'cone':
            return hip.dexct_cone_project(*head, P('vol'), P('vol_xy'), Mg, s.n_e, Sg, P('mu'), P('w'), P('counts'), P('pathlen'), lo, pw2,
                                          P('variance'), nz, sp())
        if entry == 'cone_rows':
            return hip.dexct_cone_project_rows(*head, P('vol_zc'), Mg, s.n_e, Sg, P('mu'), P('w'), P('counts'), P('pathlen'), lo, pw2,
                                               P('variance'), nz, sp())
        return hip.dexct_cone_project_grouped(*head, P('vol_zcg'), Mg, s.n_e, Sg, P('mu'), P('w'), P('counts'), P('pathlen'),
                                              P('acc_scratch'), lo, pw2, P('variance'), nz, sp())

    if expect != 0:
        for byte in (0x00, 0xFF):
            ar.fill(byte, inner=tuple(outs + scratch))
            rc = call()
            assert rc == expect, (rc, expect)
            ar.check()                                                           # synchronises; last HIP error 0; guards
            for n in outs + scratch:
                assert np.all(ar[n].get() == byte), f'{n} was written by a call that returned {rc}'
        return None

    def launch():
        rc = call()
        assert rc == 0, rc

    got = {n: b.view(F32) for n, b in twice(ar, launch, outs, scratch=scratch).items()}
    lay = (lambda a: a) if (layout == 0 or s.cone) else (lambda a: np.swapaxes(a, -2, -1))   # -> [..][rows][channels]
    shape = (nV, s.n_rows, s.n_ch) if (layout == 0 or s.cone) else (nV, s.n_ch, s.n_rows)
    out = {'counts': lay(got['counts'].reshape((Sg,) + shape))}
    if pathlen:
        pl = got['pathlen'].reshape(shape + (Mg,))
        out['pathlen'] = pl if (layout == 0 or s.cone) else np.swapaxes(pl, 1, 2)
    for n in ('variance', 'sino_log'):
        if n in got:
            out[n] = lay(got[n].reshape((Sg,) + shape))
    out['raw'] = got
    if not values:
        return out
    ref_pl, ref_cnt, ref_var = references(name, vb, ve)
    tie = br.tie_rays(s, vb, ve)
    assert tie.mean() <= 0.02
    if pathlen:
        assert np.array_equal(out['pathlen'], ref_pl)                            # every ray, every material
    if sample is None:
        rel = br.counts_rel(out['counts'], ref_cnt, tie)
        print(name, entry, 'counts rel', rel)
        assert rel < REL_TOL, rel
    if var:
        rel = br.counts_rel(out['variance'], ref_var, tie)
        assert rel < REL_TOL, rel
    if log:
        want = np_log(air, out['counts'].reshape(Sg, -1)).reshape(out['counts'].shape)
        assert np.allclose(out['sino_log'], want, rtol=5e-6, atol=5e-7), np.abs(out['sino_log'] - want).max()
    return out


def sampled_equals_add_noise(hip, name, entry, seed=5, **kw):
    """The in-kernel sample against the same entry point's noise-free counts + variance followed by dexct_add_noise."""
    s = scan(name)
    vb, ve = kw.get('vb', 0), kw.get('ve', None) or s.n_views
    layout = 0 if s.cone else kw.get('layout', 0)
    noisy = project(hip, name, entry, sample=seed, **kw)
    clean = project(hip, name, entry, var=True, **{k: v for k, v in kw.items() if k != 'log'})
    ar = Arena('cuda', hip)
    ar.alloc('counts', clean['raw']['counts'].nbytes)
    ar.alloc('variance', clean['raw']['variance'].nbytes).put(clean['raw']['variance'])

    def add():
        ar['counts'].put(clean['raw']['counts'])
        ok(hip.dexct_add_noise(ar['counts'].ptr, ar['variance'].ptr, s.n_spec, ve - vb, s.n_rows, s.n_ch, layout, vb, seed, sp()))

    want = twice(ar, add, ['counts'])['counts'].view(F32)
    assert np.array_equal(noisy['raw']['counts'].view(np.int32), want.view(np.int32))
    assert not np.array_equal(want, clean['raw']['counts'])


ROWS = ['r1', 'r3', 'r4', 'r5', 'r15', 'r16', 'r17', 'r66', 'r257', 'r1100']


@pytest.mark.parametrize('kernel', [1, 2, 3, 5, 6])
@pytest.mark.parametrize('name', ROWS)
def test_siddon_project(hip, kernel, name):
    """dexct_siddon_project, every kernel, every row count: layout 0 with path lengths and the variance (kernel 6 takes none),
    layout 1 without path lengths and with the log sinogram; a sub-range of the views for half of the cases."""
    s = scan(name)
    sub = dict(vb=1, ve=s.n_views - 1) if s.n_rows % 2 and s.n_views >= 3 else {}
    project(hip, name, 'project', kernel=kernel, layout=0, pathlen=True, var=kernel != 6, **sub)
    project(hip, name, 'project', kernel=kernel, layout=1, pathlen=False, log=True, **sub)


@pytest.mark.parametrize('kernel', [1, 2, 3, 5, 6])
@pytest.mark.parametrize('name', ['c1', 'c2', 'v1', 's1', 's3', 's4', 'wide', 'air', 'slabs'])
def test_siddon_project_edges(hip, kernel, name):
    """1 and 2 channels, a single view, 1 / 3 / 4 spectra, a fan wider than the grid (rays that miss: their counts and path
    lengths are written all the same), an all-air volume, more than 512 slabs per ray (two staging passes)."""
    project(hip, name, 'project', kernel=kernel, layout=1, pathlen=True, log=True)


@pytest.mark.parametrize('name,n_mat_scan', [('r16', 3), ('r66', 3), ('r255', 3), ('r256', 3), ('r257', 3), ('r1100', 3), ('m2', 2), ('m4', 4),
                                             ('wide', 3), ('air', 3), ('slabs', 3), ('c1', 3), ('v1', 3)])
def test_packed(hip, name, n_mat_scan):
    """dexct_siddon_project_packed: staged store (layout 1, rows % 4 == 0, <= 2 spectra) and per-round stores (layout 0; r66,
    r255, r257: ragged rows), 2 / 3 / 4 materials, the 16 / 32 / 64-lane groups, the second z-chunk; the NOISY template with
    the variance output and with the sample."""
    project(hip, name, 'packed', layout=1, pathlen=True, log=True)
    project(hip, name, 'packed', layout=0, pathlen=False, var=True)
    if name in ('r16', 'r66', 'm2', 'm4', 'r257'):
        sampled_equals_add_noise(hip, name, 'packed', layout=1, pathlen=False, log=name != 'r257')
        sampled_equals_add_noise(hip, name, 'packed', layout=0, pathlen=False)


@pytest.mark.parametrize('entry', ['project-1', 'project-2', 'grouped', 'grouped_packed', 'cone', 'cone_grouped'])
@pytest.mark.parametrize('n_mat', br.MATERIALS)
def test_material_counts(hip, entry, n_mat):
    """1 .. 200 materials on every entry point that takes the count: launch_detect_any's templates 2 .. 48 (layout 1 with 8
    rows: several rays per thread; layout 0: one) and detect_kernel_chunked beyond, and for the single material of
    dexct_cone_project_grouped."""
    cone = entry.startswith('cone')
    name = f'cm{n_mat}' if cone else f'm{n_mat}'
    if entry.startswith('project'):
        project(hip, name, 'project', kernel=int(entry[-1]), layout=1, pathlen=True)
        return
    if entry == 'cone':
        project(hip, name, 'cone', pathlen=True, var=True)
        return
    if not cone and n_mat < 2:
        project(hip, name, entry, expect=-1)                                     # the stacked-fan groups need a second material
        return
    project(hip, name, entry, layout=1, pathlen=True, log=True)
    project(hip, name, entry, layout=0, pathlen=False, var=True)
    if 2 <= n_mat <= 48:
        sampled_equals_add_noise(hip, name, entry, layout=1, pathlen=False, log=True)


@pytest.mark.parametrize('entry', ['grouped', 'grouped_packed'])
@pytest.mark.parametrize('name', ['r16', 'r66', 'r257', 'wide', 'air', 'c2'])
def test_grouped_options(hip, entry, name):
    """The group passes (rows4_kernel<.., true>, rows16_kernel<.., true>) on 3 materials - one group of two - with ragged rows, a
    view sub-range, rays that miss and air: acc_scratch of M n_rays floats is all they may touch besides the outputs."""
    s = scan(name)
    sub = dict(vb=1, ve=s.n_views - 1) if s.n_views > 3 else {}
    project(hip, name, entry, layout=0, pathlen=True, **sub)
    project(hip, name, entry, layout=1, pathlen=True, var=True, **sub)


CONE_SCANS = ['cone', 'cone_m2', 'cm1', 'cone256', 'cone512', 'cone1024', 'cone1040', 'cone1040_m2', 'cone1040_m1']
# (dexct_cone_project has one kernel: the tall volumes add nothing to it)
CONE_CASES = [('cone', n) for n in CONE_SCANS[:4]] + [(e, n) for e in ('cone_rows', 'cone_grouped') for n in CONE_SCANS]


@pytest.mark.parametrize('entry,name', CONE_CASES)
def test_cone(hip, entry, name):
    """dexct_cone_project, dexct_cone_project_rows (cone_cols_kernel with columns of 288, 544 and 1056 bytes; cone_rows_kernel for
    1040 slices; 1, 2, 3 materials) and dexct_cone_project_grouped on the same scans; with the log, with the variance, with the
    sample, a view sub-range."""
    project(hip, name, entry, pathlen=True, log=True)
    project(hip, name, entry, pathlen=False, var=True, vb=1, ve=3)
    if scan(name).n_mat > 1 or entry != 'cone_grouped':
        sampled_equals_add_noise(hip, name, entry, pathlen=False, log=True)


SPECTRA_ENTRIES = ['packed', 'grouped', 'grouped_packed', 'cone', 'cone_rows', 'cone_grouped']


@pytest.mark.parametrize('entry', SPECTRA_ENTRIES)
@pytest.mark.parametrize('n_spec', [3, 4])
def test_three_and_four_spectra(hip, entry, n_spec):
    """3 and 4 spectra on every entry point besides dexct_siddon_project (test_siddon_project_edges): S n_rays floats of counts and
    of the log; the four-slot detection; for the packed kernel (layout 1, 8 rows) the per-round stores that more than two spectra
    force where the staged store would run; the cone kernels' general energy loop.  With the variance output where the entry
    point takes one for more than two spectra (the packed kernel refuses: DEXCT_ERANGE, nothing launched)."""
    cone = entry.startswith('cone')
    name = f'cs{n_spec}' if cone else f's{n_spec}'
    project(hip, name, entry, layout=1, pathlen=True, log=True)
    if not cone:
        project(hip, name, entry, layout=0, pathlen=False, log=True)
    if entry == 'packed':
        project(hip, name, entry, layout=1, var=True, expect=ERANGE)
    else:
        project(hip, name, entry, layout=1, pathlen=False, var=True, vb=1, ve=4)


@pytest.mark.parametrize('entry', SPECTRA_ENTRIES)
def test_sample_with_one_spectrum(hip, entry):
    """noise->sample on a single spectrum (the second slot of the fused variance and of the sample idle), whole scan and a view
    sub-range: the bits of the noise-free call + dexct_add_noise, the log of the sampled counts."""
    cone = entry.startswith('cone')
    name = 'cs1' if cone else 's1'
    sampled_equals_add_noise(hip, name, entry, layout=1, pathlen=False, log=True)
    sampled_equals_add_noise(hip, name, entry, layout=0, pathlen=False, vb=2, ve=5)


@pytest.mark.parametrize('entry,name', [('packed', 'r16'), ('packed', 'r66'), ('grouped', 'm5'), ('grouped_packed', 'm7'), ('cone', 'cone'),
                                        ('cone_rows', 'cone'), ('cone_grouped', 'cm7')])
def test_sample_of_a_view_sub_range(hip, entry, name):
    """view_begin > 0 with the sample: the Philox counter takes the GLOBAL view, as dexct_add_noise with view_offset = view_begin."""
    n = scan(name).n_views
    for layout in (1, 0):
        sampled_equals_add_noise(hip, name, entry, layout=layout, pathlen=False, log=layout == 1, vb=1, ve=n - 1)


@pytest.mark.parametrize('entry', ['cone', 'cone_rows', 'cone_grouped'])
@pytest.mark.parametrize('name', ['cone_air', 'cone_wide', 'cone_tall'])
def test_cone_rays_that_miss(hip, entry, name):
    """Cone scans of air only, with a fan wider than the grid and with detector rows far beyond the volume's top and bottom: rays
    that miss the grid, or leave it through a z face, still get every output element written."""
    project(hip, name, entry, pathlen=True, log=True)
    project(hip, name, entry, pathlen=True, var=True, vb=1, ve=4)
    sampled_equals_add_noise(hip, name, entry, pathlen=False, log=True, vb=2, ve=5)


# ---- the cone kernels at the edge of the slope contract: max_abs_dz is the last float64 dexct accepts (bounds_refs.EDGE_SCANS)

EDGE_CONE = ['edge', 'edge_m2', 'edge_m1', 'edge_m5', 'edge_thin', 'edge_above', 'edge_aniso', 'edge_slabs', 'edge90']
EDGE_CASES = ([('cone', n) for n in EDGE_CONE] + [('cone_rows', n) for n, kw in br.EDGE_SCANS.items() if kw.get('n_mat', 3) <= 3]
              + [('cone_grouped', n) for n in br.EDGE_SCANS])


@pytest.mark.parametrize('entry,name', EDGE_CASES)
def test_cone_at_the_slope_limit(hip, entry, name):
    """Every ray of every edge scan: three-piece slabs with tv == tw ties (edge*), slice indices tens of slices past either z face
    under the clamp of the row kernels (edge_thin, edge_above, edge_slabs), every staged-column width and cone_rows_kernel
    (edge288 .. edge1040), a second chunk of lanes (edge_r257), a flush of the byte counters inside a steep ray (edge_slabs),
    1 / 2 / 3 materials and two and three group passes (edge_m*).  With path lengths and the log, then with the variance."""
    project(hip, name, entry, pathlen=True, log=True)
    project(hip, name, entry, pathlen=False, var=True)


@pytest.mark.parametrize('entry', CONE_ENTRIES)
@pytest.mark.parametrize('name', ['edge', 'edge_thin'])
def test_sample_at_the_slope_limit(hip, entry, name):
    sampled_equals_add_noise(hip, name, entry, pathlen=False, log=True)


CONE_KNOBS = ('DEXCT_CONE_COLS', 'DEXCT_CONE_KB', 'DEXCT_CONE_BATCH', 'DEXCT_CONE_LDSC', 'DEXCT_CONE_VIEW_TILE')
# (DEXCT_CONE_BATCH and DEXCT_CONE_LDSC act on cone_rows_kernel: on these scans together with DEXCT_CONE_COLS=0, on edge1040 alone)
EDGE_FORMS = [dict(DEXCT_CONE_COLS='0'), dict(DEXCT_CONE_KB='8'), dict(DEXCT_CONE_BATCH='2'), dict(DEXCT_CONE_BATCH='8'),
              dict(DEXCT_CONE_LDSC='0'), dict(DEXCT_CONE_VIEW_TILE='3'), dict(DEXCT_CONE_COLS='0', DEXCT_CONE_BATCH='2'),
              dict(DEXCT_CONE_COLS='0', DEXCT_CONE_BATCH='8'), dict(DEXCT_CONE_COLS='0', DEXCT_CONE_LDSC='0')]
EDGE_SWITCHES = ([('cone_rows', n, env) for n in ('edge', 'edge544') for env in EDGE_FORMS]
                 + [('cone_rows', 'edge1040', env) for env in EDGE_FORMS[2:5]] + [('cone_grouped', 'edge_m7', EDGE_FORMS[0])]
                 # cone_rows_kernel's own clamp of the slice index, 33 and 66 slices past a z face
                 + [('cone_rows', n, EDGE_FORMS[0]) for n in ('edge_thin', 'edge_above')])
_default_form = {}


@pytest.mark.parametrize('entry,name,env', EDGE_SWITCHES, ids=[f'{e}-{n}-{"-".join(f"{k}={v}" for k, v in env.items())}' for e, n, env in EDGE_SWITCHES])
def test_switches_at_the_slope_limit(hip, monkeypatch, entry, name, env):
    """The A/B launch forms on steep rays: guarded like every case, and the bits of the default form in every output."""
    for k in CONE_KNOBS:
        monkeypatch.delenv(k, raising=False)
    if (entry, name) not in _default_form:
        _default_form[entry, name] = project(hip, name, entry, pathlen=True, log=True)['raw']
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = project(hip, name, entry, pathlen=True, log=True)['raw']
    for n, a in _default_form[entry, name].items():
        assert np.array_equal(got[n].view(np.int32), a.view(np.int32)), (n, env)


SWITCHES = [('project', 'r66', dict(kernel=3), 'DEXCT_VIEW_TILE', '2'), ('packed', 'r16', {}, 'DEXCT_P16_STAGED', '0'),
            ('packed', 'r16', {}, 'DEXCT_DET_MASKS', '0'), ('packed', 'r16', {}, 'DEXCT_P16_MINW', '5'),
            ('packed', 'r16', {}, 'DEXCT_P16_MINW', '6'), ('packed', 'r16', {}, 'DEXCT_P16_MINW', '8'),
            ('packed', 'r66', {}, 'DEXCT_P16_MINW', '5'), ('project', 'r17', dict(kernel=1), 'DEXCT_RAYS_BATCH', '1'),
            ('project', 'r17', dict(kernel=1), 'DEXCT_RAYS_BATCH', '8'), ('project', 'r17', dict(kernel=1), 'DEXCT_RAYS_BATCH', '16'),
            ('cone_rows', 'cone', {}, 'DEXCT_CONE_COLS', '0'), ('cone_rows', 'cone_m2', {}, 'DEXCT_CONE_COLS', '0'),
            ('cone_rows', 'cone', {}, 'DEXCT_CONE_KB', '8'), ('cone_rows', 'cone512', {}, 'DEXCT_CONE_KB', '8'),
            ('cone_rows', 'cone', {}, 'DEXCT_CONE_VIEW_TILE', '2'), ('cone_rows', 'cone1040', {}, 'DEXCT_CONE_BATCH', '2'),
            ('cone_rows', 'cone1040', {}, 'DEXCT_CONE_BATCH', '8'), ('cone_rows', 'cone1040', {}, 'DEXCT_CONE_LDSC', '0'),
            ('cone_grouped', 'cm7', {}, 'DEXCT_CONE_COLS', '0')]


@pytest.mark.parametrize('entry,name,kw,var,value', SWITCHES, ids=[f'{e}-{n}-{v}={x}' for e, n, _, v, x in SWITCHES])
def test_switches(hip, monkeypatch, entry, name, kw, var, value):
    """The environment switches that select another launch form (read per call), one guarded case each."""
    monkeypatch.setenv(var, value)
    project(hip, name, entry, layout=0 if entry.startswith('cone') else 1, pathlen=True, log=True, **kw)
    if entry == 'packed':
        project(hip, name, entry, layout=0, pathlen=True)


@pytest.mark.parametrize('name,n,max_seg', [('r17', 1, 64), ('r17', 63, 64), ('r17', 64, 3), ('wide', 65, 40), ('slabs', 7, 1200)])
def test_siddon_trace(hip, name, n, max_seg):
    """dexct_siddon_trace on 1, 63, 64, 65 rays: n_seg and the first n_seg entries of each ray against c_oracle.dda_ray; the
    entries of a ray past its last segment keep the fill, and with max_seg = 3 a ray writes its first three segments only."""
    s = scan(name)
    g = native_geom(s)
    rng = np.random.default_rng(n)
    rays = np.stack([rng.integers(0, s.n_views, n), rng.integers(0, s.n_rows, n), rng.integers(0, s.n_ch, n)], 1).astype(np.int32)
    ar = prepare(hip, s, 'project', 0, s.n_views, s.n_mat)
    ar.alloc('ray_vrc', 12 * n).put(rays)
    outs = dict(seg_voxel=4 * n * max_seg, seg_len=4 * n * max_seg, n_seg=4 * n)
    for k, b in outs.items():
        ar.alloc(k, b)
    ref_plan = co.plan(s.geom(co.make_geom), s.view_cs, s.chan_cs, 0, s.n_views)
    og = s.geom(co.make_geom)
    got = {}
    for byte in (0x00, 0xFF):                      # entries past n_seg are not part of the contract: compare the written ones
        ar.fill(byte, inner=tuple(outs))
        ok(hip.dexct_siddon_trace(C.byref(g), ar['plan'].ptr, ar['ray_vrc'].ptr, n, max_seg, ar['seg_voxel'].ptr, ar['seg_len'].ptr,
                                  ar['n_seg'].ptr, sp()))
        ar.check()
        ns = ar['n_seg'].get(np.int32)
        vox, ln = ar['seg_voxel'].get(np.int32).reshape(n, max_seg), ar['seg_len'].get(F32).reshape(n, max_seg)
        for k, (v, r, c) in enumerate(rays):
            rv, rl = co.dda_ray(og, ref_plan[v * s.n_ch + c], s.z_first + r)
            m = min(len(rv), max_seg)
            assert ns[k] == len(rv), (k, ns[k], len(rv))                      # (the count runs on past max_seg)
            assert np.array_equal(vox[k, :m], rv[:m]) and np.array_equal(ln[k, :m], rl[:m]), k
            # nothing is written past a ray's own segments: the rest of its max_seg entries still holds the fill
            assert np.all(vox[k, m:].view(np.uint8) == byte) and np.all(ln[k, m:].view(np.uint8) == byte), k
        got[byte] = ns
    assert np.array_equal(got[0x00], got[0xFF])


# ---- 3. a refused call launches nothing ---------------------------------------------------------------------------------------

REFUSED = [
    # dexct_siddon_project
    ('project', 'r16', dict(kernel=3, geom_over=dict(nz=31)), EINVAL),            # unaligned nz for kernel 3
    ('project', 'r16', dict(kernel=3, geom_over=dict(z_first=14)), EINVAL),       # unaligned z_first
    ('project', 'r16', dict(kernel=1, w2=True), EINVAL),                          # weights2 without a variance output
    ('project', 'r16', dict(kernel=1, var=True, log=True), EINVAL),               # log_out together with a variance output
    ('project', 'r16', dict(kernel=6, var=True), EINVAL),                         # kernel 6 takes no variance
    ('project', 'r16', dict(kernel=4), EINVAL),
    ('project', 'r16', dict(kernel=1, S=5), ERANGE),                              # five spectra
    ('project', 'm5', dict(kernel=3), EINVAL),                                    # five materials on the packed-count kernel
    # dexct_siddon_project_grouped / _grouped_packed
    ('grouped', 's3', dict(sample=3), ERANGE),                                    # sample with three spectra
    ('grouped_packed', 's3', dict(sample=3), ERANGE),
    ('grouped', 'm49', dict(sample=3), ERANGE),                                   # sample with 49 materials
    ('grouped_packed', 'm49', dict(sample=3), ERANGE),
    ('grouped', 'm5', dict(w2=True), EINVAL),                                     # weights2 without variance or sample
    ('grouped_packed', 'm5', dict(w2=True), EINVAL),
    ('grouped', 'm5', dict(var=True, log=True), EINVAL),                          # log_out with a variance output and no sample
    ('grouped_packed', 'm5', dict(var=True, log=True), EINVAL),
    ('grouped', 'r16', dict(geom_over=dict(z_first=14)), EINVAL),
    ('grouped_packed', 'r16', dict(geom_over=dict(z_first=12)), EINVAL),          # a multiple of 4, not of 16
    ('grouped', 'm1', dict(), EINVAL),
    # dexct_siddon_project_packed
    ('packed', 'r16', dict(geom_over=dict(z_first=12)), EINVAL),
    ('packed', 'r16', dict(geom_over=dict(nz=24)), EINVAL),
    ('packed', 'm5', dict(), ERANGE),
    ('packed', 'r16', dict(w2=True), EINVAL),
    ('packed', 'r16', dict(var=True, log=True), EINVAL),
    ('packed', 's3', dict(sample=3), ERANGE),
    # the cone entry points
    ('cone', 'cone', dict(max_dz=1e4), ERANGE),                                   # too steep a cone
    ('cone_rows', 'cone', dict(max_dz=1e4), ERANGE),
    ('cone_grouped', 'cm7', dict(max_dz=1e4), ERANGE),
    # the float64 after the last accepted one (scan edge runs AT that one in test_cone_at_the_slope_limit)
    ('cone', 'edge', dict(max_dz=float(np.nextafter(scan('edge').max_abs_dz, np.inf))), ERANGE),
    ('cone_rows', 'edge', dict(max_dz=float(np.nextafter(scan('edge').max_abs_dz, np.inf))), ERANGE),
    ('cone_grouped', 'edge', dict(max_dz=float(np.nextafter(scan('edge').max_abs_dz, np.inf))), ERANGE),
    ('cone_rows', 'cm4', dict(), ERANGE),                                         # more than 3 materials on the row kernels
    ('cone', 'cone', dict(w2=True), EINVAL),
    ('cone_rows', 'cone', dict(w2=True), EINVAL),
    ('cone', 'cone', dict(var=True, log=True), EINVAL),
    ('cone_rows', 'cone', dict(var=True, log=True), EINVAL),
    # dexct_cone_project_grouped: these returned their code only AFTER the group traversals had written acc_scratch
    ('cone_grouped', 'cm7', dict(w2=True), EINVAL),
    ('cone_grouped', 'cm7', dict(var=True, log=True), EINVAL),
    ('cone_grouped', 'cm7', dict(sample=3, S=3), ERANGE),
    ('cone_grouped', 'cm49', dict(sample=3), ERANGE),
    ('cone_grouped', 'cm1', dict(sample=3), ERANGE),                              # one material + sample: refused (include/dexct.h)
]


@pytest.mark.parametrize('entry,name,kw,code', REFUSED, ids=[f'{e}-{n}-{"-".join(f"{k}={v}" for k, v in kw.items())}' for e, n, kw, _ in REFUSED])
def test_refused_calls_launch_nothing(hip, entry, name, kw, code):
    """A call that returns DEXCT_EINVAL / DEXCT_ERANGE has started no kernel: after the call and a synchronise every guarded
    buffer - counts, path lengths, variance, log and acc_scratch - still holds its fill byte and dexct_last_hip_error() is 0."""
    kw = dict(kw)
    if entry in FAN_ENTRIES and entry != 'project':
        kw.setdefault('layout', 1)
    project(hip, name, entry, expect=code, **kw)
