"""rows16_kernel counts the slabs in z-uniform columns once per (view, channel) pair: the column-class map and the projection that
uses it, on the device, byte for byte (guarded buffers, tests/guarded.py).  The reference everywhere is the same library with every
map off (DEXCT_P16_AIR_SKIP=0: the untouched kernels without a map), not a tolerance.

(a) dexct_volume_column_classes against a NumPy restatement: the map words and the per-id counts, guard bands pre-filled with 0x00
    and 0xFF, columns uniform in each id and uniform but for one voxel (the first, the last, each place within a byte, either side
    of a dword boundary), more columns than the capped grid covers in one trip, and the argument refusals (nothing launched).
(b) dexct_siddon_project_packed_uniform with the class map forced on against the map off: counts, log sinogram, path lengths.
    n = 32 and 160 (more than kP16Super = 128 slabs per ray: several passes); nz = 16 / 64 / 512 / 1040 (16, 16, 32 lanes per pair,
    z-chunks); 2, 3 and 4 ids; staged and unstaged (layout 0, and a row count that is no multiple of 4); n_rows below nz from
    z_first = 16; DEXCT_DET_DEDUP 0 and 1; six volumes (CONTENTS).  The noisy kernels keep the air rule (they were not built with
    the class rule): one case shows that the new entry point gives them the air map.  So does the unstaged three-material kernel
    (csrc: p16_by_class), whose runs here therefore compare the air map against no map.
(c) the map is what the kernel reads: a fabricated map that calls every column uniform in id 1 gives the bytes of an all-water
    volume of that grid; with the knob at 0 the volume's own bytes.
(d) the auto rule on both sides of its share, DEXCT_P16_UNIFORM 0 / 1 / 2, and counts the builder cannot have given."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Arena, twice

pytestmark = pytest.mark.gpu

N_VIEWS, N_CHANNELS = 8, 24


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


def ok(rc):
    assert rc == 0, rc


class SinceStart:
    """dexct_last_hip_error is sticky, and argument-check tests of other modules leave it set on purpose: Arena.check, which
    wants 0 after every launch, gets 0 while the error is the one the case started with (as tests/test_gpu_grid_passes.py)."""

    def __init__(self, hip):
        self.hip, self.before = hip, hip.dexct_last_hip_error()

    def dexct_last_hip_error(self):
        now = self.hip.dexct_last_hip_error()
        return 0 if now == self.before else now


def arena(hip):
    return Arena('cuda', SinceStart(hip))


def pack2(vol):
    """[nz][ny][nx] ids < 4 -> the bytes of vol_z2 [ny][nx][nz / 4] (NumPy restatement of dexct_volume_pack2)."""
    zf = np.ascontiguousarray(vol.transpose(1, 2, 0)).reshape(vol.shape[1], vol.shape[2], -1, 4).astype(np.uint8)
    return (zf[..., 0] | (zf[..., 1] << 2) | (zf[..., 2] << 4) | (zf[..., 3] << 6)).astype(np.uint8)


def class_words(vol):
    """The class map NumPy makes of a [nz][ny][nx] volume: (uint32 words, [columns uniform in id 0 .. 3])."""
    uniform = (vol == vol[0]).all(axis=0).reshape(-1)
    ids = vol[0].reshape(-1).astype(np.uint32)
    cls = np.zeros(-(-uniform.size // 8) * 8, dtype=np.uint32)
    cls[:uniform.size] = np.where(uniform, 1 | (ids << 1), 0)
    words = np.bitwise_or.reduce(cls.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32)), axis=1).astype(np.uint32)
    return words, [int((uniform & (ids == k)).sum()) for k in range(4)]


# ---- (a) the map builder ------------------------------------------------------------------------------------------------------

def recipes(nz):
    """What a column can be: None = uniform, or the z of its one odd voxel."""
    odd = [0, nz - 1] + [4 * (nz // 8) + p for p in range(4)] + [15, 16, 4 * (nz // 4) - 5]
    return [None] + sorted({z for z in odd if 0 <= z < nz})


def recipe_volume(nx, ny, nz, shift):
    """Column c: base id (c // R) % 4 over all z, and recipe (c + shift) % R of the R recipes; an odd voxel holds another id."""
    rec = recipes(nz)
    c = np.arange(nx * ny)
    base = ((c // len(rec)) % 4).astype(np.uint8)
    vol = np.broadcast_to(base, (nz, nx * ny)).copy()
    which = (c + shift) % len(rec)
    for k, z in enumerate(rec):
        if z is not None:
            sel = which == k
            vol[z, sel] = (base[sel] + 1 + c[sel] % 3) % 4
    return vol.reshape(nz, ny, nx)


@pytest.mark.parametrize('nx,ny,nz,offset', [(1, 1, 4, 0), (5, 7, 4, 0), (33, 31, 16, 0), (33, 31, 16, 1), (64, 64, 64, 0), (21, 19, 24, 0),
                                             (1025, 1024, 4, 0)])
def test_column_class_map(hip, nx, ny, nz, offset):
    """1025 x 1024 columns are 1024 more than the 4096 workgroups of 256 take in one trip (csrc: kColAirMaxBlocks).  Shapes with
    fewer columns than recipes run once per recipe, so that every column meets every recipe."""
    n_rec = len(recipes(nz))
    for shift in (range(n_rec) if nx * ny < 4 * n_rec else (0,)):
        vol = recipe_volume(nx, ny, nz, shift)
        want, n_want = class_words(vol)
        if nx * ny >= 4 * n_rec:
            assert all(n_want) and sum(n_want) < nx * ny, n_want        # uniform columns of every id, and mixed ones
        ar = arena(hip)
        ar.alloc('vol_z2', nx * ny * nz // 4, offset=offset).put(pack2(vol))
        ar.alloc('col_class', 4 * want.size)
        ar.alloc('n_uniform', 32)
        got = twice(ar, lambda: ok(hip.dexct_volume_column_classes(ar['vol_z2'].ptr, nx, ny, nz, ar['col_class'].ptr, ar['n_uniform'].ptr,
                                                                   sp())), ['col_class', 'n_uniform'])
        assert np.array_equal(got['col_class'].view(np.uint32), want)
        assert got['n_uniform'].view(np.uint64).tolist() == n_want


def test_column_class_map_arguments(hip):
    ar = arena(hip)
    for n, b in (('v', 64), ('m', 64), ('c', 32)):
        ar.alloc(n, b)
    call = lambda v='v', m='m', c='c', nx=4, ny=4, nz=16: hip.dexct_volume_column_classes(
        ar[v].ptr if v else None, nx, ny, nz, ar[m].ptr if m else None, ar[c].ptr if c else None, sp())
    ar.fill(0x5A, inner=('v', 'm', 'c'))
    assert call(v=None) == -1 and call(m=None) == -1 and call(c=None) == -1
    assert call(nx=0) == -1 and call(ny=-1) == -1 and call(nz=0) == -1 and call(nz=18) == -1
    assert call(nx=65536, ny=32768) == -2
    ar.check()
    assert all(np.all(ar[n].get() == 0x5A) for n in ('m', 'c'))          # a refused call launches nothing


# ---- (b) .. (d): the packed projection on guarded buffers ------------------------------------------------------------------------

def materials(n_mat):
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    return ([AIR, WATER, BONE] + [Material(f'm{i}', 1.0 + 0.1 * i, 'H(11.2)O(88.8)') for i in range(3, n_mat)])[:n_mat]


CONTENTS = ['rods', 'rods+sphere', 'one voxel off', 'water', 'shuffled', 'air']


def make_volume(kind, nz, n, n_ids, seed):
    """[nz][n][n] ids 0 .. n_ids - 1.
    'rods': an extruded disc of id 1 with two touching extruded rods inside it - ids 2 and 3, or as many of them as there are, the
        rest holes of air: crossings between uniform columns of different ids; 'rods+sphere': the same and a sphere of the last id;
    'one voxel off': every column uniform in a random id but for one voxel - nothing is droppable;
    'water': id 1 to the grid's edge - pieces outside the grid sit against non-air; 'shuffled': the voxels of every slice of
        'rods+sphere' permuted independently; 'air': nothing."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n]
    c = 0.5 * (n - 1)
    vol = np.zeros((nz, n, n), dtype=np.uint8)
    if kind == 'air':
        return vol
    if kind == 'water':
        vol[:] = 1
        return vol
    if kind == 'one voxel off':
        base = rng.integers(0, n_ids, (n, n), dtype=np.uint8)
        vol[:] = base
        vol[rng.integers(0, nz, (n, n)), y, x] = (base + rng.integers(1, n_ids, (n, n), dtype=np.uint8)) % n_ids
        return vol
    vol[:, (x - c) ** 2 + (y - c) ** 2 <= (0.42 * n) ** 2] = 1
    rod_ids = {4: (2, 3), 3: (2, 0), 2: (0, 0)}[n_ids]
    for k, rid in enumerate(rod_ids):
        cx = c + 0.1 * n * (2 * k - 1)
        vol[:, (x - cx) ** 2 + (y - c) ** 2 <= (0.1 * n) ** 2] = rid
    if kind == 'rods':
        return vol
    r = min(0.15 * n, 0.45 * nz)
    zc = 0.5 * (nz - 1)
    z0, z1 = max(0, int(zc - r)), min(nz, int(zc + r) + 2)             # (the slices the sphere can touch)
    z = np.arange(z0, z1)[:, None, None]
    vol[z0:z1][(x - c) ** 2 + (y - (c + 0.22 * n)) ** 2 + (z - zc) ** 2 <= r * r] = n_ids - 1
    if kind == 'shuffled':
        vol = rng.permuted(vol.reshape(nz, -1), axis=1).reshape(nz, n, n)
    else:
        assert kind == 'rods+sphere'
    return vol


class Scan:
    """One fan scan of an [nz][n][n] grid with ``n_ids`` ids.  The projector (kernel 7) is built on a volume that holds every id,
    so that the table rows are the ids; ``load`` then puts a volume, its packing and both its maps into guarded buffers, and
    ``run`` calls the new entry point on them with any stack of rows of that volume."""

    def __init__(self, hip, n, nz, n_ids):
        import dex_ct_sim_amd as dx
        from dex_ct_sim_amd import forward_project as fp, synthetic
        self.hip, self.n, self.nz, self.M = hip, n, nz, n_ids
        template = np.random.default_rng(1).integers(0, n_ids, (nz, n, n), dtype=np.uint8)
        ph = dx.VoxelPhantom.from_array('uniform-columns', template, materials(n_ids), dx=0.1, dy=0.1, dz=0.1)
        ct = dx.FanBeamGeometry(N_channels=N_CHANNELS, N_proj=N_VIEWS, gamma_fan=2 * np.arctan(0.5 * n * 0.1 / 60.0), SID=60.0, SDD=100.0,
                                N_rows=nz)
        specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
        for s_ in specs:
            s_.rescale_counts(1e-2)
        _, mu, w, w2 = fp.merged_tables(ct, ph, specs, with_variance=True)
        self.pj = fp.Projector(ct, ph, kernel=7)
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')
        self.mu, self.w, self.w2, self.air = dev(self.pj.compact(mu)), dev(w), dev(w2), w.sum(axis=1)
        assert self.pj.use_packed and self.pj.n_mat == n_ids and self.pj.geom.nz == nz and self.pj.geom.z_first == 0
        ar = self.ar = arena(hip)
        ar.alloc('vol_z2', nz * n * n // 4)
        ar.alloc('col_air', 4 * (-(-n * n // 32)))
        ar.alloc('n_air', 8)
        ar.alloc('col_class', 4 * (-(-n * n // 8)))
        ar.alloc('n_uniform', 32)

    def load(self, vol):
        from dex_ct_sim_amd._device import ptr
        hip, ar, n, nz = self.hip, self.ar, self.n, self.nz
        zf = torch.from_numpy(np.ascontiguousarray(vol.transpose(1, 2, 0))).cuda()         # [ny][nx][nz], what vol_zf holds
        ar.fill(0xA5, inner=('vol_z2', 'col_air', 'n_air', 'col_class', 'n_uniform'))
        ok(hip.dexct_volume_pack2(ptr(zf), vol.size, ar['vol_z2'].ptr, sp()))
        ok(hip.dexct_volume_air_columns(ar['vol_z2'].ptr, n, n, nz, ar['col_air'].ptr, ar['n_air'].ptr, sp()))
        ok(hip.dexct_volume_column_classes(ar['vol_z2'].ptr, n, n, nz, ar['col_class'].ptr, ar['n_uniform'].ptr, sp()))
        ar.check()
        words, self.n_uniform = class_words(vol)
        if vol.size <= 1 << 22:                                           # (the packing has tests of its own)
            assert np.array_equal(ar['vol_z2'].get().reshape(n, n, nz // 4), pack2(vol))
        assert np.array_equal(ar['col_class'].get(np.uint32), words) and ar['n_uniform'].get(np.uint64).tolist() == self.n_uniform
        self.n_air = int(ar['n_air'].get(np.uint64)[0])
        assert self.n_air == self.n_uniform[0]
        return self

    def run(self, *, rows=None, layout=1, both_fills=True, noisy=False, col_class='col_class', n_uniform=None, air_map=True, rc=0):
        """One call (both fills of the guards and outputs, or one); returns the host bytes of counts, sino_log and pathlen."""
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        hip, ar, pj = self.hip, self.ar, self.pj
        n_rows, z_first = rows if rows is not None else (self.nz, 0)
        geom = _native.FanGeom.from_buffer_copy(pj.geom)
        geom.n_rows, geom.z_first = n_rows, z_first
        rays = N_VIEWS * N_CHANNELS * n_rows
        names = {k: f'{k}{n_rows}' for k in ('counts', 'sino_log', 'pathlen', 'variance')}
        for k, b in (('counts', 8 * rays), ('sino_log', 8 * rays), ('variance', 8 * rays), ('pathlen', 4 * rays * self.M)):
            if names[k] not in ar.buffers:
                ar.alloc(names[k], b)
        outs = ['counts', 'sino_log', 'pathlen'] + (['variance'] if noisy else [])
        counts = (C.c_int64 * 4)(*(self.n_uniform if n_uniform is None else n_uniform))

        def launch():
            got = hip.dexct_siddon_project_packed_uniform(
                C.byref(geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, self.M, self.w.shape[1], 2, ptr(self.mu), ptr(self.w),
                ar[names['counts']].ptr, ar[names['pathlen']].ptr, layout, _native.log_out(ar[names['sino_log']].ptr, list(self.air)),
                ptr(self.w2) if noisy else None, ar[names['variance']].ptr if noisy else None, _native.noise(9) if noisy else None,
                ar['col_air'].ptr if air_map else None, self.n_air if air_map else 0, ar[col_class].ptr if col_class else None,
                counts if col_class else None, sp())
            assert got == rc, got

        got = twice(ar, launch, [names[k] for k in outs], fills=(0x00, 0xFF) if both_fills else (0x00,))
        return {k: got[names[k]] for k in outs}


def same(a, b, what):
    for n in a:
        assert n in b and np.array_equal(a[n], b[n]), f'{what}: {n} differs'


def knobs(monkeypatch, air_skip=None, uniform=None, dedup=None):
    for name, v in (('DEXCT_P16_AIR_SKIP', air_skip), ('DEXCT_P16_UNIFORM', uniform), ('DEXCT_DET_DEDUP', dedup)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def lengths(got, M):
    return got['pathlen'].view(np.float32).reshape(-1, M)


# every depth and id count on the small grid; the grid of several passes at the two depths of 16 lanes per pair with every id count,
# and once each at 32 lanes per pair and with z-chunks (passes go by a ray's slabs, lanes and chunks by its rows: they do not meet)
SCANS = ([(32, nz, ids) for nz in (16, 64, 512, 1040) for ids in (2, 3, 4)] + [(160, nz, ids) for nz in (16, 64) for ids in (2, 3, 4)] +
         [(160, 512, 3), (160, 1040, 4)])


@pytest.mark.parametrize('n,nz,n_ids', SCANS)
def test_map_on_equals_map_off(hip, monkeypatch, n, nz, n_ids):
    scan = Scan(hip, n, nz, n_ids)
    # the whole stack; rows from z_first = 16 that end before nz; the same with a row count that is no multiple of 4 (unstaged)
    stacks = [((nz, 0), 1, (0, 1)), ((nz, 0), 0, (1,))]
    if nz >= 64:
        stacks += [((nz - 32, 16), 1, (0, 1)), ((nz - 34, 16), 1, (1,)), ((nz - 34, 16), 0, (1,))]
    if nz == 16:
        stacks += [((1, 0), 1, (1,))]                                  # one row only: unstaged
    for kind in CONTENTS:
        vol = make_volume(kind, nz, n, n_ids, 31 * nz + n + n_ids)
        scan.load(vol)
        if kind == 'one voxel off':
            assert scan.n_uniform == [0, 0, 0, 0]                      # the map must say that nothing is droppable
        if kind in ('water', 'air'):
            assert scan.n_uniform[kind == 'water'] == n * n
        for rows, layout, dedups in stacks:
            for dedup in dedups:
                knobs(monkeypatch, air_skip=0, dedup=dedup)
                off = scan.run(rows=rows, layout=layout, both_fills=False)
                knobs(monkeypatch, air_skip=2, uniform=2, dedup=dedup)
                on = scan.run(rows=rows, layout=layout)
                same(off, on, f'{kind}, rows {rows}, layout {layout}, dedup {dedup}')
        if kind != 'air':
            assert lengths(off, n_ids)[:, 1:].max() > 0


def test_noisy_kernels_keep_the_air_rule(hip, monkeypatch):
    """The noisy SKIP forms were not built with the class rule: the new entry point hands them the air map, under its own knob."""
    scan = Scan(hip, 32, 64, 3).load(make_volume('rods+sphere', 64, 32, 3, 3))
    knobs(monkeypatch, air_skip=0)
    off = scan.run(noisy=True, both_fills=False)
    knobs(monkeypatch, air_skip=2, uniform=2)
    same(off, scan.run(noisy=True), 'noisy, maps forced')
    scan.ar['col_class'].inner.fill_(0x33)                             # every column "uniform in id 1": must not be looked at
    same(off, scan.run(noisy=True, n_uniform=[0, 32 * 32, 0, 0]), 'noisy, fabricated class map')
    scan.ar['col_air'].inner.fill_(0xFF)                               # ... and the air map is
    emptied = scan.run(noisy=True, n_uniform=[0, 32 * 32, 0, 0])
    assert not lengths(emptied, 3)[:, 1:].any()


@pytest.mark.parametrize('nz,n,n_ids', [(64, 32, 3), (512, 160, 4), (16, 160, 2)])
def test_the_map_is_what_the_kernel_reads(hip, monkeypatch, nz, n, n_ids):
    """A fabricated map that calls every column uniform in id 1 gives the bytes of projecting an all-water volume of that grid
    (every slab with a piece outside the grid stays listed and reads the volume - so the volume keeps water in its outermost
    columns); with the knob at 0 it gives the volume's own bytes."""
    scan = Scan(hip, n, nz, n_ids)
    knobs(monkeypatch, air_skip=0)
    water = scan.load(make_volume('water', nz, n, n_ids, 0)).run(both_fills=False)
    vol = make_volume('shuffled', nz, n, n_ids, 5)
    vol[:, 0, :] = vol[:, -1, :] = vol[:, :, 0] = vol[:, :, -1] = 1
    scan.load(vol)
    own = scan.run(both_fills=False)
    assert not np.array_equal(own['counts'], water['counts'])
    scan.ar['col_class'].inner.fill_(0x33)                             # ucount::class_of(1) in every nibble
    all_water = [0, n * n, 0, 0]
    same(own, scan.run(n_uniform=all_water), 'knob 0')
    knobs(monkeypatch, air_skip=2, uniform=2)
    same(water, scan.run(n_uniform=all_water), 'fabricated map, forced')
    knobs(monkeypatch)
    same(water, scan.run(n_uniform=all_water), 'fabricated map, auto: every column droppable')
    knobs(monkeypatch, uniform=0)
    same(own, scan.run(n_uniform=all_water), 'class map off: the (true) air map serves alone')


def test_auto_rule_and_knob(hip, monkeypatch):
    """DEXCT_P16_UNIFORM 0 / 1 / 2 and the share of droppable columns (one in eight, proj::use_class_map) on both sides, seen
    through a fabricated map: where the map is read the lengths are those of water, where it is not the volume's own."""
    n, nz, M = 32, 64, 3
    scan = Scan(hip, n, nz, M)
    knobs(monkeypatch, air_skip=0)
    water = scan.load(make_volume('water', nz, n, M, 0)).run(both_fills=False)
    vol = make_volume('one voxel off', nz, n, M, 7)
    vol[:, 0, :] = vol[:, -1, :] = vol[:, :, 0] = vol[:, :, -1] = 1
    own = scan.load(vol).run(both_fills=False)
    assert not np.array_equal(own['counts'], water['counts'])
    scan.ar['col_class'].inner.fill_(0x33)
    n_cols, first = n * n, n * n // 8
    reads = lambda got: np.array_equal(got['counts'], water['counts']) and np.array_equal(got['pathlen'], water['pathlen'])
    keeps = lambda got: np.array_equal(got['counts'], own['counts']) and np.array_equal(got['pathlen'], own['pathlen'])
    for air_map in (True, False):                                      # (the air map is optional to the new entry point)
        for split in ([first, 0, 0, 0], [0, first, 0, 0], [1, first - 3, 1, 1], [0, 0, 0, first]):
            below = list(split)
            below[int(np.argmax(split))] -= 1
            knobs(monkeypatch)
            assert reads(scan.run(n_uniform=split, air_map=air_map)), ('auto, at the share', split)
            assert keeps(scan.run(n_uniform=below, air_map=air_map)), ('auto, below the share', below)
            knobs(monkeypatch, uniform=1)
            assert reads(scan.run(n_uniform=split, air_map=air_map)) and keeps(scan.run(n_uniform=below, air_map=air_map))
            knobs(monkeypatch, uniform=2)
            assert reads(scan.run(n_uniform=below, air_map=air_map)) and reads(scan.run(n_uniform=[0, 0, 0, 0], air_map=air_map))
            knobs(monkeypatch, uniform=0)
            assert keeps(scan.run(n_uniform=[0, n_cols, 0, 0], air_map=air_map))
            knobs(monkeypatch, air_skip=0, uniform=2)
            assert keeps(scan.run(n_uniform=[0, n_cols, 0, 0], air_map=air_map))
    # counts the builder cannot have given are refused, and a class map without counts; nothing is launched
    knobs(monkeypatch)
    for bad in ([-1, 0, 0, 0], [0, n_cols + 1, 0, 0], [n_cols, 1, 0, 0], [2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62]):
        scan.ar.fill(0x5A, inner=('counts64', 'pathlen64', 'sino_log64'))
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        ar, pj = scan.ar, scan.pj
        rc = hip.dexct_siddon_project_packed_uniform(
            C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, M, scan.w.shape[1], 2, ptr(scan.mu), ptr(scan.w),
            ar['counts64'].ptr, ar['pathlen64'].ptr, 1, _native.log_out(ar['sino_log64'].ptr, list(scan.air)), None, None, None,
            ar['col_air'].ptr, scan.n_air, ar['col_class'].ptr, (C.c_int64 * 4)(*bad), sp())
        assert rc == -1, (bad, rc)
        rc = hip.dexct_siddon_project_packed_uniform(
            C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, M, scan.w.shape[1], 2, ptr(scan.mu), ptr(scan.w),
            ar['counts64'].ptr, ar['pathlen64'].ptr, 1, None, None, None, None, ar['col_air'].ptr, scan.n_air, ar['col_class'].ptr, None, sp())
        assert rc == -1, rc
        ar.check()
        assert all(np.all(ar[k].get() == 0x5A) for k in ('counts64', 'pathlen64', 'sino_log64'))
