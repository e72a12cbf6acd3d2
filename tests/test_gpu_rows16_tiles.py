"""rows16_kernel dismisses runs of slabs in uniform tiles before it classifies slabs one by one: the tile map and the projection
that uses it, on the device, byte for byte (guarded buffers, tests/guarded.py).  The reference everywhere is the same library with
the tile map off (DEXCT_P16_TILES=0: the kernels of the class map alone), not a tolerance.

(a) dexct_volume_tile_classes against a NumPy restatement of the map (both copies, the outside tiles, the spare word) and of the
    per-id counts, on every volume of (b), and its argument refusals.
(b) dexct_siddon_project_packed_tiles with DEXCT_P16_TILES = 1, 2 and 0: counts, log sinogram and path lengths agree byte for byte,
    and with them the old entry point and the new one with a null map.  Grids 16^2, 24^2, 100 x 52 (partial edge tiles on both
    axes) and 256^2; nz = rows = 16, 64 (4 pairs per wave), 512 (2 pairs), 1024 (1 pair); ten views - 0, 45 (slope 1) and 90
    degrees, and odd angles - of a fan wider than the grid, so that channels miss it and graze its corners; 2 - 4 ids; the volumes
    of VOLUMES.  A host census of the kernel's own plan (the rule of csrc/tile_class.h restated in NumPy) says what each case
    exercises - dismissed runs, surviving runs, more than one pass - and the case asserts it.
(c) the tile map is what the kernel reads: a fabricated map that calls every tile uniform in id 1 gives the lengths of a water
    volume wherever a ray stays inside the grid; with the knob at 0 the volume's own bytes; the auto rule on both sides of its
    share, and counts the builder cannot have given."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from guarded import Arena, twice

pytestmark = pytest.mark.gpu

VIEW_DEGREES = [0.0, 45.0, 90.0, 17.3, 61.9, 135.0, 180.0, 225.0, 283.7, 270.0]
N_VIEWS, N_CHANNELS, K = len(VIEW_DEGREES), 24, 8


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


def materials(n_mat):
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    return ([AIR, WATER, BONE] + [Material(f'm{i}', 1.0 + 0.1 * i, 'H(11.2)O(88.8)') for i in range(3, n_mat)])[:n_mat]


# ---- NumPy restatements ---------------------------------------------------------------------------------------------------------

def column_classes(vol):
    """[nz][ny][nx] -> [ny][nx]: 0 mixed, 1 | id << 1 uniform in id."""
    uniform = (vol == vol[0]).all(axis=0)
    return np.where(uniform, 1 | (vol[0].astype(np.uint32) << 1), 0).astype(np.uint32)


def tile_classes(cls):
    """[ny][nx] column classes -> [ty][tx] tile classes: all 64 columns uniform in one id; a tile past the grid in air only."""
    ny, nx = cls.shape
    ty, tx = -(-ny // K), -(-nx // K)
    pad = np.ones((ty * K, tx * K), dtype=np.uint32)                   # outside the grid: air
    pad[:ny, :nx] = cls
    t = pad.reshape(ty, K, tx, K).transpose(0, 2, 1, 3).reshape(ty, tx, K * K)
    same = (t == t[..., :1]).all(axis=-1) & ((t[..., 0] & 1) == 1)
    return np.where(same, t[..., 0], 0).astype(np.uint32)


def pack_nibbles(rows):
    nib = np.concatenate([np.concatenate([[1], r, [1]]) for r in rows]).astype(np.uint32)      # an air tile at either end of a row
    nib = np.concatenate([nib, np.zeros(-nib.size % 8, dtype=np.uint32)])
    return np.bitwise_or.reduce(nib.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32)), axis=1).astype(np.uint32)


def tile_words(tiles):
    """The map of include/dexct_p16_tiles.h: copy 0 (rows of tx, ty fastest), copy 1 (rows of ty, tx fastest), a spare word."""
    return np.concatenate([pack_nibbles(list(tiles.T)), pack_nibbles(list(tiles)), np.zeros(1, dtype=np.uint32)])


def census(plan, cls, tiles):
    """What the kernel's two phases meet on this plan: dismissed runs, surviving runs, the most surviving runs of one ray,
    dismissed runs in a non-air id, rays that cross the grid and have every run dismissed (`emptied`: nothing of them reaches a list),
    the most runs of one ray, whether a run of index 32 or more survives (the upper half of the kernel's mask), and the fewest slabs
    of a ray that touches the grid (a ray that grazes a corner).  The rule of csrc/tile_class.h: run R of a ray holds its slabs i = 8 R .. 8 R + 7; its pieces lie between
    the cells of its first slab and behind its last; it is dismissed when the tiles of that range - an air tile outside the grid -
    are at most three and all uniform in one id."""
    ny, nx = cls.shape
    guard = lambda m: np.pad(m, ((0, 0), (1, 1)), constant_values=1)
    maps = (guard(tiles.T), guard(tiles))                               # axis 0: i = x, j = y; axis 1: i = y, j = x
    dismissed = surviving = most = non_air = emptied = most_runs = 0
    high_alive, fewest = False, 1 << 30
    for p in plan:
        n_slabs, i_first, V0, SV, axis = int(p['n_slabs']), int(p['i_first']), int(p['V0']), int(p['SV']), int(p['flags']) & 1
        if n_slabs <= 0:
            continue
        m = maps[axis]
        tj = m.shape[1] - 2
        alive = 0
        fewest = min(fewest, n_slabs)
        most_runs = max(most_runs, ((i_first + n_slabs - 1) >> 3) - (i_first >> 3) + 1)
        for R in range(i_first >> 3, ((i_first + n_slabs - 1) >> 3) + 1):
            i_lo, i_hi = max(8 * R, i_first), min(8 * R + 7, i_first + n_slabs - 1)
            j0, j1 = (V0 + i_lo * SV) >> 40, (V0 + (i_hi + 1) * SV) >> 40
            J_lo, J_hi = (min(max(j >> 3, -1), tj) for j in (min(j0, j1), max(j0, j1)))
            e = set(int(x) for x in m[R, J_lo + 1:J_hi + 2])
            if J_hi - J_lo <= 2 and len(e) == 1 and (min(e) & 1):
                dismissed += 1
                non_air += min(e) != 1
            else:
                alive += 1
                high_alive = high_alive or R - (i_first >> 3) >= 32
        surviving += alive
        emptied += alive == 0
        most = max(most, alive)
    return types.SimpleNamespace(dismissed=dismissed, surviving=surviving, most=most, non_air=non_air, emptied=emptied, most_runs=most_runs,
                                 high_alive=high_alive, fewest=fewest)


# ---- volumes ----------------------------------------------------------------------------------------------------------------------

VOLUMES = ['air', 'one id', 'disc+sphere', 'touches the edge', 'checkerboard', 'one mixed column', 'mixed throughout']


def make_volume(kind, nz, ny, nx, n_ids, seed):
    """[nz][ny][nx] ids 0 .. n_ids - 1.
    'air': nothing; 'one id': the last id to the grid's edge - every run inside the grid is dismissed, the lists hold only the
    slabs with a piece outside; 'disc+sphere': an extruded disc of id 1 with a sphere of the last id; 'touches the edge': a bar
    of id 1 from one edge of the grid to the other, off the tile grid; 'checkerboard': tiles in the ids 1 and n_ids - 1 (or air)
    by turns - crossings between uniform tiles of different ids must stay listed; 'one mixed column': id 1 everywhere but for one
    voxel; 'mixed throughout': a random id in every voxel."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    vol = np.zeros((nz, ny, nx), dtype=np.uint8)
    if kind == 'one id':
        vol[:] = n_ids - 1
    elif kind == 'disc+sphere':
        cy, cx, r = 0.5 * (ny - 1), 0.5 * (nx - 1), 0.4 * min(nx, ny)
        vol[:, (x - cx) ** 2 + (y - cy) ** 2 <= r * r] = 1
        rs, zc = min(0.2 * min(nx, ny), 0.45 * nz), 0.5 * (nz - 1)
        z = np.arange(nz)[:, None, None]
        vol[(x - cx - 0.1 * nx) ** 2 + (y - cy) ** 2 + (z - zc) ** 2 <= rs * rs] = n_ids - 1
    elif kind == 'touches the edge':
        vol[:, ny // 3 + 1:ny // 3 + 1 + max(3, ny // 4), :] = 1
        vol[:, :, nx - 3:] = n_ids - 1
    elif kind == 'checkerboard':
        board = ((y // K + x // K) % 2).astype(np.uint8)
        vol[:] = np.where(board == 1, 1, (n_ids - 1) if n_ids > 2 else 0)
    elif kind == 'one mixed column':
        vol[:] = 1
        vol[nz // 2, ny // 2 + 1, nx // 2 - 1] = 0
    elif kind == 'mixed throughout':
        vol = rng.integers(0, n_ids, (nz, ny, nx), dtype=np.uint8)
    else:
        assert kind == 'air'
    return vol


class Scan:
    """One fan scan of an [nz][ny][nx] grid with ``n_ids`` ids, its fan a half wider than the grid's diagonal (a strip's: two and
    a half times its short side).  The projector
    (kernel 7) is built on a volume that holds every id, so that the table rows are the ids; ``load`` then puts a volume, its
    packing and its three maps into guarded buffers, and ``run`` calls an entry point on them."""

    def __init__(self, hip, nx, ny, nz, n_ids):
        import dex_ct_sim_amd as dx
        from dex_ct_sim_amd import forward_project as fp, synthetic
        self.hip, self.nx, self.ny, self.nz, self.M = hip, nx, ny, nz, n_ids
        template = np.random.default_rng(1).integers(0, n_ids, (nz, ny, nx), dtype=np.uint8)
        ph = dx.VoxelPhantom.from_array('tiles', template, materials(n_ids), dx=0.1, dy=0.1, dz=0.1)
        # (a strip - 512 x 16 - gets a fan two and a half times its SHORT side at the isocentre: the channels then stand under two cells apart, so
        # that at the views along the strip the middle channels run its whole length and the outer ones miss even its near end)
        extent = np.hypot(nx, ny) if max(nx, ny) <= 4 * min(nx, ny) else 5.0 / 3.0 * min(nx, ny)
        ct = dx.FanBeamGeometry(N_channels=N_CHANNELS, N_proj=N_VIEWS, gamma_fan=2 * np.arctan(0.75 * extent * 0.1 / 60.0),
                                SID=60.0, SDD=100.0, N_rows=nz)
        ct.thetas = np.deg2rad(np.array(VIEW_DEGREES))
        specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
        _, mu, w = fp.merged_tables(ct, ph, specs)
        self.pj = fp.Projector(ct, ph, kernel=7)
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')
        self.mu, self.w, self.air = dev(self.pj.compact(mu)), dev(w), w.sum(axis=1)
        assert self.pj.use_packed and self.pj.n_mat == n_ids and self.pj.geom.nz == nz and self.pj.geom.z_first == 0
        self.plan = self.pj.plan_host()
        assert len(self.plan) == N_VIEWS * N_CHANNELS
        self.map_words = int(hip.dexct_volume_tile_map_words(nx, ny))
        ar = self.ar = Arena('cuda', SinceStart(hip))
        ar.alloc('vol_z2', nz * ny * nx // 4)
        ar.alloc('col_class', 4 * (-(-nx * ny // 8)))
        ar.alloc('n_uniform', 32)
        ar.alloc('tile_map', 4 * self.map_words)
        ar.alloc('n_tiles', 32)
        rays = N_VIEWS * N_CHANNELS * nz
        for k, b in (('counts', 8 * rays), ('sino_log', 8 * rays), ('pathlen', 4 * rays * n_ids)):
            ar.alloc(k, b)

    def load(self, vol):
        from dex_ct_sim_amd._device import ptr
        hip, ar, nx, ny, nz = self.hip, self.ar, self.nx, self.ny, self.nz
        zf = torch.from_numpy(np.ascontiguousarray(vol.transpose(1, 2, 0))).cuda()         # [ny][nx][nz], what vol_zf holds
        ar.fill(0xA5, inner=('vol_z2', 'col_class', 'n_uniform'))
        ok(hip.dexct_volume_pack2(ptr(zf), vol.size, ar['vol_z2'].ptr, sp()))
        ok(hip.dexct_volume_column_classes(ar['vol_z2'].ptr, nx, ny, nz, ar['col_class'].ptr, ar['n_uniform'].ptr, sp()))
        ar.check()
        self.n_uniform = [int(k) for k in ar['n_uniform'].get(np.uint64)]
        # (a) the builder, on guards and contents of both fills
        got = twice(ar, lambda: ok(hip.dexct_volume_tile_classes(ar['col_class'].ptr, nx, ny, ar['tile_map'].ptr, ar['n_tiles'].ptr, sp())),
                    ['tile_map', 'n_tiles'])
        self.cls = column_classes(vol)
        self.tiles = tile_classes(self.cls)
        want = tile_words(self.tiles)
        assert want.size == self.map_words
        assert np.array_equal(got['tile_map'].view(np.uint32), want)
        self.n_tiles = [int((self.tiles == (1 | k << 1)).sum()) for k in range(4)]
        assert got['n_tiles'].view(np.uint64).tolist() == self.n_tiles
        return self

    def run(self, *, entry='tiles', tile_map=True, n_tiles=None, both_fills=True, rc=0):
        """One call (both fills of the guards and outputs, or one); returns the host bytes of counts, sino_log and pathlen."""
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        hip, ar, pj = self.hip, self.ar, self.pj
        outs = ['counts', 'sino_log', 'pathlen']
        col_counts = (C.c_int64 * 4)(*self.n_uniform)
        tile_counts = (C.c_int64 * 4)(*(self.n_tiles if n_tiles is None else n_tiles))

        def launch():
            head = (C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, self.M, self.w.shape[1], 2, ptr(self.mu), ptr(self.w),
                    ar['counts'].ptr, ar['pathlen'].ptr, 1, _native.log_out(ar['sino_log'].ptr, list(self.air)), None, None, None,
                    None, 0, ar['col_class'].ptr, col_counts)
            if entry == 'tiles':
                got = hip.dexct_siddon_project_packed_tiles(*head, ar['tile_map'].ptr if tile_map else None, tile_counts if tile_map else None, sp())
            else:
                got = hip.dexct_siddon_project_packed_uniform(*head, sp())
            assert got == rc, got

        got = twice(ar, launch, outs, fills=(0x00, 0xFF) if both_fills else (0x00,))
        return {k: got[k] for k in outs}


def same(a, b, what):
    for n in a:
        assert n in b and np.array_equal(a[n], b[n]), f'{what}: {n} differs'


def knobs(monkeypatch, tiles=None, uniform=2):
    """The class map forced on (the tile map rides on it) unless told otherwise; every other knob at its default."""
    for name, v in (('DEXCT_P16_TILES', tiles), ('DEXCT_P16_UNIFORM', uniform), ('DEXCT_P16_AIR_SKIP', 2 if uniform else None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


# grid, depth, ids, volumes.  Every volume on the small grids; the grid with partial tiles on both axes at every lane count; 256^2
# where a ray has more surviving runs than one pass takes; 512 x 16 and 16 x 512, whose longest rays fill the kernel's window of 64
# runs.  (Depth and grid do not meet in the code: lanes and pairs go by the
# rows, runs and passes by the slabs.)
CASES = [(16, 16, 16, 2, VOLUMES), (16, 16, 64, 3, VOLUMES),
         (24, 24, 64, 4, VOLUMES), (24, 24, 512, 3, ['disc+sphere', 'checkerboard', 'one mixed column']),
         (100, 52, 16, 3, VOLUMES), (100, 52, 64, 2, ['disc+sphere', 'touches the edge', 'checkerboard']),
         (100, 52, 1024, 4, ['disc+sphere', 'touches the edge', 'one id']), (52, 100, 512, 3, ['touches the edge', 'checkerboard', 'one mixed column']),
         (256, 256, 16, 3, ['mixed throughout', 'disc+sphere', 'checkerboard']), (256, 256, 64, 4, ['mixed throughout', 'one id']),
         # the longest ray the tile forms take, 64 runs, at 16, 32 and 64 lanes per pair and along either axis
         (512, 16, 16, 3, ['mixed throughout', 'touches the edge', 'one id']), (512, 16, 512, 3, ['mixed throughout', 'checkerboard']),
         (16, 512, 1024, 2, ['mixed throughout', 'touches the edge'])]


@pytest.mark.parametrize('nx,ny,nz,n_ids,volumes', CASES)
def test_tile_map_on_equals_tile_map_off(hip, monkeypatch, nx, ny, nz, n_ids, volumes):
    scan = Scan(hip, nx, ny, nz, n_ids)
    missing = sum(1 for p in scan.plan if int(p['n_slabs']) == 0)
    assert missing > 0, 'the fan is wider than the grid: channels miss it'
    for kind in volumes:
        scan.load(make_volume(kind, nz, ny, nx, n_ids, 7 * nz + nx + n_ids))
        c = census(scan.plan, scan.cls, scan.tiles)
        # channels that graze a corner: a ray that touches the grid with at most a quarter of the slabs of its longest side
        assert 0 < c.fewest <= max(nx, ny) // 4, c.fewest
        # what the volume was made for
        if kind == 'air':
            assert c.dismissed > 0 and c.surviving == 0 and scan.n_tiles == [scan.tiles.size, 0, 0, 0]      # (partial tiles vouch for air)
        if kind == 'one id':
            # every tile inside the grid, and no partial one; the runs that leave the grid survive (air outside against the id) ...
            assert c.non_air > 0 and c.surviving > 0 and scan.n_tiles[0] == 0 and scan.n_tiles[n_ids - 1] == (nx // K) * (ny // K)
            # ... and where no tile is partial, rays that enter and leave through the faces across their slab axis have EVERY run
            # dismissed: their lists stay empty and all their length comes out of the per-pair count
            assert c.emptied > 0 or nx % K or ny % K
        if kind in ('disc+sphere', 'touches the edge', 'one mixed column'):
            assert c.surviving > 0 and (c.dismissed > 0 or sum(scan.n_tiles) == 0)      # (a disc in 3 x 3 tiles leaves none uniform)
            assert c.dismissed > 0 or min(nx, ny) < 4 * K
        if kind == 'checkerboard':
            assert c.surviving > 0 and c.dismissed > 0 and scan.n_tiles[1] > 0
        if kind == 'mixed throughout':
            assert c.dismissed == 0 and c.surviving > 0
            assert c.most > 16 or max(nx, ny) < 200                       # more surviving runs than one pass takes: several passes
        if max(nx, ny) == 512:
            # the whole window: a ray of 64 runs (run trips up to t0 = 48 at 16 lanes per pair), and survivors in the mask's upper half
            assert c.most_runs == 64 and (c.high_alive or kind != 'mixed throughout')
            assert c.most == 64 or kind != 'mixed throughout'             # four full passes
        knobs(monkeypatch, tiles=0)
        off = scan.run(both_fills=False)
        for mode in (2, 1):
            knobs(monkeypatch, tiles=mode)
            same(off, scan.run(), f'{kind}: DEXCT_P16_TILES={mode}')
        same(off, scan.run(entry='uniform', both_fills=False), f'{kind}: the old entry point')
        same(off, scan.run(tile_map=False, both_fills=False), f'{kind}: null tile map')
        lengths = off['pathlen'].view(np.float32).reshape(-1, n_ids)
        assert (lengths[:, 1:].max() > 0) == (kind != 'air')
        # the tile forms against the library without any map: the untouched kernels
        if kind in ('disc+sphere', 'mixed throughout'):
            knobs(monkeypatch, tiles=None, uniform=None)
            monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '0')
            same(off, scan.run(both_fills=False), f'{kind}: no map at all')


def test_the_tile_map_is_what_the_kernel_reads(hip, monkeypatch):
    """A fabricated tile map that calls every tile uniform in id 1 dismisses every run whose cells stay inside the grid: the rays
    then carry the lengths of an all-water volume wherever the class map - the volume's own, all mixed - is not asked.  With the
    knob at 0, below the share of the auto rule or with a null map the volume's own bytes come out; impossible counts are refused."""
    nx = ny = 32
    nz, M = 64, 3
    scan = Scan(hip, nx, ny, nz, M)
    knobs(monkeypatch, tiles=0)
    water = scan.load(make_volume('one id', nz, ny, nx, 2, 0)).run(both_fills=False)
    own = scan.load(make_volume('mixed throughout', nz, ny, nx, M, 3)).run(both_fills=False)
    assert scan.n_tiles == [0, 0, 0, 0] and not np.array_equal(own['pathlen'], water['pathlen'])
    scan.ar['tile_map'].inner.fill_(0x33)                                 # ucount::class_of(1) in every nibble
    n_t = (nx // K) * (ny // K)
    all_water, first = [0, n_t, 0, 0], -(-n_t // 2)                      # proj::use_tile_map: from one uniform tile in two on
    reads = lambda got: not np.array_equal(got['pathlen'], own['pathlen'])
    keeps = lambda got: np.array_equal(got['pathlen'], own['pathlen']) and np.array_equal(got['counts'], own['counts'])
    knobs(monkeypatch, tiles=2)
    forced = scan.run(n_tiles=all_water)
    assert reads(forced)
    # every run is dismissed in water (the fabricated outside tiles say water too): nothing of the volume's bone is seen
    ol, fl = (g['pathlen'].view(np.float32).reshape(-1, M) for g in (own, forced))
    assert ol[:, 2].max() > 0 and (fl[:, 2] == 0).all() and fl[:, 1].max() >= water['pathlen'].view(np.float32).reshape(-1, M)[:, 1].max()
    assert keeps(scan.run(n_tiles=all_water, tile_map=False))
    knobs(monkeypatch, tiles=0)
    assert keeps(scan.run(n_tiles=all_water))
    for mode in (None, 1):
        knobs(monkeypatch, tiles=mode)
        assert reads(scan.run(n_tiles=[0, first, 0, 0])) and reads(scan.run(n_tiles=[1, first - 2, 0, 1]))
        assert keeps(scan.run(n_tiles=[0, first - 1, 0, 0])) and keeps(scan.run(n_tiles=[0, 0, 0, 0]))
    knobs(monkeypatch, tiles=2, uniform=0)                                # without the class map there is no tile form
    assert keeps(scan.run(n_tiles=all_water))
    knobs(monkeypatch, tiles=2)
    for bad in ([-1, 0, 0, 0], [0, n_t + 1, 0, 0], [n_t, 1, 0, 0], [2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62]):
        scan.ar.fill(0x5A, inner=('counts', 'pathlen', 'sino_log'))
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        ar, pj = scan.ar, scan.pj
        rc = hip.dexct_siddon_project_packed_tiles(
            C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, M, scan.w.shape[1], 2, ptr(scan.mu), ptr(scan.w),
            ar['counts'].ptr, ar['pathlen'].ptr, 1, _native.log_out(ar['sino_log'].ptr, list(scan.air)), None, None, None, None, 0,
            ar['col_class'].ptr, (C.c_int64 * 4)(*scan.n_uniform), ar['tile_map'].ptr, (C.c_int64 * 4)(*bad), sp())
        assert rc == -1, (bad, rc)
        ar.check()
        assert all(np.all(ar[k].get() == 0x5A) for k in ('counts', 'pathlen', 'sino_log'))


@pytest.mark.parametrize('nx,ny', [(520, 16), (16, 520)])
def test_grids_past_one_window_keep_the_slab_rule(hip, monkeypatch, nx, ny):
    """The tile forms hold one window of 64 runs (tiles::grid_fits: grids up to 512 x 512).  On a grid past that the tile map is
    never read, whatever the knob says: a fabricated map that calls every tile water changes nothing, and every setting gives the
    bytes of knob 0.  (On 512 x 16 the same fabricated map IS read: the limit is where the code says.)"""
    nz, M = 16, 3
    for gx, gy, reads_it in ((nx, ny, False), (512 if nx > ny else 16, 16 if nx > ny else 512, True)):
        scan = Scan(hip, gx, gy, nz, M)
        knobs(monkeypatch, tiles=0)
        own = scan.load(make_volume('mixed throughout', nz, gy, gx, M, 11)).run(both_fills=False)
        for mode in (2, 1):
            knobs(monkeypatch, tiles=mode)
            same(own, scan.run(), f'{gx} x {gy}: DEXCT_P16_TILES={mode}')
        scan.ar['tile_map'].inner.fill_(0x33)
        knobs(monkeypatch, tiles=2)
        got = scan.run(n_tiles=[0, scan.tiles.size, 0, 0])
        assert np.array_equal(got['pathlen'], own['pathlen']) == (not reads_it), (gx, gy)


def test_tile_map_builder_arguments(hip):
    ar = Arena('cuda', SinceStart(hip))
    for n, b in (('c', 64), ('m', 64), ('n', 32)):
        ar.alloc(n, b)
    call = lambda c='c', m='m', n='n', nx=16, ny=16: hip.dexct_volume_tile_classes(
        ar[c].ptr if c else None, nx, ny, ar[m].ptr if m else None, ar[n].ptr if n else None, sp())
    ar.fill(0x5A, inner=('c', 'm', 'n'))
    assert call(c=None) == -1 and call(m=None) == -1 and call(n=None) == -1
    assert call(nx=0) == -1 and call(ny=-1) == -1 and call(nx=65536, ny=32768) == -2
    assert hip.dexct_volume_tile_map_words(0, 4) == 0 and hip.dexct_volume_tile_map_words(65536, 32768) == 0
    assert hip.dexct_volume_tile_map_words(16, 16) == 2 * 1 + 1 and hip.dexct_volume_tile_map_words(100, 52) == 15 + 14 + 1
    ar.check()
    assert all(np.all(ar[n].get() == 0x5A) for n in ('m', 'n'))           # a refused call launches nothing
