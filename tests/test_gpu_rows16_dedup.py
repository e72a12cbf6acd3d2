"""rows16_kernel's list of distinct quads (DEXCT_DET_DEDUP, csrc/dedup_index.h) on the device: knob 1 against knob 0 byte for
byte - counts, log sinogram, path lengths - on guarded buffers (tests/guarded.py: no guard changes, no output depends on the
fill), and both against the byte-volume kernel (kernel 3).  Through both entry points of the packed projection: without the
air-column map, and with the map forced (the SKIP forms; the two-material kernel has the list in that form only).

Volumes are 32 x 32 in plane, 6 views x 10 channels; 256 / 512 / 1024 rows are 4 / 2 / 1 pairs per wave, 200 rows leave the last
lane of a pair with invalid rows, 2048 rows are two z-chunks.  A quad = a lane's four rows of one detection round; it is fresh
when a sum differs from the same row of the quad before it; F = fresh quads of a wave.  The test counts F itself from the path
lengths of the knob-0 run (``fresh_per_wave``) and asserts that every volume reaches the case it was made for:

  extruded      every pair is one fresh quad: F = pairs of the wave, one detection round
  sphere        an extruded object with one ellipsoid over part of the rows
  random        every slice random: F = every quad, the wave keeps its four rounds of rows
  levels:T      whole-plane slabs of two materials that change at T / pairs - 1 quad boundaries: F = T exactly (64: one round is
                full; 65 (where the pairs divide it, else the next count): one entry in the second; 128)
  lanes:K       the slabs change every K rows (16, 32): a fresh quad at row 0 of a lane that equals the lane's OWN last quad (16) or
                the NEXT lane's (32) - only the lane below is the right one to compare with
  air           nothing: every pair's sums are 0, the chords differ - the boundary between the channels of a wave must not merge
  rod           a thin water cylinder: all-air pairs beside water pairs (AirCache), DEXCT_DET_ABSENT on and off
and a table whose last row holds a NaN or an infinity (the absent-material short cut must stay off in the list rounds too)."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Arena, twice

pytestmark = pytest.mark.gpu

N_VIEWS, N_CHANNELS, N = 6, 10, 32


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


def lanes_per_pair(rows):
    lanes = -(-rows // 16)
    return 64 if lanes > 32 else (32 if lanes > 16 else 16)


def make_volume(kind, rows, n_ids, seed=0):
    """[rows][N][N] ids < n_ids (the projector pads the packed volume's copy to whole dwords of 16 slices with air)."""
    nz = rows
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:N, 0:N]
    c = 0.5 * (N - 1)
    vol = np.zeros((nz, N, N), dtype=np.uint8)
    other = 2 if n_ids > 2 else 0
    if kind in ('extruded', 'sphere'):
        vol[:, (x - c) ** 2 + (y - c) ** 2 <= (0.4 * N) ** 2] = 1
        for k in range(2, n_ids):                                   # rods of the other ids
            vol[:, (x - c - 3.0 * (k - 2.5) * 2) ** 2 + (y - c + 4) ** 2 <= 2.5 ** 2] = k
        if kind == 'sphere':
            z = np.arange(nz)[:, None, None]
            vol[((z - 0.45 * rows) / (rows / 7.0)) ** 2 + ((x - c + 3) / 7.0) ** 2 + ((y - c - 2) / 7.0) ** 2 <= 1.0] = n_ids - 1 if n_ids > 2 else 0
    elif kind == 'random':
        vol = rng.integers(0, n_ids, (nz, N, N), dtype=np.uint8)
    elif kind == 'rod':
        vol[:, (x - c) ** 2 + (y - c) ** 2 <= (0.15 * N) ** 2] = 1
    elif kind.startswith('levels:') or kind.startswith('lanes:'):
        quads = rows // 4
        if kind.startswith('lanes:'):
            step = int(kind.split(':')[1]) // 4
            changes = np.arange(step, quads, step)
        else:
            pairs, chunks = 64 // lanes_per_pair(rows), -(-rows // 1024)
            target = int(kind.split(':')[1])
            assert target % pairs == 0
            per_chunk = quads // chunks
            changes = []
            for k in range(chunks):              # a later chunk's first quad is fresh without a change: it gets one entry more
                n_ch = target // pairs - 1 + (1 if k else 0)
                changes += list(k * per_chunk + np.unique(np.linspace(1, per_chunk - 1, n_ch).astype(int)))
                assert len(changes) == sum(target // pairs - 1 + (1 if j else 0) for j in range(k + 1))
            changes = np.array(changes)
        level = np.zeros(quads, dtype=np.int64)
        level[changes] = 1
        level = np.cumsum(level) % 2
        vol[:rows] = np.where(np.repeat(level, 4) == 0, 1, other).astype(np.uint8)[:, None, None]
    else:
        assert kind == 'air'
    return vol


class Case:
    """One scan of ``rows`` rows on ``vol``: projectors (kernel 7 and 3) built on a volume that holds every id - so that the table
    rows are the ids - whose device volumes are then overwritten with ``vol``; the packed volume, its map and every output of the
    packed entry points live in guarded buffers."""

    def __init__(self, hip, vol, n_ids, rows):
        import dex_ct_sim_amd as dx
        from dex_ct_sim_amd import forward_project as fp, synthetic
        from dex_ct_sim_amd._device import ptr
        self.hip, self.M, self.rows = hip, n_ids, rows
        template = np.random.default_rng(1).integers(0, n_ids, vol.shape, dtype=np.uint8)
        template.reshape(-1)[:n_ids] = np.arange(n_ids)
        ph = dx.VoxelPhantom.from_array('dedup', template, materials(n_ids), dx=0.1, dy=0.1, dz=0.1)
        ct = dx.FanBeamGeometry(N_channels=N_CHANNELS, N_proj=N_VIEWS, gamma_fan=2 * np.arctan(0.5 * N * 0.1 / 60.0), SID=60.0, SDD=100.0,
                                N_rows=rows)
        specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
        for s_ in specs:
            s_.rescale_counts(1e-2)
        _, mu, w = fp.merged_tables(ct, ph, specs)
        self.pj = {k: fp.Projector(ct, ph, kernel=k) for k in (7, 3)}
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')
        self.mu, self.w, self.air = dev(self.pj[7].compact(mu)), dev(w), w.sum(axis=1)
        assert self.pj[7].use_packed and self.pj[7].n_mat == n_ids and tuple(self.mu.shape) == (n_ids, w.shape[1])
        for pj in self.pj.values():                                # the device layouts of ``vol`` in place of the template's
            nz = pj.geom.nz                                        # (the slices of the scan, padded with air to whole dwords)
            assert nz >= rows and pj.vol_yx.numel() == nz * N * N and pj.geom.z_first == 0
            pj.vol_yx.view(-1)[:vol.size].copy_(torch.from_numpy(vol.reshape(-1)).cuda())
            ok(hip.dexct_volume_layouts(ptr(pj.vol_yx), N, N, nz, ptr(pj.vol_xy), ptr(pj.vol_zf), sp()))
        nz = self.pj[7].geom.nz
        assert nz % 16 == 0
        self.rays = N_VIEWS * N_CHANNELS * rows
        ar = self.ar = Arena('cuda', SinceStart(hip))
        ar.alloc('vol_z2', nz * N * N // 4)
        ar.alloc('col_air', 4 * (N * N // 32))
        ar.alloc('n_air', 8)
        for name, b in (('counts', 8 * self.rays), ('sino_log', 8 * self.rays), ('pathlen', 4 * self.rays * n_ids)):
            ar.alloc(name, b)
        ar.fill(0xA5, inner=('vol_z2', 'col_air', 'n_air'))
        ok(hip.dexct_volume_pack2(ptr(self.pj[7].vol_zf), nz * N * N, ar['vol_z2'].ptr, sp()))
        ok(hip.dexct_volume_air_columns(ar['vol_z2'].ptr, N, N, nz, ar['col_air'].ptr, ar['n_air'].ptr, sp()))
        ar.check()
        self.n_air = int(ar['n_air'].get(np.uint64)[0])
        assert self.n_air == int((~vol.any(axis=0)).sum())

    def packed(self, skip, mu=None):
        """Both fills of one packed call; returns the host bytes of its outputs.  ``skip``: the entry point with the map."""
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        hip, ar, pj = self.hip, self.ar, self.pj[7]
        mu = self.mu if mu is None else mu

        def launch():
            args = (C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, self.M, self.w.shape[1], 2, ptr(mu), ptr(self.w),
                    ar['counts'].ptr, ar['pathlen'].ptr, 1, _native.log_out(ar['sino_log'].ptr, list(self.air)), None, None, None)
            if skip:
                ok(hip.dexct_siddon_project_packed_skip(*args, ar['col_air'].ptr, self.n_air, sp()))
            else:
                ok(hip.dexct_siddon_project_packed(*args, sp()))

        return twice(ar, launch, ['counts', 'sino_log', 'pathlen'])

    def on_and_off(self, monkeypatch, what, mu=None):
        """Knob 0, knob 1 and the default through both entry points (the map forced for the second): all the same bytes."""
        monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '2')
        monkeypatch.setenv('DEXCT_DET_DEDUP', '0')
        off = self.packed(False, mu)
        for skip in (False, True):
            for knob in ('0', '1', None):
                if knob is None:
                    monkeypatch.delenv('DEXCT_DET_DEDUP')
                else:
                    monkeypatch.setenv('DEXCT_DET_DEDUP', knob)
                got = self.packed(skip, mu)
                for n in off:
                    assert np.array_equal(off[n], got[n]), f'{what}: {n} differs (map={skip}, DEXCT_DET_DEDUP={knob})'
        return off

    def equals_byte_volume(self, got):
        c, pl, lg = self.pj[3].project_tables(self.mu, self.w, want_pathlen=True, layout=1, air=self.air)
        for name, t in (('counts', c), ('sino_log', lg), ('pathlen', pl)):
            assert np.array_equal(got[name].view(np.int32), t.contiguous().cpu().numpy().reshape(-1).view(np.int32)), \
                f'{name} differs from the byte-volume kernel'

    def fresh_per_wave(self, got):
        """[(live pairs of the wave, live quads, F)] from the path lengths of the materials 1.. (their sums x the pair's factor)."""
        rows, M = self.rows, self.M
        x = np.ascontiguousarray(got['pathlen'].view(np.int32).reshape(N_VIEWS, N_CHANNELS, rows, M)[..., 1:]).reshape(N_VIEWS, N_CHANNELS, rows // 4, -1)
        n_pairs = 64 // lanes_per_pair(rows)
        out = []
        for q0 in range(0, rows // 4, 256):                       # z-chunks of 1024 rows
            xs = x[:, :, q0:q0 + 256]
            f_pair = 1 + (xs[:, :, 1:] != xs[:, :, :-1]).any(axis=-1).sum(axis=-1)             # [view][channel]
            for c0 in range(0, N_CHANNELS, n_pairs):
                live = min(n_pairs, N_CHANNELS - c0)
                for f in f_pair[:, c0:c0 + n_pairs].sum(axis=1):
                    out.append((live, live * xs.shape[2], int(f)))
        return out


ROWS = [256, 512, 1024, 200, 2048]
NEXT_AFTER_64 = {256: 68, 512: 66, 1024: 65, 200: 68, 2048: 65}           # the smallest F above 64 that the pairs of a wave divide
KINDS = ['extruded', 'sphere', 'random', 'levels:64', 'levels:next', 'levels:128', 'lanes:16', 'lanes:32', 'air']
CASES = [(rows, kind, 3) for rows in ROWS for kind in KINDS] + \
        [(rows, kind, ids) for ids in (2, 4) for rows in (256, 1024) for kind in ('extruded', 'sphere', 'levels:64', 'levels:128', 'random')]


@pytest.mark.parametrize('rows,kind,n_ids', CASES)
def test_list_equals_rows(hip, monkeypatch, rows, kind, n_ids):
    if kind == 'levels:next':
        kind = f'levels:{NEXT_AFTER_64[rows]}'
    case = Case(hip, make_volume(kind, rows, n_ids, seed=rows + n_ids), n_ids, rows)
    off = case.on_and_off(monkeypatch, kind)
    case.equals_byte_volume(off)
    waves = case.fresh_per_wave(off)
    n_pairs = 64 // lanes_per_pair(rows)
    full = [f for live, _, f in waves if live == n_pairs]
    assert full
    if kind in ('extruded', 'air'):
        assert all(f == live for live, _, f in waves)
    elif kind == 'random':
        assert all(f == quads for _, quads, f in waves)
    elif kind.startswith('levels:'):
        target = int(kind.split(':')[1])
        want = {target} if rows <= 1024 else {target, target + 1}              # (the second z-chunk's own first quad)
        assert set(full) == want, sorted(set(full))
    elif kind.startswith('lanes:'):
        assert set(full) == {n_pairs * min(rows, 1024) // int(kind.split(':')[1])} or rows in (200, 2048), sorted(set(full))
    else:
        assert min(full) >= n_pairs and max(full) > 2 * n_pairs and max(full) < max(q for _, q, _ in waves)
    if kind == 'air':                 # neighbouring channels have equal sums and different chords: their counts differ
        c = off['counts'].view(np.float32).reshape(2, N_VIEWS, N_CHANNELS, rows)
        assert (c[:, :, 1:, 0] != c[:, :, :-1, 0]).mean() > 0.5


@pytest.mark.parametrize('rows,n_ids', [(256, 3), (512, 3), (200, 4), (1024, 4)])
@pytest.mark.parametrize('absent', ['0', '1'])
def test_air_pairs_beside_water_pairs(hip, monkeypatch, rows, n_ids, absent):
    monkeypatch.setenv('DEXCT_DET_ABSENT', absent)
    case = Case(hip, make_volume('rod', rows, n_ids), n_ids, rows)
    off = case.on_and_off(monkeypatch, 'rod')
    case.equals_byte_volume(off)
    pl = off['pathlen'].view(np.float32).reshape(N_VIEWS, N_CHANNELS, rows, n_ids)
    hit = (pl[..., 1] > 0).any(axis=2)
    assert hit.any() and not hit.all() and not pl[..., 2:].any()
    assert all(f == live for live, _, f in case.fresh_per_wave(off))


@pytest.mark.parametrize('n_ids', [3, 4])
@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_not_finite_entry_in_the_last_table_row(hip, monkeypatch, value, n_ids):
    """fma(NaN or inf, 0, pe) is NaN: the rows give NaN counts wherever the last row is looked at, so the list must too."""
    rows = 512
    case = Case(hip, make_volume('sphere', rows, n_ids - 1), n_ids, rows)
    mu = case.mu.clone()
    mu[n_ids - 1, mu.shape[1] // 2] = value
    for absent in ('0', '1'):
        monkeypatch.setenv('DEXCT_DET_ABSENT', absent)
        off = case.on_and_off(monkeypatch, f'{value} absent={absent}', mu=mu)
        assert np.isnan(off['counts'].view(np.float32)).any()
