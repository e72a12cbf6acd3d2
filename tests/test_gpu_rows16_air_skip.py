"""rows16_kernel's two exact short cuts on the device, every output byte for byte (guarded buffers, tests/guarded.py).

(a) dexct_volume_air_columns: the air-column map against NumPy's ``~vol.any(axis=z)``, bit for bit, with its count - column
    counts that are no multiple of 32 or of a wave, columns whose only voxel sits at the first or the last z, byte and dword
    columns, an unaligned volume, more columns than the capped grid covers in one pass.
(b) dexct_siddon_project_packed_skip with the map forced on against dexct_siddon_project_packed: counts, log sinogram, path
    lengths and, for the noisy form, the sample and the variance; and both against the byte-volume kernel (kernel 3).  16, 32
    and 64 lanes per pair, a grid with more than 128 slabs per ray (a second staging pass), 12 views round the circle (both
    dominant axes, both signs of the step), 50 channels; a cylinder in air, an all-air volume, a volume without an air column,
    a checkerboard of air and material columns (every crossing slab mixes them); 2, 3 and 4 ids; staged and per-round stores.
(c) the detection of a wave whose rays all miss the last material (DEXCT_DET_ABSENT) against the full detection: a volume
    without the last id (also against the projection with one table row less), bone in some channel pairs only, 3 and 4 ids,
    the noisy form (which takes the short detection with 4 ids only: the three-material noisy kernel has no registers for it),
    and NaN / inf in the absent material's table row (the short cut must then stay off)."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Arena, twice

pytestmark = pytest.mark.gpu

N_VIEWS, N_CHANNELS, SEED = 12, 50, 9


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


def materials(n_mat):
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    return ([AIR, WATER, BONE] + [Material(f'm{i}', 1.0 + 0.1 * i, 'H(11.2)O(88.8)') for i in range(3, n_mat)])[:n_mat]


def make_volume(kind, nz, n, n_ids, seed):
    """[nz][n][n] ids 0 .. n_ids - 1.  'full': random ids, no all-air column; 'checker': the same with every second column (in x
    and in y) emptied; 'cylinder': id 1 within 0.4 n of the axis, discs of the other ids over part of z; 'air': nothing."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n]
    vol = np.zeros((nz, n, n), dtype=np.uint8)
    if kind == 'air':
        return vol
    if kind == 'cylinder':
        c = 0.5 * (n - 1)
        vol[:, (x - c) ** 2 + (y - c) ** 2 <= (0.4 * n) ** 2] = 1
        for k in range(2, n_ids):
            cx, cy = c + 0.2 * n * (k - 2.5), c - 0.1 * n
            vol[nz // 4:nz // 4 + max(1, nz // 3), (x - cx) ** 2 + (y - cy) ** 2 <= (0.08 * n) ** 2] = k
        return vol
    vol = rng.integers(0, n_ids, (nz, n, n), dtype=np.uint8)
    vol[rng.integers(0, nz, (n, n)), y, x] = rng.integers(1, n_ids, (n, n), dtype=np.uint8)      # no column without a voxel
    if kind == 'checker':
        vol[:, (x + y) % 2 == 0] = 0
    else:
        assert kind == 'full'
    return vol


def air_words(vol):
    """The map NumPy makes of a [nz][ny][nx] volume: (uint32 words, count)."""
    air = ~vol.any(axis=0).reshape(-1)
    bits = np.zeros(-(-air.size // 32) * 32, dtype=np.uint8)
    bits[:air.size] = air
    return np.packbits(bits, bitorder='little').view(np.uint32), int(air.sum())


def pack2(vol):
    """[nz][ny][nx] ids < 4 -> the bytes of vol_z2 [ny][nx][nz / 4] (NumPy restatement of dexct_volume_pack2)."""
    zf = np.ascontiguousarray(vol.transpose(1, 2, 0)).reshape(vol.shape[1], vol.shape[2], -1, 4).astype(np.uint8)
    return (zf[..., 0] | (zf[..., 1] << 2) | (zf[..., 2] << 4) | (zf[..., 3] << 6)).astype(np.uint8)


# ---- (a) the map builder ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nx,ny,nz,offset', [(1, 1, 4, 0), (5, 7, 4, 0), (33, 31, 16, 0), (33, 31, 16, 1), (64, 64, 64, 0), (21, 19, 24, 0),
                                             (300, 7, 8, 2), (1025, 1027, 4, 0)])
def test_air_column_map(hip, nx, ny, nz, offset):
    """1025 x 1027 columns are 4099 more than the 4096 workgroups of 256 take in one pass (csrc: kColAirMaxBlocks)."""
    rng = np.random.default_rng(nx * 1000 + nz)
    vol = rng.integers(0, 4, (nz, ny, nx), dtype=np.uint8)
    vol[:, rng.random((ny, nx)) < 0.5] = 0
    lone = np.flatnonzero(~vol.any(axis=0).reshape(-1))
    if lone.size >= 2:                                         # a column whose only voxel is the first z, one with the last z
        vol[0, lone[0] // nx, lone[0] % nx] = 1
        vol[nz - 1, lone[-1] // nx, lone[-1] % nx] = 3
    want, n_want = air_words(vol)
    assert (nx * ny) % 32 or (nx, ny) == (64, 64)
    ar = arena(hip)
    ar.alloc('vol_z2', nx * ny * nz // 4, offset=offset).put(pack2(vol))
    ar.alloc('col_air', 4 * want.size)
    ar.alloc('n_air', 8)
    got = twice(ar, lambda: ok(hip.dexct_volume_air_columns(ar['vol_z2'].ptr, nx, ny, nz, ar['col_air'].ptr, ar['n_air'].ptr, sp())),
                ['col_air', 'n_air'])
    assert np.array_equal(got['col_air'].view(np.uint32), want)
    assert int(got['n_air'].view(np.uint64)[0]) == n_want
    if lone.size >= 2:
        w = got['col_air'].view(np.uint32)
        assert not (w[lone[0] // 32] >> (lone[0] % 32)) & 1 and not (w[lone[-1] // 32] >> (lone[-1] % 32)) & 1


def test_air_column_map_arguments(hip):
    ar = arena(hip)
    for n, b in (('v', 64), ('m', 64), ('c', 8)):
        ar.alloc(n, b)
    call = lambda v='v', m='m', c='c', nx=4, ny=4, nz=16: hip.dexct_volume_air_columns(
        ar[v].ptr if v else None, nx, ny, nz, ar[m].ptr if m else None, ar[c].ptr if c else None, sp())
    ar.fill(0x5A, inner=('v', 'm', 'c'))
    assert call(v=None) == -1 and call(m=None) == -1 and call(c=None) == -1
    assert call(nx=0) == -1 and call(ny=-1) == -1 and call(nz=0) == -1 and call(nz=18) == -1
    assert call(nx=65536, ny=32768) == -2
    ar.check()
    assert all(np.all(ar[n].get() == 0x5A) for n in ('m', 'c'))


# ---- (b), (c): the packed projection on guarded buffers --------------------------------------------------------------------------

class Case:
    """One scan on a volume of ``n_ids`` ids: projectors (kernel 7 and 3) built on a volume that holds every id - so that the
    table rows are the ids - whose device volumes are then overwritten with ``vol``; the packed volume, its map and every output
    of the packed entry points live in guarded buffers."""

    def __init__(self, hip, vol, n_ids, byte_kernel=True):
        import dex_ct_sim_amd as dx
        from dex_ct_sim_amd import forward_project as fp, synthetic
        from dex_ct_sim_amd._device import ptr
        self.hip, self.vol, self.M = hip, vol, n_ids
        nz, n, _ = vol.shape
        self.nz, self.n = nz, n
        template = make_volume('full', nz, n, n_ids, 1)
        ph = dx.VoxelPhantom.from_array('air-skip', template, materials(n_ids), dx=0.1, dy=0.1, dz=0.1)
        ct = dx.FanBeamGeometry(N_channels=N_CHANNELS, N_proj=N_VIEWS, gamma_fan=2 * np.arctan(0.5 * n * 0.1 / 60.0), SID=60.0, SDD=100.0,
                                N_rows=nz)
        self.ct = ct
        specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
        for s_ in specs:
            s_.rescale_counts(1e-2)
        _, mu, w, w2 = fp.merged_tables(ct, ph, specs, with_variance=True)
        self.pj = {k: fp.Projector(ct, ph, kernel=k) for k in ((7, 3) if byte_kernel else (7,))}
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')
        self.mu, self.w, self.w2, self.air = dev(self.pj[7].compact(mu)), dev(w), dev(w2), w.sum(axis=1)
        assert self.pj[7].use_packed and self.pj[7].n_mat == n_ids and tuple(self.mu.shape) == (n_ids, w.shape[1])
        for pj in self.pj.values():                                # the device layouts of ``vol`` in place of the template's
            pj.vol_yx.view(-1).copy_(torch.from_numpy(vol.reshape(-1)).cuda())
            ok(hip.dexct_volume_layouts(ptr(pj.vol_yx), n, n, nz, ptr(pj.vol_xy), ptr(pj.vol_zf), sp()))
        self.rays = N_VIEWS * N_CHANNELS * nz
        ar = self.ar = arena(hip)
        words, self.n_air = air_words(vol)
        ar.alloc('vol_z2', vol.size // 4)
        ar.alloc('col_air', 4 * words.size)
        ar.alloc('n_air', 8)
        for name, b in (('counts', 8 * self.rays), ('sino_log', 8 * self.rays), ('variance', 8 * self.rays), ('pathlen', 4 * self.rays * n_ids)):
            ar.alloc(name, b)
        ar.fill(0xA5, inner=('vol_z2', 'col_air', 'n_air'))
        ok(hip.dexct_volume_pack2(ptr(self.pj[7].vol_zf), vol.size, ar['vol_z2'].ptr, sp()))
        ok(hip.dexct_volume_air_columns(ar['vol_z2'].ptr, n, n, nz, ar['col_air'].ptr, ar['n_air'].ptr, sp()))
        ar.check()
        assert np.array_equal(ar['vol_z2'].get().reshape(n, n, nz // 4), pack2(vol))
        assert np.array_equal(ar['col_air'].get(np.uint32), words) and int(ar['n_air'].get(np.uint64)[0]) == self.n_air

    def packed(self, *, skip, noisy=False, M=None, mu=None, n_air=None):
        """Both fills of one packed call; returns the host bytes of its outputs.  ``skip``: the new entry point with the map."""
        from dex_ct_sim_amd import _native
        from dex_ct_sim_amd._device import ptr
        hip, ar, pj = self.hip, self.ar, self.pj[7]
        M = self.M if M is None else M
        mu = self.mu if mu is None else mu
        pl = 'pathlen' if M == self.M else f'pathlen{M}'               # (a call with fewer table rows writes fewer lengths)
        if pl not in ar.buffers:
            ar.alloc(pl, 4 * self.rays * M)
        outs = ['counts', 'sino_log', pl] + (['variance'] if noisy else [])

        def launch():
            args = (C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, M, self.w.shape[1], 2, ptr(mu), ptr(self.w),
                    ar['counts'].ptr, ar[pl].ptr, 1, _native.log_out(ar['sino_log'].ptr, list(self.air)),
                    ptr(self.w2) if noisy else None, ar['variance'].ptr if noisy else None, _native.noise(SEED) if noisy else None)
            if skip:
                ok(hip.dexct_siddon_project_packed_skip(*args, ar['col_air'].ptr, self.n_air if n_air is None else n_air, sp()))
            else:
                ok(hip.dexct_siddon_project_packed(*args, sp()))

        got = twice(ar, launch, outs)
        got['pathlen'] = got.pop(pl)
        return got

    def byte_volume(self, noisy):
        """The same outputs from the byte-volume row kernel, in the packed kernel's own layout."""
        pj = self.pj[3]
        if noisy:
            c, lg, var = pj.project_tables(self.mu, self.w, layout=1, w2_d=self.w2, seed=SEED, air=self.air, want_variance=True)
            return dict(counts=c, sino_log=lg, variance=var)
        c, pl, lg = pj.project_tables(self.mu, self.w, want_pathlen=True, layout=1, air=self.air)
        return dict(counts=c, sino_log=lg, pathlen=pl)


def same(a, b, what):
    for n in a:
        assert n in b and np.array_equal(a[n], b[n]), f'{what}: {n} differs'


SHAPES = [(64, 64), (512, 64), (1024, 64), (16, 160)]                       # (nz = rows, n): 16 / 32 / 64 lanes per pair; two passes
KINDS = ['cylinder', 'air', 'full', 'checker']
CASES = [(nz, n, kind, 3) for nz, n in SHAPES for kind in KINDS] + [(nz, 64, kind, ids) for ids in (2, 4) for nz in (64, 512)
                                                                    for kind in ('cylinder', 'checker')]


@pytest.mark.parametrize('nz,n,kind,n_ids', CASES)
def test_map_on_equals_map_off(hip, monkeypatch, nz, n, kind, n_ids):
    case = Case(hip, make_volume(kind, nz, n, n_ids, 17 * nz + n), n_ids)
    assert (case.n_air == n * n) == (kind == 'air') and (case.n_air == 0) == (kind == 'full')
    for staged in ('1', '0'):
        monkeypatch.setenv('DEXCT_P16_STAGED', staged)
        for noisy in (False, True):
            monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '0')
            off = case.packed(skip=False, noisy=noisy)
            same(off, case.packed(skip=True, noisy=noisy), 'knob 0')
            monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '2')
            on = case.packed(skip=True, noisy=noisy)
            same(off, on, f'map forced, staged={staged} noisy={noisy}')
            monkeypatch.delenv('DEXCT_P16_AIR_SKIP')
            same(off, case.packed(skip=True, noisy=noisy), 'default knob')
            if staged == '1':
                ref = case.byte_volume(noisy)
                for name, t in ref.items():
                    assert np.array_equal(on[name].view(np.float32).view(np.int32), t.contiguous().cpu().numpy().reshape(-1).view(np.int32)), \
                        f'{name} differs from the byte-volume kernel (noisy={noisy})'
    if kind != 'air':
        assert case.byte_volume(False)['pathlen'][..., 1:].max() > 0


def test_the_map_is_what_the_kernel_looks_at(hip, monkeypatch):
    """A map that calls EVERY column air empties the lists: with the knob at 2, or at 1 with a count at the share of
    proj::use_air_map, the path lengths of the materials come out 0; with the knob at 0, or at 1 with a count below the share,
    the map is not looked at.  (So the byte identities above are identities of two different traversals.)"""
    case = Case(hip, make_volume('full', 64, 64, 3, 5), 3, byte_kernel=False)
    case.ar['col_air'].inner.fill_(0xFF)
    n_cols = 64 * 64
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '0')
    off = case.packed(skip=False)
    lengths = lambda got: got['pathlen'].view(np.float32).reshape(-1, 3)
    assert lengths(off)[:, 1:].max() > 0
    same(off, case.packed(skip=True, n_air=n_cols), 'knob 0')
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '2')
    forced = case.packed(skip=True, n_air=0)
    assert not lengths(forced)[:, 1:].any() and not np.array_equal(forced['counts'], off['counts'])
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '1')
    same(off, case.packed(skip=True, n_air=0), 'auto, no air columns')
    same(forced, case.packed(skip=True, n_air=n_cols), 'auto, all air columns')
    # DEXCT_P16_MINW: a value that names no form of its own (7) runs the default forms and takes the map; 5 has no form with it
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '2')
    monkeypatch.setenv('DEXCT_P16_MINW', '7')
    same(forced, case.packed(skip=True, n_air=0), 'knob 2, MINW 7')
    monkeypatch.setenv('DEXCT_P16_MINW', '5')
    same(off, case.packed(skip=True, n_air=0), 'knob 2, MINW 5')
    monkeypatch.delenv('DEXCT_P16_MINW')
    monkeypatch.setenv('DEXCT_P16_AIR_SKIP', '1')
    # a count the builder cannot have given is refused
    from dex_ct_sim_amd import _native
    from dex_ct_sim_amd._device import ptr
    pj, ar = case.pj[7], case.ar
    bad = lambda n_air: hip.dexct_siddon_project_packed_skip(
        C.byref(pj.geom), pj.plan.data_ptr(), 0, N_VIEWS, ar['vol_z2'].ptr, 3, case.w.shape[1], 2, ptr(case.mu), ptr(case.w), ar['counts'].ptr,
        None, 1, None, None, None, None, ar['col_air'].ptr, n_air, sp())
    assert bad(-1) == -1 and bad(n_cols + 1) == -1 and bad(n_cols) == 0
    ar.check()


# ---- (c) the absent last material ------------------------------------------------------------------------------------------------

def on_and_off(case, monkeypatch, **kw):
    monkeypatch.setenv('DEXCT_DET_ABSENT', '0')
    off = case.packed(skip=False, **kw)
    monkeypatch.setenv('DEXCT_DET_ABSENT', '1')
    return case.packed(skip=False, **kw), off


@pytest.mark.parametrize('n_ids', [3, 4])
def test_volume_without_the_last_id(hip, monkeypatch, n_ids):
    """Every wave runs the detection of n_ids - 1 materials: the same counts as the full detection, and as the projection with
    the first n_ids - 1 table rows (its lengths are the first n_ids - 1 of each ray)."""
    vol = make_volume('cylinder', 64, 64, n_ids - 1, 3)
    assert vol.max() == n_ids - 2
    case = Case(hip, vol, n_ids, byte_kernel=False)
    for noisy in (False, True):
        on, off = on_and_off(case, monkeypatch, noisy=noisy)
        same(off, on, f'noisy={noisy}')
        fewer = case.packed(skip=False, noisy=noisy, M=n_ids - 1, mu=case.mu[:n_ids - 1].contiguous())
        for name in ('counts', 'sino_log') + (('variance',) if noisy else ()):
            assert np.array_equal(on[name], fewer[name]), name
        pl = on['pathlen'].view(np.float32).reshape(-1, n_ids)
        assert not pl[:, -1].any() and np.array_equal(pl[:, :-1], fewer['pathlen'].view(np.float32).reshape(-1, n_ids - 1))


@pytest.mark.parametrize('nz,n_ids', [(64, 3), (512, 3), (64, 4), (1024, 4)])
def test_last_material_in_some_pairs_only(hip, monkeypatch, nz, n_ids):
    """The cylinder's disc of the last id lies in the fan of some channels and over a third of the rows: some waves and rounds
    take the short detection, some the full one."""
    case = Case(hip, make_volume('cylinder', nz, 64, n_ids, 4), n_ids, byte_kernel=False)
    for staged in ('1', '0'):
        monkeypatch.setenv('DEXCT_P16_STAGED', staged)
        for noisy in (False, True):
            on, off = on_and_off(case, monkeypatch, noisy=noisy)
            same(off, on, f'staged={staged} noisy={noisy}')
    pl = off['pathlen'].view(np.float32).reshape(N_VIEWS, N_CHANNELS, nz, n_ids)[..., -1]
    hit = (pl > 0).any(axis=2)
    assert hit.any() and not hit.all() and not (pl > 0).any(axis=(0, 1)).all()


@pytest.mark.parametrize('n_ids', [3, 4])
@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_not_finite_row_of_the_absent_material(hip, monkeypatch, value, n_ids):
    """fma(NaN or inf, 0, pe) is NaN: the full detection gives NaN counts wherever it runs, so the short one must not run."""
    case = Case(hip, make_volume('cylinder', 64, 64, n_ids - 1, 3), n_ids, byte_kernel=False)
    mu = case.mu.clone()
    mu[n_ids - 1, mu.shape[1] // 2] = value
    for noisy in (False, True):
        on, off = on_and_off(case, monkeypatch, noisy=noisy, mu=mu)
        same(off, on, f'noisy={noisy}')
        assert np.isnan(off['variance' if noisy else 'counts'].view(np.float32)).any()      # (the sample is clamped from below)
