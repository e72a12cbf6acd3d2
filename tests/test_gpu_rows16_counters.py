"""The bit-sliced counters of rows16_kernel (csrc/sliced_count.h) on the device: the packed route (kernel 7, and kernel 8
for material groups) against the byte-volume row kernel (kernel 3; kernel 4 for groups), per-material path lengths and
counts bit for bit on every ray.  The shapes are the smallest that reach every path of the counters: a counter at 2047
(all 11 planes, the deepest ripple), slab counts around the trip sizes of the two sweeps (16 full slabs, 8 crossing
slabs: whole trips, one slab more, one less, lists that end in padding), the "both flags" plane of 4-id volumes, 4 and 2
pairs per wave with a dead pair in the last wave, and the noisy and material-group arms of the kernel template."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def projector(ct, ph, **kw):
    from dex_ct_sim_amd import forward_project as fp
    return fp.Projector(ct, ph, **kw)


def spectra():
    from dex_ct_sim_amd import synthetic
    return [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]


def materials(n_mat):
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    return ([AIR, WATER, BONE] + [Material(f'm{i}', 1.0 + 0.1 * i, 'H(11.2)O(88.8)') for i in range(3, n_mat)])[:n_mat]


def scan(vol, n_mat, n_views, n_channels, gamma_fan, dx_=0.1):
    import dex_ct_sim_amd as dx
    ph = dx.VoxelPhantom.from_array('counters', vol, materials(n_mat), dx=dx_, dy=0.1, dz=0.1)
    ct = dx.FanBeamGeometry(N_channels=n_channels, N_proj=n_views, gamma_fan=gamma_fan, SID=60.0, SDD=100.0, N_rows=vol.shape[0])
    return ct, ph


def assert_same(ct, ph, packed=7, byte=3, **kw):
    sp = spectra()
    (cb, pb), _ = projector(ct, ph, kernel=byte).project(sp, want_pathlen=True, **kw)
    pj = projector(ct, ph, kernel=packed)
    assert pj.use_packed or pj.grouped_packed
    (cp, pp), _ = pj.project(sp, want_pathlen=True, **kw)
    assert torch.equal(pp, pb)
    assert torch.equal(cp, cb)
    return pp


def test_counter_reaches_2047(hip):
    """2047 x 8 x 16 voxels of material 1 and a narrow fan: the views along x cross 2047 slabs of it, every hi[] plane
    gets set and the carry ripples through all of them; the views along y cross 8."""
    vol = np.ones((16, 8, 2047), dtype=np.uint8)
    ct, ph = scan(vol, 2, n_views=4, n_channels=24, gamma_fan=0.008, dx_=0.01)
    pl = assert_same(ct, ph)
    assert float(pl[..., 1].max()) >= 2047 * 0.01 * (1 - 1e-6)          # a ray saw material 1 in all 2047 slabs


@pytest.mark.parametrize('nx', [15, 16, 17, 24, 31, 32, 33, 40])
def test_slab_counts_around_the_trip_sizes(hip, nx):
    """40 views: 0 and 90 degrees (full slabs only), 45 and 27 degrees among the oblique ones (crossing slabs, mixed
    lists that end inside a trip)."""
    rng = np.random.default_rng(nx)
    vol = rng.integers(0, 3, (16, 8, nx), dtype=np.uint8)
    ct, ph = scan(vol, 3, n_views=40, n_channels=24, gamma_fan=0.07)
    assert_same(ct, ph)


@pytest.mark.parametrize('nx', [17, 40])
def test_four_ids_count_the_both_flags_plane(hip, nx):
    rng = np.random.default_rng(100 + nx)
    vol = rng.integers(0, 4, (16, 24, nx), dtype=np.uint8)
    ct, ph = scan(vol, 4, n_views=40, n_channels=24, gamma_fan=0.07)
    assert_same(ct, ph)


@pytest.mark.parametrize('n_rows', [16, 256, 512])
def test_pairs_per_wave_with_a_dead_pair(hip, n_rows):
    """16 and 256 rows: 16 lanes per pair, 4 pairs per wave; 512 rows: 32 lanes, 2 pairs.  21 channels leave the last
    wave of a view with one live pair."""
    rng = np.random.default_rng(n_rows)
    vol = rng.integers(0, 3, (n_rows, 33, 40), dtype=np.uint8)
    vol[rng.random(vol.shape) < 0.5] = 0
    ct, ph = scan(vol, 3, n_views=8, n_channels=21, gamma_fan=0.09)
    assert_same(ct, ph)


def test_noisy_arm(hip):
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 3, (256, 33, 40), dtype=np.uint8)
    ct, ph = scan(vol, 3, n_views=8, n_channels=21, gamma_fan=0.09)
    assert_same(ct, ph, noise=True, seed=7)


def test_material_group_arm(hip):
    rng = np.random.default_rng(6)
    vol = rng.integers(0, 7, (256, 33, 40), dtype=np.uint8)
    ct, ph = scan(vol, 7, n_views=8, n_channels=21, gamma_fan=0.09)
    assert_same(ct, ph, packed=8, byte=4)
