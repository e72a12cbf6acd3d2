"""tests/noise_refs.py on the CPU: the reference is right (published Philox known answers, moments and independence of the four
normals, the edge words), every comparison of the GPU module bites (a float32 model of the kernels passes it, the same model
with one small structural error does not), and the caps on what the comparisons cannot decide hold for exactly the inputs of
tests/test_gpu_noise.py."""
import numpy as np
import pytest

import noise_refs as nr

F32, F64, U64 = np.float32, np.float64, np.uint64


# ---- the reference itself ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """The three known-answer vectors published with Random123 (kat_vectors, philox4x32 10), scalar and as arrays."""
    assert tuple(int(x) for x in nr.philox4x32_10(*ctr, *key)) == want
    got = nr.philox4x32_10(*[np.full((2, 3), x) for x in ctr], *key)
    assert all(np.all(g == w) and g.shape == (2, 3) for g, w in zip(got, want))


def test_moments_and_independence_of_the_reference_normals():
    v, r, c = np.meshgrid(np.arange(64), np.arange(16), np.arange(128), indexing='ij')
    for seed in nr.SEEDS:
        z = nr.pixel_normals_ref(v, r, c, seed).reshape(4, -1)
        assert z.shape[1] == 131072
        assert np.all(np.abs(z.mean(axis=1)) < 0.01), z.mean(axis=1)
        assert np.all(np.abs(z.std(axis=1) - 1.0) < 0.01), z.std(axis=1)
        corr = np.corrcoef(z)
        assert np.all(np.abs(corr[~np.eye(4, dtype=bool)]) < 0.01), corr
    other = nr.pixel_normals_ref(v, r, c, nr.SEEDS[0]).reshape(4, -1)
    assert abs(np.corrcoef(z[0], other[0])[0, 1]) < 0.01                      # and between the seeds


def test_edge_words():
    """w = 0xFFFFFFFF on the radius word: (float)w + 1 = 2^32, u1 = 1, z = 0 whatever the angle.  On the angle word: u2 = 1, the
    same normals as u2 = 0.  w = 0 on the radius word: the largest radius, sqrt(64 ln 2)."""
    for angle in (0, 12345, 0x80000000, 0xFFFFFFFF):
        cs, sn = nr.box_muller(0xFFFFFFFF, angle)
        assert cs == 0.0 and sn == 0.0
    assert nr.unit_pair(0xFFFFFFFF, 0xFFFFFFFF) == (1.0, 1.0)
    for radius in (0, 7, 0x12345678, 0xFFFFFF00):
        a, b = nr.box_muller(radius, 0xFFFFFFFF), nr.box_muller(radius, 0)
        assert np.allclose(a, b, rtol=0.0, atol=1e-14)
    assert nr.box_muller(0, 0)[0] == np.sqrt(64.0 * np.log(2.0))
    assert nr.unit_pair(0, 0) == (2.0 ** -32, 0.0)


def test_decode_is_a_bijection_in_both_layouts():
    V, R, Ch = 3, 5, 7
    for layout in (0, 1):
        v, r, c = nr.decode((V, R, Ch), layout)
        assert v.max() == V - 1 and r.max() == R - 1 and c.max() == Ch - 1
        assert len(set(zip(v.tolist(), r.tolist(), c.tolist()))) == V * R * Ch
    v, r, c = nr.decode((V, R, Ch), 0)
    assert (v[36], r[36], c[36]) == (1, 0, 1)
    v, r, c = nr.decode((V, R, Ch), 1)
    assert (v[36], r[36], c[36]) == (1, 1, 0)


# ---- a float32 model of the kernels, with switches for the ways a sampler goes subtly wrong ------------------------------------

def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded once more (to float32)."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def model_decode(shape, layout, mut):
    v, r, c = nr.decode(shape, layout)
    return (v, c, r) if ('row_channel' in mut and layout == 1) else (v, r, c)


def model_normals(v, r, c, seed, mut):
    lo, hi = nr.seed_words(seed)
    w = nr.philox4x32_10(v, r, c, 0, lo, hi)
    if 'word_pairs' in mut:
        w = (w[2], w[3], w[0], w[1])
    z = []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        u1 = (a.astype(F32) + F32(1.0)) * nr.TWO_M32
        u2 = b.astype(F32) * nr.TWO_M32
        rad = np.sqrt(F32(-1.38629436111989061883) * np.log2(u1))
        ang = F32(2.0 * np.pi) * u2
        cs, sn = (np.sin(ang), np.cos(ang)) if 'sin_cos' in mut else (np.cos(ang), np.sin(ang))
        z += [rad * cs, rad * sn]
    if 'same_normal' in mut:
        z[1] = z[0]
    assert all(x.dtype == F32 for x in z)
    return np.stack(z)


def model_add_noise(counts, variance, shape, layout, view_offset, seed, mut=()):
    v, r, c = model_decode(shape, layout, mut)
    off = 0 if 'view_offset' in mut else view_offset
    z = model_normals(v + off, r, c, seed, mut)[:counts.shape[0]]
    sd = np.sqrt(np.fmax(variance, F32(0.0)))
    return np.fmax(fma32(sd, z, counts), F32(nr.FLOOR))


def model_poisson(p, mut=()):
    S, E, M = p['n_spectra'], p['n_energies'], p['n_materials']
    shape = (p['n_views'], p['n_rows'], p['n_channels'])
    v, r, c = model_decode(shape, p['layout'], mut)
    off = 0 if 'view_offset' in mut else p['view_offset']
    L = p['pathlen'].reshape(-1, M) * F32(1.44269504088896340736)
    pe = np.zeros((v.size, E), F32)
    for m in range(M):
        pe = fma32(p['mu'][m][None, :], L[:, m][:, None], pe)
    lam = p['photons'][:, None, :] * np.exp2(-pe)[None]
    gain = p['gain']
    if 'gain_on_lambda' in mut:
        lam = lam * gain[None, None, :]
    assert lam.dtype == F32
    s_word = 0 if 'no_spectrum_word' in mut else (np.arange(S, dtype=np.int64)[:, None, None] << 24)
    e_word = 0 if 'no_energy_word' in mut else np.arange(E, dtype=np.int64)[None, None, :]
    lo, hi = nr.seed_words(p['seed'])
    w = nr.philox4x32_10((v + off)[None, :, None], r[None, :, None], c[None, :, None], np.zeros((S, 1, E), np.int64) | s_word | e_word,
                         lo, hi if 'no_key_xor' in mut else hi ^ 0x9E3779B9)
    live = lam > 0
    inv = live & ((lam <= F32(30.0)) if 'branch_le_30' in mut else (lam < F32(30.0)))
    nrm = live & ~inv
    draw = np.zeros(lam.shape, F32)
    u = (w[0].astype(F64) * 4294967296.0 + w[1].astype(F64) + 0.5) * (1.0 / 18446744073709551616.0)
    draw[inv] = nr._inversion(lam[inv].astype(F64), u[inv], 0.0)
    u1 = (w[0].astype(F32) + F32(1.0)) * nr.TWO_M32
    u2 = (w[1] if 'r1_for_r2' in mut else w[2]).astype(F32) * nr.TWO_M32
    z = np.sqrt(F32(-2.0) * np.log(u1)) * np.cos(F32(np.pi) * (F32(2.0) * u2))
    draw[nrm] = np.fmax(np.floor(fma32(np.sqrt(lam[nrm]), z[nrm], lam[nrm]) + F32(0.5)), F32(0.0))
    acc = np.zeros(lam.shape[:2], F32)
    for e in range(E):
        acc = fma32(F32(1.0) if 'gain_on_lambda' in mut else gain[e], draw[:, :, e], acc)
    return np.fmax(acc, F32(nr.FLOOR))


GAUSS_MUTANTS = ['sin_cos', 'word_pairs', 'same_normal', 'view_offset', 'row_channel']
POISSON_MUTANTS = ['view_offset', 'row_channel', 'no_energy_word', 'no_spectrum_word', 'no_key_xor', 'r1_for_r2', 'gain_on_lambda']
GAUSS_CASE = dict(shape=(5, 4, 67), layout=1, view_offset=17, seed=nr.SEEDS[1])


def gauss_checks(mut):
    """The three value comparisons of dexct_add_noise in the GPU module, applied to the model: recover z, physical values,
    clipping.  [bool, bool, bool]."""
    k, S = GAUSS_CASE, 4
    out = []
    cnt, var = nr.constant_inputs(S, k['shape'], 16.0, 1.0)
    v, r, c = nr.decode(k['shape'], k['layout'])
    z_ref = nr.pixel_normals_ref(v + k['view_offset'], r, c, k['seed'])
    out.append(nr.z_within(model_add_noise(cnt, var, mut=mut, **k).astype(F64) - 16.0, z_ref))
    cnt, var = nr.physical_inputs(S, k['shape'])
    ref, bound = nr.add_noise_ref(cnt, var, **k)
    out.append(nr.within(model_add_noise(cnt, var, mut=mut, **k), ref, bound))
    cnt, var = nr.constant_inputs(S, k['shape'], 1.0, 25.0)
    _, bound, raw = nr.add_noise_ref(cnt, var, raw=True, **k)
    out.append(nr.clip_ok(model_add_noise(cnt, var, mut=mut, **k), raw, bound))
    return out


def test_gaussian_comparisons_accept_the_float32_model():
    assert gauss_checks(()) == [True, True, True]


@pytest.mark.parametrize('mutant', GAUSS_MUTANTS)
def test_gaussian_comparisons_reject(mutant):
    assert gauss_checks((mutant,)) == [False, False, False]


def test_degenerate_variances_and_nan_mean_in_the_reference():
    shape = (3, 5, 7)
    cnt, _ = nr.physical_inputs(2, shape)
    for bad in (0.0, -1.0, np.nan):
        ref, bound = nr.add_noise_ref(cnt, np.full(cnt.shape, bad, F32), shape, 0, 0, 1)
        assert np.array_equal(ref, cnt.astype(F64)) and np.all(bound == 4.0 * nr.U * cnt)
    ref, _ = nr.add_noise_ref(np.full(cnt.shape, np.nan, F32), cnt, shape, 0, 0, 1)
    assert np.all(ref == nr.FLOOR)


_refs = {}


def poisson_ref(name, problem):
    if name not in _refs:
        _refs[name] = nr.poisson_detect_ref(**problem)
    return _refs[name]


def decode_problems():
    out = {f'table{i}': nr.unattenuated_problem(t, layout=1, view_offset=17, seed=nr.SEEDS[1]) for i, t in enumerate(nr.DECODE_TABLES)}
    out['boundary'] = nr.unattenuated_problem(nr.BOUNDARY_TABLE, layout=1, view_offset=17, seed=nr.SEEDS[1])
    return out


def poisson_checks(mut):
    """poisson_within on the attenuated problem (17 materials, layout 1); poisson_within and decode_ok on the two decode tables
    and on the boundary table.  A list of booleans."""
    out = []
    p = nr.attenuated_problem(17, 1)
    lo, hi, _, _ = poisson_ref('att17', p)
    out.append(nr.poisson_within(model_poisson(p, mut), lo, hi, p['n_energies']))
    for name, p in decode_problems().items():
        lo, hi, _, detail = poisson_ref(name, p)
        sig = model_poisson(p, mut)
        out += [nr.poisson_within(sig, lo, hi, p['n_energies']), nr.decode_ok(sig, detail, p['gain'])]
    return out


def test_poisson_comparisons_accept_the_float32_model():
    assert all(poisson_checks(()))
    for n_mat in nr.ATTENUATED_MATERIALS:
        for layout in (0, 1):
            p = nr.attenuated_problem(n_mat, layout)
            lo, hi, _, _ = poisson_ref(('att', n_mat, layout), p)
            assert nr.poisson_within(model_poisson(p), lo, hi, p['n_energies']), (n_mat, layout)


@pytest.mark.parametrize('mutant', POISSON_MUTANTS)
def test_poisson_comparisons_reject(mutant):
    assert not any(poisson_checks((mutant,)))


def test_the_branch_is_decided_on_the_right_side_of_30():
    """lambda = 30.0 exactly takes the rounded normal, the float32 below it the inversion: a sampler that switches at
    lambda <= 30 is rejected by both comparisons; the reference's window is a single integer in every inversion bin and in
    nearly every rounded-normal one."""
    p = decode_problems()['boundary']
    lo, hi, ambiguous, detail = poisson_ref('boundary', p)
    at30 = np.broadcast_to((p['photons'] == F32(30.0))[:, None, :], detail['normal'].shape)
    assert np.array_equal(detail['normal'], at30) and at30.any() and not at30.all()
    assert np.all(detail['k_lo'][~at30] == detail['k_hi'][~at30]) and ambiguous < 1e-3
    sig = model_poisson(p, ('branch_le_30',))
    assert not nr.poisson_within(sig, lo, hi, 3) and not nr.decode_ok(sig, detail, p['gain'])
    sig = model_poisson(p)
    assert nr.poisson_within(sig, lo, hi, 3) and nr.decode_ok(sig, detail, p['gain'])


def test_dark_bins_give_the_floor():
    p = nr.unattenuated_problem(nr.DARK_TABLE)
    lo, hi, _, detail = nr.poisson_detect_ref(**p)
    assert np.all(lo == nr.FLOOR) and np.all(hi == nr.FLOOR) and not detail['live'].any()
    assert np.all(model_poisson(p) == F32(nr.FLOOR))


# ---- the caps, for exactly the inputs of tests/test_gpu_noise.py ---------------------------------------------------------------

def test_ambiguous_bin_cap():
    """At most 1 % of the bins of any Poisson input of the GPU module have a window of more than one integer; the attenuated
    problems span lambda = 1e-3 .. 3e3 and fill both branches; in the decode problems every inversion bin is decided."""
    for n_mat in nr.ATTENUATED_MATERIALS:
        for layout in (0, 1):
            p = nr.attenuated_problem(n_mat, layout)
            _, _, ambiguous, d = poisson_ref(('att', n_mat, layout), p)
            assert ambiguous <= nr.AMBIGUOUS_CAP, (n_mat, layout, ambiguous)
            lam = d['lam'][d['live']]
            assert lam.size > 150000 and lam.min() < 1e-3 and lam.max() == 3e3
            assert 0.2 < np.mean(lam >= 30.0) < 0.8 and np.mean((lam > 1e-3) & (lam < 30.0)) > 0.2
    for name, p in decode_problems().items():
        _, _, ambiguous, d = poisson_ref(name, p)
        assert ambiguous <= nr.AMBIGUOUS_CAP, (name, ambiguous)
        assert np.all((d['k_lo'] == d['k_hi'])[~d['normal']]) and d['k_hi'].max() < 256
    normal = [poisson_ref(f'table{i}', decode_problems()[f'table{i}'])[3]['normal'][:, 0, :] for i in (0, 1)]
    assert np.all(normal[0] ^ normal[1])                                      # every (spectrum, energy) takes both branches


def test_clipping_cap():
    """mean = 1, variance = 25: over every case of the GPU module at most 0.1 % of the pixels lie within their bound of zero (the
    expectation is pdf(-0.2) * 2 * 1e-3 = 0.078 %), and both other classes are well filled."""
    n = between = below = 0
    for shape in nr.SHAPES:
        for S, layout, off, seed in nr.add_noise_cases(shape):
            cnt, var = nr.constant_inputs(S, shape, 1.0, 25.0)
            _, bound, raw = nr.add_noise_ref(cnt, var, shape, layout, off, seed, raw=True)
            lo, _, mid = nr.clip_classes(raw, bound)
            n, between, below = n + raw.size, between + int(mid.sum()), below + int(lo.sum())
    assert between <= nr.CLIP_CAP * n, (between, n)
    assert 0.40 < below / n < 0.44                                           # P(z < -0.2) = 0.4207


def test_reference_normals_of_the_independence_case_are_uncorrelated():
    """The GPU module asks |correlation| < 0.05 of the recovered normals of the (9, 4, 131) shape; the reference's own stay
    below 0.045 there, so that a device within 1e-3 of it cannot cross the line."""
    shape = nr.SHAPES[-1]
    for layout in (0, 1):
        v, r, c = nr.decode(shape, layout)
        for off in nr.VIEW_OFFSETS:
            for seed in nr.SEEDS:
                corr = np.corrcoef(nr.pixel_normals_ref(v + off, r, c, seed))
                assert np.all(np.abs(corr[~np.eye(4, dtype=bool)]) < 0.045), (layout, off, seed, corr)
