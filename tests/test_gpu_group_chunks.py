"""The view-chunk loop of the material-group passes (Projector.project_tables): a projection that goes through in view chunks
(the scratch budget forces them) is the unchunked projection, bit for bit, on all three group entry points and at the option
combinations where one loop for all of them can go wrong: a view slice (the Philox counter follows the global view), every
further output through the chunks, the transpose and the fused log after them, the caller's own tensors, the sample drawn in
the detection pass (<= 2 spectra) and the variance through the chunks with dexct_add_noise once over the whole (3 spectra).

Shapes: the smallest that have more than one group (5 table rows: two groups), more than one chunk with a remainder
(6 views: 4 + 2, 2 + 2 + 2, six of 1; 5 views: 4 + 1, 2 + 2 + 1) and more than one row per lane group."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_VIEWS, N_CH, N_MAT, SEED = 6, 13, 5, 7
ROUTES = {'kernel4': dict(kernel=4, n_rows=8, cone=False, entry='dexct_siddon_project_grouped'),
          'kernel8': dict(kernel=8, n_rows=16, cone=False, entry='dexct_siddon_project_grouped_packed'),
          'cone2': dict(kernel=2, n_rows=5, cone=True, entry='dexct_cone_project_grouped')}
OPTIONS = ['view_slice', 'all_outputs', 'other_layout', 'callers_tensors', 'noisy_2_spectra', 'noisy_3_spectra']
_setups, _refs = {}, {}


def _setup(route):
    """Projector, device tables (mu, w, w2, air for 2 and for 3 spectra) of one route: built once for the module."""
    if route in _setups:
        return _setups[route]
    import dex_ct_sim_amd as dx
    from dex_ct_sim_amd import forward_project as fp, synthetic
    from dex_ct_sim_amd.system import AIR, BONE, WATER, Material
    r = ROUTES[route]
    nx, ny, nz = 22, 19, r['n_rows']
    dxv, dyv, dzv = 0.2, 0.25, 0.05
    rng = np.random.default_rng(5)
    vol = rng.integers(0, N_MAT, (nz, ny, nx), dtype=np.uint8)
    vol[rng.random(vol.shape) < 0.4] = 0
    mats = [AIR, WATER, BONE] + [Material(f'm{i}', 0.8 + 0.03 * i, 'H(11.2)O(88.8)') for i in range(3, N_MAT)]
    ph = dx.VoxelPhantom.from_array('chunks', vol, mats, dx=dxv, dy=dyv, dz=dzv)
    sid, sdd = 9.0, 16.0
    geo = dict(N_channels=N_CH, N_proj=N_VIEWS, gamma_fan=0.9, SID=sid, SDD=sdd, N_rows=r['n_rows'])
    if r['cone']:
        reach = 0.6 * sdd * dzv / (max(dxv, dyv) * np.sqrt(2.0))
        geo.update(cone=True, src_z=0.1 * reach, h_iso=float(reach / (0.5 * (r['n_rows'] - 1)) * sid / sdd * 0.9))
    ct = dx.FanBeamGeometry(**geo)
    pj = fp.Projector(ct, ph, kernel=r['kernel'])
    assert pj.n_mat == N_MAT
    assert (pj.cone_groups, pj.grouped, pj.grouped_packed) == (route == 'cone2', route == 'kernel4', route == 'kernel8')
    sp = [synthetic.kramers_spectrum(kvp) for kvp in (140, 80, 110)]
    for s_ in sp:
        s_.rescale_counts(1e-2)
    tabs = {}
    for n_spec in (2, 3):
        _, mu, w, w2 = fp.merged_tables(ct, ph, sp[:n_spec], with_variance=True)
        mu_d, w_d, w2_d = (torch.tensor(x, dtype=torch.float32, device='cuda').contiguous() for x in (pj.compact(mu), w, w2))
        tabs[n_spec] = (mu_d, w_d, w2_d, w.sum(axis=1))
    _setups[route] = (pj, tabs)
    return _setups[route]


def _calls(pj, tabs, option):
    """The project_tables calls of one option as (label, callable); a callable returns a tuple of tensors (None: an output
    that does not exist)."""
    mu2, w2s, v2, air2 = tabs[2]
    mu3, w3s, v3, air3 = tabs[3]
    other = 1 - pj.native_layout
    nR, nC = pj.ct.N_rows, pj.ct.N_channels

    def tup(x):
        return x if isinstance(x, tuple) else (x,)

    def own(layout, **kw):
        # out= and log_out= of the caller: the results are those tensors (prefilled: whatever the call leaves untouched shows)
        shape = (2, N_VIEWS, nR, nC) if layout == 0 else (2, N_VIEWS, nC, nR)
        out, log_out = (torch.full(shape, -1.0, dtype=torch.float32, device='cuda') for _ in range(2))
        c, lg = pj.project_tables(mu2, w2s, layout=layout, air=air2, out=out, log_out=log_out, **kw)
        assert c.data_ptr() == out.data_ptr() and lg.data_ptr() == log_out.data_ptr()
        return out, log_out

    if option == 'view_slice':
        return [('clean', lambda: tup(pj.project_tables(mu2, w2s, want_pathlen=True, air=air2, views=(1, 6)))),
                ('noisy', lambda: tup(pj.project_tables(mu2, w2s, w2_d=v2, seed=SEED, air=air2, views=(1, 6), want_variance=True))),
                ('noisy3', lambda: tup(pj.project_tables(mu3, w3s, w2_d=v3, seed=SEED, air=air3, views=(1, 6))))]
    if option == 'all_outputs':
        return [('clean', lambda: tup(pj.project_tables(mu2, w2s, want_pathlen=True, air=air2, want_variance=True))),
                ('noisy', lambda: tup(pj.project_tables(mu2, w2s, want_pathlen=True, air=air2, w2_d=v2, seed=SEED, want_variance=True))),
                ('noisy3', lambda: tup(pj.project_tables(mu3, w3s, want_pathlen=True, air=air3, w2_d=v3, seed=SEED, want_variance=True)))]
    if option == 'other_layout':
        return [('clean', lambda: tup(pj.project_tables(mu2, w2s, want_pathlen=True, air=air2, layout=other))),
                ('noisy', lambda: tup(pj.project_tables(mu2, w2s, air=air2, layout=other, w2_d=v2, seed=SEED, want_variance=True))),
                ('noisy3', lambda: tup(pj.project_tables(mu3, w3s, air=air3, layout=other, w2_d=v3, seed=SEED, views=(1, 6))))]
    if option == 'callers_tensors':
        return [('native', lambda: own(pj.native_layout)), ('other', lambda: own(other)),
                ('noisy', lambda: own(other, w2_d=v2, seed=SEED))]
    if option == 'noisy_2_spectra':
        return [('log', lambda: tup(pj.project_tables(mu2, w2s, w2_d=v2, seed=SEED, air=air2))),
                ('plain', lambda: tup(pj.project_tables(mu2, w2s, w2_d=v2, seed=SEED)))]
    assert option == 'noisy_3_spectra'
    return [('log', lambda: tup(pj.project_tables(mu3, w3s, w2_d=v3, seed=SEED, air=air3))),
            ('plain', lambda: tup(pj.project_tables(mu3, w3s, w2_d=v3, seed=SEED)))]


@pytest.mark.parametrize('option', OPTIONS)
@pytest.mark.parametrize('scratch_views', [4, 2, 0], ids=['chunks_of_4', 'chunks_of_2', 'below_one_view'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_chunked_projection_equals_the_unchunked_one(hip, route, scratch_views, option, monkeypatch):
    from dex_ct_sim_amd import forward_project as fp
    pj, tabs = _setup(route)
    per_view = N_MAT * pj.ct.N_rows * N_CH * 4
    entry = ROUTES[route]['entry']
    launches = []
    real = getattr(pj.lib, entry)
    first_view = 7 if route == 'cone2' else 2                 # where the entry point takes (view_begin, view_end)

    def counted(*args):
        launches.append((args[first_view], args[first_view + 1]))
        return real(*args)
    monkeypatch.setattr(pj.lib, entry, counted)
    if (route, option) not in _refs:                           # the unchunked results: once per route and option
        monkeypatch.setattr(fp, '_GROUP_SCRATCH_BYTES', 16 << 30)
        _refs[route, option] = {}
        for label, call in _calls(pj, tabs, option):
            launches.clear()
            _refs[route, option][label] = call()
            assert len(launches) == 1
    ref = _refs[route, option]
    # a budget below one view still goes through view by view
    monkeypatch.setattr(fp, '_GROUP_SCRATCH_BYTES', scratch_views * per_view if scratch_views else per_view - 1)
    n_chunk = max(1, scratch_views)
    for label, call in _calls(pj, tabs, option):
        launches.clear()
        got = call()
        v0, v1 = launches[0][0], launches[-1][1]
        want = [(a, min(a + n_chunk, v1)) for a in range(v0, v1, n_chunk)]
        assert launches == want and len(want) > 1, (label, launches)
        assert len(got) == len(ref[label])
        for k, (a, b) in enumerate(zip(got, ref[label])):
            assert (a is None and b is None) or torch.equal(a, b), (label, k)
    if option.startswith('noisy'):
        clean = pj.project_tables(*tabs[int(option[6])][:2])
        assert not torch.equal(clean, ref['plain'][0])       # the sample was drawn


@pytest.mark.parametrize('kind', ['packed_fan', 'cone'])
def test_noisy_project_is_project_tables_on_the_uploaded_tables(hip, kind):
    """Projector.project(noise=True) and project_tables fed by upload_tables' noisy form: one table construction, the same bits."""
    import dex_ct_sim_amd as dx
    from conftest import small_scan
    from dex_ct_sim_amd import forward_project as fp, synthetic
    if kind == 'packed_fan':
        ct, ph = small_scan(n=24, nz=16, n_views=5, n_channels=17, n_rows=16)
        pj = fp.Projector(ct, ph, kernel=7)
        assert pj.use_packed
    else:
        ct0, ph = small_scan(n=24, nz=6, n_views=5, n_channels=17, n_rows=5)
        ct = dx.FanBeamGeometry(N_channels=17, N_proj=5, gamma_fan=0.8230337, SID=60.0, SDD=100.0, h_iso=0.8, N_rows=5, cone=True,
                                eid=True, detector_file=ct0.detector_file)
        pj = fp.Projector(ct, ph)
        assert pj.cone
    sp = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
    for s_ in sp:
        s_.rescale_counts(1e-2)
    (counts, log), air = pj.project(sp, noise=True, seed=11, want_log=True)
    E, mu_d, w_d, air_t, w2_d = pj.upload_tables(sp, noise=True)
    c_t, l_t = pj.project_tables(mu_d, w_d, w2_d=w2_d, seed=11, air=air_t)
    assert np.array_equal(air, air_t) and torch.equal(c_t, counts) and torch.equal(l_t, log)
    assert not torch.equal(counts, pj.project(sp)[0])
    # the noise-free forms return what they returned: four values, float32 tables on the full grid
    E0, mu0, w0, air0 = pj.upload_tables(sp)
    assert np.array_equal(E0, E) and torch.equal(mu0, mu_d) and torch.equal(w0, w_d) and np.array_equal(air0, air)
    assert w2_d.dtype == torch.float32 and tuple(w2_d.shape) == tuple(w_d.shape)
