"""rows16_kernel: slabs in z-uniform columns counted once per pair (profiles/rows16_uniform.md).  The projection launch of the
benchmark scan (512^3, 1000 x 800 x 512, dual spectrum) on the volumes of tools/probes/p16_dedup.py.  DEXCT_ROOT names the tree
whose package is loaded (default: this one); the census needs nothing this change adds and runs on any tree with the packed route.

    python tools/probes/p16_uniform.py census        # list lengths and sweep trips per wave: today's rule against the new one
    python tools/probes/p16_uniform.py ab [rounds]   # DEXCT_P16_AIR_SKIP = 0 / DEXCT_P16_UNIFORM = 0 (air only) / defaults, ms per
                                                     # launch, results compared bit for bit
    python tools/probes/p16_uniform.py launch        # one launch per knob setting (run under a counter or a trace pass)

The census restates the classification of the SKIP loop against the kernel's own plan (dexct_fan_plan, read back): slab s of a ray
has the pieces ja = V >> 40, jb = (V + SV) >> 40 with V = V0 + (i_first + s) SV; it is FULL when both lie in the grid in one
column, CROSSING when it touches the grid otherwise.  A column is uniform when one id fills it over all z.  Today's rule leaves a
slab out when all its pieces inside the grid are air columns; the new rule when both pieces - one outside the grid reads as an air
column - are uniform in the same id.  The lists of a pass (128 slabs) are padded to the longer pair of the wave and swept in
trips of 16 (full) and 8 (crossing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.environ.get('DEXCT_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dex_ct_sim_amd import forward_project as fp
from p16_dedup import chans, ct, n, specs, views, volumes

SUPER, FULL_TRIP, CROSS_TRIP = 128, 16, 8
mode = sys.argv[1] if len(sys.argv) > 1 else 'census'


def column_classes(vol):
    """[nz][ny][nx] -> per column y * nx + x: 0 mixed, 1 | id << 1 uniform in id (int64, on the device)."""
    v = torch.from_numpy(vol).cuda()
    uniform = (v == v[0]).all(dim=0)
    return torch.where(uniform, 1 | (v[0].to(torch.int64) << 1), torch.zeros((), dtype=torch.int64, device='cuda')).reshape(-1)


def census(name, ph, chunk=25):
    lanes = (n + 15) // 16
    lpp = 64 if lanes > 32 else (32 if lanes > 16 else 16)
    n_pairs = 64 // lpp
    assert chans % n_pairs == 0
    cls = column_classes(ph.volume)
    nx, ny = ph.Nx, ph.Ny
    per_id = [int((cls == (1 | k << 1)).sum()) for k in range(4)]
    print(f'== census, {name}: {nx * ny} columns; uniform per id {per_id}; mixed {int((cls == 0).sum())}', flush=True)
    tot = dict(rays=0, waves=0, full_old=0, cross_old=0, full_new=0, cross_new=0, tf_old=0, tc_old=0, tf_new=0, tc_new=0, live=0)
    for vb in range(0, views, chunk):
        pj = fp.Projector(ct, ph, view_range=(vb, min(views, vb + chunk)))
        plan = pj.plan_host()
        dev = lambda f, dt=torch.int64: torch.from_numpy(plan[f].astype(np.int64)).to('cuda', dt)[:, None]
        V0, SV, i_first, n_slabs, flags = dev('V0'), dev('SV'), dev('i_first'), dev('n_slabs'), dev('flags')
        n_pass = (int(n_slabs.max()) + SUPER - 1) // SUPER
        s = torch.arange(n_pass * SUPER, device='cuda')[None, :]
        i = i_first + s
        Va = V0 + i * SV
        ja, jb = Va >> 40, (Va + SV) >> 40
        axis = flags & 1
        nv = torch.where(axis == 0, ny, nx)
        cu, cv = torch.where(axis == 0, 1, nx), torch.where(axis == 0, nx, 1)
        valid = s < n_slabs
        ina, inb = valid & (ja >= 0) & (ja < nv), valid & (jb >= 0) & (jb < nv)
        ea = torch.where(ina, cls[(i * cu + ja * cv).clamp(0, nx * ny - 1)], 1)
        eb = torch.where(inb, cls[(i * cu + jb * cv).clamp(0, nx * ny - 1)], 1)
        live = ina | inb
        whole = ina & inb & (ja == jb)
        drop_old = live & (ea == 1) & (eb == 1)
        drop_new = live & (ea == eb) & ((ea & 1) == 1)
        assert bool((drop_new | ~drop_old).all())
        n_rays = plan.shape[0]
        for tag, drop in (('old', drop_old), ('new', drop_new)):
            full, cross = live & whole & ~drop, live & ~whole & ~drop
            tot['full_' + tag] += int(full.sum())
            tot['cross_' + tag] += int(cross.sum())
            # per pass and pair, then the longer pair of each wave, in whole trips
            f = full.reshape(n_rays // n_pairs, n_pairs, n_pass, SUPER).sum(dim=-1).amax(dim=1)
            c = cross.reshape(n_rays // n_pairs, n_pairs, n_pass, SUPER).sum(dim=-1).amax(dim=1)
            tot['tf_' + tag] += int(((f + FULL_TRIP - 1) // FULL_TRIP).sum())
            tot['tc_' + tag] += int(((c + CROSS_TRIP - 1) // CROSS_TRIP).sum())
        tot['live'] += int(live.sum())
        tot['rays'] += n_rays
        tot['waves'] += n_rays // n_pairs
        del pj
    r, w = tot['rays'], tot['waves']
    listed_old, listed_new = tot['full_old'] + tot['cross_old'], tot['full_new'] + tot['cross_new']
    print(f'   slabs that touch the grid per ray: {tot["live"] / r:.1f}', flush=True)
    print(f'   listed per ray today:     {tot["full_old"] / r:.1f} full + {tot["cross_old"] / r:.1f} crossing', flush=True)
    print(f'   listed per ray afterwards: {tot["full_new"] / r:.1f} full + {tot["cross_new"] / r:.1f} crossing '
          f'({100.0 * listed_new / max(listed_old, 1):.1f} % of today\'s; droppable {100.0 * (1 - listed_new / max(listed_old, 1)):.1f} %)', flush=True)
    print(f'   trips per wave today:      {tot["tf_old"] / w:.2f} full + {tot["tc_old"] / w:.2f} crossing = {(tot["tf_old"] + tot["tc_old"]) / w:.2f}', flush=True)
    print(f'   trips per wave afterwards: {tot["tf_new"] / w:.2f} full + {tot["tc_new"] / w:.2f} crossing = {(tot["tf_new"] + tot["tc_new"]) / w:.2f}', flush=True)


SETTINGS = [('off', {'DEXCT_P16_AIR_SKIP': '0'}), ('air only', {'DEXCT_P16_UNIFORM': '0'}), ('defaults', {}),
            ('class map forced', {'DEXCT_P16_AIR_SKIP': '2', 'DEXCT_P16_UNIFORM': '2'})]


def set_knobs(env):
    for k in ('DEXCT_P16_AIR_SKIP', 'DEXCT_P16_UNIFORM'):
        os.environ.pop(k, None)
    os.environ.update(env)


def ab(name, ph, rounds, reps=5):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    log = torch.empty_like(out)
    print(f'== {name}: air columns {pj.n_air_columns}, uniform per id {getattr(pj, "n_uniform_columns", None)}', flush=True)
    ref = None
    for rep in range(rounds):
        for tag, env in SETTINGS:
            set_knobs(env)
            pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
            e1.record()
            torch.cuda.synchronize()
            if ref is None:
                ref = (out.clone(), log.clone())
            same = bool(torch.equal(out.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(log.view(torch.int32), ref[1].view(torch.int32)))
            print(f'{name} round {rep} {tag}: {e0.elapsed_time(e1) / reps:.3f} ms  bit-identical: {same}', flush=True)
            assert same


def launch(name, ph):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    log = torch.empty_like(out)
    for tag, env in SETTINGS:             # the launches of the trace, in this order
        set_knobs(env)
        pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
        torch.cuda.synchronize()
        print(f'{name}: launch with {tag}', flush=True)


if __name__ == '__main__':
    for name, ph in volumes():
        if mode == 'census':
            census(name, ph)
        elif mode == 'ab':
            ab(name, ph, int(sys.argv[2]) if len(sys.argv) > 2 else 2)
        else:
            launch(name, ph)
