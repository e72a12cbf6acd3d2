"""rows16_kernel: runs of slabs in uniform tiles dismissed before the slab classification (profiles/rows16_tiles.md).  The projection
launch of the benchmark scan (512^3, 1000 x 800 x 512, dual spectrum) on the volumes of tools/probes/p16_dedup.py.  DEXCT_ROOT
names the tree whose package is loaded (default: this one); the census needs nothing this change adds and runs on any tree with
the packed route.

    python tools/probes/p16_tiles.py census        # slabs classified one by one, run trips and fine trips per wave: today / tile rule
    python tools/probes/p16_tiles.py ab [rounds]   # DEXCT_P16_TILES = 0 / 1 / 2, ms per launch, results compared bit for bit
    python tools/probes/p16_tiles.py launch        # one launch per knob setting (run under a counter or a trace pass)

The census restates the kernel's two phases (csrc/tile_class.h) against the kernel's own plan (dexct_fan_plan, read back).  A TILE
is K x K columns and is uniform in an id when all its columns are (a tile that reaches past the grid: in air only); a RUN is the K
slabs i = K R .. K R + K - 1 of a ray, cut to the ray's slabs; its pieces lie between ja of its first and jb of its last slab, in
at most three tiles, and it is DISMISSED when all of them (one outside the grid counts as air) are uniform in the same id.  Lane l
of a pair takes run l of each group of lanes_per_pair runs (a RUN TRIP); the surviving runs of a window of 64 runs go through the
slab classification in passes of 128 / K runs per pair, 2 lanes_per_pair slabs per FINE TRIP.  The census asserts that a dismissed
run holds only slabs the slab rule drops."""
import os
import sys

import numpy as np
import torch

ROOT = os.environ.get('DEXCT_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dex_ct_sim_amd import forward_project as fp
from p16_dedup import chans, ct, n, specs, views, volumes
from p16_uniform import column_classes

SUPER, BATCH, WINDOW = 128, 2, 64
RUN_COST, FINE_COST = 120.0, 166.0          # instructions of a run trip against a trip of today's loop (the stop rule's weights)
mode = sys.argv[1] if len(sys.argv) > 1 else 'census'
VIEW_STEP = int(os.environ.get('VIEW_STEP', 1))


def tile_maps(cls, nx, ny, K):
    """Per slab axis the tile classes [I][J + 1] with an air tile in front of and behind every row of J."""
    c = cls.reshape(ny, nx)
    ty, tx = (ny + K - 1) // K, (nx + K - 1) // K
    pad = torch.ones((ty * K, tx * K), dtype=c.dtype, device=c.device)        # outside the grid: air
    pad[:ny, :nx] = c
    t = pad.reshape(ty, K, tx, K).permute(0, 2, 1, 3).reshape(ty, tx, K * K)
    first = t[..., 0]
    same = (t == first[..., None]).all(dim=-1) & ((first & 1) == 1)
    tile = torch.where(same, first, torch.zeros_like(first))                   # [ty][tx]; a partial tile is all 1 or mixed
    guard = lambda m: torch.nn.functional.pad(m, (1, 1), value=1)
    return guard(tile.t().contiguous()), guard(tile)                            # axis 0: i = x, j = y; axis 1: i = y, j = x


def census(name, ph, chunk=25):
    lanes = (n + 15) // 16
    lpp = 64 if lanes > 32 else (32 if lanes > 16 else 16)
    n_pairs = 64 // lpp
    assert chans % n_pairs == 0
    cls = column_classes(ph.volume)
    nx, ny = ph.Nx, ph.Ny
    per_id = [int((cls == (1 | k << 1)).sum()) for k in range(4)]
    print(f'== census, {name}: {nx * ny} columns; uniform per id {per_id}; mixed {int((cls == 0).sum())}; '
          f'{lpp} lanes per pair, every {VIEW_STEP}. chunk of views', flush=True)
    Ks = (4, 8, 16)
    maps = {K: tile_maps(cls, nx, ny, K) for K in Ks}
    for K in Ks:
        t = maps[K][1][:, 1:-1]
        print(f'   K = {K}: {t.numel()} tiles, uniform per id {[int((t == (1 | k << 1)).sum()) for k in range(4)]}', flush=True)
    tot = dict(rays=0, waves=0, slabs=0, dropped=0, listed=0, trips_today=0)
    per_k = {K: dict(fine=0, fine_ideal=0, run_trips=0, fine_trips=0, passes=0, one_pass=0, le128=0, none=0) for K in Ks}
    for vb in list(range(0, views, chunk))[::VIEW_STEP]:
        pj = fp.Projector(ct, ph, view_range=(vb, min(views, vb + chunk)))
        plan = pj.plan_host()
        dev = lambda f: torch.from_numpy(plan[f].astype(np.int64)).to('cuda')[:, None]
        V0, SV, i_first, n_slabs, flags = dev('V0'), dev('SV'), dev('i_first'), dev('n_slabs'), dev('flags')
        n_rays = plan.shape[0]
        axis = flags & 1
        nv = torch.where(axis == 0, ny, nx)
        cu, cv = torch.where(axis == 0, 1, nx), torch.where(axis == 0, nx, 1)
        # ---- the slab rule (today)
        n_max = int(n_slabs.max())
        s = torch.arange(n_max, device='cuda')[None, :]
        i = i_first + s
        Va = V0 + i * SV
        ja, jb = Va >> 40, (Va + SV) >> 40
        valid = s < n_slabs
        ina, inb = valid & (ja >= 0) & (ja < nv), valid & (jb >= 0) & (jb < nv)
        ea = torch.where(ina, cls[(i * cu + ja * cv).clamp(0, nx * ny - 1)], 1)
        eb = torch.where(inb, cls[(i * cu + jb * cv).clamp(0, nx * ny - 1)], 1)
        drop = valid & (ea == eb) & ((ea & 1) == 1)
        listed = valid & ~drop & (ina | inb)
        tot['slabs'] += int(valid.sum())
        tot['dropped'] += int((valid & drop).sum())
        tot['listed'] += int(listed.sum())
        wave_slabs = n_slabs.reshape(n_rays // n_pairs, n_pairs).amax(dim=1)
        for s0 in range(0, n_max, SUPER):            # the trips of today's loop: whole batches up to the longest ray of the wave
            left = (wave_slabs - s0).clamp(min=0)
            tot['trips_today'] += int((((left + BATCH * lpp - 1) // (BATCH * lpp)) * (BATCH * lpp)).clamp(max=SUPER).sum()) // (BATCH * lpp)
        for K in Ks:
            sh = K.bit_length() - 1
            R0 = i_first >> sh
            n_runs = torch.where(n_slabs > 0, ((i_first + n_slabs - 1) >> sh) - R0 + 1, 0)
            r = torch.arange(int(n_runs.max()), device='cuda')[None, :]
            ilo = torch.maximum((R0 + r) << sh, i_first)
            ihi = torch.minimum(((R0 + r) << sh) + K - 1, i_first + n_slabs - 1)
            rvalid = (r < n_runs) & (ilo <= ihi)
            j0, j1 = (V0 + ilo * SV) >> 40, (V0 + (ihi + 1) * SV) >> 40
            jlo, jhi = torch.minimum(j0, j1), torch.maximum(j0, j1)
            t0, t1 = maps[K]
            TJ = torch.where(axis == 0, t0.shape[1] - 2, t1.shape[1] - 2)
            Jlo = torch.minimum(torch.maximum(jlo >> sh, torch.full_like(jlo, -1)), TJ)
            Jhi = torch.minimum(torch.maximum(jhi >> sh, torch.full_like(jhi, -1)), TJ)
            I = (R0 + r)
            look = lambda J: torch.where(axis == 0, t0[I.clamp(0, t0.shape[0] - 1), (J + 1).clamp(0, t0.shape[1] - 1)],
                                         t1[I.clamp(0, t1.shape[0] - 1), (J + 1).clamp(0, t1.shape[1] - 1)])
            c0, c1, c2 = look(Jlo), look(torch.minimum(Jlo + 1, Jhi)), look(Jhi)
            dismissed = rvalid & (Jhi - Jlo <= 2) & (c0 == c1) & (c0 == c2) & ((c0 & 1) == 1)
            # a dismissed run holds only slabs the slab rule drops, all in the class of its tiles
            run_of_slab = ((i >> sh) - R0).clamp(0, r.shape[1] - 1)
            dis_slab = torch.gather(dismissed, 1, run_of_slab) & valid
            cls_slab = torch.gather(c0.expand_as(dismissed), 1, run_of_slab)
            assert bool((~dis_slab | (drop & (eb == cls_slab))).all()), 'the tile rule dismissed a slab the slab rule keeps'
            surv = rvalid & ~dismissed
            k = per_k[K]
            k['fine'] += int((torch.gather(surv, 1, run_of_slab) & valid).sum())
            # what could be seen at best: runs whose slabs are all droppable in one class
            kept_in_run = torch.zeros_like(surv, dtype=torch.int64).scatter_add_(1, run_of_slab, (valid & ~drop).to(torch.int64))
            k['fine_ideal'] += int((torch.gather(kept_in_run > 0, 1, run_of_slab) & valid).sum())
            wave_runs = n_runs.reshape(n_rays // n_pairs, n_pairs).amax(dim=1)
            k['run_trips'] += int(((wave_runs + lpp - 1) // lpp).sum())
            cap = SUPER // K
            n_surv_ray = surv.sum(dim=1)
            total_passes = torch.zeros(n_rays // n_pairs, dtype=torch.int64, device='cuda')
            for w0 in range(0, r.shape[1], WINDOW):
                sw = surv[:, w0:w0 + WINDOW].sum(dim=1).reshape(n_rays // n_pairs, n_pairs).amax(dim=1)
                while bool((sw > 0).any()):
                    take = sw.clamp(max=cap)
                    k['fine_trips'] += int(((take * K + BATCH * lpp - 1) // (BATCH * lpp)).sum())
                    total_passes += (take > 0).to(torch.int64)
                    sw = sw - take
            k['passes'] += int(total_passes.sum())
            k['one_pass'] += int((total_passes <= 1).sum())
            longer = n_surv_ray.reshape(n_rays // n_pairs, n_pairs).amax(dim=1)
            k['le128'] += int((longer * K <= SUPER).sum())
            k['none'] += int((longer == 0).sum())
        tot['rays'] += n_rays
        tot['waves'] += n_rays // n_pairs
        del pj
    rr, w = tot['rays'], tot['waves']
    print(f'   slabs per ray: {tot["slabs"] / rr:.1f}; the slab rule drops {tot["dropped"] / rr:.1f} '
          f'({100.0 * tot["dropped"] / tot["slabs"]:.1f} %) and lists {tot["listed"] / rr:.1f}', flush=True)
    print(f'   today: {tot["slabs"] / rr:.1f} slabs per ray classified one by one, {tot["trips_today"] / w:.2f} trips per wave', flush=True)
    for K in Ks:
        k = per_k[K]
        saved = tot['trips_today'] / w - k['run_trips'] / w * RUN_COST / FINE_COST - k['fine_trips'] / w
        print(f'   K = {K}: {k["fine"] / rr:.1f} fine slabs per ray ({100.0 * k["fine"] / tot["slabs"]:.1f} %); {k["fine_ideal"] / rr:.1f} if every '
              f'droppable run could be seen; {k["run_trips"] / w:.2f} run trips + {k["fine_trips"] / w:.2f} fine trips per wave in '
              f'{k["passes"] / w:.2f} passes; waves with at most {SUPER} fine slabs in their longer pair {100.0 * k["le128"] / w:.1f} %, '
              f'with at most one pass {100.0 * k["one_pass"] / w:.1f} %, without a fine slab {100.0 * k["none"] / w:.1f} %; '
              f'trips\' worth saved (stop rule: 3.5) {saved:.2f}', flush=True)


SETTINGS = [('tiles off', {'DEXCT_P16_TILES': '0'}), ('defaults', {}), ('tile map forced', {'DEXCT_P16_TILES': '2'})]


def set_knobs(env):
    os.environ.pop('DEXCT_P16_TILES', None)
    os.environ.update(env)


def ab(name, ph, rounds, reps=5):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    log = torch.empty_like(out)
    print(f'== {name}: uniform columns per id {pj.n_uniform_columns}, uniform tiles per id {getattr(pj, "n_uniform_tiles", None)}', flush=True)
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
