"""rows16_kernel: detecting each distinct quad of rows once per wave (profiles/rows16_dedup.md).  The projection launch of the
benchmark scan (512^3, 1000 x 800 x 512, dual spectrum) on three volumes: the benchmark phantom, the same phantom with the voxels
of every z slice shuffled independently (no two rows alike) and a volume of random blobs.  DEXCT_ROOT names the tree whose package
is loaded (default: this one), so that a build without the knob - where it does nothing - is measured by the same script.

    python tools/probes/p16_dedup.py census        # fresh quads per wave, from the path lengths (outside any timed region)
    python tools/probes/p16_dedup.py ab [rounds]   # DEXCT_DET_DEDUP = 0 / 1, ms per launch, results compared bit for bit
    python tools/probes/p16_dedup.py valu          # one launch with the full tables, one with their first 4 energies, per
                                                   # volume and knob: run it under rocprofv3 --pmc SQ_INSTS_VALU --kernel-trace

A quad is one lane's four rows of one detection round; it is FRESH when any of its per-material sums differs bitwise from the same
row of the quad before it in the channel (the first quad of a channel is always fresh).  The census compares the path lengths of
the materials 1.. (= sum x len_per_u of the pair: equal sums give equal lengths, and two different sums round to the same length
only by accident, so it can undercount fresh quads by a few, never overcount)."""
import os
import sys

import numpy as np
import torch

ROOT = os.environ.get('DEXCT_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import dex_ct_sim_amd as dx
from dex_ct_sim_amd import forward_project as fp, synthetic
from dex_ct_sim_amd.system import AIR, BONE, WATER

det = os.path.join(ROOT, 'dex-ct-sim_amd/input/detector/eta_eid_mv.bin')
n, views, chans = int(os.environ.get('N', 512)), int(os.environ.get('VIEWS', 1000)), int(os.environ.get('CHANS', 800))
mode = sys.argv[1] if len(sys.argv) > 1 else 'census'
ct = dx.FanBeamGeometry(N_channels=chans, N_proj=views, gamma_fan=0.8230337, SID=60.0, SDD=100.0, eid=True, detector_file=det, N_rows=n)
specs = [synthetic.kramers_spectrum(140), synthetic.kramers_spectrum(80)]
# A one-row round against a four-row round, per energy and lane, v_exp_f32 priced at two plain instructions: 5 v_fma_f32 + 1 v_exp_f32
# = 7 against 10 v_pk_fma_f32 + 4 v_exp_f32 = 18 (three materials, two spectra)
ONE_ROW = 7.0 / 18.0


def volumes():
    ph = synthetic.make_phantom(n, n, extent=51.2, seed=1234)
    which = os.environ.get('VOLUMES', 'benchmark,shuffled,blobs').split(',')
    wrap = lambda name, vol: dx.VoxelPhantom.from_array(name, vol, [AIR, WATER, BONE], dx=ph.dx, dy=ph.dy, dz=ph.dz)
    if 'benchmark' in which:
        yield 'benchmark phantom', ph
    if 'shuffled' in which:
        rng = np.random.default_rng(1)
        yield 'slices shuffled', wrap('shuffled', rng.permuted(ph.volume.reshape(n, -1), axis=1).reshape(ph.volume.shape))
    if 'blobs' in which:
        rng = np.random.default_rng(2)
        vol = np.zeros((n, n, n), dtype=np.uint8)
        z, y, x = np.ogrid[0:n, 0:n, 0:n]
        for k in range(300):
            r = rng.uniform(0.02, 0.10) * n
            c = rng.uniform(0.15, 0.85, 3) * n
            lo, hi = np.maximum(0, (c - r).astype(int)), np.minimum(n, (c + r).astype(int) + 1)
            sub = (z[lo[0]:hi[0]] - c[0]) ** 2 + (y[:, lo[1]:hi[1]] - c[1]) ** 2 + (x[:, :, lo[2]:hi[2]] - c[2]) ** 2 <= r * r
            vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][sub] = 1 + k % 2
        yield 'random blobs', wrap('blobs', vol)


def census(name, ph, chunk=50):
    lanes = (n + 15) // 16
    lpp = 64 if lanes > 32 else (32 if lanes > 16 else 16)
    n_pairs = 64 // lpp
    assert n <= 1024 and n % 4 == 0 and chans % n_pairs == 0
    hist = torch.zeros(6, dtype=torch.int64, device='cuda')
    last = torch.zeros(4, dtype=torch.int64, device='cuda')      # the last list round holds <= 16 / <= 32 / more entries; no list
    eq = torch.zeros(3, dtype=torch.float64, device='cuda')      # round-equivalents: four-row rounds / two-row rule / one-row rule
    sum_f, extruded, waves = 0, 0, 0
    for vb in range(0, views, chunk):
        pj = fp.Projector(ct, ph, view_range=(vb, min(views, vb + chunk)))
        _, mu_d, w_d, _ = pj.upload_tables(specs)
        _, pl = pj.project_tables(mu_d, w_d, want_pathlen=True, layout=1)            # [view][channel][row][material]
        x = pl[..., 1:].contiguous().view(torch.int32).reshape(pl.shape[0], chans, n // 4, -1)
        fresh = (x[:, :, 1:] != x[:, :, :-1]).any(dim=-1)
        f_pair = fresh.sum(dim=-1) + 1
        f = f_pair.reshape(pl.shape[0], chans // n_pairs, n_pairs).sum(dim=-1).reshape(-1)
        hist += torch.bincount((f + 63) // 64, minlength=6)[:6]
        # the narrow rounds (csrc/dedup_index.h: round_rows): a wave detects its list where that saves a round (fewer than the
        # four rounds of rows); every round of 64 entries is one round-equivalent, the last costs 1/2 at two rows per lane (at most
        # 32 entries left) and ONE_ROW at one (at most 16)
        rounds = (f + 63) // 64
        left = f - 64 * (rounds - 1)
        listed = rounds < 4
        kind = torch.where(listed, torch.where(left <= 16, 0, torch.where(left <= 32, 1, 2)), 3)
        last += torch.bincount(kind, minlength=4)
        full = torch.where(listed, rounds, 4).double()
        two = torch.where(listed & (left <= 32), full - 0.5, full)
        one = torch.where(listed & (left <= 16), full - 1.0 + ONE_ROW, two)
        eq += torch.stack([full.sum(), two.sum(), one.sum()])
        sum_f += int(f.sum())
        extruded += int((f == n_pairs).sum())
        waves += f.numel()
        del pj, pl, x, fresh
    hist = hist.cpu().tolist()
    quads = n_pairs * (n // 4)
    mean_rounds = sum(k * h for k, h in enumerate(hist)) / waves
    print(f'== census, {name}: {waves} waves of {quads} quads; mean F {sum_f / waves:.1f}; F = {n_pairs} (every pair extruded) in '
          f'{100.0 * extruded / waves:.1f} % of the waves', flush=True)
    print('   ceil(F / 64): ' + ', '.join(f'{k}: {100.0 * h / waves:.1f} %' for k, h in enumerate(hist) if h) + f'; mean {mean_rounds:.3f}', flush=True)
    last, eq = last.cpu().tolist(), (eq / waves).cpu().tolist()
    print('   entries left for the last list round: ' + ', '.join(f'{name}: {100.0 * h / waves:.1f} %' for name, h in
                                                                   zip(('at most 16', '17 .. 32', '33 .. 64', 'no list (four rounds of rows)'), last)), flush=True)
    print(f'   detection round-equivalents per wave: {eq[0]:.3f} with four-row rounds only, {eq[1]:.3f} with the last round at two rows '
          f'for at most 32 entries (saves {eq[0] - eq[1]:.3f}), {eq[2]:.3f} with one row for at most 16 as well (at {ONE_ROW:.3f} of a round)',
          flush=True)


def timed(pj, mu_d, w_d, air, out, log, knob, reps=5):
    os.environ.pop('DEXCT_DET_DEDUP', None)
    if knob is not None:
        os.environ['DEXCT_DET_DEDUP'] = knob
    pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        pj.project_tables(mu_d, w_d, out=out, layout=None, air=air, log_out=log)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(name, ph, rounds):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    log = torch.empty_like(out)
    ref = None
    for rep in range(rounds):
        for knob in ('0', '1', None):
            ms = timed(pj, mu_d, w_d, air, out, log, knob)
            if ref is None:
                ref = (out.clone(), log.clone())
            same = bool(torch.equal(out.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(log.view(torch.int32), ref[1].view(torch.int32)))
            print(f'{name} round {rep} det_dedup={knob}: {ms:.3f} ms  bit-identical: {same}', flush=True)
            assert same


def valu(name, ph):
    pj = fp.Projector(ct, ph)
    _, mu_d, w_d, air = pj.upload_tables(specs)
    out = torch.empty((2, views, chans, n), dtype=torch.float32, device='cuda')
    for knob in os.environ.get('KNOBS', '0,1').split(','):
        os.environ['DEXCT_DET_DEDUP'] = knob
        for n_e in (mu_d.shape[1], 4):             # the launches of the trace, in this order
            pj.project_tables(mu_d[:, :n_e].contiguous(), w_d[:, :n_e].contiguous(), out=out, layout=None)
            torch.cuda.synchronize()
            print(f'{name}: launch with det_dedup={knob}, {n_e} energies', flush=True)


if __name__ == '__main__':              # (tools/probes/gn_dedup.py imports the volumes)
    for name, ph in volumes():
        if mode == 'census':
            census(name, ph)
        elif mode == 'ab':
            ab(name, ph, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
        else:
            valu(name, ph)
