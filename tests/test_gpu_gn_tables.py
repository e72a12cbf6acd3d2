"""gn_tables_kernel (csrc/gn.hip) against a NumPy restatement: the header words, the permutation and both tables of the Newton
workspace, read back after a call on a handful of pixels.

Every value the kernel writes is one IEEE operation (a product, a cast) of its inputs, or a sum taken in the order of the
energies, or a maximum - so the comparison is of BYTES.  The one exception is the sign and payload of a NaN, which IEEE leaves
to the machine: an entry that is NaN here must be NaN there, nothing more.

  * energy counts 1, 2, 255, 256, 257 and 300: below, at and past one trip of the kernel's block of 256 threads;
  * energies of all four weight classes (both spectra, the first only, the second only, none) in an order that interleaves them,
    with one class left empty in turn, and every energy unweighted but one;
  * attenuations below, exactly at and above kMuFree = 4 (the clip-free part of a class and the part that always clips), in
    either material, and a NaN attenuation in the first material, in the second, and in both;
  * the several-bins form (one block per bin, no sorting, no float32 table).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADER, TAB, SORT_BUCKETS = 16, 14, 2048               # csrc/gn.hip kWsHeader, kTab, kSortBuckets
EXP_SCALE = float.fromhex('0x1.71547652b82fep+11')     # csrc/exp_table.h kExpScale
MU_FREE = 4.0
COUNTS = (1, 2, 255, 256, 257, 300)


def tables_of(n_e, seed, empty=None, n_bins=1):
    """(i0 [2, n_e] or [2, n_bins, n_e], mus [2, n_e]): classes interleaved (class ``empty`` left out), attenuations on both sides of
    kMuFree and at it, three NaN attenuations where there is room."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 4, size=(n_bins, n_e))
    if empty is not None:
        cls[cls == empty] = (empty + 1) % 4
    w = rng.uniform(0.5, 3.0e5, size=(2, n_bins, n_e))
    w[0][(cls == 2) | (cls == 3)] = 0.0
    w[1][(cls == 1) | (cls == 3)] = 0.0
    mus = rng.uniform(0.01, 3.9, size=(2, n_e))
    kind = rng.integers(0, 6, size=n_e)
    mus[0][kind == 0] = rng.uniform(4.1, 60.0, size=int((kind == 0).sum()))
    mus[1][kind == 1] = rng.uniform(4.1, 60.0, size=int((kind == 1).sum()))
    mus[0][kind == 2] = MU_FREE
    mus[1][kind == 3] = np.nextafter(MU_FREE, 8.0)
    mus[0][kind == 4] = -mus[0][kind == 4]                # the magnitude decides
    if n_e >= 8:
        mus[0][3], mus[1][5], mus[:, 6] = np.nan, np.nan, np.nan
    return (w[:, 0] if n_bins == 1 else w), mus


def restate(i0, mus):
    """The workspace as gn_tables_kernel must leave it: (header doubles [9], perm, tab float64, tab32 or None)."""
    n_bins = 1 if i0.ndim == 2 else i0.shape[1]
    w = i0.reshape(2, n_bins, -1)
    n_e = w.shape[-1]
    perms, tabs = [], []
    for b in range(n_bins):
        w0, w1 = w[0, b], w[1, b]
        s0, s1 = np.cumsum(w0)[-1], np.cumsum(w1)[-1]      # (cumsum adds in the order of the energies)
        scale = np.ldexp(1.0, -int(np.frexp(np.fmax(s0, s1))[1]))
        if b == 0:
            scale0 = scale
        a0, a1 = np.abs(mus[0]), np.abs(mus[1])
        if n_bins == 1:
            c = np.where((w0 != 0) & (w1 != 0), 0, np.where(w0 != 0, 1, np.where(w1 != 0, 2, 3)))
            big = ~(np.fmax(a0, a1) <= MU_FREE)
            key = 2 * c + np.where(big, 0, 1)
            perm = np.concatenate([np.flatnonzero((key == k) & (c < 3)) for k in range(6)]).astype(np.int32)
            n = [int(((c == k)).sum()) for k in range(3)]
            nc = [int(((c == k) & big).sum()) for k in range(3)]
            free = (c < 3) & ~big
            m0f = np.fmax.reduce(a0[free], initial=0.0)
            m1f = np.fmax.reduce(a1[free], initial=0.0)
        else:
            perm, n, nc, m0f, m1f = np.arange(n_e, dtype=np.int32), [n_e, 0, 0], [n_e, 0, 0], 0.0, 0.0
        if b == 0:
            header = np.array([scale0] + [float(x) for x in n] + [float(x) for x in nc] + [m0f, m1f])
        m0, m1 = mus[0][perm], mus[1][perm]
        t = np.empty((len(perm), TAB))
        t[:, 0], t[:, 1] = -m0 * EXP_SCALE, -m1 * EXP_SCALE
        m00, m01, m11 = m0 * m0, m0 * m1, m1 * m1
        for k, wk in enumerate((w0[perm], w1[perm])):
            t[:, 2 + 6 * k:8 + 6 * k] = np.stack([wk, wk * m0, wk * m1, wk * m00, wk * m01, wk * m11], axis=1)
        perms.append(perm)
        tabs.append(t)
    t32 = None
    if n_bins == 1:
        t32 = np.empty((len(perms[0]), TAB), dtype=np.float32)
        t32[:, 0], t32[:, 1] = (mus[0][perms[0]] * 1.4426950408889634), (mus[1][perms[0]] * 1.4426950408889634)
        for c in range(6):
            t32[:, 2 + 2 * c] = tabs[0][:, 2 + c] * scale0
            t32[:, 3 + 2 * c] = tabs[0][:, 8 + c] * scale0
    return header, perms, tabs, t32


def same(got, want, what):
    """bytes, but a NaN for a NaN"""
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    ok = (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (what, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


def workspace_after_a_call(i0, mus):
    from dex_ct_sim_amd import matdecomp as md
    n_pix = 64 if i0.ndim == 2 else 60                  # one tile: the tile sort, which would use the histogram, stays out
    g = torch.full((2, n_pix), 1000.0, dtype=torch.float64, device='cuda')
    md.gn_device(g[0], g[1], i0, mus, 4, 'f64', kernel=1, audit=0, stop_tol=1e-12, two_level=False, dedup=False)
    torch.cuda.synchronize()
    return md._last_run.workspaces[-1].cpu().numpy()


def check(i0, mus):
    header, perms, tabs, t32 = restate(i0, mus)
    n_bins = len(perms)
    n_e = mus.shape[1]
    ws = workspace_after_a_call(i0, mus)
    got_header = ws[:8 * 9].view(np.float64)
    same(got_header, header, 'header')
    at = 8 * HEADER
    tab = ws[at:at + 8 * n_bins * n_e * TAB].view(np.float64).reshape(n_bins, n_e, TAB)
    at += 8 * n_bins * n_e * TAB
    tab32 = ws[at:at + 4 * n_e * TAB].view(np.float32).reshape(n_e, TAB)
    at += 4 * n_e * TAB
    perm = ws[at:at + 4 * n_bins * n_e].view(np.int32).reshape(n_bins, n_e)
    at = (at + 4 * n_bins * n_e + 15) // 16 * 16
    hist = ws[at:at + 4 * SORT_BUCKETS].view(np.int32)
    for b in range(n_bins):
        n_used = len(perms[b])
        assert np.array_equal(perm[b, :n_used], perms[b]), ('perm', b)
        same(tab[b, :n_used], tabs[b], ('tab', b))
    if t32 is not None:
        same(tab32[:len(perms[0])], t32, 'tab32')
    assert not hist.any()
    return header


@pytest.mark.parametrize('n_e', COUNTS)
def test_one_spectrum_row(hip, n_e):
    seen = set()
    for empty in (None, 0, 1, 2, 3):
        i0, mus = tables_of(n_e, 100 * n_e + (empty or 0) + 1, empty)
        header = check(i0, mus)
        seen |= {k for k in range(3) if header[1 + k] > 0}
        if empty is not None and empty < 3:
            assert header[1 + empty] == 0 and header[4 + empty] == 0
    if n_e >= 255:
        assert seen == {0, 1, 2} and header[7] > 0 and header[8] > 0
    # every energy but one without weight
    i0, mus = tables_of(n_e, 7 * n_e, None)
    i0[:, :n_e - 1] = 0.0
    i0[:, n_e - 1] = (3.0, 0.0)
    header = check(i0, mus)
    assert header[1:4].tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize('n_e,n_bins', [(5, 3), (257, 2)])
def test_several_bins(hip, n_e, n_bins):
    i0, mus = tables_of(n_e, 31 * n_e, None, n_bins)
    mus = np.where(np.isnan(mus), 1.0, mus)             # (the per-bin kernel iterates every energy: keep the few pixels finite)
    header = check(i0, mus)
    assert header[1:9].tolist() == [n_e, 0, 0, n_e, 0, 0, 0.0, 0.0]
