"""The capped grids and word wraps of dexct_gn_decompose_dedup's passes (csrc/gn_dedup.hip, csrc/gn_dedup_index.h), the shapes that run
them past one trip, and a host model of the route's index side - in the manner of tests/grid_caps.py.

``CONSTANTS`` names every constant the shapes rest on with its file and value (tests/test_gn_dedup_caps.py reads the sources and
compares); ``trip_items`` derives from them what one trip of each pass covers; every shape below is derived from that.  A later
change of a cap then fails on the CPU instead of silently taking tests/test_gpu_gn_dedup_caps.py back inside one trip.

  pass            one trip covers
  probe           kProbeMaxGrid blocks x waves x kProbeUnroll bit words of the sampled lines (every kProbeStride-th)
  census          kMaxGrid x waves lines
  scan            SCAN_TRIP_SUMS block sums (of kScanBlock lines each); ``carry`` crosses trips
  gather          kMaxGrid batches of max(1, kGatherWords // words_per_line(R)) lines
  gather_chunk    kGatherWords bit words of a line that is a batch by itself (``run += total`` between chunks)
  expand          kMaxGrid columns (a view's kExpandC channels, all rows)
  expand_reload   kWave bit words of a line in registers (reload at (rb + 1) % kWave == 0, word_of_lane(.., rb % kWave))

THE MODEL (``run``) works on the fresh bits of a sinogram [L lines][R rows] alone and follows the kernels buffer by buffer: the
probe's vote, the census' bit words and counts, the block sums, their scan and F, the bases, the list (which pixel's counts stand
at which place), the results, and for every pixel the entry it takes.  Results are opaque: the "result" of a list entry is the KEY of
the pixel gathered there - the identity of that pixel's pair of counts, ``Sinogram.key`` - so two entries with equal counts are
the same result, as on the device.  The unchanged route gives every pixel its own key.

THE MUTANTS: every pass takes ('trips', n) - it stops after n trips - and 'late' - from trip 2 on, work item i reads what item
i + 1 should (the last one nothing) and writes where it should.  What a pass did not write keeps what the buffer held: the fill
byte 0x00 or 0xFF in bits, counts, bases, sums, list, results and output.  ``rejected`` says whether a mutant changes the
descriptor (use, F, cap) or any pixel's key: what tests/test_gpu_gn_dedup_caps.py compares, given that it also asserts on the
device that the direct route's results differ between the lines a mutant confuses (``confused_line_offsets``).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc')

# constant -> (source file, value)
CONSTANTS = {
    'kMaxGrid': ('gn_dedup.hip', 2048),
    'kProbeMaxGrid': ('gn_dedup.hip', 1024),
    'kProbeUnroll': ('gn_dedup.hip', 4),
    'kBlock': ('gn_dedup.hip', 256),
    'kExpandC': ('gn_dedup.hip', 32),
    'kGatherWords': ('gn_dedup_index.h', 256),
    'kScanBlock': ('gn_dedup_index.h', 1024),
    'kProbeStride': ('gn_dedup_index.h', 64),
    'kUseShare': ('gn_dedup_index.h', 8),
    'kTile': ('gn_dedup_index.h', 64),
    'kWordBits': ('gn_dedup_index.h', 64),
    'kWave': ('common.h', 64),
}
SCAN_TRIP_SUMS = 1024          # gn_dedup_scan_kernel: a literal - the block's threads and the stride of its loop (SCAN_LITERALS)
SCAN_LITERALS = (r'__launch_bounds__\(1024\) void gn_dedup_scan_kernel', r'for \(long long b0 = 0; b0 < n_blocks; b0 \+= 1024\)',
                 r'block_exclusive_scan<1024>\(v, s, &total\)', r'dim3\(1\), dim3\(1024\), 0, st, sums, n_blocks, desc')


def K(name):
    return CONSTANTS[name][1]


def source_constants():
    """{name: (file, value)} of every ``kName = VALUE`` of the ``constexpr int`` statements of the files CONSTANTS names."""
    found = {}
    for f in sorted({f for f, _ in CONSTANTS.values()}):
        for stmt in re.finditer(r'^\s*constexpr\s+int\s+([^;]*);', open(os.path.join(CSRC, f)).read(), re.M):
            for piece in stmt.group(1).split(','):
                m = re.fullmatch(r'\s*(k\w+)\s*=\s*(\d+)\s*', piece)
                if m:
                    found[m.group(1)] = (f, int(m.group(2)))
    return found


def scan_literals_present():
    text = open(os.path.join(CSRC, 'gn_dedup.hip')).read()
    return [bool(re.search(p, text)) for p in SCAN_LITERALS]


# ---- gn_dedup_index.h on the host ------------------------------------------------------------------------------------------------

def ceil_div(a, b):
    return -(-a // b)


def waves_per_block():
    return K('kBlock') // K('kWave')


def words_per_line(R):
    return ceil_div(R, K('kWordBits'))


def batch_lines(R):
    return max(1, K('kGatherWords') // words_per_line(R))


def capacity(n_pix):
    return n_pix // K('kUseShare') // K('kTile') * K('kTile')


PASSES = ('probe', 'census', 'scan', 'gather', 'gather_chunk', 'expand', 'expand_reload')


def trip_items(pass_name, R=None):
    """The work items one trip of the pass covers, in the pass' own unit (see the table above)."""
    return {'probe': K('kProbeMaxGrid') * waves_per_block() * K('kProbeUnroll'),
            'census': K('kMaxGrid') * waves_per_block(),
            'scan': SCAN_TRIP_SUMS,
            'gather': K('kMaxGrid'),
            'gather_chunk': K('kGatherWords'),
            'expand': K('kMaxGrid'),
            'expand_reload': K('kWave')}[pass_name]


def items(pass_name, V, C, R):
    """The work items the pass has on sinograms of V views x C channels x R rows."""
    L, nw = V * C, words_per_line(R)
    return {'probe': ceil_div(L, K('kProbeStride')) * nw,
            'census': L,
            'scan': ceil_div(L, K('kScanBlock')),
            'gather': ceil_div(L, batch_lines(R)),
            'gather_chunk': nw if batch_lines(R) == 1 else 1,
            'expand': V * ceil_div(C, K('kExpandC')),
            'expand_reload': nw}[pass_name]


def trips(pass_name, V, C, R):
    return max(1, ceil_div(items(pass_name, V, C, R), trip_items(pass_name, R)))


def all_trips(V, C, R):
    return {p: trips(p, V, C, R) for p in PASSES}


def trip_lines(pass_name, R):
    """One trip of the pass in LINES (probe: the lines between the first sampled line of trip 1 and of trip 2)."""
    return {'probe': trip_items('probe') // words_per_line(R) * K('kProbeStride'), 'census': trip_items('census'),
            'scan': SCAN_TRIP_SUMS * K('kScanBlock'), 'gather': K('kMaxGrid') * batch_lines(R)}[pass_name]


def confused_line_offsets(V, C, R):
    """The distances, in lines, between a line and the one a wrong trip or a late work item would read in its place."""
    L, tc, e = V * C, ceil_div(C, K('kExpandC')), K('kExpandC')
    w = {1, batch_lines(R), K('kProbeStride'), K('kScanBlock')} | {trip_lines(p, R) for p in ('probe', 'census', 'scan', 'gather')}
    q, rest = divmod(K('kMaxGrid'), tc)                      # a trip of the expansion: q views and ``rest`` tiles on, or one view more and back
    w |= {q * C + rest * e, (q + 1) * C - (tc - rest) * e, e, C - (tc - 1) * e}
    return sorted(x for x in w if 0 < x < L)


# ---- sinograms as fresh bits --------------------------------------------------------------------------------------------------------

KEY_POOL = 457                 # distinct pairs of counts the large shapes draw from (the GPU suite takes that many `inside` points)
KEY_STRIDE = 7                 # a line's next fresh run takes the pair 7 on (tests/test_gpu_gn_dedup_passes.py lines_of_fresh_rows)
SMALL_POOL = 521               # the small shapes: lines_of_fresh_rows itself, (run + 7 l) % len(live); len(live) > 520


class Sinogram:
    """step [L, R] bool: the rows whose counts differ from the row before (column 0 ignored: row 0 is always fresh).
    key [L, R]: the identity of each pixel's pair of counts - ``large``: pair (l + 7 run) % KEY_POOL, g2 advanced by l // KEY_POOL
    ulps; else lines_of_fresh_rows' (run + 7 l) % SMALL_POOL."""

    def __init__(self, V, C, R, step, large=True):
        self.V, self.C, self.R, self.L = V, C, R, V * C
        step = np.array(step, dtype=bool).reshape(self.L, R)
        step[:, 0] = False
        run = np.cumsum(step, axis=1, dtype=np.int32)
        line = np.arange(self.L, dtype=np.int32)[:, None]
        self.key = (line + KEY_STRIDE * run) % KEY_POOL + KEY_POOL * (line // KEY_POOL) if large else (run + KEY_STRIDE * line) % SMALL_POOL
        assert self.key.dtype == np.int32
        assert np.all((self.key[:, 1:] != self.key[:, :-1]) == step[:, 1:])       # a new run is a new pair, nothing else is
        step[:, 0] = True
        nw = words_per_line(R)
        padded = np.zeros((self.L, nw * 64), dtype=bool)
        padded[:, :R] = step
        self.bits = np.packbits(padded, axis=1, bitorder='little').view('<u8').reshape(self.L, nw)
        self.n_pix, self.cap = self.L * R, capacity(self.L * R)

    def expected(self):
        """include/dexct_gn_dedup.h on the host: (use, F, cap)"""
        per_word = np.bitwise_count(self.bits)
        sample = int(per_word[::K('kProbeStride')].sum())
        if sample * K('kUseShare') > ceil_div(self.L, K('kProbeStride')) * self.R:
            return (0, 0, self.cap)
        F = int(per_word.sum())
        return (int(F <= self.cap), F, self.cap)


def device_fresh(g):
    """g [2][..][R] float32 / float64 torch tensor -> bool [..][R]: the pixels whose bits differ from the row before (row 0 always)."""
    import torch
    b = g.view(torch.int32 if g.dtype == torch.float32 else torch.int64)
    fresh = torch.ones(b.shape[1:], dtype=torch.bool, device=g.device)
    fresh[..., 1:] = (b[0, ..., 1:] != b[0, ..., :-1]) | (b[1, ..., 1:] != b[1, ..., :-1])
    return fresh


def device_expected(g):
    """What last_gn_stats()['dedup'] must say after one launch on the device sinograms g [2][..][channels][rows]: the rules of
    include/dexct_gn_dedup.h (the probe's vote on every kProbeStride-th line, then the census against the capacity), on the device."""
    R = int(g.shape[-1])
    per_line = device_fresh(g).sum(dim=-1).reshape(-1)
    L = int(per_line.numel())
    cap = capacity(L * R)
    if int(per_line[::K('kProbeStride')].sum()) * K('kUseShare') > ceil_div(L, K('kProbeStride')) * R:
        return {'use': 0, 'F': 0, 'cap': cap, 'launches': 1}
    F = int(per_line.sum())
    return {'use': int(F <= cap), 'F': F, 'cap': cap, 'launches': 1}


def grid_lr(V, C, R, xp=np, **kw):
    """(l [L, 1], r [1, R]) integer grids: numpy here, torch (``xp=torch, device=...``) in the GPU suite - the patterns below use
    only operators both have."""
    return xp.arange(V * C, **kw).reshape(-1, 1), xp.arange(R, **kw).reshape(1, -1)


# ---- the large cases: step(l, r) as pure integer arithmetic ----------------------------------------------------------------------------

class Case:
    """name, (V, C, R), step(l, r) -> bool, the expected ``use``, the passes it targets: those whose mutants it must reject."""

    def __init__(self, name, shape, step, use, targets, note):
        self.name, self.shape, self.step, self.use, self.targets, self.note = name, shape, step, use, targets, note

    def sinogram(self):
        return Sinogram(*self.shape, self.step(*grid_lr(*self.shape, dtype=np.int64)))

    def mutants(self):
        """(pass, kind) of every mutant the case must reject: a pass name stands for both of its kinds"""
        return [m for t in self.targets for m in ([(t, k) for k in MUTANT_KINDS] if isinstance(t, str) else [t])]


def smallest_channels(V, lines):
    return ceil_div(lines, V)


def _large_cases():
    R, V = 16, 1000                                          # one partial word per line
    every = max(trip_lines(p, R) for p in ('probe', 'census', 'scan', 'gather'))      # the trips of probe, scan and gather end together
    assert every == trip_lines('probe', R) == trip_lines('scan', R) and 2 * trip_lines('gather', R) == every
    stride = K('kProbeStride')

    def light(l, r):                                         # two lines of three carry one more fresh pixel
        return (r == 1 + (5 * l) % (R - 1)) & (l % 3 != 0)

    # A: a quarter past the common trip; B: past two trips by more than three blocks of the scan
    CA = smallest_channels(V, every + every // 4)
    CB = smallest_channels(V, 2 * every + 3 * K('kScanBlock') + 1)
    LA = V * CA
    first_probe = trip_lines('probe', R)                     # the first line the probe's trip 2 samples
    first_scan = trip_lines('scan', R)                       # the first line whose count reaches F through ``carry``
    assert first_probe % stride == 0 and first_scan % stride == 0 and LA > max(first_probe, first_scan) + stride

    def a_no(l, r):                                          # sampled lines: trip 1 repeats, trip 2 is fresh in every row
        s = l % stride == 0
        return (s & (l >= first_probe) & (r >= 1)) | (~s & light(l, r))

    def edge(L, special):
        """The sample one pixel over the limit: two fresh pixels in every sampled line but ``special``, which holds the rest - more
        than that one."""
        n_sampled = ceil_div(L, stride)
        surplus = n_sampled * R // K('kUseShare') + 1 - 2 * (n_sampled - 1)
        assert 2 <= surplus <= R and special % stride == 0 and special < L

        def step(l, r):
            s = l % stride == 0
            return (s & (l != special) & (r == 1 + (l // stride) % (R - 1))) | ((l == special) & (r >= 1) & (r < surplus)) | (~s & light(l, r))
        return step

    # F = cap + 1 through the lines of the scan's later trips (their sampled lines stay light: the probe must vote yes)
    lines = np.arange(LA, dtype=np.int64)
    f_first = int(first_scan + np.count_nonzero(lines[:first_scan] % 3 != 0))
    n_late = LA - first_scan
    plain = n_late - ceil_div(n_late, stride)
    more = capacity(LA * R) + 1 - f_first - n_late
    base, rem = divmod(more, plain)
    assert 0 < base and base + 1 <= R - 1

    def a_over(l, r):
        o = (l - first_scan) - ((l - first_scan) // stride + 1)                 # the line's number among the later lines the probe skips
        n = base + (o < rem)
        return ((l < first_scan) & light(l, r)) | ((l >= first_scan) & (l % stride != 0) & (r >= 1) & (r <= n))

    RC = 130                                                 # three words, the last of two rows; 85 lines per batch
    CC = 10 * K('kExpandC') + 11                             # a ragged last tile of channels
    VC = ceil_div(trip_lines('gather', RC) + 15 * batch_lines(RC) + 1, CC)

    def c_runs(l, r):                                        # fresh runs across the word boundaries, as the small suites plant them
        m = (l + l // stride) % 8
        return (((m == 1) & (r >= 60) & (r < 70)) | ((m == 2) & (r >= 63) & (r < 65)) | ((m == 3) & (r == 63)) | ((m == 4) & (r == 64))
                | ((m == 5) & (r >= 126)) | ((m == 6) & (r == 128)) | ((m == 7) & (r >= 127) & (r < 129)))

    return [
        Case('A', (V, CA, R), light, 1, ('census', 'scan', 'gather', 'expand'),
             'probe trip 2 (valid and clamped unrolled items), scan trip 2, gather trip 3, census and expansion many trips'),
        Case('A-no', (V, CA, R), a_no, 0, (('probe', ('trips', 1)),),
             'the probe\'s trip 2 alone says no'),
        Case('A-edge', (V, CA, R), edge(LA, first_probe), 0, ('probe',),
             'the sample is one pixel over the limit; the first word of the probe\'s trip 2 holds more than that one'),
        Case('A-over', (V, CA, R), a_over, 0, ('scan',),
             'F = cap + 1 only through the scan\'s carry'),
        Case('B', (V, CB, R), light, 1, ('scan', ('scan', ('trips', 2))),
             'probe trip 3 and scan trip 3 (a vote of yes cannot depend on the probe\'s last words: B-edge pins them)'),
        Case('B-edge', (V, CB, R), edge(V * CB, 2 * first_probe), 0, (('probe', ('trips', 2)),),
             'the sample is one pixel over the limit; the first word of the probe\'s trip 3 holds more than that one'),
        Case('C', (VC, CC, RC), c_runs, 1, ('census', 'gather', 'expand'),
             'gather trip 2 with multi-line batches of multi-word lines, expansion trip 3'),
    ]


LARGE = {c.name: c for c in _large_cases()}
VOTES_NO = ('A-no', 'A-edge', 'B-edge')          # the cases whose sample says no: use = 0, F = 0


# ---- the small cases: fresh rows per line, for lines_of_fresh_rows -------------------------------------------------------------------

def reload_rows(C, R):
    """Fresh rows of C lines around the expansion's reload of its bit words (rows 4096, 8192) and the wrap of word_of_lane."""
    w = K('kWave') * K('kWordBits')
    edge = [w - 65, w - 64, w - 1, w, w + 1, 2 * w - 1, 2 * w]
    # (line 0, the only one where C = 1, repeats in rows 4096 and 8192: a word that holds row 4096 alone equals word 0 when that row is
    # fresh, and a stale word 0 in its place would go unnoticed)
    cycle = [[5, w - 1, 2 * w - 1], edge, range(w - 64, w + 64), [], [w], [w + 1, 2 * w], [1, 2, 3, w - 64, w + 63], [2 * w - 1]]
    return [[r for r in cycle[l % len(cycle)] if 0 < r < R] for l in range(C)]


def chunk_rows(L, R):
    """Fresh rows of L lines around the gather's chunks of kGatherWords words (rows 16384, 32768)."""
    w = K('kGatherWords') * K('kWordBits')
    cycle = [list(range(w - 4, w + 6)) + list(range(2 * w - 8, 2 * w + 7)), range(R - 70, R), [], [w - 1, w, 2 * w - 1, 2 * w], [w], range(w - 40, w + 1)]
    return [[r for r in cycle[l % len(cycle)] if 0 < r < R] for l in range(L)]


def small_sinogram(V, C, R, rows):
    step = np.zeros((V * C, R), dtype=bool)
    for l, rr in enumerate(rows):
        step[l, list(rr)] = True
    return Sinogram(V, C, R, step, large=False)


def _small_cases():
    w, g = K('kWave') * K('kWordBits'), K('kGatherWords') * K('kWordBits')
    out = {}
    for R in (w, w + 1, w + 64, 2 * w + 1):
        for C in (1, K('kExpandC') + 1):
            out[f'reload-R{R}-C{C}'] = ('expand_reload', (1, C, R), reload_rows(C, R))
    for R in (g, g + 1, g + 66, 2 * g + 1):
        for V in (1, 2):
            out[f'chunk-R{R}-V{V}'] = ('gather_chunk', (V, 3, R), chunk_rows(3 * V, R))
    return out


SMALL = _small_cases()            # name -> (the pass it targets, (V, C, R), fresh rows per line)


# ---- the model ------------------------------------------------------------------------------------------------------------------

MUTANT_KINDS = (('trips', 1), 'late')
MUTANTS = [(p, k) for p in PASSES for k in MUTANT_KINDS]          # two for each of the seven passes
M32 = np.uint64(0xFFFFFFFF)
KEPT = {0x00: -1, 0xFF: -2}       # an entry nobody wrote: what the fill left
PAD, OUTSIDE = -3, -4             # the list's pad (the count 1.0); a place or a pixel outside its array


def item_map(n, per_trip, kind):
    """src [n]: the work item each of the n work items reads; -1: it does not run."""
    src = np.arange(n, dtype=np.int64)
    if kind == 'late':
        src[per_trip:] += 1
        src[src >= n] = -1
    elif kind is not None:
        src[kind[1] * per_trip:] = -1
    return src


def take(values, src, kept):
    out = values[np.maximum(src, 0)]
    out[src < 0] = kept
    return out


def run(s, fill=0x00, mutant=None):
    """The route on the Sinogram ``s`` with every buffer pre-filled with ``fill`` -> ((use, F, cap), keys [L, R] or None where the
    direct launch ran: every pixel then has its own).  mutant: None or (pass, kind)."""
    name, kind = mutant if mutant else (None, None)
    kind_of = lambda p: kind if name == p else None
    L, R, C, V, cap = s.L, s.R, s.C, s.V, s.cap
    nw, waves = words_per_line(R), waves_per_block()
    word_fill = np.uint64(0 if fill == 0 else 0xFFFFFFFFFFFFFFFF)
    count_fill = np.uint64(0 if fill == 0 else 0xFFFFFFFF)
    per_word = np.bitwise_count(s.bits).astype(np.int64)
    # probe
    sampled = per_word[::K('kProbeStride')].reshape(-1)
    grid = min(K('kProbeMaxGrid'), ceil_div(sampled.size, waves * K('kProbeUnroll')))
    fresh = int(take(sampled, item_map(sampled.size, grid * waves * K('kProbeUnroll'), kind_of('probe')), 0).sum())
    if fresh * K('kUseShare') > ceil_div(L, K('kProbeStride')) * R:
        return (0, 0, cap), None
    # census
    src = item_map(L, min(K('kMaxGrid'), ceil_div(L, waves)) * waves, kind_of('census'))
    bits = take(s.bits, src, word_fill)
    counts = take(per_word.sum(axis=1).astype(np.uint64), src, count_fill)
    # block sums, their scan, F
    nb = ceil_div(L, K('kScanBlock'))
    blocks = np.zeros(nb * K('kScanBlock'), dtype=np.uint64)
    blocks[:L] = counts
    blocks = blocks.reshape(nb, K('kScanBlock'))
    sums = blocks.sum(axis=1) & M32
    src = item_map(nb, SCAN_TRIP_SUMS, kind_of('scan'))
    v = take(sums, src, np.uint64(0))
    nt = ceil_div(nb, SCAN_TRIP_SUMS)
    vt = np.zeros(nt * SCAN_TRIP_SUMS, dtype=np.uint64)
    vt[:nb] = v
    vt = vt.reshape(nt, SCAN_TRIP_SUMS)
    totals = vt.sum(axis=1) & M32
    carry = np.cumsum(totals) - totals
    ex = ((np.cumsum(vt, axis=1) - vt) & M32)
    scanned = ((((carry & M32)[:, None] + ex) & M32).reshape(-1))[:nb]
    sums = np.where(src >= 0, scanned, sums)
    F = int(totals.sum())
    if F > cap:
        return (0, F, cap), None
    bases = ((sums[:, None] + ((np.cumsum(blocks, axis=1) - blocks) & M32)) & M32).reshape(-1)[:L].astype(np.int64)
    # gather: which word each word of each batch reads
    batch = batch_lines(R)
    n_batches = ceil_div(L, batch)
    w = np.arange(L * nw, dtype=np.int64)
    b_own = (w // nw) // batch
    b_src = item_map(n_batches, min(K('kMaxGrid'), n_batches), kind_of('gather'))[b_own]
    word_src = np.where(b_src >= 0, w + (b_src - b_own) * batch * nw, -1)
    if name == 'gather_chunk' and batch == 1:                # the chunks of a line that is a batch by itself
        k_of = item_map(nw, K('kGatherWords'), kind)[w % nw]
        word_src = np.where(k_of >= 0, (w // nw) * nw + k_of, -1)
    word_src[word_src >= L * nw] = -1
    words = take(bits.reshape(-1), word_src, np.uint64(0))
    pos = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder='little'))
    w_own, bit = pos // 64, pos % 64
    b_of = (w_own // nw) // batch
    per_batch = np.bincount(b_of, minlength=n_batches)
    j = np.arange(pos.size, dtype=np.int64) - (np.cumsum(per_batch) - per_batch)[b_of]
    place = cap - F + bases[b_of * batch] + j
    ws = word_src[w_own]
    pixel = (ws // nw) * R + (ws % nw) * 64 + bit
    pixel[pixel >= s.n_pix] = OUTSIDE
    lst = np.full(cap, KEPT[fill], dtype=np.int64)
    pad_begin = (cap - F) // K('kTile') * K('kTile')
    lst[pad_begin:cap - F] = PAD
    ok = (place >= 0) & (place < cap)
    lst[place[ok]] = pixel[ok]
    # the Newton launch on the list's tiles from the pad on; the "result" of a pixel is its key
    results = np.full(cap, KEPT[fill], dtype=np.int64)
    results[pad_begin:] = lst[pad_begin:]
    flat_key = s.key.reshape(-1)
    results = np.where(results >= 0, flat_key[np.maximum(results, 0)], results)
    # expansion: the word in the registers for each tile of rows, the ranks, the places
    k_src = np.arange(nw, dtype=np.int64)
    if name == 'expand_reload' and nw > K('kWave'):
        wave, k = K('kWave'), np.arange(nw, dtype=np.int64)
        if kind == 'late':
            k_src = np.where(k >= wave, np.minimum(k // wave * wave + 1 + k % wave, nw - 1), k)
        else:
            k_src = np.where(k >= kind[1] * wave, (kind[1] - 1) * wave + k % wave, k)
    used = np.ascontiguousarray(bits[:, k_src])
    rank = np.cumsum(np.unpackbits(used.view(np.uint8).reshape(L, nw * 8), axis=1, bitorder='little')[:, :R], axis=1, dtype=np.int32)
    place = (cap - F) + bases[:, None] + rank - 1
    inside = (place >= 0) & (place < cap)
    read = np.where(inside, results[np.clip(place, 0, cap - 1)], OUTSIDE)
    # ... by columns of kExpandC channels
    e = K('kExpandC')
    tc = ceil_div(C, e)
    line = np.arange(L, dtype=np.int64)
    col = (line // C) * tc + (line % C) // e
    c_src = item_map(V * tc, min(K('kMaxGrid'), V * tc), kind_of('expand'))[col]
    line_src = np.where(c_src >= 0, (c_src // tc) * C + np.minimum((c_src % tc) * e + (line % C) % e, C - 1), -1)
    out = read[np.maximum(line_src, 0)]
    out[line_src < 0] = KEPT[fill]
    return (1, F, cap), out


def vacuous(s, mutant):
    """Whether the mutant does exactly what the kernels do on this shape (its pass stays inside one trip)."""
    name, kind = mutant
    n, per = items(name, s.V, s.C, s.R), trip_items(name, s.R)
    if name == 'expand_reload' and kind == 'late':            # the load beyond the line's last word is clamped to it
        nw = words_per_line(s.R)
        return nw <= per or all(min(k // per * per + 1 + k % per, nw - 1) == k for k in range(per, nw))
    return n <= per * (kind[1] if kind != 'late' else 1)


def rejected(s, fill, mutant):
    """Whether the comparison of the GPU suite tells the mutant from the route: the descriptor, or some pixel's key."""
    desc, keys = run(s, fill, mutant)
    if desc != s.expected():
        return True
    return keys is not None and not np.array_equal(keys, s.key)
