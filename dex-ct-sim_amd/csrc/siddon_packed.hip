// rows16_kernel: the stacked-fan traversal on a 2-BIT PACKED volume with bit-sliced counters (gfx950).
//
// Material ids of the fast path are < 4, so a voxel needs 2 bits, not 8.  dexct_volume_pack2 stores the z-fastest
// volume with four voxels per byte: column (x, y) is nz / 4 bytes, row z in bits 2(z % 16), 2(z % 16) + 1 of dword
// z / 16.  One dword load then serves SIXTEEN detector rows (rows4_kernel: four), the volume is a quarter of the bytes
// (a 1024^3 phantom is 256 MiB: it fits the Infinity Cache) and a (view, channel) pair of 1024 rows is one wave.
//
// Counting.  The loaded word x IS 32 one-bit flags: bit 2r = "row r sees id 1", bit 2r + 1 = "row r sees id 2" (ids
// 0, 1, 2).  n_1 and n_2 per row are therefore per-bit-position population counts over the slabs of the ray.  They are
// kept BIT-SLICED (Harley-Seal, sliced_count.h): words ones / twos / fours / eights hold bits 0..3 of the 32 counters,
// hi[0..6] bits 4..10.  (Id 3 sets both flags: with 4 ids - a full material group, or a 4-material phantom - a second
// set of counters runs on x & (x >> 1), the "both" flags at the even positions, and n_1 = n(bit 0) - n_3,
// n_2 = n(bit 1) - n_3.)  Sixteen loaded words are folded by fifteen carry-save adders (2 instructions each:
// v_bitop3_b32 for the majority and for the parity) and the one carry of weight 16 ripples into hi[] (10, two planes
// per step): 40 instructions per 16 dwords = 0.16 per row and slab against 0.75 (+ a v_readfirstlane per 4 rows) in
// rows4_kernel.  The crossing slabs go eight at a time (seven adders, a half adder, the ripple: 26 per 8).  The
// counters are un-sliced once per ray plane.
// Corrections (float32, in slab order, only where a crossing separates two materials) are applied per row exactly as
// in rows4_kernel, so per-material path lengths are bit-identical to every other kernel and to the oracle.
//
// Lanes: a pair of n_rows rows needs n_rows / 16 lanes.  For n_rows / 16 < 64 a wave carries 64 / (n_rows / 16)
// neighbouring channels of one view (per-lane pair index; each pair has its own slab lists in LDS and list entries
// beyond a pair's count point outside the buffer, which reads as air and counts nothing).
//
// Air columns.  A column (x, y) that is air over all z is a run of zero words: it adds nothing to a counter and never differs
// from another such column.  dexct_volume_air_columns marks these columns in a bit map (once per volume) and the SKIP forms of
// the kernel (dexct_siddon_project_packed_skip) enter no slab in their lists whose pieces all lie in marked columns: the sweeps
// get shorter, every sum keeps its bits (profiles/rows16_air_skip.md).
//
// Uniform columns.  A column that holds ONE id over all z - the water of an extruded cylinder, not only the air round it - adds
// the same word to every lane, so every slab in such columns adds the same integer to all the counters of a pair.
// dexct_volume_column_classes classes every column as mixed or uniform in an id (four bits per column, once per volume) and the
// noise-free SKIP forms (dexct_siddon_project_packed_uniform) also leave out the full slabs in uniform columns and the crossing
// slabs between two columns of the same id; each lane counts what it left out per id in one register, one sum over the pair's
// lanes follows the slab loop, and the pair's integers join every row's integer before it becomes a float.  The lists, their
// order, the sweeps, correct() and everything behind the un-slicing are what they were (uniform_count.h has the rule and the
// argument; profiles/rows16_uniform.md the measurements).  The same forms read an air map as a class map of air and mixed
// columns; the noisy SKIP forms keep the air rule.
#include "common.h"
#include "dedup_index.h"
#include "noise_sample.h"
#include "proj_host.h"
#include "sliced_count.h"
#include "tile_class.h"
#include "uniform_count.h"

namespace dexct {

static_assert(tiles::kFixFrac == DEXCT_FIX_FRAC, "the cells of a run are the cells of dda_slab");

constexpr int kP16Super = 128;      // slabs staged per pass
constexpr uint32_t kOob = 0xF0000000u;   // a list offset outside every buffer (< 3.75 GiB): the load returns 0 (air), no traffic
constexpr int kFullTrip = 16;       // full slabs per trip of their sweep (Sliced::add16)
constexpr int kCrossTrip = 8;       // crossing slabs per trip of theirs (Sliced::add8)
constexpr int kAirBatch = 2;         // classification iterations whose air-map lookups fly together (kP16Super / 64 = 2 at least)
static_assert(kP16Super % (kAirBatch * 64) == 0, "whole batches for every lane group");
static_assert(kP16Super % kFullTrip == 0 && kP16Super % kCrossTrip == 0, "the lists are padded to whole trips inside their LDS");
// LDS of a wave (= workgroup) that carries n_pairs pairs: their lists, and at least the staged store of the results (64 bytes per
// lane and spectrum), which reuses the lists' space
__host__ __device__ constexpr int p16_lds_bytes(int n_pairs) {
  const int lists = n_pairs * kP16Super * (int)(sizeof(CrossRec) + sizeof(uint32_t));
  return lists < 2 * 64 * 64 ? 2 * 64 * 64 : lists;
}
// Which SKIP forms take a column-class map (kernel and host agree through this): the noise-free ones, but for the unstaged
// three-material form.  That form sits at the 128 VGPRs of its four waves per SIMD and spilled 3 of them to scratch with the
// count in it; the noisy forms have no register to spare either (three materials: 127).  The forms left out keep the air rule.
__host__ __device__ constexpr bool p16_by_class(int n_materials, bool staged, bool noisy) {
  return !noisy && !(n_materials == 3 && !staged);
}
// what the list of distinct quads (dedup_index.h) keeps behind itself, in the last bytes of the wave's LDS - not in registers:
// the detection rounds have none to spare
struct DedupTail {
  float2 chord[4];       // (chord_u, len_per_u) of the wave's pairs
  int pair_end[4];       // [k], k < 3: entries of the pairs 0..k (an entry finds its pair by counting); [3]: entries in all
  uint32_t src[64];      // per lane, 8 bits per quad: the entry whose results the quad takes (< 192)
};

// GROUPED: a material-group pass (ids = codes 0..3 of one group of three materials): raw accumulators (units of u) go to
// acc_out[(mat_base + code) * n_rays + ray], no detection (dexct_siddon_project_grouped_packed).
// STAGED: results leave through LDS as whole lines (see below); the host picks it whenever it applies.
// NOISY (round 6; at most two spectra): the scan with quantum noise - the reference's live mode, spectra scaled to a dose
// (main.py:68,101).  The detection rounds accumulate the variance of the signal next to the signal (detect_energies<VAR>:
// the exponentials are shared) and, pa.sample, draw the sample in the registers that hold both (noise_sample.h: one Philox
// block per ray serves both spectra): what leaves the kernel is the noisy sinogram - no variance array, no pass over it.
// a.variance (optional) receives the variances as well (tests; callers that sample with dexct_add_noise).
// SKIP: the classification looks every slab up in the air-column map pa.col_air (dexct_siddon_project_packed_skip) and enters
// no slab that lies in all-air columns; the forms without it are the kernels as they were.
// TILES (the staged noise-free SKIP forms with a class map): runs of eight slabs whose tiles of the tile map (its address in
// pa.seed_lo / pa.seed_hi) are uniform in one id are dismissed before any of their slabs is classified (tile_class.h).  The tile forms are the instantiations
// with kTileForm added to MINW: a template parameter of their own would rename every other form of the kernel.
constexpr int kTileForm = 16;
template <int NM, int MINW_FORM = 4, bool GROUPED = false, bool STAGED = false, bool NOISY = false, bool SKIP = false>      // MINW: waves per SIMD the register allocation must allow
__global__ __launch_bounds__(64, MINW_FORM % kTileForm) void rows16_kernel(PackedArgs pa, const float* __restrict__ mu, const float* __restrict__ w,
                                                    const float* __restrict__ w2) {
  constexpr int MINW = MINW_FORM % kTileForm;
  constexpr bool TILES = MINW_FORM >= kTileForm;
  static_assert(MINW_FORM >= 1 && MINW_FORM < 2 * kTileForm && MINW >= 1 && MINW <= 8, "MINW_FORM is MINW (1 .. 8), or kTileForm + MINW");
  static_assert(NM >= 2 && NM <= 4, "ids 0..3");
  constexpr bool BOTH = NM > 3;              // id 3 exists: count the "both flags" plane too
  // detect_store<.., SHORT>: waves whose rays all miss the last material detect without it.  Not in the noisy three-material
  // form: its 127 VGPRs leave no room (with the second energy loop it spilled 4 - 7 VGPRs to scratch)
  constexpr bool kShort = !GROUPED && NM >= 3 && !(NOISY && NM == 3);
  extern __shared__ uint32_t lds_lists[];          // per pair: kP16Super crossing records (16 B), then kP16Super offsets
  const ProjArgs& a = pa.a;
  const int lane = threadIdx.x;
  BlockMasks bm{{~0ull, ~0ull}, false};
  if (!GROUPED) {
    bm = detect_block_masks(w, a.n_energies, a.n_spectra);      // all 64 lanes are here
    bm.use = bm.use && pa.det_masks;
    if (kShort) bm.drop_last = row_finite(mu + (size_t)(NM - 1) * a.n_energies, a.n_energies) && pa.det_absent;
  }
  const int lpp = pa.lanes_per_pair, n_pairs = 64 / lpp;
  CrossRec (*list_cross)[kP16Super] = reinterpret_cast<CrossRec (*)[kP16Super]>(lds_lists);
  uint32_t (*list_full)[kP16Super] = reinterpret_cast<uint32_t (*)[kP16Super]>(lds_lists + (size_t)n_pairs * kP16Super * 4);
  const int g = lane / lpp, li = lane - g * lpp;                 // this lane's pair and its index inside the pair
  // block -> (view, channel group, z-chunk): contiguous logical ids per XCD, views fastest inside a tile
  const int n_cg = (a.g.n_channels + n_pairs - 1) / n_pairs;
  const uint32_t nblk = gridDim.x, bid = blockIdx.x, per = nblk >> 3;
  const uint32_t logical = (bid < (per << 3)) ? (bid & 7u) * per + (bid >> 3) : bid;
  const uint32_t group = (uint32_t)pa.view_tile * n_cg * pa.n_zchunks;
  const uint32_t gq = logical / group, rem = logical - gq * group;
  const uint32_t views_here = min((uint32_t)pa.view_tile, (uint32_t)a.n_local_views - gq * pa.view_tile);
  const int zc = rem % pa.n_zchunks;
  const uint32_t qq = rem / pa.n_zchunks;
  const int v = gq * pa.view_tile + qq % views_here;
  const int c = (qq / views_here) * n_pairs + g;
  const bool pair_live = c < a.g.n_channels;
  dexct_ray_plan p;
  if (pair_live) p = a.plan[(size_t)v * a.g.n_channels + c];
  else { p.V0 = 0; p.SV = 0; p.i_first = 0; p.n_slabs = 0; p.kf = 0; p.len_per_u = 0; p.chord_u = 0; p.flags = 0; }
  const int axis = p.flags & 1u;
  const uint32_t smask = (p.flags & 2u) ? 0xFFFFFFFFu : 0u;
  const int nv = axis == 0 ? a.g.ny : a.g.nx;
  const uint32_t zb = (uint32_t)a.g.nz >> 2;                               // bytes per column
  const uint32_t su = (axis == 0 ? 1u : (uint32_t)a.g.nx) * zb;
  const uint32_t sv = (axis == 0 ? (uint32_t)a.g.nx : 1u) * zb;
  const int r0 = (zc * 64 + li) * 16;                                      // first of this lane's 16 rows
  // byte offset of the lane's dword inside a column; lanes past the last row read the last dword and store nothing
  const uint32_t zoff = (uint32_t)min((a.g.z_first + r0) >> 2, (int)zb - 4);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(pa.vol_z2), 0, (int)((size_t)a.g.nx * a.g.ny * zb), 0x00020000);
  auto ld16 = [&](uint32_t off) {           // off + zoff beyond the buffer (list padding, edge pieces): 0, no access
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(off + zoff), 0, 0);
  };
  Sliced cnt, cnt3;                          // cnt3: flags of id 3 at the even bit positions (BOTH only)
  float corr[NM - 1][16];                    // [material - 1][row]
#pragma unroll
  for (int m = 0; m < NM - 1; ++m)
#pragma unroll
    for (int q = 0; q < 16; ++q) corr[m][q] = 0.0f;
  auto correct = [&](uint32_t xa, uint32_t xb, float t) {
    const uint32_t d = xa ^ xb;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      if ((d >> (2 * rr)) & 3u) {
        const uint32_t ia = (xa >> (2 * rr)) & 3u, ib = (xb >> (2 * rr)) & 3u;
#pragma unroll
        for (int m = 1; m < NM; ++m) {
          corr[m - 1][rr] += (ia == (uint32_t)m) ? t : 0.0f;
          corr[m - 1][rr] -= (ib == (uint32_t)m) ? t : 0.0f;
        }
      }
    }
  };
  // the longest ray of the wave sets the trip count (wave-uniform)
  int n_slabs_max = 0;
  for (int k = 0; k < n_pairs; ++k) n_slabs_max = max(n_slabs_max, __builtin_amdgcn_readlane(p.n_slabs, k * lpp));
  const unsigned long long group_mask = (lpp == 64 ? ~0ull : ((1ull << lpp) - 1ull)) << (g * lpp);
  const unsigned long long below_mask = group_mask & ((1ull << lane) - 1ull);
  static_assert(!(GROUPED && SKIP), "the group passes take no map");
  // the noise-free SKIP forms class columns as mixed or uniform in an id (a class map; an air map read as one) and count the
  // slabs they leave out, per id.  The other SKIP forms keep the air rule and the code they had (p16_by_class).
  constexpr bool kByClass = SKIP && p16_by_class(NM, STAGED, NOISY);
  uint32_t dropped = 0u;                     // this lane's dropped slabs (ucount::bump), over all passes
  // TILES: the slabs are not taken 128 at a time.  Phase 1 (run trips, before the passes): a lane takes one RUN of its pair - the
  // up to eight slabs of one tile row - finds the cells of its first and last piece (the cells between are the other pieces': j
  // is monotone in the slab) and reads the at most three tiles they span, consecutive nibbles of one row of the tile map; a run
  // whose tiles are all uniform in one id is dismissed and counted in `dropped` with all its slabs, which is what the slab rule
  // would have done one slab at a time (tile_class.h has the argument).  One ballot per trip gives each pair's surviving runs; a
  // ray has at most tiles::kWindow = 64 runs (the host launches these forms for grids up to 512 x 512 only), so a pair's
  // surviving runs are ONE 64-bit mask, and the number of passes is known before the first: the pass loop stays a counted loop.
  // (A pass loop that ended on the mask - runs left or not - cost the benchmark form 50 VGPRs spilled to scratch: the sums
  // `corr` went to scratch round every classification.)  Phase 2 (passes): the next 16 surviving runs of every pair are 128 fine
  // slabs, in slab order; lane li < 16 finds the li-th of them in the mask and fine slab f takes run f / 8 from that lane.  From
  // there on the classification, the lists and the sweeps are those of the lean loop below: the same slabs reach the lists in
  // the same order.
  static_assert(!TILES || (SKIP && STAGED && !NOISY && kByClass), "the tile forms: staged, noise-free, with a class map");
  [[maybe_unused]] unsigned long long alive_runs = 0ull;       // TILES: bit r = run r of this lane's pair survived
  [[maybe_unused]] int n_passes = 0;
  if constexpr (TILES) {
    static_assert(tiles::kFineSlabs == kP16Super && tiles::kRunsPerPass <= 16, "a pass fills the lists; its runs fit a pair's lanes");
    const tiles::Layout ty = tiles::layout((uint32_t)a.g.nx, (uint32_t)a.g.ny);
    // Both words of a run are read through this bounds-checked buffer of exactly the map's words, each at its own VECTOR offset (the
    // range check covers the vector and the immediate offset, not the scalar one).  A lane without a run (have == false: tile rows
    // R >= ti, whose nibbles lie in or behind the spare word) and a plan that leaves the grid along the slab axis read behind the
    // map: 0 without an access (tiles::checked_word on the host) - mixed, and the run of a lane that has one survives.
    const __amdgpu_buffer_rsrc_t tile_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<uint32_t*>((uintptr_t)pa.seed_lo | (uintptr_t)pa.seed_hi << 32), 0, (int)(4u * ty.words), 0x00020000);
    const uint32_t tj = axis == 0 ? ty.tj[0] : ty.tj[1], copy_at = axis == 0 ? ty.first_nibble[0] : ty.first_nibble[1];
    const int R0 = tiles::first_run(p.i_first), n_runs = tiles::n_runs(p.i_first, p.n_slabs);
    int n_runs_max = 0;
    for (int k = 0; k < n_pairs; ++k) n_runs_max = max(n_runs_max, __builtin_amdgcn_readlane(n_runs, k * lpp));
    for (int t0 = 0; t0 < tiles::kWindow && t0 < n_runs_max; t0 += lpp) {
      const int r = t0 + li, R = R0 + r;
      const bool have = r < n_runs;
      const int i_lo = tiles::run_i_lo(R, p.i_first), i_hi = tiles::run_i_hi(R, p.i_first, p.n_slabs);
      const int j0 = tiles::cell_of(p.V0, p.SV, i_lo), j1 = tiles::cell_of(p.V0, p.SV, i_hi + 1);
      const int J_lo = tiles::tile_of_cell(min(j0, j1), tj), J_hi = tiles::tile_of_cell(max(j0, j1), tj);
      const uint32_t nib = tiles::nibble_at(copy_at, tj, (uint32_t)R, J_lo);
      const uint32_t w_lo = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(tile_rsrc, (int)(tiles::word_of_nibble(nib) << 2), 0, 0);
      const uint32_t w_hi = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(tile_rsrc, (int)((tiles::word_of_nibble(nib) + 1u) << 2), 0, 0);
      const uint32_t e = tiles::dismissed_in(tiles::nibbles_from(w_lo, w_hi, nib), J_hi - J_lo + 1);
      dropped += have ? tiles::bump_run(e, i_hi - i_lo + 1) : 0u;
      const unsigned long long alive = __ballot(have && e == 0u);
      alive_runs |= ((alive & group_mask) >> (g * lpp)) << t0;
    }
    int most = 0;
    for (int k = 0; k < n_pairs; ++k) most = max(most, __builtin_amdgcn_readlane((int)__popcll(alive_runs), k * lpp));
    n_passes = (most + tiles::kRunsPerPass - 1) / tiles::kRunsPerPass;
  }
  // a pass: the next 128 slabs of the wave's rays - TILES: the next 16 surviving runs of its pairs
  for (int s0 = 0; s0 < (TILES ? n_passes * kP16Super : n_slabs_max); s0 += kP16Super) {
    // ---- geometry: the lanes of a pair classify its slabs s0 + li, s0 + li + lpp, ... (slab order kept per pair)
    int run_f = 0, run_c = 0;               // per pair (identical in all lanes of a pair)
    // SKIP: the same classification as below, kAirBatch iterations at a time so that their map words are in
    // flight together, and a slab whose pieces inside the grid all lie in all-air columns is entered in neither list.  Its
    // words are 0: they add nothing to a counter and two equal words cause no correction, so every sum keeps its bits; the
    // slabs that stay keep their order.  A crossing slab with one air piece stays (its count and its correction are needed).
    // The offsets are column index x zb: the same integers as i * su + j * sv.
    // kByClass (the noise-free SKIP forms): the map is of either kind (uniform_count.h: one lookup for both) and a slab also
    // leaves when both its pieces lie in columns uniform in the same id; the lane counts it in `dropped` (one field per id).
    // The argument why every output keeps its bytes stands in uniform_count.h.
    // kLeanClass (the staged noise-free SKIP forms; the others keep the loop below as it was - the unstaged three-material form
    // spilled 2 VGPRs to scratch with the first two changes): the same classification, the same lists, with less work per slab.
    //   - The trips end with the slots that can hold a slab of the wave's longest ray (whole batches; wave-uniform): the last
    //     pass of a 446-slab ray has 62 live slots of 128, and the padding and the sweeps below cope with short lists anyway.
    //   - The slab coordinate V0 + (i_first + s) SV is formed once per pass and lane, for the lane's first slab, and moves on by
    //     lpp SV per iteration: the same integer modulo 2^64 as the product per slab.
    //   - The slab geometry runs without a branch (a lane without a slab has no piece inside: `have`), and the column index
    //     i cu + j cv is formed with 24-bit multiplies (i < 2^13, j < nv <= 2047 for a piece inside, cu, cv <= 2047; the index
    //     of a piece outside is not used).
    //   - The map is read through a bounds-checked buffer of exactly its words: an index beyond it - a piece outside the grid,
    //     whose word is ignored anyway - returns 0 without an access, so no index is clamped or replaced.  A piece outside the
    //     grid classes as air through ina / inb as before, never through the word.
    //   - The offsets col x zb are formed only where a slab is written to a list.
    constexpr bool kLeanClass = SKIP && STAGED && !NOISY;
    if constexpr (TILES) {
      const uint32_t cu = axis == 0 ? 1u : (uint32_t)a.g.nx, cv = axis == 0 ? (uint32_t)a.g.nx : 1u;
      constexpr ucount::MapKind mk = ucount::map_kind(true);
      const __amdgpu_buffer_rsrc_t map_rsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint32_t*>(pa.col_air), 0, (int)(4u * ucount::map_words((uint32_t)a.g.nx * (uint32_t)a.g.ny, mk)), 0x00020000);
      // the pass's runs: lane li < 16 holds the li-th of them, by its rank among the pair's surviving runs (64: none)
      const int first = tiles::kRunsPerPass * (s0 / kP16Super);
      const int n_mine = min(tiles::kRunsPerPass, max(0, (int)__popcll(alive_runs) - first));
      const int mine = li < n_mine ? tiles::surviving_run(alive_runs, first + li) : tiles::kWindow;
      int n_taken = 0;
      for (int k = 0; k < n_pairs; ++k) n_taken = max(n_taken, __builtin_amdgcn_readlane(n_mine, k * lpp));
      const int q_end = min(kP16Super, (tiles::kSide * n_taken + kAirBatch * lpp - 1) & ~(kAirBatch * lpp - 1));
      for (int q0 = 0; q0 < q_end; q0 += kAirBatch * lpp) {
        uint32_t cola[kAirBatch], colb[kAirBatch], wa[kAirBatch], wb[kAirBatch];
        float tt[kAirBatch];
        bool ina[kAirBatch], inb[kAirBatch], one[kAirBatch];
#pragma unroll
        for (int u = 0; u < kAirBatch; ++u) {
          // fine slab f of the pass: slab f % 8 of the pair's (f / 8)-th run; the rest is the lean loop's
          const int f = q0 + u * lpp + li;
          const int run = __shfl(mine, g * lpp + tiles::fine_rank(f));
          const int i = ((tiles::first_run(p.i_first) + run) << tiles::kShift) + tiles::fine_slab(f);
          const bool have = tiles::fine_rank(f) < n_mine && (uint32_t)(i - p.i_first) < (uint32_t)p.n_slabs;
          const SlabPieces sp = dda_slab((long long)((unsigned long long)p.V0 + (unsigned long long)((long long)i * p.SV)), p.SV, smask, p.kf);
          ina[u] = have && (uint32_t)sp.ja < (uint32_t)nv;
          inb[u] = have && (uint32_t)sp.jb < (uint32_t)nv;
          const uint32_t icu = __umul24((uint32_t)i, cu);
          cola[u] = icu + __umul24((uint32_t)sp.ja, cv);
          colb[u] = icu + __umul24((uint32_t)sp.jb, cv);
          one[u] = sp.ja == sp.jb;
          tt[u] = sp.t;
          wa[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(map_rsrc, (int)(ucount::word_of(cola[u], mk) << 2), 0, 0);
          wb[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(map_rsrc, (int)(ucount::word_of(colb[u], mk) << 2), 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kAirBatch; ++u) {
          const uint32_t ea = ina[u] ? ucount::class_in(wa[u], cola[u], mk) : ucount::kAirClass;
          const uint32_t eb = inb[u] ? ucount::class_in(wb[u], colb[u], mk) : ucount::kAirClass;
          const bool keep = !ucount::droppable(ea, eb);
          dropped += keep ? 0u : ucount::bump(eb);
          const bool whole = ina[u] && inb[u] && one[u];
          const bool is_full = whole && keep, is_cross = !whole && (ina[u] || inb[u]) && keep;
          const unsigned long long mf = __ballot(is_full), mc = __ballot(is_cross);
          if (is_full) list_full[g][run_f + __popcll(mf & below_mask)] = colb[u] * zb;
          if (is_cross)
            list_cross[g][run_c + __popcll(mc & below_mask)] = CrossRec{ina[u] ? cola[u] * zb : kOob, inb[u] ? colb[u] * zb : kOob, tt[u], 0u};
          run_f += __popcll(mf & group_mask);
          run_c += __popcll(mc & group_mask);
        }
      }
    } else if constexpr (kLeanClass) {
      const uint32_t cu = axis == 0 ? 1u : (uint32_t)a.g.nx, cv = axis == 0 ? (uint32_t)a.g.nx : 1u;
      const ucount::MapKind mk = ucount::map_kind(pa.col_class != 0);       // (wave-uniform)
      const __amdgpu_buffer_rsrc_t map_rsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint32_t*>(pa.col_air), 0, (int)(4u * ucount::map_words((uint32_t)a.g.nx * (uint32_t)a.g.ny, mk)), 0x00020000);
      const int q_end = min(kP16Super, (n_slabs_max - s0 + kAirBatch * lpp - 1) & ~(kAirBatch * lpp - 1));
      unsigned long long va_next = (unsigned long long)p.V0 + (unsigned long long)((long long)(p.i_first + s0 + li) * p.SV);
      const unsigned long long va_step = (unsigned long long)p.SV * (unsigned long long)lpp;
      for (int q0 = 0; q0 < q_end; q0 += kAirBatch * lpp) {
        uint32_t cola[kAirBatch], colb[kAirBatch], wa[kAirBatch], wb[kAirBatch];
        float tt[kAirBatch];
        bool ina[kAirBatch], inb[kAirBatch], one[kAirBatch];          // one: both pieces in the same column
#pragma unroll
        for (int u = 0; u < kAirBatch; ++u) {
          const int s = s0 + q0 + u * lpp + li;
          const bool have = s < p.n_slabs;
          const SlabPieces sp = dda_slab((long long)va_next, p.SV, smask, p.kf);
          va_next += va_step;
          ina[u] = have && (uint32_t)sp.ja < (uint32_t)nv;
          inb[u] = have && (uint32_t)sp.jb < (uint32_t)nv;
          const uint32_t icu = __umul24((uint32_t)(p.i_first + s), cu);
          cola[u] = icu + __umul24((uint32_t)sp.ja, cv);
          colb[u] = icu + __umul24((uint32_t)sp.jb, cv);
          one[u] = sp.ja == sp.jb;
          tt[u] = sp.t;
          wa[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(map_rsrc, (int)(ucount::word_of(cola[u], mk) << 2), 0, 0);
          wb[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(map_rsrc, (int)(ucount::word_of(colb[u], mk) << 2), 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kAirBatch; ++u) {
          // (a lane without a slab has no piece inside: air on both sides, dropped, and air counts nothing)
          const uint32_t ea = ina[u] ? ucount::class_in(wa[u], cola[u], mk) : ucount::kAirClass;
          const uint32_t eb = inb[u] ? ucount::class_in(wb[u], colb[u], mk) : ucount::kAirClass;
          const bool keep = !ucount::droppable(ea, eb);
          dropped += keep ? 0u : ucount::bump(eb);
          const bool whole = ina[u] && inb[u] && one[u];
          const bool is_full = whole && keep, is_cross = !whole && (ina[u] || inb[u]) && keep;
          const unsigned long long mf = __ballot(is_full), mc = __ballot(is_cross);
          if (is_full) list_full[g][run_f + __popcll(mf & below_mask)] = colb[u] * zb;
          if (is_cross)
            list_cross[g][run_c + __popcll(mc & below_mask)] = CrossRec{ina[u] ? cola[u] * zb : kOob, inb[u] ? colb[u] * zb : kOob, tt[u], 0u};
          run_f += __popcll(mf & group_mask);
          run_c += __popcll(mc & group_mask);
        }
      }
    }
    for (int q0 = 0; SKIP && !kLeanClass && q0 < kP16Super; q0 += kAirBatch * lpp) {
      const uint32_t cu = axis == 0 ? 1u : (uint32_t)a.g.nx, cv = axis == 0 ? (uint32_t)a.g.nx : 1u;
      const ucount::MapKind mk = ucount::map_kind(kByClass && pa.col_class != 0);       // (wave-uniform)
      const uint32_t last_word = ((uint32_t)a.g.nx * (uint32_t)a.g.ny - 1u) >> (kByClass ? mk.word_shift : 5u);
      uint32_t cola[kAirBatch], colb[kAirBatch], wa[kAirBatch], wb[kAirBatch];
      float tt[kAirBatch];
      bool ina[kAirBatch], inb[kAirBatch], one[kAirBatch];          // one: both pieces in the same column
#pragma unroll
      for (int u = 0; u < kAirBatch; ++u) {
        const int s = s0 + q0 + u * lpp + li;
        cola[u] = colb[u] = 0u;
        tt[u] = 0.0f;
        ina[u] = inb[u] = one[u] = false;
        if (s < p.n_slabs) {
          const int i = p.i_first + s;
          const SlabPieces sp = dda_slab(p.V0 + (long long)i * p.SV, p.SV, smask, p.kf);
          ina[u] = (uint32_t)sp.ja < (uint32_t)nv;
          inb[u] = (uint32_t)sp.jb < (uint32_t)nv;
          cola[u] = (uint32_t)i * cu + (uint32_t)sp.ja * cv;
          colb[u] = (uint32_t)i * cu + (uint32_t)sp.jb * cv;
          one[u] = sp.ja == sp.jb;
          tt[u] = sp.t;
        }
        // (a piece outside the grid, and a lane without a slab, look at word 0 and ignore it; the map is read through a plain
        // pointer, not a bounds-checked buffer, so the word index is held inside it whatever the plan says)
        if constexpr (kByClass) {
          wa[u] = pa.col_air[ina[u] ? min(ucount::word_of(cola[u], mk), last_word) : 0u];
          wb[u] = pa.col_air[inb[u] ? min(ucount::word_of(colb[u], mk), last_word) : 0u];
        } else {
          wa[u] = pa.col_air[ina[u] ? min(cola[u] >> 5, last_word) : 0u];
          wb[u] = pa.col_air[inb[u] ? min(colb[u] >> 5, last_word) : 0u];
        }
      }
#pragma unroll
      for (int u = 0; u < kAirBatch; ++u) {
        bool keep;
        if constexpr (kByClass) {
          // (a lane without a slab has no piece inside: air on both sides, dropped, and air counts nothing)
          const uint32_t ea = ina[u] ? ucount::class_in(wa[u], cola[u], mk) : ucount::kAirClass;
          const uint32_t eb = inb[u] ? ucount::class_in(wb[u], colb[u], mk) : ucount::kAirClass;
          keep = !ucount::droppable(ea, eb);
          dropped += keep ? 0u : ucount::bump(eb);
        } else {
          const bool air_a = !ina[u] || ((wa[u] >> (cola[u] & 31u)) & 1u), air_b = !inb[u] || ((wb[u] >> (colb[u] & 31u)) & 1u);
          keep = !(air_a && air_b);
        }
        const bool whole = ina[u] && inb[u] && one[u];
        const bool is_full = whole && keep, is_cross = !whole && (ina[u] || inb[u]) && keep;
        const uint32_t offa = ina[u] ? cola[u] * zb : kOob, offb = inb[u] ? colb[u] * zb : kOob;
        const unsigned long long mf = __ballot(is_full), mc = __ballot(is_cross);
        if (is_full) list_full[g][run_f + __popcll(mf & below_mask)] = offb;
        if (is_cross) list_cross[g][run_c + __popcll(mc & below_mask)] = CrossRec{offa, offb, tt[u], 0u};
        run_f += __popcll(mf & group_mask);
        run_c += __popcll(mc & group_mask);
      }
    }
    for (int q0 = 0; !SKIP && q0 < kP16Super; q0 += lpp) {
      const int s = s0 + q0 + li;
      bool is_full = false, is_cross = false;
      uint32_t offa = kOob, offb = kOob;
      float tt = 0.0f;
      if (s < p.n_slabs) {
        const int i = p.i_first + s;
        const SlabPieces sp = dda_slab(p.V0 + (long long)i * p.SV, p.SV, smask, p.kf);
        const bool ina = (uint32_t)sp.ja < (uint32_t)nv, inb = (uint32_t)sp.jb < (uint32_t)nv;
        if (ina) offa = (uint32_t)i * su + (uint32_t)sp.ja * sv;
        if (inb) offb = (uint32_t)i * su + (uint32_t)sp.jb * sv;
        tt = sp.t;
        is_full = ina && inb && sp.ja == sp.jb;
        // everything else that touches the grid goes to the crossing list: a piece outside the grid keeps kOob and
        // reads as air, which is what the edge slabs of rows4_kernel do (count b, correct against id 0)
        is_cross = !is_full && (ina || inb);
      }
      const unsigned long long mf = __ballot(is_full), mc = __ballot(is_cross);
      if (is_full) list_full[g][run_f + __popcll(mf & below_mask)] = offb;
      if (is_cross) list_cross[g][run_c + __popcll(mc & below_mask)] = CrossRec{offa, offb, tt, 0u};
      run_f += __popcll(mf & group_mask);
      run_c += __popcll(mc & group_mask);
    }
    // pad each pair's lists to the wave's longest (whole batches), so that the sweeps below need no per-pair bounds
    int n_full = 0, n_cross = 0;
    for (int k = 0; k < n_pairs; ++k) {
      n_full = max(n_full, __builtin_amdgcn_readlane(run_f, k * lpp));
      n_cross = max(n_cross, __builtin_amdgcn_readlane(run_c, k * lpp));
    }
    n_full = (n_full + kFullTrip - 1) & ~(kFullTrip - 1);
    n_cross = (n_cross + kCrossTrip - 1) & ~(kCrossTrip - 1);
    for (int k = run_f + li; k < n_full; k += lpp) list_full[g][k] = kOob;
    for (int k = run_c + li; k < n_cross; k += lpp) list_cross[g][k] = CrossRec{kOob, kOob, 0.0f, 0u};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // ---- full slabs: 16 dword loads (16 rows each) in flight, fifteen carry-save adders and one ripple
    for (int k = 0; k < n_full; k += kFullTrip) {
      uint32_t x[kFullTrip];
#pragma unroll
      for (int q = 0; q < kFullTrip; ++q) x[q] = ld16(list_full[g][k + q]);
      __builtin_amdgcn_sched_barrier(0);
      cnt.add16(x);
      if (BOTH) {
        uint32_t b[kFullTrip];
#pragma unroll
        for (int q = 0; q < kFullTrip; ++q) b[q] = x[q] & (x[q] >> 1);
        cnt3.add16(b);
      }
    }
    // ---- crossing slabs (and the edge slabs): count the b voxel, correct where the two voxels differ (in slab order)
    for (int k = 0; k < n_cross; k += kCrossTrip) {
      uint32_t xa[kCrossTrip], xb[kCrossTrip];
      float t8[kCrossTrip];
#pragma unroll
      for (int j = 0; j < kCrossTrip; ++j) {
        const CrossRec q = list_cross[g][k + j];
        xa[j] = ld16(q.offa);
        xb[j] = ld16(q.offb);
        t8[j] = q.t;
      }
      __builtin_amdgcn_sched_barrier(0);
      cnt.add8(xb);
      if (BOTH) {
        uint32_t b[kCrossTrip];
#pragma unroll
        for (int j = 0; j < kCrossTrip; ++j) b[j] = xb[j] & (xb[j] >> 1);
        cnt3.add8(b);
      }
      uint32_t any = 0;
#pragma unroll
      for (int j = 0; j < kCrossTrip; ++j) any |= xa[j] ^ xb[j];
      if (any) {
#pragma unroll
        for (int j = 0; j < kCrossTrip; ++j)
          if (xa[j] != xb[j]) correct(xa[j], xb[j], t8[j]);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // kByClass: ONE sum over the lanes of each pair (all 64 lanes are here; a pair is an aligned power of two of them) gives the
  // pair's dropped slabs per id, and from them what the sweeps would have added to every row's counter of each flag plane:
  // id 1 sets plane 0, id 2 plane 1, id 3 both and the "both" plane.
  uint32_t drop0 = 0u, drop1 = 0u, drop3 = 0u;
  if constexpr (kByClass) {
    uint32_t lo = ucount::spread_lo(dropped), mid = ucount::spread_mid(dropped);
    for (int d = 1; d < lpp; d <<= 1) {
      lo += (uint32_t)__shfl_xor((int)lo, d);
      mid += (uint32_t)__shfl_xor((int)mid, d);
    }
    drop3 = lo >> 16;
    drop0 = (lo & 0xFFFFu) + drop3;
    drop1 = mid + drop3;
    // (the un-slicing below holds up to 64 words: it must not be drawn up between the shuffles to hide their latency)
    __builtin_amdgcn_sched_barrier(0);
  }
  // STAGED (the usual case: row-fastest output, whole groups of 4 rows, one or two spectra): each detection round leaves
  // its results in LDS and the wave stores them at the end, so that one store instruction writes 1 KiB of consecutive
  // addresses (whole lines) instead of 64 separate 16-byte pieces per round - every lane's 64 output bytes used to
  // leave as four partial writes (WRITE_SIZE 2.1x the output bytes).  All lanes then stay to the end, because a lane
  // also stores pieces of other lanes.
  constexpr int kResSlots = 2;               // spectra whose results the stage holds
  static_assert(!(GROUPED && STAGED), "group passes hand over raw accumulators");
  static_assert(!(GROUPED && NOISY), "group passes hand over raw accumulators");
  constexpr bool staged = STAGED;            // host: layout 1, n_rows % 4 == 0, n_spectra <= kResSlots
  const bool lane_live = pair_live && r0 < a.g.n_rows;
  if (!staged && !lane_live) return;
  // (STAGED: lanes without rows of their own run the code below too, on counters that saw nothing but air - branching
  // around it per lane made the detection loops divergent in the compiler's eyes, and the tables then arrived by vector
  // loads instead of through the scalar cache: +23 %)
  // ---- un-slice the counters (in place of the corrections), then detect 4 rows at a time.  The rounds are a real
  // loop with ONE copy of the detection code (rows move down the register array between rounds): four inlined copies
  // made the kernel as large as the instruction cache two CUs share.
  {
    // the sums are formed exactly as in rows4_kernel: (float) count + corrections
    uint32_t n[32], n3[32];
    cnt.unslice(n);
    if (BOTH) cnt3.unslice(n3);
#pragma unroll
    for (int row = 0; row < 16; ++row) {
      if constexpr (kByClass) {                // the dropped slabs join the integers they were left out of, before the conversion
        n[2 * row] += drop0;
        n[2 * row + 1] += drop1;
        if (BOTH) n3[2 * row] += drop3;
      }
      if (BOTH) {
        corr[0][row] = (float)(int32_t)(n[2 * row] - n3[2 * row]) + corr[0][row];
        corr[1][row] = (float)(int32_t)(n[2 * row + 1] - n3[2 * row]) + corr[1][row];
        corr[2][row] = (float)(int32_t)n3[2 * row] + corr[2][row];
      } else {
        corr[0][row] = (float)(int32_t)n[2 * row] + corr[0][row];
        if (NM > 2) corr[1][row] = (float)(int32_t)n[2 * row + 1] + corr[1][row];
      }
    }
  }
  if (GROUPED) {         // hand the raw accumulators to the detection kernel, one plane per material of the group
    if (!lane_live) return;
    const size_t n_rays = (size_t)a.n_local_views * a.g.n_rows * a.g.n_channels;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int r = r0 + 4 * q4;
      if (r >= a.g.n_rows) break;
      const bool vec4 = a.layout == 1 && (a.g.n_rows & 3) == 0;
#pragma unroll
      for (int m = 1; m < NM; ++m) {
        float* plane = a.acc_out + (size_t)(a.mat_base + m) * n_rays;
        if (vec4) {
          *reinterpret_cast<float4*>(plane + ray_index(a, v, r, c)) =
              make_float4(corr[m - 1][4 * q4], corr[m - 1][4 * q4 + 1], corr[m - 1][4 * q4 + 2], corr[m - 1][4 * q4 + 3]);
        } else {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            if (r + rr < a.g.n_rows) plane[ray_index(a, v, r + rr, c)] = corr[m - 1][4 * q4 + rr];
        }
      }
    }
    return;
  }
  // ---- Distinct quads (the staged noise-free forms; pa.det_dedup).  The counts of a ray are a function of its sums and of its
  // pair's chord, and in a stacked fan the rows of a pair cross the same slabs: rows whose columns carry the same ids along the
  // ray have bitwise equal sums (an extruded part of the object, the water above and below an insert).  A quad = a lane's four
  // rows of one round; it is FRESH when a sum differs bitwise from the same row of the quad before it in the pair (the same
  // lane's round before, for round 0 the last round of the lane below; a pair's first quad always is).  The fresh quads go to a
  // list in LDS (the slab lists are dead: the space the staged store reuses too), lane j of round k detects entry 64 k + j and
  // writes the results over it, and every quad then takes the results of the last fresh quad at or before it into the stage.
  // Where the list saves no round (dedup::use_list: wave-uniform) the rounds run on the rows as they always did.
  // (Not in the two-material form without the air-column map: it fits the 96 VGPRs of a fifth wave per SIMD, and with the list
  // in it it took 99, or 96 with 3 of them spilled to scratch; its SKIP form runs four waves either way and has the list.)
  constexpr bool kDedup = STAGED && !NOISY && !GROUPED && !(NM == 2 && !SKIP);
  constexpr int kEntry = dedup::entry_bytes(NM);
  constexpr int kNarrowRows = 2;             // the narrowest list round built: lists of at most 16 entries take the two-row round too
  constexpr bool kNarrow = kDedup && MINW == (NM == 4 ? 3 : 4);      // (the DEXCT_P16_MINW forms keep four-row rounds: A/B forms)
  int list_rounds = 0;                       // > 0: the wave detects its list, in so many rounds
  int list_fresh = 0;                        // entries of that list (wave-uniform: popcounts of ballots)
  auto dedup_tail = [&]() { return reinterpret_cast<DedupTail*>(reinterpret_cast<uint8_t*>(lds_lists) + p16_lds_bytes(n_pairs) - sizeof(DedupTail)); };
  float chord_u = p.chord_u, len_per_u = p.len_per_u;
  if constexpr (kDedup) {
    if (pa.det_dedup) {
      // (lpp is a power of two; the lane's place in its pair is taken from the lane, not kept from the traversal)
      const bool pair_first = (lane & (lpp - 1)) == 0;
      int live_rounds = 0, n_fresh = 0, below = 0;        // below: fresh quads (of all rounds) in the lanes below this one
      uint32_t own = 0;                                    // bit q: quad (lane, q) is fresh
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bool diff = q == 0 && pair_first;
#pragma unroll
        for (int m = 0; m < NM - 1; ++m)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const uint32_t mine = __float_as_uint(corr[m][4 * q + rr]);
            // (every lane takes part in the shuffle; lane 0 reads itself and is the first of its pair)
            const uint32_t prev = q == 0 ? (uint32_t)__shfl_up((int)__float_as_uint(corr[m][12 + rr]), 1) : __float_as_uint(corr[m][4 * q - 4 + rr]);
            diff |= mine != prev;
          }
        const bool live_q = lane_live && r0 + 4 * q < a.g.n_rows;
        const unsigned long long fresh_q = __ballot(diff && live_q);
        own |= (diff && live_q) ? 1u << q : 0u;
        below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(fresh_q >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fresh_q, (uint32_t)below));
        n_fresh += __popcll(fresh_q);
        live_rounds += __ballot(live_q) != 0ull ? 1 : 0;
      }
      if (dedup::use_list(n_fresh, live_rounds, NM, p16_lds_bytes(n_pairs), (int)sizeof(DedupTail))) {
        list_rounds = dedup::list_rounds(n_fresh);
        list_fresh = n_fresh;
        if (a.pathlen) {             // (test output) per ray, as the rounds write it: the rows go once round the register array
#pragma unroll 1
          for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int r = r0 + 4 * q4 + rr;
              float others = 0.0f;
#pragma unroll
              for (int m = 1; m < NM; ++m) others += corr[m - 1][rr];
              if (lane_live && r < a.g.n_rows) {
                float* pl = a.pathlen + ray_index(a, v, r, c) * NM;
                pl[0] = (p.chord_u - others) * p.len_per_u;
#pragma unroll
                for (int m = 1; m < NM; ++m) pl[m] = corr[m - 1][rr] * p.len_per_u;
              }
            }
#pragma unroll
            for (int m = 0; m < NM - 1; ++m) {
              float first[4];
#pragma unroll
              for (int rr = 0; rr < 4; ++rr) first[rr] = corr[m][rr];
#pragma unroll
              for (int row = 0; row < 12; ++row) corr[m][row] = corr[m][row + 4];
#pragma unroll
              for (int rr = 0; rr < 4; ++rr) corr[m][12 + rr] = first[rr];
            }
          }
        }
        uint8_t* entries = reinterpret_cast<uint8_t*>(lds_lists);
        DedupTail* tail = dedup_tail();
        uint32_t src_entry = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = dedup::prefix_from_counts(below, own, q) - 1;
          src_entry |= ((uint32_t)e & 0xFFu) << (8 * q);
          if ((own >> q) & 1u) {
#pragma unroll
            for (int m = 0; m < NM - 1; ++m)
              *reinterpret_cast<float4*>(entries + e * kEntry + m * 16) =
                  make_float4(corr[m][4 * q], corr[m][4 * q + 1], corr[m][4 * q + 2], corr[m][4 * q + 3]);
          }
        }
        tail->src[lane] = src_entry;
        // the entries of a pair end where those of the next pair begin: what lies below that pair's first lane (the last pair's,
        // and the unused ones', at the end of the list; the stores of a wave land in program order)
        const int pair = lane >> __builtin_ctz((unsigned)lpp);
        if (lane < 4) tail->pair_end[lane] = n_fresh;
        if (pair_first) {
          tail->chord[pair] = make_float2(p.chord_u, p.len_per_u);
          if (pair > 0) tail->pair_end[pair - 1] = below;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  AirCache air_cache{0.0f, {0.0f, 0.0f}, false, {0.0f, 0.0f}};
  const size_t sstride_n = (size_t)a.n_local_views * a.g.n_rows * a.g.n_channels;
  const bool use_list = kDedup && list_rounds > 0;
  // Narrow list rounds (dedup_index.h: round_rows; pa.det_dedup = 2: four rows per lane in every round, for the A/B).  A round costs
  // what the rows of a lane cost, however few lanes have an entry, and the last round of a list is mostly short (an extruded wave:
  // one entry per pair).  With at most 32 entries left for it, the last round detects two rows per lane, behind the loop of the
  // four-row rounds.  The width is a function of the scalars list_fresh and list_rounds: the detection stays wave-uniform and its
  // tables scalar operands.
  const bool narrow_last = kNarrow && use_list && pa.det_dedup != 2 && dedup::round_rows(list_fresh, list_rounds - 1, kNarrowRows) == 2;
#pragma unroll 1
  for (int q4 = 0; q4 < (use_list ? list_rounds - (narrow_last ? 1 : 0) : 4); ++q4) {
    const bool round_live = lane_live && r0 + 4 * q4 < a.g.n_rows;
    if (!staged && !round_live) break;
    if (staged && !use_list && __ballot(round_live) == 0ull) break;          // wave-uniform: nobody has rows left
    const int entry = 64 * q4 + lane;          // (list rounds)
    bool entry_live = false;
    if constexpr (kDedup) {
      if (use_list) {      // this round's rows are the entry's; lanes past the end of the list detect air, which disturbs no wave-wide short cut
        const uint8_t* entries = reinterpret_cast<const uint8_t*>(lds_lists);
        const DedupTail* tail = dedup_tail();
        const int pair_end[4] = {tail->pair_end[0], tail->pair_end[1], tail->pair_end[2], tail->pair_end[3]};
        entry_live = entry < pair_end[3];
        const float2 cl = tail->chord[entry_live ? dedup::entry_pair(entry, pair_end, n_pairs) : 0];
        chord_u = cl.x;
        len_per_u = cl.y;
#pragma unroll
        for (int m = 0; m < NM - 1; ++m) {
          float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (entry_live) x = *reinterpret_cast<const float4*>(entries + entry * kEntry + m * 16);
          corr[m][0] = x.x;
          corr[m][1] = x.y;
          corr[m][2] = x.z;
          corr[m][3] = x.w;
        }
      }
    }
    float res[2][4];
    {
      float L[4][NM];
      size_t rays[4];
      bool valid[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = r0 + 4 * q4 + rr;
        valid[rr] = r < a.g.n_rows;
        rays[rr] = ray_index(a, v, valid[rr] ? r : 0, c);
        float others = 0.0f;
#pragma unroll
        for (int m = 1; m < NM; ++m) others += corr[m - 1][rr];
        L[rr][0] = (chord_u - others) * len_per_u;
#pragma unroll
        for (int m = 1; m < NM; ++m) L[rr][m] = corr[m - 1][rr] * len_per_u;
      }
      if constexpr (staged || NOISY) {
        if (a.pathlen && !use_list) {             // (test output) written here so that the detection holds no store addresses
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            if (valid[rr] && round_live) {
#pragma unroll
              for (int m = 0; m < NM; ++m) a.pathlen[rays[rr] * NM + m] = L[rr][m];
            }
        }
      }
      if constexpr (NOISY) {
        float var[2][4];
        detect_store<NM, 4, false, true, kShort>(L, a, mu, w, w2, rays, valid, bm, &air_cache, &res, &var);
        if (a.variance && round_live) {            // (optional output: plain stores)
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (s < a.n_spectra) {
#pragma unroll
              for (int rr = 0; rr < 4; ++rr)
                if (valid[rr]) a.variance[rays[rr] + s * sstride_n] = var[s][rr];
            }
        }
        if (pa.sample) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            float z[2];
            pixel_normals<2>((uint32_t)(pa.view_begin + v), (uint32_t)(r0 + 4 * q4 + rr), (uint32_t)c, pa.seed_lo, pa.seed_hi, z);
            res[0][rr] = noisy_count(res[0][rr], var[0][rr], z[0]);
            res[1][rr] = noisy_count(res[1][rr], var[1][rr], z[1]);
          }
        }
        if constexpr (!staged) {                   // the round's stores (what detect_store does for the noise-free kernel)
          if (round_live) {
            const bool vec4 = a.layout == 1 && (a.g.n_rows & 3) == 0 && valid[3];
#pragma unroll
            for (int s = 0; s < 2; ++s)
              if (s < a.n_spectra) {
                if (vec4) {
                  *reinterpret_cast<float4*>(a.counts + rays[0] + s * sstride_n) = make_float4(res[s][0], res[s][1], res[s][2], res[s][3]);
                  if (a.sino_log)
                    *reinterpret_cast<float4*>(a.sino_log + rays[0] + s * sstride_n) =
                        make_float4(log_ratio(a.air[s], res[s][0]), log_ratio(a.air[s], res[s][1]),
                                    log_ratio(a.air[s], res[s][2]), log_ratio(a.air[s], res[s][3]));
                } else {
#pragma unroll
                  for (int rr = 0; rr < 4; ++rr)
                    if (valid[rr]) {
                      a.counts[rays[rr] + s * sstride_n] = res[s][rr];
                      if (a.sino_log) a.sino_log[rays[rr] + s * sstride_n] = log_ratio(a.air[s], res[s][rr]);
                    }
                }
              }
          }
        }
      } else if constexpr (staged) {
        detect_store<NM, 4, false, false, kShort>(L, a, mu, w, w2, rays, valid, bm, &air_cache, &res);
      } else {
        detect_store<NM, 4, true, false, kShort>(L, a, mu, w, w2, rays, valid, bm, &air_cache);
      }
    }
    // STAGED: the round's results go to LDS right away (plane s, float index 16 lane + row): no registers are held for
    // them, and the (corr[0][row], corr[1][row]) register pairs of the traversal's v_pk_add_f32 stay undisturbed
    if constexpr (staged) {
      if (kDedup && use_list) {      // list rounds: the results replace the entry
        if (entry_live) {
          float4* e_w = reinterpret_cast<float4*>(reinterpret_cast<uint8_t*>(lds_lists) + entry * kEntry);
          e_w[0] = make_float4(res[0][0], res[0][1], res[0][2], res[0][3]);
          e_w[1] = make_float4(res[1][0], res[1][1], res[1][2], res[1][3]);
        }
      } else if (round_live) {
        float* stage_w = reinterpret_cast<float*>(lds_lists) + lane * 16 + 4 * q4;
#pragma unroll
        for (int s = 0; s < kResSlots; ++s)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) stage_w[s * 1024 + rr] = res[s][rr];
      }
    }
#pragma unroll
    for (int m = 0; m < NM - 1; ++m)
#pragma unroll
      for (int row = 0; row < 12; ++row) corr[m][row] = corr[m][row + 4];
  }
  // The narrow last round of a list (narrow_last, above), behind the four-row rounds and outside their loop: lane j detects the
  // two rows 2 (j & 1), + 1 of entry 64 q4 + (j >> 1) - per ray the operations of the four-row form (detect_energies: each half
  // of a pair runs the scalar sequence), half of the instructions.  A lane reads and writes its own half of every 16 bytes of its
  // entry and nothing else.
  if constexpr (kNarrow) {
    if (narrow_last) {
      const int q4 = list_rounds - 1;
      uint8_t* entries = reinterpret_cast<uint8_t*>(lds_lists);
      const DedupTail* tail = dedup_tail();
      const int pair_end[4] = {tail->pair_end[0], tail->pair_end[1], tail->pair_end[2], tail->pair_end[3]};
      const int e2 = dedup::lane_entry(2, q4, lane), first = dedup::lane_first_row(2, lane);
      const bool e2_live = e2 < pair_end[3];
      const float2 cl = tail->chord[e2_live ? dedup::entry_pair(e2, pair_end, n_pairs) : 0];
      float2 sum2[NM - 1];
#pragma unroll
      for (int m = 0; m < NM - 1; ++m) {
        sum2[m] = make_float2(0.0f, 0.0f);      // (lanes past the end of the list detect air, as in the four-row rounds)
        if (e2_live) sum2[m] = *reinterpret_cast<const float2*>(entries + e2 * kEntry + dedup::piece_in(m, first));
      }
      float L[2][NM];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        float others = 0.0f;
#pragma unroll
        for (int m = 1; m < NM; ++m) others += rr ? sum2[m - 1].y : sum2[m - 1].x;
        L[rr][0] = (cl.x - others) * cl.y;
#pragma unroll
        for (int m = 1; m < NM; ++m) L[rr][m] = (rr ? sum2[m - 1].y : sum2[m - 1].x) * cl.y;
      }
      const size_t rays2[2] = {0, 0};           // (the caller stores: detect_store looks at neither)
      const bool valid2[2] = {true, true};
      float res2[2][2];
      __builtin_assume(a.n_spectra <= 2);        // (STAGED: the host's condition)
      detect_store<NM, 2, false, false, kShort>(L, a, mu, w, w2, rays2, valid2, bm, nullptr, &res2);
      if (e2_live) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
          *reinterpret_cast<float2*>(entries + e2 * kEntry + dedup::piece_out(s, first)) = make_float2(res2[s][0], res2[s][1]);
      }
    }
  }
  if constexpr (!staged) return;
  if constexpr (kDedup) {
    if (use_list) {      // every quad takes its entry's results (all reads, then all writes: the stage lies over the list)
      const uint8_t* entries = reinterpret_cast<const uint8_t*>(lds_lists);
      float4 got[4][2];
      const uint32_t src_entry = dedup_tail()->src[lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4* e_r = reinterpret_cast<const float4*>(entries + ((src_entry >> (8 * q)) & 0xFFu) * kEntry);
        got[q][0] = got[q][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (lane_live && r0 + 4 * q < a.g.n_rows) {      // (a quad without rows has no entry to look at)
          got[q][0] = e_r[0];
          got[q][1] = e_r[1];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (lane_live && r0 + 4 * q < a.g.n_rows) {
          float4* stage_w = reinterpret_cast<float4*>(lds_lists) + lane * 4 + q;
          stage_w[0] = got[q][0];
          stage_w[256] = got[q][1];
        }
      }
    }
  }
  // ---- whole-line stores: the rounds left the 16 results of lane l and spectrum s in LDS at plane s, float index
  // 16 l + row; store instruction k takes the 16-byte piece 64 k + lane = (lane l' = piece / 4, rows 4 (piece % 4) ...):
  // consecutive lanes write consecutive 16 bytes
  float* stage = reinterpret_cast<float*>(lds_lists);
  const int lpp_shift = __builtin_ctz((unsigned)lpp);
  const int c_base = c - g;                                    // first channel of the wave
  const size_t sstride = (size_t)a.n_local_views * a.g.n_rows * a.g.n_channels;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int s = 0; s < kResSlots; ++s) {
    if (s >= a.n_spectra) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int piece = k * 64 + lane, l2 = piece >> 2, c2 = piece & 3;
      const int g2 = l2 >> lpp_shift, li2 = l2 - (g2 << lpp_shift);
      const int row = (zc * 64 + li2) * 16 + 4 * c2, chan = c_base + g2;
      if (chan < a.g.n_channels && row < a.g.n_rows) {
        const float4 x = *reinterpret_cast<const float4*>(stage + s * 1024 + piece * 4);
        const size_t at = s * sstride + ((size_t)v * a.g.n_channels + chan) * a.g.n_rows + row;
        *reinterpret_cast<float4*>(a.counts + at) = x;
        if (a.sino_log)
          *reinterpret_cast<float4*>(a.sino_log + at) = make_float4(log_ratio(a.air[s], x.x), log_ratio(a.air[s], x.y),
                                                                    log_ratio(a.air[s], x.z), log_ratio(a.air[s], x.w));
      }
    }
  }
}

// vol_zf [ny][nx][nz] (one byte per voxel, ids < 4) -> vol_z2 [ny][nx][nz / 4] (2 bits per voxel, z fastest)
__global__ __launch_bounds__(256) void pack2_kernel(const uint8_t* __restrict__ vol_zf, size_t n_bytes_out,
                                                    uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_bytes_out) return;
  const uint32_t x = *reinterpret_cast<const uint32_t*>(vol_zf + 4 * i);
  out[i] = (uint8_t)((x & 3u) | (((x >> 8) & 3u) << 2) | (((x >> 16) & 3u) << 4) | (((x >> 24) & 3u) << 6));
}

// The air-column map of the packed volume: bit c % 32 of word c / 32 is set iff the zb bytes of column c = y * nx + x are all
// 0; the bits past the last column stay clear.  A workgroup takes 256 columns at a time (grid-stride over such chunks:
// block-uniform, so every lane reaches the ballot); a wave's ballot is two words of the map.  n_air receives the set bits.
__global__ __launch_bounds__(256) void col_air_kernel(const uint8_t* __restrict__ vol_z2, uint32_t n_cols, uint32_t zb,
                                                      uint32_t* __restrict__ col_air, unsigned long long* __restrict__ n_air) {
  const uint32_t n_chunks = (n_cols + 255u) / 256u, n_words = (n_cols + 31u) / 32u;
  const bool dwords = (zb & 3u) == 0 && (reinterpret_cast<uintptr_t>(vol_z2) & 3u) == 0;
  for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const uint32_t col = ch * 256u + threadIdx.x;
    uint32_t any = 1u;
    if (col < n_cols) {
      const uint8_t* q = vol_z2 + (size_t)col * zb;
      any = 0u;
      if (dwords)
        for (uint32_t k = 0; k < zb; k += 4) any |= *reinterpret_cast<const uint32_t*>(q + k);
      else
        for (uint32_t k = 0; k < zb; ++k) any |= q[k];
    }
    const unsigned long long m = __ballot(any == 0u);
    if ((threadIdx.x & 63u) == 0u) {
      const uint32_t wi = (ch * 256u + threadIdx.x) >> 5;
      if (wi < n_words) col_air[wi] = (uint32_t)m;
      if (wi + 1 < n_words) col_air[wi + 1] = (uint32_t)(m >> 32);
      if (m) atomicAdd(n_air, (unsigned long long)__popcll(m));
    }
  }
}

// The column-class map of the packed volume (uniform_count.h, include/dexct_p16_uniform.h): nibble c % 8 of word c / 8 is
// ucount::class_of(id) iff all zb bytes of column c = y * nx + x hold id in each of their four voxels, else 0 (mixed); the nibbles
// past the last column stay 0.  Chunks of 256 columns per workgroup as in col_air_kernel; the three bit planes of a wave's 64
// classes come from three ballots and its first eight lanes write a word each.  n_uniform[id] receives the uniform columns per id.
__global__ __launch_bounds__(256) void col_class_kernel(const uint8_t* __restrict__ vol_z2, uint32_t n_cols, uint32_t zb,
                                                        uint32_t* __restrict__ col_class, unsigned long long* __restrict__ n_uniform) {
  const uint32_t n_chunks = (n_cols + 255u) / 256u, n_words = (n_cols + 7u) / 8u;
  const bool dwords = (zb & 3u) == 0 && (reinterpret_cast<uintptr_t>(vol_z2) & 3u) == 0;
  for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const uint32_t col = ch * 256u + threadIdx.x;
    uint32_t cls = 0u;
    if (col < n_cols) {
      const uint8_t* q = vol_z2 + (size_t)col * zb;
      const uint32_t id = q[0] & 3u;
      uint32_t diff = 0u;
      if (dwords)
        for (uint32_t k = 0; k < zb; k += 4) diff |= *reinterpret_cast<const uint32_t*>(q + k) ^ (id * 0x55555555u);
      else
        for (uint32_t k = 0; k < zb; ++k) diff |= (uint32_t)q[k] ^ (id * 0x55u);
      cls = diff == 0u ? ucount::class_of(id) : 0u;
    }
    const unsigned long long m0 = __ballot(cls & 1u), m1 = __ballot(cls & 2u), m2 = __ballot(cls & 4u);
    const uint32_t sub = threadIdx.x & 63u;
    if (sub < 8u) {
      const uint32_t wi = ((ch * 256u + threadIdx.x - sub) >> 3) + sub;
      uint32_t word = 0u;
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t at = 8u * sub + j;
        word |= ((uint32_t)((m0 >> at) & 1u) | (uint32_t)((m1 >> at) & 1u) << 1 | (uint32_t)((m2 >> at) & 1u) << 2) << (4u * j);
      }
      if (wi < n_words) col_class[wi] = word;
    }
    if (sub == 0u && m0) {
      const unsigned long long per_id[4] = {m0 & ~m1 & ~m2, m0 & m1 & ~m2, m0 & ~m1 & m2, m0 & m1 & m2};
#pragma unroll
      for (int id = 0; id < 4; ++id)
        if (per_id[id]) atomicAdd(n_uniform + id, (unsigned long long)__popcll(per_id[id]));
    }
  }
}

// The tile map of a column-class map (tile_class.h, include/dexct_p16_tiles.h): one thread per nibble of either copy, the outside
// tiles in front of and behind every row included; the map was cleared before, and the eight threads of a word OR their nibbles
// into it.  n_uniform[id] receives the uniform tiles of the grid per id, counted in copy 1 (both copies hold the same tiles).
__global__ __launch_bounds__(256) void tile_class_kernel(const uint32_t* __restrict__ col_class, uint32_t nx, uint32_t ny,
                                                         uint32_t* __restrict__ tile_map, unsigned long long* __restrict__ n_uniform) {
  const tiles::Layout y = tiles::layout(nx, ny);
  const uint32_t per_copy[2] = {y.ti[0] * tiles::row_nibbles(y.tj[0]), y.ti[1] * tiles::row_nibbles(y.tj[1])};
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < per_copy[0] + per_copy[1]; k += gridDim.x * 256u) {
    const int axis = k < per_copy[0] ? 0 : 1;
    const uint32_t at = k - (axis ? per_copy[0] : 0u), row = tiles::row_nibbles(y.tj[axis]);
    const uint32_t I = at / row;
    const int32_t J = (int32_t)(at - I * row) - 1;
    const uint32_t e = tiles::class_of_nibble(col_class, nx, ny, axis, I, J);
    const uint32_t nib = tiles::nibble_of(y, axis, I, J);
    if (e) atomicOr(tile_map + tiles::word_of_nibble(nib), e << ((nib & 7u) << 2));
    if (e && axis == 1 && J >= 0 && J < (int32_t)y.tj[1]) atomicAdd(n_uniform + (e >> 1), 1ull);
  }
}

// the grid cap of col_air_kernel and col_class_kernel (one column per thread)
constexpr int kColAirMaxBlocks = 4096;

// Material groups on the packed volume: ids 3g+1..3g+3 -> codes 1..3, everything else 0 (group_codes_kernel of
// siddon.hip), packed four voxels per byte: out [n_groups][n_voxels / 4]
__global__ __launch_bounds__(256) void group_codes_pack2_kernel(const uint8_t* __restrict__ vol_zf, size_t n_bytes_out,
                                                                int n_groups, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_bytes_out) return;
  const uint32_t x = *reinterpret_cast<const uint32_t*>(vol_zf + 4 * i);
  for (int g = 0; g < n_groups; ++g) {
    uint32_t y = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t rel = ((x >> (8 * b)) & 0xFFu) - 3u * g;      // 1..3 inside the group
      y |= ((rel >= 1u && rel <= 3u) ? rel : 0u) << (2 * b);
    }
    out[(size_t)g * n_bytes_out + i] = (uint8_t)y;
  }
}

// one launch of rows16_kernel
struct P16Launch {
  PackedArgs pa;
  Tables t;
  dim3 grid;
  size_t lds;
  hipStream_t st;
  bool staged_store;      // DEXCT_P16_STAGED: store the results of a wave through LDS as whole lines (0: per-round 16-B stores)
};
// TWO ENCODINGS to know before adding a form (both keep every other form's name and PackedArgs as they were):
//  - MINW here is the kernel's MINW_FORM: the waves per SIMD (1 .. 8), plus kTileForm for a tile form (launch_p16_tiles is the only
//    caller that adds it; a value of DEXCT_P16_MINW never reaches this parameter - the entry point maps it to 4, 5, 6 or 8);
//  - a tile form reads l.pa.seed_lo / seed_hi as the address of the tile map.  The noisy forms read the same words as the seed of
//    their sample, so a noisy tile form needs a place of its own for one of the two (the kernel asserts that TILES excludes NOISY).
template <int NM, int MINW, bool GROUPED, bool STAGED, bool NOISY, bool SKIP = false>
static int launch_p16(const P16Launch& l) {
  hipLaunchKernelGGL((rows16_kernel<NM, MINW, GROUPED, STAGED, NOISY, SKIP>), l.grid, dim3(64), l.lds, l.st, l.pa, l.t.mu, l.t.w, l.t.w2);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

// what both entry points check, in this order; fills the launch shape
static int packed_shape(const dexct_fan_geom* geom, int32_t view_begin, int32_t view_end, int32_t layout, PackedArgs& pa,
                        dim3& grid, size_t& lds) {
  if (!proj::views_ok(*geom, view_begin, view_end)) return DEXCT_EINVAL;
  if (geom->n_rows < 1) return DEXCT_EINVAL;
  if (!proj::stack_ok(*geom)) return DEXCT_EINVAL;
  if (!proj::stack_aligned(*geom, 16)) return DEXCT_EINVAL;
  if (!proj::offsets_fit(*geom, 4, 0xEFFF0000ull)) return DEXCT_ERANGE;    // below kOob
  if (geom->nx > 2047 || geom->ny > 2047) return DEXCT_ERANGE;             // 11-bit sliced counters: one count per slab
  if (!proj::layout_ok(layout)) return DEXCT_EINVAL;
  if (!proj::fits_16bit(*geom, view_begin, view_end)) return DEXCT_ERANGE;
  // a (view, channel) pair takes ceil(n_rows / 16) lanes: 16 or 32 lanes per pair (4 or 2 pairs per wave) or whole
  // waves; lanes past the last row idle (the caller decides whether that is still worth it)
  const int lanes = (geom->n_rows + 15) / 16;
  pa.lanes_per_pair = lanes > 32 ? 64 : (lanes > 16 ? 32 : 16);
  pa.n_zchunks = lanes > 64 ? (lanes + 63) / 64 : 1;
  pa.view_tile = proj::read_knob(proj::knob::kViewTileP16);
  pa.det_masks = proj::read_knob(proj::knob::kDetMasks) != 0;
  pa.det_absent = proj::read_knob(proj::knob::kDetAbsent) != 0;
  pa.det_dedup = proj::read_knob(proj::knob::kDetDedup);      // 0: off, 2: four-row list rounds only, else the narrow rounds too
  pa.view_begin = view_begin;
  const int n_pairs = 64 / pa.lanes_per_pair;
  if (!proj::grid_1d((size_t)(view_end - view_begin) * ((geom->n_channels + n_pairs - 1) / n_pairs) * pa.n_zchunks, grid))
    return DEXCT_ERANGE;
  lds = p16_lds_bytes(n_pairs);
  return DEXCT_OK;
}

// the SKIP forms rows16_kernel<NM, MINW, false, STAGED, NOISY, true> (MINW as the forms without the map; the DEXCT_P16_MINW forms have none)
static int launch_p16_skip(const P16Launch& l, int n_materials, bool staged, bool noisy) {
  if (noisy) {
    if (n_materials == 2) return staged ? launch_p16<2, 4, false, true, true, true>(l) : launch_p16<2, 4, false, false, true, true>(l);
    if (n_materials == 4) return staged ? launch_p16<4, 3, false, true, true, true>(l) : launch_p16<4, 3, false, false, true, true>(l);
    return staged ? launch_p16<3, 4, false, true, true, true>(l) : launch_p16<3, 4, false, false, true, true>(l);
  }
  if (n_materials == 2) return staged ? launch_p16<2, 4, false, true, false, true>(l) : launch_p16<2, 4, false, false, false, true>(l);
  if (n_materials == 4) return staged ? launch_p16<4, 3, false, true, false, true>(l) : launch_p16<4, 3, false, false, false, true>(l);
  return staged ? launch_p16<3, 4, false, true, false, true>(l) : launch_p16<3, 4, false, false, false, true>(l);
}
// the tile forms: the staged noise-free SKIP forms with kTileForm added to their MINW (the tile map's address and a class map are set)
static int launch_p16_tiles(const P16Launch& l, int n_materials) {
  if (n_materials == 2) return launch_p16<2, kTileForm + 4, false, true, false, true>(l);
  if (n_materials == 4) return launch_p16<4, kTileForm + 3, false, true, false, true>(l);
  return launch_p16<3, kTileForm + 4, false, true, false, true>(l);
}

}  // namespace dexct

using namespace dexct;

extern "C" {

int dexct_volume_pack2(const uint8_t* vol_zf, int64_t n_voxels, uint8_t* vol_z2, void* stream) {
  if (!vol_zf || !vol_z2 || n_voxels <= 0 || (n_voxels & 3)) return DEXCT_EINVAL;
  const size_t nb = (size_t)n_voxels / 4;
  dim3 grid;
  if (!proj::grid_1d((nb + 255) / 256, grid)) return DEXCT_ERANGE;
  hipLaunchKernelGGL(pack2_kernel, grid, dim3(256), 0, as_stream(stream), vol_zf, nb, vol_z2);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_volume_groups_pack2(const uint8_t* vol_zf, int64_t n_voxels, int32_t n_materials, uint8_t* codes2, void* stream) {
  if (!vol_zf || !codes2 || n_voxels <= 0 || (n_voxels & 3)) return DEXCT_EINVAL;
  if (n_materials < 2 || n_materials > DEXCT_MAX_MATERIALS) return DEXCT_ERANGE;
  const size_t nb = (size_t)n_voxels / 4;
  dim3 grid;
  if (!proj::grid_1d((nb + 255) / 256, grid)) return DEXCT_ERANGE;
  hipLaunchKernelGGL(group_codes_pack2_kernel, grid, dim3(256), 0, as_stream(stream), vol_zf, nb, proj::n_groups(n_materials, true),
                     codes2);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_volume_air_columns(const uint8_t* vol_z2, int32_t nx, int32_t ny, int32_t nz, uint32_t* col_air, uint64_t* n_air,
                             void* stream) {
  if (!vol_z2 || !col_air || !n_air || nx < 1 || ny < 1 || nz < 4 || (nz & 3)) return DEXCT_EINVAL;
  if ((uint64_t)nx * ny > 0x7FFFFF00ull) return DEXCT_ERANGE;                 // 32-bit column indices (whole chunks of 256)
  const uint32_t n_cols = (uint32_t)nx * (uint32_t)ny;
  hipStream_t st = as_stream(stream);
  DEXCT_HIP_TRY(hipMemsetAsync(n_air, 0, sizeof(uint64_t), st));
  uint32_t nblk = (n_cols + 255u) / 256u;
  if (nblk > (uint32_t)kColAirMaxBlocks) nblk = kColAirMaxBlocks;
  hipLaunchKernelGGL(col_air_kernel, dim3(nblk), dim3(256), 0, st, vol_z2, n_cols, (uint32_t)nz >> 2, col_air,
                     reinterpret_cast<unsigned long long*>(n_air));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_volume_column_classes(const uint8_t* vol_z2, int32_t nx, int32_t ny, int32_t nz, uint32_t* col_class, uint64_t* n_uniform,
                                void* stream) {
  if (!vol_z2 || !col_class || !n_uniform || nx < 1 || ny < 1 || nz < 4 || (nz & 3)) return DEXCT_EINVAL;
  if ((uint64_t)nx * ny > 0x7FFFFF00ull) return DEXCT_ERANGE;                 // 32-bit column indices (whole chunks of 256)
  const uint32_t n_cols = (uint32_t)nx * (uint32_t)ny;
  hipStream_t st = as_stream(stream);
  DEXCT_HIP_TRY(hipMemsetAsync(n_uniform, 0, 4 * sizeof(uint64_t), st));
  uint32_t nblk = (n_cols + 255u) / 256u;
  if (nblk > (uint32_t)kColAirMaxBlocks) nblk = kColAirMaxBlocks;
  hipLaunchKernelGGL(col_class_kernel, dim3(nblk), dim3(256), 0, st, vol_z2, n_cols, (uint32_t)nz >> 2, col_class,
                     reinterpret_cast<unsigned long long*>(n_uniform));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int64_t dexct_volume_tile_map_words(int32_t nx, int32_t ny) {
  if (nx < 1 || ny < 1 || (uint64_t)nx * ny > 0x7FFFFF00ull) return 0;
  return tiles::layout((uint32_t)nx, (uint32_t)ny).words;
}

int dexct_volume_tile_classes(const uint32_t* col_class, int32_t nx, int32_t ny, uint32_t* tile_map, uint64_t* n_uniform, void* stream) {
  if (!col_class || !tile_map || !n_uniform || nx < 1 || ny < 1) return DEXCT_EINVAL;
  if ((uint64_t)nx * ny > 0x7FFFFF00ull) return DEXCT_ERANGE;
  const tiles::Layout y = tiles::layout((uint32_t)nx, (uint32_t)ny);
  hipStream_t st = as_stream(stream);
  DEXCT_HIP_TRY(hipMemsetAsync(n_uniform, 0, 4 * sizeof(uint64_t), st));
  DEXCT_HIP_TRY(hipMemsetAsync(tile_map, 0, (size_t)y.words * sizeof(uint32_t), st));
  const uint32_t n_nibbles = y.ti[0] * tiles::row_nibbles(y.tj[0]) + y.ti[1] * tiles::row_nibbles(y.tj[1]);
  uint32_t nblk = (n_nibbles + 255u) / 256u;
  if (nblk > (uint32_t)kColAirMaxBlocks) nblk = kColAirMaxBlocks;
  hipLaunchKernelGGL(tile_class_kernel, dim3(nblk), dim3(256), 0, st, col_class, (uint32_t)nx, (uint32_t)ny, tile_map,
                     reinterpret_cast<unsigned long long*>(n_uniform));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int dexct_siddon_project_packed(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                int32_t n_spectra, const float* mu, const float* weights, float* counts, float* pathlen,
                                int32_t layout, const dexct_log_out* log_out, const float* weights2, float* variance,
                                const dexct_noise* noise, void* stream) {
  return dexct_siddon_project_packed_skip(geom, plan, view_begin, view_end, vol_z2, n_materials, n_energies, n_spectra, mu, weights,
                                          counts, pathlen, layout, log_out, weights2, variance, noise, nullptr, 0, stream);
}

int dexct_siddon_project_packed_skip(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                     int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                     int32_t n_spectra, const float* mu, const float* weights, float* counts, float* pathlen,
                                     int32_t layout, const dexct_log_out* log_out, const float* weights2, float* variance,
                                     const dexct_noise* noise, const uint32_t* col_air, int64_t n_air_columns, void* stream) {
  return dexct_siddon_project_packed_uniform(geom, plan, view_begin, view_end, vol_z2, n_materials, n_energies, n_spectra, mu,
                                             weights, counts, pathlen, layout, log_out, weights2, variance, noise, col_air,
                                             n_air_columns, nullptr, nullptr, stream);
}

int dexct_siddon_project_packed_uniform(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                        int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                        int32_t n_spectra, const float* mu, const float* weights, float* counts, float* pathlen,
                                        int32_t layout, const dexct_log_out* log_out, const float* weights2, float* variance,
                                        const dexct_noise* noise, const uint32_t* col_air, int64_t n_air_columns,
                                        const uint32_t* col_class, const int64_t* n_uniform_columns, void* stream) {
  return dexct_siddon_project_packed_tiles(geom, plan, view_begin, view_end, vol_z2, n_materials, n_energies, n_spectra, mu, weights,
                                           counts, pathlen, layout, log_out, weights2, variance, noise, col_air, n_air_columns,
                                           col_class, n_uniform_columns, nullptr, nullptr, stream);
}

int dexct_siddon_project_packed_tiles(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                      int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                      int32_t n_spectra, const float* mu, const float* weights, float* counts, float* pathlen,
                                      int32_t layout, const dexct_log_out* log_out, const float* weights2, float* variance,
                                      const dexct_noise* noise, const uint32_t* col_air, int64_t n_air_columns,
                                      const uint32_t* col_class, const int64_t* n_uniform_columns, const uint32_t* tile_map,
                                      const int64_t* n_uniform_tiles, void* stream) {
  if (!geom || !plan || !vol_z2 || !mu || !weights || !counts) return DEXCT_EINVAL;
  if (n_energies < 1 || n_spectra < 1) return DEXCT_EINVAL;
  if (n_materials < 2 || n_materials > 4 || n_spectra > DEXCT_MAX_SPECTRA) return DEXCT_ERANGE;     // ids 0..3
  const proj::NoiseLog nl = proj::noise_log_args(weights2, variance, noise, log_out, n_spectra, n_materials, proj::NoiseBy::kTwoSlots);
  if (nl.noise_rc != DEXCT_OK) return nl.noise_rc;
  P16Launch l{};
  const int rc = packed_shape(geom, view_begin, view_end, layout, l.pa, l.grid, l.lds);
  if (rc != DEXCT_OK) return rc;
  if (nl.log_rc != DEXCT_OK) return nl.log_rc;
  l.pa.a = proj::fill_proj_args(*geom, plan, view_begin, view_end, n_materials, n_energies, n_spectra, counts, pathlen, variance, layout,
                                nl);
  l.pa.a.view_tile = l.pa.view_tile;
  l.pa.vol_z2 = vol_z2;
  const int64_t n_cols = (int64_t)geom->nx * geom->ny;
  if (col_air && (n_air_columns < 0 || n_air_columns > n_cols)) return DEXCT_EINVAL;
  if (col_class && (!n_uniform_columns || !proj::class_counts_ok(n_uniform_columns, n_cols))) return DEXCT_EINVAL;
  const bool noisy = weights2 != nullptr;
  l.t = Tables{mu, weights, weights2};
  l.st = as_stream(stream);
  l.staged_store = proj::read_knob(proj::knob::kP16Staged) != 0;
  // whole-line stores through LDS (STAGED) wherever the output allows them: row-fastest layout, whole groups of 4 rows,
  // one or two spectra (what the stage holds)
  const bool staged = l.staged_store && layout == 1 && geom->n_rows % 4 == 0 && n_spectra <= 2;
  // rows16_kernel<NM, MINW, false, STAGED, NOISY>: MINW is 4 for two and three materials, 3 for four.  (The order of the arms
  // is the order in which the kernels are instantiated, hence their order in the code object.)
  // with the air-column map: the SKIP forms (instantiated after all the others, below); the DEXCT_P16_MINW forms have none
  // three materials without noise also have the forms DEXCT_P16_MINW asks for: 5 with and without the staged store, 6 and 8
  // without; every other value is 4 - and any value but 4 and 5 has always cost the staged store
  const int minw = (noisy || n_materials != 3) ? 4 : proj::read_knob(proj::knob::kP16MinW);
  const bool minw_form = minw == 5 || minw == 6 || minw == 8;
  const bool skip_staged = staged && minw == 4;            // the SKIP form a map would run
  // a map costs a few instructions per slab and lane and pays them back with the slabs it drops: proj::use_class_map for the
  // class map (the SKIP forms that take one: p16_by_class), else proj::use_air_map for the air map
  const int air_mode = proj::read_knob(proj::knob::kP16AirSkip);
  const bool by_class = p16_by_class(n_materials, skip_staged, noisy) &&
                        proj::use_class_map(proj::read_knob(proj::knob::kP16Uniform), air_mode, col_class != nullptr, n_uniform_columns, n_cols);
  if (by_class) l.pa.col_air = col_class;
  else l.pa.col_air = proj::use_air_map(air_mode, col_air != nullptr, n_air_columns, n_cols) ? col_air : nullptr;
  proj::copy_noise(l.pa, view_begin, nl);     // (rows16_kernel draws the sample itself: PackedArgs, not its ProjArgs)
  if (!noisy) l.pa.col_class = by_class ? 1 : 0;      // (the word is `sample` to the noisy forms)
  // the tile map rides on the class map, in the staged forms that take one (the words are the seed to the noisy forms)
  const int64_t n_tiles = (int64_t)tiles::tiles_along((uint32_t)geom->nx) * tiles::tiles_along((uint32_t)geom->ny);
  if (tile_map && (!n_uniform_tiles || !proj::class_counts_ok(n_uniform_tiles, n_tiles))) return DEXCT_EINVAL;
  const bool by_tiles = by_class && skip_staged && !minw_form && tiles::grid_fits((uint32_t)geom->nx, (uint32_t)geom->ny) &&
                        proj::use_tile_map(proj::read_knob(proj::knob::kP16Tiles), tile_map != nullptr, n_uniform_tiles, n_tiles);
  if (by_tiles) {
    l.pa.seed_lo = (uint32_t)reinterpret_cast<uintptr_t>(tile_map);      // (PackedArgs: the seed's words, which these forms do not draw from)
    l.pa.seed_hi = (uint32_t)(reinterpret_cast<uintptr_t>(tile_map) >> 32);
    return launch_p16_tiles(l, n_materials);
  }
  // with a map: the SKIP forms, which exist for the default MINW only
  if (l.pa.col_air && !minw_form) return launch_p16_skip(l, n_materials, skip_staged, noisy);
  if (noisy) {
    if (n_materials == 2) return staged ? launch_p16<2, 4, false, true, true>(l) : launch_p16<2, 4, false, false, true>(l);
    if (n_materials == 4) return staged ? launch_p16<4, 3, false, true, true>(l) : launch_p16<4, 3, false, false, true>(l);
    return staged ? launch_p16<3, 4, false, true, true>(l) : launch_p16<3, 4, false, false, true>(l);
  }
  if (n_materials == 2) return staged ? launch_p16<2, 4, false, true, false>(l) : launch_p16<2, 4, false, false, false>(l);
  if (n_materials == 4) return staged ? launch_p16<4, 3, false, true, false>(l) : launch_p16<4, 3, false, false, false>(l);
  if (staged && minw == 4) return launch_p16<3, 4, false, true, false>(l);
  if (minw == 5) return staged ? launch_p16<3, 5, false, true, false>(l) : launch_p16<3, 5, false, false, false>(l);
  if (minw == 6) return launch_p16<3, 6, false, false, false>(l);
  if (minw == 8) return launch_p16<3, 8, false, false, false>(l);
  return launch_p16<3, 4, false, false, false>(l);
}

int dexct_siddon_project_grouped_packed(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                        int32_t view_end, const uint8_t* codes2, int32_t n_materials, int32_t n_energies,
                                        int32_t n_spectra, const float* mu, const float* weights, float* counts,
                                        float* pathlen, float* acc_scratch, int32_t layout, const float* weights2,
                                        float* variance, const dexct_log_out* log_out, const dexct_noise* noise, void* stream) {
  if (!geom || !plan || !codes2 || !mu || !weights || !counts || !acc_scratch) return DEXCT_EINVAL;
  if (n_materials < 2 || n_energies < 1 || n_spectra < 1) return DEXCT_EINVAL;
  if (n_materials > DEXCT_MAX_MATERIALS || n_spectra > DEXCT_MAX_SPECTRA) return DEXCT_ERANGE;
  P16Launch l{};
  const int rc = packed_shape(geom, view_begin, view_end, layout, l.pa, l.grid, l.lds);
  if (rc != DEXCT_OK) return rc;
  const proj::NoiseLog nl = proj::noise_log_args(weights2, variance, noise, log_out, n_spectra, n_materials, proj::NoiseBy::kGroupPass);
  if (nl.status() != DEXCT_OK) return nl.status();
  ProjArgs& a = l.pa.a;
  a = proj::fill_proj_args(*geom, plan, view_begin, view_end, n_materials, n_energies, n_spectra, counts, pathlen, variance, layout, nl);
  proj::copy_noise(a, view_begin, nl);          // (the detection pass draws the sample, not rows16_kernel)
  a.acc_out = acc_scratch;
  a.view_tile = l.pa.view_tile;
  l.st = as_stream(stream);                     // (the group passes take no tables: l.t stays null)
  const size_t group_bytes = (size_t)geom->nx * geom->ny * (geom->nz / 4);
  for (int g = 0; g < proj::n_groups(n_materials, true); ++g) {
    l.pa.vol_z2 = codes2 + (size_t)g * group_bytes;
    a.mat_base = 3 * g;
    // (codes 0..3 of a group: its materials and "none of them")
    const int lrc = proj::for_materials<4, 3, 2>(proj::group_size(n_materials, true, g) + 1, [&](auto nm) {
      constexpr int NM = decltype(nm)::value;
      return launch_p16<NM, (NM == 4 ? 3 : 4), true, false, false>(l);
    });
    if (lrc != DEXCT_OK) return lrc;
  }
  return launch_detect_any(a, Tables{mu, weights, weights2}, l.st);
}

}  // extern "C"
