// Tile classes of rows16_kernel's tile forms (siddon_packed.hip): the map of K x K blocks of columns, the rule that dismisses a
// run of K slabs before they are classified one by one, the sharing-out of runs and fine slabs to the lanes of a pair, and the
// bound on the per-lane count under that sharing-out.  The one copy; plain C++, so that a host program can include it
// (tests/tile_class_host.cpp, also under the sanitizers).
//
// WHY EVERY OUTPUT KEEPS ITS BYTES.  uniform_count.h lets a slab leave the lists when both its pieces lie in columns uniform in
//   the same id (a piece outside the grid reads as air) and counts it in the integer of its id.  A TILE is kSide x kSide columns,
//   uniform in an id when all its columns are; a RUN is the slabs i = kSide R .. kSide R + kSide - 1 of a ray, cut to the ray's
//   own slabs.  Slab i has the pieces j(i) and j(i + 1) with j(i) = (V0 + i SV) >> 40, monotone in i; so all the pieces of a run
//   lie between j of its first slab and j(last + 1), in tile row R, in the tiles of that j range.  When all those tiles are
//   uniform in one id - a tile wholly outside the grid counts as air, one that reaches past the grid is uniform in air or mixed -
//   every piece of every slab of the run lies in a column of that id or, for air, outside the grid: the slab rule would drop each
//   of them into the same integer.  The run adds its number of slabs to that integer at once.  Every other run SURVIVES and its
//   slabs go through the slab rule in slab order, so the lists hold the same slabs in the same order.
#pragma once
#include <cstdint>

#include "gn_dedup_index.h"
#include "uniform_count.h"

namespace dexct {
namespace tiles {

constexpr int kShift = 3, kSide = 1 << kShift;        // K = 8 (profiles/rows16_tiles.md has the census for 4, 8 and 16)
constexpr int kTilesPerRun = 3;                        // slope <= 1: kSide slabs reach at most kSide + 1 cells beyond the first
constexpr int kWindow = 64;                            // runs of a pair whose surviving mask is held at once
constexpr int kFixFrac = 40;                           // DEXCT_FIX_FRAC
// the kernel holds ONE window: the grids whose rays (slabs 0 .. n - 1 along their axis, dexct_fan_plan) have at most kWindow runs
DEXCT_UCOUNT_FN constexpr bool grid_fits(uint32_t nx, uint32_t ny) { return nx <= (uint32_t)(kSide * kWindow) && ny <= (uint32_t)(kSide * kWindow); }

// ---- the map: four bits per tile with the class codes of ucount (0 mixed, kUniform | id << 1), eight tiles per word, in TWO
// copies, one per slab axis.  Copy a holds, for every tile row I along its slab axis, the tiles J = -1 .. tj along the other
// axis: the tiles -1 and tj are outside the grid (air), so that a j range clamped to them needs no test of its own.  The at most
// three tiles of a run are consecutive nibbles of one row: at most two neighbouring words.  Copy 1 starts on a whole word; one
// spare word ends the map, so that word + 1 exists for every nibble OF A TILE ROW OF THE GRID (I < ti).  A reader that also forms
// nibbles of rows I >= ti - the kernel's lanes without a run do - lands in the spare word or behind the map: every word is read
// through a check against the map's size (checked_word; in the kernel a bounds-checked buffer), and a word outside reads 0, mixed.
struct Layout {
  uint32_t ti[2], tj[2];       // tiles along the slab axis / across it, per copy (axis 0: slabs along x; axis 1: along y)
  uint32_t first_nibble[2];    // where each copy starts
  uint32_t words;              // of the whole map
};
DEXCT_UCOUNT_FN constexpr uint32_t tiles_along(uint32_t n) { return (n + kSide - 1u) >> kShift; }
DEXCT_UCOUNT_FN constexpr uint32_t row_nibbles(uint32_t tj) { return tj + 2u; }
DEXCT_UCOUNT_FN constexpr Layout layout(uint32_t nx, uint32_t ny) {
  const uint32_t tx = tiles_along(nx), ty = tiles_along(ny);
  const uint32_t words0 = (tx * row_nibbles(ty) + 7u) >> 3, words1 = (ty * row_nibbles(tx) + 7u) >> 3;
  return Layout{{tx, ty}, {ty, tx}, {0u, 8u * words0}, words0 + words1 + 1u};
}
// the nibble of tile (I, J) of a copy, J = -1 .. tj: from the copy's first nibble and its tj (the kernel picks the two per pair;
// an array indexed per lane would live in scratch), or from the layout
DEXCT_UCOUNT_FN constexpr uint32_t nibble_at(uint32_t first_nibble, uint32_t tj, uint32_t I, int32_t J) {
  return first_nibble + I * row_nibbles(tj) + (uint32_t)(J + 1);
}
DEXCT_UCOUNT_FN constexpr uint32_t nibble_of(const Layout& y, int axis, uint32_t I, int32_t J) {
  return nibble_at(y.first_nibble[axis], y.tj[axis], I, J);
}
DEXCT_UCOUNT_FN constexpr uint32_t word_of_nibble(uint32_t nibble) { return nibble >> 3; }
// word w of a map of `words` words; 0 (eight mixed tiles) outside it
DEXCT_UCOUNT_FN constexpr uint32_t checked_word(const uint32_t* map, uint32_t words, uint32_t w) { return w < words ? map[w] : 0u; }
// the nibbles from `nibble` on, out of its word and the one behind it
DEXCT_UCOUNT_FN constexpr uint32_t nibbles_from(uint32_t word, uint32_t next_word, uint32_t nibble) {
  return (uint32_t)(((uint64_t)next_word << 32 | word) >> ((nibble & 7u) << 2));
}
// the tile of a cell j across the slab axis, held to -1 .. tj: every cell outside the grid falls on an outside tile
DEXCT_UCOUNT_FN constexpr int32_t tile_of_cell(int32_t j, uint32_t tj) {
  const int32_t J = j >> kShift;      // (arithmetic: j < 0 gives J < 0)
  return J < -1 ? -1 : (J > (int32_t)tj ? (int32_t)tj : J);
}

// the class of tile (tx, ty) of the grid from the column-class map (ucount: four bits per column): all its columns uniform in
// one id; a tile that reaches past nx or ny is uniform only in air
DEXCT_UCOUNT_FN uint32_t class_of_tile(const uint32_t* col_class, uint32_t nx, uint32_t ny, uint32_t tx, uint32_t ty) {
  constexpr ucount::MapKind mk = ucount::map_kind(true);
  const uint32_t x0 = tx << kShift, y0 = ty << kShift;
  const bool partial = x0 + kSide > nx || y0 + kSide > ny;
  uint32_t first = 0u;
  bool same = true;
  for (uint32_t y = y0; y < y0 + kSide && y < ny; ++y)
    for (uint32_t x = x0; x < x0 + kSide && x < nx; ++x) {
      const uint32_t c = y * nx + x, e = ucount::class_in(col_class[ucount::word_of(c, mk)], c, mk);
      if (y == y0 && x == x0) first = e;
      same = same && e == first;
    }
  if (!same || (first & ucount::kUniform) == 0u) return 0u;
  return (partial && first != ucount::kAirClass) ? 0u : first;
}
// what the builder stores in nibble (I, J) of a copy: J = -1 and J = tj are the outside tiles
DEXCT_UCOUNT_FN uint32_t class_of_nibble(const uint32_t* col_class, uint32_t nx, uint32_t ny, int axis, uint32_t I, int32_t J) {
  const uint32_t tj = tiles_along(axis == 0 ? ny : nx);
  if (J < 0 || J >= (int32_t)tj) return ucount::kAirClass;
  return axis == 0 ? class_of_tile(col_class, nx, ny, I, (uint32_t)J) : class_of_tile(col_class, nx, ny, (uint32_t)J, I);
}

// ---- runs.  Run r of a ray (r = 0 .. n_runs - 1) is tile row first_run + r; it holds the slabs i_lo .. i_hi (at least one).
DEXCT_UCOUNT_FN constexpr int32_t first_run(int32_t i_first) { return i_first >> kShift; }
DEXCT_UCOUNT_FN constexpr int32_t n_runs(int32_t i_first, int32_t n_slabs) {
  return n_slabs > 0 ? ((i_first + n_slabs - 1) >> kShift) - (i_first >> kShift) + 1 : 0;
}
DEXCT_UCOUNT_FN constexpr int32_t run_i_lo(int32_t R, int32_t i_first) { return (R << kShift) > i_first ? (R << kShift) : i_first; }
DEXCT_UCOUNT_FN constexpr int32_t run_i_hi(int32_t R, int32_t i_first, int32_t n_slabs) {
  return (R << kShift) + kSide - 1 < i_first + n_slabs - 1 ? (R << kShift) + kSide - 1 : i_first + n_slabs - 1;
}
DEXCT_UCOUNT_FN constexpr int32_t cell_of(int64_t V0, int64_t SV, int32_t i) {
  return (int32_t)((int64_t)((uint64_t)V0 + (uint64_t)((int64_t)i * SV)) >> kFixFrac);
}
// The rule.  `nibbles`: the row's nibbles from tile J_lo on (nibbles_from); n_tiles = J_hi - J_lo + 1 >= 1 with J = tile_of_cell
// of the run's lowest and highest cell.  Returns the class the whole run is dropped in, or 0: the run survives.
DEXCT_UCOUNT_FN constexpr uint32_t dismissed_in(uint32_t nibbles, int32_t n_tiles) {
  const uint32_t c = nibbles & 15u;
  if (n_tiles > kTilesPerRun || (c & ucount::kUniform) == 0u) return 0u;
  const uint32_t m = (1u << (4 * n_tiles)) - 1u;
  return (nibbles & m) == ((c * 0x111u) & m) ? c : 0u;
}
// what a run dismissed in class e adds to the lane's register (ucount::bump per slab)
DEXCT_UCOUNT_FN constexpr uint32_t bump_run(uint32_t e, int32_t n_slabs_of_run) { return (uint32_t)n_slabs_of_run * ucount::bump(e); }

// ---- sharing-out.  The runs of a pair go to its lanes a WINDOW of kWindow at a time: run w0 + t + l to lane l, t = 0, lanes,
// 2 lanes ..; the surviving runs of the window are a 64-bit mask.  A PASS takes the next kRunsPerPass surviving runs of the
// mask; fine slab f of the pass (f = 0 .. kFineSlabs - 1, slab order) is slab f % kSide of the f / kSide-th of them.
// (rows16_kernel runs the first window only - grid_fits - and takes the k-th pass's runs by their rank, first = k kRunsPerPass,
// from the mask as it is: the same runs as after_pass applied k times.)
constexpr int kFineSlabs = 128;                         // kP16Super: the capacity of a pair's lists
constexpr int kRunsPerPass = kFineSlabs / kSide;
DEXCT_UCOUNT_FN constexpr int fine_rank(int f) { return f >> kShift; }
DEXCT_UCOUNT_FN constexpr int fine_slab(int f) { return f & (kSide - 1); }
// the k-th surviving run of the mask (k < popcount), and the mask without its first kRunsPerPass surviving runs
DEXCT_UCOUNT_FN constexpr int surviving_run(uint64_t mask, int k) { return gn_dedup::select_bit(mask, k); }
DEXCT_UCOUNT_FN constexpr uint64_t after_pass(uint64_t mask) {
  if (__builtin_popcountll(mask) <= kRunsPerPass) return 0u;
  return mask & ~gn_dedup::mask_through(gn_dedup::select_bit(mask, kRunsPerPass - 1));
}
// (gn_dedup::select_bit and mask_through are constexpr - DEXCT_GN_DEDUP_HD ends in it - so these two are usable at compile time)
static_assert(surviving_run(0xAull, 1) == 3 && after_pass(0x1FFFFull) == 0x10000ull && after_pass(0xFFFFull) == 0ull, "rank select at compile time");

// ---- the per-lane count (ucount::kFieldBits).  The bound is for the GENERAL sharing-out above - every window of the longest
// ray, kMaxRuns runs - which is more than rows16_kernel runs: it takes one window (grid_fits: at most kWindow runs, 64 slabs a
// lane at 16 lanes), so the bound holds for it with room, and stays right for a kernel that takes more windows.  In the run trips
// a lane takes one run in `lanes`: at most kSide slabs each.  In the passes a lane takes kFineSlabs / lanes fine slabs per pass,
// and a window of kWindow runs has at most kWindow / kRunsPerPass passes.
constexpr int kMaxRuns = (ucount::kMaxSlabs + kSide - 2) / kSide + 1;
DEXCT_UCOUNT_FN constexpr int lane_field_bound(int lanes) {
  const int from_runs = kSide * ((kMaxRuns + lanes - 1) / lanes);
  const int passes = ((kMaxRuns + kWindow - 1) / kWindow) * (kWindow / kRunsPerPass);
  return from_runs + passes * (kFineSlabs / lanes);
}
static_assert(lane_field_bound(ucount::kMinLanes) <= (int)ucount::kFieldMask, "a lane's field holds its share of the longest ray");
static_assert(kWindow % kRunsPerPass == 0 && kFineSlabs % kSide == 0, "whole runs per pass");

}  // namespace tiles
}  // namespace dexct
