// Host check of the tile rule of rows16_kernel's tile forms (csrc/tile_class.h) and of proj::use_tile_map (csrc/proj_pure.h): a
// brute force over small grids that walks a ray twice - slab by slab under the slab rule of uniform_count.h, and as the kernel
// does, in run trips and passes of fine slabs - and asserts that
//  - a dismissed run holds only slabs the slab rule drops, all in the class the run was dismissed in;
//  - the per-id totals of a pair, summed as the kernel sums its lanes' registers, equal the slab rule's;
//  - the kept slabs are the same, in the same order;
//  - a tile that reaches past the grid never vouches for an id but air, and every tile's class is what its columns say;
//  - the fine-slab index reaches every slab of every surviving run exactly once, and no slab of a dismissed run;
//  - no lane's field passes lane_field_bound, which fits the field, at the longest ray over the fewest lanes;
//  - use_tile_map holds at its edges: share - 1, share, impossible counts;
//  - the words every tile row of the grid needs, the next word included, lie inside the map; the rows behind the grid that the
//    kernel's lanes without a run form lie in the spare word or behind the map, read 0 through the size check and dismiss nothing;
//  - grid_fits admits exactly the grids whose rays have at most kWindow runs.
// Built and run by tests/test_tile_class_host.py, plainly and under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "proj_pure.h"
#include "tile_class.h"

namespace {

using namespace dexct;

int checks = 0, mismatches = 0;
long long seen_dismissed = 0, seen_surviving = 0, seen_multi_pass = 0;      // what the rays exercised

void expect(long long got, long long want, const char* what, long long a, long long b) {
  ++checks;
  if (got != want) {
    ++mismatches;
    if (mismatches < 50) std::printf("MISMATCH %s (%lld, %lld): got %lld, want %lld\n", what, a, b, got, want);
  }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {      // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// ---- the two walks over one ray, on anything that can class a run and a slab -----------------------------------------------
struct Walk {
  long long total[4] = {0, 0, 0, 0};     // dropped slabs per id
  std::vector<int> kept;                 // the slabs i that reach a list, in order
  int max_field = 0;                     // the largest count any lane holds in one id
  int dismissed_runs = 0, surviving_runs = 0, passes = 0;
};

// slab_class(i): the class the slab rule drops slab i in, or 0 = kept.  (Air is class 1: dropped, counted for nothing.)
template <class SlabClass>
Walk slab_walk(int i_first, int n_slabs, SlabClass slab_class) {
  Walk w;
  for (int s = 0; s < n_slabs; ++s) {
    const uint32_t e = slab_class(i_first + s);
    if (e) ++w.total[e >> 1];
    else w.kept.push_back(i_first + s);
  }
  return w;
}

// run_class(R, i_lo, i_hi): the class run R is dismissed in, or 0.  The kernel's loops, lane by lane.
template <class RunClass, class SlabClass>
Walk tile_walk(int i_first, int n_slabs, int lanes, RunClass run_class, SlabClass slab_class, std::vector<int>& visits) {
  Walk w;
  std::vector<uint32_t> reg(lanes, 0u);
  std::vector<int> plain((size_t)lanes * 4, 0);
  const int R0 = tiles::first_run(i_first), n_runs = tiles::n_runs(i_first, n_slabs);
  visits.assign(n_slabs, 0);
  for (int w0 = 0; w0 < n_runs; w0 += tiles::kWindow) {
    uint64_t pending = 0;
    for (int t0 = 0; t0 < tiles::kWindow && w0 + t0 < n_runs; t0 += lanes)
      for (int li = 0; li < lanes; ++li) {
        const int r = w0 + t0 + li, R = R0 + r;
        if (r >= n_runs) continue;
        const int i_lo = tiles::run_i_lo(R, i_first), i_hi = tiles::run_i_hi(R, i_first, n_slabs);
        expect(i_lo <= i_hi && i_lo >= i_first && i_hi < i_first + n_slabs && (i_lo >> tiles::kShift) == R && (i_hi >> tiles::kShift) == R,
               true, "a run holds slabs of the ray, in its tile row", R, i_first);
        const uint32_t e = run_class(R, i_lo, i_hi);
        if (e) {
          ++w.dismissed_runs;
          reg[li] += tiles::bump_run(e, i_hi - i_lo + 1);
          plain[li * 4 + (e >> 1)] += i_hi - i_lo + 1;
          for (int i = i_lo; i <= i_hi; ++i) expect(slab_class(i), e, "a dismissed run holds slabs dropped in its class", i, R);
        } else {
          ++w.surviving_runs;
          pending |= uint64_t(1) << (t0 + li);
        }
      }
    while (pending) {
      ++w.passes;
      const int n_mine = __builtin_popcountll(pending) < tiles::kRunsPerPass ? __builtin_popcountll(pending) : tiles::kRunsPerPass;
      for (int f = 0; f < tiles::kFineSlabs; ++f) {
        if (tiles::fine_rank(f) >= n_mine) continue;
        const int run = tiles::surviving_run(pending, tiles::fine_rank(f));
        expect((pending >> run) & 1u, 1, "the rank select lands on a surviving run", run, f);
        const int i = ((R0 + w0 + run) << tiles::kShift) + tiles::fine_slab(f);
        if (i < i_first || i >= i_first + n_slabs) continue;
        ++visits[i - i_first];
        const uint32_t e = slab_class(i);
        const int li = f % lanes;
        if (e) {
          reg[li] += ucount::bump(e);
          ++plain[li * 4 + (e >> 1)];
        } else {
          w.kept.push_back(i);
        }
      }
      const uint64_t before = pending;
      pending = tiles::after_pass(pending);
      expect(__builtin_popcountll(before) - __builtin_popcountll(pending), n_mine, "a pass takes its runs off the mask", n_mine, 0);
      expect((pending & ~before) == 0 && (pending == 0 || pending > (before ^ pending)), true, "... the lowest ones", 0, 0);
    }
  }
  // the pair's sums as the kernel forms them
  uint32_t lo = 0, mid = 0;
  for (int l = 0; l < lanes; ++l) {
    lo += ucount::spread_lo(reg[l]);
    mid += ucount::spread_mid(reg[l]);
    for (int id = 1; id < 4; ++id) {
      if (plain[l * 4 + id] > w.max_field) w.max_field = plain[l * 4 + id];
      expect((reg[l] >> (ucount::kFieldBits * (id - 1))) & ucount::kFieldMask, plain[l * 4 + id], "a lane's field", l, id);
    }
  }
  w.total[1] = lo & 0xFFFFu;
  w.total[2] = mid;
  w.total[3] = lo >> 16;
  return w;
}

void compare(const Walk& slab, const Walk& tile, long long tag_a, long long tag_b) {
  for (int id = 1; id < 4; ++id) expect(tile.total[id], slab.total[id], "per-id total", tag_a, tag_b);
  expect(tile.kept == slab.kept, true, "kept slabs, in order", tag_a, tag_b);
}

// ---- grids ------------------------------------------------------------------------------------------------------------------
struct Grid {
  uint32_t nx, ny;
  std::vector<uint32_t> cls;        // per column
  std::vector<uint32_t> col_words;  // exactly the words of the class map: out of bounds is ASan's
  std::vector<uint32_t> tile_words; // exactly the words of the tile map
  tiles::Layout lay;
};

Grid make_grid(uint32_t nx, uint32_t ny, int flavour) {
  Grid g{nx, ny, std::vector<uint32_t>(nx * ny), {}, {}, tiles::layout(nx, ny)};
  // patches of one id with an offset against the tile grid, mixed columns sprinkled in: 0 sparse, 1 dense, 2 none (all uniform
  // tiles of random ids), 3 everything mixed, 4 one id everywhere
  const uint32_t ox = rnd() % 8, oy = rnd() % 8, patch = flavour == 2 ? 8 : 8 + 8 * (rnd() % 2);
  std::vector<uint32_t> patch_id(64 * 64);
  for (auto& p : patch_id) p = rnd() % 4;
  const uint32_t one = rnd() % 4;
  for (uint32_t y = 0; y < ny; ++y)
    for (uint32_t x = 0; x < nx; ++x) {
      uint32_t id = patch_id[((y + (flavour == 2 ? 0 : oy)) / patch) * 64 + (x + (flavour == 2 ? 0 : ox)) / patch];
      if (flavour == 4) id = one;
      uint32_t e = ucount::class_of(id);
      if (flavour == 0 && rnd() % 97 == 0) e = 0;
      if (flavour == 1 && rnd() % 9 == 0) e = 0;
      if (flavour == 3) e = 0;
      g.cls[y * nx + x] = e;
    }
  constexpr ucount::MapKind mk = ucount::map_kind(true);
  g.col_words.assign(ucount::map_words(nx * ny, mk), 0u);
  for (uint32_t c = 0; c < nx * ny; ++c) g.col_words[c / 8] |= g.cls[c] << (4 * (c % 8));
  g.tile_words.assign(g.lay.words, 0u);
  for (int axis = 0; axis < 2; ++axis)
    for (uint32_t I = 0; I < g.lay.ti[axis]; ++I)
      for (int32_t J = -1; J <= (int32_t)g.lay.tj[axis]; ++J) {
        const uint32_t nib = tiles::nibble_of(g.lay, axis, I, J);
        expect(tiles::word_of_nibble(nib) + 1 < g.tile_words.size(), true, "a nibble's word and the next lie inside the map", nib, axis);
        expect((g.tile_words[nib / 8] >> (4 * (nib % 8))) & 15u, 0, "no two tiles share a nibble", nib, axis);
        g.tile_words[nib / 8] |= tiles::class_of_nibble(g.col_words.data(), nx, ny, axis, I, J) << (4 * (nib % 8));
      }
  return g;
}

void check_tiles(const Grid& g) {
  const uint32_t tx = tiles::tiles_along(g.nx), ty = tiles::tiles_along(g.ny);
  expect(g.lay.ti[0] == tx && g.lay.tj[0] == ty && g.lay.ti[1] == ty && g.lay.tj[1] == tx, true, "layout", g.nx, g.ny);
  for (uint32_t J = 0; J < ty; ++J)
    for (uint32_t I = 0; I < tx; ++I) {
      // the tile's class from its columns, spelled out
      bool same = true, partial = false;
      uint32_t first = 0xFFu;
      for (uint32_t y = 8 * J; y < 8 * J + 8; ++y)
        for (uint32_t x = 8 * I; x < 8 * I + 8; ++x) {
          if (x >= g.nx || y >= g.ny) { partial = true; continue; }
          if (first == 0xFFu) first = g.cls[y * g.nx + x];
          same = same && g.cls[y * g.nx + x] == first;
        }
      uint32_t want = (same && (first & 1u)) ? first : 0u;
      if (partial && want != ucount::kAirClass) want = 0u;
      const uint32_t got = tiles::class_of_tile(g.col_words.data(), g.nx, g.ny, I, J);
      expect(got, want, "class of a tile", I, J);
      if (partial) expect(got == 0u || got == ucount::kAirClass, true, "a partial tile vouches for air only", I, J);
      // both copies hold it, between their outside tiles
      for (int axis = 0; axis < 2; ++axis) {
        const uint32_t nib = axis == 0 ? tiles::nibble_of(g.lay, 0, I, (int32_t)J) : tiles::nibble_of(g.lay, 1, J, (int32_t)I);
        expect((g.tile_words[nib / 8] >> (4 * (nib % 8))) & 15u, want, "the tile in its copy", I, J);
      }
    }
  for (int axis = 0; axis < 2; ++axis)
    for (uint32_t I = 0; I < g.lay.ti[axis]; ++I)
      for (const int32_t J : {-1, (int32_t)g.lay.tj[axis]}) {
        const uint32_t nib = tiles::nibble_of(g.lay, axis, I, J);
        expect((g.tile_words[nib / 8] >> (4 * (nib % 8))) & 15u, ucount::kAirClass, "an outside tile is air", I, J);
      }
}

// What a lane WITHOUT a run reads: the kernel's idle lanes form the nibble of tile rows I = ti, ti + 1, .. (up to kWindow rows behind
// the ray's last run) and read its word and the next like every other lane.  Those words are the spare word or lie behind the map:
// each must go through the size check (the vectors hold exactly the map's words: a read past them is ASan's), read 0 and dismiss
// nothing.  Also the words every tile row of the grid needs, word + 1 included, do lie inside the map.
long long seen_behind_map = 0, seen_spare_word = 0;
void idle_lanes(const Grid& g) {
  const uint32_t words = (uint32_t)g.tile_words.size();
  expect(words, g.lay.words, "the map has the layout's words", g.nx, g.ny);
  for (int axis = 0; axis < 2; ++axis) {
    const uint32_t ti = g.lay.ti[axis];
    const int32_t tj = (int32_t)g.lay.tj[axis];
    for (uint32_t I = 0; I < ti + (uint32_t)tiles::kWindow; ++I)
      for (int32_t J = -1; J <= tj; ++J) {
        const uint32_t nib = tiles::nibble_of(g.lay, axis, I, J), w = tiles::word_of_nibble(nib);
        if (I < ti) {
          expect(w + 1 < words, true, "a grid row's word and the next lie inside the map", I, J);
          continue;
        }
        seen_spare_word += w + 1 == words;
        seen_behind_map += w + 1 >= words;
        if (axis == 1) expect(w + 2 >= words, true, "a row behind copy 1 lies in its last word, the spare word or behind the map", I, J);
        const uint32_t lo = tiles::checked_word(g.tile_words.data(), words, w), hi = tiles::checked_word(g.tile_words.data(), words, w + 1);
        if (w >= words) expect(lo, 0, "a word behind the map reads 0", I, J);
        if (w + 1 >= words) expect(hi, 0, "the next word behind the map reads 0", I, J);
        if (w + 1 == words) expect(lo, 0, "the spare word is 0", I, J);
        if (w >= words - 1) for (int n = 1; n <= 3; ++n) expect(tiles::dismissed_in(tiles::nibbles_from(lo, hi, nib), n), 0, "nothing behind the map is dismissed", I, n);
      }
  }
}

void rays_on(const Grid& g) {
  constexpr ucount::MapKind mk = ucount::map_kind(true);
  const int64_t one = int64_t(1) << tiles::kFixFrac;
  for (int axis = 0; axis < 2; ++axis) {
    const int nu = axis == 0 ? (int)g.nx : (int)g.ny, nv = axis == 0 ? (int)g.ny : (int)g.nx;
    const uint32_t cu = axis == 0 ? 1u : g.nx, cv = axis == 0 ? g.nx : 1u;
    for (int k = 0; k < 60; ++k) {
      // slopes of both signs up to 1 and exactly 0, +1, -1; a start that lies inside, outside, or grazes a corner
      int64_t SV = (int64_t)(((uint64_t)rnd() << 9) % (uint64_t)(one + 1));
      if (k % 10 == 0) SV = one;
      if (k % 10 == 1) SV = 0;
      if (k % 10 == 2) SV = (int64_t)(rnd() % 1000);
      if (k & 1) SV = -SV;
      const int i_first = k % 3 == 0 ? 0 : (int)(rnd() % (uint32_t)nu);
      const int n_slabs = k % 3 == 0 ? nu : 1 + (int)(rnd() % (uint32_t)(nu - i_first));
      const int64_t j_start = (int64_t)(rnd() % (uint32_t)(nv + 12)) - 6;
      int64_t V0 = j_start * one + (int64_t)(((uint64_t)rnd() << 9) % (uint64_t)one) - (int64_t)i_first * SV;
      if (k % 10 == 3) V0 = (SV < 0 ? (int64_t)nv * one - 1 : 0) - (int64_t)i_first * SV;      // corner to corner
      const uint32_t tj = g.lay.tj[axis];
      auto slab_class = [&](int i) -> uint32_t {
        const int ja = tiles::cell_of(V0, SV, i), jb = tiles::cell_of(V0, SV, i + 1);
        const bool ina = (uint32_t)ja < (uint32_t)nv, inb = (uint32_t)jb < (uint32_t)nv;
        const uint32_t ca = (uint32_t)i * cu + (uint32_t)ja * cv, cb = (uint32_t)i * cu + (uint32_t)jb * cv;
        const uint32_t ea = ina ? ucount::class_in(g.col_words[ucount::word_of(ca, mk)], ca, mk) : ucount::kAirClass;
        const uint32_t eb = inb ? ucount::class_in(g.col_words[ucount::word_of(cb, mk)], cb, mk) : ucount::kAirClass;
        return ucount::droppable(ea, eb) ? eb : 0u;
      };
      auto run_class = [&](int R, int i_lo, int i_hi) -> uint32_t {
        const int j0 = tiles::cell_of(V0, SV, i_lo), j1 = tiles::cell_of(V0, SV, i_hi + 1);
        const int J_lo = tiles::tile_of_cell(j0 < j1 ? j0 : j1, tj), J_hi = tiles::tile_of_cell(j0 < j1 ? j1 : j0, tj);
        expect(J_hi - J_lo + 1 <= tiles::kTilesPerRun, true, "a run of slope <= 1 spans at most three tiles", J_lo, J_hi);
        const uint32_t nib = tiles::nibble_of(g.lay, axis, (uint32_t)R, J_lo);
        const uint32_t word = tiles::word_of_nibble(nib);
        expect(word + 1 < g.tile_words.size(), true, "a run of the ray reads inside the map", word, R);
        const uint32_t n_words = (uint32_t)g.tile_words.size();
        return tiles::dismissed_in(tiles::nibbles_from(tiles::checked_word(g.tile_words.data(), n_words, word),
                                                       tiles::checked_word(g.tile_words.data(), n_words, word + 1), nib), J_hi - J_lo + 1);
      };
      const Walk slab = slab_walk(i_first, n_slabs, slab_class);
      for (const int lanes : {16, 32, 64}) {
        std::vector<int> visits;
        const Walk tile = tile_walk(i_first, n_slabs, lanes, run_class, slab_class, visits);
        compare(slab, tile, g.nx * 100 + g.ny, k);
        seen_dismissed += tile.dismissed_runs;
        seen_surviving += tile.surviving_runs;
        seen_multi_pass += tile.passes > 1;
        // every slab of a surviving run once, no slab of a dismissed run
        const int R0 = tiles::first_run(i_first);
        for (int r = 0; r < tiles::n_runs(i_first, n_slabs); ++r) {
          const int i_lo = tiles::run_i_lo(R0 + r, i_first), i_hi = tiles::run_i_hi(R0 + r, i_first, n_slabs);
          const int want = run_class(R0 + r, i_lo, i_hi) ? 0 : 1;
          for (int i = i_lo; i <= i_hi; ++i) expect(visits[i - i_first], want, "visits of a slab", i, r);
        }
        expect(tile.max_field <= tiles::lane_field_bound(lanes), true, "a lane's field under its bound", tile.max_field, lanes);
      }
    }
  }
}

// the longest ray over the fewest lanes, with runs that are dismissed or survive in patterns of their own (no grid behind them)
void longest_ray() {
  expect(tiles::lane_field_bound(ucount::kMinLanes) <= (int)ucount::kFieldMask, true, "the bound fits the field", 0, 0);
  for (const int i_first : {0, 7, 3})
    for (int pattern = 0; pattern < 6; ++pattern)
      for (const int lanes : {16, 32, 64}) {
        const int n_slabs = ucount::kMaxSlabs;
        expect(tiles::n_runs(i_first, n_slabs) <= tiles::kMaxRuns, true, "runs of the longest ray", i_first, n_slabs);
        std::vector<uint32_t> run_e(tiles::kMaxRuns + 2), slab_e(n_slabs + 16);
        for (auto& e : run_e) e = pattern == 0 ? ucount::class_of(1) : pattern == 1 ? 0u : pattern == 2 ? (rnd() % 2 ? ucount::class_of(2) : 0u)
                                                                                                     : (rnd() % 4 ? 0u : ucount::class_of(1 + rnd() % 3));
        const int R0 = tiles::first_run(i_first);
        for (int i = i_first; i < i_first + n_slabs; ++i) {
          const uint32_t re = run_e[(i >> tiles::kShift) - R0];
          // the slabs of a surviving run: all droppable in one id (the worst for a lane's field), none, or random
          slab_e[i - i_first] = re ? re : pattern == 1 ? ucount::class_of(3) : pattern == 5 ? 0u : (rnd() % 3 ? ucount::class_of(1 + rnd() % 3) : 0u);
        }
        auto slab_class = [&](int i) { return slab_e[i - i_first]; };
        auto run_class = [&](int R, int, int) { return run_e[R - R0]; };
        std::vector<int> visits;
        const Walk slab = slab_walk(i_first, n_slabs, slab_class);
        const Walk tile = tile_walk(i_first, n_slabs, lanes, run_class, slab_class, visits);
        compare(slab, tile, pattern, lanes);
        seen_multi_pass += tile.passes > 1;      // (the small grids have at most eight runs to a ray: one pass)
        for (int s = 0; s < n_slabs; ++s) expect(visits[s], run_e[((i_first + s) >> tiles::kShift) - R0] ? 0 : 1, "visits of a slab", s, pattern);
        expect(tile.max_field <= tiles::lane_field_bound(lanes) && tile.max_field <= (int)ucount::kFieldMask, true, "a lane's field at the longest ray",
               tile.max_field, lanes);
      }
}

void host_rule() {
  using namespace dexct::proj;
  const int64_t grids[] = {1, 2, 7, 8, 9, 63, 64, 65, 4096, 65536, 256ll * 256ll, (int64_t)1 << 61, INT64_MAX};
  for (const int64_t n : grids) {
    const int64_t first = (int64_t)(((__int128)n * kTileMapShareNum + kTileMapShareDen - 1) / kTileMapShareDen);
    for (const int64_t c : {(int64_t)0, (int64_t)1, first - 1, first, first + 1, n - 1, n}) {
      if (c < 0 || c > n) continue;
      for (int split = 0; split < 5; ++split) {
        int64_t u[4] = {0, 0, 0, 0};
        if (split < 4) u[split] = c;
        else { u[0] = c / 4; u[1] = c / 4; u[2] = c / 4; u[3] = c - 3 * (c / 4); }
        expect(use_tile_map(1, true, u, n), c >= first, "auto", c, n);
        expect(use_tile_map(2, true, u, n), true, "forced", c, n);
        expect(use_tile_map(0, true, u, n), false, "off", c, n);
        for (int mode = 0; mode <= 2; ++mode) expect(use_tile_map(mode, false, u, n), false, "no map", c, n);
      }
    }
    for (int id = 0; id < 4; ++id) {
      int64_t neg[4] = {0, 0, 0, 0}, past[4] = {0, 0, 0, 0}, sum_past[4] = {0, 0, 0, 0}, huge[4] = {0, 0, 0, 0};
      neg[id] = -1;
      past[id] = n < INT64_MAX ? n + 1 : INT64_MIN;
      sum_past[id] = n;
      sum_past[(id + 1) % 4] = 1;
      huge[id] = INT64_MAX;
      huge[(id + 2) % 4] = INT64_MAX;
      for (const int64_t* bad : {neg, past, sum_past, huge})
        for (int mode = 0; mode <= 2; ++mode) expect(use_tile_map(mode, true, bad, n), false, "impossible counts", id, n);
    }
    for (int mode = 0; mode <= 2; ++mode) expect(use_tile_map(mode, true, nullptr, n), false, "no counts", mode, n);
  }
  const int64_t zero[4] = {0, 0, 0, 0};
  for (int mode = 0; mode <= 2; ++mode) expect(use_tile_map(mode, true, zero, 0), false, "empty grid", mode, 0);
}

void small_functions() {
  // the grids the one-window kernel takes: every ray has at most kWindow runs
  for (const uint32_t n : {1u, 8u, 511u, 512u, 513u, 520u, 2047u}) {
    expect(tiles::grid_fits(n, 16), n <= 512u, "grid_fits along x", n, 16);
    expect(tiles::grid_fits(16, n), n <= 512u, "grid_fits along y", 16, n);
    if (tiles::grid_fits(n, n))
      for (int i_first = 0; i_first < (int)n; i_first += 3) expect(tiles::n_runs(i_first, (int)n - i_first) <= tiles::kWindow, true, "runs of a ray in a grid that fits", n, i_first);
  }
  expect(tiles::n_runs(0, 512), tiles::kWindow, "the longest ray that fits has kWindow runs", 0, 512);
  expect(tiles::n_runs(0, 513), tiles::kWindow + 1, "one slab more is a run more", 0, 513);
  for (int j = -40; j < 90; ++j)
    for (const uint32_t tj : {1u, 2u, 3u, 8u}) {
      const int J = tiles::tile_of_cell(j, tj);
      const int want = j < 0 ? -1 : (j / 8 >= (int)tj ? (int)tj : j / 8);
      expect(J, want, "tile of a cell", j, tj);
    }
  // the rule on nibbles: every triple of classes, every count of tiles
  for (uint32_t x = 0; x < 4096; ++x)
    for (int n = 1; n <= 4; ++n) {
      const uint32_t c0 = x & 15u, c1 = (x >> 4) & 15u, c2 = (x >> 8) & 15u;
      const bool ok = n <= 3 && (c0 & 1u) && (n < 2 || c1 == c0) && (n < 3 || c2 == c0);
      expect(tiles::dismissed_in(x | 0xABCD0000u, n), ok ? c0 : 0u, "dismissed_in", x, n);
    }
  for (uint32_t nib = 0; nib < 16; ++nib)
    expect(tiles::nibbles_from(0x76543210u, 0xFEDCBA98u, nib & 7u) & 0xFFFu, ((nib & 7u) * 0x111u + 0x210u) & 0xFFFu, "nibbles across two words", nib, 0);
}

}  // namespace

int main() {
  small_functions();
  host_rule();
  const uint32_t sizes[] = {8, 13, 16, 17, 24, 64};
  for (const uint32_t nx : sizes)
    for (const uint32_t ny : sizes)
      for (int flavour = 0; flavour < 5; ++flavour) {
        const Grid g = make_grid(nx, ny, flavour);
        check_tiles(g);
        idle_lanes(g);
        rays_on(g);
      }
  longest_ray();
  expect(seen_behind_map > 1000 && seen_spare_word > 100, true, "idle lanes met the spare word and words behind the map", seen_behind_map, seen_spare_word);
  expect(seen_dismissed > 1000 && seen_surviving > 1000 && seen_multi_pass > 0, true, "the rays met dismissed runs, surviving runs and second passes",
         seen_dismissed, seen_surviving);
  std::printf("%d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
