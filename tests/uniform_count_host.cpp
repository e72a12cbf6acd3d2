// Host check of what the column-class map adds to the projection host layer and to rows16_kernel's classification:
//  - proj::class_counts_ok / proj::use_class_map (csrc/proj_pure.h): every mode of DEXCT_P16_UNIFORM and DEXCT_P16_AIR_SKIP, a
//    missing map, impossible counts (negative, past the grid, sums past the grid, sums that would overflow) and the share of
//    droppable columns at its boundary, the droppable columns spread over the ids in every way;
//  - ucount (csrc/uniform_count.h): the lookup in both kinds of map against a map built bit by bit, the drop rule over all pairs
//    of classes against its three cases spelled out, and the packed per-lane count against plain counters - the longest ray shared
//    out over the fewest lanes, all slabs in one id - with the sums over a pair taken as the kernel takes them.
// Built and run by tests/test_uniform_count_host.py, plainly and under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "proj_pure.h"
#include "uniform_count.h"

namespace {

int checks = 0, mismatches = 0;

void expect(long long got, long long want, const char* what, long long a, long long b) {
  ++checks;
  if (got != want) {
    ++mismatches;
    std::printf("MISMATCH %s (%lld, %lld): got %lld, want %lld\n", what, a, b, got, want);
  }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {      // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

void host_rule() {
  using namespace dexct::proj;
  const int64_t grids[] = {1, 2, 7, 8, 9, 31, 32, 33, 1023, 4096, 262144, 2047ll * 2047ll, 0x7FFFFF00ll, (int64_t)1 << 61, INT64_MAX};
  for (const int64_t n : grids) {
    const int64_t first = (int64_t)(((__int128)n * kAirMapShareNum + kAirMapShareDen - 1) / kAirMapShareDen);
    const int64_t totals[] = {0, 1, first - 1, first, first + 1, n - 1, n};
    for (const int64_t c : totals) {
      if (c < 0 || c > n) continue;
      // the droppable columns in one id, and split over two, three and four
      for (int split = 0; split < 7; ++split) {
        int64_t u[4] = {0, 0, 0, 0};
        if (split < 4) u[split] = c;
        else if (split == 4) { u[0] = c / 2; u[1] = c - c / 2; }
        else if (split == 5) { u[1] = c / 3; u[2] = c / 3; u[3] = c - 2 * (c / 3); }
        else { u[0] = c / 4; u[1] = c / 4; u[2] = c / 4; u[3] = c - 3 * (c / 4); }
        expect(class_counts_ok(u, n), true, "counts ok", c, n);
        for (int air = 0; air <= 2; ++air) {
          expect(use_class_map(1, air, true, u, n), air != 0 && c >= first, "auto", c, n);
          expect(use_class_map(2, air, true, u, n), air != 0, "forced", c, n);
          expect(use_class_map(0, air, true, u, n), false, "off", c, n);
          for (int mode = 0; mode <= 2; ++mode) expect(use_class_map(mode, air, false, u, n), false, "no map", c, n);
        }
      }
    }
    // counts the builder cannot have given never switch the map on
    for (int id = 0; id < 4; ++id) {
      int64_t neg[4] = {0, 0, 0, 0}, past[4] = {0, 0, 0, 0}, sum_past[4] = {0, 0, 0, 0}, huge[4] = {0, 0, 0, 0};
      neg[id] = -1;
      past[id] = n < INT64_MAX ? n + 1 : INT64_MIN;
      sum_past[id] = n;
      sum_past[(id + 1) % 4] = 1;
      huge[id] = INT64_MAX;
      huge[(id + 2) % 4] = INT64_MAX;
      for (const int64_t* bad : {neg, past, sum_past, huge}) {
        expect(class_counts_ok(bad, n), false, "impossible counts", id, n);
        for (int mode = 0; mode <= 2; ++mode) expect(use_class_map(mode, 2, true, bad, n), false, "impossible counts", id, n);
      }
    }
    expect(class_counts_ok(nullptr, n), false, "no counts", 0, n);
    expect(use_class_map(2, 2, true, nullptr, n), false, "no counts", 0, n);
  }
  const int64_t zero[4] = {0, 0, 0, 0};
  for (int mode = 0; mode <= 2; ++mode) {
    expect(use_class_map(mode, 1, true, zero, 0), false, "empty grid", 0, 0);
    expect(use_class_map(mode, 1, true, zero, -5), false, "negative grid", 0, -5);
  }
}

void lookups() {
  using namespace dexct::ucount;
  static_assert(kAirClass == class_of(0) && class_of(3) == 7u, "classes are uniform | id << 1");
  const uint32_t sizes[] = {1, 7, 8, 9, 31, 32, 33, 64, 1000, 2047u * 2047u};
  for (const uint32_t n_cols : sizes) {
    const uint32_t sample = n_cols < 5000 ? n_cols : 5000;
    for (int kind = 0; kind < 2; ++kind) {
      const MapKind k = map_kind(kind != 0);
      std::vector<uint32_t> words(map_words(n_cols, k), 0u);        // exactly the words the builders write: out-of-bounds is ASan's
      expect(words.size(), kind ? (n_cols + 7u) / 8u : (n_cols + 31u) / 32u, "words", n_cols, kind);
      std::vector<uint32_t> cols(sample), want(sample);
      for (uint32_t q = 0; q < sample; ++q) {
        cols[q] = n_cols < 5000 ? q : (q == 0 ? n_cols - 1 : rnd() % n_cols);
        // (a column drawn twice keeps its first class)
        bool seen = false;
        for (uint32_t p = 0; p < q && n_cols >= 5000 && !seen; ++p) seen = cols[p] == cols[q];
        if (seen) { want[q] = 0xFFFFFFFFu; continue; }
        const uint32_t cls = kind ? (rnd() % 5 == 0 ? 0u : class_of(rnd() % 4)) : rnd() % 2;
        want[q] = cls;
        if (kind) words[cols[q] / 8] |= cls << (4 * (cols[q] % 8));
        else words[cols[q] / 32] |= cls << (cols[q] % 32);
      }
      for (uint32_t q = 0; q < sample; ++q) {
        if (want[q] == 0xFFFFFFFFu) continue;
        const uint32_t w = word_of(cols[q], k);
        expect(w < words.size(), true, "word inside the map", cols[q], n_cols);
        expect(class_in(words[w], cols[q], k), want[q], "class", cols[q], kind);
      }
    }
  }
  // bit 3 of a nibble is not read: no id above 3 comes out of any word
  const MapKind k = map_kind(true);
  for (uint32_t c = 0; c < 8; ++c) expect(class_in(0xFFFFFFFFu, c, k), 7, "three bits", c, 0);
}

void rule_and_counts() {
  using namespace dexct::ucount;
  // droppable(ea, eb) against the three cases; an outside piece is kAirClass.  Classes 0 .. 7 (odd = uniform)
  for (uint32_t ea = 0; ea < 8; ++ea)
    for (uint32_t eb = 0; eb < 8; ++eb) {
      const bool ua = ea & 1u, ub = eb & 1u;
      const bool want = ua && ub && (ea >> 1) == (eb >> 1);
      expect(droppable(ea, eb), want, "drop rule", ea, eb);
    }
  expect(droppable(kAirClass, kAirClass), true, "all air", 0, 0);
  expect(droppable(kAirClass, class_of(1)), false, "outside piece against water", 0, 0);
  expect(droppable(class_of(1), class_of(2)), false, "two ids", 0, 0);
  expect(droppable(0u, 0u), false, "mixed", 0, 0);
  for (uint32_t id = 0; id < 4; ++id) {
    const uint32_t b = bump(class_of(id));
    expect(b, id == 0 ? 0u : 1u << (kFieldBits * (id - 1)), "bump", id, 0);
  }
  // the longest ray over the fewest lanes: every slab dropped, in one id or in random ids; the pair's sums as the kernel forms them
  for (const int lanes : {16, 32, 64})
    for (int pattern = 0; pattern < 5; ++pattern) {
      std::vector<uint32_t> reg(lanes, 0u);
      long long plain[4] = {0, 0, 0, 0};
      for (int s = 0; s < kMaxSlabs; ++s) {
        const uint32_t id = pattern < 4 ? (uint32_t)pattern : rnd() % 4;
        reg[s % lanes] += bump(class_of(id));
        ++plain[id];
      }
      uint32_t lo = 0, mid = 0;
      for (int l = 0; l < lanes; ++l) {
        lo += spread_lo(reg[l]);
        mid += spread_mid(reg[l]);
      }
      expect(lo & 0xFFFFu, plain[1], "id 1 of the pair", lanes, pattern);
      expect(mid, plain[2], "id 2 of the pair", lanes, pattern);
      expect(lo >> 16, plain[3], "id 3 of the pair", lanes, pattern);
    }
}

}  // namespace

int main() {
  host_rule();
  lookups();
  rule_and_counts();
  std::printf("%d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
