// Host check of the index arithmetic of rows16_kernel's list of distinct quads (csrc/dedup_index.h): the prefix counts, the
// entry every quad takes its results from, the pair an entry belongs to and the decision to detect the list at all, against a
// walk over the 256 quads in channel order.  Ballots: empty but for the first quad, full, single bits at the edges of the words,
// exactly 64 / 65 / 128 / 192 / 193 fresh quads, and random ones of every density.  Built and run by tests/test_dedup_index_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dedup_index.h"

namespace {

using namespace dexct::dedup;

int checks = 0, mismatches = 0;

void expect(long long got, long long want, const char* what, long long a, long long b) {
  ++checks;
  if (got != want) {
    ++mismatches;
    if (mismatches < 50) std::printf("MISMATCH %s (%lld, %lld): got %lld, want %lld\n", what, a, b, got, want);
  }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// one wave: the walk in channel order (quad 4 lane + q) against the header
void check_wave(const uint64_t (&fresh)[kRounds], int lanes_per_pair) {
  const int n_pairs = kWaveLanes / lanes_per_pair;
  int seen = 0, pair_end[4] = {0, 0, 0, 0};
  std::vector<int> owner;                       // pair of every entry
  for (int lane = 0; lane < kWaveLanes; ++lane) {
    for (int q = 0; q < kRounds; ++q) {
      if ((fresh[q] >> lane) & 1u) {
        ++seen;
        owner.push_back(lane / lanes_per_pair);
      }
      expect(prefix_inclusive(fresh, lane, q), seen, "prefix", lane, q);
      expect(source_entry(fresh, lane, q), seen - 1, "source", lane, q);
    }
    for (int k = 0; k < 4; ++k)
      if (lane == (k + 1) * lanes_per_pair - 1 || (lane == kWaveLanes - 1 && (k + 1) * lanes_per_pair >= kWaveLanes)) pair_end[k] = seen;
  }
  expect(fresh_total(fresh), seen, "total", seen, 0);
  for (int k = 0; k < 4; ++k) {
    const int last = ((k + 1) * lanes_per_pair < kWaveLanes ? (k + 1) * lanes_per_pair : kWaveLanes) - 1;
    expect(prefix_inclusive(fresh, last, kRounds - 1), pair_end[k], "pair end", k, lanes_per_pair);
  }
  for (int e = 0; e < seen; ++e) expect(entry_pair(e, pair_end, n_pairs), owner[e], "entry pair", e, lanes_per_pair);
}

// a ballot set with exactly n fresh quads, the first quad among them, spread over the rounds
void with_count(int n, uint64_t (&fresh)[kRounds]) {
  for (int q = 0; q < kRounds; ++q) fresh[q] = 0;
  fresh[0] = 1;
  int have = 1;
  while (have < n) {
    const int q = (int)(next() % kRounds), lane = (int)(next() % kWaveLanes);
    if (!((fresh[q] >> lane) & 1u)) {
      fresh[q] |= uint64_t(1) << lane;
      ++have;
    }
  }
}

}  // namespace

int main() {
  static_assert(entry_bytes(2) == 32 && entry_bytes(3) == 32 && entry_bytes(4) == 48, "sums in, 2 x 4 results out");
  static_assert(list_rounds(1) == 1 && list_rounds(64) == 1 && list_rounds(65) == 2 && list_rounds(128) == 2 && list_rounds(129) == 3 &&
                    list_rounds(192) == 3 && list_rounds(193) == 4 && list_rounds(256) == 4,
                "whole waves of entries");
  const int lpps[] = {16, 32, 64};
  uint64_t fresh[kRounds];
  for (const int lpp : lpps) {
    const uint64_t firsts = lpp == 64 ? 1ull : (lpp == 32 ? 0x0000000100000001ull : 0x0001000100010001ull);
    // only the first quad of every pair; everything; single bits at the edges of the 32-bit halves
    fresh[0] = firsts; fresh[1] = fresh[2] = fresh[3] = 0;
    check_wave(fresh, lpp);
    for (int q = 0; q < kRounds; ++q) fresh[q] = ~0ull;
    check_wave(fresh, lpp);
    const int edges[] = {0, 1, 15, 16, 31, 32, 33, 47, 48, 62, 63};
    for (const int lane : edges)
      for (int q = 0; q < kRounds; ++q) {
        fresh[0] = firsts; fresh[1] = fresh[2] = fresh[3] = 0;
        fresh[q] |= uint64_t(1) << lane;
        check_wave(fresh, lpp);
      }
    const int counts[] = {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256};
    for (const int n : counts) {
      with_count(n, fresh);
      check_wave(fresh, lpp);
      if (fresh_total(fresh) != n) ++mismatches;
    }
    for (int rep = 0; rep < 300; ++rep) {
      const int density = rep % 6;                // AND of `density` random words: from half the bits down to a few
      for (int q = 0; q < kRounds; ++q) {
        fresh[q] = next();
        for (int k = 0; k < density; ++k) fresh[q] &= next();
      }
      fresh[0] |= firsts;
      check_wave(fresh, lpp);
    }
  }
  // the decision: only where a round is saved and the list, with what is kept behind it, fits
  for (int nm = 2; nm <= 4; ++nm)
    for (int live = 0; live <= 4; ++live)
      for (int f = 0; f <= 256; ++f) {
        const int lds_sizes[] = {8192, 10240};
        for (const int lds : lds_sizes) {
          const int reserve = 304;
          const bool saves = f >= 1 && (f + 63) / 64 < live;
          const bool fits = (long long)f * entry_bytes(nm) + reserve <= lds;
          expect(use_list(f, live, nm, lds, reserve), saves && fits, "use_list", f, live);
          if (use_list(f, live, nm, lds, reserve)) {
            // every byte the list rounds touch lies inside the wave's LDS and below what is kept behind the list
            expect((long long)(f - 1) * entry_bytes(nm) + entry_bytes(nm) <= lds - reserve, 1, "list inside LDS", f, nm);
            expect((long long)(f - 1) * entry_bytes(nm) + kResultBytes <= lds - reserve, 1, "results inside the entry", f, nm);
            expect(f <= 192, 1, "an entry index fits 8 bits", f, nm);
          }
        }
      }
  std::printf("%d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
