// rows16_kernel: the index arithmetic of "detect each distinct quad of rows once per wave" (siddon_packed.hip).  Pure integer
// functions of the four ballots of a wave, for host and device alike (tests/dedup_index_host.cpp).
//
// A QUAD is one lane's four rows of one detection round: quad (lane, q), q = 0..3, holds rows 16 lane + 4 q ... + 3 of the wave;
// in channel order it is number 4 lane + q.  A quad is FRESH when its sums differ bitwise from those of the quad before it (or
// when it is the first of its channel); fresh[q] is the ballot of "quad (lane, q) is fresh" over the lanes.  The fresh quads, in
// channel order, are the LIST the wave detects; every quad takes the result of the last fresh quad at or before it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEXCT_DEDUP_HD __host__ __device__ constexpr
#else
#define DEXCT_DEDUP_HD constexpr
#endif

namespace dexct {
namespace dedup {

constexpr int kWaveLanes = 64;
constexpr int kRounds = 4;                       // quads per lane
constexpr int kResultBytes = 32;                 // what a list entry receives: 2 spectrum slots x 4 rows

// bytes of a list entry: the 4 rows' sums of the NM - 1 materials going in, the results coming back over them
DEXCT_DEDUP_HD int entry_bytes(int n_materials) {
  const int in = (n_materials - 1) * 16;
  return in > kResultBytes ? in : kResultBytes;
}

// F: fresh quads of the wave
DEXCT_DEDUP_HD int fresh_total(const uint64_t (&fresh)[kRounds]) {
  int f = 0;
  for (int q = 0; q < kRounds; ++q) f += __builtin_popcountll(fresh[q]);
  return f;
}

// Fresh quads in channel order up to and including quad (lane, q), from what a lane of the kernel holds: below = fresh quads of
// all rounds in the lanes below it (v_mbcnt on the ballots), own = bit k set iff its quad k is fresh
DEXCT_DEDUP_HD int prefix_from_counts(int below, uint32_t own, int q) { return below + __builtin_popcount(own & ((2u << q) - 1u)); }

// the two from the ballots
DEXCT_DEDUP_HD int count_below(const uint64_t (&fresh)[kRounds], int lane) {
  int n = 0;
  for (int k = 0; k < kRounds; ++k) n += __builtin_popcountll(fresh[k] & ((uint64_t(1) << lane) - 1u));
  return n;
}
DEXCT_DEDUP_HD uint32_t own_bits(const uint64_t (&fresh)[kRounds], int lane) {
  uint32_t own = 0;
  for (int k = 0; k < kRounds; ++k) own |= (uint32_t)((fresh[k] >> lane) & 1u) << k;
  return own;
}
DEXCT_DEDUP_HD int prefix_inclusive(const uint64_t (&fresh)[kRounds], int lane, int q) {
  return prefix_from_counts(count_below(fresh, lane), own_bits(fresh, lane), q);
}

// the list entry whose result quad (lane, q) takes (its own slot if it is fresh); -1: no fresh quad at or before it
DEXCT_DEDUP_HD int source_entry(const uint64_t (&fresh)[kRounds], int lane, int q) { return prefix_inclusive(fresh, lane, q) - 1; }

// detection rounds of a list of n_fresh entries
DEXCT_DEDUP_HD int list_rounds(int n_fresh) { return (n_fresh + kWaveLanes - 1) / kWaveLanes; }

// Whether the wave detects the list instead of its live_rounds rounds of rows: only where that saves a round, and where the
// list fits the wave's LDS (lds_bytes; reserve_bytes of it are kept for other use)
DEXCT_DEDUP_HD bool use_list(int n_fresh, int live_rounds, int n_materials, int lds_bytes, int reserve_bytes) {
  if (n_fresh < 1 || list_rounds(n_fresh) >= live_rounds) return false;
  return (long long)n_fresh * entry_bytes(n_materials) + reserve_bytes <= (long long)lds_bytes;
}

// the pair (channel of the wave) a list entry belongs to: pair_end[k] = fresh quads of the pairs 0..k (ascending; the entries
// of a pair are consecutive)
DEXCT_DEDUP_HD int entry_pair(int entry, const int (&pair_end)[4], int n_pairs) {
  int g = 0;
  for (int k = 0; k + 1 < n_pairs; ++k) g += entry >= pair_end[k] ? 1 : 0;
  return g;
}

}  // namespace dedup
}  // namespace dexct
