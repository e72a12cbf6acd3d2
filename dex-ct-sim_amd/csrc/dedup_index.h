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

// ---- Narrow rounds.  A round of 64 entries detects four rows per lane: lane j takes entry 64 k + j.  The LAST round of a list
// may hold far fewer entries than the wave has lanes (an extruded wave: one entry per pair), and what a round costs follows the
// rows a lane carries, not the lanes that work.  So a last round of at most 32 entries runs with TWO rows per lane (lane j: rows
// 2 (j & 1), + 1 of entry 64 k + (j >> 1)) and one of at most 16 with ONE (lane j: row j & 3 of entry 64 k + (j >> 2)).
// The rows of a round are wave-uniform: a function of n_fresh and k alone.
constexpr int kRowsPerQuad = 4;

// entries of round k (0: the list has no such round)
DEXCT_DEDUP_HD int round_entries(int n_fresh, int k) {
  const int left = n_fresh - kWaveLanes * k;
  return left < 0 ? 0 : (left > kWaveLanes ? kWaveLanes : left);
}
// rows per lane of round k: 1, 2 or 4.  min_rows: the narrowest form the caller has (a kernel built without the one-row form
// runs its shortest lists two rows per lane)
DEXCT_DEDUP_HD int round_rows(int n_fresh, int k, int min_rows = 1) {
  const int n = round_entries(n_fresh, k);
  const int rows = n <= kWaveLanes / 4 ? 1 : (n <= kWaveLanes / 2 ? 2 : kRowsPerQuad);
  return rows < min_rows ? min_rows : rows;
}
// the entry lane j detects in round k at `rows` rows per lane, and the first of its rows inside the entry
DEXCT_DEDUP_HD int lane_entry(int rows, int k, int lane) { return kWaveLanes * k + lane / (kRowsPerQuad / rows); }
DEXCT_DEDUP_HD int lane_first_row(int rows, int lane) { return (lane % (kRowsPerQuad / rows)) * rows; }
// whether the lane has an entry at all (the others detect air and store nothing)
DEXCT_DEDUP_HD bool lane_live(int n_fresh, int rows, int k, int lane) { return lane_entry(rows, k, lane) < n_fresh; }
// Byte offsets inside an entry of the piece (4 * rows bytes) a lane reads for the m-th material that has a sum (m = 0: material 1)
// and of the piece it writes for spectrum slot s: the results go over the sums, as with four rows
DEXCT_DEDUP_HD int piece_in(int m, int first_row) { return 16 * m + 4 * first_row; }
DEXCT_DEDUP_HD int piece_out(int s, int first_row) { return 16 * s + 4 * first_row; }

// the pair (channel of the wave) a list entry belongs to: pair_end[k] = fresh quads of the pairs 0..k (ascending; the entries
// of a pair are consecutive)
DEXCT_DEDUP_HD int entry_pair(int entry, const int (&pair_end)[4], int n_pairs) {
  int g = 0;
  for (int k = 0; k + 1 < n_pairs; ++k) g += entry >= pair_end[k] ? 1 : 0;
  return g;
}

}  // namespace dedup
}  // namespace dexct
