// Host check of the bit-sliced counters of rows16_kernel (csrc/sliced_count.h, portable adders): word streams go
// through add16 / add8 / add4 in mixed order, as the two sweeps of the kernel interleave them, and every one of the 32
// counters must equal the plain per-bit count.  Built and run by tests/test_sliced_count_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sliced_count.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rng() {          // splitmix64, high half
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

enum Pattern { kRandom, kSparse, kOnes, kZeros, kAlternating, kSingleBit, kNumPatterns };
const char* const kPatternName[] = {"random", "sparse", "ones", "zeros", "alternating", "single-bit"};

std::vector<uint32_t> make_stream(Pattern p, int n, int bit) {
  std::vector<uint32_t> w((size_t)n);
  for (int i = 0; i < n; ++i) {
    switch (p) {
      case kRandom: w[i] = rng(); break;
      case kSparse: w[i] = rng() & rng() & rng(); break;
      case kOnes: w[i] = 0xFFFFFFFFu; break;
      case kZeros: w[i] = 0u; break;
      case kAlternating: w[i] = (i & 1) ? 0xAAAAAAAAu : 0x55555555u; break;
      default: w[i] = 1u << bit; break;
    }
  }
  return w;
}

// the chunk sizes a schedule cycles through; a chunk that does not fit the rest of the stream gives way to the next
// smaller one, and the last words are padded with zeros (air) to a chunk of 4, as the kernel pads its lists
const int kSchedules[][4] = {{16, 16, 16, 16}, {8, 8, 8, 8}, {4, 4, 4, 4}, {16, 8, 4, 8}, {4, 8, 16, 4}, {8, 16, 16, 8}, {16, 4, 16, 8}};
constexpr int kNumSchedules = sizeof(kSchedules) / sizeof(kSchedules[0]);

template <int N>
void feed(dexct::Sliced& s, const uint32_t* w, int have) {
  uint32_t x[N];
  for (int q = 0; q < N; ++q) x[q] = q < have ? w[q] : 0u;
  if constexpr (N == 16) s.add16(x);
  else if constexpr (N == 8) s.add8(x);
  else s.add4(x);
}

int check(Pattern p, int n, int bit, int schedule) {
  const std::vector<uint32_t> w = make_stream(p, n, bit);
  dexct::Sliced s;
  int at = 0, turn = 0;
  while (at < n) {
    int chunk = kSchedules[schedule][turn++ & 3];
    while (chunk > 4 && chunk > n - at) chunk >>= 1;
    const int have = n - at < chunk ? n - at : chunk;
    if (chunk == 16) feed<16>(s, w.data() + at, have);
    else if (chunk == 8) feed<8>(s, w.data() + at, have);
    else feed<4>(s, w.data() + at, have);
    at += have;
  }
  uint32_t got[32];
  s.unslice(got);
  int bad = 0;
  for (int b = 0; b < 32; ++b) {
    uint32_t want = 0;
    for (int i = 0; i < n; ++i) want += (w[i] >> b) & 1u;
    if (got[b] != want) {
      std::printf("MISMATCH %s n=%d schedule=%d bit=%d: counter %u, plain count %u\n", kPatternName[p], n, schedule, b, got[b], want);
      ++bad;
    }
  }
  return bad;
}

}  // namespace

int main() {
  const int lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 2047};
  int bad = 0, cases = 0;
  for (int schedule = 0; schedule < kNumSchedules; ++schedule)
    for (int n : lengths)
      for (int p = 0; p < kNumPatterns; ++p) {
        if (p == kSingleBit) {
          for (int bit : {0, 1, 15, 30, 31}) { bad += check(kSingleBit, n, bit, schedule); ++cases; }
        } else {
          bad += check((Pattern)p, n, 0, schedule);
          ++cases;
        }
      }
  // 2047 all-ones words: every counter at 2047, all 11 planes set
  {
    const std::vector<uint32_t> w = make_stream(kOnes, 2047, 0);
    dexct::Sliced s;
    int at = 0;
    for (; at + 16 <= 2047; at += 16) feed<16>(s, w.data() + at, 16);
    feed<16>(s, w.data() + at, 2047 - at);
    const uint32_t planes[11] = {s.ones, s.twos, s.fours, s.eights, s.hi[0], s.hi[1], s.hi[2], s.hi[3], s.hi[4], s.hi[5], s.hi[6]};
    for (int k = 0; k < 11; ++k)
      if (planes[k] != 0xFFFFFFFFu) { std::printf("MISMATCH plane %d of the full counters: %08x\n", k, planes[k]); ++bad; }
    uint32_t got[32];
    s.unslice(got);
    for (int b = 0; b < 32; ++b)
      if (got[b] != 2047u) { std::printf("MISMATCH full counter %d: %u\n", b, got[b]); ++bad; }
    ++cases;
  }
  std::printf("%d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
