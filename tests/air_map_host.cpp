// Host check of the pure decisions of the projection host layer (csrc/proj_pure.h): when a launch of rows16_kernel looks
// columns up in the air-column map.  Every mode, a missing map, counts outside 0 .. n_cols, and the share of air columns at its
// boundary for grids from one column to 2047 x 2047.  Built and run by tests/test_air_map_host.py.
#include <cstdint>
#include <cstdio>

#include "proj_pure.h"

namespace {

int checks = 0, mismatches = 0;

void expect(bool got, bool want, const char* what, long long a, long long b) {
  ++checks;
  if (got != want) {
    ++mismatches;
    std::printf("MISMATCH %s (%lld, %lld): got %d, want %d\n", what, a, b, (int)got, (int)want);
  }
}

}  // namespace

int main() {
  using dexct::proj::kAirMapShareDen;
  using dexct::proj::kAirMapShareNum;
  using dexct::proj::use_air_map;
  static_assert(kAirMapShareNum > 0 && kAirMapShareDen >= kAirMapShareNum, "a share in (0, 1]");
  const int64_t grids[] = {1, 2, 7, 8, 9, 31, 32, 33, 1023, 4096, 262144, 2047ll * 2047ll, 0x7FFFFF00ll, (int64_t)1 << 61, INT64_MAX};
  for (const int64_t n : grids) {
    // the smallest count that reaches the share: ceil(n * num / den)
    const int64_t first = (int64_t)(((__int128)n * kAirMapShareNum + kAirMapShareDen - 1) / kAirMapShareDen);
    const int64_t counts[] = {0, 1, first - 1, first, first + 1, n - 1, n};
    for (const int64_t c : counts) {
      if (c < 0 || c > n) continue;
      expect(use_air_map(1, true, c, n), c >= first, "auto", c, n);
      expect(use_air_map(2, true, c, n), true, "forced", c, n);
      expect(use_air_map(0, true, c, n), false, "off", c, n);
      for (int mode = 0; mode <= 2; ++mode) expect(use_air_map(mode, false, c, n), false, "no map", c, n);
    }
    // counts the builder cannot have given never switch the map on
    for (int mode = 0; mode <= 2; ++mode) {
      expect(use_air_map(mode, true, -1, n), false, "negative count", -1, n);
      if (n < INT64_MAX) expect(use_air_map(mode, true, n + 1, n), false, "count past the grid", n + 1, n);
      expect(use_air_map(mode, true, INT64_MIN, n), false, "negative count", 0, n);
    }
  }
  for (int mode = 0; mode <= 2; ++mode) {
    expect(use_air_map(mode, true, 0, 0), false, "empty grid", 0, 0);
    expect(use_air_map(mode, true, 0, -5), false, "negative grid", 0, -5);
  }
  std::printf("%d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
