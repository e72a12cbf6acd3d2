// Host check of the narrow list rounds of rows16_kernel (csrc/dedup_index.h: round_entries, round_rows, lane_entry, lane_first_row,
// lane_live, piece_in, piece_out).  For every list length 1 .. 256, with and without the one-row form: every (entry, row) is
// detected by exactly one live lane of exactly one round; the widths are what the rule says at the remainders 1, 16, 17, 32, 33, 64;
// no lane reads or writes a byte outside its entry, and no lane writes a byte that another lane of the round reads or writes
// (the results go over the sums, so a round must not depend on the order of its lanes).  The bytes are marked in a model of the
// list itself - a vector of exactly n_fresh entries - so that the sanitizers see every access.  Built and run by
// tests/test_dedup_narrow_host.py.
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

// the rule, restated: whole rounds at four rows; the last by its remainder
int want_rows(int n_fresh, int k, int min_rows) {
  const int left = n_fresh - 64 * k;
  int rows = 4;
  if (left < 64) rows = left <= 16 ? 1 : (left <= 32 ? 2 : 4);
  return rows < min_rows ? min_rows : rows;
}

void check_list(int n_fresh, int n_materials, int min_rows) {
  const int eb = entry_bytes(n_materials), n_sums = n_materials - 1;
  std::vector<int> detected(4 * (size_t)n_fresh, 0);            // [entry][row]: lanes that detect it, over all rounds
  const int rounds = list_rounds(n_fresh);
  int entries_seen = 0;
  for (int k = 0; k < rounds; ++k) {
    const int rows = round_rows(n_fresh, k, min_rows);
    expect(rows, want_rows(n_fresh, k, min_rows), "rows of the round", n_fresh, k);
    expect(rows == 1 || rows == 2 || rows == 4, 1, "1, 2 or 4 rows", n_fresh, k);
    expect(round_entries(n_fresh, k), n_fresh - 64 * k < 64 ? n_fresh - 64 * k : 64, "entries of the round", n_fresh, k);
    expect(round_entries(n_fresh, k) * (4 / rows) <= kWaveLanes, 1, "the round fits the wave", n_fresh, k);
    entries_seen += round_entries(n_fresh, k);
    // bytes of the list: who reads and who writes them in this round (lane + 1; 0: nobody)
    std::vector<int> reader((size_t)n_fresh * eb, 0), writer((size_t)n_fresh * eb, 0);
    for (int lane = 0; lane < kWaveLanes; ++lane) {
      const int e = lane_entry(rows, k, lane), first = lane_first_row(rows, lane);
      expect(lane_live(n_fresh, rows, k, lane), e < n_fresh, "live", n_fresh, lane);
      expect(e >= 64 * k && first >= 0 && first + rows <= 4, 1, "entry of this round, rows inside the quad", n_fresh, lane);
      if (!lane_live(n_fresh, rows, k, lane)) continue;
      for (int r = first; r < first + rows; ++r) ++detected.at(4 * (size_t)e + r);
      for (int m = 0; m < n_sums; ++m) {
        const int at = piece_in(m, first);
        expect(at >= 0 && at + 4 * rows <= eb, 1, "the piece read lies inside the entry", n_fresh, lane);
        for (int b = at; b < at + 4 * rows; ++b) reader.at((size_t)e * eb + b) = lane + 1;
      }
      for (int s = 0; s < 2; ++s) {
        const int at = piece_out(s, first);
        expect(at >= 0 && at + 4 * rows <= eb && at + 4 * rows <= kResultBytes, 1, "the piece written lies inside the entry", n_fresh, lane);
        for (int b = at; b < at + 4 * rows; ++b) {
          int& w = writer.at((size_t)e * eb + b);
          expect(w, 0, "one writer per byte", n_fresh, lane);
          w = lane + 1;
        }
      }
    }
    for (size_t b = 0; b < reader.size(); ++b)
      if (reader[b] && writer[b]) expect(writer[b], reader[b], "a byte is written by the lane that read it", n_fresh, (long long)b);
    // the results of a live entry are complete: 2 slots x 4 rows, where the copy to the stage looks for them
    for (int e = 64 * k; e < 64 * k + round_entries(n_fresh, k); ++e)
      for (int b = 0; b < kResultBytes; ++b) expect(writer.at((size_t)e * eb + b) != 0, 1, "all 32 result bytes written", n_fresh, e);
  }
  expect(entries_seen, n_fresh, "the rounds hold the list", n_fresh, rounds);
  for (size_t i = 0; i < detected.size(); ++i) expect(detected[i], 1, "every row of every entry detected once", n_fresh, (long long)i);
}

}  // namespace

int main() {
  // the widths at the remainders the rule names (one-row form built / not built)
  static_assert(round_rows(1, 0) == 1 && round_rows(16, 0) == 1 && round_rows(17, 0) == 2 && round_rows(32, 0) == 2 &&
                    round_rows(33, 0) == 4 && round_rows(64, 0) == 4,
                "first round");
  static_assert(round_rows(65, 0) == 4 && round_rows(65, 1) == 1 && round_rows(80, 1) == 1 && round_rows(81, 1) == 2 &&
                    round_rows(96, 1) == 2 && round_rows(97, 1) == 4 && round_rows(128, 1) == 4 && round_rows(128, 0) == 4,
                "second round");
  static_assert(round_rows(129, 2) == 1 && round_rows(160, 2) == 2 && round_rows(161, 2) == 4 && round_rows(192, 2) == 4 &&
                    round_rows(192, 1) == 4,
                "third round");
  static_assert(round_rows(1, 0, 2) == 2 && round_rows(16, 0, 2) == 2 && round_rows(17, 0, 2) == 2 && round_rows(33, 0, 2) == 4 &&
                    round_rows(16, 0, 4) == 4,
                "without the one-row form");
  static_assert(lane_entry(4, 1, 5) == 69 && lane_first_row(4, 5) == 0 && lane_entry(2, 1, 5) == 66 && lane_first_row(2, 5) == 2 &&
                    lane_entry(1, 1, 5) == 65 && lane_first_row(1, 5) == 1,
                "lane -> (entry, first row)");
  for (int nm = 2; nm <= 4; ++nm)
    for (int min_rows = 1; min_rows <= 4; min_rows *= 2)
      for (int f = 1; f <= 256; ++f) check_list(f, nm, min_rows);
  std::printf("%d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
