// Host check of the index arithmetic of dexct_gn_decompose_dedup (csrc/gn_dedup_index.h): the list filled from the back, the pad
// range, the queue heads, the capacity rule, the bit rows and the workspace layout, for R in {1, 31, 32, 33, 63, 64, 65, 512} and
// F in {0, 1, 63, 64, 65, cap - 1, cap, cap + 1}.  Every place is written into a model of the workspace - one owner per byte - so
// an index that leaves its array, or the workspace, is seen.  Built and run by tests/test_gn_dedup_index_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gn_dedup_index.h"

namespace {

using namespace dexct::gn_dedup;

long long checks = 0, mismatches = 0;

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

// the workspace as owners of bytes: 0 nobody, else the array's number
struct Model {
  std::vector<uint8_t> owner;
  Layout y;
  int elem;
  Model(const Layout& layout, int elem_bytes) : owner((size_t)layout.bytes, 0), y(layout), elem(elem_bytes) {}
  // the array `id` at byte offset `at` with `n` elements of `size` bytes takes element i
  void touch(int id, int64_t at, int64_t n, int size, int64_t i, const char* what) {
    expect(i >= 0 && i < n, 1, what, i, n);
    if (i < 0 || i >= n) return;
    for (int b = 0; b < size; ++b) {
      const int64_t p = at + i * size + b;
      expect(p >= 0 && p < y.bytes, 1, "inside the workspace", p, y.bytes);
      if (p < 0 || p >= y.bytes) return;
      expect(owner[(size_t)p] == 0 || owner[(size_t)p] == id, 1, "one owner per byte", p, id);
      owner[(size_t)p] = (uint8_t)id;
    }
  }
};

// a sinogram of n_lines lines of R rows with exactly n_fresh fresh pixels (row 0 of every line among them), spread at random
std::vector<uint64_t> fresh_bits(int64_t n_lines, int R, int64_t n_fresh) {
  const int W = words_per_line(R);
  std::vector<uint64_t> bits((size_t)(n_lines * W), 0);
  for (int64_t l = 0; l < n_lines; ++l) bits[(size_t)word_index(l, R, 0)] |= 1u;
  int64_t left = n_fresh - n_lines;
  while (left > 0) {
    const int64_t l = (int64_t)(next() % (uint64_t)n_lines);
    const int r = (int)(next() % (uint64_t)R);
    uint64_t& w = bits[(size_t)word_index(l, R, word_of_row(r))];
    if (!((w >> bit_of_row(r)) & 1u)) { w |= uint64_t(1) << bit_of_row(r); --left; }
  }
  return bits;
}

void check_case(int R, int64_t n_lines, int64_t n_fresh, int elem) {
  const int64_t n_pix = n_lines * R, cap = capacity(n_pix);
  const Layout y = layout(n_pix, R, elem);
  expect(y.cap, cap, "layout cap", R, n_fresh);
  expect(y.n_lines, n_lines, "layout lines", R, n_fresh);
  expect(cap % kTile, 0, "cap in whole tiles", cap, 0);
  expect(cap <= n_pix / kUseShare && cap + kTile > n_pix / kUseShare, 1, "cap is an eighth, rounded down", cap, n_pix);
  const int64_t offs[] = {y.desc, y.bits, y.counts, y.bases, y.sums, y.list1, y.list2, y.results, y.bytes};
  for (int k = 0; k + 1 < 9; ++k) {
    expect(offs[k] % kAlign, 0, "aligned", k, offs[k]);
    expect(offs[k] < offs[k + 1], 1, "ascending", k, offs[k]);
  }
  const int W = words_per_line(R);
  Model m(y, elem);
  for (int k = 0; k < kDescWords; ++k) m.touch(1, y.desc, kDescWords, 8, k, "descriptor");
  for (int64_t b = 0; b < scan_blocks(n_lines); ++b) m.touch(5, y.sums, scan_blocks(n_lines), 4, b, "block sums");
  expect(scan_blocks(n_lines) * kScanBlock >= n_lines && (scan_blocks(n_lines) - 1) * kScanBlock < n_lines, 1, "scan blocks", n_lines, 0);
  // the bit rows: every row has one word and bit, and they give the row back
  for (int r = 0; r < R; ++r) {
    expect(row_of(word_of_row(r), bit_of_row(r)), r, "row round trip", r, R);
    expect(word_of_row(r) < W && bit_of_row(r) < kWordBits, 1, "word inside the line", r, R);
  }
  expect(row_of(W - 1, 0) < R && row_of(W, 0) >= R, 1, "words per line", R, W);
  for (int bit = 0; bit < kWordBits; ++bit) expect(__builtin_popcountll(mask_through(bit)), bit + 1, "mask through", bit, 0);

  const bool fits = list_fits(n_fresh, cap);
  expect(fits, n_fresh <= cap, "list fits", n_fresh, cap);
  expect(list_queue_head(cap, n_fresh, false), cap / kTile, "head without the list", cap, n_fresh);
  expect(direct_queue_head(12345, false), 0, "direct head, direct route", 0, 0);
  expect(direct_queue_head(12345, true), 12345, "direct head, list route", 0, 0);
  if (!fits || n_fresh < n_lines) return;            // (a census always finds row 0 of every line)

  // census, scan, gather and expand as the kernels index them
  const std::vector<uint64_t> bits = fresh_bits(n_lines, R, n_fresh);
  std::vector<int64_t> base((size_t)n_lines, 0);
  int64_t run = 0;
  for (int64_t l = 0; l < n_lines; ++l) {
    base[(size_t)l] = run;
    m.touch(3, y.counts, n_lines, 4, l, "counts");
    m.touch(4, y.bases, n_lines, 4, l, "bases");
    for (int k = 0; k < W; ++k) {
      m.touch(2, y.bits, n_lines * W, 8, word_index(l, R, k), "bits");
      run += __builtin_popcountll(bits[(size_t)word_index(l, R, k)]);
    }
  }
  expect(run, n_fresh, "census total", R, n_fresh);
  const int64_t head = list_queue_head(cap, n_fresh, true);
  expect(head * kTile, pad_begin(cap, n_fresh), "the head's tile starts the pad", cap, n_fresh);
  expect(pad_end(cap, n_fresh), list_place(cap, n_fresh, 0), "the pad ends at the first entry", cap, n_fresh);
  expect(pad_end(cap, n_fresh) - pad_begin(cap, n_fresh) < kTile && pad_begin(cap, n_fresh) <= pad_end(cap, n_fresh), 1, "pad within a tile", cap, n_fresh);
  expect(list_place(cap, n_fresh, n_fresh - 1), cap - 1, "the last entry is the list's last place", cap, n_fresh);
  expect(head >= 0 && head <= cap / kTile, 1, "head inside the queue", head, cap);
  expect((cap / kTile - head) * kTile >= n_fresh && (cap / kTile - head - 1) * kTile < n_fresh, 1, "exactly the tiles with entries", head, n_fresh);
  for (int64_t p = pad_begin(cap, n_fresh); p < pad_end(cap, n_fresh); ++p) {
    m.touch(6, y.list1, cap, elem, p, "pad of list 1");
    m.touch(7, y.list2, cap, elem, p, "pad of list 2");
  }
  std::vector<uint8_t> filled((size_t)cap, 0);
  int64_t j = 0;
  for (int64_t l = 0; l < n_lines; ++l) {
    int before = 0;
    for (int k = 0; k < W; ++k) {
      const uint64_t word = bits[(size_t)word_index(l, R, k)];
      for (int bit = 0; bit < kWordBits && row_of(k, bit) < R; ++bit) {
        const int rank = rank_inclusive(before, word, bit);
        const int64_t place = result_place(cap, n_fresh, base[(size_t)l], rank);
        if ((word >> bit) & 1u) {                    // gather: fresh pixel j of the call
          expect(place, list_place(cap, n_fresh, j), "gather place", l, row_of(k, bit));
          m.touch(6, y.list1, cap, elem, place, "list 1");
          m.touch(7, y.list2, cap, elem, place, "list 2");
          if (place >= 0 && place < cap) {
            expect(filled[(size_t)place], 0, "one pixel per place", place, j);
            filled[(size_t)place] = 1;
          }
          ++j;
        }
        // expand: the entry of the last fresh pixel at or before this one, inside the solved tiles
        expect(place, list_place(cap, n_fresh, j - 1), "expand place", l, row_of(k, bit));
        expect(place >= head * kTile && place < cap, 1, "expand reads a solved tile", place, head);
        m.touch(8, y.results, cap, kResultBytes, place, "results");
      }
      before += __builtin_popcountll(word);
    }
  }
  expect(j, n_fresh, "gathered", R, n_fresh);
  for (int64_t p = head * kTile; p < cap; ++p)
    expect(filled[(size_t)p] || (p >= pad_begin(cap, n_fresh) && p < pad_end(cap, n_fresh)), 1, "every place of a solved tile is an entry or a pad", p, cap);
}

}  // namespace

int main() {
  const int rows[] = {1, 31, 32, 33, 63, 64, 65, 512};
  for (int R : rows) {
    for (int64_t want_pix : {int64_t(512), int64_t(1024), int64_t(5000), int64_t(70000)}) {
      const int64_t n_lines = (want_pix + R - 1) / R, cap = capacity(n_lines * R);
      expect(sizes_allow(n_lines * R, R, 1), cap >= kTile, "sizes allow", R, n_lines);
      const int64_t fresh[] = {0, 1, 63, 64, 65, cap - 1, cap, cap + 1, n_lines, n_lines + 1, (n_lines + cap) / 2};
      for (int64_t f : fresh)
        for (int elem : {4, 8})
          if (f >= 0) check_case(R, n_lines, f, elem);
    }
  }
  // the probe's vote and the sample
  expect(probe_votes_use(8, 64), 1, "an eighth votes yes", 8, 64);
  expect(probe_votes_use(9, 64), 0, "more than an eighth votes no", 9, 64);
  expect(probe_votes_use(0, 0), 1, "nothing sampled", 0, 0);
  for (int64_t n : {1, 63, 64, 65, 128, 129, 800000}) expect(probe_lines(n), (n + 63) / 64, "sampled lines", n, 0);
  expect(sizes_allow(int64_t(1) << 31, 512, 1), 0, "2^31 pixels", 0, 0);
  expect(sizes_allow((int64_t(1) << 31) - 512, 512, 1), 1, "just below 2^31 pixels", 0, 0);
  expect(sizes_allow(511, 511, 1), 0, "no whole tile", 0, 0);
  expect(sizes_allow(1024, 512, 3), 0, "not whole views", 0, 0);
  // the benchmark's size: 1.3 GB
  const Layout big = layout(int64_t(409600000), 512, 4);
  expect(big.bytes > 1250000000ll && big.bytes < 1350000000ll, 1, "benchmark workspace", big.bytes, 0);
  std::printf("%lld checks, %lld mismatches\n", checks, mismatches);
  return mismatches == 0 ? 0 : 1;
}
