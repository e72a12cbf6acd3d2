// Host check of the gather's batch arithmetic of dexct_gn_decompose_dedup (csrc/gn_dedup_index.h: gather_batch_lines,
// gather_batches, word_of_fresh, select_bit, pixel_of_batch_word).  The gather is played the way the kernel runs it - batch by
// batch, chunk by chunk, fresh pixel j of a chunk by "thread" j - on random bit rows, and must visit the fresh pixels of the call
// in the order of the pixels, each exactly once, at consecutive places from the first line's base on; every index into the
// chunk's prefix sums, the bit rows and the sinogram is checked against its array.  Built and run by
// tests/test_gn_dedup_gather_index_host.py.
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

uint64_t rng_state = 0xD1B54A32D192ED03ull;
uint64_t next() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// bit rows of n_lines lines of R rows: row 0 of every line, every other row with probability num / 8; kind 1: nothing after row
// 0, kind 2: every row (only bits of rows of the line are ever set: the census sets no other)
std::vector<uint64_t> bit_rows(int64_t n_lines, int R, int num, int kind) {
  const int W = words_per_line(R);
  std::vector<uint64_t> bits((size_t)(n_lines * W), 0);
  for (int64_t l = 0; l < n_lines; ++l)
    for (int r = 0; r < R; ++r) {
      const bool fresh = r == 0 || kind == 2 || (kind == 0 && (int)(next() % 8u) < num);
      if (fresh) bits[(size_t)word_index(l, R, word_of_row(r))] |= uint64_t(1) << bit_of_row(r);
    }
  return bits;
}

void play(int64_t n_lines, int R, int num, int kind) {
  const int W = words_per_line(R), batch = gather_batch_lines(R);
  const std::vector<uint64_t> bits = bit_rows(n_lines, R, num, kind);
  // what the census and the scan leave: the fresh pixels in the order of the pixels, and every line's base
  std::vector<int64_t> fresh, bases((size_t)n_lines);
  for (int64_t l = 0; l < n_lines; ++l) {
    bases[(size_t)l] = (int64_t)fresh.size();
    for (int r = 0; r < R; ++r)
      if ((bits[(size_t)word_index(l, R, word_of_row(r))] >> bit_of_row(r)) & 1u) fresh.push_back(l * R + r);
  }
  expect(batch >= 1 && (batch == 1 || (int64_t)batch * W <= kGatherWords) && (int64_t)(batch + 1) * W > kGatherWords, 1, "lines of a batch", R, batch);
  expect(gather_batches(n_lines, R), (n_lines + batch - 1) / batch, "batches", n_lines, R);
  int64_t lines_seen = 0, visited = 0;
  for (int64_t b = 0; b < gather_batches(n_lines, R); ++b) {
    const int64_t line0 = b * batch, lines_here = n_lines - line0 < batch ? n_lines - line0 : batch;
    expect(line0 < n_lines && lines_here >= 1, 1, "a batch has lines", b, n_lines);
    lines_seen += lines_here;
    const int64_t w_begin = line0 * W, n_here = lines_here * W;
    int64_t run = bases[(size_t)line0];
    for (int64_t iw0 = 0; iw0 < n_here; iw0 += kGatherWords) {
      uint64_t word[kGatherWords];
      uint32_t prefix[kGatherWords], total = 0;
      for (int t = 0; t < kGatherWords; ++t) {
        const int64_t iw = iw0 + t, at = w_begin + (iw < n_here ? iw : n_here - 1);
        expect(at >= 0 && at < (int64_t)bits.size(), 1, "word inside the bit rows", at, (long long)bits.size());
        word[t] = iw < n_here ? bits[(size_t)at] : 0;
        prefix[t] = total;
        total += (uint32_t)__builtin_popcountll(word[t]);
      }
      for (uint32_t j = 0; j < total; ++j) {
        const int i = word_of_fresh(prefix, kGatherWords, j);
        expect(i >= 0 && i < kGatherWords, 1, "word inside the chunk", i, j);
        if (i < 0 || i >= kGatherWords) continue;
        expect(prefix[i] <= j && j - prefix[i] < (uint32_t)__builtin_popcountll(word[i]), 1, "the word holds fresh pixel j", i, j);
        const int bit = select_bit(word[i], (int)(j - prefix[i]));
        expect(bit >= 0 && bit < kWordBits && ((word[i] >> bit) & 1u), 1, "a set bit", i, bit);
        const int64_t from = pixel_of_batch_word(line0, (int)iw0 + i, R, bit), to = run + j;
        expect(to >= 0 && to < (int64_t)fresh.size(), 1, "place inside the list", to, (long long)fresh.size());
        if (to >= 0 && to < (int64_t)fresh.size()) expect(from, fresh[(size_t)to], "pixel of the place", to, R);
        expect(to, visited, "places in order, each once", to, visited);
        ++visited;
      }
      run += total;
    }
    if (line0 + lines_here < n_lines) expect(run, bases[(size_t)(line0 + lines_here)], "a batch ends where the next begins", b, R);
  }
  expect(lines_seen, n_lines, "every line in one batch", n_lines, R);
  expect(visited, (int64_t)fresh.size(), "every fresh pixel moved", n_lines, R);
}

}  // namespace

int main() {
  // select_bit against counting, word_of_fresh against a walk
  for (int rep = 0; rep < 4000; ++rep) {
    uint64_t w = next();
    if (rep % 4 == 1) w &= next() & next();
    if (rep % 4 == 2) w |= next() | next();
    if (rep == 0) w = ~uint64_t(0);
    if (rep == 1) w = 1;
    if (rep == 2) w = uint64_t(1) << 63;
    int k = 0;
    for (int bit = 0; bit < kWordBits; ++bit)
      if ((w >> bit) & 1u) expect(select_bit(w, k++), bit, "select_bit", rep, bit);
  }
  for (int rep = 0; rep < 300; ++rep) {
    uint32_t prefix[kGatherWords], total = 0;
    for (int t = 0; t < kGatherWords; ++t) {
      prefix[t] = total;
      total += (rep % 3 == 0 && next() % 4u) ? 0u : (uint32_t)(next() % 65u);
    }
    for (uint32_t j = 0; j < total; j += 1 + (uint32_t)(next() % 7u)) {
      int want = 0;
      for (int t = 0; t < kGatherWords; ++t)
        if (prefix[t] <= j) want = t;
      expect(word_of_fresh(prefix, kGatherWords, j), want, "word_of_fresh", rep, j);
    }
  }
  expect(gather_batch_lines(1), kGatherWords, "batch lines", 1, 0);
  expect(gather_batch_lines(64), kGatherWords, "batch lines", 64, 0);
  expect(gather_batch_lines(65), kGatherWords / 2, "batch lines", 65, 0);
  expect(gather_batch_lines(130), kGatherWords / 3, "batch lines", 130, 0);
  expect(gather_batch_lines(512), kGatherWords / 8, "batch lines", 512, 0);
  expect(gather_batch_lines(64 * kGatherWords), 1, "batch lines", 64 * kGatherWords, 0);
  expect(gather_batch_lines(64 * kGatherWords + 1), 1, "batch lines", 64 * kGatherWords + 1, 0);
  // the gather played: rows with one to eight words and a partial last word, a line of exactly / more than a chunk's words; line
  // counts one below, at and one above a multiple of the batch, and a single line
  const int rows[] = {1, 31, 63, 64, 65, 130, 512, 64 * kGatherWords - 1, 64 * kGatherWords, 64 * kGatherWords + 1, 64 * kGatherWords * 2 + 70};
  for (int R : rows) {
    const int batch = gather_batch_lines(R);
    const int64_t lines[] = {1, batch - 1, batch, batch + 1, 3 * (int64_t)batch - 1, 3 * (int64_t)batch, 3 * (int64_t)batch + 1};
    for (int64_t n_lines : lines) {
      if (n_lines < 1 || n_lines * R > (int64_t(1) << 22)) continue;
      for (int num : {0, 1, 4, 8}) play(n_lines, R, num, 0);
      play(n_lines, R, 0, 1);
      play(n_lines, R, 0, 2);
    }
  }
  std::printf("%lld checks, %lld mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
