// dexct_gn_decompose_dedup: the index arithmetic of "solve repeated rows once, expand the results" (gn_dedup.hip).  Pure integer
// functions for host and device alike (tests/gn_dedup_index_host.cpp).
//
// The sinograms are [..][channel][row]; a LINE is the R consecutive rows of one channel, line l = pixels [l R, l R + R).  A pixel
// is FRESH when the bit patterns of its two counts differ from those of the row before it in its line (row 0 always is); every
// other pixel is a REPEAT and takes the result of the last fresh pixel at or before it.  The fresh pixels of the whole call, in
// the order of the pixels, are the LIST the Newton kernel solves: F entries in an array of `cap` places, filled FROM THE BACK, so
// that the kernel's tile queue, started at queue_head, hands out exactly the 64-pixel tiles that hold entries.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEXCT_GN_DEDUP_HD __host__ __device__ constexpr
#else
#define DEXCT_GN_DEDUP_HD constexpr
#endif

namespace dexct {
namespace gn_dedup {

constexpr int kTile = 64;                        // pixels of a tile of the Newton kernels (plain tiling)
constexpr int kWordBits = 64;                    // rows per word of a line's bit row
constexpr int kResultBytes = 16;                 // (a0, a1)
constexpr int kProbeStride = 64;                 // the probe reads every 64th line (every 16th cost an input without repeats up to 1.5 % of its launch, profiles/gn_dedup.md)
constexpr int kUseShare = 8;                     // the list is used while at most 1 / 8 of the pixels are fresh
constexpr int kScanBlock = 1024;                 // lines per block of the scan
constexpr int64_t kAlign = 256;                  // every array of the workspace starts on a multiple of this

// the descriptor: uint64 words at the start of the workspace
enum DescWord { kDescUse = 0, kDescFresh = 1, kDescCap = 2, kDescProbeFresh = 3, kDescProbeDone = 4, kDescProbePixels = 5, kDescWords = 8 };

// capacity of the list: an eighth of the pixels, in whole tiles
DEXCT_GN_DEDUP_HD int64_t capacity(int64_t n_pix) { return n_pix / kUseShare / kTile * kTile; }

// the sample's verdict, and the census's
DEXCT_GN_DEDUP_HD bool probe_votes_use(uint64_t sampled_fresh, uint64_t sampled_pixels) { return sampled_fresh * kUseShare <= sampled_pixels; }
DEXCT_GN_DEDUP_HD bool list_fits(int64_t n_fresh, int64_t cap) { return n_fresh <= cap; }
DEXCT_GN_DEDUP_HD int64_t probe_lines(int64_t n_lines) { return (n_lines + kProbeStride - 1) / kProbeStride; }

// where fresh pixel j (0 <= j < F) of the call goes, and the places before the first entry that share its tile (filled with
// the count 1.0)
DEXCT_GN_DEDUP_HD int64_t list_place(int64_t cap, int64_t n_fresh, int64_t j) { return cap - n_fresh + j; }
DEXCT_GN_DEDUP_HD int64_t pad_begin(int64_t cap, int64_t n_fresh) { return (cap - n_fresh) / kTile * kTile; }
DEXCT_GN_DEDUP_HD int64_t pad_end(int64_t cap, int64_t n_fresh) { return cap - n_fresh; }

// the word kWsQueueHead before the launch on the list (use = 0: every wave's first reservation finds the queue used up) ...
DEXCT_GN_DEDUP_HD int64_t list_queue_head(int64_t cap, int64_t n_fresh, bool use) { return use ? (cap - n_fresh) / kTile : cap / kTile; }
// ... and before the direct launch on the n_tiles tiles of the sinograms
DEXCT_GN_DEDUP_HD int64_t direct_queue_head(int64_t n_tiles, bool use) { return use ? n_tiles : 0; }

// a line's bit row: words_per_line words of 64 rows
DEXCT_GN_DEDUP_HD int words_per_line(int rows) { return (rows + kWordBits - 1) / kWordBits; }
DEXCT_GN_DEDUP_HD int word_of_row(int row) { return row / kWordBits; }
DEXCT_GN_DEDUP_HD int bit_of_row(int row) { return row % kWordBits; }
DEXCT_GN_DEDUP_HD int row_of(int word, int bit) { return word * kWordBits + bit; }
DEXCT_GN_DEDUP_HD int64_t word_index(int64_t line, int rows, int word) { return line * words_per_line(rows) + word; }
// the bits of a word up to and including `bit`
DEXCT_GN_DEDUP_HD uint64_t mask_through(int bit) { return bit >= kWordBits - 1 ? ~uint64_t(0) : (uint64_t(2) << bit) - 1u; }
// fresh pixels of the line up to and including the row, from the fresh pixels of its earlier words and its own word
DEXCT_GN_DEDUP_HD int rank_inclusive(int before, uint64_t word, int bit) { return before + __builtin_popcountll(word & mask_through(bit)); }

// the entry of the result array a pixel takes: base = fresh pixels of all earlier lines, rank = rank_inclusive >= 1
DEXCT_GN_DEDUP_HD int64_t result_place(int64_t cap, int64_t n_fresh, int64_t base, int rank) { return cap - n_fresh + base + rank - 1; }

// ---- the gather's batches -------------------------------------------------------------------------------------------------------
// A block of the gather takes a BATCH of consecutive lines: as many whole lines as have kGatherWords bit words between them (one
// line where a line alone has more), and works through the batch's words in chunks of kGatherWords.  The fresh pixels of a chunk
// are numbered j = 0, 1, ... in the order of the pixels; pixel j's word is found in the exclusive prefix sums of the words'
// popcounts, its bit by its rank within the word.
constexpr int kGatherWords = 256;
DEXCT_GN_DEDUP_HD int gather_batch_lines(int rows) { return words_per_line(rows) >= kGatherWords ? 1 : kGatherWords / words_per_line(rows); }
DEXCT_GN_DEDUP_HD int64_t gather_batches(int64_t n_lines, int rows) { return (n_lines + gather_batch_lines(rows) - 1) / gather_batch_lines(rows); }
// the last of the n (a power of two) words whose exclusive prefix is <= j: the word that holds fresh pixel j < the chunk's total
// (words without a fresh pixel share their prefix with the word after them, so the last such word is never one of them)
DEXCT_GN_DEDUP_HD int word_of_fresh(const uint32_t* prefix, int n, uint32_t j) {
  int i = 0;
  for (int step = n >> 1; step >= 1; step >>= 1)
    if (prefix[i + step] <= j) i += step;
  return i;
}
// the bit of the k-th set bit of `word`, k = 0 the lowest (k < popcount(word))
DEXCT_GN_DEDUP_HD int select_bit(uint64_t word, int k) {
  int bit = 0;
  for (int half = kWordBits / 2; half >= 1; half >>= 1) {
    const int low = __builtin_popcountll(word & ((uint64_t(1) << half) - 1u));
    if (k >= low) {
      k -= low;
      word >>= half;
      bit += half;
    }
  }
  return bit;
}
// the pixel of bit `bit` of the batch's word iw (0 = word 0 of the batch's first line, line0)
DEXCT_GN_DEDUP_HD int64_t pixel_of_batch_word(int64_t line0, int iw, int rows, int bit) {
  return (line0 + iw / words_per_line(rows)) * rows + row_of(iw % words_per_line(rows), bit);
}

// ---- the workspace: descriptor | bits | counts | bases | block sums of the scan | list of g1 | list of g2 | results ---------------
struct Layout {
  int64_t n_lines, cap;
  int64_t desc, bits, counts, bases, sums, list1, list2, results, bytes;       // byte offsets, and the size of it all
};

DEXCT_GN_DEDUP_HD int64_t align_up(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }
DEXCT_GN_DEDUP_HD int64_t scan_blocks(int64_t n_lines) { return (n_lines + kScanBlock - 1) / kScanBlock; }

// n_pix a multiple of rows >= 1; elem_bytes 4 / 8: the counts' type
DEXCT_GN_DEDUP_HD Layout layout(int64_t n_pix, int rows, int elem_bytes) {
  Layout y{};
  y.n_lines = n_pix / rows;
  y.cap = capacity(n_pix);
  y.desc = 0;
  y.bits = align_up(kDescWords * 8);
  y.counts = y.bits + align_up(y.n_lines * words_per_line(rows) * 8);
  y.bases = y.counts + align_up(y.n_lines * 4);
  y.sums = y.bases + align_up(y.n_lines * 4);
  y.list1 = y.sums + align_up(scan_blocks(y.n_lines) * 4);
  y.list2 = y.list1 + align_up(y.cap * elem_bytes);
  y.results = y.list2 + align_up(y.cap * elem_bytes);
  y.bytes = y.results + align_up(y.cap * kResultBytes);
  return y;
}

// whether the sizes allow the route at all (the other conditions - precision, pass, kernel - are the caller's)
DEXCT_GN_DEDUP_HD bool sizes_allow(int64_t n_pix, int64_t rows, int64_t channels) {
  return rows >= 1 && channels >= 1 && n_pix > 0 && n_pix < (int64_t(1) << 31) && n_pix % (rows * channels) == 0 && capacity(n_pix) >= kTile;
}

}  // namespace gn_dedup
}  // namespace dexct
