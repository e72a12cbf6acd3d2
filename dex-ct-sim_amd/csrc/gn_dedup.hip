// dexct_gn_decompose_dedup: solve repeated rows once, expand the results.
//
// The result of a float64 shared-spectrum Newton kernel is a pure function of a pixel's two counts (and the mask threshold).  In
// an extruded phantom most rows of a (view, channel) line carry bitwise the counts of the row below.  The passes here find the
// pixels that differ from the row before (FRESH), copy their counts into a list, and - after the unchanged Newton kernel has
// solved the list - write every pixel's result from the list's.  The index arithmetic is gn_dedup_index.h; the Newton launches
// and the order of it all are dexct_gn_decompose's host code (gn.hip).
//
//   probe    every 64th line: fresh pixels of the sample -> use = (share <= 1 / 8).  The only pass an input without repeats
//            pays: every kernel below returns at once when use = 0.
//   census   one bit per pixel (a 64-bit word per 64 rows of a line), one count per line
//   scan     exclusive scan of the counts (block sums, scan of the sums, bases): F; F > cap -> use = 0
//   gather   fresh pixel j -> list place cap - F + j; the places before it in its tile get the count 1.0.  A block takes a batch
//            of consecutive lines, loads their bit words at once, and thread j moves the batch's fresh pixel j
//   expand   pixel -> result place cap - F + base[line] + rank in the line - 1, tiles of 32 channels x 64 rows through LDS,
//            512-byte runs along the channels, non-temporal; a block walks up a column of tiles with a line's bit words in
//            registers and the next tile's results in flight
#include "gn_dedup.h"

namespace dexct {
namespace {

using namespace gn_dedup;

constexpr int kBlock = 256, kWavesPerBlock = kBlock / kWave;
constexpr int kMaxGrid = 2048;                   // the line and tile loops stride: a grid that returns at once stays cheap
constexpr int kExpandC = 32, kExpandR = kWordBits;       // the expansion's tile: channels x rows
typedef double d2 __attribute__((ext_vector_type(2)));

template <typename B> __device__ __forceinline__ B one_bits();
template <> __device__ __forceinline__ uint32_t one_bits<uint32_t>() { return 0x3F800000u; }
template <> __device__ __forceinline__ uint64_t one_bits<uint64_t>() { return 0x3FF0000000000000ull; }

// the ballot of "row r0 + lane of the line at `at` is fresh" (rows beyond the line: 0).  The four loads are unconditional - a row
// beyond the line reads the last one - so that the loads of several calls can be in flight together.
template <typename B>
__device__ __forceinline__ unsigned long long fresh_ballot(const B* __restrict__ g1, const B* __restrict__ g2, long long at, int r0,
                                                           int rows, int lane, bool valid = true) {
  const int r = r0 + lane, rc = r < rows ? r : rows - 1, rp = rc > 0 ? rc - 1 : 0;
  const B x1 = g1[at + rc], p1 = g1[at + rp], x2 = g2[at + rc], p2 = g2[at + rp];
  return __ballot(valid && r < rows && (r == 0 || x1 != p1 || x2 != p2));
}

// The probe.  Its work items are the 64-row words of the sampled lines, four of them in flight per wave; the blocks meet in ONE
// word, (blocks done << 40) + fresh pixels, so that a block pays one atomic and the last one holds the total.
constexpr int kProbeUnroll = 4, kProbeMaxGrid = 1024, kProbeDoneShift = 40;

template <typename B>
__global__ __launch_bounds__(kBlock) void gn_dedup_probe_kernel(const B* __restrict__ g1, const B* __restrict__ g2, long long n_sampled,
                                                                 int rows, long long cap, unsigned long long* __restrict__ desc) {
  __shared__ unsigned s_cnt[kWavesPerBlock];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, n_words = words_per_line(rows);
  const long long n_items = n_sampled * n_words, n_waves = (long long)gridDim.x * kWavesPerBlock;
  unsigned cnt = 0u;
  for (long long i0 = (long long)blockIdx.x * kWavesPerBlock + wv; i0 < n_items; i0 += kProbeUnroll * n_waves) {
    unsigned long long m[kProbeUnroll];
#pragma unroll
    for (int j = 0; j < kProbeUnroll; ++j) {
      const long long i = i0 + j * n_waves, ic = i < n_items ? i : n_items - 1;
      const long long s = ic / n_words;
      m[j] = fresh_ballot(g1, g2, s * kProbeStride * rows, row_of((int)(ic - s * n_words), 0), rows, lane, i < n_items);
    }
#pragma unroll
    for (int j = 0; j < kProbeUnroll; ++j) cnt += (unsigned)__popcll(m[j]);
  }
  if (lane == 0) s_cnt[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long mine = 1ull << kProbeDoneShift;
    for (int k = 0; k < kWavesPerBlock; ++k) mine += s_cnt[k];
    const unsigned long long all = atomicAdd(&desc[kDescProbeFresh], mine) + mine;
    if ((all >> kProbeDoneShift) == (unsigned long long)gridDim.x) {        // the last block: the verdict
      const unsigned long long fresh = all & ((1ull << kProbeDoneShift) - 1ull), pixels = (unsigned long long)n_sampled * rows;
      desc[kDescProbeFresh] = fresh;
      desc[kDescProbeDone] = (unsigned long long)gridDim.x;
      desc[kDescProbePixels] = pixels;
      desc[kDescCap] = (unsigned long long)cap;
      desc[kDescFresh] = 0ull;
      desc[kDescUse] = probe_votes_use(fresh, pixels) ? 1ull : 0ull;
    }
  }
}

template <typename B>
__global__ __launch_bounds__(kBlock) void gn_dedup_census_kernel(const B* __restrict__ g1, const B* __restrict__ g2, long long n_lines,
                                                                  int rows, const unsigned long long* __restrict__ desc,
                                                                  unsigned long long* __restrict__ bits, unsigned* __restrict__ counts) {
  if (desc[kDescUse] == 0ull) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, n_words = words_per_line(rows);
  for (long long line = (long long)blockIdx.x * kWavesPerBlock + wv; line < n_lines; line += (long long)gridDim.x * kWavesPerBlock) {
    unsigned cnt = 0u;
    for (int k = 0; k < n_words; ++k) {
      const unsigned long long m = fresh_ballot(g1, g2, line * rows, row_of(k, 0), rows, lane);
      if (lane == 0) bits[word_index(line, rows, k)] = m;
      cnt += (unsigned)__popcll(m);
    }
    if (lane == 0) counts[line] = cnt;
  }
}

// The census of float32 counts whose lines are whole 16-byte pieces (rows a multiple of 4, both sinograms aligned to 16 bytes;
// census_is_wide).  A lane loads FOUR rows of each sinogram in one piece, a wave 256 rows of a line = four bit words, and two
// such chunks are loaded before the first is looked at: 4 KB of distinct bytes in flight per wave where fresh_ballot has 1 KB,
// half of it the neighbour's (profiles/gn_route_streaming.md).  The row before a lane's first comes from the lane below (the
// chunk before: from its last lane), the comparison is the bit patterns' as in fresh_ballot, and a lane's four bits - its
// nibble - are OR-ed over the 16 lanes of a DPP row into the row's word: over quads, over half rows, and the upper half row's
// 32 bits into the lower's.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kWideRows = 4, kWideChunkWords = kWave * kWideRows / kWordBits, kWideUnroll = 2;
constexpr int kDppQuadSwap1 = 0xB1, kDppQuadSwap2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;

__host__ __device__ inline bool census_is_wide(const void* g1, const void* g2, int rows, bool f64) {
  return !f64 && rows % kWideRows == 0 && (reinterpret_cast<uintptr_t>(g1) & 15u) == 0 && (reinterpret_cast<uintptr_t>(g2) & 15u) == 0;
}

template <int CTRL>
__device__ __forceinline__ uint32_t or_dpp(uint32_t x) {
  return x | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
}

__global__ __launch_bounds__(kBlock) void gn_dedup_census_wide_kernel(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                                       long long n_lines, int rows, const unsigned long long* __restrict__ desc,
                                                                       unsigned long long* __restrict__ bits, unsigned* __restrict__ counts) {
  if (desc[kDescUse] == 0ull) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, n_words = words_per_line(rows);
  const int n_quads = rows / kWideRows, n_chunks = (n_quads + kWave - 1) / kWave;
  for (long long line = (long long)blockIdx.x * kWavesPerBlock + wv; line < n_lines; line += (long long)gridDim.x * kWavesPerBlock) {
    const u32x4* __restrict__ q1 = reinterpret_cast<const u32x4*>(g1 + line * rows);
    const u32x4* __restrict__ q2 = reinterpret_cast<const u32x4*>(g2 + line * rows);
    unsigned cnt = 0u;                                   // (lanes 0, 16, 32, 48: the fresh pixels of their words)
    uint32_t last1 = 0u, last2 = 0u;                     // the last row of the chunk before
    for (int j0 = 0; j0 < n_chunks; j0 += kWideUnroll) {
      u32x4 x1[kWideUnroll], x2[kWideUnroll];
#pragma unroll
      for (int u = 0; u < kWideUnroll; ++u) {            // (unconditional: a piece beyond the line reads the line's last)
        const int q = (j0 + u) * kWave + lane, qc = q < n_quads ? q : n_quads - 1;
        x1[u] = q1[qc];
        x2[u] = q2[qc];
      }
#pragma unroll
      for (int u = 0; u < kWideUnroll; ++u) {
        const int q = (j0 + u) * kWave + lane;
        uint32_t p1 = (uint32_t)__shfl_up((int)x1[u].w, 1), p2 = (uint32_t)__shfl_up((int)x2[u].w, 1);
        if (lane == 0) { p1 = last1; p2 = last2; }
        last1 = (uint32_t)__builtin_amdgcn_readlane((int)x1[u].w, kWave - 1);
        last2 = (uint32_t)__builtin_amdgcn_readlane((int)x2[u].w, kWave - 1);
        uint32_t nibble = (q == 0 || x1[u].x != p1 || x2[u].x != p2 ? 1u : 0u) | (x1[u].y != x1[u].x || x2[u].y != x2[u].x ? 2u : 0u) |
                          (x1[u].z != x1[u].y || x2[u].z != x2[u].y ? 4u : 0u) | (x1[u].w != x1[u].z || x2[u].w != x2[u].z ? 8u : 0u);
        if (q >= n_quads) nibble = 0u;
        uint32_t half = nibble << (kWideRows * (lane & 7));
        half = or_dpp<kDppRowHalfMirror>(or_dpp<kDppQuadSwap2>(or_dpp<kDppQuadSwap1>(half)));
        const uint32_t upper = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)half, kDppRowMirror, 0xF, 0xF, false);
        const unsigned long long word = ((unsigned long long)upper << 32) | half;
        const int k = (j0 + u) * kWideChunkWords + (lane >> 4);
        if ((lane & 15) == 0 && k < n_words) {
          bits[word_index(line, rows, k)] = word;
          cnt += (unsigned)__popcll(word);
        }
      }
    }
    cnt = (unsigned)(__builtin_amdgcn_readlane((int)cnt, 0) + __builtin_amdgcn_readlane((int)cnt, 16) + __builtin_amdgcn_readlane((int)cnt, 32) +
                     __builtin_amdgcn_readlane((int)cnt, 48));
    if (lane == 0) counts[line] = cnt;
  }
}

// exclusive scan of one value per thread over a block of N threads (s: N words of LDS); *total: the block's sum
template <int N>
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* s, unsigned* total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  unsigned x = v;
  for (int d = 1; d < N; d <<= 1) {
    const unsigned y = t >= d ? s[t - d] : 0u;
    __syncthreads();
    x += y;
    s[t] = x;
    __syncthreads();
  }
  *total = s[N - 1];
  __syncthreads();
  return x - v;
}

constexpr int kScanPerThread = kScanBlock / kBlock;

// the fresh pixels of each block of kScanBlock lines
__global__ __launch_bounds__(kBlock) void gn_dedup_sums_kernel(const unsigned* __restrict__ counts, long long n_lines,
                                                                const unsigned long long* __restrict__ desc, unsigned* __restrict__ sums) {
  if (desc[kDescUse] == 0ull) return;
  __shared__ unsigned s[kBlock];
  const long long first = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanPerThread;
  unsigned v = 0u;
  for (int q = 0; q < kScanPerThread; ++q) v += first + q < n_lines ? counts[first + q] : 0u;
  unsigned total;
  block_exclusive_scan<kBlock>(v, s, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: the sums become the blocks' bases; F; the list's capacity decides
__global__ __launch_bounds__(1024) void gn_dedup_scan_kernel(unsigned* __restrict__ sums, long long n_blocks,
                                                              unsigned long long* __restrict__ desc) {
  if (desc[kDescUse] == 0ull) return;
  __shared__ unsigned s[1024];
  unsigned long long carry = 0ull;
  for (long long b0 = 0; b0 < n_blocks; b0 += 1024) {
    const long long b = b0 + threadIdx.x;
    const unsigned v = b < n_blocks ? sums[b] : 0u;
    unsigned total;
    const unsigned ex = block_exclusive_scan<1024>(v, s, &total);
    if (b < n_blocks) sums[b] = (unsigned)carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    desc[kDescFresh] = carry;
    if (!list_fits((int64_t)carry, (int64_t)desc[kDescCap])) desc[kDescUse] = 0ull;
  }
}

// base[line] = fresh pixels of all earlier lines
__global__ __launch_bounds__(kBlock) void gn_dedup_bases_kernel(const unsigned* __restrict__ counts, long long n_lines,
                                                                 const unsigned long long* __restrict__ desc,
                                                                 const unsigned* __restrict__ sums, unsigned* __restrict__ bases) {
  if (desc[kDescUse] == 0ull) return;
  __shared__ unsigned s[kBlock];
  const long long first = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanPerThread;
  unsigned c[kScanPerThread], v = 0u;
  for (int q = 0; q < kScanPerThread; ++q) {
    c[q] = first + q < n_lines ? counts[first + q] : 0u;
    v += c[q];
  }
  unsigned total;
  unsigned run = sums[blockIdx.x] + block_exclusive_scan<kBlock>(v, s, &total);
  for (int q = 0; q < kScanPerThread; ++q) {
    if (first + q < n_lines) bases[first + q] = run;
    run += c[q];
  }
}

template <typename B>
__global__ __launch_bounds__(kBlock) void gn_dedup_gather_kernel(const B* __restrict__ g1, const B* __restrict__ g2, long long n_lines,
                                                                  int rows, const unsigned long long* __restrict__ desc,
                                                                  const unsigned long long* __restrict__ bits,
                                                                  const unsigned* __restrict__ bases, B* __restrict__ list1,
                                                                  B* __restrict__ list2) {
  if (desc[kDescUse] == 0ull) return;
  static_assert(kGatherWords == kBlock, "a thread per word of a chunk");
  __shared__ unsigned long long s_word[kGatherWords];
  __shared__ uint32_t s_prefix[kGatherWords];
  __shared__ unsigned s_wave[kWavesPerBlock];
  const long long n_fresh = (long long)desc[kDescFresh], cap = (long long)desc[kDescCap];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, n_words = words_per_line(rows), batch = gather_batch_lines(rows);
  if (blockIdx.x == 0 && wv == 0) {                      // the places that share the first entry's tile
    const long long p = pad_begin(cap, n_fresh) + lane;
    if (p < pad_end(cap, n_fresh)) { list1[p] = one_bits<B>(); list2[p] = one_bits<B>(); }
  }
  // The lines of a batch own consecutive places of the list, from list_place(base of the first line) on.  Every load of the
  // index - the base, the bit words - is issued up front and unconditionally (a word beyond the batch reads the batch's last and
  // counts as empty); the places then come from prefix sums of popcounts in LDS, so that thread j moves the chunk's fresh pixel j:
  // neighbouring threads write neighbouring places, and no load of a value waits for more than the chunk's words.
  for (long long b = blockIdx.x; b < gather_batches(n_lines, rows); b += gridDim.x) {
    const long long line0 = b * batch, lines_here = n_lines - line0 < batch ? n_lines - line0 : batch;
    const long long w_begin = line0 * n_words, n_here = lines_here * n_words;
    long long run = list_place(cap, n_fresh, bases[line0]);
    for (long long iw0 = 0; iw0 < n_here; iw0 += kGatherWords) {
      const long long iw = iw0 + threadIdx.x;
      unsigned long long word = bits[w_begin + (iw < n_here ? iw : n_here - 1)];
      if (iw >= n_here) word = 0ull;
      const unsigned mine = (unsigned)__popcll(word);
      unsigned upto = mine;                              // inclusive scan over the wave, then over the block's waves
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const unsigned y = __shfl_up(upto, d);
        if (lane >= d) upto += y;
      }
      if (lane == kWave - 1) s_wave[wv] = upto;
      __syncthreads();
      unsigned waves_before = 0u, total = 0u;
#pragma unroll
      for (int k = 0; k < kWavesPerBlock; ++k) {
        const unsigned c = s_wave[k];
        if (k < wv) waves_before += c;
        total += c;
      }
      s_word[threadIdx.x] = word;
      s_prefix[threadIdx.x] = waves_before + upto - mine;
      __syncthreads();
      for (unsigned j = threadIdx.x; j < total; j += kBlock) {
        const int i = word_of_fresh(s_prefix, kGatherWords, j);
        const long long from = pixel_of_batch_word(line0, (int)iw0 + i, rows, select_bit(s_word[i], (int)(j - s_prefix[i])));
        list1[run + j] = g1[from];
        list2[run + j] = g2[from];
      }
      run += total;
      __syncthreads();                                   // (the next chunk writes s_wave, s_word and s_prefix)
    }
  }
}

// *head: where the tile queue of the next Newton launch starts
__global__ void gn_dedup_list_head_kernel(const unsigned long long* __restrict__ desc, unsigned long long* __restrict__ head) {
  *head = (unsigned long long)list_queue_head((int64_t)desc[kDescCap], (int64_t)desc[kDescFresh], desc[kDescUse] != 0ull);
}

__global__ void gn_dedup_direct_head_kernel(const unsigned long long* __restrict__ desc, unsigned long long* __restrict__ head,
                                            unsigned long long* __restrict__ progress, long long direct_tiles) {
  const bool use = desc[kDescUse] != 0ull;
  *head = (unsigned long long)direct_queue_head(direct_tiles, use);
  if (use) *progress = 0ull;                             // (the list's pixels; the expansion counts the sinograms')
}

// the word of lane `l` (the same l in every lane) of a value every lane holds one of
__device__ __forceinline__ unsigned long long word_of_lane(unsigned long long x, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void gn_dedup_expand_kernel(const unsigned long long* __restrict__ desc,
                                                                  const unsigned long long* __restrict__ bits,
                                                                  const unsigned* __restrict__ bases, const d2* __restrict__ results,
                                                                  long long n_views, int rows, int channels, d2* __restrict__ out_a,
                                                                  unsigned long long* __restrict__ progress) {
  if (desc[kDescUse] == 0ull) return;
  __shared__ d2 tile[kExpandC][kExpandR + 1];            // (+ 1: the channel-wise reads spread over the banks)
  const long long n_fresh = (long long)desc[kDescFresh], cap = (long long)desc[kDescCap];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tiles_r = words_per_line(rows), tiles_c = (channels + kExpandC - 1) / kExpandC;
  constexpr int kPerWave = kExpandC / kWavesPerBlock, kRowsPerTrip = kBlock / kExpandC;
  const int co = threadIdx.x % kExpandC, ro0 = threadIdx.x / kExpandC;
  unsigned long long written = 0ull;
  // a block takes a COLUMN of tiles - kExpandC channels of a view, all rows - from the first row up: the fresh pixels of a line
  // before the tile's word are then a running sum, not a loop over the earlier words
  for (long long col = blockIdx.x; col < n_views * tiles_c; col += gridDim.x) {
    const int cb = (int)(col % tiles_c), c = cb * kExpandC + co;
    const long long v = col / tiles_c;
    // (the loads below are unconditional - a channel beyond the last reads the last, a row beyond the line the line's last
    // entry - so that all of a wave's lines are in flight together)
    long long line[kPerWave], base[kPerWave];
    int before[kPerWave];
    unsigned long long words[kPerWave];                  // lane l: word rb0 + l of the line's bit row (rb0: a multiple of 64)
    auto load_words = [&](int rb0) {
#pragma unroll
      for (int q = 0; q < kPerWave; ++q) words[q] = bits[word_index(line[q], rows, rb0 + lane < tiles_r ? rb0 + lane : tiles_r - 1)];
    };
    // in: a wave reads 64 rows of a line at a time (neighbouring lanes: the same or neighbouring entries of the results); the
    // place is arithmetic on registers
    auto load_values = [&](int rb, d2* val) {
#pragma unroll
      for (int q = 0; q < kPerWave; ++q) {
        const unsigned long long word = word_of_lane(words[q], rb % kWave);
        val[q] = results[result_place(cap, n_fresh, base[q], rank_inclusive(before[q], word, lane))];
        before[q] += (int)__popcll(word);
      }
    };
#pragma unroll
    for (int q = 0; q < kPerWave; ++q) {
      const int cq = cb * kExpandC + wv * kPerWave + q;
      line[q] = v * channels + (cq < channels ? cq : channels - 1);
      base[q] = bases[line[q]];
      before[q] = 0;
    }
    load_words(0);
    d2 val[kPerWave];
    load_values(0, val);
    for (int rb = 0; rb < tiles_r; ++rb) {
#pragma unroll
      for (int q = 0; q < kPerWave; ++q) tile[wv * kPerWave + q][lane] = val[q];
      if (rb + 1 < tiles_r) {                            // the next tile's values travel, into registers, while this one is written out
        if ((rb + 1) % kWave == 0) load_words(rb + 1);
        load_values(rb + 1, val);
      }
      __syncthreads();
      // out: kExpandC lanes write the channels of a row, one run
#pragma unroll
      for (int k = 0; k < kExpandR / kRowsPerTrip; ++k) {
        const int ro = ro0 + k * kRowsPerTrip, r = row_of(rb, ro);
        if (c < channels && r < rows) __builtin_nontemporal_store(tile[co][ro], out_a + ((v * rows + r) * channels + c));
      }
      __syncthreads();
    }
    const int nc = channels - cb * kExpandC < kExpandC ? channels - cb * kExpandC : kExpandC;
    written += (unsigned long long)nc * rows;
  }
  if (threadIdx.x == 0 && written) atomicAdd(progress, written);
}

unsigned capped_grid(long long n) { return (unsigned)(n < 1 ? 1 : (n > kMaxGrid ? kMaxGrid : n)); }

template <typename B>
int prepare(const GnDedupCall& dc, const void* g1v, const void* g2v, hipStream_t st) {
  const Layout y = dc.at();
  const B* g1 = reinterpret_cast<const B*>(g1v);
  const B* g2 = reinterpret_cast<const B*>(g2v);
  unsigned long long* desc = dc.array<unsigned long long>(y.desc);
  unsigned long long* bits = dc.array<unsigned long long>(y.bits);
  unsigned* counts = dc.array<unsigned>(y.counts);
  unsigned* bases = dc.array<unsigned>(y.bases);
  unsigned* sums = dc.array<unsigned>(y.sums);
  DEXCT_HIP_TRY(hipMemsetAsync(desc, 0, kDescWords * sizeof(unsigned long long), st));
  const long long n_sampled = probe_lines(y.n_lines), line_blocks = (y.n_lines + kWavesPerBlock - 1) / kWavesPerBlock;
  const long long probe_blocks = (n_sampled * words_per_line(dc.rows) + kWavesPerBlock * kProbeUnroll - 1) / (kWavesPerBlock * kProbeUnroll);
  hipLaunchKernelGGL(gn_dedup_probe_kernel<B>, dim3((unsigned)(probe_blocks > kProbeMaxGrid ? kProbeMaxGrid : probe_blocks)), dim3(kBlock), 0, st,
                     g1, g2, n_sampled, dc.rows, (long long)y.cap, desc);
  DEXCT_LAUNCH_CHECK();
  if (census_is_wide(g1v, g2v, dc.rows, sizeof(B) == 8))
    hipLaunchKernelGGL(gn_dedup_census_wide_kernel, dim3(capped_grid(line_blocks)), dim3(kBlock), 0, st, reinterpret_cast<const uint32_t*>(g1v),
                       reinterpret_cast<const uint32_t*>(g2v), (long long)y.n_lines, dc.rows, (const unsigned long long*)desc, bits, counts);
  else
    hipLaunchKernelGGL(gn_dedup_census_kernel<B>, dim3(capped_grid(line_blocks)), dim3(kBlock), 0, st, g1, g2, (long long)y.n_lines, dc.rows,
                       (const unsigned long long*)desc, bits, counts);
  DEXCT_LAUNCH_CHECK();
  const long long n_blocks = scan_blocks(y.n_lines);
  hipLaunchKernelGGL(gn_dedup_sums_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, (const unsigned*)counts, (long long)y.n_lines,
                     (const unsigned long long*)desc, sums);
  DEXCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_dedup_scan_kernel, dim3(1), dim3(1024), 0, st, sums, n_blocks, desc);
  DEXCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_dedup_bases_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, (const unsigned*)counts, (long long)y.n_lines,
                     (const unsigned long long*)desc, (const unsigned*)sums, bases);
  DEXCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_dedup_gather_kernel<B>, dim3(capped_grid(gather_batches(y.n_lines, dc.rows))), dim3(kBlock), 0, st, g1, g2, (long long)y.n_lines, dc.rows,
                     (const unsigned long long*)desc, (const unsigned long long*)bits, (const unsigned*)bases, dc.array<B>(y.list1),
                     dc.array<B>(y.list2));
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // namespace

int gn_dedup_prepare(const GnDedupCall& dc, const void* g1, const void* g2, hipStream_t st) {
  return dc.g_is_f64 ? prepare<uint64_t>(dc, g1, g2, st) : prepare<uint32_t>(dc, g1, g2, st);
}

int gn_dedup_list_head(const GnDedupCall& dc, unsigned long long* head, hipStream_t st) {
  hipLaunchKernelGGL(gn_dedup_list_head_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)dc.array<unsigned long long>(dc.at().desc), head);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int gn_dedup_direct_head(const GnDedupCall& dc, unsigned long long* head, unsigned long long* progress, int64_t direct_tiles, hipStream_t st) {
  hipLaunchKernelGGL(gn_dedup_direct_head_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)dc.array<unsigned long long>(dc.at().desc),
                     head, progress, (long long)direct_tiles);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

int gn_dedup_expand(const GnDedupCall& dc, double* out_a, unsigned long long* progress, hipStream_t st) {
  const Layout y = dc.at();
  const long long n_views = dc.n_pix / ((long long)dc.rows * dc.channels);
  const long long n_columns = n_views * ((dc.channels + kExpandC - 1) / kExpandC);
  hipLaunchKernelGGL(gn_dedup_expand_kernel, dim3(capped_grid(n_columns)), dim3(kBlock), 0, st,
                     (const unsigned long long*)dc.array<unsigned long long>(y.desc), (const unsigned long long*)dc.array<unsigned long long>(y.bits),
                     (const unsigned*)dc.array<unsigned>(y.bases), (const d2*)dc.array<d2>(y.results), n_views, dc.rows, dc.channels,
                     reinterpret_cast<d2*>(out_a), progress);
  DEXCT_LAUNCH_CHECK();
  return DEXCT_OK;
}

}  // namespace dexct
