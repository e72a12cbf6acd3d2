// Column classes of rows16_kernel's SKIP forms (siddon_packed.hip): the lookup in either kind of column map, the rule that lets a
// slab leave the lists, and the per-lane register that counts the slabs that left, per id.  The one copy; plain C++, so that a
// host program can include it (tests/uniform_count_host.cpp, also under the sanitizers).
//
// WHY EVERY OUTPUT KEEPS ITS BYTES.  A ray's sum for material m is (float)(int32) count_m + corrections_m.
//   count_m is an integer: the number of listed slabs whose counted voxel - the slab's voxel for a full slab, the b piece for a
//   crossing slab - has id m in that row.  A slab whose counted voxel lies in a column uniform in id m adds 1 to count_m of EVERY
//   row, so counting it in one integer per pair and adding that integer to every row's integer after the un-slicing, before the
//   conversion to float, gives the same integer.  (The kernel counts flag planes, not ids: id 1 sets plane 0, id 2 plane 1, id 3
//   both and the "both" plane; the per-pair integers are added plane by plane, which is what the sweeps would have done.)
//   corrections_m are float32 sums in slab order and must not be reordered; a crossing slab corrects only where its two words
//   differ.  So a slab leaves the lists ONLY when
//     1. it is a full slab in a uniform column,
//     2. it is a crossing slab whose two pieces both lie inside the grid, in uniform columns of the SAME id, or
//     3. all its pieces inside the grid are air (a piece outside the grid reads as air),
//   all three of which are droppable(ea, eb) below with an outside piece classed as uniform air.  Two equal words cause no
//   correction, so nothing is taken out of a float sum.  A crossing slab between uniform columns of different ids, one with a
//   piece outside the grid next to a uniform non-air column, and every slab that touches a mixed column stay in their list at
//   their place.  A column counts as uniform only when one id fills ALL nz / 4 bytes of it: every voxel any lane can load,
//   whatever z_first and n_rows are.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DEXCT_UCOUNT_FN __host__ __device__ __forceinline__
#else
#define DEXCT_UCOUNT_FN inline
#endif

namespace dexct {
namespace ucount {

// ---- classes: 0 = mixed, kUniform | id << 1 = one id over all z (include/dexct_p16_uniform.h: DEXCT_COL_CLASS)
constexpr uint32_t kUniform = 1u;
constexpr uint32_t kAirClass = kUniform;           // uniform in id 0; also what a piece outside the grid counts as
DEXCT_UCOUNT_FN constexpr uint32_t class_of(uint32_t id) { return kUniform | id << 1; }

// ---- the two kinds of map behind one lookup (wave-uniform words: the lookup costs the same instructions for both).
// Air map (dexct_volume_air_columns): one bit per column, 32 columns per word; a set bit reads as kAirClass, a clear one as
// mixed - which gives exactly the air rule.  Class map (dexct_volume_column_classes): four bits per column, eight per word, of
// which the low three are read (bit 3 is 0 in every map the builder makes; a map from elsewhere cannot name an id above 3).
struct MapKind {
  uint32_t word_shift;     // column -> word
  uint32_t col_mask;       // column -> place in its word
  uint32_t bit_shift;      // place -> bit
  uint32_t class_mask;
};
DEXCT_UCOUNT_FN constexpr MapKind map_kind(bool class_map) { return class_map ? MapKind{3u, 7u, 2u, 7u} : MapKind{5u, 31u, 0u, 1u}; }
DEXCT_UCOUNT_FN constexpr uint32_t word_of(uint32_t col, const MapKind& k) { return col >> k.word_shift; }
DEXCT_UCOUNT_FN constexpr uint32_t class_in(uint32_t word, uint32_t col, const MapKind& k) {
  return (word >> ((col & k.col_mask) << k.bit_shift)) & k.class_mask;
}
// words of a map of n_cols columns (n_cols >= 1)
DEXCT_UCOUNT_FN constexpr uint32_t map_words(uint32_t n_cols, const MapKind& k) { return ((n_cols - 1u) >> k.word_shift) + 1u; }

// the rule: both pieces uniform in the same id (an outside piece = kAirClass)
DEXCT_UCOUNT_FN constexpr bool droppable(uint32_t ea, uint32_t eb) { return ea == eb && (ea & kUniform) != 0u; }

// ---- the per-lane count of dropped slabs: three fields of kFieldBits bits for the ids 1, 2, 3 (air counts nothing).
// A ray has at most kMaxSlabs slabs (nx, ny <= 2047, and a margin of as many again); the lanes of a pair share them out, slab
// s to lane s % lanes_per_pair with at least kMinLanes lanes, so a lane's field stays below 2^kFieldBits over the whole ray.
// The sums over a pair need more: reduce_lo / reduce_mid spread the fields before the lanes are added (16 bits each).
constexpr int kFieldBits = 10;
constexpr uint32_t kFieldMask = (1u << kFieldBits) - 1u;
constexpr int kMaxSlabs = 2 * 2047, kMinLanes = 16;
static_assert((kMaxSlabs + kMinLanes - 1) / kMinLanes <= (int)kFieldMask, "a lane's field holds its share of the longest ray");
static_assert(3 * kFieldBits <= 32, "three fields in one register");
static_assert(kMaxSlabs < (1 << 16), "the sums of a pair fit the 16 bits they are spread to");
// what a dropped slab of class e adds to the lane's register: 1 in the field of its id, nothing for air
DEXCT_UCOUNT_FN constexpr uint32_t bump(uint32_t e) { return (1u << (kFieldBits * (e >> 1))) >> kFieldBits; }
// id 1 in bits 0..15 and id 3 in bits 16..31 / id 2 in bits 0..15: summed over lanes without a carry between the fields
DEXCT_UCOUNT_FN constexpr uint32_t spread_lo(uint32_t packed) { return (packed & kFieldMask) | ((packed >> (2 * kFieldBits)) << 16); }
DEXCT_UCOUNT_FN constexpr uint32_t spread_mid(uint32_t packed) { return (packed >> kFieldBits) & kFieldMask; }

}  // namespace ucount
}  // namespace dexct
