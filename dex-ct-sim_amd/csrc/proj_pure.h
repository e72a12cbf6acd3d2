// Decisions of the projection host layer that are pure functions of integers: no HIP, no environment, nothing but <stdint.h>, so
// that a stand-alone host program can run them (tests/air_map_host.cpp, tests/uniform_count_host.cpp, also under the sanitizers).
// proj_host.h includes this.
#pragma once
#include <stdint.h>

namespace dexct {
namespace proj {

// ---- the air-column map of rows16_kernel (dexct_siddon_project_packed_skip): whether a launch looks columns up in it.
// mode: DEXCT_P16_AIR_SKIP (knob::kP16AirSkip) - 0 never, 1 when it pays, 2 whenever there is a map.  The lookup costs every
// slab of every lane a few instructions and gives back the sweeps of the slabs it drops, so in mode 1 the map is used from
// a share of all-air columns on: kAirMapShareNum / kAirMapShareDen of the n_cols columns (profiles/rows16_air_skip.md has the
// two measurements the share comes from: on 512^3 the lookup costs 0.15 ms of 10.3 where no column is air and gains 0.56 ms
// of 9.6 where 49.6 % are, so it breaks even near one column in ten).  Counts outside 0..n_cols never use the map.
constexpr int64_t kAirMapShareNum = 1, kAirMapShareDen = 8;
inline bool use_air_map(int mode, bool have_map, int64_t n_air_columns, int64_t n_cols) {
  if (!have_map || mode == 0 || n_cols <= 0 || n_air_columns < 0 || n_air_columns > n_cols) return false;
  if (mode == 2) return true;
  // the smallest count that reaches the share, ceil(n_cols * num / den), formed without a product of n_cols
  const int64_t first = (n_cols / kAirMapShareDen) * kAirMapShareNum +
                        ((n_cols % kAirMapShareDen) * kAirMapShareNum + kAirMapShareDen - 1) / kAirMapShareDen;
  return n_air_columns >= first;
}

// ---- the column-class map (dexct_siddon_project_packed_uniform): the counts the builder gave, and whether a launch looks
// columns up in the map.  n_uniform[id], id = 0 .. 3: columns that hold id over all z.
// The counts a builder can have given: none negative, together no more than the grid has columns (summed without overflow).
inline bool class_counts_ok(const int64_t* n_uniform, int64_t n_cols) {
  if (!n_uniform || n_cols <= 0) return false;
  int64_t sum = 0;
  for (int id = 0; id < 4; ++id) {
    if (n_uniform[id] < 0 || n_uniform[id] > n_cols - sum) return false;
    sum += n_uniform[id];
  }
  return true;
}
// mode: DEXCT_P16_UNIFORM (knob::kP16Uniform) - 0 never (the air map serves alone, under its own rule), 1 when it pays, 2 whenever
// there is a class map; air_mode: DEXCT_P16_AIR_SKIP, whose 0 turns every map off.  A lookup in the class map costs what one in
// the air map costs and a dropped slab gives back the same sweeps, so mode 1 carries the share of the air map over: the class map
// is used from kAirMapShareNum / kAirMapShareDen DROPPABLE columns on - columns uniform in any id (profiles/rows16_uniform.md
// has the measurement on a volume where nothing but air is droppable).  Impossible counts never use the map.
inline bool use_class_map(int mode, int air_mode, bool have_map, const int64_t* n_uniform, int64_t n_cols) {
  if (!have_map || mode == 0 || air_mode == 0 || !class_counts_ok(n_uniform, n_cols)) return false;
  if (mode == 2) return true;
  const int64_t droppable = n_uniform[0] + n_uniform[1] + n_uniform[2] + n_uniform[3];      // <= n_cols: class_counts_ok
  const int64_t first = (n_cols / kAirMapShareDen) * kAirMapShareNum +
                        ((n_cols % kAirMapShareDen) * kAirMapShareNum + kAirMapShareDen - 1) / kAirMapShareDen;
  return droppable >= first;
}

// ---- the tile map (dexct_siddon_project_packed_tiles): whether a launch that uses the class map also dismisses runs by tiles.
// mode: DEXCT_P16_TILES (knob::kP16Tiles) - 0 never, 1 when it pays, 2 whenever there is a tile map.  n_uniform[id]: tiles uniform
// in id (class_counts_ok against the n_tiles tiles of the grid; impossible counts never use the map).  Measured on 512^3
// (profiles/rows16_tiles.md): with 88 % of the tiles uniform (the benchmark phantom) the tile forms gain 0.52 ms of 3.76; with
// 34 % (random blobs) they LOSE 0.07 ms of 19.5, with none (shuffled slices, class map forced) 0.23 ms of 34.7 - the run trips
// and the dearer fine trips are not paid back; straight lines through neighbouring points break even at 40 % and 49 %.  So
// mode 1 uses the map from kTileMapShareNum / kTileMapShareDen uniform tiles on.
constexpr int64_t kTileMapShareNum = 1, kTileMapShareDen = 2;
inline bool use_tile_map(int mode, bool have_map, const int64_t* n_uniform, int64_t n_tiles) {
  if (!have_map || mode == 0 || !class_counts_ok(n_uniform, n_tiles)) return false;
  if (mode == 2) return true;
  const int64_t uniform = n_uniform[0] + n_uniform[1] + n_uniform[2] + n_uniform[3];      // <= n_tiles: class_counts_ok
  const int64_t first = (n_tiles / kTileMapShareDen) * kTileMapShareNum +
                        ((n_tiles % kTileMapShareDen) * kTileMapShareNum + kTileMapShareDen - 1) / kTileMapShareDen;
  return uniform >= first;
}

}  // namespace proj
}  // namespace dexct
