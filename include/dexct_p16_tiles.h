/* Additive to ABI 6 of dexct.h (which includes this header; include that one): the tile map of a column-class map and the packed
 * projection that dismisses runs of slabs in uniform tiles before it classifies them one by one.  dexct_volume_column_classes,
 * dexct_siddon_project_packed_uniform and every other declaration of dexct.h and dexct_p16_uniform.h are unchanged. */
#ifndef DEXCT_P16_TILES_H
#define DEXCT_P16_TILES_H

#include "dexct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A tile is DEXCT_TILE_SIDE x DEXCT_TILE_SIDE columns of a packed volume: tile (tx, ty) holds the columns x = 8 tx .. 8 tx + 7,
 * y = 8 ty .. 8 ty + 7.  Its class is four bits with the codes of DEXCT_COL_CLASS: DEXCT_COL_CLASS(id) when all 64 columns are
 * uniform in id, else 0 (mixed); a tile that reaches past nx or ny is uniform only in air (all its columns inside the grid are
 * air), else mixed.  The map holds two copies, eight tiles per word (csrc/tile_class.h has the layout in code):
 *   copy 0, for rays whose slabs run along x: for tx = 0 .. TX - 1 a row of TY + 2 nibbles - an air tile, the tiles ty = 0 .. TY - 1,
 *           an air tile; nibble tx (TY + 2) + ty + 1;
 *   copy 1, for slabs along y, from the next whole word on: for ty = 0 .. TY - 1 a row of TX + 2 nibbles in the same manner;
 *   one spare word.  TX = ceil(nx / 8), TY = ceil(ny / 8).
 * The at most three tiles a run of eight slabs touches are consecutive nibbles of one row.
 *
 * dexct_volume_tile_map_words: the words of the map of an nx x ny grid (0: impossible sizes).
 * dexct_volume_tile_classes: builds tile_map[dexct_volume_tile_map_words(nx, ny)] (device memory) from the column-class map of
 *   dexct_volume_column_classes; n_uniform[4] (device memory) receives the number of tiles uniform in id 0 .. 3.  Once per
 *   volume, next to the class map.
 * dexct_siddon_project_packed_tiles: dexct_siddon_project_packed_uniform with that map as well (tile_map, and the counts the
 *   builder gave, n_uniform_tiles[4]: HOST memory).  Where the class map is used by a kernel with whole-line stores (row-fastest
 *   layout, n_rows a multiple of 4, at most two spectra), a run - the up to eight slabs of a ray inside one row of tiles - whose
 *   tiles are all uniform in the same id (a tile outside the grid is air) is counted for that id at once; the slabs of every other
 *   run are classified as before, in their order.  EVERY output keeps its bits.
 *   DEXCT_P16_TILES (read on every call) = 1 (default) uses the tile map from one uniform tile in two on (and only for grids up
 *   to 512 x 512: a ray of the kernel has at most 64 runs), 2 whenever one is passed, 0 never; where it is not used the call is dexct_siddon_project_packed_uniform.  tile_map null = that call.  A count
 *   outside 0 .. TX*TY, or counts that sum to more, is DEXCT_EINVAL. */
#define DEXCT_TILE_SIDE 8

int64_t dexct_volume_tile_map_words(int32_t nx, int32_t ny);
int dexct_volume_tile_classes(const uint32_t* col_class, int32_t nx, int32_t ny, uint32_t* tile_map, uint64_t* n_uniform, void* stream);
int dexct_siddon_project_packed_tiles(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                      int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                      int32_t n_spectra, const float* mu, const float* weights, float* counts,
                                      float* pathlen, int32_t layout, const dexct_log_out* log_out, const float* weights2,
                                      float* variance, const dexct_noise* noise, const uint32_t* col_air,
                                      int64_t n_air_columns, const uint32_t* col_class, const int64_t* n_uniform_columns,
                                      const uint32_t* tile_map, const int64_t* n_uniform_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXCT_P16_TILES_H */
