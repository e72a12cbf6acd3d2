/* Additive to ABI 6 of dexct.h (which includes this header; include that one): the column-class map of a packed volume and the
 * packed projection that counts slabs in z-uniform columns once per (view, channel) pair.  dexct_volume_air_columns,
 * dexct_siddon_project_packed, dexct_siddon_project_packed_skip and every other declaration of dexct.h are unchanged. */
#ifndef DEXCT_P16_UNIFORM_H
#define DEXCT_P16_UNIFORM_H

#include "dexct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The class of a column (x, y) of a packed volume: four bits, eight columns per word.  Column c = y*nx + x has bits
 * 4 (c % 8) .. 4 (c % 8) + 3 of word c / 8: 0 = mixed, DEXCT_COL_UNIFORM | id << 1 = one id fills all nz/4 bytes of the column
 * (every voxel a detector row can see, whatever z_first and n_rows are).  The nibbles past the last column are 0. */
#define DEXCT_COL_UNIFORM 1u
#define DEXCT_COL_CLASS_BITS 4
#define DEXCT_COL_CLASS(id) (DEXCT_COL_UNIFORM | (uint32_t)(id) << 1)

/* dexct_volume_column_classes: col_class[(nx*ny + 7) / 8] words as above; n_uniform[4] (device memory, like col_class) receives
 *   the number of columns uniform in id 0 .. 3.  nz a multiple of 4; nx*ny < 2^31.  The map belongs to the volume: it is built
 *   once, next to vol_z2.
 * dexct_siddon_project_packed_uniform: dexct_siddon_project_packed_skip with that map as well (col_class, and the counts the
 *   builder gave, n_uniform_columns[4]: HOST memory).  The noise-free kernel then leaves out of its lists
 *     - every full slab in a uniform column,
 *     - every crossing slab whose two pieces lie inside the grid in uniform columns of the SAME id,
 *     - every slab whose pieces inside the grid are all air (the rule of dexct_siddon_project_packed_skip),
 *   and adds the number of left-out slabs of each id, one integer per pair, to the integer count of every row before it becomes
 *   a float.  A slab that touches a mixed column, crosses between columns of different ids or has a piece outside the grid next
 *   to a non-air column stays in its list at its place: the float32 corrections are summed in the order they were, and EVERY
 *   output keeps its bits.
 *   DEXCT_P16_UNIFORM (read on every call) = 1 (default) uses the class map from one droppable column (uniform in any id) in
 *   eight on, 2 whenever one is passed, 0 never.  Where the class map is not used - that knob, a volume with few uniform columns,
 *   the noisy kernels, which keep the air rule - the call is dexct_siddon_project_packed_skip with col_air / n_air_columns
 *   (either may be absent: NULL / 0), under DEXCT_P16_AIR_SKIP as before; DEXCT_P16_AIR_SKIP=0 turns both maps off.
 *   col_class null = dexct_siddon_project_packed_skip.  A count outside 0 .. nx*ny, or counts that sum to more, is DEXCT_EINVAL. */
int dexct_volume_column_classes(const uint8_t* vol_z2, int32_t nx, int32_t ny, int32_t nz, uint32_t* col_class, uint64_t* n_uniform,
                                void* stream);
int dexct_siddon_project_packed_uniform(const dexct_fan_geom* geom, const dexct_ray_plan* plan, int32_t view_begin,
                                        int32_t view_end, const uint8_t* vol_z2, int32_t n_materials, int32_t n_energies,
                                        int32_t n_spectra, const float* mu, const float* weights, float* counts,
                                        float* pathlen, int32_t layout, const dexct_log_out* log_out, const float* weights2,
                                        float* variance, const dexct_noise* noise, const uint32_t* col_air,
                                        int64_t n_air_columns, const uint32_t* col_class, const int64_t* n_uniform_columns,
                                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXCT_P16_UNIFORM_H */
