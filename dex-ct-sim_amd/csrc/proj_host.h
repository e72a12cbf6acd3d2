// The host half the seven projection entry points share (siddon.hip, siddon_packed.hip, siddon_cone.hip, detect.hip): the
// argument predicates, the noise / log rule, the fill of ProjArgs, the tuning knobs, the dispatch on the material count and
// the arithmetic of the material groups (internal, host only: nothing here is device code).
#pragma once
#include <climits>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "proj_pure.h"
#include "siddon_detect.h"

namespace dexct {
namespace proj {

// ---- argument predicates (true = acceptable).  Each entry point strings them together in its own order: the order decides
// which code a call with several faults gets (tests/test_projection_args.py pins it).
inline bool views_ok(const dexct_fan_geom& g, int view_begin, int view_end) {
  return view_begin >= 0 && view_end <= g.n_views && view_end > view_begin;
}
// the stack of detector rows lies inside the volume ...
inline bool stack_ok(const dexct_fan_geom& g) { return g.z_first >= 0 && g.z_first + g.n_rows <= g.nz; }
// ... and starts and ends on whole groups of k slices (4: a dword of the z-fastest layout, 16: a dword of the packed one)
inline bool stack_aligned(const dexct_fan_geom& g, int k) { return g.nz % k == 0 && g.z_first % k == 0; }
inline bool layout_ok(int layout) { return layout == 0 || layout == 1; }
// rows and local views travel as 16-bit halves (grid dimensions, packed block ids)
inline bool fits_16bit(const dexct_fan_geom& g, int view_begin, int view_end) {
  return g.n_rows <= 65535 && view_end - view_begin <= 65535;
}
// 32-bit voxel offsets: the bytes of a layout with z_per_byte slices per byte stay at or below the caller's bound
inline bool offsets_fit(const dexct_fan_geom& g, int z_per_byte = 1, uint64_t bound = 0xFFFFFFFEull) {
  return (uint64_t)g.nx * g.ny * (g.nz / z_per_byte) <= bound;
}
// Cone beam: at most one z-plane per dominant-axis slab, |dz/du| <= 1 for every ray.  du/ds >= 1/(sqrt(2) max(dx, dy))
// along the dominant axis, dz/ds <= max|z_det - z_src| / SDD (max_abs_dz is supplied by the caller, who owns row_z on the
// device).
inline bool cone_slope_ok(const dexct_fan_geom& g, double max_abs_dz) {
  const double dmax = g.dx > g.dy ? g.dx : g.dy;
  return max_abs_dz >= 0 && !(max_abs_dz / g.sdd / g.dz * dmax * 1.4142135623730951 > 1.0);
}
// a one-dimensional grid of nblk workgroups; false beyond the 31 bits a grid dimension has
inline bool grid_1d(size_t nblk, dim3& grid) {
  if (nblk > 0x7FFFFFFFull) return false;
  grid = dim3((unsigned)nblk);
  return true;
}

// ---- quantum noise and the log sinogram: the one rule of every entry point.
// weights2 switches the variance on; it then needs somewhere to go - the optional `variance` output, the sample the kernel
// draws itself (noise->sample), or both.  What the caller's detection can do with it:
enum class NoiseBy {
  kOwnLoop,    // a variance loop of its own, or the cone kernels' fused one: every spectrum count
  kTwoSlots,   // rows16_kernel: the fused variance runs in the two-slot detection - at most 2 spectra whenever noisy
  kGroupPass,  // detect_kernel after the material groups: the SAMPLE needs the fused variance (two spectrum slots, register
               // lengths: 2..48 materials; a single material goes to detect_kernel_chunked, which draws no sample - only
               // dexct_cone_project_grouped admits one material at all)
};
// log_out of the C ABI (null, or a null sino_log: no log sinogram).  The log of a noisy sinogram is the log of the SAMPLED
// counts: a launch that leaves the variance to dexct_add_noise writes counts that are not the final ones, and its caller
// then uses dexct_sino_log - so a log with weights2 needs the sample.
struct NoiseLog {
  // the verdicts of the two rules, apart because dexct_siddon_project and dexct_siddon_project_packed test other things
  // between them; everyone else returns status()
  int noise_rc = DEXCT_OK, log_rc = DEXCT_OK;
  int sample = 0;
  uint32_t seed_lo = 0, seed_hi = 0;
  float* sino_log = nullptr;
  float air[DEXCT_MAX_SPECTRA] = {1.0f, 1.0f, 1.0f, 1.0f};
  int status() const { return noise_rc != DEXCT_OK ? noise_rc : log_rc; }
};
static_assert(DEXCT_MAX_SPECTRA == 4, "NoiseLog::air lists its defaults");

inline NoiseLog noise_log_args(const float* weights2, const float* variance, const dexct_noise* noise, const dexct_log_out* log_out,
                               int n_spectra, int n_materials, NoiseBy by) {
  NoiseLog r;
  const bool noisy = weights2 != nullptr, sample = noise && noise->sample;
  if (noisy ? (!variance && !sample) : (variance || sample)) r.noise_rc = DEXCT_EINVAL;
  else if (noisy && by == NoiseBy::kTwoSlots && n_spectra > 2) r.noise_rc = DEXCT_ERANGE;
  else if (sample && by == NoiseBy::kGroupPass && (n_spectra > 2 || n_materials > kManyMaterials || n_materials < 2))
    r.noise_rc = DEXCT_ERANGE;
  else if (sample) {
    r.sample = 1;
    r.seed_lo = (uint32_t)noise->seed;
    r.seed_hi = (uint32_t)(noise->seed >> 32);
  }
  if (log_out && log_out->sino_log) {
    if (noisy && !sample) r.log_rc = DEXCT_EINVAL;
    else {
      r.sino_log = log_out->sino_log;
      for (int s = 0; s < DEXCT_MAX_SPECTRA; ++s) r.air[s] = log_out->air[s];
    }
  }
  return r;
}

// NoiseLog -> a launch struct (ProjArgs, PackedArgs, ConeArgs name these fields alike).  The Philox counter needs the GLOBAL
// view of a ray, hence view_begin.
template <class Args>
void copy_noise(Args& a, int view_begin, const NoiseLog& nl) {
  a.view_begin = view_begin;
  a.sample = nl.sample;
  a.seed_lo = nl.seed_lo;
  a.seed_hi = nl.seed_hi;
}
template <class Args>
void copy_log(Args& a, const NoiseLog& nl) {
  a.sino_log = nl.sino_log;
  for (int s = 0; s < DEXCT_MAX_SPECTRA; ++s) a.air[s] = nl.air[s];
}

// What every ProjArgs holds; the rest is value-initialised, and the entry point sets what is its own: the volumes, acc_out,
// mat_base, acc_lengths, view_tile, and with copy_noise the sample of a detection that draws one.
inline ProjArgs fill_proj_args(const dexct_fan_geom& g, const dexct_ray_plan* plan, int view_begin, int view_end, int n_materials,
                               int n_energies, int n_spectra, float* counts, float* pathlen, float* variance, int layout,
                               const NoiseLog& nl) {
  ProjArgs a{};
  a.g = g;
  a.plan = plan;
  a.n_local_views = view_end - view_begin;
  a.n_materials = n_materials;
  a.n_energies = n_energies;
  a.n_spectra = n_spectra;
  a.counts = counts;
  a.pathlen = pathlen;
  a.variance = variance;
  a.layout = layout;
  copy_log(a, nl);
  return a;
}

// ---- tuning knobs: integers from the environment, read on EVERY call (include/dexct.h promises that a change takes effect
// with the next call).  A value outside lo..hi - and text atoi reads as such a value - counts as not set.
struct Knob {
  const char* name;
  int def, lo, hi;
};
inline int read_knob(const Knob& k) {
  const char* e = getenv(k.name);
  if (!e) return k.def;
  const int v = atoi(e);
  return v < k.lo || v > k.hi ? k.def : v;
}

namespace knob {
// views per locality tile of the row-parallel kernels; one name, two defaults: rows16_kernel has 16 (8 until round 5, 16
// measured 2 - 4 % faster on every stacked-fan configuration, tools/probes/p16_knobs.py)
constexpr Knob kViewTile{"DEXCT_VIEW_TILE", 8, 1, 4096};
constexpr Knob kViewTileP16{"DEXCT_VIEW_TILE", 16, 1, 4096};
// rays_kernel with register accumulators: slabs per batch with all their loads in flight, 4 / 8 / 16; anything else = the
// form of 256 lanes without batches (measured on the reference's 1000 x 800 single-row scan: 0.620 / 0.440 / 0.450 /
// 0.457 ms for 1 / 4 / 8 / 16, profiles/r03_kernels.md)
constexpr Knob kRaysBatch{"DEXCT_RAYS_BATCH", 4, INT_MIN, INT_MAX};
// rows16_kernel: skip detection FMAs of spectrum slots with zero weights (blocks of four energies); 0 = off
constexpr Knob kDetMasks{"DEXCT_DET_MASKS", 1, INT_MIN, INT_MAX};
// rows16_kernel, 3 and 4 materials: a wave whose rays all miss the last material runs the detection of one material less; 0 = off
constexpr Knob kDetAbsent{"DEXCT_DET_ABSENT", 1, INT_MIN, INT_MAX};
// rows16_kernel, staged noise-free forms: a wave detects each distinct quad of rows once where that saves a round; 0 = off,
// 2 = every list round detects four rows per lane (no narrow last round: the A/B of dedup_index.h's round_rows)
constexpr Knob kDetDedup{"DEXCT_DET_DEDUP", 1, INT_MIN, INT_MAX};
// rows16_kernel: store the results of a wave through LDS as whole lines; 0 = per-round 16-B stores
constexpr Knob kP16Staged{"DEXCT_P16_STAGED", 1, INT_MIN, INT_MAX};
// rows16_kernel, three materials: waves per SIMD the register allocation must allow; acts on 5 / 6 / 8
constexpr Knob kP16MinW{"DEXCT_P16_MINW", 4, INT_MIN, INT_MAX};
// rows16_kernel, the air-column map of dexct_siddon_project_packed_skip: 0 = never used, 1 = used when use_air_map
// (proj_pure.h) says it pays, 2 = used whenever the caller passes one
constexpr Knob kP16AirSkip{"DEXCT_P16_AIR_SKIP", 1, 0, 2};
// rows16_kernel, the column-class map of dexct_siddon_project_packed_uniform: 0 = never used (the air map serves alone: the A/B
// against the air rule), 1 = used when use_class_map (proj_pure.h) says it pays, 2 = used whenever the caller passes one;
// DEXCT_P16_AIR_SKIP = 0 turns it off with the air map
constexpr Knob kP16Uniform{"DEXCT_P16_UNIFORM", 1, 0, 2};
// rows16_kernel, the tile map of dexct_siddon_project_packed_tiles: 0 = never used (the class map serves alone: the A/B against
// the slab rule), 1 = used when use_tile_map (proj_pure.h) says it pays, 2 = used whenever the caller passes one and the class
// map is in use
constexpr Knob kP16Tiles{"DEXCT_P16_TILES", 1, 0, 2};
// cone row kernels, views per tile of the block order: 1 = all channels of a view before the next view (round 3: 9.6 ->
// 9.2 ms on a 100-view scan, whose views 3.6 degrees apart share no columns; no difference at 0.36 degrees)
constexpr Knob kConeViewTile{"DEXCT_CONE_VIEW_TILE", 1, 1, INT_MAX};
// round 3: columns staged in LDS (cone_cols_kernel) whenever a column fits the reserved bytes; 0 = cone_rows_kernel, for A/B
constexpr Knob kConeCols{"DEXCT_CONE_COLS", 1, INT_MIN, INT_MAX};
// cone_cols_kernel, slabs per staged batch: 4 (default: 64 VGPRs and 17 KB of LDS = 8 waves per SIMD; 9.6 ms) or 8 (92
// VGPRs, 26 KB: 5 waves; 10.4 ms) - the loop waits for the staged loads of the next batch, so waves in flight are what counts
constexpr Knob kConeKb{"DEXCT_CONE_KB", 4, INT_MIN, INT_MAX};
// cone_rows_kernel, three materials: slabs per batch; acts on 2 / 8
constexpr Knob kConeBatch{"DEXCT_CONE_BATCH", 4, INT_MIN, INT_MAX};
// cone_rows_kernel, three materials: 0 = corrections in registers (the round-2 form), for A/B
constexpr Knob kConeLdsc{"DEXCT_CONE_LDSC", 1, INT_MIN, INT_MAX};
}  // namespace knob

// ---- dispatch on the material count, in the style of gnpix::for_shape: launch(std::integral_constant<int, N>{}) for the first N
// of the list that equals n.  A 0 in the list takes every n (put it last: the kernels' NM = 0 is their any-count form); without
// one, a count that is not listed is DEXCT_EINVAL.
template <int... NS, class Launch>
int for_materials(int n, Launch launch) {
  int rc = DEXCT_EINVAL;
  // (a LEFT fold: the compiler then instantiates the launches, and with them the kernels, in the order of the list)
  (void)(... || ((NS == 0 || n == NS) ? (rc = launch(std::integral_constant<int, NS>{}), true) : false));
  return rc;
}
// the counts FIRST .. FIRST + sizeof...(I) - 1
template <int FIRST, int... I, class Launch>
int for_materials_from(int n, std::integer_sequence<int, I...>, Launch launch) {
  return for_materials<(FIRST + I)...>(n, launch);
}

// ---- material groups: a pass of the row kernels takes three materials.  The stacked fan takes material 0 from the chord
// (chord0), so its groups cover materials 1 .. M-1; the cone-beam groups cover all M.
inline int n_groups(int n_materials, bool chord0) { return (n_materials - (chord0 ? 1 : 0) + 2) / 3; }
// materials in group g: 1..3
inline int group_size(int n_materials, bool chord0, int g) {
  const int left = n_materials - (chord0 ? 1 : 0) - 3 * g;
  return left >= 3 ? 3 : left;
}

}  // namespace proj
}  // namespace dexct
