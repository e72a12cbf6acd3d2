/* Additive to ABI 6 of dexct.h (which includes this header; include that one): the Newton decomposition that solves repeated
 * rows once.  dexct_gn_decompose and every other declaration of dexct.h are unchanged. */
#ifndef DEXCT_GN_DEDUP_H
#define DEXCT_GN_DEDUP_H

#include "dexct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dexct_gn_decompose that solves repeated rows once.  Additive to ABI 6; dexct_gn_decompose is unchanged.  The result of the
 * float64 shared-spectrum kernels is a pure function of a pixel's two counts and the mask threshold, and in a scan of an extruded
 * phantom most rows of a (view, channel) pair - a LINE: options->out_rows consecutive values of the [..][channel][row] input -
 * carry bitwise the counts of the row before.  The call probes every 64th line; where at most 1 / 8 of the sampled pixels differ
 * from the row before it marks those pixels of the whole input (one bit per pixel), copies them to a list of at most
 * cap = n_pix / 8 (in whole 64-pixel tiles) entries, runs the pass's unchanged Newton kernel on the list and writes every pixel's
 * result from the list's: out_a is byte for byte that of dexct_gn_decompose.  If the sample has fewer repeats, or the list would
 * overflow, the usual launch runs instead.  All of it is decided on the device (nothing is read back, allocated or synchronised):
 * both Newton launches are always enqueued, and one of them finds its tile queue used up.
 *   The route exists for precision == 0, n_bins == 1, pass 0 or DEXCT_GN_PASS_SHORTCUT, the lane-per-pixel kernels (not the
 *   cooperative one), options->out_rows / out_channels set, n_pix < 2^31 and cap >= 64; any other call - and every call with
 *   dedup_workspace == NULL or DEXCT_GN_DEDUP=0 in the environment (read once, with the variables above) - is exactly
 *   dexct_gn_decompose.  An input without repeats pays the probe and the empty launches (profiles/gn_dedup.md).
 *   dedup_workspace  device scratch of dexct_gn_dedup_workspace_bytes(n_pix, out_rows, g_is_f64) bytes, 16-byte aligned
 *                    (DEXCT_EINVAL otherwise): 64 bytes of descriptor,
 *                    8 bytes per 64 rows of a line, 8 bytes per line, cap x (4 or 8, twice) bytes of list and cap x 16 bytes of
 *                    results, each array rounded up to 256 bytes - n_pix x (1/8 + 3 or 4) bytes + 8 per line for out_rows a
 *                    multiple of 64 (1.3 GB for 4.1e8 float32 pixels in lines of 512).  Its previous contents do not matter.
 *                    After the call its first three uint64 words hold `use` (1: the list was solved and expanded, 0: the usual
 *                    launch ran), F (the distinct pixels counted; 0 if the probe said no) and cap.
 *   The workspace's diagnostic words then describe the launch that worked: DEXCT_GN_WS_EXECUTED counts the steps of the F solved
 *   pixels, DEXCT_GN_WS_PROGRESS ends at n_pix either way. */
#define DEXCT_GN_DEDUP_USE 0           /* byte offsets of the dedup workspace's descriptor words (uint64) */
#define DEXCT_GN_DEDUP_FRESH 8
#define DEXCT_GN_DEDUP_CAP 16
int64_t dexct_gn_dedup_workspace_bytes(int64_t n_pix, int32_t rows, int32_t g_is_f64);
int dexct_gn_decompose_dedup(const void* g1, const void* g2, int32_t g_is_f64, int64_t n_pix, const double* i0,
                             const double* mus, int32_t n_energies, int32_t n_bins, int32_t bin_div, int32_t n_iters,
                             int32_t precision, int32_t n_polish, const double* mask_max, double mask_frac, double* out_a,
                             const dexct_gn_options* options, void* workspace, void* dedup_workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXCT_GN_DEDUP_H */
