// dexct_gn_decompose_dedup: the passes around the Newton launches (gn_dedup.hip), as dexct_gn_decompose's host code calls them.
// Everything is decided on the device and passed on through the descriptor at the start of the dedup workspace
// (gn_dedup_index.h); no call allocates, synchronises or reads anything back.  All return DEXCT_OK or DEXCT_EHIP.
#pragma once
#include "common.h"
#include "gn_dedup_index.h"

namespace dexct {

struct GnDedupCall {             // what every pass needs to know of the call
  void* workspace;               // dexct_gn_dedup_workspace_bytes(n_pix, rows, g_is_f64) bytes
  int64_t n_pix;
  int rows, channels;            // the sinograms are [n_pix / (rows channels)][channels][rows]
  int g_is_f64;
  gn_dedup::Layout at() const { return gn_dedup::layout(n_pix, rows, g_is_f64 ? 8 : 4); }
  template <typename T> T* array(int64_t offset) const { return reinterpret_cast<T*>(reinterpret_cast<char*>(workspace) + offset); }
};

// probe, census, scan, gather: leaves the descriptor (use, F, cap) and, with use = 1, the list, the bit rows and the bases
int gn_dedup_prepare(const GnDedupCall& dc, const void* g1, const void* g2, hipStream_t st);
// the word kWsQueueHead (`head`) before the launch on the list / before the direct launch on direct_tiles tiles; the latter
// also takes the list launch's pixels out of the progress word, which the expansion then counts up to n_pix
int gn_dedup_list_head(const GnDedupCall& dc, unsigned long long* head, hipStream_t st);
int gn_dedup_direct_head(const GnDedupCall& dc, unsigned long long* head, unsigned long long* progress, int64_t direct_tiles, hipStream_t st);
// with use = 1: every pixel's result from the list's, in [..][row][channel] order
int gn_dedup_expand(const GnDedupCall& dc, double* out_a, unsigned long long* progress, hipStream_t st);

}  // namespace dexct
