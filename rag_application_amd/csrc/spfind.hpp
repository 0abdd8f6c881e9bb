// The wave-wide lookup of a term in an inverted-index view's live-term array: shared by k_sparse_prep (sprescore.hip)
// and k_sparse_df (spstats.hip).
#pragma once
#include "hx_common.hpp"

namespace hx {

// live-term index of `term` by one wave in 64-ary steps: ~log64(n_live) dependent loads (`term` is
// wave-uniform); -1 if absent
__device__ __forceinline__ int sp_find_term_wave(const uint32_t* uterms, int n_live, uint32_t term, int lane) {
  int lo = 0, hi = n_live;   // the first index whose term is >= `term` lies in [lo, hi]
  while (hi - lo > 64) {
    const int step = (hi - lo + 63) >> 6;
    const int p = lo + lane * step;
    const bool in = p < hi;
    const uint32_t v = in ? uterms[p] : 0xFFFFFFFFu;
    const int c = __popcll(__ballot(in && v < term));   // ascending list: a prefix of the probes
    if (c == 0) {
      hi = lo + 1;
      break;
    }
    const int nhi = lo + c * step + 1;                  // probe c (if any) is >= term
    lo = lo + (c - 1) * step + 1;                       // probe c - 1 is < term
    hi = nhi < hi ? nhi : hi;
  }
  const int p = lo + lane;
  const bool in = p < hi;
  const uint32_t v = in ? uterms[p] : 0xFFFFFFFFu;
  const unsigned long long eq = __ballot(in && v == term);
  return eq ? lo + (int)__builtin_ctzll(eq) : -1;
}

}  // namespace hx
