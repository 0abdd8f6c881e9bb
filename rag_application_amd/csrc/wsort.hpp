// In-register bitonic sorting network of one wave: 64 E 64-bit keys, E per lane (E = 4: 256 keys, E = 8: 512),
// index i = lane * E + e, descending.  Strides below E are register swaps, the rest lane exchanges (no LDS traffic
// of its own, no barrier).  Used by k_compact_top (select.hip) and the candidate cut of k_sparse_select
// (sparse2.hip).  E is deduced from the register array.  compact_top_core folds the sorted runs of a block's waves into
// its best 64 E keys: k_compact_top and k_dense_finish (select.hip) and the top stage of a facet (facet.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hx {

__device__ __forceinline__ uint64_t k64max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t k64min(uint64_t a, uint64_t b) { return a > b ? b : a; }
// compare-exchange stage (k, j) of the descending bitonic network over i = lane * E + e
template <int K, int J, int E>
__device__ __forceinline__ void w_cx(uint64_t (&v)[E], int lane) {
  if constexpr (J < E) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if ((e & J) == 0) {
        const bool desc = K < E ? ((e & K) == 0) : (((lane * E) & K) == 0);
        const uint64_t mx = k64max(v[e], v[e ^ J]), mn = k64min(v[e], v[e ^ J]);
        v[e] = desc ? mx : mn;
        v[e ^ J] = desc ? mn : mx;
      }
    }
  } else {
    constexpr int LM = J / E;
    const bool lower = (lane & LM) == 0;
    const bool desc = ((lane * E) & K) == 0;
    const bool take_max = lower == desc;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint64_t y = (uint64_t)__shfl_xor((unsigned long long)v[e], LM, 64);
      v[e] = take_max ? k64max(v[e], y) : k64min(v[e], y);
    }
  }
}
template <int K, int J, int E>
__device__ __forceinline__ void w_merge(uint64_t (&v)[E], int lane) {
  w_cx<K, J>(v, lane);
  if constexpr (J > 1) w_merge<K, J / 2>(v, lane);
}
template <int K, int E>
__device__ __forceinline__ void w_sort(uint64_t (&v)[E], int lane) {
  if constexpr (K > 2) w_sort<K / 2>(v, lane);
  w_merge<K, K / 2>(v, lane);
}

// The fold itself, for a block of exactly NW waves: src[0, n) (n <= NW * 64 E) -> wave 0 holds the best 64 E keys in v,
// sorted (index lane * E + e); returns the number of non-empty keys.  Every thread of the block must call it.
template <int NW, int E, typename LOAD>
__device__ __forceinline__ int compact_top_core(LOAD&& load, int n, uint64_t (&v)[E], int lane, int w) {
  constexpr int R = 64 * E;          // keys per wave
  // a wave hands its run to its partner through slot w / 2: the only earlier reader of that slot is the wave itself
  // (as the partner of wave w + 1 in the first round), so NW / 2 slots serve every round
  __shared__ uint64_t buf[NW > 1 ? (NW / 2) * R : 1];
  __shared__ int s_tot[NW];
  int tot = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {   // the order inside an unsorted run is free: coalesced loads
    const int i = w * R + e * 64 + lane;
    v[e] = i < n ? load(i) : 0ull;
    tot += __popcll(__ballot(v[e] != 0ull));
  }
  if (n > w * R) w_sort<R>(v, lane);
  if (NW > 1) {
    if (lane == 0) s_tot[w] = tot;
#pragma unroll
    for (int s = 0; (1 << s) < NW; ++s) {
      const int m = (2 << s) - 1;
      if ((w & m) == (1 << s)) {
#pragma unroll
        for (int e = 0; e < E; ++e) buf[(w >> 1) * R + lane * E + e] = v[e];
      }
      __syncthreads();   // also: every wave's loads have landed before any store below (in-place use)
      const int pw = w + (1 << s);
      if ((w & m) == 0 && n > pw * R) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = k64max(v[e], buf[(pw >> 1) * R + (R - 1) - (lane * E + e)]);
        w_merge<R, R / 2>(v, lane);
      }
    }
    tot = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) tot += s_tot[x];
  }
  return tot;
}

}  // namespace hx
