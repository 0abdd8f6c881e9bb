// Payload facets (hx_payload_facet / hx_facet_top): how many kept rows hold each code of a U32 or
// LIST_U32 payload column, and the codes with the largest counts.
//
//   k_facet_count_u32   one row per lane, FACET_U row groups per wave and pass (the mask kernel's shape); the lane loads
//                       its cell and its mask bit.
//   k_facet_count_list  the walk of section 17: a wave's FACET_LR rows own one contiguous element run [S, E), the wave
//                       walks it 64 elements at a time, lane j owns element base + j.  The lane finds its element's row by
//                       a binary search over the rows' offsets (relative to S, staged in LDS once per pass), reads the
//                       row's mask bit, and counts the element unless an EARLIER element of the same row equals it: it
//                       scans backward from its element to the row's start and stops at the first equal one (the wave keeps
//                       its last two chunks of codes in LDS: only a row longer than that is read from global memory).  A row of k elements costs at most k (k - 1) / 2
//                       comparisons -- k distinct values; a row of k elements with d distinct values about k d.
//   both                before any atomic the wave aggregates runs: a lane compares its code with that of the nearest lane
//                       below it that counts anything, the heads of runs are balloted, and each head adds its run's
//                       length (the counting lanes up to the next head, bit operations on the two ballots).  Two tiers
//                       by n_codes: up to HX_FACET_LDS_CODES a histogram per workgroup in LDS (LDS integer atomics; one
//                       global atomic per non-zero counter at the end), above it global atomics straight into counts.
//                       Integer sums: the result does not depend on order.
//   k_facet_keys        the top stage's first pass: a workgroup takes FACET_SLICE codes, builds the keys count << 32 |
//                       (0xFFFFFFFF - rank) of its non-zero counters and -- limit <= 512 -- keeps its best `limit` with
//                       the register sort and fold of wsort.hpp; above, it writes all of them.  launch_compact merges the
//                       slices' lists, 8192 keys at a time, until one is left.
#include "../../include/hx.h"
#include "hx_common.hpp"
#include "kernels.hpp"
#include "wsort.hpp"

#include <algorithm>

namespace hx {

constexpr int FACET_U = 4;                  // row groups (of 64 rows) per wave and pass of the scalar kernel
constexpr int FACET_LR = 256;               // rows per wave and pass of the list kernel
constexpr uint32_t FACET_NONE = 0xFFFFFFFFu;   // a lane with nothing to count (HX_PAY_U32_MISSING: never a code)
constexpr unsigned FACET_GRID_LDS = 512;    // two workgroups per CU: what 64 KB of histogram leave room for
constexpr unsigned FACET_GRID_GLOBAL = 2048;

// One add per run of equal keys among the wave's 64; every lane must call it.  Lanes with nothing to count are
// transparent: a lane's neighbour is the nearest LIVE lane below it, so the rows a mask drops do not cut a run of 50
// equal document ids into 25 runs of one.  A run's head adds the live lanes from itself to the next head.
template <bool LDS>
__device__ __forceinline__ void facet_add(uint32_t key, int lane, uint32_t* hist, uint32_t* __restrict__ counts) {
  const unsigned long long lives = __ballot(key != FACET_NONE);
  const unsigned long long lower = (1ull << lane) - 1ull;                // lanes [0, lane)
  const unsigned long long below = lives & lower;
  const int p = below ? 63 - __clzll((long long)below) : lane;           // the nearest live lane below (else: itself)
  const uint32_t prev = (uint32_t)__shfl((int)key, p, 64);
  const bool head = key != FACET_NONE && (!below || prev != key);
  const unsigned long long heads = __ballot(head);
  if (head) {
    const unsigned long long above = (heads >> lane) >> 1;               // the heads of the lanes after this one
    const int next = above ? lane + __ffsll(above) : 64;                 // the next head's lane
    const unsigned long long upto = next >= 64 ? ~0ull : (1ull << next) - 1ull;
    const uint32_t len = (uint32_t)__popcll(lives & upto & ~lower);      // live lanes in [lane, next)
    if (LDS) atomicAdd(&hist[key], len);
    else atomicAdd(&counts[key], len);
  }
}

// what one wave wrote to LDS is visible to its other lanes (the waves of a workgroup walk runs of different lengths: no
// workgroup barrier inside the walk)
__device__ __forceinline__ void facet_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool LDS, int NT>
__device__ __forceinline__ void facet_finish(const FacetArgs& a, uint32_t* hist, uint32_t stray, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) stray += (uint32_t)__shfl_down((int)stray, off, 64);
  if (lane == 0 && stray) atomicAdd(a.stray, (unsigned long long)stray);
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_codes; i += NT) {
      const uint32_t v = hist[i];
      if (v) atomicAdd(&a.counts[i], v);
    }
  }
}

template <bool LDS, int NT>
__global__ void __launch_bounds__(NT) k_facet_count_u32(FacetArgs a) {
  __shared__ uint32_t hist[LDS ? HX_FACET_LDS_CODES : 1];
  const int lane = threadIdx.x & (WAVE - 1);
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < a.n_codes; i += NT) hist[i] = 0u;
    __syncthreads();
  }
  const int64_t wave = (int64_t)blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (NT / WAVE);
  uint32_t stray = 0;
  for (int64_t g0 = wave * FACET_U; g0 * WAVE < a.n; g0 += n_waves * FACET_U) {
    uint32_t key[FACET_U];
#pragma unroll
    for (int u = 0; u < FACET_U; ++u) {
      const int64_t row = (g0 + u) * WAVE + lane;
      const bool in = row < a.n;
      const uint32_t cell = in ? a.p0[row] : FACET_NONE;
      const uint32_t word = (a.mask && in) ? a.mask[row >> 5] : 0xFFFFFFFFu;
      const bool live = in && ((word >> (row & 31)) & 1u) && cell < HX_PAY_U32_NULL;
      stray += (live && cell >= a.n_codes) ? 1u : 0u;
      key[u] = (live && cell < a.n_codes) ? cell : FACET_NONE;
    }
#pragma unroll
    for (int u = 0; u < FACET_U; ++u) facet_add<LDS>(key[u], lane, hist, a.counts);
  }
  facet_finish<LDS, NT>(a, hist, stray, lane);
}

template <bool LDS, int NT>
__global__ void __launch_bounds__(NT) k_facet_count_list(FacetArgs a) {
  __shared__ uint32_t hist[LDS ? HX_FACET_LDS_CODES : 1];
  __shared__ uint32_t s_off[NT / WAVE][FACET_LR + 1];   // a wave's offsets relative to S; past its rows 0xFFFFFFFF
  __shared__ uint32_t s_el[NT / WAVE][2 * WAVE];        // a wave's last two chunks of codes, the current one in [64, 128)
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (LDS)
    for (uint32_t i = threadIdx.x; i < a.n_codes; i += NT) hist[i] = 0u;
  const int64_t blk_rows = (int64_t)(NT / WAVE) * FACET_LR;
  uint32_t stray = 0;
  // (the trip count is the workgroup's: the barriers below are met by every wave, one without rows walks nothing)
  for (int64_t blk = blockIdx.x; blk * blk_rows < a.n; blk += gridDim.x) {
    const int64_t r0 = blk * blk_rows + (int64_t)w * FACET_LR;
    const int64_t r1 = std::min<int64_t>(r0 + FACET_LR, a.n);        // (below r0 for a wave without rows)
    const int64_t S = r0 < a.n ? a.off[r0] : 0, E = r0 < a.n ? a.off[r1] : 0;
    __syncthreads();                   // the previous pass has read s_off (first pass: hist is zeroed)
    for (int i = lane; i <= FACET_LR; i += WAVE)
      s_off[w][i] = r0 + i <= r1 ? (uint32_t)(a.off[r0 + i] - S) : 0xFFFFFFFFu;
    __syncthreads();
    uint32_t code_before = FACET_NONE;   // the lane's code of the previous chunk
    for (int64_t base = S; base < E; base += WAVE) {
      const int64_t e = base + lane;
      const bool ok = e < E;
      const uint32_t code = ok ? a.e0[e] : FACET_NONE;
      // the backward scan below reads the 64 + lane codes before its own out of LDS (a chain of dependent reads: from
      // global memory it was the whole kernel's time), the rest of a longer row from global memory
      facet_wave_sync();                 // the previous chunk's scans are done
      s_el[w][lane] = code_before;
      s_el[w][WAVE + lane] = code;
      code_before = code;
      facet_wave_sync();
      bool count = false;
      if (ok) {
        // the element's row: the last row of the wave whose offset is <= the element's (empty rows share an offset
        // with their successor and are passed over); entry r1 - r0 is E - S, above every element
        const uint32_t rel = (uint32_t)(e - S);
        int lo = 0;
#pragma unroll
        for (int step = FACET_LR / 2; step > 0; step >>= 1)
          if (s_off[w][lo + step] <= rel) lo += step;
        const int64_t row = r0 + lo;
        const bool kept = !a.mask || ((a.mask[row >> 5] >> (row & 31)) & 1u);
        stray += (kept && code >= a.n_codes) ? 1u : 0u;
        count = kept && code < a.n_codes;
        if (count) {
          const int64_t back = e - (S + s_off[w][lo]);               // the row's elements before this one
          for (int64_t d = 1; d <= back; ++d) {
            const uint32_t x = d <= WAVE + lane ? s_el[w][WAVE + lane - (int)d] : a.e0[e - d];
            if (x == code) {
              count = false;
              break;
            }
          }
        }
      }
      facet_add<LDS>(count ? code : FACET_NONE, lane, hist, a.counts);
    }
  }
  facet_finish<LDS, NT>(a, hist, stray, lane);
}

void launch_facet_count(const FacetArgs& a, int grid_cap, hipStream_t st) {
  if (a.n <= 0) return;
  const bool lds = a.n_codes <= (uint32_t)HX_FACET_LDS_CODES;
  auto grid_of = [&](int64_t rows_per_wg) {
    unsigned g = (unsigned)std::min<int64_t>((a.n + rows_per_wg - 1) / rows_per_wg, lds ? FACET_GRID_LDS : FACET_GRID_GLOBAL);
    return grid_cap > 0 ? std::min(g, (unsigned)grid_cap) : g;
  };
  if (a.off) {
    if (lds) hipLaunchKernelGGL((k_facet_count_list<true, 512>), dim3(grid_of(8 * FACET_LR)), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((k_facet_count_list<false, 256>), dim3(grid_of(4 * FACET_LR)), dim3(256), 0, st, a);
  } else {
    if (lds) hipLaunchKernelGGL((k_facet_count_u32<true, 1024>), dim3(grid_of(1024 * FACET_U)), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL((k_facet_count_u32<false, 256>), dim3(grid_of(256 * FACET_U)), dim3(256), 0, st, a);
  }
  HX_HIP(hipGetLastError());
}

// ---- the top stage's first pass ------------------------------------------------------------------------------------------
template <bool FOLD>
__global__ void __launch_bounds__(256) k_facet_keys(const uint32_t* __restrict__ counts, uint32_t n_codes,
                                                    const uint32_t* __restrict__ rank, uint64_t* __restrict__ lists,
                                                    int list_len) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t c0 = (int64_t)blockIdx.x * FACET_SLICE;
  auto key_of = [&](int i) -> uint64_t {
    const int64_t c = c0 + i;
    if (c >= (int64_t)n_codes) return 0ull;
    const uint32_t v = counts[c];
    if (!v) return 0ull;
    const uint32_t r = rank ? rank[c] : (uint32_t)c;
    return ((uint64_t)v << 32) | (uint64_t)(0xFFFFFFFFu - r);
  };
  uint64_t* o = lists + (int64_t)blockIdx.x * list_len;
  if constexpr (!FOLD) {               // list_len = FACET_SLICE: the merge sorts
    for (int i = tid; i < FACET_SLICE; i += 256) o[i] = key_of(i);
  } else {                             // list_len <= 512: wave 0 ends with the slice's best 512, sorted
    uint64_t v[8];
    compact_top_core<4, 8>(key_of, FACET_SLICE, v, lane, w);
    if (w == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = lane * 8 + e;
        if (i < list_len) o[i] = v[e];
      }
    }
  }
}

void launch_facet_keys(const uint32_t* counts, uint32_t n_codes, const uint32_t* rank, uint64_t* lists, int list_len,
                       hipStream_t st) {
  const unsigned grid = (unsigned)(((int64_t)n_codes + FACET_SLICE - 1) / FACET_SLICE);
  if (list_len == FACET_SLICE) hipLaunchKernelGGL(k_facet_keys<false>, dim3(grid), dim3(256), 0, st, counts, n_codes, rank, lists, list_len);
  else hipLaunchKernelGGL(k_facet_keys<true>, dim3(grid), dim3(256), 0, st, counts, n_codes, rank, lists, list_len);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
