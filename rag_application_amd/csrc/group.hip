// Grouped search (hx_group): the best n_groups groups of a ranked list, at most group_size hits
// each, the group of a row being its cell in a U32 payload column.  The result is the walk of the list in rank order --
// a row without a cell is skipped, a row joins its group while the group has room, a row opens its group while fewer
// than n_groups are open -- computed in closed form: with r = the row's rank among the eligible rows of its group and g
// = the number of group leaders (r = 0) ranked before its group's leader, a row is kept iff r < group_size and g <
// n_groups, and goes to slot g * group_size + r.
#include "hx_common.hpp"
#include "kernels.hpp"

namespace hx {

constexpr int GROUP_MAX = MAX_LIMIT;             // most keys of a list, and most slots of a result
constexpr uint32_t GROUP_NO_CODE = 0xFFFFFFFFu;  // sort code of a row without a group: behind every real code

// One workgroup per query, NT = 256 (lists of at most 512 keys) or 1024 threads; at most two elements per thread.
//  1. pair[i] = code(row of key i) << 32 | i for the n slots of the list, GROUP_NO_CODE for an empty slot, a row
//     outside [0, n_rows) or a MISSING / NULL cell; padded to P = the next power of two >= n (at least 64);
//  2. bitonic sort, ascending: the rows of a group are adjacent and in rank order, its first row is its leader;
//  3. per sorted element a binary search for the first pair of its code: r = the distance, the leader's rank sits
//     there.  Leaders raise a flag at their rank; an exclusive block scan of the flags numbers the groups;
//  4. kept rows leave their rank in the slot table (which takes the place of the pairs), the table is written out.
template <int NT>
__global__ __launch_bounds__(NT) void k_group_select(GroupArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t pair[GROUP_MAX];   // 16 KB; later the slot table (uint32 ranks + 1)
  __shared__ int lead[GROUP_MAX];                                       // 8 KB: leader flags by rank, then their ordinals
  __shared__ int wsum[NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint64_t* keys = a.keys + (int64_t)b * a.stride;     // as the caller gave them: what the result carries
  const uint64_t* ikeys = a.ikeys + (int64_t)b * a.stride;   // the same slots with internal ids: what names the rows
  int n = a.counts ? a.counts[b] : a.stride;
  n = n < 0 ? 0 : (n < a.stride ? n : a.stride);
  int P = 64;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += NT) {
    uint32_t code = GROUP_NO_CODE;
    if (i < n) {
      const uint64_t k = ikeys[i];
      const uint32_t id = key_id(k), row = id - a.id_base;
      if (k != 0ull && id >= a.id_base && (int64_t)row < a.n_rows) {
        const uint32_t c = a.p0[row];
        if (c < HX_GROUP_NULL) code = c;
      }
    }
    pair[i] = ((uint64_t)code << 32) | (uint32_t)i;
    lead[i] = 0;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t x = pair[i], y = pair[ixj];
          const bool asc = (i & k) == 0;
          if (asc ? (x > y) : (x < y)) {
            pair[i] = y;
            pair[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  // P <= 2 NT: the sorted elements tid and tid + NT
  uint32_t e_code[2], e_rank[2], e_r[2], e_lead[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int j = tid + e * NT;
    e_code[e] = GROUP_NO_CODE;
    e_rank[e] = e_r[e] = e_lead[e] = 0;
    if (j < P) {
      const uint64_t x = pair[j];
      e_code[e] = (uint32_t)(x >> 32);
      e_rank[e] = (uint32_t)x;
      const uint64_t first = x & 0xFFFFFFFF00000000ull;
      int lo = 0, hi = j;                        // the first pair >= first lies in [0, j]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pair[mid] < first) lo = mid + 1; else hi = mid;
      }
      e_r[e] = (uint32_t)(j - lo);
      e_lead[e] = (uint32_t)pair[lo];
      if (e_code[e] != GROUP_NO_CODE && lo == j) lead[e_rank[e]] = 1;
    }
  }
  __syncthreads();
  // exclusive scan of lead[0, P): thread t owns `per` consecutive ranks
  const int per = P >= NT ? P / NT : 1;
  const int base = tid * per;
  int f0 = 0, f1 = 0;
  if (base < P) {
    f0 = lead[base];
    if (per == 2) f1 = lead[base + 1];
  }
  const int c = f0 + f1;
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if ((tid & 63) >= off) incl += v;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  __syncthreads();
  int before = 0, opened = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int v = wsum[w];
    if (w < (tid >> 6)) before += v;
    opened += v;
  }
  if (base < P) {
    lead[base] = before + incl - c;
    if (per == 2) lead[base + 1] = before + incl - c + f0;
  }
  // the pairs are in registers: their place becomes the slot table
  uint32_t* slot = (uint32_t*)pair;
  const int G = a.n_groups, S = a.group_size, GS = G * S;
  __syncthreads();
  for (int i = tid; i < GS; i += NT) slot[i] = 0u;
  __syncthreads();
  uint32_t* gcodes = a.group_codes + (int64_t)b * G;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (e_code[e] != GROUP_NO_CODE && e_r[e] < (uint32_t)S) {
      const int g = lead[e_lead[e]];
      if (g < G) {
        slot[g * S + (int)e_r[e]] = e_rank[e] + 1u;
        if (e_r[e] == 0u) gcodes[g] = e_code[e];
      }
    }
  }
  const int shown = opened < G ? opened : G;
  for (int g = shown + tid; g < G; g += NT) gcodes[g] = HX_GROUP_MISSING;
  if (tid == 0) a.group_counts[b] = shown;
  __syncthreads();
  uint64_t* o = a.out + (int64_t)b * GS;
  for (int i = tid; i < GS; i += NT) {
    const uint32_t v = slot[i];
    o[i] = v ? keys[v - 1u] : 0ull;
  }
}

void launch_group_select(const GroupArgs& a, int B, hipStream_t st) {
  if (a.stride > 512) hipLaunchKernelGGL(k_group_select<1024>, dim3(B), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(k_group_select<256>, dim3(B), dim3(256), 0, st, a);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
