// A stage that filters a ranked list (hx_list_keep): per query the walk of the list in rank order,
// keeping a slot when its key is not 0, (mask) its id names a row of this index whose bit is set and (thr) its score is
// not below the query's threshold; the first `limit` kept keys leave unchanged and in order, zeros follow them.
#include "hx_common.hpp"
#include "kernels.hpp"

namespace hx {

constexpr int LK_WAVES = 4;   // queries (waves) of one workgroup; the waves share nothing
constexpr int LK_U = 4;       // 64-key pieces a wave has in flight per step

// One wave per query.  The walk is order-preserving by construction: a step loads LK_U pieces of 64 consecutive slots (and,
// under a mask, gathers the mask word of each slot's row -- all loads of the step are issued before the first is used),
// then takes the pieces in order: __ballot of the keep predicate, a lane's output position = the keys written so far + the
// kept lanes below it.  The running count is wave-uniform, so the early stop (`limit` keys written) is a uniform branch.
// No LDS, no barrier, no atomics; lists of at most 8192 slots = 32 steps.
__global__ __launch_bounds__(LK_WAVES * 64) void k_list_keep(ListKeepArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * LK_WAVES + (threadIdx.x >> 6);
  if (b >= a.B) return;                                    // (wave-uniform)
  const uint64_t* keys = a.keys + (int64_t)b * a.stride;
  const uint64_t* ikeys = a.ikeys + (int64_t)b * a.stride;
  const bool same_ids = a.ikeys == a.keys;
  uint64_t* out = a.out + (int64_t)b * a.limit;
  int n = a.counts ? a.counts[b] : a.stride;
  n = n < 0 ? 0 : (n < a.stride ? n : a.stride);
  const bool has_thr = a.thr != nullptr;
  const float thr = has_thr ? a.thr[b] : 0.0f;
  const uint64_t below = (1ull << lane) - 1ull;
  int written = 0;
  for (int base = 0; base < n && written < a.limit; base += 64 * LK_U) {
    uint64_t k[LK_U];
    bool keep[LK_U];
#pragma unroll
    for (int u = 0; u < LK_U; ++u) {
      const int i = base + u * 64 + lane;
      k[u] = i < n ? keys[i] : 0ull;
      keep[u] = k[u] != 0ull;
    }
    if (a.mask) {
      uint32_t row[LK_U], word[LK_U];
#pragma unroll
      for (int u = 0; u < LK_U; ++u) {
        const int i = base + u * 64 + lane;
        const uint64_t ik = same_ids ? k[u] : (i < n ? ikeys[i] : 0ull);   // 0: an id of another index
        const uint32_t id = key_id(ik);
        row[u] = id - a.id_base;
        keep[u] = keep[u] && ik != 0ull && id >= a.id_base && (int64_t)row[u] < a.n_rows;
      }
#pragma unroll
      for (int u = 0; u < LK_U; ++u) word[u] = keep[u] ? a.mask[row[u] >> 5] : 0u;
#pragma unroll
      for (int u = 0; u < LK_U; ++u) keep[u] = ((word[u] >> (row[u] & 31u)) & 1u) != 0u;
    }
#pragma unroll
    for (int u = 0; u < LK_U; ++u) {
      if (has_thr) keep[u] = keep[u] && !(key_score(k[u]) < thr);
      const uint64_t kept = __ballot(keep[u]);
      const int pos = written + __popcll(kept & below);
      if (keep[u] && pos < a.limit) out[pos] = k[u];
      written += __popcll(kept);
    }
  }
  written = written < a.limit ? written : a.limit;
  for (int i = written + lane; i < a.limit; i += 64) out[i] = 0ull;
  if (lane == 0) a.out_counts[b] = written;
}

void launch_list_keep(const ListKeepArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_list_keep, dim3((unsigned)((a.B + LK_WAVES - 1) / LK_WAVES)), dim3(LK_WAVES * 64), 0, st, a);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
