// MMR search (hx_mmr): maximal marginal relevance over a ranked pool.  With d = diversity,
// a = 1 - d, rel_i = the score of the key at position i and sim(i, j) = spec_dot(row_i, row_j) over the padded width of
// the normalised fp32 rows, step 0 values a position at v_i = a * rel_i and step t > 0 at v_i = a * rel_i - d * m_i, m_i =
// the largest sim(i, s) over the picks s so far; every step picks the eligible, unpicked position of the largest v, the
// smaller position on a tie.  All products, sums and differences are single fp32 operations (-ffp-contract=off and the
// _rn intrinsics), v + 0.0f makes -0 and +0 one value of the key order.
#include <stdlib.h>
#include "hx_common.hpp"
#include "kernels.hpp"

namespace hx {

constexpr int MMR_POOL = MAX_LIMIT;              // most keys of a pool
constexpr int MMR_DIM = 4096;                    // widest padded row (hx_create: dim <= 4096)
constexpr int MMR_R = 4;                         // candidate rows in flight per wave
constexpr uint32_t MMR_NO_ROW = 0xFFFFFFFFu;

// max over the workgroup of one 64-bit key per thread; `wbest` holds one word per wave.  Every thread returns the max.
template <int NT>
__device__ __forceinline__ uint64_t block_max_key(uint64_t k, uint64_t* wbest, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((long long)k, off, 64);
    k = o > k ? o : k;
  }
  __syncthreads();                               // (the words of the step before have been read)
  if ((tid & 63) == 0) wbest[tid >> 6] = k;
  __syncthreads();
  uint64_t best = 0ull;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint64_t o = wbest[w];
    best = o > best ? o : best;
  }
  return best;
}

// One workgroup per query, NT = 256 or 1024 threads.
//  setup   per position i < n: the key's internal id -> the local row, MMR_NO_ROW for an empty slot, a row this index does
//          not hold or a row whose bit is clear in the eligibility plane; rel[i] = the key's score; m[i] = -inf;
//  step t  (t > 0: the row picked last is staged into LDS, coalesced; wave w takes the positions 4 (w + k NT / 64) ..
//          + 3: all loads of its (up to) four rows are issued, then each row's sum against the staged row in
//          wave_spec_dot's order; lane 0 folds the result into m[i]);
//          every thread values the positions tid + k NT, v = a rel - d m (+ 0.0f), as the key orderable(v) << 32 |
//          0xFFFFFFFF - i; the largest key of the workgroup is the pick (shuffles inside a wave, one LDS word per wave).
template <int NT>
__global__ __launch_bounds__(NT) void k_mmr_select(MmrArgs a) {
  __shared__ __attribute__((aligned(16))) float stage[MMR_DIM];       // 16 KB: the row picked last
  __shared__ float rel[MMR_POOL];                                     // 8 KB
  __shared__ float mx[MMR_POOL];                                      // 8 KB
  __shared__ uint32_t rowof[MMR_POOL];                                // 8 KB: the local row; MMR_NO_ROW = never a pick
  __shared__ uint8_t picked[MMR_POOL];                                // 2 KB
  __shared__ uint64_t wbest[NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NW = NT / 64;
  const uint64_t* keys = a.keys + (int64_t)b * a.stride;     // as the caller gave them: what the result carries
  const uint64_t* ikeys = a.ikeys + (int64_t)b * a.stride;   // the same slots with internal ids: what names the rows
  int n = a.counts ? a.counts[b] : a.stride;
  n = n < 0 ? 0 : (n < a.stride ? n : a.stride);
  for (int i = tid; i < n; i += NT) {
    const uint64_t k = ikeys[i];
    const uint32_t id = key_id(k), row = id - a.id_base;
    uint32_t r = MMR_NO_ROW;
    if (k != 0ull && id >= a.id_base && (int64_t)row < a.n_rows) {
      if (!a.eligible || ((a.eligible[row >> 5] >> (row & 31)) & 1u)) r = row;
    }
    rowof[i] = r;
    rel[i] = key_score(k);
    mx[i] = -__builtin_inff();
    picked[i] = 0;
  }
  const float d = a.diversity, am = __fsub_rn(1.0f, d);
  uint64_t* okeys = a.out_keys + (int64_t)b * a.limit;
  float* ovals = a.out_values + (int64_t)b * a.limit;
  int t = 0;
  for (; t < a.limit; ++t) {                     // (block-uniform: every thread sees the same pick)
    __syncthreads();
    uint64_t best = 0ull;
    for (int i = tid; i < n; i += NT) {
      if (rowof[i] != MMR_NO_ROW && !picked[i]) {
        float v = __fmul_rn(am, rel[i]);
        if (t > 0) v = __fsub_rn(v, __fmul_rn(d, mx[i]));
        v = __fadd_rn(v, 0.0f);
        const uint64_t k = ((uint64_t)f32_orderable(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
        best = k > best ? k : best;
      }
    }
    best = block_max_key<NT>(best, wbest, tid);
    if (best == 0ull) break;                     // the pool is exhausted
    const int s = (int)(0xFFFFFFFFu - (uint32_t)best);
    if (tid == 0) {
      okeys[t] = keys[s];
      ovals[t] = orderable_f32((uint32_t)(best >> 32));
      picked[s] = 1;
    }
    if (t + 1 == a.limit) {
      ++t;
      break;
    }
    // the picked row into LDS
    const float* srow = a.rows + (int64_t)rowof[s] * a.dim_pad;
    for (int j = tid * 4; j < a.dim_pad; j += NT * 4) *(float4*)(stage + j) = *(const float4*)(srow + j);
    __syncthreads();
    for (int i0 = w * MMR_R; i0 < n; i0 += NW * MMR_R) {       // wave-uniform
      const float* x[MMR_R];
      bool on[MMR_R];
#pragma unroll
      for (int r = 0; r < MMR_R; ++r) {
        const int i = i0 + r;
        const uint32_t row = i < n ? rowof[i] : MMR_NO_ROW;
        on[r] = __builtin_amdgcn_readfirstlane((int)(row != MMR_NO_ROW && !picked[i < n ? i : 0]));
        x[r] = a.rows + (int64_t)(on[r] ? row : 0u) * a.dim_pad;
      }
      if (!(on[0] || on[1] || on[2] || on[3])) continue;
      float p[MMR_R] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int base = 0; base < a.dim_pad; base += 1024) {     // one pass for rows of at most 1024 floats
        const int left = a.dim_pad - base;
        float xv[MMR_R][16];
#pragma unroll
        for (int r = 0; r < MMR_R; ++r) {
#pragma unroll
          for (int c = 0; c < 16; ++c) xv[r][c] = (on[r] && c * 64 < left) ? x[r][base + c * 64 + lane] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          if (c * 64 < left) {
            const float q = stage[base + c * 64 + lane];
#pragma unroll
            for (int r = 0; r < MMR_R; ++r) p[r] = __fadd_rn(p[r], __fmul_rn(xv[r][c], q));
          }
        }
      }
#pragma unroll
      for (int r = 0; r < MMR_R; ++r) {
        float q = p[r];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) q = __fadd_rn(q, __shfl_down(q, off, 64));
        q = __fadd_rn(q, 0.0f);
        if (on[r] && lane == 0) {
          const float old = mx[i0 + r];
          mx[i0 + r] = q > old ? q : old;
        }
      }
    }
  }
  for (int i = t + tid; i < a.limit; i += NT) {
    okeys[i] = 0ull;
    ovals[i] = 0.0f;
  }
  if (tid == 0) a.out_counts[b] = t;
}

// threads of the workgroup for pools of `stride` slots; HX_DEBUG_MMR_NT=256|1024 forces one (scripts/mmr_bench.py)
static int mmr_threads(int stride) {
  static const int forced = getenv("HX_DEBUG_MMR_NT") ? atoi(getenv("HX_DEBUG_MMR_NT")) : 0;
  if (forced == 256 || forced == 1024) return forced;
  return stride > 64 ? 1024 : 256;   // measured: level at a pool of 50, 1024 ahead at 100 and 200
}

void launch_mmr_select(const MmrArgs& a, int B, hipStream_t st) {
  if (mmr_threads(a.stride) == 1024) hipLaunchKernelGGL(k_mmr_select<1024>, dim3(B), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(k_mmr_select<256>, dim3(B), dim3(256), 0, st, a);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
