// Discovery and context search (hx_discover): a target and context pairs scored in one exact scan.
// The examples of a call lie in the matrix X of reco.hip (launch_reco_examples), request by request: the target when the
// request has one, then pos_0, neg_0, pos_1, neg_1, ...  k_discover_scan scores every row of the collection against
// every example as k_reco_scan does -- sim(x, e) = spec_dot(x, e) in wave_spec_dot's order, four rows per wave, the packed
// 7-exchange tree; that core is restated here so that k_reco_scan's registers do not move -- and folds a pair's two sims
// into the score as soon as the second is known.  Selection is on the 64-bit KEY, not on the score: context scores are
// exactly +0 for every row on the positive side of every pair, and a score threshold would pass each of those rows.
#include "hx_common.hpp"
#include "kernels.hpp"
#include "../../include/hx.h"

#include <mutex>

namespace hx {

constexpr int DISC_NT = 256;             // four waves: one per SIMD
constexpr int DISC_MAX_REQ = HX_RECO_MAX_REQUESTS;

// v / (1 + |v|): one add, one correctly rounded division
__device__ __forceinline__ float fast_sigmoid(float v) { return __fdiv_rn(v, __fadd_rn(1.0f, __builtin_fabsf(v))); }

// tau_key[r] = the limit-th best key of request r when its compacted list is full (launch_compact leaves it sorted), else 0
__global__ __launch_bounds__(64) void k_discover_tau(const uint64_t* __restrict__ cand, int cap, const int* __restrict__ cnt,
                                                     int R, int limit, uint64_t* tau_key) {
  const int r = threadIdx.x;
  if (r < R) tau_key[r] = cnt[r] >= limit ? cand[(int64_t)r * cap + limit - 1] : 0ull;
}
void launch_discover_tau(const uint64_t* cand, int cap, const int* cnt, int R, int limit, uint64_t* tau_key, hipStream_t st) {
  HX_CHECK(R >= 1 && R <= 64 && limit >= 1 && limit <= cap, "discover tau: sizes");
  hipLaunchKernelGGL(k_discover_tau, dim3(1), dim3(64), 0, st, cand, cap, cnt, R, limit, tau_key);
  HX_HIP(hipGetLastError());
}

// The row walk, the staging and the reduction are k_reco_scan's (reco.hip: the two forms, the LDS layout, lanes 0, 16, 32
// and 48 owning rows 0, 2, 1 and 3).  RecoReq.n_pos is 1 when the request has a target (its first example) and 0 when not.
// Per request the owner lanes keep three floats: the target's sim, the sim of the pair's positive, the running rank / sum.
template <bool WIDE>
__global__ __launch_bounds__(DISC_NT) void k_discover_scan(DiscoverScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ex[];
  __shared__ RecoReq s_req[DISC_MAX_REQ];
  __shared__ uint32_t s_excl[DISC_MAX_REQ * RECO_MAX_EXCL];
  __shared__ uint64_t s_tau[DISC_MAX_REQ];
  constexpr int NC = 16, RR = WIDE ? 1 : 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dim_pad = a.dim_pad;
  if (tid < a.n_req) {
    s_req[tid] = a.req[tid];
    s_tau[tid] = a.tau_key[a.req[tid].slot];
  }
  __syncthreads();
  for (int i = 0; i < a.n_req; ++i) {
    const RecoReq r = s_req[i];
    const float* src = a.X + (int64_t)r.ex0 * dim_pad;
    float* dst = ex + (int64_t)r.lds0 * dim_pad;
    for (int j = tid * 4; j < r.n_ex * dim_pad; j += DISC_NT * 4) *(float4*)(dst + j) = *(const float4*)(src + j);
    if (tid < r.n_excl) s_excl[i * RECO_MAX_EXCL + tid] = a.excl[r.excl0 + tid];
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * (DISC_NT / 64) * RR;
  for (int64_t r0 = a.row_begin + ((int64_t)blockIdx.x * (DISC_NT / 64) + w) * RR; r0 < a.row_end; r0 += stride) {
    bool on[RR];
    bool any = false;
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const int64_t row = r0 + r;
      bool o = row < a.row_end;
      if (o && a.mask) o = (a.mask[row >> 5] >> (row & 31)) & 1u;
      on[r] = __builtin_amdgcn_readfirstlane((int)o);
      any = any || on[r];
    }
    if (!any) continue;
    float xv[RR][NC];
    const float* x[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      x[r] = a.dense + (on[r] ? r0 + r : a.row_begin) * dim_pad + lane;
      if (!WIDE) {
#pragma unroll
        for (int c = 0; c < NC; ++c) xv[r][c] = (on[r] && c * 64 < dim_pad) ? x[r][c * 64] : 0.0f;
      }
    }
    const int my_r = WIDE ? 0 : ((((lane >> 4) & 1) << 1) | ((lane >> 5) & 1));
    bool my_on = on[0];
#pragma unroll
    for (int r = 1; r < RR; ++r) my_on = my_r == r ? on[r] : my_on;
    const uint32_t my_row = (uint32_t)(r0 + my_r);
    const bool owner = WIDE ? lane == 0 : (lane & 15) == 0;
    for (int i = 0; i < a.n_req; ++i) {
      const RecoReq rq = s_req[i];
      const bool has_target = rq.n_pos != 0;
      float tsim = 0.0f, spos = 0.0f, acc = 0.0f;
      for (int e = 0; e < rq.n_ex; ++e) {
        const float* qe = ex + (int64_t)(rq.lds0 + e) * dim_pad + lane;
        float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float s;
        if (WIDE) {
          for (int j = 0; j < dim_pad; j += 64) p[0] = __fadd_rn(p[0], __fmul_rn(x[0][j], qe[j]));
          s = p[0];
#pragma unroll
          for (int off = 32; off >= 16; off >>= 1) s = __fadd_rn(s, __shfl_down(s, off, 64));
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (c * 64 < dim_pad) {
              const float q = qe[c * 64];
#pragma unroll
              for (int r = 0; r < RR; ++r) p[r] = __fadd_rn(p[r], __fmul_rn(xv[r][c], q));
            }
          }
          const bool up = (lane & 32) != 0, hi = (lane & 16) != 0;
          const float A = __fadd_rn(up ? p[1] : p[0], __shfl_xor(up ? p[0] : p[1], 32, 64));
          const float B = __fadd_rn(up ? p[3] : p[2], __shfl_xor(up ? p[2] : p[3], 32, 64));
          s = __fadd_rn(hi ? B : A, __shfl_xor(hi ? A : B, 16, 64));
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) s = __fadd_rn(s, __shfl_down(s, off, 64));
        s = __fadd_rn(s, 0.0f);                    // the owner lanes hold sim(x, e) of their rows
        const int k = e - rq.n_pos;                // position among the pairs' examples: even = positive, odd = negative
        if (k < 0) {
          tsim = s;
        } else if ((k & 1) == 0) {
          spos = s;
        } else if (has_target) {                   // discovery: the pair votes +1, -1 or 0
          acc = __fadd_rn(acc, spos > s ? 1.0f : (spos < s ? -1.0f : 0.0f));
        } else {                                   // context: what the row lacks to the pair's positive side, squashed
          const float d = __fsub_rn(__fsub_rn(spos, s), 0x1p-23f);
          acc = __fadd_rn(acc, fast_sigmoid(d < 0.0f ? d : 0.0f));
        }
      }
      // a stored example of the request?  the 16 lanes of a quarter compare the request's (at most 32) rows with theirs
      const int j = lane & 15;
      const uint32_t* xl = s_excl + i * RECO_MAX_EXCL;
      const bool hit = (j < rq.n_excl && xl[j] == my_row) || (j + 16 < rq.n_excl && xl[j + 16] == my_row);
      const uint64_t m = __ballot(hit);
      const bool excluded = WIDE ? m != 0ull : ((m >> (lane & 48)) & 0xFFFFull) != 0ull;
      if (owner && my_on && !excluded) {
        float s = acc;
        if (has_target) s = __fadd_rn(acc, __fmul_rn(0.5f, __fadd_rn(fast_sigmoid(tsim), 1.0f)));
        s = __fadd_rn(s, 0.0f);
        // the key, id included, against the limit-th best key so far: a tied row of a later chunk has a larger id and a
        // smaller key, so it never passes
        const uint64_t key = make_key(s, a.id_base + my_row);
        if (key > s_tau[i]) {
          const int slot = atomicAdd(a.cnt + rq.slot, 1);
          if (slot < a.cap) a.cand[(int64_t)rq.slot * a.cap + slot] = key;
          else a.ovf[rq.slot] = 1;
        }
      }
    }
  }
}

template <bool WIDE>
static void discover_scan_launch(const DiscoverScanArgs& a, int lds_examples, hipStream_t st) {
  const size_t lds = (size_t)lds_examples * a.dim_pad * 4;
  {   // the dynamic-LDS opt-in is a property of the function ON A DEVICE: once per device, under a lock
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      HX_HIP(hipFuncSetAttribute((const void*)k_discover_scan<WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 RECO_LDS_FLOATS * 4));
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  // the grid of reco_scan_launch: what the rows give, at most the CUs times the workgroups one CU's 160 KB of LDS hold
  constexpr int RR = WIDE ? 1 : 4;
  const int64_t rows = a.row_end - a.row_begin;
  const int64_t want = (rows + (DISC_NT / 64) * RR - 1) / ((DISC_NT / 64) * RR);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + 4096)));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 256 * per_cu));
  hipLaunchKernelGGL(k_discover_scan<WIDE>, dim3(grid), dim3(DISC_NT), lds, st, a);
  HX_HIP(hipGetLastError());
}

void launch_discover_scan(const DiscoverScanArgs& a, int lds_examples, hipStream_t st) {
  if (a.row_end <= a.row_begin || a.n_req <= 0) return;
  HX_CHECK(a.n_req <= DISC_MAX_REQ && (int64_t)lds_examples * a.dim_pad <= RECO_LDS_FLOATS, "discover scan: launch too large");
  HX_CHECK(a.dim_pad % 64 == 0 && a.dim_pad <= 4096, "discover scan: row width");
  if (a.dim_pad <= 1024) discover_scan_launch<false>(a, lds_examples, st);
  else discover_scan_launch<true>(a, lds_examples, st);
}

}  // namespace hx
