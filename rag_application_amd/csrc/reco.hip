// Recommend search (hx_recommend): points like given examples.  The examples of a call lie in one
// matrix X [E x dim_pad] of normalised fp32 rows (stored rows copied where they lie, raw vectors prepared by
// k_prep_queries_f).  HX_RECO_AVERAGE forms one dense query per request here and goes through the dense stage; the two
// other strategies score every row of the collection against every example in k_reco_scan: sim(x, e) = spec_dot(x, e) in
// wave_spec_dot's order (lane-strided products added in index order, the off = 32 .. 1 tree, + 0.0f), every product, sum
// and difference one fp32 operation (-ffp-contract=off and the _rn intrinsics).
#include "hx_common.hpp"
#include "kernels.hpp"
#include "../../include/hx.h"

#include <mutex>

namespace hx {

// ---- the example matrix ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reco_examples(const float* __restrict__ dense, const float* __restrict__ raw_n,
                                                       const int64_t* __restrict__ src, int dim_pad, float* X) {
  const int e = blockIdx.x;
  const int64_t s = src[e];
  const float* from = s >= 0 ? dense + s * dim_pad : raw_n + (-1 - s) * dim_pad;
  for (int j = threadIdx.x * 4; j < dim_pad; j += 256 * 4)
    *(float4*)(X + (int64_t)e * dim_pad + j) = *(const float4*)(from + j);
}
void launch_reco_examples(const float* dense, const float* raw_n, const int64_t* src, int E, int dim_pad, float* X,
                          hipStream_t st) {
  if (E <= 0) return;
  hipLaunchKernelGGL(k_reco_examples, dim3(E), dim3(256), 0, st, dense, raw_n, src, dim_pad, X);
  HX_HIP(hipGetLastError());
}

// one workgroup per request; thread k owns elements k, k + 256, ...
__global__ __launch_bounds__(256) void k_reco_average(const float* __restrict__ X, const RecoReq* __restrict__ req, int dim,
                                                      int dim_pad, float* q) {
  const RecoReq r = req[blockIdx.x];
  const float* x = X + (int64_t)r.ex0 * dim_pad;
  const int n_neg = r.n_ex - r.n_pos;
  for (int k = threadIdx.x; k < dim; k += 256) {
    float p = x[k];
    for (int e = 1; e < r.n_pos; ++e) p = __fadd_rn(p, x[(int64_t)e * dim_pad + k]);
    p = __fdiv_rn(p, (float)r.n_pos);
    float o = p;
    if (n_neg > 0) {
      float n = x[(int64_t)r.n_pos * dim_pad + k];
      for (int e = r.n_pos + 1; e < r.n_ex; ++e) n = __fadd_rn(n, x[(int64_t)e * dim_pad + k]);
      n = __fdiv_rn(n, (float)n_neg);
      o = __fadd_rn(p, __fsub_rn(p, n));
    }
    q[(int64_t)blockIdx.x * dim + k] = o;
  }
}
void launch_reco_average(const float* X, const RecoReq* req, int R, int dim, int dim_pad, float* q, hipStream_t st) {
  hipLaunchKernelGGL(k_reco_average, dim3(R), dim3(256), 0, st, X, req, dim, dim_pad, q);
  HX_HIP(hipGetLastError());
}

// one wave per request: the ranked list minus the request's stored examples, cut to `limit`
__global__ __launch_bounds__(64) void k_reco_drop(const uint64_t* __restrict__ in, int in_stride, const int* __restrict__ in_cnt,
                                                  const RecoReq* __restrict__ req, const uint32_t* __restrict__ excl,
                                                  uint32_t id_base, int limit, uint64_t* out, int* out_cnt) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const RecoReq r = req[b];
  int n = in_cnt[b];
  n = n < in_stride ? n : in_stride;
  int base = 0;
  for (int i0 = 0; i0 < n && base < limit; i0 += 64) {
    const int i = i0 + lane;
    const uint64_t k = i < n ? in[(int64_t)b * in_stride + i] : 0ull;
    bool keep = k != 0ull;
    const uint32_t row = key_id(k) - id_base;
    for (int j = 0; j < r.n_excl; ++j) keep = keep && excl[r.excl0 + j] != row;
    const uint64_t m = __ballot(keep);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < limit) out[(int64_t)b * limit + pos] = k;
    base += __popcll(m);
  }
  const int kept = base < limit ? base : limit;
  for (int i = kept + lane; i < limit; i += 64) out[(int64_t)b * limit + i] = 0ull;
  if (lane == 0) out_cnt[b] = kept;
}
void launch_reco_drop(const uint64_t* in, int in_stride, const int* in_cnt, const RecoReq* req, const uint32_t* excl,
                      uint32_t id_base, int R, int limit, uint64_t* out, int* out_cnt, hipStream_t st) {
  hipLaunchKernelGGL(k_reco_drop, dim3(R), dim3(64), 0, st, in, in_stride, in_cnt, req, excl, id_base, limit, out, out_cnt);
  HX_HIP(hipGetLastError());
}

// ---- the scan ---------------------------------------------------------------------------------------------------------
constexpr int RECO_NT = 256;             // four waves: one per SIMD
constexpr int RECO_MAX_REQ = HX_RECO_MAX_REQUESTS;

// Rows of at most 1024 floats (WIDE = false): a wave keeps four rows in flight, 16 chunks of 64 floats each in registers --
// all loads of its rows are issued before the first sum, as in wave_spec_dot and k_mmr_select.  Wider rows (WIDE = true):
// one row per wave, walked once per example in passes of 1024 floats, as wave_spec_dot walks them -- the row comes from
// the vector cache from the second example on; holding 64 chunks under run-time predicates spilled scalar registers.
// The workgroup stages the examples of its launch's requests in LDS once (dynamic: lds_examples x dim_pad floats, sized
// by the examples actually staged), with the requests' descriptors and their sorted stored-example rows.  Then, per
// row and request: every example's sum in wave_spec_dot's order, the six-step tree, + 0.0f; the lane that ends up with a
// row's sims folds them into the strategy's score and appends.
template <bool WIDE>
__global__ __launch_bounds__(RECO_NT) void k_reco_scan(RecoScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ex[];
  __shared__ RecoReq s_req[RECO_MAX_REQ];
  __shared__ uint32_t s_excl[RECO_MAX_REQ * RECO_MAX_EXCL];
  __shared__ float s_tau[RECO_MAX_REQ];
  constexpr int NC = 16, RR = WIDE ? 1 : 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dim_pad = a.dim_pad;
  if (tid < a.n_req) {
    s_req[tid] = a.req[tid];
    s_tau[tid] = a.tau[a.req[tid].slot];
  }
  __syncthreads();
  for (int i = 0; i < a.n_req; ++i) {
    const RecoReq r = s_req[i];
    const float* src = a.X + (int64_t)r.ex0 * dim_pad;
    float* dst = ex + (int64_t)r.lds0 * dim_pad;
    for (int j = tid * 4; j < r.n_ex * dim_pad; j += RECO_NT * 4) *(float4*)(dst + j) = *(const float4*)(src + j);
    if (tid < r.n_excl) s_excl[i * RECO_MAX_EXCL + tid] = a.excl[r.excl0 + tid];
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * (RECO_NT / 64) * RR;
  for (int64_t r0 = a.row_begin + ((int64_t)blockIdx.x * (RECO_NT / 64) + w) * RR; r0 < a.row_end; r0 += stride) {
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
    // The sims of the wave's four rows against one example are reduced TOGETHER: the off = 32 step of rows 0 | 1 (and of
    // 2 | 3) is one exchange of half-waves -- the lower half keeps row 0 and takes row 0's upper partials, the upper half
    // keeps row 1 and takes row 1's lower ones --, the off = 16 step folds the two results the same way, and off = 8 .. 1
    // run once on the packed register: 7 exchanges instead of 24, every sum the one lane 0's tree makes (fp32 addition
    // commutes bit for bit).  Lanes 0, 16, 32 and 48 then hold the sims of rows 0, 2, 1 and 3 and fold them into their
    // row's score; the wide form keeps its one row's tree in lane 0.
    const int my_r = WIDE ? 0 : ((((lane >> 4) & 1) << 1) | ((lane >> 5) & 1));
    bool my_on = on[0];
#pragma unroll
    for (int r = 1; r < RR; ++r) my_on = my_r == r ? on[r] : my_on;
    const uint32_t my_row = (uint32_t)(r0 + my_r);
    const bool owner = WIDE ? lane == 0 : (lane & 15) == 0;
    for (int i = 0; i < a.n_req; ++i) {
      const RecoReq rq = s_req[i];
      float sp = -__builtin_inff(), sm = -__builtin_inff(), acc = 0.0f;
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
        if (e < rq.n_pos) {
          sp = s > sp ? s : sp;
          acc = __fadd_rn(acc, s);
        } else {
          sm = s > sm ? s : sm;
          acc = __fsub_rn(acc, s);
        }
      }
      // a stored example of the request?  the 16 lanes of a quarter compare the request's (at most 32) rows with theirs
      const int j = lane & 15;
      const uint32_t* xl = s_excl + i * RECO_MAX_EXCL;
      const bool hit = (j < rq.n_excl && xl[j] == my_row) || (j + 16 < rq.n_excl && xl[j + 16] == my_row);
      const uint64_t m = __ballot(hit);
      const bool excluded = WIDE ? m != 0ull : ((m >> (lane & 48)) & 0xFFFFull) != 0ull;
      if (owner && my_on && !excluded) {
        float s = a.strategy == HX_RECO_BEST_SCORE ? (sp > sm ? sp : -__fmul_rn(sm, sm)) : acc;
        s = __fadd_rn(s, 0.0f);
        if (s >= s_tau[i]) {
          const int slot = atomicAdd(a.cnt + rq.slot, 1);
          if (slot < a.cap) a.cand[(int64_t)rq.slot * a.cap + slot] = make_key(s, a.id_base + my_row);
          else a.ovf[rq.slot] = 1;
        }
      }
    }
  }
}

template <bool WIDE>
static void reco_scan_launch(const RecoScanArgs& a, int lds_examples, hipStream_t st) {
  const size_t lds = (size_t)lds_examples * a.dim_pad * 4;
  {   // the dynamic-LDS opt-in is a property of the function ON A DEVICE: once per device, under a lock
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      HX_HIP(hipFuncSetAttribute((const void*)k_reco_scan<WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 RECO_LDS_FLOATS * 4));
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  // Workgroups: what the rows give, at most the CUs (256) times the workgroups one CU's LDS (160 KB) and wave slots hold
  // -- a launch with three examples runs eight workgroups per CU, one with 128 KB of them one.
  constexpr int RR = WIDE ? 1 : 4;
  const int64_t rows = a.row_end - a.row_begin;
  const int64_t want = (rows + (RECO_NT / 64) * RR - 1) / ((RECO_NT / 64) * RR);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + 4096)));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 256 * per_cu));
  hipLaunchKernelGGL(k_reco_scan<WIDE>, dim3(grid), dim3(RECO_NT), lds, st, a);
  HX_HIP(hipGetLastError());
}

void launch_reco_scan(const RecoScanArgs& a, int lds_examples, hipStream_t st) {
  if (a.row_end <= a.row_begin || a.n_req <= 0) return;
  HX_CHECK(a.n_req <= RECO_MAX_REQ && (int64_t)lds_examples * a.dim_pad <= RECO_LDS_FLOATS, "reco scan: launch too large");
  HX_CHECK(a.dim_pad % 64 == 0 && a.dim_pad <= 4096, "reco scan: row width");
  if (a.dim_pad <= 1024) reco_scan_launch<false>(a, lds_examples, st);
  else reco_scan_launch<true>(a, lds_examples, st);
}

}  // namespace hx
