// Distance matrix search (hx_search_matrix): for every point of a sample, its nearest neighbours
// among the other points of the sample.  The sample is S local rows; sim(a, b) = spec_dot(row_a, row_b) in wave_spec_dot's
// order (lane-strided products added in index order, the off = 32 .. 1 tree, + 0.0f), every product and sum one fp32
// operation (-ffp-contract=off and the _rn intrinsics) -- the scan of k_reco_scan turned on itself: the staged "examples"
// are sample rows too.  Two kernels:
//   k_matrix_scan    every sim of the sample into an S x S fp32 plane; both (a, b) and (b, a) are computed, the products
//                    commute and the sums are made in the same order, so the two are the same bits;
//   k_matrix_select  one workgroup per sample row: the keys of its candidates, a bitonic sort in LDS, the best `limit` out.
// Nothing but the S sample rows of `dense` is read; keys are integers and every plane cell has one writer: the result does
// not depend on arrival order.
#include "hx_common.hpp"
#include "kernels.hpp"
#include "../../include/hx.h"

#include <algorithm>
#include <mutex>

namespace hx {

constexpr int MX_NT = 256;                      // four waves: one per SIMD
constexpr int MX_MAX_TJ = 64;                   // most staged rows of a workgroup
constexpr int MX_LDS_FLOATS = 12288;            // staged floats up to width 1024: 48 KB, three workgroups per CU
constexpr int MX_WIDE_TJ = 8;                   // staged rows above width 1024: 128 KB at width 4096
constexpr int MX_MAX_LDS = MX_WIDE_TJ * 4096 * 4;

int matrix_tile_rows(int dim_pad) {
  return dim_pad <= 1024 ? std::clamp(MX_LDS_FLOATS / dim_pad, MX_WIDE_TJ, MX_MAX_TJ) : MX_WIDE_TJ;
}

// Workgroup (bx, by): sample rows j in [by * TJ, + TJ) are staged in LDS (dynamic: TJ x dim_pad floats), read where they lie
// in `dense` through the row list; its waves then walk the sample rows i in [bx * TI, + TI).
// Rows of at most 1024 floats (WIDE = false): a wave keeps four rows i in registers, 16 chunks of 64 floats each -- all
// loads issued before the first sum -- and reduces the four trees of one staged row together, the packed 7-exchange
// reduction of k_reco_scan.  Wider rows (WIDE = true): one row i per wave, walked once per staged row in index order; the
// row comes from the vector cache from the second staged row on.
template <bool WIDE>
__global__ __launch_bounds__(MX_NT) void k_matrix_scan(MatrixArgs a, int TJ, int TI) {
  extern __shared__ __attribute__((aligned(16))) float stage[];
  __shared__ uint32_t s_jrow[MX_MAX_TJ];
  constexpr int NC = 16, RR = WIDE ? 1 : 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dim_pad = a.dim_pad, S = a.S;
  const int j0 = blockIdx.y * TJ;
  const int nj = S - j0 < TJ ? S - j0 : TJ;
  if (tid < nj) s_jrow[tid] = a.rows[j0 + tid];
  __syncthreads();
  for (int t = tid * 4; t < nj * dim_pad; t += MX_NT * 4) {     // (dim_pad is a multiple of 64: a float4 stays in its row)
    const int jj = t / dim_pad, k = t - jj * dim_pad;
    *(float4*)(stage + t) = *(const float4*)(a.dense + (int64_t)s_jrow[jj] * dim_pad + k);
  }
  __syncthreads();
  const int i_begin = blockIdx.x * TI;
  const int i_end = i_begin + TI < S ? i_begin + TI : S;
  for (int i0 = i_begin + w * RR; i0 < i_end; i0 += (MX_NT / 64) * RR) {       // wave-uniform
    bool on[RR];
    float xv[RR][NC];
    const float* x[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      on[r] = i0 + r < i_end;
      const uint32_t row = a.rows[on[r] ? i0 + r : i_begin];
      x[r] = a.dense + (int64_t)row * dim_pad + lane;
      if (!WIDE) {
#pragma unroll
        for (int c = 0; c < NC; ++c) xv[r][c] = c * 64 < dim_pad ? x[r][c * 64] : 0.0f;   // (a row past the end: row i_begin again, never written)
      }
    }
    // lanes 0, 16, 32 and 48 end up with the sims of rows 0, 2, 1 and 3 (k_reco_scan); the wide form keeps its row in lane 0
    const int my_r = WIDE ? 0 : ((((lane >> 4) & 1) << 1) | ((lane >> 5) & 1));
    bool my_on = on[0];
#pragma unroll
    for (int r = 1; r < RR; ++r) my_on = my_r == r ? on[r] : my_on;
    const bool owner = (WIDE ? lane == 0 : (lane & 15) == 0) && my_on;
    float* out = a.plane + (int64_t)(i0 + my_r) * S + j0;
    for (int jj = 0; jj < nj; ++jj) {
      const float* q = stage + jj * dim_pad + lane;
      float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      float s;
      if (WIDE) {
        for (int k = 0; k < dim_pad; k += 64) p[0] = __fadd_rn(p[0], __fmul_rn(x[0][k], q[k]));
        s = p[0];
#pragma unroll
        for (int off = 32; off >= 16; off >>= 1) s = __fadd_rn(s, __shfl_down(s, off, 64));
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (c * 64 < dim_pad) {
            const float qc = q[c * 64];
#pragma unroll
            for (int r = 0; r < RR; ++r) p[r] = __fadd_rn(p[r], __fmul_rn(xv[r][c], qc));
          }
        }
        const bool up = (lane & 32) != 0, hi = (lane & 16) != 0;
        const float A = __fadd_rn(up ? p[1] : p[0], __shfl_xor(up ? p[0] : p[1], 32, 64));
        const float B = __fadd_rn(up ? p[3] : p[2], __shfl_xor(up ? p[2] : p[3], 32, 64));
        s = __fadd_rn(hi ? B : A, __shfl_xor(hi ? A : B, 16, 64));
      }
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) s = __fadd_rn(s, __shfl_down(s, off, 64));
      s = __fadd_rn(s, 0.0f);
      if (owner) out[jj] = s;
    }
  }
}

// One workgroup per sample row i, blockDim.x = P / 2 threads (at least 64, at most 1024), P = the power of two >= S: slot j
// of the LDS array takes the key of candidate j, 0 for j = i, a sim below the threshold (a NaN sim included) and j >= S; a
// bitonic sort, descending; the first min(limit, candidates) keys out, 0 past them.
__global__ __launch_bounds__(1024) void k_matrix_select(MatrixArgs a, float threshold, uint32_t id_base, int limit, int P,
                                                        uint64_t* __restrict__ out_keys, int* __restrict__ out_counts) {
  __shared__ uint64_t ks[HX_MATRIX_MAX_SAMPLE];
  __shared__ int s_cnt;
  const int i = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, S = a.S;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const float* sims = a.plane + (int64_t)i * S;
  int mine = 0;
  for (int j = tid; j < P; j += nt) {
    uint64_t k = 0ull;
    if (j < S && j != i) {
      const float s = sims[j];
      if (s >= threshold) {
        k = make_key(s, id_base + a.rows[j]);
        ++mine;
      }
    }
    ks[j] = k;
  }
  if (mine) atomicAdd(&s_cnt, mine);               // (an integer sum: the same on every run)
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += nt) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t kl = ks[lo], kh = ks[hi];
        if ((kl < kh) == ((lo & k) == 0)) {
          ks[lo] = kh;
          ks[hi] = kl;
        }
      }
      __syncthreads();
    }
  const int n = s_cnt < limit ? s_cnt : limit;     // (n <= S - 1 < P)
  for (int t = tid; t < limit; t += nt) out_keys[(int64_t)i * limit + t] = t < n ? ks[t] : 0ull;
  if (tid == 0) out_counts[i] = n;
}

template <bool WIDE>
static void matrix_scan_launch(const MatrixArgs& a, hipStream_t st) {
  {   // the dynamic-LDS opt-in is a property of the function ON A DEVICE: once per device, under a lock
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      HX_HIP(hipFuncSetAttribute((const void*)k_matrix_scan<WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, MX_MAX_LDS));
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  constexpr int RR = WIDE ? 1 : 4;
  const int TJ = matrix_tile_rows(a.dim_pad);
  const int nby = (a.S + TJ - 1) / TJ;
  // rows i of a workgroup: one group of RR per wave while that fills the device (256 CUs, several workgroups each), four
  // groups per wave above -- a staged block then serves four times the rows
  int TI = (MX_NT / 64) * RR;
  if ((int64_t)((a.S + TI - 1) / TI) * nby >= 8192) TI *= 4;
  const int nbx = (a.S + TI - 1) / TI;
  hipLaunchKernelGGL(k_matrix_scan<WIDE>, dim3(nbx, nby), dim3(MX_NT), (size_t)TJ * a.dim_pad * 4, st, a, TJ, TI);
  HX_HIP(hipGetLastError());
}

void launch_matrix_scan(const MatrixArgs& a, hipStream_t st) {
  HX_CHECK(a.S >= 1 && a.S <= HX_MATRIX_MAX_SAMPLE, "matrix scan: sample size");
  HX_CHECK(a.dim_pad % 64 == 0 && a.dim_pad >= 64 && a.dim_pad <= 4096, "matrix scan: row width");
  if (a.dim_pad <= 1024) matrix_scan_launch<false>(a, st);
  else matrix_scan_launch<true>(a, st);
}

void launch_matrix_select(const MatrixArgs& a, float threshold, uint32_t id_base, int limit, uint64_t* out_keys,
                          int* out_counts, hipStream_t st) {
  HX_CHECK(a.S >= 1 && a.S <= HX_MATRIX_MAX_SAMPLE && limit >= 1, "matrix select: sample size or limit");
  const int P = next_pow2(std::max(a.S, 2));
  const int nt = std::clamp(P / 2, 64, 1024);
  hipLaunchKernelGGL(k_matrix_select, dim3(a.S), dim3(nt), 0, st, a, threshold, id_base, limit, P, out_keys, out_counts);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
