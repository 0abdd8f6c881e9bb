// Upsert by an existing id (hx.h: hx_replace_rows, hx_payload_replace, hx_payload_replace_lists):
// the kernels that write derived rows into named positions and splice a CSR in which some documents change length.
//
// rows[0, count) are the replaced local rows, unique, in the caller's order; row i of a staging array (the derived copies
// of the new raw rows, laid out as the stored arrays are) goes to row rows[i] of the stored one.  Staging and destination
// are different allocations and the rows are unique, so a launch reads nothing it writes and no two lanes write one
// byte: one launch per array, no chunk plan, no bounce buffer (compact.hip needs both because it moves rows inside ONE
// allocation).
//   k_scatter_rows16 / k_scatter_u32   dst row rows[i] = src row i, 16-byte vectors (or one 4-byte word) per row
//   k_splice_map                       map[d - f] = i for every replaced document d = rows[i] >= f (the rest 0xFFFFFFFF)
//   k_csr_splice_len / k_csr_splice    the document-major CSR from document f on: the length of every document (the new
//            vector's where it is replaced), then the segmented copy of the postings from TWO sources -- the uploaded
//            batch for a replaced document, the old arrays for any other -- coalesced over destination postings, min /
//            max of the weights fused in, as k_csr_compact
//   k_csr_splice_u32                   the same segmented copy for one 4-byte element plane of a payload list column
// The offsets behind the copy come from compact.hip's k_csr_new_indptr, the copy back from its k_copy_u32.
#include "hx_common.hpp"
#include "kernels.hpp"
#include "replace.hpp"

#include <algorithm>

namespace hx {

constexpr int RP_WG = 256;
constexpr unsigned RP_GRID_MAX = 2048;   // 8 workgroups per CU, as compact.hip
constexpr uint32_t RP_KEEP = 0xFFFFFFFFu;   // map word of a document that is not replaced

// The mirror of k_compact_rows16: one wave per group of G SOURCE rows (G * vpr >= 1024 vectors where there are that many:
// 4 loads in flight per lane before the first store); magic = ceil(2^32 / vpr): e / vpr = umulhi(e, magic) for
// e < G * vpr.  The loads are consecutive, the stores are consecutive within a row.
__global__ void __launch_bounds__(RP_WG) k_scatter_rows16(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          const uint32_t* __restrict__ rows, int64_t count, int vpr,
                                                          int G, uint32_t magic) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * (RP_WG / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (RP_WG / WAVE);
  for (int64_t g = wave * G; g < count; g += n_waves * G) {
    const uint32_t T = (uint32_t)std::min<int64_t>(G, count - g) * (uint32_t)vpr;
    for (uint32_t e0 = lane; e0 < T; e0 += 4 * WAVE) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t e = e0 + k * WAVE;
        if (e < T) v[k] = src[g * vpr + e];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t e = e0 + k * WAVE;
        if (e < T) {
          const uint32_t r = __umulhi(e, magic);
          dst[(int64_t)rows[g + r] * vpr + (e - r * vpr)] = v[k];
        }
      }
    }
  }
}

void launch_scatter_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                           hipStream_t st) {
  if (count <= 0) return;
  HX_CHECK(row_bytes % 16 == 0 && row_bytes >= 32 && row_bytes <= 16384,
           "replace: row bytes must be a multiple of 16 in [32, 16384]");
  const int vpr = (int)(row_bytes / 16);
  const int G = std::max(4, (1024 + vpr - 1) / vpr);
  const uint32_t magic = (uint32_t)(((1ull << 32) + vpr - 1) / vpr);
  const int64_t waves = (count + G - 1) / G;
  const unsigned grid = (unsigned)std::min<int64_t>((waves + RP_WG / WAVE - 1) / (RP_WG / WAVE), RP_GRID_MAX);
  hipLaunchKernelGGL(k_scatter_rows16, dim3(grid), dim3(RP_WG), 0, st, (const uint4*)src, (uint4*)dst, rows, count, vpr, G,
                     magic);
  HX_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(RP_WG) k_scatter_u32(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                       const uint32_t* __restrict__ rows, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * RP_WG + threadIdx.x; i < count; i += (int64_t)gridDim.x * RP_WG)
    dst[rows[i]] = src[i];
}

void launch_scatter_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st) {
  if (count <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((count + RP_WG - 1) / RP_WG, RP_GRID_MAX);
  hipLaunchKernelGGL(k_scatter_u32, dim3(grid), dim3(RP_WG), 0, st, (const uint32_t*)src, (uint32_t*)dst, rows, count);
  HX_HIP(hipGetLastError());
}

// map[rows[i] - f] = i for the replaced documents at or past f (the caller filled map with RP_KEEP)
__global__ void __launch_bounds__(RP_WG) k_splice_map(const uint32_t* __restrict__ rows, int64_t count, uint32_t f,
                                                      int64_t docs, uint32_t* __restrict__ map) {
  for (int64_t i = (int64_t)blockIdx.x * RP_WG + threadIdx.x; i < count; i += (int64_t)gridDim.x * RP_WG) {
    const uint32_t r = rows[i];
    if (r >= f && (int64_t)(r - f) < docs) map[r - f] = (uint32_t)i;
  }
}

void launch_splice_map(const uint32_t* rows, int64_t count, int64_t f, int64_t docs, uint32_t* map, hipStream_t st) {
  if (count <= 0 || docs <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((count + RP_WG - 1) / RP_WG, RP_GRID_MAX);
  hipLaunchKernelGGL(k_splice_map, dim3(grid), dim3(RP_WG), 0, st, rows, count, (uint32_t)f, docs, map);
  HX_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------
// CSR splice: documents [f, f + m); indptr points at the offset of document f, new_indptr at the batch's offsets
// ---------------------------------------------------------------------------------
// len[j] = postings of document f + j after the call
__global__ void __launch_bounds__(RP_WG) k_csr_splice_len(const int64_t* __restrict__ indptr,
                                                          const uint32_t* __restrict__ map,
                                                          const int64_t* __restrict__ new_indptr, int64_t m,
                                                          int64_t* __restrict__ len) {
  const int64_t j = (int64_t)blockIdx.x * RP_WG + threadIdx.x;
  if (j >= m) return;
  const uint32_t b = map[j];
  len[j] = b == RP_KEEP ? indptr[j + 1] - indptr[j] : new_indptr[b + 1] - new_indptr[b];
}

void launch_csr_splice_len(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, int64_t m, int64_t* len,
                           hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_splice_len, dim3((unsigned)((m + RP_WG - 1) / RP_WG)), dim3(RP_WG), 0, st, indptr, map, new_indptr,
                     m, len);
  HX_HIP(hipGetLastError());
}

// k_csr_compact with two sources.  One workgroup per 256 documents: their source offsets -- into the uploaded batch for
// a replaced document (kept in LDS as -1 - offset), into the old arrays for any other -- and their destination offsets
// (off = the exclusive prefix of len, off[m] = the total) go to LDS, then the threads walk the workgroup's postings in
// destination order and find a posting's document by a binary search of the 256 offsets.  The postings go to idx2 /
// val2 (a spare buffer: destination position off[j] + k); mm[0] / mm[1] take the min / max of the copied weights as
// orderable u32 (k_minmax_f32's words).
__global__ void __launch_bounds__(RP_WG) k_csr_splice(const int64_t* __restrict__ indptr, const uint32_t* __restrict__ map,
                                                      const int64_t* __restrict__ new_indptr,
                                                      const int64_t* __restrict__ off, int64_t m,
                                                      const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                      const int32_t* __restrict__ new_idx,
                                                      const float* __restrict__ new_val, int32_t* __restrict__ idx2,
                                                      float* __restrict__ val2, uint32_t* __restrict__ mm) {
  __shared__ int64_t s_src[RP_WG];
  __shared__ int64_t s_dst[RP_WG + 1];
  const int64_t j0 = (int64_t)blockIdx.x * RP_WG;
  const int nd = (int)std::min<int64_t>(RP_WG, m - j0);
  const int64_t o0 = off[j0];
  if ((int)threadIdx.x < nd) {
    const uint32_t b = map[j0 + threadIdx.x];
    s_src[threadIdx.x] = b == RP_KEEP ? indptr[j0 + threadIdx.x] : -1 - new_indptr[b];
    s_dst[threadIdx.x] = off[j0 + threadIdx.x] - o0;
  }
  if (threadIdx.x == 0) s_dst[nd] = off[j0 + nd] - o0;
  __syncthreads();
  const int64_t total = s_dst[nd];
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int64_t p = threadIdx.x; p < total; p += RP_WG) {
    int a = 0, b = nd;               // the last document d with s_dst[d] <= p (empty documents share an offset)
    while (b - a > 1) {
      const int c = (a + b) >> 1;
      if (s_dst[c] <= p) a = c;
      else b = c;
    }
    const int64_t s0 = s_src[a], k = p - s_dst[a];
    int32_t t;
    float v;
    if (s0 < 0) {
      t = new_idx[-1 - s0 + k];
      v = new_val[-1 - s0 + k];
    } else {
      t = idx[s0 + k];
      v = val[s0 + k];
    }
    idx2[o0 + p] = t;
    val2[o0 + p] = v;
    const uint32_t u = f32_orderable(v);
    lo = u < lo ? u : lo;
    hi = u > hi ? u : hi;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, o, WAVE), h2 = __shfl_xor(hi, o, WAVE);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && lo <= hi) {
    atomicMin(mm + 0, lo);
    atomicMax(mm + 1, hi);
  }
}

void launch_csr_splice(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, const int64_t* off, int64_t m,
                       const int32_t* idx, const float* val, const int32_t* new_idx, const float* new_val, int32_t* idx2,
                       float* val2, uint32_t* mm, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_splice, dim3((unsigned)((m + RP_WG - 1) / RP_WG)), dim3(RP_WG), 0, st, indptr, map, new_indptr, off,
                     m, idx, val, new_idx, new_val, idx2, val2, mm);
  HX_HIP(hipGetLastError());
}

// k_csr_splice for one 4-byte plane without weights: the elements of a payload list column (a column of doubles calls
// it once per plane), written the way k_csr_compact_u32 stands beside k_csr_compact.
__global__ void __launch_bounds__(RP_WG) k_csr_splice_u32(const int64_t* __restrict__ indptr,
                                                          const uint32_t* __restrict__ map,
                                                          const int64_t* __restrict__ new_indptr,
                                                          const int64_t* __restrict__ off, int64_t m,
                                                          const uint32_t* __restrict__ src,
                                                          const uint32_t* __restrict__ new_src,
                                                          uint32_t* __restrict__ dst) {
  __shared__ int64_t s_src[RP_WG];
  __shared__ int64_t s_dst[RP_WG + 1];
  const int64_t j0 = (int64_t)blockIdx.x * RP_WG;
  const int nd = (int)std::min<int64_t>(RP_WG, m - j0);
  const int64_t o0 = off[j0];
  if ((int)threadIdx.x < nd) {
    const uint32_t b = map[j0 + threadIdx.x];
    s_src[threadIdx.x] = b == RP_KEEP ? indptr[j0 + threadIdx.x] : -1 - new_indptr[b];
    s_dst[threadIdx.x] = off[j0 + threadIdx.x] - o0;
  }
  if (threadIdx.x == 0) s_dst[nd] = off[j0 + nd] - o0;
  __syncthreads();
  const int64_t total = s_dst[nd];
  for (int64_t p = threadIdx.x; p < total; p += RP_WG) {
    int a = 0, b = nd;               // the last row d with s_dst[d] <= p (empty rows share an offset)
    while (b - a > 1) {
      const int c = (a + b) >> 1;
      if (s_dst[c] <= p) a = c;
      else b = c;
    }
    const int64_t s0 = s_src[a], k = p - s_dst[a];
    dst[o0 + p] = s0 < 0 ? new_src[-1 - s0 + k] : src[s0 + k];
  }
}

void launch_csr_splice_u32(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, const int64_t* off,
                           int64_t m, const uint32_t* src, const uint32_t* new_src, uint32_t* dst, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_splice_u32, dim3((unsigned)((m + RP_WG - 1) / RP_WG)), dim3(RP_WG), 0, st, indptr, map, new_indptr,
                     off, m, src, new_src, dst);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
