// Per-point deletes (hx.h: hx_retain_rows): the kernels that compact the stored copies.
//
// rows[0, count) is the ascending list of kept rows (mask.hip); row i of the result is old row rows[i], so a row only
// ever moves DOWN (i <= rows[i]) and the rows in front of the first deleted one do not move at all.  One in-place
// gather launch would still race: the workgroup that writes position p may run before the one that has to read old
// row p.  The host (lifecycle.hip) therefore cuts the destination rows into stream-ordered chunks [d0, d1) of two kinds:
//   direct   rows[d0] >= d1: every source row of the chunk lies at or past d1, every destination row below it -- the
//            launch reads nothing it writes, the gather goes straight into place;
//   bounced  otherwise: the chunk is gathered into a bounce buffer small enough to stay in the Infinity Cache and
//            copied into place by the next launch.  Later chunks only read rows at or past d1, which neither touched.
//   k_compact_rows16 / k_compact_u32   dst row i = src row rows[i], 16-byte vectors (or one 4-byte scale) per row
//   k_copy16 / k_copy_u32              the bounce buffer into place
//   k_csr_keep_len / k_csr_compact / k_csr_new_indptr   the document-major CSR: lengths of the kept documents, the
//            segmented copy of their postings (coalesced over postings, min / max of the surviving weights fused in),
//            the new offsets
//   k_csr_compact_u32                  the same segmented copy for one 4-byte element plane of a payload list column
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int CP_WG = 256;
constexpr unsigned CP_GRID_MAX = 2048;   // 8 workgroups per CU: 32 waves with 4 x 16 B in flight per lane

// One wave per group of G destination rows (G * vpr >= 1024 vectors where the chunk has that many: 4 loads in flight
// per lane before the first store).  magic = ceil(2^32 / vpr): e / vpr = umulhi(e, magic) for e < G * vpr (engine.hip
// keeps G * vpr * vpr below 2^32).  src and dst may be the same allocation; the launch never reads a byte it writes.
__global__ void __launch_bounds__(CP_WG) k_compact_rows16(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          const uint32_t* __restrict__ rows, int64_t count, int vpr,
                                                          int G, uint32_t magic) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * (CP_WG / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (CP_WG / WAVE);
  for (int64_t g = wave * G; g < count; g += n_waves * G) {
    const uint32_t T = (uint32_t)std::min<int64_t>(G, count - g) * (uint32_t)vpr;
    for (uint32_t e0 = lane; e0 < T; e0 += 4 * WAVE) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t e = e0 + k * WAVE;
        if (e < T) {
          const uint32_t r = __umulhi(e, magic);
          v[k] = src[(int64_t)rows[g + r] * vpr + (e - r * vpr)];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t e = e0 + k * WAVE;
        if (e < T) dst[g * vpr + e] = v[k];
      }
    }
  }
}

void launch_compact_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                           hipStream_t st) {
  if (count <= 0) return;
  HX_CHECK(row_bytes % 16 == 0 && row_bytes >= 32 && row_bytes <= 16384,
           "compact: row bytes must be a multiple of 16 in [32, 16384]");
  const int vpr = (int)(row_bytes / 16);
  const int G = std::max(4, (1024 + vpr - 1) / vpr);
  const uint32_t magic = (uint32_t)(((1ull << 32) + vpr - 1) / vpr);
  const int64_t waves = (count + G - 1) / G;
  const unsigned grid = (unsigned)std::min<int64_t>((waves + CP_WG / WAVE - 1) / (CP_WG / WAVE), CP_GRID_MAX);
  hipLaunchKernelGGL(k_compact_rows16, dim3(grid), dim3(CP_WG), 0, st, (const uint4*)src, (uint4*)dst, rows, count, vpr, G,
                     magic);
  HX_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(CP_WG) k_compact_u32(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                       const uint32_t* __restrict__ rows, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * CP_WG + threadIdx.x; i < count; i += (int64_t)gridDim.x * CP_WG)
    dst[i] = src[rows[i]];
}

void launch_compact_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st) {
  if (count <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((count + CP_WG - 1) / CP_WG, CP_GRID_MAX);
  hipLaunchKernelGGL(k_compact_u32, dim3(grid), dim3(CP_WG), 0, st, (const uint32_t*)src, (uint32_t*)dst, rows, count);
  HX_HIP(hipGetLastError());
}

// dst[0, n) = src[0, n) (16-byte vectors; disjoint buffers), four loads in flight per lane
__global__ void __launch_bounds__(CP_WG) k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * CP_WG;
  for (int64_t e0 = (int64_t)blockIdx.x * CP_WG + threadIdx.x; e0 < n; e0 += 4 * step) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e0 + k * step < n) v[k] = src[e0 + k * step];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e0 + k * step < n) dst[e0 + k * step] = v[k];
  }
}

void launch_copy16(const void* src, void* dst, int64_t bytes, hipStream_t st) {
  if (bytes <= 0) return;
  HX_CHECK(bytes % 16 == 0, "compact: copy bytes must be a multiple of 16");
  const int64_t n = bytes / 16;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 4 * CP_WG - 1) / (4 * CP_WG), CP_GRID_MAX);
  hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(CP_WG), 0, st, (const uint4*)src, (uint4*)dst, n);
  HX_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(CP_WG) k_copy_u32(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                    int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * CP_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * CP_WG) dst[i] = src[i];
}

void launch_copy_u32(const void* src, void* dst, int64_t n, hipStream_t st) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((n + CP_WG - 1) / CP_WG, CP_GRID_MAX);
  hipLaunchKernelGGL(k_copy_u32, dim3(grid), dim3(CP_WG), 0, st, (const uint32_t*)src, (uint32_t*)dst, n);
  HX_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------
// document-major CSR
// ---------------------------------------------------------------------------------
// len[j] = postings of kept document rows[j], j < m
__global__ void __launch_bounds__(CP_WG) k_csr_keep_len(const int64_t* __restrict__ indptr,
                                                        const uint32_t* __restrict__ rows, int64_t m,
                                                        int64_t* __restrict__ len) {
  const int64_t j = (int64_t)blockIdx.x * CP_WG + threadIdx.x;
  if (j >= m) return;
  const int64_t r = rows[j];
  len[j] = indptr[r + 1] - indptr[r];
}

void launch_csr_keep_len(const int64_t* indptr, const uint32_t* rows, int64_t m, int64_t* len, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_keep_len, dim3((unsigned)((m + CP_WG - 1) / CP_WG)), dim3(CP_WG), 0, st, indptr, rows, m, len);
  HX_HIP(hipGetLastError());
}

// One workgroup per 256 kept documents: their source offsets and their destination offsets (off = the exclusive prefix
// of len, off[m] = the total) go to LDS, then the threads walk the workgroup's postings in destination order -- every
// wave reads and writes consecutive postings except where a document ends -- and find a posting's document by a binary
// search of the 256 offsets.  The postings go to idx2 / val2 (a spare buffer: destination position off[j] + k); mm[0] /
// mm[1] take the min / max of the copied weights as orderable u32 (k_minmax_f32's words).
__global__ void __launch_bounds__(CP_WG) k_csr_compact(const int64_t* __restrict__ indptr,
                                                       const uint32_t* __restrict__ rows,
                                                       const int64_t* __restrict__ off, int64_t m,
                                                       const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                       int32_t* __restrict__ idx2, float* __restrict__ val2,
                                                       uint32_t* __restrict__ mm) {
  __shared__ int64_t s_src[CP_WG];
  __shared__ int64_t s_dst[CP_WG + 1];
  const int64_t j0 = (int64_t)blockIdx.x * CP_WG;
  const int nd = (int)std::min<int64_t>(CP_WG, m - j0);
  const int64_t o0 = off[j0];
  if ((int)threadIdx.x < nd) {
    s_src[threadIdx.x] = indptr[rows[j0 + threadIdx.x]];
    s_dst[threadIdx.x] = off[j0 + threadIdx.x] - o0;
  }
  if (threadIdx.x == 0) s_dst[nd] = off[j0 + nd] - o0;
  __syncthreads();
  const int64_t total = s_dst[nd];
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int64_t p = threadIdx.x; p < total; p += CP_WG) {
    int a = 0, b = nd;               // the last document d with s_dst[d] <= p (empty documents share an offset)
    while (b - a > 1) {
      const int c = (a + b) >> 1;
      if (s_dst[c] <= p) a = c;
      else b = c;
    }
    const int64_t s = s_src[a] + (p - s_dst[a]);
    const float v = val[s];
    idx2[o0 + p] = idx[s];
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

void launch_csr_compact(const int64_t* indptr, const uint32_t* rows, const int64_t* off, int64_t m, const int32_t* idx,
                        const float* val, int32_t* idx2, float* val2, uint32_t* mm, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_compact, dim3((unsigned)((m + CP_WG - 1) / CP_WG)), dim3(CP_WG), 0, st, indptr, rows, off, m, idx,
                     val, idx2, val2, mm);
  HX_HIP(hipGetLastError());
}

// k_csr_compact for one 4-byte plane without weights: the elements of a payload list column (a
// column of doubles calls it once per plane).  Same walk: 256 kept rows per workgroup, destination order.
__global__ void __launch_bounds__(CP_WG) k_csr_compact_u32(const int64_t* __restrict__ indptr,
                                                           const uint32_t* __restrict__ rows,
                                                           const int64_t* __restrict__ off, int64_t m,
                                                           const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  __shared__ int64_t s_src[CP_WG];
  __shared__ int64_t s_dst[CP_WG + 1];
  const int64_t j0 = (int64_t)blockIdx.x * CP_WG;
  const int nd = (int)std::min<int64_t>(CP_WG, m - j0);
  const int64_t o0 = off[j0];
  if ((int)threadIdx.x < nd) {
    s_src[threadIdx.x] = indptr[rows[j0 + threadIdx.x]];
    s_dst[threadIdx.x] = off[j0 + threadIdx.x] - o0;
  }
  if (threadIdx.x == 0) s_dst[nd] = off[j0 + nd] - o0;
  __syncthreads();
  const int64_t total = s_dst[nd];
  for (int64_t p = threadIdx.x; p < total; p += CP_WG) {
    int a = 0, b = nd;               // the last row d with s_dst[d] <= p (empty rows share an offset)
    while (b - a > 1) {
      const int c = (a + b) >> 1;
      if (s_dst[c] <= p) a = c;
      else b = c;
    }
    dst[o0 + p] = src[s_src[a] + (p - s_dst[a])];
  }
}

void launch_csr_compact_u32(const int64_t* indptr, const uint32_t* rows, const int64_t* off, int64_t m, const uint32_t* src,
                            uint32_t* dst, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_csr_compact_u32, dim3((unsigned)((m + CP_WG - 1) / CP_WG)), dim3(CP_WG), 0, st, indptr, rows, off, m,
                     src, dst);
  HX_HIP(hipGetLastError());
}

// indptr[j] = base + off[j], j <= m (the offsets of the documents that moved; behind the segmented copy, which reads
// the old ones)
__global__ void __launch_bounds__(CP_WG) k_csr_new_indptr(int64_t* __restrict__ indptr, const int64_t* __restrict__ off,
                                                          int64_t m, int64_t base) {
  const int64_t j = (int64_t)blockIdx.x * CP_WG + threadIdx.x;
  if (j <= m) indptr[j] = base + off[j];
}

void launch_csr_new_indptr(int64_t* indptr, const int64_t* off, int64_t m, int64_t base, hipStream_t st) {
  if (m < 0) return;
  hipLaunchKernelGGL(k_csr_new_indptr, dim3((unsigned)((m + 1 + CP_WG - 1) / CP_WG)), dim3(CP_WG), 0, st, indptr, off, m,
                     base);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
