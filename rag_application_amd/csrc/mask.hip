// Row masks of the pre-filtered hybrid query (hx.h: hx_hybrid_query_*_masked).
//
// A mask is ceil(n / 32) uint32 words, bit r & 31 of word r >> 5 (LSB first) = local row r; bits at or past n are
// ignored.  The whole-collection dense scans of a masked query run unchanged on gathered copies of the kept rows (a
// "view": view row i = local row rows[i]); the sparse stage tests the mask itself (sparse2.hip, sprescore.hip).
//   k_mask_count / k_mask_offsets / k_mask_rows   mask -> ascending list of kept rows + its count (two passes over
//                                                  the words: per-workgroup popcounts, their exclusive prefix in one
//                                                  workgroup, then every word writes its rows at its offset);
//   k_gather_rows16 / k_gather_u32                 the kept rows of one scanned copy (16-byte loads and stores) or of
//                                                  one per-row scale;
//   k_view_ids                                     candidate keys of a scan of the view -> keys of the index's rows.
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int MASK_WG = 256;   // words per workgroup of k_mask_count / k_mask_rows

__device__ __forceinline__ uint32_t mask_word(const uint32_t* mask, int64_t w, int64_t nw, int64_t n) {
  if (w >= nw) return 0u;
  uint32_t m = mask[w];
  const int tail = (int)(n & 31);
  if (w == nw - 1 && tail) m &= (1u << tail) - 1u;   // bits at or past n are ignored
  return m;
}

// exclusive prefix of v over a 256-thread workgroup; *total = the workgroup's sum
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[MASK_WG / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  uint32_t x = v;
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, WAVE);
    if (lane >= o) x += y;
  }
  if (lane == WAVE - 1) wsum[wv] = x;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int i = 0; i < MASK_WG / WAVE; ++i) {
    off += i < wv ? wsum[i] : 0u;
    tot += wsum[i];
  }
  __syncthreads();                   // wsum is read by every thread before a next call writes it
  *total = tot;
  return off + x - v;
}

__global__ void __launch_bounds__(MASK_WG) k_mask_count(const uint32_t* __restrict__ mask, int64_t nw, int64_t n,
                                                        uint32_t* __restrict__ blk) {
  const int64_t w = (int64_t)blockIdx.x * MASK_WG + threadIdx.x;
  uint32_t tot;
  (void)wg_exclusive_scan((uint32_t)__popc(mask_word(mask, w, nw, n)), &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// one workgroup: blk[0, nb) -> its exclusive prefix, in place; *count = the sum
__global__ void __launch_bounds__(MASK_WG) k_mask_offsets(uint32_t* __restrict__ blk, int64_t nb,
                                                          uint32_t* __restrict__ count) {
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += MASK_WG) {
    const int64_t b = b0 + threadIdx.x;
    const uint32_t v = b < nb ? blk[b] : 0u;
    uint32_t tot;
    const uint32_t ex = wg_exclusive_scan(v, &tot);
    if (b < nb) blk[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ void __launch_bounds__(MASK_WG) k_mask_rows(const uint32_t* __restrict__ mask, int64_t nw, int64_t n,
                                                       const uint32_t* __restrict__ blk, uint32_t* __restrict__ rows) {
  const int64_t w = (int64_t)blockIdx.x * MASK_WG + threadIdx.x;
  uint32_t m = mask_word(mask, w, nw, n);
  uint32_t tot;
  uint32_t o = blk[blockIdx.x] + wg_exclusive_scan((uint32_t)__popc(m), &tot);
  while (m) {
    const int b = __ffs(m) - 1;
    rows[o++] = (uint32_t)(w * 32 + b);
    m &= m - 1u;
  }
}

void launch_mask_rows(const uint32_t* mask, int64_t n, uint32_t* blk, uint32_t* rows, uint32_t* count, hipStream_t st) {
  const int64_t nw = (n + 31) / 32;
  const int64_t nb = std::max<int64_t>((nw + MASK_WG - 1) / MASK_WG, 1);
  hipLaunchKernelGGL(k_mask_count, dim3((unsigned)nb), dim3(MASK_WG), 0, st, mask, nw, n, blk);
  HX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mask_offsets, dim3(1), dim3(MASK_WG), 0, st, blk, nb, count);
  HX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)nb), dim3(MASK_WG), 0, st, mask, nw, n, blk, rows);
  HX_HIP(hipGetLastError());
}

static unsigned gather_grid(int64_t elems) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>((elems + 255) / 256, 1), 1 << 16);
}

// dst row i = src row rows[i], vpr 16-byte vectors per row
__global__ void __launch_bounds__(256) k_gather_rows16(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                       const uint32_t* __restrict__ rows, int64_t count, int vpr) {
  const int64_t total = count * vpr;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / vpr;
    const int64_t c = e - i * vpr;
    dst[e] = src[(int64_t)rows[i] * vpr + c];
  }
}

void launch_gather_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                          hipStream_t st) {
  if (count <= 0) return;
  HX_CHECK(row_bytes % 16 == 0, "gather: row bytes must be a multiple of 16");
  const int vpr = (int)(row_bytes / 16);
  hipLaunchKernelGGL(k_gather_rows16, dim3(gather_grid(count * vpr)), dim3(256), 0, st, (const uint4*)src, (uint4*)dst,
                     rows, count, vpr);
  HX_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(256) k_gather_u32(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                    const uint32_t* __restrict__ rows, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = src[rows[i]];
}

void launch_gather_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_gather_u32, dim3(gather_grid(count)), dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst,
                     rows, count);
  HX_HIP(hipGetLastError());
}

// key of internal id id_base + v (v a view row) -> key of internal id id_base + rows[v]; the score bits are kept, empty slots stay empty
__global__ void __launch_bounds__(256) k_view_ids(uint64_t* __restrict__ keys, int64_t n, const uint32_t* __restrict__ rows,
                                                  uint32_t count, uint32_t id_base) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  if (k == 0ull) return;
  const uint32_t v = key_id(k) - id_base;   // (a key below id_base wraps past count: emptied)
  keys[i] = v < count ? (k & 0xFFFFFFFF00000000ull) | (uint64_t)(0xFFFFFFFFu - (id_base + rows[v])) : 0ull;
}

void launch_view_ids(uint64_t* keys, int64_t n, const uint32_t* rows, uint32_t count, uint32_t id_base, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_view_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, n, rows, count, id_base);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
