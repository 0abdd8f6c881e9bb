// Payload index, nested blocks (hx.h: HX_PAY_NESTED): which rows hold ONE object that meets a whole
// conjunction of conditions on its fields.
//
// An array of objects is stored as one list column (section 17) per indexed field, each holding ONE element per object: the
// columns of one parent are element-aligned -- equal heads and offsets -- so position e of every column speaks of the same
// object.  A block's element program is postfix over a per-ELEMENT boolean stack.
//
//   k_payload_nested   the 256 rows of a wave's pass own one contiguous element run [S, E) of the anchor's offsets (both
//                      uniform: scalar loads).  The wave walks it 64 positions at a time, one position per lane: the lane
//                      loads the planes of the block's distinct columns once (at most 8 columns, 16 words; the table of
//                      their pointers sits in device memory beside the program), then runs the
//                      element program on ONE 32-bit stack register (top of stack = bit 0).  The program is read
//                      uniformly -- every lane runs the same op, a column slot picks its registers with uniform selects, no
//                      lane-dependent branch outside the binary search of a large set, whose trip count is uniform too.
//                      The 64 verdicts are balloted and every row lane ORs the bits of its own segment, as the list ops of
//                      k_payload_mask do.  The trip count is the wave's, never a lane's.  A row's verdict is balloted and
//                      written by lane 0 as the mask kernel writes its words: a packed plane for PAY_D_BITS.
//   k_payload_same_offsets   heads and offsets of two list columns compared entry by entry (hx_payload_same_offsets).
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int PN_WG = 256;
constexpr int PN_U = 4;                   // row groups (of 64 rows) per wave and pass, as PAY_U
constexpr unsigned PN_GRID_MAX = 2048;

__device__ __forceinline__ double pn_f64(uint32_t lo, uint32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// pay_in_set of payload.hip
template <typename T>
__device__ __forceinline__ bool pn_in_set(const T* __restrict__ s, uint32_t cnt, T v) {
  if (cnt <= (uint32_t)PAY_INLINE_SET) {
    bool hit = false;
    for (uint32_t i = 0; i < cnt; ++i) hit |= (s[i] == v);
    return hit;
  }
  const T* b = s;
  for (uint32_t len = cnt; len > 1;) {
    const uint32_t half = len >> 1;
    b = (b[half - 1] < v) ? b + half : b;
    len -= half;
  }
  return *b == v;
}

__device__ __forceinline__ unsigned long long pn_low_bits(uint32_t k) {
  return k >= 64u ? ~0ull : (1ull << k) - 1ull;
}

__global__ void __launch_bounds__(PN_WG) k_payload_nested(const int64_t* __restrict__ off, int64_t n,
                                                          const PayNestedCols* __restrict__ cols,
                                                          const PayElOpDev* __restrict__ prog, int n_ops,
                                                          uint32_t* __restrict__ plane) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * (PN_WG / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (PN_WG / WAVE);
  const int64_t nw = (n + 31) >> 5;
  for (int64_t g0 = wave * PN_U; g0 * WAVE < n; g0 += n_waves * PN_U) {
    const int64_t r0 = (int64_t)__builtin_amdgcn_readfirstlane((int)g0) * WAVE;
    const int64_t S = off[r0], E = off[std::min<int64_t>(r0 + PN_U * WAVE, n)];
    uint32_t rs[PN_U], re[PN_U];          // the rows' segments relative to S (a column holds fewer than 2^31 elements)
#pragma unroll
    for (int u = 0; u < PN_U; ++u) {
      const int64_t row = r0 + u * WAVE + lane;
      const bool in = row < n;
      rs[u] = in ? (uint32_t)(off[row] - S) : 0u;
      re[u] = in ? (uint32_t)(off[row + 1] - S) : 0u;
    }
    uint32_t hit = 0u;                    // bit u = the verdict of the lane's row of group u
    for (int64_t base = S; base < E; base += WAVE) {
      const int64_t e = base + lane;
      const bool ok = e < E;
      uint32_t lo[PAY_NESTED_COLS], hi[PAY_NESTED_COLS];
      // the column table is read again for every chunk (scalar loads that hit the scalar cache): sixteen plane pointers
      // held across the walk would cost more scalar registers than a wave has to spare
      const PayNestedCols* ct = cols;
      asm volatile("" : "+s"(ct));
      const int n_cols = ct->n_cols;
#pragma unroll
      for (int k = 0; k < PAY_NESTED_COLS; ++k) {
        lo[k] = hi[k] = 0u;
        if (k < n_cols) {                 // (uniform)
          const uint32_t* p0 = ct->e0[k];
          const uint32_t* p1 = ct->e1[k];
          lo[k] = ok ? p0[e] : 0u;
          hi[k] = (ok && p1) ? p1[e] : 0u;
        }
      }
      uint32_t s = 0u;
      for (int i = 0; i < n_ops; ++i) {
        const PayElOpDev op = prog[i];    // (uniform: scalar loads)
        uint32_t vl = lo[0], vh = hi[0];
#pragma unroll
        for (int k = 1; k < PAY_NESTED_COLS; ++k) {
          vl = op.slot == (uint32_t)k ? lo[k] : vl;
          vh = op.slot == (uint32_t)k ? hi[k] : vh;
        }
        const double x = pn_f64(vl, vh);
        const double c = __longlong_as_double((long long)op.imm), c2 = __longlong_as_double((long long)op.imm2);
        bool b = false;
        switch (op.op) {
          case PAY_E_AND: { const uint32_t t = s & 1u; s >>= 1; s &= (t | ~1u); continue; }
          case PAY_E_OR:  { const uint32_t t = s & 1u; s >>= 1; s |= t; continue; }
          case PAY_E_NOT: s ^= 1u; continue;
          case PAY_E_TRUE: b = true; break;
          case PAY_E_FALSE: b = false; break;
          case PAY_E_EQ_U32: b = vl == (uint32_t)op.imm; break;
          case PAY_E_IN_U32: b = pn_in_set<uint32_t>((const uint32_t*)op.imm, op.cnt, vl); break;
          case PAY_E_EQ_F64: b = x == c; break;
          case PAY_E_IN_F64: b = pn_in_set<double>((const double*)op.imm, op.cnt, x); break;
          case PAY_E_RANGE: b = c <= x && x <= c2; break;
          default: break;
        }
        s = (s << 1) | (b ? 1u : 0u);
      }
      const unsigned long long hits = __ballot(ok && (s & 1u));
      const uint32_t rel = (uint32_t)(base - S);
#pragma unroll
      for (int u = 0; u < PN_U; ++u) {
        const uint32_t a = rs[u] > rel ? std::min(rs[u] - rel, (uint32_t)WAVE) : 0u;
        const uint32_t b = re[u] > rel ? std::min(re[u] - rel, (uint32_t)WAVE) : 0u;
        hit |= ((hits & pn_low_bits(b) & ~pn_low_bits(a)) != 0ull ? 1u : 0u) << u;
      }
    }
#pragma unroll
    for (int u = 0; u < PN_U; ++u) {
      const unsigned long long v = __ballot((hit >> u) & 1u);      // (a row at or past n owns no position)
      const int64_t w = (g0 + u) * 2;
      if (lane == 0) {
        if (w < nw) plane[w] = (uint32_t)v;
        if (w + 1 < nw) plane[w + 1] = (uint32_t)(v >> 32);
      }
    }
  }
}

void launch_payload_nested(const int64_t* off, int64_t n, const PayNestedCols* cols, const PayElOpDev* prog, int n_ops,
                           uint32_t* plane, int grid_cap, hipStream_t st) {
  if (n <= 0) return;
  const int64_t rows_per_wg = (int64_t)PN_WG * PN_U;
  unsigned grid = (unsigned)std::min<int64_t>((n + rows_per_wg - 1) / rows_per_wg, PN_GRID_MAX);
  if (grid_cap > 0) grid = std::min(grid, (unsigned)grid_cap);
  hipLaunchKernelGGL(k_payload_nested, dim3(grid), dim3(PN_WG), 0, st, off, n, cols, prog, n_ops, plane);
  HX_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(256) k_payload_same_offsets(const uint32_t* __restrict__ head_a,
                                                              const uint32_t* __restrict__ head_b,
                                                              const int64_t* __restrict__ off_a,
                                                              const int64_t* __restrict__ off_b, int64_t n,
                                                              uint32_t* __restrict__ same) {
  bool diff = false;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x) {
    diff |= off_a[r] != off_b[r];
    if (r < n) diff |= head_a[r] != head_b[r];
  }
  if (diff) *same = 0u;                   // (every writer stores the same word)
}

void launch_payload_same_offsets(const uint32_t* head_a, const uint32_t* head_b, const int64_t* off_a, const int64_t* off_b,
                                 int64_t n, uint32_t* same, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<int64_t>((n + 1 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_payload_same_offsets, dim3(grid), dim3(256), 0, st, head_a, head_b, off_a, off_b, n, same);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
