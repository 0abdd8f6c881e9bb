// Payload index (hx.h: hx_payload_*): a compiled filter evaluated over every row on the device.
//
// A column is one plane of uint32 per row (HX_PAY_U32: the cell) or two (HX_PAY_F64: the low and the high word of the
// double).  "Missing" and "null" are the codes 0xFFFFFFFF / 0xFFFFFFFE; an F64 cell says the same with two fixed NaN
// patterns whose low words are those codes and whose high word is 0x7FF80000, so one test serves both kinds (a U32
// column reads as if its high word were 0x7FF80000).  A stored number is never a NaN (the caller's encoder refuses it).
//
//   k_payload_mask   one row per lane, PAY_U rows per lane and pass (that many loads in flight per plane); the program
//                    is postfix over a per-row boolean stack held in ONE 32-bit register per row (top of stack = bit 0),
//                    read uniformly -- every lane of the grid runs the same op, no lane-dependent branch outside the
//                    binary search of a large set, whose trip count is uniform too.  A plane is loaded once per pass:
//                    consecutive ops on the same column reuse the registers.  The wave's 64 verdicts of a row group are
//                    combined with a ballot and written by lane 0 as two ordinary 4-byte stores.
//                    A list column (a head plane, int64 offsets, element planes) is matched by
//                    the ANY_* ops: the wave walks the contiguous element run of its rows in chunks of 64, one element
//                    per lane, and each row lane picks the bits of its own segment out of the chunk's ballot.
//                    PAY_D_BITS (device-only) pushes the row's bit of a packed verdict plane that
//                    another kernel wrote in front of this one: how HX_PAY_TEXT_ALL (paytext.hip) joins a program.
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int PAY_WG = 256;
constexpr int PAY_U = 4;                  // row groups (of 64 rows) per wave and pass
constexpr unsigned PAY_GRID_MAX = 2048;   // 8 workgroups per CU
constexpr uint32_t PAY_NAN_HI = 0x7FF80000u;

__device__ __forceinline__ double pay_f64(uint32_t lo, uint32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// membership of v in the ascending set s[0, cnt): compared one by one up to PAY_INLINE_SET entries (uniform reads), a
// branch-free lower bound above (cnt is uniform, so is the trip count; the set stays in L2)
template <typename T>
__device__ __forceinline__ bool pay_in_set(const T* __restrict__ s, uint32_t cnt, T v) {
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

// bits [0, k) of a ballot, k in [0, 64]
__device__ __forceinline__ unsigned long long pay_low_bits(uint32_t k) {
  return k >= 64u ? ~0ull : (1ull << k) - 1ull;
}

__global__ void __launch_bounds__(PAY_WG) k_payload_mask(const PayOpDev* __restrict__ prog, int n_ops, int64_t n,
                                                         uint32_t* __restrict__ mask, uint32_t* __restrict__ kept) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * (PAY_WG / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (PAY_WG / WAVE);
  const int64_t nw = (n + 31) >> 5;
  uint32_t total = 0;
  for (int64_t g0 = wave * PAY_U; g0 * WAVE < n; g0 += n_waves * PAY_U) {
    uint32_t stack[PAY_U], lo[PAY_U], hi[PAY_U];
    int64_t row[PAY_U];
    bool in[PAY_U];
#pragma unroll
    for (int u = 0; u < PAY_U; ++u) {
      row[u] = (g0 + u) * WAVE + lane;
      in[u] = row[u] < n;
      stack[u] = 0u;
      lo[u] = 0xFFFFFFFFu;
      hi[u] = PAY_NAN_HI;
    }
    const uint32_t* have = nullptr;       // the plane in lo / hi
    for (int i = 0; i < n_ops; ++i) {
      const PayOpDev op = prog[i];        // (uniform: scalar loads)
      const uint32_t code = op.op;
      if (code >= PAY_D_FIRST_COL && op.p0 != have) {
        have = op.p0;
#pragma unroll
        for (int u = 0; u < PAY_U; ++u) {
          lo[u] = in[u] ? op.p0[row[u]] : 0xFFFFFFFFu;
          hi[u] = (op.p1 && in[u]) ? op.p1[row[u]] : PAY_NAN_HI;
        }
      }
      // A list op: the rows of the pass own ONE contiguous element run [S, E) of the column (both
      // offsets are uniform: scalar loads).  The wave walks it 64 elements at a time -- lane j tests element base + j,
      // the 64 verdicts are balloted -- and every row lane ORs the bits of its own segment [rs, re) (relative to S; the
      // engine keeps a column below 2^31 elements) into its verdict.  The trip count is the wave's, not the lane's: a
      // long row costs the wave its length / 64 steps, nothing waits for one lane.  Rows at or past n own no element.
      uint32_t lhit = 0u;                 // bit u = the verdict of row group u
      if (code >= PAY_D_FIRST_LIST) {
        const int64_t r0 = (int64_t)__builtin_amdgcn_readfirstlane((int)g0) * WAVE;
        const int64_t S = op.off[r0], E = op.off[std::min<int64_t>(r0 + PAY_U * WAVE, n)];
        uint32_t rs[PAY_U], re[PAY_U];
#pragma unroll
        for (int u = 0; u < PAY_U; ++u) {
          rs[u] = in[u] ? (uint32_t)(op.off[row[u]] - S) : 0u;
          re[u] = in[u] ? (uint32_t)(op.off[row[u] + 1] - S) : 0u;
        }
        if (code == PAY_D_IS_EMPTY_LIST) {
#pragma unroll
          for (int u = 0; u < PAY_U; ++u) lhit |= (lo[u] == 0u && rs[u] == re[u] ? 1u : 0u) << u;
        } else {
          const double c = __longlong_as_double((long long)op.imm), c2 = __longlong_as_double((long long)op.imm2);
          for (int64_t base = S; base < E; base += WAVE) {
            const int64_t e = base + lane;
            const bool ok = e < E;
            const uint32_t vl = ok ? op.e0[e] : 0u;
            const uint32_t vh = (ok && op.e1) ? op.e1[e] : 0u;
            const double x = pay_f64(vl, vh);
            bool p = false;
            switch (code) {
              case PAY_D_ANY_EQ_U32: p = vl == (uint32_t)op.imm; break;
              case PAY_D_ANY_IN_U32: p = pay_in_set<uint32_t>((const uint32_t*)op.imm, op.cnt, vl); break;
              case PAY_D_ANY_EQ_F64: p = x == c; break;
              case PAY_D_ANY_IN_F64: p = pay_in_set<double>((const double*)op.imm, op.cnt, x); break;
              case PAY_D_ANY_RANGE: p = c <= x && x <= c2; break;
              default: break;
            }
            const unsigned long long hits = __ballot(ok && p);
            const uint32_t rel = (uint32_t)(base - S);
#pragma unroll
            for (int u = 0; u < PAY_U; ++u) {
              const uint32_t a = rs[u] > rel ? std::min(rs[u] - rel, (uint32_t)WAVE) : 0u;
              const uint32_t b = re[u] > rel ? std::min(re[u] - rel, (uint32_t)WAVE) : 0u;
              lhit |= ((hits & pay_low_bits(b) & ~pay_low_bits(a)) != 0ull ? 1u : 0u) << u;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PAY_U; ++u) {
        const bool missing = hi[u] == PAY_NAN_HI && lo[u] == 0xFFFFFFFFu;
        const bool null = hi[u] == PAY_NAN_HI && lo[u] == 0xFFFFFFFEu;
        const double x = pay_f64(lo[u], hi[u]), c = __longlong_as_double((long long)op.imm);
        uint32_t s = stack[u];
        bool b = false;
        switch (code) {
          case PAY_D_AND: { const uint32_t t = s & 1u; s >>= 1; s &= (t | ~1u); stack[u] = s; continue; }
          case PAY_D_OR:  { const uint32_t t = s & 1u; s >>= 1; s |= t; stack[u] = s; continue; }
          case PAY_D_NOT: stack[u] = s ^ 1u; continue;
          case PAY_D_TRUE: b = true; break;
          case PAY_D_FALSE: b = false; break;
          case PAY_D_ROW_IN: b = pay_in_set<uint32_t>((const uint32_t*)op.imm, op.cnt, (uint32_t)row[u]); break;
          case PAY_D_BITS: b = in[u] && ((((const uint32_t*)op.imm)[row[u] >> 5] >> (row[u] & 31)) & 1u); break;
          case PAY_D_IS_MISSING: b = missing; break;
          case PAY_D_IS_NULL: b = null; break;
          case PAY_D_PRESENT: b = !(missing || null); break;
          case PAY_D_EQ_U32: b = lo[u] == (uint32_t)op.imm && !(missing || null); break;
          case PAY_D_IN_U32: b = !(missing || null) && pay_in_set<uint32_t>((const uint32_t*)op.imm, op.cnt, lo[u]); break;
          case PAY_D_EQ_F64: b = x == c; break;           // (IEEE: a missing or null cell is a NaN, never equal or ordered)
          case PAY_D_IN_F64: b = pay_in_set<double>((const double*)op.imm, op.cnt, x); break;
          case PAY_D_LT: b = x < c; break;
          case PAY_D_LE: b = x <= c; break;
          case PAY_D_GT: b = x > c; break;
          case PAY_D_GE: b = x >= c; break;
          case PAY_D_IS_EMPTY_LIST: case PAY_D_ANY_EQ_U32: case PAY_D_ANY_IN_U32: case PAY_D_ANY_EQ_F64:
          case PAY_D_ANY_IN_F64: case PAY_D_ANY_RANGE: b = (lhit >> u) & 1u; break;
          default: break;
        }
        stack[u] = (s << 1) | (b ? 1u : 0u);
      }
    }
#pragma unroll
    for (int u = 0; u < PAY_U; ++u) {
      const unsigned long long v = __ballot(in[u] && (stack[u] & 1u));
      const int64_t w = (g0 + u) * 2;
      if (lane == 0) {
        if (w < nw) mask[w] = (uint32_t)v;
        if (w + 1 < nw) mask[w + 1] = (uint32_t)(v >> 32);
      }
      total += (uint32_t)__popcll(v);
    }
  }
  if (kept && lane == 0 && total) atomicAdd(kept, total);
}

void launch_payload_mask(const PayOpDev* prog, int n_ops, int64_t n, uint32_t* mask, uint32_t* kept, int grid_cap,
                         hipStream_t st) {
  if (n <= 0) return;
  const int64_t rows_per_wg = (int64_t)PAY_WG * PAY_U;
  unsigned grid = (unsigned)std::min<int64_t>((n + rows_per_wg - 1) / rows_per_wg, PAY_GRID_MAX);
  if (grid_cap > 0) grid = std::min(grid, (unsigned)grid_cap);
  hipLaunchKernelGGL(k_payload_mask, dim3(grid), dim3(PAY_WG), 0, st, prog, n_ops, n, mask, kept);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
