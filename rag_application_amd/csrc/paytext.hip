// Payload index, `match text` (hx.h: HX_PAY_TEXT_ALL): which rows of a text column hold every
// pattern of a set as a byte substring.
//
// A text column is stored as a list column is (section 17): a head plane (missing, null or the row's byte length), int64
// offsets counting 32-bit words, and one word plane holding the rows' bytes, each row padded with zero bytes to a word.
//
//   k_payload_text   the 256 rows of a wave's pass own one contiguous word run [S, E) (both uniform).  The wave walks it
//                    1 KB at a time: every lane loads 16 bytes (one dwordx4, three steps ahead of the one it tests), the
//                    step and the first 64 bytes of the next one (the halo a match may reach into) are staged in the
//                    wave's LDS.  Per pattern -- a loop that is uniform over the wave -- a lane tests its 16 start
//                    positions with one masked 32-bit compare of the pattern's first bytes, and compares the rest only
//                    behind it.  A match at word w, byte b belongs to the row whose words hold w (a lower bound over the
//                    256 row starts in LDS), and only when it ends within that row's byte length: padding and the next
//                    row are not text.  The lane ORs the pattern's bit into the row's "found" word in LDS; at the end of
//                    the pass a row's verdict is found == all patterns, balloted and written by lane 0 as the mask
//                    kernel writes its words.  No lane loops over its own row: one long row costs its wave length / 1 KB
//                    steps and holds nobody else.
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int PT_WG = 256;
constexpr int PT_WAVES = PT_WG / WAVE;
constexpr int PT_U = 4;                        // row groups (of 64 rows) per wave and pass, as PAY_U
constexpr int PT_ROWS = PT_U * WAVE;
constexpr uint32_t PT_STEP = WAVE * 4;         // words per step: 16 bytes per lane
constexpr int PT_HALO = 16;                    // words of the next step a match may reach into (64 bytes >= the longest pattern - 1)
constexpr unsigned PT_GRID_MAX = 2048;
constexpr uint32_t PT_NULL = 0xFFFFFFFEu;      // heads from here on say "null" / "missing"

struct PtWave {                                // one wave's LDS: 4160 bytes
  uint4 text[WAVE + PT_HALO / 4];              // the step's 256 words and the halo's 16
  uint32_t start[PT_ROWS];                     // first word of every row of the pass (rows past n: E)
  uint32_t blen[PT_ROWS];                      // their heads
  uint32_t found[PT_ROWS];                     // bit p = pattern p occurs in the row
};

// LDS written by some lanes of the wave is read by others: keep the compiler from moving accesses across
__device__ __forceinline__ void pt_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the 4 bytes that start `sh` / 8 bytes into lo (little-endian words lo, hi)
__device__ __forceinline__ uint32_t pt_window(uint32_t lo, uint32_t hi, uint32_t sh) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh);
}

__global__ void __launch_bounds__(PT_WG) k_payload_text(const uint32_t* __restrict__ head, const int64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ text, int64_t n,
                                                        const PayTextPat* __restrict__ pats, int n_pats,
                                                        uint32_t* __restrict__ plane) {
  __shared__ PtWave lds[PT_WAVES];
  PtWave& L = lds[threadIdx.x / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * PT_WAVES + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * PT_WAVES;
  const int64_t nw = (n + 31) >> 5;
  const uint32_t full = n_pats >= 32 ? 0xFFFFFFFFu : (1u << n_pats) - 1u;
  for (int64_t g0 = wave * PT_U; g0 * WAVE < n; g0 += n_waves * PT_U) {
    const int64_t r0 = (int64_t)__builtin_amdgcn_readfirstlane((int)g0) * WAVE;
    const int nrows = (int)std::min<int64_t>(PT_ROWS, n - r0);
    // (a column holds fewer than 2^31 words: word offsets fit 32 bits)
    const uint32_t S = (uint32_t)off[r0], E = (uint32_t)off[r0 + nrows];
#pragma unroll
    for (int u = 0; u < PT_U; ++u) {
      const int r = u * WAVE + lane;
      const bool in = r < nrows;
      L.start[r] = in ? (uint32_t)off[r0 + r] : E;
      L.blen[r] = in ? head[r0 + r] : 0xFFFFFFFFu;
      L.found[r] = 0u;
    }
    pt_wave_sync();
    if (S < E) {
      // the walk starts at a multiple of four words, so every load is 16-byte aligned; the words in front of S belong to
      // rows of another pass and are refused by the row test below.  No load reaches a word at or past E rounded up to
      // four: a lane past the end reads the run's first words again (an unconditional load keeps the wait counts exact)
      // and zeroes them.
      const uint32_t A = S & ~3u;
      auto load = [&](uint32_t base) -> uint4 {
        const uint32_t a = base + (uint32_t)lane * 4u;
        const bool ok = a < E;
        const uint4 v = *(const uint4*)(text + (ok ? a : A));
        return ok ? v : make_uint4(0u, 0u, 0u, 0u);
      };
      // one step: `cur` = the lane's 16 bytes at word base + 4 lane, `nxt` = the same of the following step (the halo)
      auto step = [&](const uint4& cur, const uint4& nxt, uint32_t base) {
        pt_wave_sync();                              // (the previous step's reads are done)
        L.text[lane] = cur;
        if (lane < PT_HALO / 4) L.text[WAVE + lane] = nxt;
        pt_wave_sync();
        const uint32_t* tw = (const uint32_t*)L.text + lane * 4;
        const uint32_t w[5] = {cur.x, cur.y, cur.z, cur.w, tw[4]};
        uint32_t win[16];                            // the 4 bytes at each of the lane's 16 start positions
#pragma unroll
        for (int j = 0; j < 16; ++j) win[j] = pt_window(w[j >> 2], w[(j >> 2) + 1], (uint32_t)(j & 3) * 8u);
        for (int p = 0; p < n_pats; ++p) {           // (uniform: scalar loads of the pattern)
          const uint32_t plen = pats[p].len, fm = pats[p].fmask, f0 = pats[p].w[0];
          uint32_t hm = 0u;
#pragma unroll
          for (int j = 0; j < 16; ++j) hm |= (((win[j] ^ f0) & fm) == 0u ? 1u : 0u) << j;
          while (hm) {                               // rare: the rest of the pattern, then the row
            const uint32_t j = (uint32_t)__ffs((int)hm) - 1u;
            hm &= hm - 1u;
            const uint32_t jw = j >> 2, sh = (j & 3u) * 8u;
            bool eq = true;
            for (uint32_t k = 1; k * 4u < plen; ++k) {
              const uint32_t rem = plen - k * 4u;
              const uint32_t m = rem >= 4u ? 0xFFFFFFFFu : (1u << (rem * 8u)) - 1u;
              eq &= ((pt_window(tw[jw + k], tw[jw + k + 1], sh) ^ pats[p].w[k]) & m) == 0u;
            }
            if (!eq) continue;
            const uint32_t wi = base + (uint32_t)lane * 4u + jw;
            int i = 0;                                // the last row that starts at or before the word
#pragma unroll
            for (int s = PT_ROWS / 2; s > 0; s >>= 1) i += L.start[i + s] <= wi ? s : 0;
            const uint32_t rs = L.start[i], bl = L.blen[i];
            if (wi >= rs && bl < PT_NULL && (uint64_t)(wi - rs) * 4u + (j & 3u) + plen <= (uint64_t)bl)
              atomicOr(&L.found[i], 1u << p);
          }
        }
      };
      // three steps' loads in flight; the rotation is unrolled so that no register copy waits for a load
      uint4 c0 = load(A), c1 = load(A + PT_STEP), c2 = load(A + 2u * PT_STEP);
      for (uint32_t base = A; base < E;) {
        step(c0, c1, base);
        c0 = load(base + 3u * PT_STEP);
        if ((base += PT_STEP) >= E) break;
        step(c1, c2, base);
        c1 = load(base + 3u * PT_STEP);
        if ((base += PT_STEP) >= E) break;
        step(c2, c0, base);
        c2 = load(base + 3u * PT_STEP);
        base += PT_STEP;
      }
    }
    pt_wave_sync();
#pragma unroll
    for (int u = 0; u < PT_U; ++u) {
      const int r = u * WAVE + lane;
      const unsigned long long v = __ballot(r < nrows && L.blen[r] < PT_NULL && L.found[r] == full);
      const int64_t wd = (g0 + u) * 2;
      if (lane == 0) {
        if (wd < nw) plane[wd] = (uint32_t)v;
        if (wd + 1 < nw) plane[wd + 1] = (uint32_t)(v >> 32);
      }
    }
    pt_wave_sync();                                   // (the next pass overwrites the rows' LDS)
  }
}

void launch_payload_text(const uint32_t* head, const int64_t* off, const uint32_t* text, int64_t n, const PayTextPat* pats,
                         int n_pats, uint32_t* plane, int grid_cap, hipStream_t st) {
  if (n <= 0) return;
  const int64_t rows_per_wg = (int64_t)PT_WG * PT_U;
  unsigned grid = (unsigned)std::min<int64_t>((n + rows_per_wg - 1) / rows_per_wg, PT_GRID_MAX);
  if (grid_cap > 0) grid = std::min(grid, (unsigned)grid_cap);
  hipLaunchKernelGGL(k_payload_text, dim3(grid), dim3(PT_WG), 0, st, head, off, text, n, pats, n_pats, plane);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
