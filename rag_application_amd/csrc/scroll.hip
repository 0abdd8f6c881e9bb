// Scroll (hx_scroll_rows / hx_payload_order): a page of the rows a mask keeps, in row order or in
// the order of an F64 payload column.
//
// The ordered page is a radix select over the order key s of hx.h (64 bits: smallest (s, row) first in both directions),
// then a sort of the at most 2048 chosen rows.  Its cost depends neither on the order of the data nor on how many rows
// share a value: every pass reads the column once, whatever it holds.
//
//   k_order_init    zeroes the six histograms and sets the state block: need = limit, no digit chosen.
//   k_order_hist    one digit per pass, 11 / 11 / 10 bits over the high word and again over the low word.  A lane reads four
//                   consecutive rows with one 16-byte load per plane (and one mask word), tests eligibility and the digits
//                   chosen so far, and counts the digit into a 2048-bin histogram of its workgroup in LDS; the workgroup
//                   ends with one global integer atomic per non-zero bin.  The first three passes read the high-word plane
//                   only: a lane fetches a row's low word just where the high word does not decide -- the sentinels'
//                   high word, -0.0's, and the high word of start_from / after_value.  A wave step whose counted rows all
//                   fall into one bin (timestamps in an early pass) is one LDS add.  A wave holds two steps in flight.
//   k_order_pick    one wave: the bin holding the need-th matching row; extends the prefix, lowers need by the rows of
//                   the bins before it.  The first pick learns the number of eligible rows: below `limit`, all are taken.
//   k_first_count / k_first_prefix / k_first_emit
//                   "the first m rows of a predicate, in row order": a count per contiguous row slice (one workgroup
//                   each), an exclusive prefix over the slices (one workgroup), and an emit (one wave per slice) that
//                   places a row at prefix + its rank in the slice -- the rank from ballots and popcounts; a slice
//                   without such a row, or past the m-th, is not read.  The plain
//                   scroll is this with the predicate "mask bit and row >= start_row"; the ordered page uses it for its
//                   ties, "eligible and s == T", the first `need` of them.  The ordered count pass also appends the rows
//                   with s < T (fewer than `limit`) to the candidates through an atomic cursor, in any order.
//   k_order_sort    one workgroup: a bitonic sort in LDS of the chosen (s, row) pairs, then rows and stored cells out.
//
// Everything is integer: counts, prefixes and ranks do not depend on arrival order, the result is the same on every run.
#include "../../include/hx.h"
#include "hx_common.hpp"
#include "kernels.hpp"

#include <algorithm>

namespace hx {

constexpr int SCROLL_NT = 256;
constexpr int SCROLL_STEP = 4 * WAVE;           // rows of one wave step: four consecutive rows per lane
constexpr unsigned ORDER_GRID = 2048;           // eight workgroups per CU
constexpr int ORDER_SHIFT[ORDER_PASSES] = {53, 42, 32, 21, 10, 0};
constexpr int ORDER_WIDTH[ORDER_PASSES] = {11, 11, 10, 11, 11, 10};

// the order key of a cell (hx.h); false for a missing or null cell
__device__ __forceinline__ bool order_key(uint32_t hi, uint32_t lo, int desc, uint64_t& s) {
  uint64_t b = ((uint64_t)hi << 32) | lo;
  if (b == HX_PAY_F64_MISSING || b == HX_PAY_F64_NULL) return false;
  if (b == 0x8000000000000000ull) b = 0ull;                       // -0.0 + 0.0
  const uint64_t u = b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
  s = desc ? ~u : u;
  return true;
}
__device__ __forceinline__ bool order_within(const OrderArgs& a, uint64_t s, int64_t row) {
  return (!a.has_start || s >= a.s_start) && (!a.has_after || s > a.s_after || (s == a.s_after && row > a.after_row));
}

struct Rows4 {
  uint32_t hi[4], lo[4];
  uint32_t live;           // bit j: row0 + j is a row and the mask keeps it
};
// Rows row0 .. row0 + 3 (row0 a multiple of four: the planes' capacity is a multiple of 256 rows, the 16-byte loads stay
// inside them).  LOW: both planes; otherwise the low word only where the high word does not decide (see above).
// Two phases, so that a caller with several steps in flight issues every unconditional load before the first wait.
template <bool LOW>
__device__ __forceinline__ Rows4 order_load_planes(const OrderArgs& a, int64_t row0) {
  Rows4 r;
  r.live = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) r.hi[j] = r.lo[j] = 0u;
  if (row0 >= a.n) return r;
  const uint4 h = *reinterpret_cast<const uint4*>(a.hi + row0);
  r.hi[0] = h.x, r.hi[1] = h.y, r.hi[2] = h.z, r.hi[3] = h.w;
  if (LOW) {
    const uint4 l = *reinterpret_cast<const uint4*>(a.lo + row0);
    r.lo[0] = l.x, r.lo[1] = l.y, r.lo[2] = l.z, r.lo[3] = l.w;
  }
  const uint32_t word = a.mask ? a.mask[row0 >> 5] : 0xFFFFFFFFu;
  const int sh = (int)(row0 & 31);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (row0 + j < a.n && ((word >> (sh + j)) & 1u)) r.live |= 1u << j;
  return r;
}
// the high-word passes: the low word of a kept row whose high word does not decide
__device__ __forceinline__ void order_load_undecided(const OrderArgs& a, int64_t row0, Rows4& r) {
  const uint32_t start_hi = (uint32_t)(a.s_start >> 32), after_hi = (uint32_t)(a.s_after >> 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t x = r.hi[j];
    const uint32_t uhi = (x >> 31) ? ~x : (x ^ 0x80000000u);
    const uint32_t shi = a.desc ? ~uhi : uhi;
    const bool undecided = x == 0x80000000u || x == 0x7FF80000u || (a.has_start && shi == start_hi) ||
                           (a.has_after && shi == after_hi);
    if (((r.live >> j) & 1u) && undecided) r.lo[j] = a.lo[row0 + j];
  }
}
template <bool LOW>
__device__ __forceinline__ Rows4 order_load(const OrderArgs& a, int64_t row0) {
  Rows4 r = order_load_planes<LOW>(a, row0);
  if (!LOW) order_load_undecided(a, row0, r);
  return r;
}

// One wave step of a histogram pass: the digits of the step's counted rows into the workgroup's histogram.  A step whose
// counted rows all fall into one bin is ONE add (timestamps and runs in an early pass: every step).
__device__ __forceinline__ void order_count_step(const OrderArgs& a, const OrderState& st, const Rows4& r, int64_t row0,
                                                 int shift, int top, uint32_t dmask, int lane, uint32_t* hist) {
  uint32_t d[4], okm = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint64_t s = 0ull;
    const bool ok = ((r.live >> j) & 1u) && order_key(r.hi[j], r.lo[j], a.desc, s) && order_within(a, s, row0 + j) &&
                    (top >= 64 || ((s ^ st.prefix) >> top) == 0ull);
    d[j] = (uint32_t)(s >> shift) & dmask;
    okm |= ok ? 1u << j : 0u;
  }
  const unsigned long long any = __ballot(okm != 0u);
  if (!any) return;                                    // (wave-uniform)
  const int first = __ffsll(any) - 1;
  const uint32_t mine = (okm & 1u) ? d[0] : (okm & 2u) ? d[1] : (okm & 4u) ? d[2] : d[3];
  const uint32_t d0 = (uint32_t)__shfl((int)mine, first, 64);
  bool other = false;
  uint32_t total = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    other |= ((okm >> j) & 1u) && d[j] != d0;
    total += (uint32_t)__popcll(__ballot((okm >> j) & 1u));
  }
  if (__ballot(other) == 0ull) {
    if (lane == first) atomicAdd(&hist[d0], total);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((okm >> j) & 1u) atomicAdd(&hist[d[j]], 1u);
  }
}

__global__ void __launch_bounds__(1024) k_order_init(OrderArgs a) {
  for (int i = threadIdx.x; i < ORDER_PASSES * ORDER_BINS; i += 1024) a.hist[i] = 0u;
  if (threadIdx.x == 0) {
    OrderState s;
    s.prefix = 0ull;
    s.need = (uint32_t)a.limit;
    s.all = s.total = s.n_less = 0u;
    *a.st = s;
  }
}

template <bool LOW>
__global__ void __launch_bounds__(SCROLL_NT) k_order_hist(OrderArgs a, int pass, int shift, int width) {
  __shared__ uint32_t hist[ORDER_BINS];
  const OrderState st = *a.st;
  if (st.all) return;
  for (int i = threadIdx.x; i < ORDER_BINS; i += SCROLL_NT) hist[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int top = shift + width;                       // the bits from here up are chosen
  const uint32_t dmask = (1u << width) - 1u;
  const int64_t wave = (int64_t)blockIdx.x * (SCROLL_NT / WAVE) + threadIdx.x / WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (SCROLL_NT / WAVE);
  // two steps in flight per wave: with one, the pass waits for a load's latency, not for the memory's rate
  for (int64_t base = wave * (2 * SCROLL_STEP); base < a.n; base += n_waves * (2 * SCROLL_STEP)) {
    const int64_t row0 = base + lane * 4, row1 = row0 + SCROLL_STEP;
    Rows4 r0 = order_load_planes<LOW>(a, row0);
    Rows4 r1 = order_load_planes<LOW>(a, row1);
    if (!LOW) {
      order_load_undecided(a, row0, r0);
      order_load_undecided(a, row1, r1);
    }
    order_count_step(a, st, r0, row0, shift, top, dmask, lane, hist);
    order_count_step(a, st, r1, row1, shift, top, dmask, lane, hist);
  }
  __syncthreads();
  uint32_t* out = a.hist + pass * ORDER_BINS;
  for (int i = threadIdx.x; i < ORDER_BINS; i += SCROLL_NT) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(&out[i], v);
  }
}

__global__ void __launch_bounds__(WAVE) k_order_pick(OrderArgs a, int pass, int shift) {
  OrderState* st = a.st;
  const uint32_t need = st->need;
  if (st->all) return;
  const int lane = threadIdx.x;
  constexpr int PER = ORDER_BINS / WAVE;
  const uint32_t* h = a.hist + pass * ORDER_BINS + lane * PER;
  uint32_t sum = 0u;
  for (int i = 0; i < PER; ++i) sum += h[i];
  uint32_t inc = sum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, off, 64);
    if (lane >= off) inc += t;
  }
  const uint32_t total = (uint32_t)__shfl((int)inc, WAVE - 1, 64);
  if (pass == 0) {
    if (lane == 0) st->total = total;
    if (total < need) {                                // every eligible row is taken
      if (lane == 0) st->all = 1u;
      return;
    }
  }
  const uint32_t before = inc - sum;
  if (before < need && need <= inc) {                  // one lane: its bins hold the need-th row
    uint32_t cum = before;
    for (int i = 0; i < PER; ++i) {
      const uint32_t c = h[i];
      if (cum + c >= need) {
        st->prefix |= (uint64_t)(lane * PER + i) << shift;
        st->need = need - cum;
        break;
      }
      cum += c;
    }
  }
}

// ---- the first m rows of a predicate -------------------------------------------------------------------------------------
struct FirstArgs {
  const uint32_t* mask;    // the plain scroll's mask, NULL = every row
  int64_t n, start_row;
  int64_t slice_rows;      // a multiple of 1024
  uint32_t limit;
  uint32_t* slice_cnt;
  uint32_t* slice_pre;
  uint32_t* out_rows;      // the plain scroll's outputs
  int32_t* out_count;
};

// bit j of the result: row0 + j meets the predicate.  ORDER: "eligible and s == T"; `less` = the rows that are chosen
// whatever their row (s < T, or every eligible row when all are taken), s = the keys.
template <bool ORDER>
__device__ __forceinline__ uint32_t first_pred4(const FirstArgs& f, const OrderArgs& a, const OrderState& st, int64_t row0,
                                                uint32_t& less, uint64_t (&s)[4]) {
  uint32_t hit = 0u;
  less = 0u;
  if (ORDER) {
    const Rows4 r = order_load<true>(a, row0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = 0ull;
      const bool ok = ((r.live >> j) & 1u) && order_key(r.hi[j], r.lo[j], a.desc, s[j]) && order_within(a, s[j], row0 + j);
      if (ok && (st.all || s[j] < st.prefix)) less |= 1u << j;
      if (ok && !st.all && s[j] == st.prefix) hit |= 1u << j;
    }
  } else {
    if (row0 >= f.n) return 0u;
    const uint32_t word = f.mask ? f.mask[row0 >> 5] : 0xFFFFFFFFu;
    const int sh = (int)(row0 & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (row0 + j < f.n && row0 + j >= f.start_row && ((word >> (sh + j)) & 1u)) hit |= 1u << j;
  }
  return hit;
}

// the rows of slice b that can meet the predicate: [begin, end), begin a multiple of 1024
template <bool ORDER>
__device__ __forceinline__ void first_slice(const FirstArgs& f, int64_t b, int64_t& begin, int64_t& end) {
  begin = b * f.slice_rows;
  end = std::min<int64_t>(begin + f.slice_rows, f.n);
  if (!ORDER) begin = std::max<int64_t>(begin, f.start_row / 1024 * 1024);
}

template <bool ORDER>
__global__ void __launch_bounds__(SCROLL_NT) k_first_count(FirstArgs f, OrderArgs a) {
  __shared__ uint32_t wsum[SCROLL_NT / WAVE];
  OrderState st{};
  if (ORDER) st = *a.st;
  int64_t begin, end;
  first_slice<ORDER>(f, blockIdx.x, begin, end);
  uint32_t cnt = 0u;
  for (int64_t row0 = begin + (int64_t)threadIdx.x * 4; row0 < end; row0 += SCROLL_NT * 4) {
    uint32_t less;
    uint64_t s[4];
    const uint32_t hit = first_pred4<ORDER>(f, a, st, row0, less, s);
    cnt += (uint32_t)__popc(hit);
    if (ORDER) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((less >> j) & 1u) {
          const uint32_t slot = atomicAdd(&a.st->n_less, 1u);
          if (slot < (uint32_t)HX_SCROLL_MAX_LIMIT) {
            a.cand_s[slot] = s[j];
            a.cand_row[slot] = (uint32_t)(row0 + j);
          }
        }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += (uint32_t)__shfl_down((int)cnt, off, 64);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0u;
    for (int w = 0; w < SCROLL_NT / WAVE; ++w) t += wsum[w];
    f.slice_cnt[blockIdx.x] = t;
  }
}

template <bool ORDER>
__global__ void __launch_bounds__(FIRST_MAX_SLICES) k_first_prefix(FirstArgs f, int n_slices) {
  __shared__ uint32_t sc[FIRST_MAX_SLICES];
  const int t = threadIdx.x;
  const uint32_t v = t < n_slices ? f.slice_cnt[t] : 0u;
  sc[t] = v;
  __syncthreads();
  for (int off = 1; off < FIRST_MAX_SLICES; off <<= 1) {
    const uint32_t x = t >= off ? sc[t - off] : 0u;
    __syncthreads();
    sc[t] += x;
    __syncthreads();
  }
  if (t < n_slices) f.slice_pre[t] = sc[t] - v;
  if (!ORDER) {                                        // the plain scroll ends here but for the rows themselves
    const uint32_t count = std::min(sc[FIRST_MAX_SLICES - 1], f.limit);
    if (t == 0) *f.out_count = (int32_t)count;
    for (uint32_t i = count + (uint32_t)t; i < f.limit; i += FIRST_MAX_SLICES) f.out_rows[i] = 0u;
  }
}

template <bool ORDER>
__global__ void __launch_bounds__(WAVE) k_first_emit(FirstArgs f, OrderArgs a) {
  OrderState st{};
  if (ORDER) st = *a.st;
  if (ORDER && st.all) return;
  const uint32_t m = ORDER ? st.need : f.limit;        // rows wanted
  const uint32_t slot0 = ORDER ? (uint32_t)a.limit - st.need : 0u;
  uint32_t base = f.slice_pre[blockIdx.x];             // rows of the predicate in the slices before this one
  // (a slice without such a row has nothing to place, and the walk ends with the slice's last one)
  const uint32_t stop = std::min(m, base + f.slice_cnt[blockIdx.x]);
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t begin, end;
  first_slice<ORDER>(f, blockIdx.x, begin, end);
  for (int64_t c0 = begin; c0 < end && base < stop; c0 += SCROLL_STEP) {   // (wave-uniform)
    const int64_t row0 = c0 + lane * 4;
    uint32_t less;
    uint64_t s[4];
    const uint32_t hit = first_pred4<ORDER>(f, a, st, row0, less, s);
    uint32_t rank = base, step = 0u;                   // the lanes below hold the rows before this lane's four
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long bj = __ballot((hit >> j) & 1u);
      rank += (uint32_t)__popcll(bj & below);
      step += (uint32_t)__popcll(bj);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((hit >> j) & 1u) {
        if (rank < m) {
          if (ORDER) {
            const uint32_t slot = slot0 + rank;
            if (slot < (uint32_t)HX_SCROLL_MAX_LIMIT) {
              a.cand_s[slot] = st.prefix;
              a.cand_row[slot] = (uint32_t)(row0 + j);
            }
          } else {
            f.out_rows[rank] = (uint32_t)(row0 + j);
          }
        }
        ++rank;
      }
    base += step;
  }
}

// P: a power of two >= limit, at most HX_SCROLL_MAX_LIMIT
__global__ void __launch_bounds__(1024) k_order_sort(OrderArgs a, int P, uint32_t* __restrict__ out_rows,
                                                     uint64_t* __restrict__ out_bits, int32_t* __restrict__ out_count) {
  __shared__ uint64_t ks[HX_SCROLL_MAX_LIMIT];
  __shared__ uint32_t kr[HX_SCROLL_MAX_LIMIT];
  const OrderState st = *a.st;
  const int count = st.all ? (int)st.total : a.limit;  // (all: total < limit)
  for (int i = threadIdx.x; i < P; i += 1024) {
    ks[i] = i < count ? a.cand_s[i] : ~0ull;
    kr[i] = i < count ? a.cand_row[i] : 0xFFFFFFFFu;
  }
  __syncthreads();
  const int t = threadIdx.x;                             // one pair per thread: P / 2 <= 1024
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (t < P / 2) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
        const uint64_t si = ks[i], sx = ks[x];
        const uint32_t ri = kr[i], rx = kr[x];
        const bool gt = si > sx || (si == sx && ri > rx);
        if (gt == ((i & k) == 0)) {
          ks[i] = sx, ks[x] = si;
          kr[i] = rx, kr[x] = ri;
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < a.limit; i += 1024) {
    const uint32_t row = i < count ? kr[i] : 0u;
    const bool ok = i < count && (int64_t)row < a.n;
    out_rows[i] = ok ? row : 0u;
    out_bits[i] = ok ? ((uint64_t)a.hi[row] << 32) | a.lo[row] : 0ull;
  }
  if (threadIdx.x == 0) *out_count = count;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
int first_slices(int64_t n, int grid_cap, int64_t* slice_rows) {
  int64_t g = std::min<int64_t>((n + 1023) / 1024, FIRST_MAX_SLICES);
  if (grid_cap > 0) g = std::min<int64_t>(g, grid_cap);
  g = std::max<int64_t>(g, 1);
  const int64_t rows = std::max<int64_t>(round_up((n + g - 1) / g, 1024), 1024);
  *slice_rows = rows;
  return (int)std::max<int64_t>((n + rows - 1) / rows, 1);
}

void launch_scroll_rows(const uint32_t* mask, int64_t n, int64_t start_row, int limit, uint32_t* slice_cnt,
                        uint32_t* slice_pre, uint32_t* out_rows, int32_t* out_count, int grid_cap, hipStream_t st) {
  FirstArgs f{};
  f.mask = mask;
  f.n = n;
  f.start_row = start_row;
  f.limit = (uint32_t)limit;
  f.slice_cnt = slice_cnt;
  f.slice_pre = slice_pre;
  f.out_rows = out_rows;
  f.out_count = out_count;
  const int g = first_slices(n, grid_cap, &f.slice_rows);
  const OrderArgs none{};
  hipLaunchKernelGGL(k_first_count<false>, dim3(g), dim3(SCROLL_NT), 0, st, f, none);
  hipLaunchKernelGGL(k_first_prefix<false>, dim3(1), dim3(FIRST_MAX_SLICES), 0, st, f, g);
  hipLaunchKernelGGL(k_first_emit<false>, dim3(g), dim3(WAVE), 0, st, f, none);
  HX_HIP(hipGetLastError());
}

void launch_payload_order(const OrderArgs& a, uint32_t* out_rows, uint64_t* out_bits, int32_t* out_count, int grid_cap,
                          hipStream_t st) {
  unsigned grid = (unsigned)std::min<int64_t>((a.n + SCROLL_NT * 8 - 1) / (SCROLL_NT * 8), ORDER_GRID);
  if (grid_cap > 0) grid = std::min(grid, (unsigned)grid_cap);
  hipLaunchKernelGGL(k_order_init, dim3(1), dim3(1024), 0, st, a);
  for (int p = 0; p < ORDER_PASSES; ++p) {
    if (p < 3) hipLaunchKernelGGL(k_order_hist<false>, dim3(grid), dim3(SCROLL_NT), 0, st, a, p, ORDER_SHIFT[p], ORDER_WIDTH[p]);
    else hipLaunchKernelGGL(k_order_hist<true>, dim3(grid), dim3(SCROLL_NT), 0, st, a, p, ORDER_SHIFT[p], ORDER_WIDTH[p]);
    hipLaunchKernelGGL(k_order_pick, dim3(1), dim3(WAVE), 0, st, a, p, ORDER_SHIFT[p]);
  }
  FirstArgs f{};
  f.n = a.n;
  f.limit = (uint32_t)a.limit;
  f.slice_cnt = a.slice_cnt;
  f.slice_pre = a.slice_pre;
  const int g = first_slices(a.n, grid_cap, &f.slice_rows);
  hipLaunchKernelGGL(k_first_count<true>, dim3(g), dim3(SCROLL_NT), 0, st, f, a);
  hipLaunchKernelGGL(k_first_prefix<true>, dim3(1), dim3(FIRST_MAX_SLICES), 0, st, f, g);
  hipLaunchKernelGGL(k_first_emit<true>, dim3(g), dim3(WAVE), 0, st, f, a);
  hipLaunchKernelGGL(k_order_sort, dim3(1), dim3(1024), 0, st, a, next_pow2(std::max(a.limit, 2)), out_rows, out_bits, out_count);
  HX_HIP(hipGetLastError());
}

}  // namespace hx
