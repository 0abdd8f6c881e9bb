// Binary quantization: the 1-bit copy of the stored rows and the Hamming scan stage over it
// (hx_binary_enable, hx_search_bin).  One sign bit per dimension nominates candidates with XOR and popcount -- a 768-wide
// row is 96 bytes, an eighth of the int8 candidate copy -- and a dense re-scoring node above the stage ranks the
// survivors by the exact vectors (query_tree.py: using="binary").  The stage is exact in its own terms: integer scores,
// the engine's total order.  The kernels, their launches, the stage's host side and its entries of the C ABI are here;
// k_binarize_rows, which derives the copy, is in prep.hip beside k_prep_rows.
#include "index.hpp"

namespace hx {

constexpr int BIN_QG = 8;                // queries scored per walk over a staged tile: 8 x BIN_MAX_SLOTS x 16 B = 4 KB of LDS

// One wave per query, four per workgroup: the sign bits of the RAW query (no normalisation: the sign does not need it),
// a ballot per 64 columns; the columns from dim up to 32 * words give 0.
__global__ __launch_bounds__(256) void k_bin_queries(const float* __restrict__ q, int dim, int B, int words,
                                                     uint32_t* __restrict__ qbits, int* bad) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* x = q + (int64_t)b * dim;
  uint32_t* o = qbits + (int64_t)b * words;
  bool nonfinite = false;
  for (int j = 0; j < (words >> 1); ++j) {
    const int c = (j << 6) + lane;
    const float v = c < dim ? x[c] : 0.0f;
    nonfinite = nonfinite || !(__builtin_fabsf(v) <= 3.40282347e38f);
    const uint64_t m = __ballot(v > 0.0f);
    if (lane == 0) *(uint2*)(o + 2 * j) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
  }
  if (__ballot(nonfinite) != 0ull && lane == 0) atomicAdd(bad, 1);
}
void launch_bin_queries(const float* q, int dim, int B, int words, uint32_t* qbits, int* bad, hipStream_t st) {
  HX_CHECK(B >= 1 && words % 4 == 0 && words * 32 >= dim, "bin queries: sizes");
  hipLaunchKernelGGL(k_bin_queries, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, q, dim, B, words, qbits, bad);
  HX_HIP(hipGetLastError());
}

// tau_key[b] = the limit-th best key of query b when its compacted list is full (launch_compact leaves it sorted), else 0
__global__ __launch_bounds__(256) void k_bin_tau(const uint64_t* __restrict__ cand, int cap, const int* __restrict__ cnt, int B,
                                                 int limit, uint64_t* tau_key) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) tau_key[b] = cnt[b] >= limit ? cand[(int64_t)b * cap + limit - 1] : 0ull;
}
void launch_bin_tau(const uint64_t* cand, int cap, const int* cnt, int B, int limit, uint64_t* tau_key, hipStream_t st) {
  HX_CHECK(B >= 1 && limit >= 1 && limit <= cap, "bin tau: sizes");
  hipLaunchKernelGGL(k_bin_tau, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, cand, cap, cnt, B, limit, tau_key);
  HX_HIP(hipGetLastError());
}

// The scan.  A workgroup walks 256-row tiles: the tile's words come from HBM as one contiguous run of 16-byte loads (a
// lane-per-row read would touch every 128-byte line with several instructions) into LDS, rows `lstride` slots apart
// (odd: the 16 lanes of a ds_read_b128 group fall on 16 different slots).  Then lane r owns row r: per group of QG queries
// it walks its row's slots once -- one 16-byte LDS read of the row's slot, and per query one 16-byte LDS read of the
// query's slot, every lane the same address (a broadcast), then per word one XOR and one accumulating population count.
// The group's query words are staged in LDS (s_q, slot-major: slot s of query q at s * QG + q) at the head of the group:
// read straight from global memory they came as per-lane vector loads, one wait each, although the address is
// wave-uniform -- the stores to `cand` in the same loop may alias them as far as the compiler can tell.  A batch above QG
// queries loops over groups with the tile resident in LDS: the rows are read from HBM once per tile, not once per query.
// Rows wider than BIN_PASS_SLOTS slots (dim above 1664) are staged in column passes; with several passes AND several
// groups the tile is staged again per group (from L2).
// Selection is discover.hip's: the 64-bit KEY against the limit-th best key so far -- scores take dim + 1 values, so almost
// every row ties with thousands of others, and a tied row of a later chunk has a larger id, a smaller key, and never
// passes -- with one atomic per wave and query, the passing lanes ranked by a ballot.
// magic / magic_last: ceil(2^32 / slots) of a full pass and of the last one (i / slots for i < 2^13 by one mul-high).
template <int QG>
__global__ __launch_bounds__(BIN_NT) void k_bin_scan(BinScanArgs a, int nslots, int lstride, uint32_t magic,
                                                     uint32_t magic_last, int64_t n_tiles) {
  extern __shared__ __attribute__((aligned(16))) uint4 tile[];
  __shared__ __attribute__((aligned(16))) uint4 s_q[QG * BIN_MAX_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int n_groups = (a.B + QG - 1) / QG;
  const int n_pass = (nslots + BIN_PASS_SLOTS - 1) / BIN_PASS_SLOTS;
  const uint4* rows4 = (const uint4*)a.bits;
  const uint4* q4 = (const uint4*)a.qbits;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t row0 = a.row_begin + t * BIN_NT;
    const int rows = (int)(a.row_end - row0 < BIN_NT ? a.row_end - row0 : BIN_NT);
    const int64_t row = row0 + tid;
    bool on = tid < rows;
    if (a.mask) {
      if (on) on = (a.mask[row >> 5] >> (row & 31)) & 1u;
      if (!__syncthreads_or(on)) continue;                   // the mask keeps no row of the tile: nothing is read
    }
    const uint4* src = rows4 + row0 * nslots;
    for (int g = 0; g < n_groups; ++g) {
      int acc[QG];
#pragma unroll
      for (int q = 0; q < QG; ++q) acc[q] = 0;
      for (int p = 0; p < n_pass; ++p) {
        const int s0 = p * BIN_PASS_SLOTS;
        const int ns = nslots - s0 < BIN_PASS_SLOTS ? nslots - s0 : BIN_PASS_SLOTS;
        const bool stage = g == 0 || n_pass > 1;
        if (stage || p == 0) {
          __syncthreads();                                   // the readers of what the tile and s_q held are done
          if (p == 0) {                                      // the group's query words; a query past B repeats the last
            for (int i = tid; i < QG * nslots; i += BIN_NT) {
              const int q = i & (QG - 1), sl = i / QG;
              const int b = g * QG + q < a.B ? g * QG + q : a.B - 1;
              s_q[i] = q4[(int64_t)b * nslots + sl];
            }
          }
          if (stage) {
            const uint32_t mg = p == n_pass - 1 ? magic_last : magic;
            for (uint32_t i = tid; i < (uint32_t)(rows * ns); i += BIN_NT) {
              const uint32_t r = ns == 1 ? i : __umulhi(i, mg);
              const uint32_t c = i - r * (uint32_t)ns;
              tile[r * lstride + c] = src[(int64_t)r * nslots + s0 + c];
            }
          }
          __syncthreads();
        }
        const uint4* mine = tile + tid * lstride;
        for (int c = 0; c < ns; ++c) {
          const uint4 x = mine[c];
          const uint4* qs = s_q + (s0 + c) * QG;             // the same address in every lane: an LDS broadcast
#pragma unroll
          for (int q = 0; q < QG; ++q) {
            const uint4 w = qs[q];
            acc[q] += __builtin_popcount(x.x ^ w.x) + __builtin_popcount(x.y ^ w.y) + __builtin_popcount(x.z ^ w.z) +
                      __builtin_popcount(x.w ^ w.w);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < QG; ++q) {
        const int b = g * QG + q;
        if (b >= a.B) break;                                 // (uniform)
        const uint64_t key = make_key((float)(a.dim - 2 * acc[q]), a.id_base + (uint32_t)row);
        const bool pass = on && key > a.tau_key[b];
        const uint64_t m = __ballot(pass);
        if (m == 0ull) continue;
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(a.cnt + b, __builtin_popcountll(m));
        base = __shfl(base, leader, 64);
        if (pass) {
          const int slot = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
          if (slot < a.cap) a.cand[(int64_t)b * a.cap + slot] = key;
          else a.ovf[b] = 1;
        }
      }
    }
  }
}

void launch_bin_scan(const BinScanArgs& a, hipStream_t st) {
  if (a.row_end <= a.row_begin || a.B <= 0) return;
  HX_CHECK(a.words % 4 == 0 && a.words >= 4 && a.words <= 128, "bin scan: row width");
  HX_CHECK(a.row_end <= 0xFFFFFFFFll && a.cap >= 1, "bin scan: sizes");
  const int nslots = a.words / 4;
  const int pass = std::min(nslots, BIN_PASS_SLOTS);
  const int lstride = pass | 1;
  const int last = nslots - (nslots - 1) / BIN_PASS_SLOTS * BIN_PASS_SLOTS;
  const size_t lds = (size_t)BIN_NT * lstride * 16;          // at most 52 KB: with s_q inside what a launch may ask without an opt-in
  const int64_t n_tiles = (a.row_end - a.row_begin + BIN_NT - 1) / BIN_NT;
  // what the rows give, at most the CUs times the workgroups one CU's 160 KB of LDS hold
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + 1024)));
  int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, 256 * per_cu));
  if (a.max_grid > 0) grid = std::min(grid, a.max_grid);     // tests: a workgroup walks several tiles at a few thousand rows
#define HX_BIN(QG)                                                                                              \
  hipLaunchKernelGGL(k_bin_scan<QG>, dim3(grid), dim3(BIN_NT), lds, st, a, nslots, lstride, bin_magic(pass), \
                     bin_magic(last), n_tiles)
  if (a.B == 1) HX_BIN(1);
  else if (a.B == 2) HX_BIN(2);
  else if (a.B <= 4) HX_BIN(4);
  else HX_BIN(BIN_QG);
#undef HX_BIN
  HX_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------
// the stage (hx_search_bin; hx.h states the contract)
// ---------------------------------------------------------------------------------
// every refusal that needs no device work
void bin_check(hx_index* h, const void* q_dev, int B, int limit, const void* mask_dev, int64_t mask_rows,
                      const void* keys_dev, const void* counts_dev) {
  HX_CHECK(h, "NULL argument");
  HX_CHECK(h->bin_on, "search_bin: the index keeps no binary copy of its rows (hx_binary_enable)");
  HX_CHECK(B > 0, "B must be positive");
  HX_CHECK(limit >= 1 && limit <= MAX_LIMIT, "limit out of range [1, 2048]");
  HX_CHECK(q_dev && keys_dev && counts_dev, "NULL argument");
  HX_CHECK(!mask_dev || mask_rows == h->n, "mask_rows must equal the index's row count (hx_count)");
}

// The exhaustive scan in growing chunks with a non-predictive threshold, as chunked_example_scan (byexample.hip): the first
// chunk, at most the buffer's capacity, passes every row; after every chunk each query's buffer is compacted to its best L,
// sorted, and the threshold becomes the L-th of them.  A chunk (g - 1) times as long as the rows before it appends about
// (g - 1) L keys of an exchangeable corpus (each new row passes with probability L / rows before); g is chosen so that this
// is at most half of the C - L keys the buffer takes.  A query whose buffer overflowed all the same (a corpus ordered so that
// every chunk beats the threshold) is scanned again in fixed chunks of C - L rows, every row appended, a compaction after
// each: the same list by construction.  ONE host round trip: the overflow flags and the count of non-finite queries, read
// together behind the scan.  Keys leave with internal ids.  The loop is the stage's whatever scores the rows: `s` (BinStage,
// index.hpp) gives the kernel that stages the queries and the scan launch -- hx_search_bin's below, the asymmetric stage's
// in binasym.hip.
void bin_stage_search(hx_index* h, const BinStage& s, int B, int L, const uint32_t* mask_dev, uint64_t* out_keys,
                      int* out_cnt, hipStream_t st) {
  if (h->n == 0) {
    zero_outputs(out_keys, out_cnt, B, L, st);
    return;
  }
  const int C = h->bin_cap ? std::max(h->bin_cap, 2 * L) : std::clamp(next_pow2(8 * L), 2048, CAND_CAP);
  const int64_t chunk0 = h->bin_chunk0 ? std::min(h->bin_chunk0, C) : C;
  const int64_t grow = std::clamp((C + L) / (2 * L), 2, 16);
  uint32_t* qbits = (uint32_t*)h->ws.get(s.q_slot, (size_t)B * s.qwords * 4);
  uint64_t* cand = (uint64_t*)h->ws.get(WS_BIN_CAND, (size_t)B * C * 8);
  int* cnt = (int*)h->ws.get(WS_BIN_CNT, (size_t)B * 4);
  int* flags = (int*)h->ws.get(WS_BIN_FLAGS, (size_t)(B + 1) * 4);     // [0, B) overflow, [B] non-finite queries
  uint64_t* tau = (uint64_t*)h->ws.get(WS_BIN_TAU, (size_t)B * 8);
  uint64_t* tau0 = (uint64_t*)h->ws.get(WS_BIN_TAU0, (size_t)B * 8);   // stays 0: the redo's threshold
  HX_HIP(hipMemsetAsync(cnt, 0, (size_t)B * 4, st));
  HX_HIP(hipMemsetAsync(flags, 0, (size_t)(B + 1) * 4, st));
  HX_HIP(hipMemsetAsync(tau, 0, (size_t)B * 8, st));
  HX_HIP(hipMemsetAsync(tau0, 0, (size_t)B * 8, st));
  s.queries(qbits, flags + B, st);
  BinScanArgs a{};
  a.bits = h->bits;
  a.words = h->bin_words();
  a.dim = h->dim;
  a.qbits = qbits;
  a.B = B;
  a.mask = mask_dev;
  a.tau_key = tau;
  a.cand = cand;
  a.cnt = cnt;
  a.ovf = flags;
  a.cap = C;
  a.id_base = (uint32_t)h->id_base;
  a.max_grid = h->bin_grid;
  for (int64_t r0 = 0, r1 = std::min<int64_t>(h->n, chunk0); r0 < h->n;) {
    a.row_begin = r0;
    a.row_end = r1;
    s.scan(a, 0, st);
    launch_compact(cand, C, cnt, B, L, 0, cand, C, cnt, nullptr, C, st);
    r0 = r1;
    r1 = std::min<int64_t>(h->n, grow * r1);
    if (r0 < h->n) launch_bin_tau(cand, C, cnt, B, L, tau, st);
  }
  std::vector<int> flagged((size_t)B + 1);
  HX_HIP(hipMemcpyAsync(flagged.data(), flags, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CHECK(flagged[(size_t)B] == 0, std::string(s.who) + ": query values must be finite");
  for (int b = 0; b < B; ++b) {
    if (!flagged[(size_t)b]) continue;
    BinScanArgs r = a;
    r.qbits = qbits + (int64_t)b * s.qwords;
    r.B = 1;
    r.tau_key = tau0;
    r.cand = cand + (int64_t)b * C;
    r.cnt = cnt + b;
    r.ovf = flags + b;
    HX_HIP(hipMemsetAsync(cnt + b, 0, 4, st));
    for (int64_t r0 = 0; r0 < h->n; r0 += C - L) {
      r.row_begin = r0;
      r.row_end = std::min<int64_t>(h->n, r0 + (C - L));
      s.scan(r, b, st);
      launch_compact(r.cand, C, r.cnt, 1, L, 0, r.cand, C, r.cnt, nullptr, C, st);
    }
  }
  HX_HIP(hipMemcpy2DAsync(out_keys, (size_t)L * 8, cand, (size_t)C * 8, (size_t)L * 8, (size_t)B, hipMemcpyDeviceToDevice, st));
  HX_HIP(hipMemcpyAsync(out_cnt, cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
}

// hx_search_bin: the sign bits of the queries (k_bin_queries) and k_bin_scan in the loop above
static void search_bin(hx_index* h, const float* q_dev, int B, int L, const uint32_t* mask_dev, uint64_t* out_keys,
                       int* out_cnt, hipStream_t st) {
  const int words = h->bin_words();
  BinStage s;
  s.who = "search_bin";
  s.qwords = words;
  s.q_slot = WS_BIN_Q;
  s.queries = [=](uint32_t* qbits, int* bad, hipStream_t t) { launch_bin_queries(q_dev, h->dim, B, words, qbits, bad, t); };
  s.scan = [](const BinScanArgs& a, int, hipStream_t t) { launch_bin_scan(a, t); };
  bin_stage_search(h, s, B, L, mask_dev, out_keys, out_cnt, st);
}

}  // namespace hx

extern "C" {

int hx_binary_enable(hx_index* h) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  if (h->bin_on) return 0;
  h->set_device();
  HX_HIP(hipDeviceSynchronize());        // the rows' writes may be queued on a caller's stream (hx_add_rows_dev)
  const int64_t rb = (int64_t)h->bin_words() * 4;
  if (h->cap > 0) {
    HX_HIP(hipMalloc((void**)&h->bits, (size_t)(h->cap * rb)));
    launch_binarize_rows(h->dense, h->dim_pad, h->bin_words(), h->n, h->bits, nullptr);
    HX_HIP(hipStreamSynchronize(nullptr));
  }
  h->bin_on = true;
  HX_CATCH
}

int hx_binary_enabled(hx_index* h, int32_t* on) {
  HX_TRY
  HX_CHECK(h && on, "NULL argument");
  *on = h->bin_on ? 1 : 0;
  HX_CATCH
}

int hx_binary_debug_row(hx_index* h, int64_t row, uint32_t* words_out, int32_t cap_words) {
  HX_TRY
  HX_CHECK(h && words_out, "NULL argument");
  HX_CHECK(h->bin_on, "binary_debug_row: the index keeps no binary copy of its rows (hx_binary_enable)");
  HX_CHECK(row >= 0 && row < h->n, "row out of range");
  HX_CHECK(cap_words >= h->dim_pad / 32, "binary_debug_row: room for dim_pad / 32 words is needed");
  h->set_device();
  HX_HIP(hipMemcpy(words_out, h->bits + row * h->bin_words(), (size_t)(h->dim_pad / 32) * 4, hipMemcpyDeviceToHost));
  HX_CATCH
}

int hx_search_bin_masked(hx_index* h, const float* q_dev, int32_t B, int32_t limit, const uint32_t* mask_dev,
                         int64_t mask_rows, uint64_t* keys_dev, int32_t* counts_dev, void* stream) {
  HX_TRY
  bin_check(h, q_dev, B, limit, mask_dev, mask_rows, keys_dev, counts_dev);
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  search_bin(h, q_dev, B, limit, mask_dev, keys_dev, counts_dev, st);
  remap_out(h, keys_dev, (int64_t)B * limit, st);
  HX_CATCH
}

int hx_search_bin(hx_index* h, const float* q_dev, int32_t B, int32_t limit, uint64_t* keys_dev, int32_t* counts_dev,
                  void* stream) {
  return hx_search_bin_masked(h, q_dev, B, limit, nullptr, 0, keys_dev, counts_dev, stream);
}

}  // extern "C"
