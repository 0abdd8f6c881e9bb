// Binary quantization with an asymmetric query: the rows stay at one sign bit per dimension, the
// query keeps 4 or 8 bits -- Qdrant's BinaryQuantization(query_encoding = scalar4bits | scalar8bits).  The score of a row is
// the dot product of the query's small-integer codes with the row's +-1 values: 2 S - T, S = the sum of the codes over the
// row's set bits, T = the sum of all codes.  S comes from the bit planes of the codes' two's complement: one AND and one
// accumulating population count per plane and 32-bit word.  The stored copy, the chunked loop, the threshold kernel and
// the compaction are hx_search_bin's (binscan.hip: bin_stage_search); the query kernel, the scan and the entries are here.
#include "index.hpp"

namespace hx {

// One wave per query, four per workgroup.  m = max |q| by a wave reduction; the code of a column is
// (int) rintf((q / m) * QMAX) -- one correctly rounded fp32 division, one fp32 multiplication, round half to even; |q / m|
// <= 1, so no clamp -- and 0 for m == 0 and for the columns from dim up to 32 * words; per 64 columns and plane one ballot.
template <int P>
__global__ __launch_bounds__(256) void k_asym_queries(const float* __restrict__ q, int dim, int B, int words,
                                                      uint32_t* __restrict__ planes, int* __restrict__ totals, int* bad) {
  constexpr float QMAX = (float)((1 << (P - 1)) - 1);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* x = q + (int64_t)b * dim;
  uint32_t* o = planes + (int64_t)b * P * words;
  bool nonfinite = false;
  float m = 0.0f;
  for (int c = lane; c < dim; c += 64) {
    const float v = __builtin_fabsf(x[c]);
    nonfinite = nonfinite || !(v <= 3.40282347e38f);
    m = v > m ? v : m;
  }
  for (int s = 32; s > 0; s >>= 1) {
    const float v = __shfl_xor(m, s, 64);
    m = v > m ? v : m;
  }
  const bool any_bad = __ballot(nonfinite) != 0ull;          // the call fails; the codes are not read
  int t = 0;
  for (int j = 0; j < (words >> 1); ++j) {
    const int c = (j << 6) + lane;
    int code = 0;
    if (c < dim && m > 0.0f && !any_bad) {
      const float d = x[c] / m;
      code = (int)rintf(d * QMAX);
    }
    t += code;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const uint64_t mk = __ballot(((code >> k) & 1) != 0);
      if (lane == 0) *(uint2*)(o + (int64_t)k * words + 2 * j) = make_uint2((uint32_t)mk, (uint32_t)(mk >> 32));
    }
  }
  for (int s = 32; s > 0; s >>= 1) t += __shfl_xor(t, s, 64);
  if (lane == 0) {
    totals[b] = t;
    if (any_bad) atomicAdd(bad, 1);
  }
}

void launch_asym_queries(const float* q, int dim, int B, int words, int P, uint32_t* planes, int* totals, int* bad,
                         hipStream_t st) {
  HX_CHECK(B >= 1 && words % 4 == 0 && words * 32 >= dim && (P == 4 || P == 8), "asym queries: sizes");
  const dim3 grid((unsigned)((B + 3) / 4));
  if (P == 8) hipLaunchKernelGGL(k_asym_queries<8>, grid, dim3(256), 0, st, q, dim, B, words, planes, totals, bad);
  else hipLaunchKernelGGL(k_asym_queries<4>, grid, dim3(256), 0, st, q, dim, B, words, planes, totals, bad);
  HX_HIP(hipGetLastError());
}

struct AsymScanArgs {
  BinScanArgs s;           // qbits = the planes, [B x P x words]
  const int* totals;       // [B]
};

// k_bin_scan's schedule (binscan.hip has the account): 256-row tiles brought to LDS by one contiguous run of 16-byte loads,
// rows `lstride` slots apart (odd), lane r owning row r, column passes for rows above BIN_PASS_SLOTS slots, a batch above QG
// queries looping over groups with the tile resident, the grid-stride loop, the key against tau_key with one atomic per
// wave and query.  What differs is the walk: per slot of its row a lane reads, per query of the group, the P plane slots
// (s_q, at ((slot * QG + query) * P + plane): the same address in every lane, a broadcast) and per plane and word does one
// AND and one accumulating population count into the accumulator of that (query, plane); the planes are combined once per
// row: S = -2^(P-1) acc[P-1] + sum_{k < P-1} 2^k acc[k], score = 2 S - T.
// LDS: s_q is QG x P x BIN_MAX_SLOTS x 16 B of static LDS beside the dynamic tile of at most 52 KB; QG x P <= 16 keeps it at
// 8 KB, 60 KB together, inside the 64 KB a launch may ask for without an opt-in.
template <int P, int QG>
__global__ __launch_bounds__(BIN_NT) void k_asym_scan(AsymScanArgs aa, int nslots, int lstride, uint32_t magic,
                                                      uint32_t magic_last, int64_t n_tiles) {
  static_assert(P * QG <= 16, "s_q above 8 KB leaves no room for a 52 KB tile");
  extern __shared__ __attribute__((aligned(16))) uint4 tile[];
  __shared__ __attribute__((aligned(16))) uint4 s_q[QG * P * BIN_MAX_SLOTS];
  const BinScanArgs& a = aa.s;
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
      int acc[QG][P];
#pragma unroll
      for (int q = 0; q < QG; ++q)
#pragma unroll
        for (int k = 0; k < P; ++k) acc[q][k] = 0;
      for (int p = 0; p < n_pass; ++p) {
        const int s0 = p * BIN_PASS_SLOTS;
        const int ns = nslots - s0 < BIN_PASS_SLOTS ? nslots - s0 : BIN_PASS_SLOTS;
        const bool stage = g == 0 || n_pass > 1;
        if (stage || p == 0) {
          __syncthreads();                                   // the readers of what the tile and s_q held are done
          if (p == 0) {                                      // the group's planes; a query past B repeats the last
            for (int i = tid; i < QG * P * nslots; i += BIN_NT) {
              const int k = i & (P - 1), q = (i / P) & (QG - 1), sl = i / (P * QG);
              const int b = g * QG + q < a.B ? g * QG + q : a.B - 1;
              s_q[i] = q4[((int64_t)b * P + k) * nslots + sl];
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
          const uint4* qs = s_q + (s0 + c) * (QG * P);       // the same address in every lane: an LDS broadcast
#pragma unroll
          for (int q = 0; q < QG; ++q) {
#pragma unroll
            for (int k = 0; k < P; ++k) {
              const uint4 w = qs[q * P + k];
              acc[q][k] += __builtin_popcount(x.x & w.x) + __builtin_popcount(x.y & w.y) + __builtin_popcount(x.z & w.z) +
                           __builtin_popcount(x.w & w.w);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < QG; ++q) {
        const int b = g * QG + q;
        if (b >= a.B) break;                                 // (uniform)
        int S = -(acc[q][P - 1] << (P - 1));
#pragma unroll
        for (int k = 0; k < P - 1; ++k) S += acc[q][k] << k;
        const uint64_t key = make_key((float)(2 * S - aa.totals[b]), a.id_base + (uint32_t)row);
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

// The queries per walk: what fits beside the tile (P x QG <= 16) -- 2 at 8 planes, 4 at 4 -- and no more than the batch has.
// A partial last group (B = 3 at 4 planes) scores its repeated last query for nothing; what that costs was not measured.
void launch_asym_scan(const BinScanArgs& a, const int* totals, int P, hipStream_t st) {
  if (a.row_end <= a.row_begin || a.B <= 0) return;
  HX_CHECK(a.words % 4 == 0 && a.words >= 4 && a.words <= 4 * BIN_MAX_SLOTS, "asym scan: row width");
  HX_CHECK(a.row_end <= 0xFFFFFFFFll && a.cap >= 1 && (P == 4 || P == 8), "asym scan: sizes");
  const int nslots = a.words / 4;
  const int pass = std::min(nslots, BIN_PASS_SLOTS);
  const int lstride = pass | 1;
  const int last = nslots - (nslots - 1) / BIN_PASS_SLOTS * BIN_PASS_SLOTS;
  const size_t lds = (size_t)BIN_NT * lstride * 16;          // at most 52 KB
  const int QG = a.B == 1 ? 1 : (a.B == 2 || P == 8) ? 2 : 4;
  const size_t lds_q = (size_t)QG * P * BIN_MAX_SLOTS * 16;
  const int64_t n_tiles = (a.row_end - a.row_begin + BIN_NT - 1) / BIN_NT;
  // what the rows give, at most the CUs times the workgroups one CU's 160 KB of LDS hold
  // (+ 1 KB: the kernel's static LDS is a little above s_q, and a grid of one workgroup per CU more than are resident runs
  // its last share at a fraction of the occupancy)
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + lds_q + 1024)));
  int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, 256 * per_cu));
  if (a.max_grid > 0) grid = std::min(grid, a.max_grid);
  const AsymScanArgs aa{a, totals};
#define HX_ASYM(P_, QG_)                                                                                              \
  hipLaunchKernelGGL((k_asym_scan<P_, QG_>), dim3(grid), dim3(BIN_NT), lds, st, aa, nslots, lstride, bin_magic(pass), \
                     bin_magic(last), n_tiles)
  if (P == 8) {
    if (QG == 1) HX_ASYM(8, 1);
    else HX_ASYM(8, 2);
  } else {
    if (QG == 1) HX_ASYM(4, 1);
    else if (QG == 2) HX_ASYM(4, 2);
    else HX_ASYM(4, 4);
  }
#undef HX_ASYM
  HX_HIP(hipGetLastError());
}

static void check_query_bits(int query_bits) {
  HX_CHECK(query_bits == 4 || query_bits == 8, "query_bits must be 4 or 8");
}

}  // namespace hx

extern "C" {

int hx_search_bin_asym_masked(hx_index* h, const float* q_dev, int32_t B, int32_t limit, int32_t query_bits,
                              const uint32_t* mask_dev, int64_t mask_rows, uint64_t* keys_dev, int32_t* counts_dev,
                              void* stream) {
  HX_TRY
  check_query_bits(query_bits);
  bin_check(h, q_dev, B, limit, mask_dev, mask_rows, keys_dev, counts_dev);
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  const int words = h->bin_words(), P = query_bits, dim = h->dim;
  int* totals = h->n ? (int*)h->ws.get(WS_ASYM_TOT, (size_t)B * 4) : nullptr;
  BinStage s;
  s.who = "search_bin_asym";
  s.qwords = P * words;
  s.q_slot = WS_ASYM_PLANES;
  s.queries = [=](uint32_t* planes, int* bad, hipStream_t t) {
    launch_asym_queries(q_dev, dim, B, words, P, planes, totals, bad, t);
  };
  s.scan = [=](const BinScanArgs& a, int b0, hipStream_t t) { launch_asym_scan(a, totals + b0, P, t); };
  bin_stage_search(h, s, B, limit, mask_dev, keys_dev, counts_dev, st);
  remap_out(h, keys_dev, (int64_t)B * limit, st);
  HX_CATCH
}

int hx_search_bin_asym(hx_index* h, const float* q_dev, int32_t B, int32_t limit, int32_t query_bits, uint64_t* keys_dev,
                       int32_t* counts_dev, void* stream) {
  return hx_search_bin_asym_masked(h, q_dev, B, limit, query_bits, nullptr, 0, keys_dev, counts_dev, stream);
}

int hx_bin_asym_debug_query(hx_index* h, const float* q_dev, int32_t B, int32_t query_bits, uint32_t* planes_out,
                            int32_t* totals_out, int64_t cap_words) {
  HX_TRY
  check_query_bits(query_bits);
  HX_CHECK(h && q_dev && planes_out && totals_out, "NULL argument");
  HX_CHECK(B > 0, "B must be positive");
  const int64_t out_words = h->dim_pad / 32;
  HX_CHECK(cap_words >= (int64_t)B * query_bits * out_words,
           "bin_asym_debug_query: room for B * query_bits * dim_pad / 32 words is needed");
  h->set_device();
  const int words = h->bin_words();
  uint32_t* planes = (uint32_t*)h->ws.get(WS_ASYM_PLANES, (size_t)B * query_bits * words * 4);
  int* totals = (int*)h->ws.get(WS_ASYM_TOT, (size_t)(B + 1) * 4);   // [B]: the non-finite queries
  HX_HIP(hipMemsetAsync(totals + B, 0, 4, nullptr));
  launch_asym_queries(q_dev, h->dim, B, words, query_bits, planes, totals, totals + B, nullptr);
  std::vector<int> tot((size_t)B + 1);
  HX_HIP(hipMemcpy(tot.data(), totals, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost));
  HX_CHECK(tot[(size_t)B] == 0, "bin_asym_debug_query: query values must be finite");
  HX_HIP(hipMemcpy2D(planes_out, (size_t)out_words * 4, planes, (size_t)words * 4, (size_t)out_words * 4,
                     (size_t)B * query_bits, hipMemcpyDeviceToHost));
  std::memcpy(totals_out, tot.data(), (size_t)B * 4);
  HX_CATCH
}

}  // extern "C"
