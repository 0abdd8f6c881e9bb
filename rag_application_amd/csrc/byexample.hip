// Host side of the searches by example: recommend, discovery and context search (section 29) and the
// distance matrix (section 28) -- their checks, their scans as launches on one stream, and their entries of the C ABI.  The
// kernels are in reco.hip, discover.hip and matrix.hip; the average route's dense stage is engine.hip's.
#include "index.hpp"

#include <cmath>
#include <string>

namespace hx {

// ---------------------------------------------------------------------------------
// the examples of a recommend or discover call
// ---------------------------------------------------------------------------------
// A call as the kernels take it: the examples request by request (recommend: positives first, each group in the order
// given; discover: the order given).
struct RecoCall {
  std::vector<RecoReq> req;
  std::vector<int64_t> src;       // per example: the stored row, or -1 - (index of the raw vector)
  std::vector<uint32_t> excl;     // per request from excl0: its stored rows, ascending, unique
  int n_raw = 0, max_excl = 0;
};

// the refusals both calls share on their sizes, their mask and the head of the example offsets
static void examples_check(hx_index* h, const char* who, int R, const int64_t* indptr, const void* mask, int64_t mask_rows,
                           int limit) {
  const std::string w = std::string(who) + ": ";
  HX_CHECK(R >= 1 && R <= HX_RECO_MAX_REQUESTS, w + "requests out of range [1, 16]");
  HX_CHECK(limit >= 1 && limit <= HX_RECO_MAX_LIMIT, w + "limit out of range [1, 1024]");
  HX_CHECK(!mask || mask_rows == h->n, w + "mask_rows must equal the index's row count (hx_count)");
  HX_CHECK(indptr[0] == 0, w + "bad example indptr");
}
// A request begins: its descriptor, after the caller's checks on its example count.
static RecoReq request_begin(hx_index* h, const RecoCall& c, const char* who, int r, int64_t n_ex) {
  HX_CHECK(n_ex * h->dim_pad <= RECO_LDS_FLOATS, std::string(who) + ": examples x padded width above 32768 floats");
  RecoReq q{};
  q.ex0 = (int)c.src.size();
  q.excl0 = (int)c.excl.size();
  q.slot = r;
  q.n_ex = (int)n_ex;
  return q;
}
// One example, checked: a raw vector (row == -1: the next of vecs; returns -1 - its index) or a stored row (returns it; it
// joins the request's excluded rows).
static int64_t example_source(hx_index* h, RecoCall& c, const char* who, int64_t row, const float* vecs) {
  if (row == -1) {
    HX_CHECK(vecs != nullptr, "NULL argument");
    const float* v = vecs + (int64_t)c.n_raw * h->dim;
    for (int k = 0; k < h->dim; ++k)
      HX_CHECK(std::isfinite(v[k]), std::string(who) + ": example vector values must be finite");
    return -1 - (int64_t)c.n_raw++;
  }
  HX_CHECK(row >= 0 && row < h->n, std::string(who) + ": example row out of range");
  c.excl.push_back((uint32_t)row);
  return row;
}
// A request ends: its excluded rows sorted and unique, the request appended.
static void request_end(RecoCall& c, RecoReq q) {
  std::sort(c.excl.begin() + q.excl0, c.excl.end());
  c.excl.erase(std::unique(c.excl.begin() + q.excl0, c.excl.end()), c.excl.end());
  q.n_excl = (int)c.excl.size() - q.excl0;
  c.max_excl = std::max(c.max_excl, q.n_excl);
  c.req.push_back(q);
}

// every refusal of hx_recommend, before any device work
static RecoCall reco_check(hx_index* h, int strategy, int R, const int64_t* indptr, const int64_t* rows, const int8_t* sign,
                           const float* vecs, const void* mask, int64_t mask_rows, int limit) {
  HX_CHECK(h && indptr && rows && sign, "NULL argument");
  HX_CHECK(strategy == HX_RECO_AVERAGE || strategy == HX_RECO_BEST_SCORE || strategy == HX_RECO_SUM_SCORES,
           "recommend: unknown strategy");
  examples_check(h, "recommend", R, indptr, mask, mask_rows, limit);
  RecoCall c;
  for (int r = 0; r < R; ++r) {
    const int64_t b = indptr[r], e = indptr[r + 1];
    HX_CHECK(e - b >= 1 && e - b <= HX_RECO_MAX_EXAMPLES, "recommend: a request takes 1 to 32 examples");
    RecoReq q = request_begin(h, c, "recommend", r, e - b);
    std::vector<int64_t> src_of((size_t)(e - b));
    for (int64_t i = b; i < e; ++i) {
      HX_CHECK(sign[i] == 1 || sign[i] == -1, "recommend: a sign must be +1 or -1");
      src_of[(size_t)(i - b)] = example_source(h, c, "recommend", rows[i], vecs);
    }
    for (int s = 1; s >= -1; s -= 2)
      for (int64_t i = b; i < e; ++i)
        if (sign[i] == s) {
          c.src.push_back(src_of[(size_t)(i - b)]);
          if (s == 1) ++q.n_pos;
        }
    HX_CHECK(strategy != HX_RECO_AVERAGE || q.n_pos >= 1, "recommend: the average strategy needs a positive example");
    request_end(c, q);
  }
  return c;
}

// every refusal of hx_discover, before any device work.  The examples keep the order given (the target, then the pairs);
// RecoReq.n_pos = 1 when the request has a target.
static RecoCall discover_check(hx_index* h, int R, const int64_t* indptr, const int64_t* rows, const float* vecs,
                               const int32_t* has_target, const void* mask, int64_t mask_rows, int limit) {
  HX_CHECK(h && indptr && rows && has_target, "NULL argument");
  examples_check(h, "discover", R, indptr, mask, mask_rows, limit);
  RecoCall c;
  for (int r = 0; r < R; ++r) {
    const int64_t b = indptr[r], e = indptr[r + 1];
    HX_CHECK(has_target[r] == 0 || has_target[r] == 1, "discover: has_target must be 0 or 1");
    HX_CHECK(e - b >= 1, "discover: a request needs a target or a context pair");
    HX_CHECK(e - b <= HX_RECO_MAX_EXAMPLES, "discover: a request takes at most 32 examples (the target and two per pair)");
    HX_CHECK((e - b - has_target[r]) % 2 == 0, "discover: context examples come in pairs (positive, negative)");
    RecoReq q = request_begin(h, c, "discover", r, e - b);
    q.n_pos = has_target[r];
    for (int64_t i = b; i < e; ++i) c.src.push_back(example_source(h, c, "discover", rows[i], vecs));
    request_end(c, q);
  }
  return c;
}

// What both scans need from a call, on the device: the example matrix X, the request descriptors and the excluded rows,
// and the scan's launches -- requests in order, as many as fit the LDS together: the corpus is read once per launch.
struct ExamplePlan {
  RecoCall c;                                // (req[].lds0: where a request's examples are staged in its launch)
  std::vector<std::pair<int, int>> groups;   // [first request, end) of a launch
  std::vector<uint8_t> meta;                 // the upload's source, read until the caller synchronises
  uint8_t* meta_dev;
  const RecoReq* req_dev;
  const uint32_t* excl_dev;
  float* X;
  int lds_examples(int g1) const { return c.req[g1 - 1].lds0 + c.req[g1 - 1].n_ex; }   // of the launch that ends at g1
};
static void example_plan(hx_index* h, int R, const RecoCall& c_in, const float* vecs, hipStream_t st, ExamplePlan& p) {
  RecoCall& c = p.c = c_in;
  const int E = (int)c.src.size(), dp = h->dim_pad;
  for (int r = 0, g0 = 0, used = 0; r < R; ++r) {
    if ((int64_t)(used + c.req[r].n_ex) * dp > RECO_LDS_FLOATS) {
      p.groups.push_back({g0, r});
      g0 = r;
      used = 0;
    }
    c.req[r].lds0 = used;
    used += c.req[r].n_ex;
    if (r == R - 1) p.groups.push_back({g0, R});
  }
  // one upload: the descriptors, the example sources, the excluded rows
  const size_t o_src = round_up(R * sizeof(RecoReq), 16), o_excl = o_src + round_up((size_t)E * 8, 16);
  const size_t meta_bytes = o_excl + c.excl.size() * 4 + 16;
  p.meta.assign(meta_bytes, 0);
  std::memcpy(p.meta.data(), c.req.data(), R * sizeof(RecoReq));
  std::memcpy(p.meta.data() + o_src, c.src.data(), (size_t)E * 8);
  if (!c.excl.empty()) std::memcpy(p.meta.data() + o_excl, c.excl.data(), c.excl.size() * 4);
  p.meta_dev = (uint8_t*)h->ws.get(WS_RECO_META, meta_bytes);
  HX_HIP(hipMemcpyAsync(p.meta_dev, p.meta.data(), meta_bytes, hipMemcpyHostToDevice, st));
  p.req_dev = (const RecoReq*)p.meta_dev;
  p.excl_dev = (const uint32_t*)(p.meta_dev + o_excl);
  float* raw_n = nullptr;
  if (c.n_raw) {   // raw vectors: the dense stage's query preparation (finite: checked on the host)
    float* raw = (float*)h->ws.get(WS_RECO_RAW, (size_t)c.n_raw * h->dim * 4);
    raw_n = (float*)h->ws.get(WS_RECO_RAWN, (size_t)c.n_raw * dp * 4);
    HX_HIP(hipMemcpyAsync(raw, vecs, (size_t)c.n_raw * h->dim * 4, hipMemcpyHostToDevice, st));
    launch_prep_queries_f(raw, h->dim, c.n_raw, c.n_raw, h->dim, dp, raw_n, nullptr, st);
  }
  p.X = (float*)h->ws.get(WS_RECO_X, (size_t)E * dp * 4);
  launch_reco_examples(h->dense, raw_n, (const int64_t*)(p.meta_dev + o_src), E, dp, p.X, st);
}

// The candidate buffers of the exhaustive scan, counters and overflow flags zeroed: C keys per request (cap: the test's
// override) and the rows of the first chunk, at most C.
struct ScanBuffers {
  int C;
  int64_t chunk0;
  uint64_t* cand;
  int *cnt, *ovf;
};
static ScanBuffers scan_buffers(hx_index* h, int R, int L, int cap, int chunk0, hipStream_t st) {
  ScanBuffers b{};
  b.C = cap ? std::max(cap, 2 * L) : std::clamp(next_pow2(8 * L), 2048, CAND_CAP);
  b.chunk0 = chunk0 ? std::min(chunk0, b.C) : b.C;
  b.cand = (uint64_t*)h->ws.get(WS_RECO_CAND, (size_t)R * b.C * 8);
  b.cnt = (int*)h->ws.get(WS_RECO_CNT, (size_t)R * 4);
  b.ovf = (int*)h->ws.get(WS_RECO_OVF, (size_t)R * 4);
  HX_HIP(hipMemsetAsync(b.cnt, 0, (size_t)R * 4, st));
  HX_HIP(hipMemsetAsync(b.ovf, 0, (size_t)R * 4, st));
  return b;
}
// what the two scans' argument structs share
template <typename Args>
static Args scan_args(hx_index* h, const ExamplePlan& p, const ScanBuffers& b, const uint32_t* mask_dev) {
  Args a{};
  a.dense = h->dense;
  a.dim_pad = h->dim_pad;
  a.X = p.X;
  a.excl = p.excl_dev;
  a.mask = mask_dev;
  a.cand = b.cand;
  a.cnt = b.cnt;
  a.ovf = b.ovf;
  a.cap = b.C;
  a.id_base = (uint32_t)h->id_base;
  return a;
}

// The exhaustive scan in geometric chunks with a non-predictive threshold, as chunked_scan: the first chunk, at most the
// buffer's capacity, passes every row; fold() compacts every request's buffer to its best L, sorted, and sets the
// threshold from them.  A doubling chunk of an exchangeable corpus appends about L ln 2 keys; the buffer takes C - L.
// scan(g0, g1, r0, r1, redo) launches requests [g0, g1) over rows [r0, r1), with the threshold that passes every row when
// redo.  redone (may be NULL) counts the requests that went through the redo.  Synchronises `st`.
template <typename Scan, typename Fold>
static void chunked_example_scan(hx_index* h, ExamplePlan& p, const ScanBuffers& b, int R, int L, Scan&& scan, Fold&& fold,
                                 int64_t* redone, uint64_t* out_keys, int* out_cnt, hipStream_t st) {
  const int C = b.C;
  for (int64_t r0 = 0, r1 = std::min<int64_t>(h->n, b.chunk0); r0 < h->n;) {
    for (const auto& g : p.groups) scan(g.first, g.second, r0, r1, false);
    fold();
    r0 = r1;
    r1 = std::min<int64_t>(h->n, 2 * r1);
  }
  // the overflow word, read once behind the scan
  std::vector<int> flagged((size_t)R);
  HX_HIP(hipMemcpyAsync(flagged.data(), b.ovf, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  // A request whose buffer overflowed (a corpus ordered so that every chunk beats the threshold): again in fixed chunks of
  // C - L rows, every row appended, a compaction after each -- as exact_range_fallback; the same list by construction.
  for (int r = 0; r < R; ++r) {
    if (!flagged[(size_t)r]) continue;
    if (redone) ++*redone;
    p.c.req[r].lds0 = 0;
    HX_HIP(hipMemcpyAsync(p.meta_dev + r * sizeof(RecoReq), &p.c.req[r], sizeof(RecoReq), hipMemcpyHostToDevice, st));
    HX_HIP(hipMemsetAsync(b.cnt + r, 0, 4, st));
    for (int64_t r0 = 0; r0 < h->n; r0 += C - L) {
      scan(r, r + 1, r0, std::min<int64_t>(h->n, r0 + (C - L)), true);
      launch_compact(b.cand + (int64_t)r * C, C, b.cnt + r, 1, L, 0, b.cand + (int64_t)r * C, C, b.cnt + r, nullptr, C, st);
    }
  }
  HX_HIP(hipMemcpy2DAsync(out_keys, (size_t)L * 8, b.cand, (size_t)C * 8, (size_t)L * 8, (size_t)R, hipMemcpyDeviceToDevice, st));
  HX_HIP(hipMemcpyAsync(out_cnt, b.cnt, (size_t)R * 4, hipMemcpyDeviceToDevice, st));
  HX_HIP(hipStreamSynchronize(st));
}

// ---------------------------------------------------------------------------------
// recommend search (hx_recommend)
// ---------------------------------------------------------------------------------
// count_known: the kept rows of the mask when the caller counted them (the host entry), -1 otherwise.  Keys leave with
// internal ids.  Synchronises `st`.
static void recommend_dev(hx_index* h, int strategy, int R, const RecoCall& c, const float* vecs, const uint32_t* mask_dev,
                          int64_t count_known, int L, uint64_t* out_keys, int* out_cnt, hipStream_t st) {
  if (h->n == 0 || count_known == 0) {
    zero_outputs(out_keys, out_cnt, R, L, st);
    HX_HIP(hipStreamSynchronize(st));
    return;
  }
  ExamplePlan p;
  example_plan(h, R, c, vecs, st, p);
  if (strategy == HX_RECO_AVERAGE) {
    // the dense stage, unchanged, for R queries and room for every stored example; then the examples are dropped
    const int Lin = L + c.max_excl;
    float* q = (float*)h->ws.get(WS_RECO_Q, (size_t)R * h->dim * 4);
    uint64_t* keys = (uint64_t*)h->ws.get(WS_RECO_KEYS, (size_t)R * Lin * 8);
    int* kcnt = (int*)h->ws.get(WS_RECO_KCNT, (size_t)R * 4);
    launch_reco_average(p.X, p.req_dev, R, h->dim, h->dim_pad, q, st);
    if (masked_dense_dev(h, q, R, Lin, mask_dev, count_known, keys, kcnt, st))
      launch_reco_drop(keys, Lin, kcnt, p.req_dev, p.excl_dev, (uint32_t)h->id_base, R, L, out_keys, out_cnt, st);
    else zero_outputs(out_keys, out_cnt, R, L, st);
    HX_HIP(hipStreamSynchronize(st));
    return;
  }
  // BEST_SCORE / SUM_SCORES: the threshold is a score -- tau = -inf passes every row, and every compaction sets tau to the
  // exact L-th score so far
  const ScanBuffers b = scan_buffers(h, R, L, h->reco_cap, h->reco_chunk0, st);
  float* tau = (float*)h->ws.get(WS_RECO_TAU, (size_t)R * 4);
  float* tau0 = (float*)h->ws.get(WS_RECO_TAU0, (size_t)R * 4);   // stays -inf: the redo's threshold
  launch_fill_f32(tau, R, -__builtin_inff(), st);
  launch_fill_f32(tau0, R, -__builtin_inff(), st);
  RecoScanArgs a = scan_args<RecoScanArgs>(h, p, b, mask_dev);
  a.strategy = strategy;
  const auto scan = [&](int g0, int g1, int64_t r0, int64_t r1, bool redo) {
    a.req = p.req_dev + g0;
    a.n_req = g1 - g0;
    a.row_begin = r0;
    a.row_end = r1;
    a.tau = redo ? tau0 : tau;
    launch_reco_scan(a, p.lds_examples(g1), st);
  };
  const auto fold = [&] { launch_compact(b.cand, b.C, b.cnt, R, L, 0, b.cand, b.C, b.cnt, tau, b.C, st); };
  chunked_example_scan(h, p, b, R, L, scan, fold, nullptr, out_keys, out_cnt, st);
}

// ---------------------------------------------------------------------------------
// discovery and context search (hx_discover)
// ---------------------------------------------------------------------------------
// count_known: the kept rows of the mask when the caller counted them (the host entry), -1 otherwise.  Keys leave with
// internal ids.  Synchronises `st`.
static void discover_dev(hx_index* h, int R, const RecoCall& c, const float* vecs, const uint32_t* mask_dev,
                         int64_t count_known, int L, uint64_t* out_keys, int* out_cnt, hipStream_t st) {
  if (h->n == 0 || count_known == 0) {
    zero_outputs(out_keys, out_cnt, R, L, st);
    HX_HIP(hipStreamSynchronize(st));
    return;
  }
  ExamplePlan p;
  example_plan(h, R, c, vecs, st, p);
  // The threshold is ON THE KEY: tau_key = 0 passes every row; every compaction keeps the best L, sorted, and k_discover_tau
  // sets tau_key to the L-th of them.  Chunks ascend in row order, so a later row that ties the L-th score has a larger id, a
  // smaller key, and is not appended: a collection of tied scores appends what one of distinct scores appends.
  const ScanBuffers b = scan_buffers(h, R, L, h->discover_cap, h->discover_chunk0, st);
  uint64_t* tau = (uint64_t*)h->ws.get(WS_DISC_TAU, (size_t)R * 8);
  uint64_t* tau0 = (uint64_t*)h->ws.get(WS_DISC_TAU0, (size_t)R * 8);   // stays 0: the redo's threshold
  HX_HIP(hipMemsetAsync(tau, 0, (size_t)R * 8, st));
  HX_HIP(hipMemsetAsync(tau0, 0, (size_t)R * 8, st));
  DiscoverScanArgs a = scan_args<DiscoverScanArgs>(h, p, b, mask_dev);
  const auto scan = [&](int g0, int g1, int64_t r0, int64_t r1, bool redo) {
    a.req = p.req_dev + g0;
    a.n_req = g1 - g0;
    a.row_begin = r0;
    a.row_end = r1;
    a.tau_key = redo ? tau0 : tau;
    launch_discover_scan(a, p.lds_examples(g1), st);
  };
  const auto fold = [&] {
    launch_compact(b.cand, b.C, b.cnt, R, L, 0, b.cand, b.C, b.cnt, nullptr, b.C, st);
    launch_discover_tau(b.cand, b.C, b.cnt, R, L, tau, st);
  };
  chunked_example_scan(h, p, b, R, L, scan, fold, &h->discover_redone, out_keys, out_cnt, st);
}

// ---------------------------------------------------------------------------------
// distance matrix search (hx_search_matrix)
// ---------------------------------------------------------------------------------
// every refusal of the call, before any device work; the sample as the kernels take it
static std::vector<uint32_t> matrix_check(hx_index* h, const int64_t* rows, int S, int limit, float threshold) {
  HX_CHECK(h, "NULL argument");
  HX_CHECK(S >= 1 && S <= HX_MATRIX_MAX_SAMPLE, "search_matrix: sample out of range [1, 4096]");
  HX_CHECK(limit >= 1 && limit <= HX_MATRIX_MAX_LIMIT, "search_matrix: limit out of range [1, 1024]");
  HX_CHECK(rows, "NULL argument");
  HX_CHECK(!std::isnan(threshold), "search_matrix: the score threshold is NaN");
  std::vector<uint32_t> r((size_t)S);
  for (int i = 0; i < S; ++i) {
    HX_CHECK(rows[i] >= 0 && rows[i] < h->n, "search_matrix: sample row out of range");
    r[(size_t)i] = (uint32_t)rows[i];
  }
  std::vector<uint32_t> sorted = r;
  std::sort(sorted.begin(), sorted.end());
  HX_CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "search_matrix: a sample row is listed twice");
  return r;
}

// Keys leave with internal ids.  Synchronises `st` (the row list is uploaded from this frame).
static void search_matrix_dev(hx_index* h, const std::vector<uint32_t>& rows, int L, float threshold, uint64_t* out_keys,
                              int* out_cnt, hipStream_t st) {
  const int S = (int)rows.size();
  MatrixArgs a{};
  a.dense = h->dense;
  a.S = S;
  a.dim_pad = h->dim_pad;
  uint32_t* rows_dev = (uint32_t*)h->ws.get(WS_MATRIX_ROWS, (size_t)S * 4);
  HX_HIP(hipMemcpyAsync(rows_dev, rows.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
  a.rows = rows_dev;
  a.plane = (float*)h->ws.get(WS_MATRIX_PLANE, (size_t)S * S * 4);   // 64 MB at the cap, sized by S, freed with the index
  launch_matrix_scan(a, st);
  if (h->matrix_scan_only) zero_outputs(out_keys, out_cnt, S, L, st);
  else launch_matrix_select(a, threshold, (uint32_t)h->id_base, L, out_keys, out_cnt, st);
  HX_HIP(hipStreamSynchronize(st));
}

// ---------------------------------------------------------------------------------
// the frames of the entries
// ---------------------------------------------------------------------------------
// A device entry: run(mask count unknown, the caller's buffers), then the ids that cross the ABI.
template <typename Run>
static void example_entry_dev(hx_index* h, int N, int limit, uint64_t* keys_dev, int32_t* counts_dev, void* stream, Run&& run) {
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  run(-1, keys_dev, counts_dev, st);
  remap_out(h, keys_dev, (int64_t)N * limit, st);
  HX_HIP(hipStreamSynchronize(st));
}
// A *_host entry: the host mask (NULL = every row) counted -- no read-back -- and uploaded, run(mask_dev, its kept rows,
// the lists' buffers) for N lists of `limit` slots, the lists to the host.
struct OutSlots {
  int keys, cnt, sc, id;
};
constexpr OutSlots RECO_OUT{WS_RECO_OUT, WS_RECO_OCNT, WS_RECO_SC, WS_RECO_ID};
constexpr OutSlots MATRIX_OUT{WS_MATRIX_OUT, WS_MATRIX_OCNT, WS_MATRIX_SC, WS_MATRIX_ID};
template <typename Run>
static void example_entry_host(hx_index* h, const uint32_t* mask_host, int N, int limit, const OutSlots& slots,
                               float* scores_host, int64_t* ids_host, int32_t* counts_host, Run&& run) {
  h->set_device();
  hipStream_t st = nullptr;
  const int64_t n_out = (int64_t)N * limit;
  const int64_t kept = mask_host ? host_mask_count(h, mask_host) : -1;
  const uint32_t* mask_dev = mask_host ? host_mask_upload(h, mask_host, WS_RECO_MASK, st) : nullptr;
  uint64_t* keys = (uint64_t*)h->ws.get(slots.keys, (size_t)n_out * 8);
  int* cnt = (int*)h->ws.get(slots.cnt, (size_t)N * 4);
  run(mask_dev, kept, keys, cnt, st);
  results_to_host(h, keys, n_out, slots.sc, slots.id, scores_host, ids_host, st);
  HX_HIP(hipMemcpyAsync(counts_host, cnt, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
}

}  // namespace hx

extern "C" {

int hx_recommend(hx_index* h, int32_t strategy, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host,
                 const int8_t* ex_sign_host, const float* ex_vecs_host, const uint32_t* mask_dev, int64_t mask_rows,
                 int32_t limit, uint64_t* keys_dev, int32_t* counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(keys_dev && counts_dev, "NULL argument");
  const RecoCall c = reco_check(h, strategy, R, ex_indptr_host, ex_rows_host, ex_sign_host, ex_vecs_host, mask_dev, mask_rows,
                                limit);
  example_entry_dev(h, R, limit, keys_dev, counts_dev, stream, [&](int64_t kept, uint64_t* keys, int* cnt, hipStream_t st) {
    recommend_dev(h, strategy, R, c, ex_vecs_host, mask_dev, kept, limit, keys, cnt, st);
  });
  HX_CATCH
}

int hx_recommend_host(hx_index* h, int32_t strategy, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host,
                      const int8_t* ex_sign_host, const float* ex_vecs_host, const uint32_t* mask_host, int64_t mask_rows,
                      int32_t limit, float* scores_host, int64_t* ids_host, int32_t* counts_host) {
  HX_TRY
  HX_CHECK(scores_host && ids_host && counts_host, "NULL argument");
  const RecoCall c = reco_check(h, strategy, R, ex_indptr_host, ex_rows_host, ex_sign_host, ex_vecs_host, mask_host, mask_rows,
                                limit);
  example_entry_host(h, mask_host, R, limit, RECO_OUT, scores_host, ids_host, counts_host,
                     [&](const uint32_t* mask_dev, int64_t kept, uint64_t* keys, int* cnt, hipStream_t st) {
                       recommend_dev(h, strategy, R, c, ex_vecs_host, mask_dev, kept, limit, keys, cnt, st);
                     });
  HX_CATCH
}

int hx_discover(hx_index* h, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host, const float* ex_vecs_host,
                const int32_t* has_target_host, const uint32_t* mask_dev, int64_t mask_rows, int32_t limit,
                uint64_t* keys_dev, int32_t* counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(keys_dev && counts_dev, "NULL argument");
  const RecoCall c = discover_check(h, R, ex_indptr_host, ex_rows_host, ex_vecs_host, has_target_host, mask_dev, mask_rows,
                                    limit);
  example_entry_dev(h, R, limit, keys_dev, counts_dev, stream, [&](int64_t kept, uint64_t* keys, int* cnt, hipStream_t st) {
    discover_dev(h, R, c, ex_vecs_host, mask_dev, kept, limit, keys, cnt, st);
  });
  HX_CATCH
}

int hx_discover_host(hx_index* h, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host,
                     const float* ex_vecs_host, const int32_t* has_target_host, const uint32_t* mask_host, int64_t mask_rows,
                     int32_t limit, float* scores_host, int64_t* ids_host, int32_t* counts_host) {
  HX_TRY
  HX_CHECK(scores_host && ids_host && counts_host, "NULL argument");
  const RecoCall c = discover_check(h, R, ex_indptr_host, ex_rows_host, ex_vecs_host, has_target_host, mask_host, mask_rows,
                                    limit);
  example_entry_host(h, mask_host, R, limit, RECO_OUT, scores_host, ids_host, counts_host,
                     [&](const uint32_t* mask_dev, int64_t kept, uint64_t* keys, int* cnt, hipStream_t st) {
                       discover_dev(h, R, c, ex_vecs_host, mask_dev, kept, limit, keys, cnt, st);
                     });
  HX_CATCH
}

int hx_discover_redone(hx_index* h, int64_t* requests) {
  HX_TRY
  HX_CHECK(h && requests, "NULL argument");
  *requests = h->discover_redone;
  HX_CATCH
}

int hx_search_matrix(hx_index* h, const int64_t* rows_host, int32_t S, int32_t limit, float score_threshold,
                     uint64_t* keys_dev, int32_t* counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(keys_dev && counts_dev, "NULL argument");
  const std::vector<uint32_t> rows = matrix_check(h, rows_host, S, limit, score_threshold);
  example_entry_dev(h, S, limit, keys_dev, counts_dev, stream, [&](int64_t, uint64_t* keys, int* cnt, hipStream_t st) {
    search_matrix_dev(h, rows, limit, score_threshold, keys, cnt, st);
  });
  HX_CATCH
}

int hx_search_matrix_host(hx_index* h, const int64_t* rows_host, int32_t S, int32_t limit, float score_threshold,
                          float* scores_host, int64_t* ids_host, int32_t* counts_host) {
  HX_TRY
  HX_CHECK(scores_host && ids_host && counts_host, "NULL argument");
  const std::vector<uint32_t> rows = matrix_check(h, rows_host, S, limit, score_threshold);
  example_entry_host(h, nullptr, S, limit, MATRIX_OUT, scores_host, ids_host, counts_host,
                     [&](const uint32_t*, int64_t, uint64_t* keys, int* cnt, hipStream_t st) {
                       search_matrix_dev(h, rows, limit, score_threshold, keys, cnt, st);
                     });
  HX_CATCH
}

}  // extern "C"
