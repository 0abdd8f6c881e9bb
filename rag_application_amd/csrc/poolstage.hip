// Host side of the stages over the query's pool (DESIGN.md sections 20, 21, 23, 27) and of every *_host entry of the hybrid
// query: the query front that leaves the pool on the device, the grouped, MMR, rerank and boosted stages as hx_group /
// hx_mmr / hx_maxsim / hx_formula take them, and the six hx_hybrid_query_*host* entries.  The query itself is engine.hip's
// (hybrid_query_dev, masked_query_dev); the kernels are in group.hip, mmr.hip, maxsim.hip and formula.hip.
#include "index.hpp"

#include <numeric>
#include <string>
#include <utility>

namespace hx {

// ---- the query front of the *_host entries ------------------------------------------------------------------------------
// The refusals every entry begins with, in this order.  outs_ok: the entry's own result pointers, which share the first
// refusal's text.
static void check_host_args(hx_index* h, const float* qd, const int64_t* qip, int32_t B, const hx_params* p, bool outs_ok) {
  HX_CHECK(h && qd && qip && outs_ok && B > 0, "bad argument");
  HX_CHECK(p != nullptr, "params is NULL");
}
// ... and those of an entry that takes an optional mask, in front of them
static void check_host_args(hx_index* h, const uint32_t* mask_host, int64_t mask_rows, const float* qd, const int64_t* qip,
                            int32_t B, const hx_params* p, bool outs_ok) {
  HX_CHECK(h, "NULL argument");
  HX_CHECK(!mask_host || mask_rows == h->n, "mask_rows must equal the index's row count (hx_count)");
  check_host_args(h, qd, qip, B, p, outs_ok);
}

// The lists of a query on the device, internal ids: [B x L] keys and their counts; dq = the uploaded dense queries.
struct Pool {
  float* dq;
  uint64_t* keys;
  int* cnt;
  int L;
  std::vector<int32_t> six;          // the sorted terms: the uploads read them until the caller synchronises
  std::vector<float> sv;
};

// The query of a *_host entry, mask_host NULL = every row: the checks on p and on the sparse queries, the upload, the query.
// The lists are p's -- final_limit slots -- and stay on the device.  result_slots: slots per query of what the entry hands
// out when that is not the lists themselves (0 then).
static Pool query_front(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv, int32_t B,
                        const hx_params* p, const uint32_t* mask_host, int result_slots, hipStream_t st) {
  check_params(p);
  h->set_device();
  const int64_t kept = mask_host ? host_mask_count(h, mask_host) : -1;
  const int64_t nnz = qip[B];
  HX_CHECK(qip[0] == 0 && nnz >= 0, "bad query indptr");
  // sort each query's terms by id (the spec's summation order), reject duplicates
  std::vector<int32_t> six((size_t)nnz);
  std::vector<float> sv((size_t)nnz);
  std::vector<int> ord;
  for (int b = 0; b < B; ++b) {
    const int64_t s = qip[b], e = qip[b + 1];
    HX_CHECK(e >= s && e <= nnz, "bad query indptr");
    ord.resize((size_t)(e - s));
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return qix[s + x] < qix[s + y]; });
    for (size_t i = 0; i < ord.size(); ++i) {
      six[(size_t)s + i] = qix[s + ord[i]];
      sv[(size_t)s + i] = qv[s + ord[i]];
      HX_CHECK(six[(size_t)s + i] >= 0, "sparse index out of range");
      HX_CHECK(i == 0 || six[(size_t)s + i] != six[(size_t)s + i - 1], "duplicate sparse index in query");
    }
  }
  Pool q{};
  q.six = std::move(six);
  q.sv = std::move(sv);
  q.L = p->final_limit;
  q.dq = (float*)h->ws.get(WS_H_QD, (size_t)B * h->dim * 4);
  int64_t* dip = (int64_t*)h->ws.get(WS_H_QIP, (size_t)(B + 1) * 8);
  int32_t* dix = (int32_t*)h->ws.get(WS_H_QIX, (size_t)std::max<int64_t>(nnz, 1) * 4);
  float* dv = (float*)h->ws.get(WS_H_QV, (size_t)std::max<int64_t>(nnz, 1) * 4);
  q.keys = (uint64_t*)h->ws.get(WS_H_OUT, (size_t)B * q.L * 8);
  q.cnt = (int*)h->ws.get(WS_H_OCNT, (size_t)B * 4);
  // results_to_host's two slots, sized here: a first call allocates them ahead of the query's own buffers, as it always has
  // (profiles/query_split_10m.txt: allocated behind them, the B = 64 host call measured 0.02-0.05 ms longer)
  h->ws.get(WS_H_SC, (size_t)B * std::max(q.L, result_slots) * 4);
  h->ws.get(WS_H_ID, (size_t)B * std::max(q.L, result_slots) * 8);
  HX_HIP(hipMemcpyAsync(q.dq, qd, (size_t)B * h->dim * 4, hipMemcpyHostToDevice, st));
  HX_HIP(hipMemcpyAsync(dip, qip, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
  if (nnz) {
    HX_HIP(hipMemcpyAsync(dix, q.six.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    HX_HIP(hipMemcpyAsync(dv, q.sv.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  if (kept < 0 || kept == h->n)
    hybrid_query_dev(h, q.dq, dip, dix, dv, B, p, q.keys, q.cnt, st);
  else
    masked_query_dev(h, q.dq, dip, dix, dv, B, p, host_mask_upload(h, mask_host, WS_M_MASK, st), kept, q.keys, q.cnt, st);
  return q;
}

// hx_hybrid_query_host and its masked form (mask_host NULL = every row)
static void query_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv, int32_t B,
                       const hx_params* p, const uint32_t* mask_host, float* scores, int64_t* ids, int32_t* counts) {
  check_host_args(h, qd, qip, B, p, scores && ids && counts);
  hipStream_t st = nullptr;
  const Pool q = query_front(h, qd, qip, qix, qv, B, p, mask_host, 0, st);
  results_to_host(h, q.keys, (int64_t)B * q.L, WS_H_SC, WS_H_ID, scores, ids, st);
  HX_HIP(hipMemcpyAsync(counts, q.cnt, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
}

// ---- what the four stage entries share ------------------------------------------------------------------------------------
// A stage entry runs the query for its POOL -- final_limit = the pool size -- and hands out what its stage makes of it; the
// stage reads internal ids, so it runs before results_to_host.
static void check_mode(const hx_params* p) {
  HX_CHECK(p->mode == HX_MODE_TREE || p->mode == HX_MODE_H1, "unknown mode");
}
constexpr const char* CANDIDATES_RANGE = "candidates_limit must be 0 (the whole pool) or in [1, the mode's pool size]";
// p with final_limit = the pool: `requested` lists slots, 0 = all the mode's two lists can hold (the caller's params are
// never written)
static hx_params pool_params(const hx_params* p, int32_t requested, const char* range_refusal) {
  check_mode(p);
  const int64_t other = p->mode == HX_MODE_TREE ? p->rrf_limit : p->sparse_limit;
  const int64_t pool_max = std::min<int64_t>((int64_t)p->dense_limit + other, MAX_LIMIT);
  HX_CHECK(requested >= 0 && requested <= pool_max && pool_max >= 1, range_refusal);
  hx_params pool = *p;
  pool.final_limit = requested ? requested : (int32_t)pool_max;
  return pool;
}
// mask_root_only: the query runs unmasked and the stage reads the mask as its eligible rows.  Returns that mask, taken
// from mask_host, or NULL.
static const uint32_t* take_root_mask(const hx_params* p, const char* stage, int32_t root_only, const uint32_t*& mask_host) {
  check_mode(p);
  HX_CHECK(root_only == 0 || root_only == 1, std::string(stage) + ": mask_root_only must be 0 or 1");
  HX_CHECK(!(mask_host && root_only && p->mode == HX_MODE_H1),
           std::string(stage) + ": a root-only mask belongs to the tree query's root: use HX_MODE_TREE (or mask_root_only = 0)");
  return root_only ? std::exchange(mask_host, nullptr) : nullptr;
}
static const uint32_t* root_mask_dev(hx_index* h, const uint32_t* root_mask, hipStream_t st) {
  return root_mask ? host_mask_upload(h, root_mask, WS_M_MASK, st) : nullptr;
}

// ---- grouped search ----------------------------------------------------------------------------
// the checks of hx_group on its sizes and its column, before any device work; returns the column's cells
static const uint32_t* group_plane(hx_index* h, int32_t col, int32_t n_groups, int32_t group_size) {
  HX_CHECK(n_groups >= 1 && group_size >= 1 && (int64_t)n_groups * group_size <= MAX_LIMIT,
           "group: n_groups and group_size must be at least 1 and n_groups * group_size at most 2048");
  const hx_index::PayCol& c = pay_col(h, col);
  HX_CHECK(c.kind == HX_PAY_U32, "group: the column kind must be HX_PAY_U32 (keyword codes or bools)");
  HX_CHECK(c.filled == h->n, "group: the column is not filled to the index's row count (hx_count)");
  return c.p0;
}
static void group_enqueue(hx_index* h, const uint32_t* p0, const uint64_t* keys, const uint64_t* ikeys, int stride,
                          const int* counts, int B, int n_groups, int group_size, uint64_t* out, uint32_t* codes,
                          int* group_counts, hipStream_t st) {
  GroupArgs g{};
  g.keys = keys;
  g.ikeys = ikeys;
  g.stride = stride;
  g.counts = counts;
  g.p0 = p0;
  g.n_rows = h->n;
  g.id_base = (uint32_t)h->id_base;
  g.n_groups = n_groups;
  g.group_size = group_size;
  g.out = out;
  g.group_codes = codes;
  g.group_counts = group_counts;
  launch_group_select(g, B, st);
}

// ---- MMR search -------------------------------------------------------------------------------
// the checks of hx_mmr on its sizes, before any device work
static void mmr_check(int32_t limit, float diversity) {
  HX_CHECK(limit >= 1 && limit <= HX_MMR_MAX_LIMIT, "mmr: limit out of range [1, 256]");
  HX_CHECK(diversity >= 0.0f && diversity <= 1.0f, "mmr: diversity must be in [0, 1]");   // (false for a NaN)
}
static void mmr_enqueue(hx_index* h, const uint64_t* keys, const uint64_t* ikeys, int stride, const int* counts, int B,
                        int limit, float diversity, const uint32_t* eligible, uint64_t* out_keys, float* out_values,
                        int* out_counts, hipStream_t st) {
  HX_CHECK(h->dim_pad <= 4096, "mmr: rows wider than 4096 floats");
  MmrArgs m{};
  m.keys = keys;
  m.ikeys = ikeys;
  m.stride = stride;
  m.counts = counts;
  m.rows = h->dense;
  m.dim_pad = (int)h->dim_pad;
  m.n_rows = h->n;
  m.id_base = (uint32_t)h->id_base;
  m.eligible = eligible;
  m.limit = limit;
  m.diversity = diversity;
  m.out_keys = out_keys;
  m.out_values = out_values;
  m.out_counts = out_counts;
  launch_mmr_select(m, B, st);
}

// ---- late-interaction rerank ---------------------------------------------------------------------
// every refusal of hx_maxsim, before any device work; returns the token column
static const hx_index::PayCol& maxsim_check(hx_index* h, int32_t col, int32_t stride, int32_t B, const int64_t* q_indptr_host,
                                            int32_t limit) {
  HX_CHECK(B >= 1, "maxsim: B < 1");
  HX_CHECK(stride >= 1 && stride <= MAX_LIMIT, "maxsim: stride out of range [1, 2048]");
  HX_CHECK(limit >= 1 && limit <= MAX_LIMIT, "maxsim: limit out of range [1, 2048]");
  HX_CHECK(q_indptr_host[0] == 0, "maxsim: the query token offsets start at 0");
  for (int b = 0; b < B; ++b) {
    const int64_t tq = q_indptr_host[b + 1] - q_indptr_host[b];
    HX_CHECK(tq >= 1 && tq <= HX_MAXSIM_MAX_QTOKENS, "maxsim: a query holds 1 to 64 tokens");
  }
  const hx_index::PayCol& c = pay_col(h, col);
  HX_CHECK(c.kind == HX_PAY_TOKENS, "maxsim: the column kind must be HX_PAY_TOKENS");
  HX_CHECK(c.filled == h->n, "maxsim: the column is not filled to the index's row count (hx_count)");
  return c;
}
// out_keys [B x limit] and out_counts [B] as hx_maxsim hands them out; first (may be NULL) = the scores the pool carried
static void maxsim_enqueue(hx_index* h, const hx_index::PayCol& c, const uint64_t* keys, const uint64_t* ikeys, int stride,
                           const int* counts, int B, const int8_t* q8, const float* qscale, const int64_t* q_indptr,
                           const uint32_t* eligible, int limit, uint64_t* out_keys, int* out_counts, float* first,
                           hipStream_t st) {
  MaxsimArgs m{};
  m.keys = keys;
  m.ikeys = ikeys;
  m.stride = stride;
  m.counts = counts;
  m.head = c.p0;
  m.off = c.off;
  m.words = c.e0;
  m.dim_t = c.dim_t;
  m.n_rows = h->n;
  m.id_base = (uint32_t)h->id_base;
  m.eligible = eligible;
  m.q8 = q8;
  m.qscale = qscale;
  m.q_indptr = q_indptr;
  m.pos_keys = (uint64_t*)h->ws.get(WS_MS_POS, (size_t)B * stride * 8);
  if (h->n == 0) {                       // (no row, no column arrays: nothing is eligible)
    HX_HIP(hipMemsetAsync(out_keys, 0, (size_t)B * limit * 8, st));
    HX_HIP(hipMemsetAsync(out_counts, 0, (size_t)B * 4, st));
    if (first) launch_fill_f32(first, (int64_t)B * limit, -__builtin_inff(), st);
    return;
  }
  launch_maxsim_score(m, B, st);
  launch_compact(m.pos_keys, stride, nullptr, B, std::min(limit, stride), 0, out_keys, limit, out_counts, nullptr, stride, st);
  launch_maxsim_finish(keys, stride, out_keys, first, B, limit, st);
}

// ---- score-boosting search ------------------------------------------------------------------------
// the checks of hx_formula on its sizes, then every refusal that concerns the program and its planes (formula_lower), before
// any device work
static void formula_check(hx_index* h, int32_t stride, int32_t B, int32_t limit, const hx_formula_op* ops, int32_t n_ops,
                          const uint32_t* const* planes, int32_t n_planes, FormulaArgs& f) {
  HX_CHECK(B >= 1, "formula: B < 1");
  HX_CHECK(stride >= 1 && stride <= MAX_LIMIT, "formula: stride out of range [1, 2048]");
  HX_CHECK(limit >= 1 && limit <= MAX_LIMIT, "formula: limit out of range [1, 2048]");
  formula_lower(h, ops, n_ops, n_planes, f);
  HX_CHECK(n_planes == 0 || planes, "NULL argument");
  for (int i = 0; i < n_planes; ++i) HX_CHECK(planes[i] != nullptr, "NULL argument");
}
// f: lowered by formula_lower; planes: n_planes device planes; out_base may be NULL
static void formula_enqueue(hx_index* h, FormulaArgs& f, const uint32_t* const* planes, int n_planes, const uint64_t* keys,
                            const uint64_t* ikeys, int stride, const int* counts, int B, int limit, float threshold,
                            const uint32_t* eligible, uint64_t* out_keys, int* out_pos, float* out_base, int* out_counts,
                            int* out_dropped, hipStream_t st) {
  for (int i = 0; i < n_planes; ++i) f.planes[i] = planes[i];
  f.keys = keys;
  f.ikeys = ikeys;
  f.counts = counts;
  f.eligible = eligible;
  f.out_keys = out_keys;
  f.out_pos = out_pos;
  f.out_base = out_base;
  f.out_counts = out_counts;
  f.out_dropped = out_dropped;
  f.n_rows = h->n;
  f.id_base = (uint32_t)h->id_base;
  f.stride = stride;
  f.limit = limit;
  f.threshold = threshold;
  f.has_threshold = threshold == threshold;
  launch_formula(f, B, st);
}

}  // namespace hx

extern "C" {

int hx_hybrid_query_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix,
                         const float* qv, int32_t B, const hx_params* p, float* scores, int64_t* ids,
                         int32_t* counts) {
  HX_TRY
  query_host(h, qd, qip, qix, qv, B, p, nullptr, scores, ids, counts);
  HX_CATCH
}

int hx_hybrid_query_host_masked(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv,
                                int32_t B, const hx_params* p, const uint32_t* mask_host, int64_t mask_rows,
                                float* scores, int64_t* ids, int32_t* counts) {
  HX_TRY
  HX_CHECK(h && mask_host, "NULL argument");
  HX_CHECK(mask_rows == h->n, "mask_rows must equal the index's row count (hx_count)");
  query_host(h, qd, qip, qix, qv, B, p, mask_host, scores, ids, counts);
  HX_CATCH
}

int hx_group(hx_index* h, int32_t col, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
             int32_t n_groups, int32_t group_size, uint64_t* out_keys_dev, uint32_t* group_codes_dev,
             int32_t* group_counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && keys_dev && out_keys_dev && group_codes_dev && group_counts_dev, "NULL argument");
  HX_CHECK(B >= 1, "group: B < 1");
  HX_CHECK(stride >= 1 && stride <= MAX_LIMIT, "group: stride out of range [1, 2048]");
  const uint32_t* p0 = group_plane(h, col, n_groups, group_size);
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  const uint64_t* ikeys = remap_in(h, keys_dev, (int64_t)B * stride, st);
  group_enqueue(h, p0, keys_dev, ikeys, stride, counts_dev, B, n_groups, group_size, out_keys_dev, group_codes_dev,
                group_counts_dev, st);
  HX_CATCH
}

// ---- a ranked list filtered by a row mask and / or a score threshold ---------------------------
int hx_list_keep(hx_index* h, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
                 const uint32_t* mask_dev, int64_t mask_rows, const float* thr_dev, int32_t limit,
                 uint64_t* out_keys_dev, int32_t* out_counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && keys_dev && out_keys_dev && out_counts_dev, "NULL argument");
  HX_CHECK(mask_dev || thr_dev, "list_keep: a mask or thresholds (or both) are needed");
  HX_CHECK(B >= 1, "list_keep: B < 1");
  HX_CHECK(stride >= 1 && stride <= CAND_CAP, "list_keep: stride out of range [1, 8192]");
  HX_CHECK(limit >= 1 && limit <= CAND_CAP, "list_keep: limit out of range [1, 8192]");
  HX_CHECK(!mask_dev || mask_rows == h->n, "list_keep: mask_rows must equal the index's row count (hx_count)");
  const uintptr_t in0 = (uintptr_t)keys_dev, in1 = in0 + (size_t)B * stride * 8;
  const uintptr_t out0 = (uintptr_t)out_keys_dev, out1 = out0 + (size_t)B * limit * 8;
  HX_CHECK(out1 <= in0 || in1 <= out0, "list_keep: the output must not overlap the input");
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  ListKeepArgs a{};
  a.keys = keys_dev;
  a.ikeys = mask_dev ? remap_in(h, keys_dev, (int64_t)B * stride, st) : keys_dev;   // (ids matter under a mask only)
  a.stride = stride;
  a.counts = counts_dev;
  a.B = B;
  a.mask = mask_dev;
  a.n_rows = h->n;
  a.id_base = (uint32_t)h->id_base;
  a.thr = thr_dev;
  a.limit = limit;
  a.out = out_keys_dev;
  a.out_counts = out_counts_dev;
  launch_list_keep(a, st);
  HX_CATCH
}

int hx_hybrid_query_groups_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv,
                                int32_t B, const hx_params* p, const uint32_t* mask_host, int64_t mask_rows, int32_t col,
                                int32_t group_pool, int32_t n_groups, int32_t group_size, float* scores, int64_t* ids,
                                uint32_t* group_codes, int32_t* group_counts) {
  HX_TRY
  check_host_args(h, mask_host, mask_rows, qd, qip, B, p, scores && ids);
  HX_CHECK(group_codes && group_counts, "bad argument");
  const hx_params pool = pool_params(p, group_pool, "group_pool must be 0 (the whole pool) or in [1, the mode's pool size]");
  check_params(&pool);
  const uint32_t* p0 = group_plane(h, col, n_groups, group_size);
  hipStream_t st = nullptr;
  const int GS = n_groups * group_size;
  const Pool q = query_front(h, qd, qip, qix, qv, B, &pool, mask_host, GS, st);
  uint64_t* gk = (uint64_t*)h->ws.get(WS_G_KEYS, (size_t)B * GS * 8);
  uint32_t* gc = (uint32_t*)h->ws.get(WS_G_CODES, (size_t)B * n_groups * 4);
  int* gn = (int*)h->ws.get(WS_G_CNT, (size_t)B * 4);
  group_enqueue(h, p0, q.keys, q.keys, q.L, q.cnt, B, n_groups, group_size, gk, gc, gn, st);
  results_to_host(h, gk, (int64_t)B * GS, WS_H_SC, WS_H_ID, scores, ids, st);
  HX_HIP(hipMemcpyAsync(group_codes, gc, (size_t)B * n_groups * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipMemcpyAsync(group_counts, gn, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CATCH
}

int hx_mmr(hx_index* h, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B, int32_t limit,
           float diversity, const uint32_t* eligible_dev, int64_t eligible_rows, uint64_t* out_keys_dev,
           float* out_values_dev, int32_t* out_counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && keys_dev && out_keys_dev && out_values_dev && out_counts_dev, "NULL argument");
  HX_CHECK(B >= 1, "mmr: B < 1");
  HX_CHECK(stride >= 1 && stride <= MAX_LIMIT, "mmr: stride out of range [1, 2048]");
  mmr_check(limit, diversity);
  HX_CHECK(!eligible_dev || eligible_rows == h->n, "mmr: eligible_rows must equal the index's row count (hx_count)");
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  const uint64_t* ikeys = remap_in(h, keys_dev, (int64_t)B * stride, st);
  mmr_enqueue(h, keys_dev, ikeys, stride, counts_dev, B, limit, diversity, eligible_dev, out_keys_dev, out_values_dev,
              out_counts_dev, st);
  HX_CATCH
}

int hx_hybrid_query_mmr_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv,
                             int32_t B, const hx_params* p, const uint32_t* mask_host, int64_t mask_rows,
                             int32_t mask_root_only, int32_t candidates_limit, int32_t limit, float diversity,
                             float* scores, int64_t* ids, float* values, int32_t* counts) {
  HX_TRY
  check_host_args(h, mask_host, mask_rows, qd, qip, B, p, scores && ids);
  HX_CHECK(values && counts, "bad argument");
  const uint32_t* root_mask = take_root_mask(p, "mmr", mask_root_only, mask_host);
  const hx_params pool = pool_params(p, candidates_limit, CANDIDATES_RANGE);
  mmr_check(limit, diversity);
  hipStream_t st = nullptr;
  const Pool q = query_front(h, qd, qip, qix, qv, B, &pool, mask_host, limit, st);
  const uint64_t* keys = q.keys;
  const int* cnt = q.cnt;
  if (pool.mode == HX_MODE_H1) {         // relevance is the dense cosine: the fused list through the re-score stage
    uint64_t* rk = (uint64_t*)h->ws.get(WS_MMR_POOL, (size_t)B * q.L * 8);
    int* rc = (int*)h->ws.get(WS_MMR_PCNT, (size_t)B * 4);
    rescore(h, q.dq, B, 0, q.keys, q.L, q.cnt, q.L, rk, rc, st);
    keys = rk;
    cnt = rc;
  }
  const uint32_t* elig = root_mask_dev(h, root_mask, st);
  uint64_t* mk = (uint64_t*)h->ws.get(WS_MMR_KEYS, (size_t)B * limit * 8);
  float* mv = (float*)h->ws.get(WS_MMR_VAL, (size_t)B * limit * 4);
  int* mn = (int*)h->ws.get(WS_MMR_CNT, (size_t)B * 4);
  mmr_enqueue(h, keys, keys, q.L, cnt, B, limit, diversity, elig, mk, mv, mn, st);
  results_to_host(h, mk, (int64_t)B * limit, WS_H_SC, WS_H_ID, scores, ids, st);
  HX_HIP(hipMemcpyAsync(values, mv, (size_t)B * limit * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipMemcpyAsync(counts, mn, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CATCH
}

int hx_formula(hx_index* h, const hx_formula_op* ops_host, int32_t n_ops, const uint32_t* const* planes_dev,
               int32_t n_planes, int64_t plane_rows, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev,
               int32_t B, int32_t limit, float score_threshold, const uint32_t* eligible_dev, int64_t eligible_rows,
               uint64_t* out_keys_dev, int32_t* out_pos_dev, int32_t* out_counts_dev, int32_t* out_dropped_dev,
               void* stream) {
  HX_TRY
  HX_CHECK(h && ops_host && keys_dev && out_keys_dev && out_pos_dev && out_counts_dev && out_dropped_dev, "NULL argument");
  FormulaArgs f{};
  formula_check(h, stride, B, limit, ops_host, n_ops, planes_dev, n_planes, f);
  HX_CHECK(n_planes == 0 || plane_rows == h->n, "formula: plane_rows must equal the index's row count (hx_count)");
  HX_CHECK(!eligible_dev || eligible_rows == h->n, "formula: eligible_rows must equal the index's row count (hx_count)");
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  const uint64_t* ikeys = remap_in(h, keys_dev, (int64_t)B * stride, st);
  formula_enqueue(h, f, planes_dev, n_planes, keys_dev, ikeys, stride, counts_dev, B, limit, score_threshold, eligible_dev,
                  out_keys_dev, out_pos_dev, nullptr, out_counts_dev, out_dropped_dev, st);
  HX_CATCH
}

int hx_hybrid_query_formula_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv,
                                 int32_t B, const hx_params* p, const uint32_t* mask_host, int64_t mask_rows,
                                 int32_t mask_root_only, int32_t candidates_limit, const hx_formula_op* ops_host,
                                 int32_t n_ops, const uint32_t* const* planes_host, int32_t n_planes, int32_t limit,
                                 float score_threshold, float* scores, int64_t* ids, float* base_scores, int32_t* counts,
                                 int32_t* dropped) {
  HX_TRY
  check_host_args(h, mask_host, mask_rows, qd, qip, B, p, scores && ids);
  HX_CHECK(base_scores && counts && dropped, "bad argument");
  const uint32_t* root_mask = take_root_mask(p, "formula", mask_root_only, mask_host);
  const hx_params pool = pool_params(p, candidates_limit, CANDIDATES_RANGE);
  FormulaArgs f{};
  formula_check(h, pool.final_limit, B, limit, ops_host, n_ops, planes_host, n_planes, f);
  hipStream_t st = nullptr;
  const Pool q = query_front(h, qd, qip, qix, qv, B, &pool, mask_host, limit, st);
  const int64_t nw = (h->n + 31) / 32;
  const uint32_t* elig = root_mask_dev(h, root_mask, st);
  const uint32_t* planes[HX_FORMULA_MAX_PLANES] = {};
  if (n_planes) {
    uint32_t* dp = (uint32_t*)h->ws.get(WS_FORMULA_PLANES, (size_t)n_planes * std::max<int64_t>(nw, 1) * 4);
    for (int i = 0; i < n_planes; ++i) {
      if (nw) HX_HIP(hipMemcpyAsync(dp + (int64_t)i * nw, planes_host[i], (size_t)nw * 4, hipMemcpyHostToDevice, st));
      planes[i] = dp + (int64_t)i * nw;
    }
  }
  uint64_t* fk = (uint64_t*)h->ws.get(WS_FORMULA_KEYS, (size_t)B * limit * 8);
  int* fp = (int*)h->ws.get(WS_FORMULA_POS, (size_t)B * limit * 4);
  float* fb = (float*)h->ws.get(WS_FORMULA_BASE, (size_t)B * limit * 4);
  int* fn = (int*)h->ws.get(WS_FORMULA_CNT, (size_t)B * 4);
  int* fd = (int*)h->ws.get(WS_FORMULA_DROP, (size_t)B * 4);
  formula_enqueue(h, f, planes, n_planes, q.keys, q.keys, q.L, q.cnt, B, limit, score_threshold, elig, fk, fp, fb, fn, fd, st);
  results_to_host(h, fk, (int64_t)B * limit, WS_H_SC, WS_H_ID, scores, ids, st);
  HX_HIP(hipMemcpyAsync(base_scores, fb, (size_t)B * limit * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipMemcpyAsync(counts, fn, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipMemcpyAsync(dropped, fd, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CATCH
}

int hx_maxsim(hx_index* h, int32_t col, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
              const int8_t* q8_dev, const float* qscale_dev, const int64_t* q_indptr_dev, const int64_t* q_indptr_host,
              const uint32_t* eligible_dev, int64_t eligible_rows, int32_t limit, uint64_t* out_keys_dev,
              int32_t* out_counts_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && keys_dev && q8_dev && qscale_dev && q_indptr_dev && q_indptr_host && out_keys_dev && out_counts_dev,
           "NULL argument");
  const hx_index::PayCol& c = maxsim_check(h, col, stride, B, q_indptr_host, limit);
  HX_CHECK(!eligible_dev || eligible_rows == h->n, "maxsim: eligible_rows must equal the index's row count (hx_count)");
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  const uint64_t* ikeys = remap_in(h, keys_dev, (int64_t)B * stride, st);
  maxsim_enqueue(h, c, keys_dev, ikeys, stride, counts_dev, B, q8_dev, qscale_dev, q_indptr_dev, eligible_dev, limit,
                 out_keys_dev, out_counts_dev, nullptr, st);
  HX_CATCH
}

int hx_hybrid_query_rerank_host(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv,
                                int32_t B, const hx_params* p, const uint32_t* mask_host, int64_t mask_rows,
                                int32_t mask_root_only, int32_t candidates_limit, int32_t col, const int8_t* q8_host,
                                const float* qscale_host, const int64_t* qtok_indptr_host, int32_t limit, float* scores,
                                int64_t* ids, float* first_scores, int32_t* counts) {
  HX_TRY
  check_host_args(h, mask_host, mask_rows, qd, qip, B, p, scores && ids);
  HX_CHECK(q8_host && qscale_host && qtok_indptr_host && first_scores && counts, "bad argument");
  const uint32_t* root_mask = take_root_mask(p, "rerank", mask_root_only, mask_host);
  const hx_params pool = pool_params(p, candidates_limit, CANDIDATES_RANGE);
  const hx_index::PayCol& tok = maxsim_check(h, col, pool.final_limit, B, qtok_indptr_host, limit);
  hipStream_t st = nullptr;
  const Pool q = query_front(h, qd, qip, qix, qv, B, &pool, mask_host, limit, st);
  const uint32_t* elig = root_mask_dev(h, root_mask, st);
  const int64_t nt = qtok_indptr_host[B];
  int8_t* q8 = (int8_t*)h->ws.get(WS_MS_Q8, (size_t)nt * tok.dim_t);
  float* qs = (float*)h->ws.get(WS_MS_QS, (size_t)nt * 4);
  int64_t* qtip = (int64_t*)h->ws.get(WS_MS_QIP, (size_t)(B + 1) * 8);
  HX_HIP(hipMemcpyAsync(q8, q8_host, (size_t)nt * tok.dim_t, hipMemcpyHostToDevice, st));
  HX_HIP(hipMemcpyAsync(qs, qscale_host, (size_t)nt * 4, hipMemcpyHostToDevice, st));
  HX_HIP(hipMemcpyAsync(qtip, qtok_indptr_host, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
  uint64_t* mk = (uint64_t*)h->ws.get(WS_MS_KEYS, (size_t)B * limit * 8);
  float* mf = (float*)h->ws.get(WS_MS_FIRST, (size_t)B * limit * 4);
  int* mn = (int*)h->ws.get(WS_MS_CNT, (size_t)B * 4);
  maxsim_enqueue(h, tok, q.keys, q.keys, q.L, q.cnt, B, q8, qs, qtip, elig, limit, mk, mn, mf, st);
  results_to_host(h, mk, (int64_t)B * limit, WS_H_SC, WS_H_ID, scores, ids, st);
  HX_HIP(hipMemcpyAsync(first_scores, mf, (size_t)B * limit * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipMemcpyAsync(counts, mn, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CATCH
}

}  // extern "C"
