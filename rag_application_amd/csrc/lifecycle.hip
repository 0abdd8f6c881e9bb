// Host side of what removes, renumbers or rewrites stored rows: hx_truncate, per-point deletes (hx_retain_rows, DESIGN.md
// section 14), upsert by an existing id (hx_replace_rows, section 18) and persistence (hx_save / hx_load).  Every entry
// starts with a device synchronisation and ends with one: nothing here runs beside a query.  The kernels are in compact.hip
// and replace.hip; the payload columns take part through the hooks of paystore.hip (index.hpp).
#include "index.hpp"

#include <cstdio>
#include <string>

namespace hx {

// The weight range after a compaction or a splice: got = {min, max} (orderable u32) of the new_nnz weights the index now
// holds, as launch_minmax_f32 and the fused copies left them.  (track_weights_dev MERGES a batch's range: ingest.)
static void set_weight_range(hx_index* h, const uint32_t got[2], int64_t new_nnz) {
  if (new_nnz > 0 && got[0] <= got[1]) {
    h->sp_wmin = orderable_f32(got[0]);
    h->sp_wmax = orderable_f32(got[1]);
    h->sp_have_w = true;
  } else {
    h->sp_wmin = h->sp_wmax = 0.f;
    h->sp_have_w = false;
  }
}

// ---- per-point deletes ----------------------------------------------------------------------

// The kept rows of a host mask, for the chunk plan: rank -> row without the list itself (that one is built on the device).
struct KeepIndex {
  const uint32_t* m;
  int64_t n, nw;
  std::vector<int64_t> cum;          // set bits in front of word w; cum[nw] = the kept rows
  uint32_t word(int64_t w) const {
    uint32_t v = m[w];
    const int tail = (int)(n & 31);
    if (w == nw - 1 && tail) v &= (1u << tail) - 1u;
    return v;
  }
  KeepIndex(const uint32_t* mask, int64_t n_) : m(mask), n(n_), nw((n_ + 31) / 32), cum((size_t)((n_ + 31) / 32) + 1, 0) {
    for (int64_t w = 0; w < nw; ++w) cum[(size_t)w + 1] = cum[(size_t)w] + __builtin_popcount(word(w));
  }
  int64_t kept() const { return cum[(size_t)nw]; }
  int64_t kept_below(int64_t r) const {          // kept rows in [0, r), r <= n
    if (r >= n) return kept();
    const int64_t w = r >> 5;
    return cum[(size_t)w] + __builtin_popcount(word(w) & ((1u << (r & 31)) - 1u));
  }
  int64_t row_of(int64_t i) const {              // the i-th kept row, i < kept()
    const int64_t w = (std::upper_bound(cum.begin(), cum.end(), i) - cum.begin()) - 1;
    uint32_t v = word(w);
    for (int64_t k = i - cum[(size_t)w]; k > 0; --k) v &= v - 1u;
    return w * 32 + (__builtin_ffs((int)v) - 1);
  }
  int64_t first_removed() const {                // rows in front of it do not move
    for (int64_t w = 0; w < nw; ++w) {
      const uint32_t full = (w == nw - 1 && (n & 31)) ? (1u << (n & 31)) - 1u : 0xFFFFFFFFu;
      const uint32_t gone = ~word(w) & full;
      if (gone) return w * 32 + (__builtin_ffs((int)gone) - 1);
    }
    return n;
  }
};

// Bytes of the bounce buffer of a bounced chunk: the chunk is written there, read back and written into place while
// its source rows stream past -- three times its size between the two uses of a line, inside the 256 MiB Infinity Cache.
constexpr int64_t COMPACT_BOUNCE_BYTES = 32ll << 20;

struct CompactChunk {
  int64_t d0, d1;
  bool direct;
};
// Destination rows [first, count) in stream-ordered chunks (compact.hip): a chunk whose first source row lies at or
// past its end is gathered in place, any other goes through the bounce buffer, `chunk` rows at a time.
static std::vector<CompactChunk> compact_plan(const KeepIndex& k, int64_t first, int64_t count, int64_t chunk) {
  std::vector<CompactChunk> plan;
  for (int64_t d = first; d < count;) {
    const int64_t shift = k.row_of(d) - d;       // >= 1 from the first removed row on
    const bool direct = shift >= chunk;
    const int64_t e = std::min(count, d + (direct ? shift : chunk));
    plan.push_back({d, e, direct});
    d = e;
  }
  return plan;
}

// The compaction of a CSR of which `kept` documents stay (compact.hip), the delete side's SplicePlan: documents [0, f)
// stay where they are, f = min(first removed row, kept); the `docs` kept documents behind them -- rows[0, docs), the kept
// rows from `first` on -- move to base + off[j].  base = the offset of document f, moved = the postings behind it after the
// call.  The lengths and their exclusive prefix lie in `lenoff` (2 * (docs + 1) words) where the caller has such a buffer,
// in an allocation of the plan's own otherwise.
struct KeepPlan {
  int64_t f = 0, docs = 0, base = 0, moved = 0;
  const uint32_t* rows = nullptr;
  int64_t* off = nullptr;
  DevTmp own;
};
static void keep_plan(KeepPlan& k, const int64_t* indptr, int64_t first, const uint32_t* rows_first, int64_t kept,
                      int64_t* lenoff, hipStream_t st) {
  k.f = std::min(first, kept);
  k.docs = kept - k.f;
  k.rows = rows_first;
  HX_HIP(hipMemcpy(&k.base, indptr + k.f, 8, hipMemcpyDeviceToHost));
  if (k.docs == 0) return;
  if (!lenoff) {
    k.own.alloc((size_t)(k.docs + 1) * 8 * 2);
    lenoff = (int64_t*)k.own.p;
  }
  int64_t* len = lenoff;
  k.off = len + (k.docs + 1);
  HX_HIP(hipMemsetAsync(len + k.docs, 0, 8, st));
  launch_csr_keep_len(indptr, k.rows, k.docs, len, st);
  exclusive_scan_i64(len, k.off, k.docs, st);
  HX_HIP(hipMemcpy(&k.moved, k.off + k.docs, 8, hipMemcpyDeviceToHost));
}
// one 4-byte plane of the CSR's elements (the offsets are still the old ones): through `spare`, moved words
static void keep_apply_u32(const KeepPlan& k, const int64_t* indptr, uint32_t* plane, void* spare, hipStream_t st) {
  launch_csr_compact_u32(indptr, k.rows, k.off, k.docs, plane, (uint32_t*)spare, st);
  launch_copy_u32(spare, plane + k.base, k.moved, st);
}

static void retain_rows(hx_index* h, const uint32_t* keep, int64_t* n_removed) {
  const int64_t n = h->n;
  const KeepIndex k(keep, n);
  const int64_t count = k.kept();
  if (n_removed) *n_removed = n - count;
  if (count == n) return;                          // nothing to do: nothing touched, nothing invalidated
  HX_CHECK(h->sp_rows <= n, "hx_retain_rows: sparse vectors are pending for rows not added yet");
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  hipStream_t st = nullptr;
  const int64_t first = k.first_removed();
  const bool sparse = h->sp_rows > 0 && h->sp_indptr != nullptr;
  const int64_t kept_sp = sparse ? k.kept_below(h->sp_rows) : 0;   // kept documents that have a sparse row

  // ---- everything that can fail comes first: the row list, the plans, the temporaries, the CSR offsets ----
  struct Arr {
    void* p;
    int64_t rb;                      // row bytes; 4 = one scale per row
    std::vector<CompactChunk> plan;
  };
  std::vector<Arr> arrs;
  const std::vector<PayMoved> cols = pay_moved(h, n);    // the payload columns that cover every row; a lagging one is dropped
  if (count > 0) {
    for (const RowArray& a : row_arrays(h))
      if (a.p()) arrs.push_back({a.p(), a.rb, {}});
    for (const PayMoved& c : cols)
      for (uint32_t* p : {c.p0, c.p1})
        if (p) arrs.push_back({p, 4, {}});
  }
  int64_t bounce_bytes = 0;
  for (auto& a : arrs) {
    const int64_t chunk = h->compact_chunk > 0 ? h->compact_chunk : std::max<int64_t>(COMPACT_BOUNCE_BYTES / a.rb, 1);
    a.plan = compact_plan(k, first, count, chunk);
    for (const auto& c : a.plan)
      if (!c.direct) bounce_bytes = std::max(bounce_bytes, (c.d1 - c.d0) * a.rb);
  }
  uint32_t* rows = nullptr;
  if (count > 0) {
    const int64_t nw = (n + 31) / 32;
    uint32_t* dm = (uint32_t*)h->ws.get(WS_M_MASK, (size_t)nw * 4);
    HX_HIP(hipMemcpyAsync(dm, keep, (size_t)nw * 4, hipMemcpyHostToDevice, st));
    uint32_t* count_dev = nullptr;
    mask_rows_dev(h, dm, rows, count_dev, st);
  }
  const uint32_t* rows_first = rows ? rows + first : nullptr;     // the kept rows from the first removed one on
  DevTmp bounce;
  if (bounce_bytes > 0) bounce.alloc((size_t)bounce_bytes);
  // the list and text columns that cover every row (sections 17, 19): the head plane is in `arrs`; offsets and elements
  // go the sparse CSR's way
  struct CsrTmp {
    KeepPlan plan;
    DevTmp t0, t1;                   // spare buffers of the moved elements
  };
  std::vector<CsrTmp> col_tmp(cols.size());
  for (size_t i = 0; i < cols.size(); ++i) {
    CsrTmp& t = col_tmp[i];
    if (!cols[i].off) continue;
    keep_plan(t.plan, cols[i].off, first, rows_first, count, nullptr, st);
    if (t.plan.moved > 0) {
      t.t0.alloc((size_t)t.plan.moved * 4);
      if (cols[i].e1) t.t1.alloc((size_t)t.plan.moved * 4);
    }
  }
  // the sparse vectors: the documents [0, first) stay; the kept documents behind them move
  CsrTmp sp;
  int64_t new_nnz = 0;
  uint32_t* mm = nullptr;
  if (sparse && kept_sp > 0) {
    mm = (uint32_t*)h->ws.get(WS_SP_MM, 16);
    const int64_t m = kept_sp - std::min(first, kept_sp);
    keep_plan(sp.plan, h->sp_indptr, first, rows_first, kept_sp,
              m > 0 ? (int64_t*)h->ws.get(WS_C_LEN, (size_t)(m + 1) * 8 * 2) : nullptr, st);
    if (sp.plan.moved > 0) {
      sp.t0.alloc((size_t)sp.plan.moved * 4);
      sp.t1.alloc((size_t)sp.plan.moved * 4);
    }
    new_nnz = sp.plan.base + sp.plan.moved;
  }

  // ---- the rows move ----
  for (const auto& a : arrs) {
    uint8_t* p = (uint8_t*)a.p;
    for (const auto& c : a.plan) {
      const int64_t cnt = c.d1 - c.d0;
      void* dst = c.direct ? (void*)(p + c.d0 * a.rb) : bounce.p;
      if (a.rb == 4) launch_compact_u32(p, dst, rows + c.d0, cnt, st);
      else launch_compact_rows16(p, dst, a.rb, rows + c.d0, cnt, st);
      if (c.direct) continue;
      if (a.rb == 4) launch_copy_u32(bounce.p, p + c.d0 * 4, cnt, st);
      else launch_copy16(bounce.p, p + c.d0 * a.rb, cnt * a.rb, st);
    }
  }
  // (the per-row scales behind the last row are zero in a freshly grown buffer)
  if (h->q8_rinv) HX_HIP(hipMemsetAsync(h->q8_rinv + count, 0, (size_t)(n - count) * 4, st));
  if (h->q8s_scale) HX_HIP(hipMemsetAsync(h->q8s_scale + count, 0, (size_t)(n - count) * 4, st));
  uint32_t got[3] = {0xFFFFFFFFu, 0u, 0u};
  if (mm && new_nnz > 0) {
    const KeepPlan& p = sp.plan;
    HX_HIP(hipMemcpyAsync(mm, got, 12, hipMemcpyHostToDevice, st));
    launch_minmax_f32(h->sp_val, p.base, (float*)mm, st);         // the documents that stay where they are
    if (p.moved > 0) {               // (both planes in one launch, which also takes the range of the copied weights)
      launch_csr_compact(h->sp_indptr, p.rows, p.off, p.docs, h->sp_idx, h->sp_val, (int32_t*)sp.t0.p, (float*)sp.t1.p, mm, st);
      // (4-byte words: base need not be a multiple of 4 postings)
      launch_copy_u32(sp.t0.p, h->sp_idx + p.base, p.moved, st);
      launch_copy_u32(sp.t1.p, h->sp_val + p.base, p.moved, st);
    }
    HX_HIP(hipMemcpyAsync(got, mm, 12, hipMemcpyDeviceToHost, st));
  }
  if (sp.plan.docs > 0) launch_csr_new_indptr(h->sp_indptr + first, sp.plan.off, sp.plan.docs, sp.plan.base, st);
  for (size_t i = 0; i < cols.size(); ++i) {
    const KeepPlan& p = col_tmp[i].plan;
    if (!cols[i].off) continue;
    if (p.moved > 0) {
      keep_apply_u32(p, cols[i].off, cols[i].e0, col_tmp[i].t0.p, st);
      if (cols[i].e1) keep_apply_u32(p, cols[i].off, cols[i].e1, col_tmp[i].t1.p, st);
    }
    if (p.docs > 0) launch_csr_new_indptr(cols[i].off + first, p.off, p.docs, p.base, st);
    *cols[i].n_el = p.base + p.moved;
  }
  HX_HIP(hipDeviceSynchronize());

  // ---- the index of the kept rows ----
  h->n = count;
  pay_retained(h, n, count);
  h->tm_q8.rows = h->tm_q8s.rows = -1;
  if (sparse) {
    h->sp_rows = kept_sp;
    h->nnz = new_nnz;
    set_weight_range(h, got, new_nnz);
  }
  free_sparse_index(h);
  h->sparse_stale = true;
  auto& b = h->ids;
  b.row0.clear();
  b.gid0.clear();
  if (count > 0) {
    b.row0.push_back(0u);
    b.gid0.push_back((uint32_t)h->id_base);
  }
  b.end = count > 0 ? h->id_base + count : -1;
  b.next = -1;
  b.dirty = true;
}

// ---- upsert by an existing id ---------------------------------------------------------------

std::vector<uint32_t> replace_rows_checked(const int64_t* rows_host, int64_t m, int64_t limit, const char* who) {
  std::vector<uint32_t> r((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    HX_CHECK(rows_host[i] >= 0 && rows_host[i] < limit, std::string(who) + ": a row lies outside [0, count)");
    r[(size_t)i] = (uint32_t)rows_host[i];
  }
  std::vector<uint32_t> s(r);
  std::sort(s.begin(), s.end());
  HX_CHECK(std::adjacent_find(s.begin(), s.end()) == s.end(), std::string(who) + ": the rows must be unique");
  return r;
}

void splice_plan(SplicePlan& s, const int64_t* indptr, int64_t total, int64_t f, const uint32_t* rows_dev, int64_t m,
                 const int64_t* new_indptr_dev, hipStream_t st) {
  s.f = f;
  s.docs = total - f;
  s.map_.alloc((size_t)s.docs * 4);
  HX_HIP(hipMemsetAsync(s.map_.p, 0xFF, (size_t)s.docs * 4, st));
  launch_splice_map(rows_dev, m, f, s.docs, (uint32_t*)s.map_.p, st);
  s.lenoff.alloc((size_t)(s.docs + 1) * 8 * 2);
  int64_t* len = (int64_t*)s.lenoff.p;
  int64_t* off = len + (s.docs + 1);
  HX_HIP(hipMemsetAsync(len + s.docs, 0, 8, st));
  launch_csr_splice_len(indptr + f, s.map(), new_indptr_dev, s.docs, len, st);
  exclusive_scan_i64(len, off, s.docs, st);
  HX_HIP(hipStreamSynchronize(st));
  HX_HIP(hipMemcpy(&s.base, indptr + f, 8, hipMemcpyDeviceToHost));
  HX_HIP(hipMemcpy(&s.moved, off + s.docs, 8, hipMemcpyDeviceToHost));
}

static void replace_rows(hx_index* h, const int64_t* rows_host, int64_t m, const float* dense_host, const int64_t* indptr,
                         const int32_t* idx, const float* val) {
  const int64_t n = h->n;
  HX_CHECK(ids_identity(h) && h->ids.next < 0,
           "hx_replace_rows: the ids of this index were named with hx_set_next_id (a shard of a sharded collection): "
           "replacing its rows is not supported");
  HX_CHECK(h->sp_rows <= n, "hx_replace_rows: sparse vectors are pending for rows not added yet");
  const std::vector<uint32_t> rows = replace_rows_checked(rows_host, m, n, "hx_replace_rows");
  int64_t nnz_new = 0;
  if (indptr) {
    HX_CHECK(indptr[0] == 0, "indptr[0] must be 0");
    nnz_new = indptr[m];
    HX_CHECK(nnz_new >= 0, "negative nnz");
    HX_CHECK(nnz_new == 0 || (idx && val), "idx/val is NULL");
    for (int64_t r = 0; r < m; ++r) HX_CHECK(indptr[r + 1] >= indptr[r] && indptr[r + 1] <= nnz_new, "indptr not monotone");
  }
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  hipStream_t st = nullptr;
  DevTmp rows_dev_;
  rows_dev_.alloc((size_t)m * 4);
  HX_HIP(hipMemcpy(rows_dev_.p, rows.data(), (size_t)m * 4, hipMemcpyHostToDevice));
  const uint32_t* rows_dev = (const uint32_t*)rows_dev_.p;

  // ---- the sparse batch: uploaded beside the index and checked there, as hx_add_sparse checks its batch ----
  DevTmp nip, nidx, nval;
  if (indptr) {
    nip.alloc((size_t)(m + 1) * 8);
    nidx.alloc((size_t)nnz_new * 4);
    nval.alloc((size_t)nnz_new * 4);
    HX_HIP(hipMemcpy(nip.p, indptr, (size_t)(m + 1) * 8, hipMemcpyHostToDevice));
    if (nnz_new) {
      HX_HIP(hipMemcpy(nidx.p, idx, (size_t)nnz_new * 4, hipMemcpyHostToDevice));
      HX_HIP(hipMemcpy(nval.p, val, (size_t)nnz_new * 4, hipMemcpyHostToDevice));
      float lo = 0.f, hi = 0.f;
      check_sparse_batch_dev(h, (const int64_t*)nip.p, (const int32_t*)nidx.p, (const float*)nval.p, m, 0, nnz_new, indptr, idx,
                             &lo, &hi);
    }
  }

  // ---- the dense rows: derived in a staging block laid out as the stored arrays are (k_prep_rows as the add path
  // launches it), the batch's non-finite word read before anything stored changes ----
  HX_CHECK(!h->cand8 || (h->q8s && h->q8s_scale && h->s8_err), "int8 candidate copy enabled but not allocated");
  std::vector<RowArray> ra = row_arrays(h);
  // (staged and scattered as a file lists them, the derived copies behind the others)
  std::stable_partition(ra.begin(), ra.end(), [](const RowArray& a) { return a.in_file; });
  std::vector<DevTmp> stage(ra.size());
  std::vector<void*> stage_p;
  for (size_t i = 0; i < ra.size(); ++i) {
    stage[i].alloc((size_t)(m * ra[i].rb));
    stage_p.push_back(stage[i].p);
  }
  const int64_t CH = 65536;
  float* raw = (float*)h->ws.get(WS_RAW, (size_t)std::min(m, CH) * h->dim * 4);
  int* chk = rows_check_begin(h, st);
  for (int64_t r0 = 0; r0 < m; r0 += CH) {
    const int64_t k = std::min(CH, m - r0);
    HX_HIP(hipMemcpy(raw, dense_host + r0 * h->dim, (size_t)k * h->dim * 4, hipMemcpyHostToDevice));
    PrepRowsArgs c = prep_rows_args(h, ra, stage_p.data(), r0);
    c.raw = raw;
    c.n = k;
    c.nonfinite = chk;
    launch_prep_rows(c, st);
    if (r0 + k >= m) rows_check_fetch(h, chk, st);
    HX_HIP(hipStreamSynchronize(st));
  }
  rows_check_end(h, chk, st);

  // ---- the CSR's plan: offsets, spare buffers, capacity ----
  SplicePlan sp;
  DevTmp idx2, val2;
  int64_t new_nnz = h->nnz;
  uint32_t* mm = nullptr;
  if (indptr) {
    const int64_t rmin = *std::min_element(rows.begin(), rows.end()), rmax = *std::max_element(rows.begin(), rows.end());
    if (rmax >= h->sp_rows) {          // trailing rows that never got a sparse vector: empty documents, as finalize pads them
      reserve_sparse(h, n, h->nnz);
      std::vector<int64_t> tail((size_t)(n - h->sp_rows), h->nnz);
      if (h->sp_rows == 0) {
        const int64_t zero = 0;
        HX_HIP(hipMemcpy(h->sp_indptr, &zero, 8, hipMemcpyHostToDevice));
      }
      HX_HIP(hipMemcpy(h->sp_indptr + h->sp_rows + 1, tail.data(), tail.size() * 8, hipMemcpyHostToDevice));
      h->sp_rows = n;
      h->sparse_stale = true;
    }
    splice_plan(sp, h->sp_indptr, h->sp_rows, rmin, rows_dev, m, (const int64_t*)nip.p, st);
    new_nnz = sp.base + sp.moved;
    HX_CHECK(new_nnz < 0xFFFFFFFFll, "nnz per shard must stay below 2^32");
    if (sp.moved > 0) {
      idx2.alloc((size_t)sp.moved * 4);
      val2.alloc((size_t)sp.moved * 4);
    }
    reserve_sparse(h, h->sp_rows, new_nnz);
    mm = (uint32_t*)h->ws.get(WS_SP_MM, 16);
  }

  // ---- the stored arrays change ----
  for (size_t i = 0; i < ra.size(); ++i) {
    if (ra[i].rb == 4) launch_scatter_u32(stage_p[i], ra[i].p(), rows_dev, m, st);
    else launch_scatter_rows16(stage_p[i], ra[i].p(), ra[i].rb, rows_dev, m, st);
  }
  uint32_t got[3] = {0xFFFFFFFFu, 0u, 0u};
  if (indptr) {
    if (new_nnz > 0) {
      HX_HIP(hipMemcpyAsync(mm, got, 12, hipMemcpyHostToDevice, st));
      launch_minmax_f32(h->sp_val, sp.base, (float*)mm, st);        // the documents in front of the first replaced one
      if (sp.moved > 0) {
        launch_csr_splice(h->sp_indptr + sp.f, sp.map(), (const int64_t*)nip.p, sp.off(), sp.docs, h->sp_idx, h->sp_val,
                          (const int32_t*)nidx.p, (const float*)nval.p, (int32_t*)idx2.p, (float*)val2.p, mm, st);
        launch_copy_u32(idx2.p, h->sp_idx + sp.base, sp.moved, st);
        launch_copy_u32(val2.p, h->sp_val + sp.base, sp.moved, st);
      }
      HX_HIP(hipMemcpyAsync(got, mm, 12, hipMemcpyDeviceToHost, st));
    }
    launch_csr_new_indptr(h->sp_indptr + sp.f, sp.off(), sp.docs, sp.base, st);
  }
  HX_HIP(hipDeviceSynchronize());

  // ---- what was derived from the old rows ----
  h->tm_q8.rows = h->tm_q8s.rows = -1;
  h->mv.have = 0;                      // the gathered copies of the mask view: a masked query reads the new rows
  h->mv.tm_q8.rows = h->mv.tm_q8s.rows = -1;
  if (indptr) {
    h->nnz = new_nnz;
    set_weight_range(h, got, new_nnz);
    free_sparse_index(h);
    h->sparse_stale = true;
  }
}

// ---- persistence -------------------------------------------------
// The reference asks Qdrant for on-disk storage (qdrant_handler.py:47-55, 62: on_disk=True,
// memmap_threshold).  A collection is written as one file: header, then the device arrays as they
// stand (derived vectors are stored, not re-derived: loading reproduces the index bit for bit) and
// the doc-major sparse CSR; the inverted index is rebuilt on load (K9, ~1.4 s per 10^9 postings).
namespace {
struct HxFileHeader {
  char magic[8];             // "HXIDX\0\0\2" (version 1: no id-block table, n_blocks reads 0)
  int32_t dim, n_pre, psize[3], n_blocks;
  int64_t id_base, n, sp_rows, nnz;
};
const char HX_MAGIC[8] = {'H', 'X', 'I', 'D', 'X', 0, 0, 2};
constexpr size_t HX_IO_CHUNK = (size_t)64 << 20;

struct File {
  FILE* f;
  explicit File(const char* path, const char* mode) : f(fopen(path, mode)) {
    if (!f) throw Error(std::string("cannot open ") + path);
  }
  ~File() { if (f) fclose(f); }
};
void dev_to_file(FILE* f, const void* dev, size_t bytes, std::vector<char>& buf) {
  for (size_t o = 0; o < bytes; o += HX_IO_CHUNK) {
    const size_t m = std::min(HX_IO_CHUNK, bytes - o);
    HX_HIP(hipMemcpy(buf.data(), (const char*)dev + o, m, hipMemcpyDeviceToHost));
    HX_CHECK(fwrite(buf.data(), 1, m, f) == m, "short write");
  }
}
void file_to_dev(FILE* f, void* dev, size_t bytes, std::vector<char>& buf) {
  for (size_t o = 0; o < bytes; o += HX_IO_CHUNK) {
    const size_t m = std::min(HX_IO_CHUNK, bytes - o);
    HX_CHECK(fread(buf.data(), 1, m, f) == m, "short read: truncated index file");
    HX_HIP(hipMemcpy((char*)dev + o, buf.data(), m, hipMemcpyHostToDevice));
  }
}
}  // namespace

}  // namespace hx

extern "C" {

// Roll the collection back to its first n_rows rows (a batch that one shard of a sharded collection could not
// store is undone on the shards that did store it; qdrant_handler.py:190-193 upserts a batch as one request).
int hx_truncate(hx_index* h, int64_t n_rows) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  HX_CHECK(n_rows >= 0 && n_rows <= h->n, "hx_truncate: n_rows out of range [0, count]");
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  h->ids.next = -1;
  pay_truncate(h, n_rows);
  if (n_rows == h->n && h->sp_rows <= n_rows) return 0;
  h->n = n_rows;
  h->tm_q8.rows = h->tm_q8s.rows = -1;
  if (h->sp_rows > n_rows) {
    int64_t nnz = 0;
    if (n_rows > 0) HX_HIP(hipMemcpy(&nnz, h->sp_indptr + n_rows, 8, hipMemcpyDeviceToHost));
    h->sp_rows = n_rows;
    h->nnz = nnz;
  }
  // the inverted index: a base that reaches past the cut is rebuilt, the tail always is.  The weight range stays
  // as it was: an upper bound of the remaining weights is all the select pass needs.
  free_sparse_ix(h->sp_tail);
  if (h->sp_base.n_docs > h->sp_rows) free_sparse_ix(h->sp_base);
  h->sparse_stale = true;
  auto& b = h->ids;
  while (!b.row0.empty() && (int64_t)b.row0.back() >= n_rows) {
    b.row0.pop_back();
    b.gid0.pop_back();
  }
  b.end = b.row0.empty() ? -1 : (int64_t)b.gid0.back() + (n_rows - (int64_t)b.row0.back());
  b.dirty = true;
  HX_CATCH
}

int hx_retain_rows(hx_index* h, const uint32_t* keep_host, int64_t mask_rows, int64_t* n_removed) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  HX_CHECK(mask_rows >= 0, "hx_retain_rows: mask_rows < 0");
  HX_CHECK(keep_host || mask_rows == 0, "hx_retain_rows: mask is NULL");
  HX_CHECK(mask_rows == h->n, "mask_rows must equal the index's row count (hx_count)");
  HX_CHECK(ids_identity(h) && h->ids.next < 0,
           "hx_retain_rows: the ids of this index were named with hx_set_next_id (a shard of a sharded collection): "
           "renumbering them is not supported");
  if (mask_rows == 0) {
    if (n_removed) *n_removed = 0;
    return 0;
  }
  retain_rows(h, keep_host, n_removed);
  HX_CATCH
}

int hx_replace_rows(hx_index* h, const int64_t* rows_host, int64_t m, const float* dense_host, const int64_t* indptr_host,
                    const int32_t* idx_host, const float* val_host) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  HX_CHECK(m >= 0, "hx_replace_rows: m < 0");
  HX_CHECK(m == 0 || (rows_host && dense_host), "hx_replace_rows: rows / dense is NULL");
  if (m == 0) return 0;
  replace_rows(h, rows_host, m, dense_host, indptr_host, idx_host, val_host);
  HX_CATCH
}

int hx_save(hx_index* h, const char* path) {
  HX_TRY
  HX_CHECK(h && path, "NULL argument");
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  File fl(path, "wb");
  HxFileHeader hd{};
  memcpy(hd.magic, HX_MAGIC, 8);
  hd.dim = h->dim;
  hd.n_pre = h->n_pre;
  for (int p = 0; p < 3; ++p) hd.psize[p] = h->psize[p];
  hd.id_base = h->id_base;
  hd.n = h->n;
  hd.sp_rows = h->sp_rows;
  hd.nnz = h->nnz;
  hd.n_blocks = (int32_t)h->ids.row0.size();
  HX_CHECK(fwrite(&hd, sizeof hd, 1, fl.f) == 1, "short write");
  if (hd.n_blocks) {         // the id-block table: row0 column, then gid0 column
    HX_CHECK(fwrite(h->ids.row0.data(), 4, (size_t)hd.n_blocks, fl.f) == (size_t)hd.n_blocks, "short write");
    HX_CHECK(fwrite(h->ids.gid0.data(), 4, (size_t)hd.n_blocks, fl.f) == (size_t)hd.n_blocks, "short write");
  }
  std::vector<char> buf(HX_IO_CHUNK);
  for (const RowArray& a : row_arrays(h))
    if (a.in_file) dev_to_file(fl.f, a.p(), (size_t)h->n * (size_t)a.rb, buf);
  if (h->sp_rows > 0) {
    dev_to_file(fl.f, h->sp_indptr, ((size_t)h->sp_rows + 1) * 8, buf);
    dev_to_file(fl.f, h->sp_idx, (size_t)h->nnz * 4, buf);
    dev_to_file(fl.f, h->sp_val, (size_t)h->nnz * 4, buf);
  }
  HX_CHECK(fflush(fl.f) == 0, "flush failed");
  HX_CATCH
}

int hx_load(const char* path, int32_t device, hx_index** out) {
  HX_TRY
  HX_CHECK(path && out, "NULL argument");
  File fl(path, "rb");
  HxFileHeader hd{};
  HX_CHECK(fread(&hd, sizeof hd, 1, fl.f) == 1, "short read: not an index file");
  HX_CHECK(memcmp(hd.magic, HX_MAGIC, 7) == 0 && (hd.magic[7] == 1 || hd.magic[7] == 2),
           "not an hx index file (bad magic / version)");
  if (hd.magic[7] == 1) hd.n_blocks = 0;     // version 1: ids are id_base + row
  // The header is not trusted: every size is checked against the limits of the add path and against the
  // length of the file BEFORE anything is allocated (a corrupt count must not become a huge hipMalloc).
  HX_CHECK(hd.n >= 0 && hd.sp_rows >= 0 && hd.nnz >= 0 && hd.n_pre >= 0 && hd.n_pre <= 3, "corrupt header");
  HX_CHECK(hd.dim >= 1 && hd.dim <= 4096, "corrupt header: dim");
  HX_CHECK(hd.id_base >= 0 && hd.id_base + hd.n < 0xFFFFFFFFll, "corrupt header: row ids");
  HX_CHECK(hd.nnz < 0xFFFFFFFFll && hd.sp_rows <= hd.n && (hd.sp_rows > 0 || hd.nnz == 0), "corrupt header: sparse counts");
  {
    hx_index shape;            // the row widths hx_create gives an index of the header's sizes: what a row takes in the file
    shape.dim = hd.dim;
    shape.dim_pad = (int)round_up(hd.dim, 64);
    shape.dim_pad8 = (int)round_up(hd.dim, 128);
    shape.n_pre = hd.n_pre;
    for (int p = 0; p < hd.n_pre; ++p) {
      HX_CHECK(hd.psize[p] >= 64 && hd.psize[p] <= hd.dim && hd.psize[p] % 64 == 0, "corrupt header: prefix sizes");
      shape.psize[p] = hd.psize[p];
    }
    int64_t per_row = 0;
    for (const RowArray& a : row_arrays(&shape))
      if (a.in_file) per_row += a.rb;
    HX_CHECK(hd.n_blocks >= 0 && hd.n_blocks <= hd.n, "corrupt header: id blocks");
    int64_t want = (int64_t)sizeof hd + (int64_t)hd.n_blocks * 8 + hd.n * per_row;
    if (hd.sp_rows > 0) want += (hd.sp_rows + 1) * 8 + hd.nnz * 8;
    HX_CHECK(fseek(fl.f, 0, SEEK_END) == 0, "cannot seek");
    const int64_t have = (int64_t)ftell(fl.f);
    HX_CHECK(fseek(fl.f, (long)sizeof hd, SEEK_SET) == 0, "cannot seek");
    HX_CHECK(have == want, "index file length does not match its header (truncated or corrupt)");
  }
  // the id-block table: both columns ascend strictly from row 0, a block's ids end before the next block's begin,
  // the last id stays below 2^32 - 1
  std::vector<uint32_t> row0((size_t)hd.n_blocks), gid0((size_t)hd.n_blocks);
  if (hd.n_blocks) {
    HX_CHECK(fread(row0.data(), 4, row0.size(), fl.f) == row0.size(), "short read: truncated index file");
    HX_CHECK(fread(gid0.data(), 4, gid0.size(), fl.f) == gid0.size(), "short read: truncated index file");
    HX_CHECK(row0[0] == 0, "corrupt index file: id blocks");
    for (size_t k = 0; k < row0.size(); ++k) {
      const int64_t len = (k + 1 < row0.size() ? (int64_t)row0[k + 1] : hd.n) - (int64_t)row0[k];
      HX_CHECK(len >= 1 && (int64_t)gid0[k] + len < 0xFFFFFFFFll, "corrupt index file: id blocks");
      HX_CHECK(k + 1 == row0.size() || (int64_t)gid0[k] + len <= (int64_t)gid0[k + 1], "corrupt index file: id blocks");
    }
  } else if (hd.n > 0) {
    row0.assign(1, 0u);
    gid0.assign(1, (uint32_t)hd.id_base);
  }
  hx_index* h = nullptr;
  const int rc = hx_create(hd.dim, hd.psize, hd.n_pre, device, hd.id_base, &h);
  if (rc != 0) return rc;
  try {
    h->set_device();
    if (!row0.empty()) {
      h->ids.end = (int64_t)gid0.back() + (hd.n - (int64_t)row0.back());
      h->ids.row0.swap(row0);
      h->ids.gid0.swap(gid0);
      h->ids.dirty = true;
    }
    std::vector<char> buf(HX_IO_CHUNK);
    reserve_rows(h, hd.n);
    for (const RowArray& a : row_arrays(h))
      if (a.in_file) file_to_dev(fl.f, a.p(), (size_t)hd.n * (size_t)a.rb, buf);
    h->n = hd.n;
    // the candidate copy is derived data (not in the file): one pass over the stored rows
    if (h->cand8) launch_requant_rows(h->dense, h->dim_pad, h->dim_pad8, hd.n, h->q8s, h->q8s_scale, h->s8_err, nullptr);
    if (hd.sp_rows > 0) {
      reserve_sparse(h, hd.sp_rows, hd.nnz);
      file_to_dev(fl.f, h->sp_indptr, ((size_t)hd.sp_rows + 1) * 8, buf);
      file_to_dev(fl.f, h->sp_idx, (size_t)hd.nnz * 4, buf);
      file_to_dev(fl.f, h->sp_val, (size_t)hd.nnz * 4, buf);
      // what the add path guarantees and the kernels rely on: monotone indptr from 0 to nnz, term ids in
      // [0, 2^31), finite values
      int* bad = (int*)h->ws.get(WS_MISC, 4);
      HX_HIP(hipMemset(bad, 0, 4));
      launch_csr_check(h->sp_indptr, h->sp_idx, hd.sp_rows, 0, hd.nnz, bad, nullptr);
      int hbad = 0;
      HX_HIP(hipMemcpy(&hbad, bad, 4, hipMemcpyDeviceToHost));
      HX_CHECK(hbad == 0, "corrupt index file: sparse CSR is inconsistent");
      // term ids unique within a row (hx_add_sparse enforces it; the exact pass finds a query term with ONE ballot)
      constexpr int LONG_CAP = 4096;
      int64_t* long_rows = (int64_t*)h->ws.get(WS_LONG_ROWS, (size_t)LONG_CAP * 8 + 8);
      int* n_long = (int*)(long_rows + LONG_CAP);
      HX_HIP(hipMemset(n_long, 0, 4));
      launch_csr_unique(h->sp_indptr, h->sp_idx, hd.sp_rows, bad, long_rows, LONG_CAP, n_long, nullptr);
      int hn_long = 0;
      HX_HIP(hipMemcpy(&hbad, bad, 4, hipMemcpyDeviceToHost));
      HX_HIP(hipMemcpy(&hn_long, n_long, 4, hipMemcpyDeviceToHost));
      HX_CHECK(hbad == 0, "corrupt index file: a sparse vector repeats a term id");
      if (hn_long > 0) {            // the rows too long for the wave compare: sorted on the host
        std::vector<int64_t> rows;
        if (hn_long <= LONG_CAP) {
          rows.resize((size_t)hn_long);
          HX_HIP(hipMemcpy(rows.data(), long_rows, rows.size() * 8, hipMemcpyDeviceToHost));
        } else {                    // more of them than the device list holds (hx_add_sparse accepts any number): find
                                    // them all from the offsets -- a valid file, not a corrupt one
          std::vector<int64_t> ip((size_t)hd.sp_rows + 1);
          HX_HIP(hipMemcpy(ip.data(), h->sp_indptr, ip.size() * 8, hipMemcpyDeviceToHost));
          for (int64_t r = 0; r < hd.sp_rows; ++r)
            if (ip[(size_t)r + 1] - ip[(size_t)r] > CSR_UNIQUE_WAVE_MAX) rows.push_back(r);
        }
        std::vector<int32_t> ids;
        for (int64_t r : rows) {
          int64_t be[2];
          HX_HIP(hipMemcpy(be, h->sp_indptr + r, 16, hipMemcpyDeviceToHost));
          ids.resize((size_t)(be[1] - be[0]));
          HX_HIP(hipMemcpy(ids.data(), h->sp_idx + be[0], ids.size() * 4, hipMemcpyDeviceToHost));
          std::sort(ids.begin(), ids.end());
          HX_CHECK(std::adjacent_find(ids.begin(), ids.end()) == ids.end(), "corrupt index file: a sparse vector repeats a term id");
        }
      }
      track_weights_dev(h, h->sp_val, hd.nnz, nullptr);
      h->sp_rows = hd.sp_rows;
      h->nnz = hd.nnz;
      h->sparse_stale = true;
    }
  } catch (...) {
    (void)hx_destroy(h);
    throw;
  }
  *out = h;
  HX_CATCH
}

}  // extern "C"
