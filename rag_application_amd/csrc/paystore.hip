// Host side of the payload index (DESIGN.md sections 15, 17, 19, 26): the storage of the columns, every hx_payload_* entry,
// and what the lifecycle of the rows (lifecycle.hip) does to a column.  The kernels are in payload.hip, paytext.hip and
// paynested.hip, the splice of a list or text column in replace.hip.
#include "index.hpp"

namespace hx {

using PayCol = hx_index::PayCol;

PayCol& pay_col(hx_index* h, int32_t col) {
  for (auto& c : h->pay)
    if (c.id == col) return c;
  throw Error("payload: unknown column " + std::to_string(col));
}

void pay_free(PayCol& c) {
  for (void* q : {(void*)c.p0, (void*)c.p1, (void*)c.off, (void*)c.e0, (void*)c.e1})
    if (q) (void)hipFree(q);
  c.p0 = c.p1 = c.e0 = c.e1 = nullptr;
  c.off = nullptr;
  c.filled = c.cap = c.n_el = c.el_cap = 0;
}

// ---- what the lifecycle does to a column -----------------------------------------------------------------------------------
void pay_truncate(hx_index* h, int64_t n_rows) {
  for (auto& c : h->pay) {
    if (c.csr() && c.filled > n_rows)      // (the elements past off[n_rows] are dead)
      HX_HIP(hipMemcpy(&c.n_el, c.off + n_rows, 8, hipMemcpyDeviceToHost));
    c.filled = std::min(c.filled, n_rows);
  }
}

std::vector<PayMoved> pay_moved(hx_index* h, int64_t n) {
  std::vector<PayMoved> cols;
  for (auto& c : h->pay)
    if (c.filled == n) cols.push_back({c.p0, c.p1, c.csr() ? c.off : nullptr, c.e0, c.e1, &c.n_el});
  return cols;
}

void pay_retained(hx_index* h, int64_t n, int64_t count) {
  for (size_t i = h->pay.size(); i-- > 0;) {
    if (h->pay[i].filled == n) {
      h->pay[i].filled = count;
      continue;
    }
    pay_free(h->pay[i]);
    h->pay.erase(h->pay.begin() + (long)i);
  }
}

// ---- the word planes of doubles ----------------------------------------------------------------------------------------------
// nan_refusal: what a NaN cell is refused with (NULL: the caller's cells are taken as they are)
static void split_f64(const void* cells, int64_t n, std::vector<uint32_t>& lo, std::vector<uint32_t>& hi,
                      const char* nan_refusal = nullptr) {
  const uint64_t* v = (const uint64_t*)cells;
  const double* d = (const double*)cells;
  lo.resize((size_t)n);
  hi.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (nan_refusal) HX_CHECK(d[i] == d[i], nan_refusal);
    lo[(size_t)i] = (uint32_t)v[i];
    hi[(size_t)i] = (uint32_t)(v[i] >> 32);
  }
}
static void join_f64(const std::vector<uint32_t>& lo, const std::vector<uint32_t>& hi, void* cells) {
  uint64_t* out = (uint64_t*)cells;
  for (size_t i = 0; i < lo.size(); ++i) out[i] = ((uint64_t)hi[i] << 32) | lo[i];
}

// ---- growth ------------------------------------------------------------------------------------------------------------------
// a device array of `want` entries that holds the first `keep` of `old` (the new one is made before the old one goes)
template <typename T>
static T* pay_grown(const T* old, int64_t keep, int64_t want) {
  T* a = nullptr;
  if (hipMalloc((void**)&a, (size_t)want * sizeof(T)) != hipSuccess) throw Error("payload: out of device memory");
  if (keep > 0 && hipMemcpy(a, old, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
    (void)hipFree(a);
    throw Error("payload: device copy failed");
  }
  return a;
}

// Room for `rows` rows and, in a list or text column, `els` words per element plane -- all or nothing: every new array is
// allocated and filled before an old one is freed, and a failure leaves the column as it was.
static void pay_reserve(hx_index* h, PayCol& c, int64_t rows, int64_t els) {
  uint32_t *np0 = nullptr, *np1 = nullptr, *ne0 = nullptr, *ne1 = nullptr;
  int64_t* noff = nullptr;
  int64_t nc = c.cap, nec = c.el_cap;
  try {
    if (rows > c.cap || (c.csr() && !c.off)) {
      nc = round_up(std::max<int64_t>(std::max(rows, c.cap * 2), h->cap), 256);
      HX_HIP(hipDeviceSynchronize());
      np0 = pay_grown(c.p0, c.filled, nc);
      if (c.kind == HX_PAY_F64) np1 = pay_grown(c.p1, c.filled, nc);
      if (c.csr()) noff = pay_grown(c.off, c.off ? c.filled + 1 : 0, nc + 1);
    }
    if (els > c.el_cap) {
      nec = round_up(std::max<int64_t>(els, c.el_cap * 2), 256);
      HX_HIP(hipDeviceSynchronize());
      ne0 = pay_grown(c.e0, c.n_el, nec);
      if (c.kind == HX_PAY_LIST_F64) ne1 = pay_grown(c.e1, c.n_el, nec);
    }
  } catch (...) {
    for (void* q : {(void*)np0, (void*)np1, (void*)noff, (void*)ne0, (void*)ne1})
      if (q) (void)hipFree(q);
    throw;
  }
  if (np0) {
    for (void* q : {(void*)c.p0, (void*)c.p1, (void*)c.off})
      if (q) (void)hipFree(q);
    c.p0 = np0;
    c.p1 = np1;
    c.off = noff;
    c.cap = nc;
  }
  if (ne0) {
    if (c.e0) (void)hipFree(c.e0);
    if (c.e1) (void)hipFree(c.e1);
    c.e0 = ne0;
    c.e1 = ne1;
    c.el_cap = nec;
  }
}

// ---- list and text cells as a column stores them ---------------------------------------------------------------------------
// The checked cells of n list rows: heads[n] as the head plane keeps them (missing / null / 0 = a list), off[n + 1] = the
// rows' offsets in elements from `base`, and -- of doubles only: codes are stored as they come -- lo / hi = the elements'
// word planes.  Refuses element counts that do not sum to n_values or pass `room`, NaNs and reserved codes.  Returns the
// element count.
static int64_t pay_list_pack(const uint32_t* heads_host, int64_t n, const void* values_host, int64_t n_values, int64_t base,
                             int kind, int64_t room, std::vector<uint32_t>& heads, std::vector<int64_t>& off,
                             std::vector<uint32_t>& lo, std::vector<uint32_t>& hi) {
  heads.resize((size_t)n);
  off.resize((size_t)n + 1);
  int64_t total = 0;
  off[0] = base;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t hd = heads_host[i];
    const bool is_list = hd < HX_PAY_U32_NULL;
    heads[(size_t)i] = is_list ? 0u : hd;
    if (is_list) total += hd;
    HX_CHECK(total <= n_values, "payload: the element counts of the heads do not sum to n_values");
    off[(size_t)i + 1] = base + total;
  }
  HX_CHECK(total == n_values, "payload: the element counts of the heads do not sum to n_values");
  HX_CHECK(total <= room, "payload: a list column holds fewer than 2^31 elements");
  if (kind == HX_PAY_LIST_F64) {
    split_f64(values_host, total, lo, hi, "payload: a list element is a NaN");
  } else {
    const uint32_t* v = (const uint32_t*)values_host;
    for (int64_t i = 0; i < total; ++i) HX_CHECK(v[i] < HX_PAY_U32_NULL, "payload: a list element is a reserved code");
  }
  return total;
}

// The checked cells of n text rows: off[n + 1] = the rows' offsets in 32-bit words from `base`, words = the rows' bytes
// one after another, each row padded with zero bytes to a word.  Refuses lengths that do not sum to n_bytes.
static void pay_text_pack(const uint32_t* heads_host, int64_t n, const void* bytes_host, int64_t n_bytes, int64_t base,
                          std::vector<int64_t>& off, std::vector<uint32_t>& words) {
  off.resize((size_t)n + 1);
  off[0] = base;
  int64_t total = 0, n_words = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t hd = heads_host[i];
    if (hd < HX_PAY_U32_NULL) {
      total += hd;
      n_words += ((int64_t)hd + 3) / 4;
    }
    HX_CHECK(total <= n_bytes, "payload: the byte lengths of the heads do not sum to n_bytes");
    off[(size_t)i + 1] = base + n_words;
  }
  HX_CHECK(total == n_bytes, "payload: the byte lengths of the heads do not sum to n_bytes");
  words.assign((size_t)n_words, 0u);
  const uint8_t* src = (const uint8_t*)bytes_host;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t hd = heads_host[i];
    if (hd >= HX_PAY_U32_NULL || hd == 0u) continue;
    std::memcpy((uint8_t*)words.data() + (size_t)(off[(size_t)i] - base) * 4, src, hd);
    src += hd;
  }
}

// words of a token row of td tokens: td x dim_t bytes, td scales, zero words up to a multiple of four (16 bytes)
static int64_t pay_token_words(int64_t td, int dim_t) { return td * (dim_t / 4) + round_up(td, 4); }

// The checked cells of n token rows (hx.h states the layout): off[n + 1] = the rows' offsets in 32-bit words from `base`,
// words = the rows one after another.  Refuses counts that do not sum to n_tokens, a column of 2^31 words or more (before
// a token is read) and a scale that is negative or not finite.
static void pay_tokens_pack(const uint32_t* heads_host, int64_t n, const int8_t* x8, const float* scales, int64_t n_tokens,
                            int dim_t, int64_t base, std::vector<int64_t>& off, std::vector<uint32_t>& words) {
  off.resize((size_t)n + 1);
  off[0] = base;
  int64_t total = 0, n_words = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t hd = heads_host[i];
    if (hd < HX_PAY_U32_NULL) {
      total += hd;
      n_words += pay_token_words(hd, dim_t);
    }
    HX_CHECK(total <= n_tokens, "payload: the token counts of the heads do not sum to n_tokens");
    off[(size_t)i + 1] = base + n_words;
  }
  HX_CHECK(total == n_tokens, "payload: the token counts of the heads do not sum to n_tokens");
  HX_CHECK(base + n_words <= 0x7FFFFFFFll, "payload: a token column holds fewer than 2^31 words");
  for (int64_t t = 0; t < total; ++t)
    HX_CHECK(scales[t] >= 0.0f && scales[t] <= 3.402823466e38f, "payload: a token scale is negative or not finite");
  words.assign((size_t)n_words, 0u);
  int64_t t = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t hd = heads_host[i];
    if (hd >= HX_PAY_U32_NULL || hd == 0u) continue;
    uint8_t* row = (uint8_t*)(words.data() + (off[(size_t)i] - base));
    std::memcpy(row, x8 + t * dim_t, (size_t)hd * dim_t);
    std::memcpy(row + (size_t)hd * dim_t, scales + t, (size_t)hd * 4);
    t += hd;
  }
}

// Store the checked cells of rows [filled, filled + n) of a list or text column: heads[n] as the head plane keeps them,
// off[n + 1] = the rows' offsets (off[0] = n_el), e0_host / e1_host = `total` new words per element plane (e1_host: the
// high words of a HX_PAY_LIST_F64 column, NULL otherwise).  Every allocation comes before the column changes.
static void pay_store_csr(hx_index* h, PayCol& c, const uint32_t* heads, const int64_t* off, int64_t n, const void* e0_host,
                          const void* e1_host, int64_t total) {
  const bool f64 = c.kind == HX_PAY_LIST_F64;
  if (n == 0) return;
  h->set_device();
  const int64_t want = c.filled + n, want_el = c.n_el + total;
  pay_reserve(h, c, want, want_el);
  // (the cells behind `filled` and the elements behind n_el are dead until `filled` moves: a failed copy changes nothing)
  HX_HIP(hipMemcpy(c.p0 + c.filled, heads, (size_t)n * 4, hipMemcpyHostToDevice));
  HX_HIP(hipMemcpy(c.off + c.filled, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
  if (total > 0) {
    HX_HIP(hipMemcpy(c.e0 + c.n_el, e0_host, (size_t)total * 4, hipMemcpyHostToDevice));
    if (f64) HX_HIP(hipMemcpy(c.e1 + c.n_el, e1_host, (size_t)total * 4, hipMemcpyHostToDevice));
  }
  c.filled = want;
  c.n_el = want_el;
}

// Replace the checked cells of m stored rows of a list or text column: heads[m] as the head plane keeps them, noff[m + 1] =
// the new rows' offsets from 0, e0_host / e1_host = their `total` words per element plane.  The heads are scattered; offsets
// and elements are spliced from the first replaced row on.  Every refusal and allocation comes before the column changes.
static void pay_splice_csr(hx_index* h, PayCol& c, const int64_t* rows_host, int64_t m, const uint32_t* heads,
                           const int64_t* noff, const void* e0_host, const void* e1_host, int64_t total, const char* who) {
  const bool f64 = c.kind == HX_PAY_LIST_F64;
  if (m == 0) return;
  const std::vector<uint32_t> rows = replace_rows_checked(rows_host, m, c.filled, who);
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  hipStream_t st = nullptr;
  DevTmp rows_dev, heads_dev, noff_dev, n0, n1, t0, t1;
  rows_dev.alloc((size_t)m * 4);
  heads_dev.alloc((size_t)m * 4);
  noff_dev.alloc((size_t)(m + 1) * 8);
  n0.alloc((size_t)total * 4);
  if (f64) n1.alloc((size_t)total * 4);
  HX_HIP(hipMemcpy(rows_dev.p, rows.data(), (size_t)m * 4, hipMemcpyHostToDevice));
  HX_HIP(hipMemcpy(heads_dev.p, heads, (size_t)m * 4, hipMemcpyHostToDevice));
  HX_HIP(hipMemcpy(noff_dev.p, noff, (size_t)(m + 1) * 8, hipMemcpyHostToDevice));
  if (total > 0) {
    HX_HIP(hipMemcpy(n0.p, e0_host, (size_t)total * 4, hipMemcpyHostToDevice));
    if (f64) HX_HIP(hipMemcpy(n1.p, e1_host, (size_t)total * 4, hipMemcpyHostToDevice));
  }
  // rows in front of the first replaced one keep their elements and offsets; the rest go the sparse CSR's way
  SplicePlan sp;
  splice_plan(sp, c.off, c.filled, *std::min_element(rows.begin(), rows.end()), (const uint32_t*)rows_dev.p, m,
              (const int64_t*)noff_dev.p, st);
  const int64_t want_el = sp.base + sp.moved;
  HX_CHECK(want_el <= 0x7FFFFFFFll, c.tokens() ? "payload: a token column holds fewer than 2^31 words"
                                    : c.text() ? "payload: a text column holds fewer than 2^31 words"
                                               : "payload: a list column holds fewer than 2^31 elements");
  if (sp.moved > 0) {
    t0.alloc((size_t)sp.moved * 4);
    if (f64) t1.alloc((size_t)sp.moved * 4);
  }
  pay_reserve(h, c, c.filled, want_el);
  // ---- the column changes ----
  launch_scatter_u32(heads_dev.p, c.p0, (const uint32_t*)rows_dev.p, m, st);
  if (sp.moved > 0) {
    launch_csr_splice_u32(c.off + sp.f, sp.map(), (const int64_t*)noff_dev.p, sp.off(), sp.docs, c.e0, (const uint32_t*)n0.p,
                          (uint32_t*)t0.p, st);
    if (f64)
      launch_csr_splice_u32(c.off + sp.f, sp.map(), (const int64_t*)noff_dev.p, sp.off(), sp.docs, c.e1,
                            (const uint32_t*)n1.p, (uint32_t*)t1.p, st);
    launch_copy_u32(t0.p, c.e0 + sp.base, sp.moved, st);
    if (f64) launch_copy_u32(t1.p, c.e1 + sp.base, sp.moved, st);
  }
  launch_csr_new_indptr(c.off + sp.f, sp.off(), sp.docs, sp.base, st);
  HX_HIP(hipDeviceSynchronize());
  c.n_el = want_el;
}

// what hx_payload_debug_list / _text read of a stored row: its head and the offsets of its elements, o[0] and o[1]
static void pay_row_span(hx_index* h, const PayCol& c, int64_t row, const void* out, int64_t cap, uint32_t* hd, int64_t o[2]) {
  HX_CHECK(row >= 0 && row < c.filled, "payload: row out of range");
  HX_CHECK(cap >= 0 && (out || cap == 0), "payload: bad output buffer");
  h->set_device();
  HX_HIP(hipMemcpy(hd, c.p0 + row, 4, hipMemcpyDeviceToHost));
  HX_HIP(hipMemcpy(o, c.off + row, 16, hipMemcpyDeviceToHost));
}

// ---- payload facets -------------------------------------------------------------------------------
// every refusal of hx_payload_facet, before any device work
static FacetArgs facet_args(hx_index* h, int32_t col, const uint32_t* mask, int64_t mask_rows, uint32_t n_codes) {
  HX_CHECK(n_codes >= 1 && n_codes <= 0xFFFFFFFEu, "facet: n_codes out of range [1, 0xFFFFFFFE]");
  const PayCol& c = pay_col(h, col);
  HX_CHECK(c.kind == HX_PAY_U32 || c.kind == HX_PAY_LIST_U32,
           "facet: the column kind must be HX_PAY_U32 or HX_PAY_LIST_U32 (keyword codes or bools)");
  HX_CHECK(c.filled == h->n, "facet: the column is not filled to the index's row count (hx_count)");
  HX_CHECK(!mask || mask_rows == h->n, "facet: mask_rows must equal the index's row count (hx_count)");
  FacetArgs a{};
  a.p0 = c.p0;
  a.off = c.list() ? c.off : nullptr;
  a.e0 = c.list() ? c.e0 : nullptr;
  a.mask = mask;
  a.n = h->n;
  a.n_codes = n_codes;
  return a;
}
static void facet_count_enqueue(hx_index* h, FacetArgs a, uint32_t* counts, uint64_t* stray, hipStream_t st) {
  a.counts = counts;
  a.stray = (unsigned long long*)stray;
  HX_HIP(hipMemsetAsync(counts, 0, (size_t)a.n_codes * 4, st));
  HX_HIP(hipMemsetAsync(stray, 0, 8, st));
  launch_facet_count(a, h->pay_grid, st);
}
static void facet_top_check(uint32_t n_codes, int32_t limit) {
  HX_CHECK(n_codes >= 1 && n_codes <= 0xFFFFFFFEu, "facet: n_codes out of range [1, 0xFFFFFFFE]");
  HX_CHECK(limit >= 1 && limit <= MAX_LIMIT, "facet: limit out of range [1, 2048]");
}
// The slices' lists (launch_facet_keys) merged by the compaction, at most CAND_CAP keys per merged list, until one list
// is left: the top L of a union lies in the union of the top Ls.  A round turns k lists of `len`
// keys into ceil(k / g) lists of `limit` keys, g = CAND_CAP / len.
static void facet_top_enqueue(hx_index* h, const uint32_t* counts, uint32_t n_codes, const uint32_t* rank, int limit,
                              uint64_t* out_keys, int32_t* out_count, hipStream_t st) {
  int len = limit <= 512 ? limit : FACET_SLICE;
  int64_t lists = ((int64_t)n_codes + FACET_SLICE - 1) / FACET_SLICE;
  const int64_t g0 = CAND_CAP / len, g1 = CAND_CAP / limit;
  const size_t keys = (size_t)std::max((lists + g0) * len, ((lists + g0 - 1) / g0 + g1) * limit);
  uint64_t* cur = (uint64_t*)h->ws.get(WS_FACET_A, keys * 8);
  uint64_t* nxt = (uint64_t*)h->ws.get(WS_FACET_B, keys * 8);
  int* cnt = (int*)h->ws.get(WS_FACET_CNT, (size_t)((lists + g0 - 1) / g0) * 4);
  launch_facet_keys(counts, n_codes, rank, cur, len, st);
  for (;;) {
    const int64_t g = CAND_CAP / len;
    if (lists <= g) {
      launch_compact(cur, (int)(lists * len), nullptr, 1, limit, 0, out_keys, limit, out_count, nullptr,
                     (int)(lists * len), st);
      return;
    }
    const int64_t groups = (lists + g - 1) / g;
    if (groups * g > lists)              // the last group's missing lists read as empty
      HX_HIP(hipMemsetAsync(cur + lists * len, 0, (size_t)(groups * g - lists) * len * 8, st));
    launch_compact(cur, (int)(g * len), nullptr, (int)groups, limit, 0, nxt, limit, cnt, nullptr, (int)(g * len), st);
    std::swap(cur, nxt);
    lists = groups;
    len = limit;
  }
}

// ---- scroll -----------------------------------------------------------------------------------------
// every refusal of hx_scroll_rows, before any device work
static void scroll_check(hx_index* h, const uint32_t* mask, int64_t mask_rows, int64_t start_row, int32_t limit) {
  HX_CHECK(limit >= 1 && limit <= HX_SCROLL_MAX_LIMIT, "scroll: limit out of range [1, 2048]");
  HX_CHECK(!mask || mask_rows == h->n, "scroll: mask_rows must equal the index's row count (hx_count)");
  HX_CHECK(start_row >= 0 && start_row <= h->n, "scroll: start_row out of range [0, hx_count]");
}
// the order key s of a bound (hx.h)
static uint64_t order_s(double x, int desc) {
  x += 0.0;
  uint64_t b;
  std::memcpy(&b, &x, 8);
  const uint64_t u = b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
  return desc ? ~u : u;
}
// every refusal of hx_payload_order, before any device work; the scratch pointers are the caller's to fill
static OrderArgs order_args(hx_index* h, int32_t col, const uint32_t* mask, int64_t mask_rows, int32_t direction,
                            int32_t flags, double start_from, double after_value, int64_t after_row, int32_t limit) {
  scroll_check(h, mask, mask_rows, 0, limit);
  const PayCol& c = pay_col(h, col);
  HX_CHECK(c.kind == HX_PAY_F64, "scroll: the column kind must be HX_PAY_F64 (numbers)");
  HX_CHECK(c.filled == h->n, "scroll: the column is not filled to the index's row count (hx_count)");
  HX_CHECK(direction == HX_ORDER_ASC || direction == HX_ORDER_DESC, "scroll: direction must be HX_ORDER_ASC or HX_ORDER_DESC");
  HX_CHECK((flags & ~(HX_ORDER_HAS_START | HX_ORDER_HAS_AFTER)) == 0, "scroll: unknown flag bits");
  const bool has_start = flags & HX_ORDER_HAS_START, has_after = flags & HX_ORDER_HAS_AFTER;
  HX_CHECK(!has_start || start_from == start_from, "scroll: start_from is a NaN");
  HX_CHECK(!has_after || after_value == after_value, "scroll: after_value is a NaN");
  HX_CHECK(!has_after || after_row >= 0, "scroll: after_row is negative");
  OrderArgs a{};
  a.lo = c.p0;
  a.hi = c.p1;
  a.mask = mask;
  a.n = h->n;
  a.desc = direction;
  a.has_start = has_start;
  a.has_after = has_after;
  a.s_start = has_start ? order_s(start_from, direction) : 0ull;
  a.s_after = has_after ? order_s(after_value, direction) : 0ull;
  a.after_row = has_after ? after_row : 0;
  a.limit = limit;
  return a;
}
// the scratch of both calls, one block: [histograms | state | candidate keys | candidate rows | slice counts | prefixes]
struct ScrollWork {
  uint32_t* hist;
  OrderState* st;
  uint64_t* cand_s;
  uint32_t *cand_row, *slice_cnt, *slice_pre;
};
static ScrollWork scroll_work(hx_index* h) {
  const size_t hist = (size_t)ORDER_PASSES * ORDER_BINS * 4, state = 64, cs = (size_t)HX_SCROLL_MAX_LIMIT * 8,
               cr = (size_t)HX_SCROLL_MAX_LIMIT * 4, sl = (size_t)FIRST_MAX_SLICES * 4;
  uint8_t* p = (uint8_t*)h->ws.get(WS_SCROLL_WORK, hist + state + cs + cr + 2 * sl);
  ScrollWork w;
  w.hist = (uint32_t*)p;
  w.st = (OrderState*)(p + hist);
  w.cand_s = (uint64_t*)(p + hist + state);
  w.cand_row = (uint32_t*)(p + hist + state + cs);
  w.slice_cnt = (uint32_t*)(p + hist + state + cs + cr);
  w.slice_pre = w.slice_cnt + FIRST_MAX_SLICES;
  return w;
}
static void scroll_rows_enqueue(hx_index* h, const uint32_t* mask, int64_t start_row, int32_t limit, uint32_t* out_rows,
                                int32_t* out_count, hipStream_t st) {
  if (h->n == 0) {
    HX_HIP(hipMemsetAsync(out_rows, 0, (size_t)limit * 4, st));
    HX_HIP(hipMemsetAsync(out_count, 0, 4, st));
    return;
  }
  const ScrollWork w = scroll_work(h);
  launch_scroll_rows(mask, h->n, start_row, limit, w.slice_cnt, w.slice_pre, out_rows, out_count, h->pay_grid, st);
}
static void order_enqueue(hx_index* h, OrderArgs a, uint32_t* out_rows, uint64_t* out_bits, int32_t* out_count,
                          hipStream_t st) {
  if (h->n == 0) {
    HX_HIP(hipMemsetAsync(out_rows, 0, (size_t)a.limit * 4, st));
    HX_HIP(hipMemsetAsync(out_bits, 0, (size_t)a.limit * 8, st));
    HX_HIP(hipMemsetAsync(out_count, 0, 4, st));
    return;
  }
  const ScrollWork w = scroll_work(h);
  a.hist = w.hist;
  a.st = w.st;
  a.cand_s = w.cand_s;
  a.cand_row = w.cand_row;
  a.slice_cnt = w.slice_cnt;
  a.slice_pre = w.slice_pre;
  launch_payload_order(a, out_rows, out_bits, out_count, h->pay_grid, st);
}
// the host forms' mask on the device (NULL: every row), and their result block [bits: limit x 8 | rows: limit x 4 | count]
static const uint32_t* scroll_mask_up(hx_index* h, const uint32_t* mask_host, hipStream_t st) {
  const size_t mask_bytes = (size_t)((h->n + 31) / 32) * 4;
  if (!mask_host || !mask_bytes) return nullptr;
  uint32_t* m = (uint32_t*)h->ws.get(WS_SCROLL_MASK, mask_bytes);
  HX_HIP(hipMemcpyAsync(m, mask_host, mask_bytes, hipMemcpyHostToDevice, st));
  return m;
}

}  // namespace hx

extern "C" {

// ---- payload index ---------------------------------------------------------------------------
int hx_payload_create(hx_index* h, int32_t kind, int32_t* col) {
  HX_TRY
  HX_CHECK(h && col, "NULL argument");
  HX_CHECK(kind == HX_PAY_U32 || kind == HX_PAY_F64 || kind == HX_PAY_LIST_U32 || kind == HX_PAY_LIST_F64 ||
               kind == HX_PAY_TEXT,
           "payload: kind must be HX_PAY_U32, HX_PAY_F64, HX_PAY_LIST_U32, HX_PAY_LIST_F64 or HX_PAY_TEXT");
  HX_CHECK((int)h->pay.size() < HX_PAY_MAX_COLUMNS, "payload: an index holds at most 64 columns");
  hx_index::PayCol c;
  c.id = h->pay_next_id++;
  c.kind = kind;
  h->pay.push_back(c);
  *col = c.id;
  HX_CATCH
}

int hx_payload_drop(hx_index* h, int32_t col) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  pay_free(c);
  h->pay.erase(h->pay.begin() + (&c - h->pay.data()));
  HX_CATCH
}

int hx_payload_rows(hx_index* h, int32_t col, int64_t* filled) {
  HX_TRY
  HX_CHECK(h && filled, "NULL argument");
  *filled = pay_col(h, col).filled;
  HX_CATCH
}

int hx_payload_append(hx_index* h, int32_t col, const void* cells_host, int64_t n) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(n >= 0, "payload: n < 0");
  HX_CHECK(cells_host || n == 0, "payload: cells are NULL");
  HX_CHECK(!c.list(), "payload: a list column takes hx_payload_append_lists (column kind)");
  HX_CHECK(!c.text(), "payload: a text column takes hx_payload_append_text (column kind)");
  HX_CHECK(!c.tokens(), "payload: a token column takes hx_payload_append_tokens (column kind)");
  HX_CHECK(c.filled + n <= h->n, "payload: the cells reach past the index's row count (hx_count)");
  if (n == 0) return 0;
  h->set_device();
  const int64_t want = c.filled + n;
  pay_reserve(h, c, want, 0);          // (everything that can fail comes before the column changes)
  if (c.kind != HX_PAY_F64) {
    HX_HIP(hipMemcpy(c.p0 + c.filled, cells_host, (size_t)n * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<uint32_t> lo, hi;
    split_f64(cells_host, n, lo, hi);
    HX_HIP(hipMemcpy(c.p0 + c.filled, lo.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HX_HIP(hipMemcpy(c.p1 + c.filled, hi.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  c.filled = want;
  HX_CATCH
}

int hx_payload_append_lists(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const void* values_host,
                            int64_t n_values) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.list(), "payload: hx_payload_append_lists needs a list column (column kind)");
  HX_CHECK(n >= 0 && n_values >= 0, "payload: n < 0");
  HX_CHECK((heads_host || n == 0) && (values_host || n_values == 0), "payload: cells are NULL");
  HX_CHECK(c.filled + n <= h->n, "payload: the cells reach past the index's row count (hx_count)");
  // ---- every refusal and every allocation before the column changes ----
  std::vector<uint32_t> heads, lo, hi;
  std::vector<int64_t> off;
  const bool f64 = c.kind == HX_PAY_LIST_F64;
  const int64_t total =
      pay_list_pack(heads_host, n, values_host, n_values, c.n_el, c.kind, 0x7FFFFFFFll - c.n_el, heads, off, lo, hi);
  pay_store_csr(h, c, heads.data(), off.data(), n, f64 ? (const void*)lo.data() : values_host, f64 ? hi.data() : nullptr, total);
  HX_CATCH
}

// ---- the cells of rows that stay where they are (upsert by an existing id) --------------------
int hx_payload_replace(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const void* cells_host) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(m >= 0, "payload: m < 0");
  HX_CHECK(m == 0 || (rows_host && cells_host), "payload: rows / cells are NULL");
  HX_CHECK(!c.list(), "payload: a list column takes hx_payload_replace_lists (column kind)");
  HX_CHECK(!c.text(), "payload: a text column takes hx_payload_replace_text (column kind)");
  HX_CHECK(!c.tokens(), "payload: a token column takes hx_payload_replace_tokens (column kind)");
  if (m == 0) return 0;
  const std::vector<uint32_t> rows = replace_rows_checked(rows_host, m, c.filled, "hx_payload_replace");
  h->set_device();
  HX_HIP(hipDeviceSynchronize());
  const bool f64 = c.kind == HX_PAY_F64;
  DevTmp rows_dev, lo_dev, hi_dev;
  rows_dev.alloc((size_t)m * 4);
  lo_dev.alloc((size_t)m * 4);
  HX_HIP(hipMemcpy(rows_dev.p, rows.data(), (size_t)m * 4, hipMemcpyHostToDevice));
  if (!f64) {
    HX_HIP(hipMemcpy(lo_dev.p, cells_host, (size_t)m * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<uint32_t> lo, hi;
    split_f64(cells_host, m, lo, hi);
    hi_dev.alloc((size_t)m * 4);
    HX_HIP(hipMemcpy(lo_dev.p, lo.data(), (size_t)m * 4, hipMemcpyHostToDevice));
    HX_HIP(hipMemcpy(hi_dev.p, hi.data(), (size_t)m * 4, hipMemcpyHostToDevice));
  }
  launch_scatter_u32(lo_dev.p, c.p0, (const uint32_t*)rows_dev.p, m, nullptr);
  if (f64) launch_scatter_u32(hi_dev.p, c.p1, (const uint32_t*)rows_dev.p, m, nullptr);
  HX_HIP(hipDeviceSynchronize());
  HX_CATCH
}

int hx_payload_replace_lists(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                             const void* values_host, int64_t n_values) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.list(), "payload: hx_payload_replace_lists needs a list column (column kind)");
  HX_CHECK(m >= 0 && n_values >= 0, "payload: m < 0");
  HX_CHECK((m == 0 || (rows_host && heads_host)) && (values_host || n_values == 0), "payload: rows / cells are NULL");
  // ---- every refusal and every allocation before the column changes (the element count: once the splice is planned) ----
  std::vector<uint32_t> heads, lo, hi;
  std::vector<int64_t> noff;
  const bool f64 = c.kind == HX_PAY_LIST_F64;
  const int64_t total = pay_list_pack(heads_host, m, values_host, n_values, 0, c.kind, INT64_MAX, heads, noff, lo, hi);
  pay_splice_csr(h, c, rows_host, m, heads.data(), noff.data(), f64 ? (const void*)lo.data() : values_host,
                 f64 ? hi.data() : nullptr, total, "hx_payload_replace_lists");
  HX_CATCH
}

int hx_payload_debug_list(hx_index* h, int32_t col, int64_t row, uint32_t* head, void* values_out, int64_t cap,
                          int64_t* count) {
  HX_TRY
  HX_CHECK(h && head && count, "NULL argument");
  auto& c = pay_col(h, col);
  HX_CHECK(c.list(), "payload: hx_payload_debug_list needs a list column (column kind)");
  uint32_t hd = 0;
  int64_t o[2] = {0, 0};
  pay_row_span(h, c, row, values_out, cap, &hd, o);
  const int64_t len = o[1] - o[0];
  HX_CHECK(len >= 0 && o[0] >= 0 && o[1] <= c.n_el, "payload: corrupt list offsets");
  *count = len;
  *head = hd >= HX_PAY_U32_NULL ? hd : (uint32_t)len;
  const int64_t k = std::min(len, cap);
  if (k <= 0) return 0;
  if (c.kind == HX_PAY_LIST_U32) {
    HX_HIP(hipMemcpy(values_out, c.e0 + o[0], (size_t)k * 4, hipMemcpyDeviceToHost));
  } else {
    std::vector<uint32_t> lo((size_t)k), hi((size_t)k);
    HX_HIP(hipMemcpy(lo.data(), c.e0 + o[0], (size_t)k * 4, hipMemcpyDeviceToHost));
    HX_HIP(hipMemcpy(hi.data(), c.e1 + o[0], (size_t)k * 4, hipMemcpyDeviceToHost));
    join_f64(lo, hi, values_out);
  }
  HX_CATCH
}

// ---- text columns (HX_PAY_TEXT) ----------------------------------------------------------------
int hx_payload_append_text(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const void* bytes_host,
                           int64_t n_bytes) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.text(), "payload: hx_payload_append_text needs a text column (column kind)");
  HX_CHECK(n >= 0 && n_bytes >= 0, "payload: n < 0");
  HX_CHECK((heads_host || n == 0) && (bytes_host || n_bytes == 0), "payload: cells are NULL");
  HX_CHECK(c.filled + n <= h->n, "payload: the cells reach past the index's row count (hx_count)");
  // ---- every refusal and every allocation before the column changes ----
  std::vector<int64_t> off;
  std::vector<uint32_t> words;
  pay_text_pack(heads_host, n, bytes_host, n_bytes, c.n_el, off, words);
  HX_CHECK(c.n_el + (int64_t)words.size() <= 0x7FFFFFFFll, "payload: a text column holds fewer than 2^31 words");
  pay_store_csr(h, c, heads_host, off.data(), n, words.data(), nullptr, (int64_t)words.size());
  HX_CATCH
}

int hx_payload_replace_text(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                            const void* bytes_host, int64_t n_bytes) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.text(), "payload: hx_payload_replace_text needs a text column (column kind)");
  HX_CHECK(m >= 0 && n_bytes >= 0, "payload: m < 0");
  HX_CHECK((m == 0 || (rows_host && heads_host)) && (bytes_host || n_bytes == 0), "payload: rows / cells are NULL");
  std::vector<int64_t> noff;
  std::vector<uint32_t> words;
  pay_text_pack(heads_host, m, bytes_host, n_bytes, 0, noff, words);
  pay_splice_csr(h, c, rows_host, m, heads_host, noff.data(), words.data(), nullptr, (int64_t)words.size(),
                 "hx_payload_replace_text");
  HX_CATCH
}

int hx_payload_debug_text(hx_index* h, int32_t col, int64_t row, uint32_t* head, void* bytes_out, int64_t cap,
                          int64_t* count) {
  HX_TRY
  HX_CHECK(h && head && count, "NULL argument");
  auto& c = pay_col(h, col);
  HX_CHECK(c.text(), "payload: hx_payload_debug_text needs a text column (column kind)");
  uint32_t hd = 0;
  int64_t o[2] = {0, 0};
  pay_row_span(h, c, row, bytes_out, cap, &hd, o);
  const int64_t len = hd < HX_PAY_U32_NULL ? (int64_t)hd : 0;
  HX_CHECK(o[0] >= 0 && o[1] <= c.n_el && o[1] - o[0] == (len + 3) / 4, "payload: corrupt text offsets");
  *head = hd;
  *count = len;
  const int64_t k = std::min(len, cap);
  if (k <= 0) return 0;
  std::vector<uint32_t> words((size_t)(k + 3) / 4);
  HX_HIP(hipMemcpy(words.data(), c.e0 + o[0], words.size() * 4, hipMemcpyDeviceToHost));
  std::memcpy(bytes_out, words.data(), (size_t)k);
  HX_CATCH
}

// ---- token columns (HX_PAY_TOKENS) -------------------------------------------------------------
int hx_payload_create_tokens(hx_index* h, int32_t dim_t, int32_t* col) {
  HX_TRY
  HX_CHECK(h && col, "NULL argument");
  HX_CHECK(dim_t >= 64 && dim_t <= HX_TOKENS_MAX_DIM && dim_t % 64 == 0,
           "payload: dim_t must be a multiple of 64 in [64, 1024]");
  HX_CHECK((int)h->pay.size() < HX_PAY_MAX_COLUMNS, "payload: an index holds at most 64 columns");
  hx_index::PayCol c;
  c.id = h->pay_next_id++;
  c.kind = HX_PAY_TOKENS;
  c.dim_t = dim_t;
  h->pay.push_back(c);
  *col = c.id;
  HX_CATCH
}

int hx_payload_append_tokens(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const int8_t* x8_host,
                             const float* scales_host, int64_t n_tokens) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.tokens(), "payload: hx_payload_append_tokens needs a token column (column kind)");
  HX_CHECK(n >= 0 && n_tokens >= 0, "payload: n < 0");
  HX_CHECK((heads_host || n == 0) && ((x8_host && scales_host) || n_tokens == 0), "payload: cells are NULL");
  HX_CHECK(c.filled + n <= h->n, "payload: the cells reach past the index's row count (hx_count)");
  // ---- every refusal and every allocation before the column changes ----
  std::vector<int64_t> off;
  std::vector<uint32_t> words;
  pay_tokens_pack(heads_host, n, x8_host, scales_host, n_tokens, c.dim_t, c.n_el, off, words);
  pay_store_csr(h, c, heads_host, off.data(), n, words.data(), nullptr, (int64_t)words.size());
  HX_CATCH
}

int hx_payload_replace_tokens(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                              const int8_t* x8_host, const float* scales_host, int64_t n_tokens) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  auto& c = pay_col(h, col);
  HX_CHECK(c.tokens(), "payload: hx_payload_replace_tokens needs a token column (column kind)");
  HX_CHECK(m >= 0 && n_tokens >= 0, "payload: m < 0");
  HX_CHECK((m == 0 || (rows_host && heads_host)) && ((x8_host && scales_host) || n_tokens == 0),
           "payload: rows / cells are NULL");
  std::vector<int64_t> noff;
  std::vector<uint32_t> words;
  pay_tokens_pack(heads_host, m, x8_host, scales_host, n_tokens, c.dim_t, 0, noff, words);
  pay_splice_csr(h, c, rows_host, m, heads_host, noff.data(), words.data(), nullptr, (int64_t)words.size(),
                 "hx_payload_replace_tokens");
  HX_CATCH
}

int hx_payload_debug_tokens(hx_index* h, int32_t col, int64_t row, uint32_t* head, int8_t* x8_out, float* scales_out,
                            int64_t cap, int64_t* count, int32_t* dim_t) {
  HX_TRY
  HX_CHECK(h && head && count, "NULL argument");
  auto& c = pay_col(h, col);
  HX_CHECK(c.tokens(), "payload: hx_payload_debug_tokens needs a token column (column kind)");
  HX_CHECK(cap == 0 || scales_out, "payload: bad output buffer");
  uint32_t hd = 0;
  int64_t o[2] = {0, 0};
  pay_row_span(h, c, row, x8_out, cap, &hd, o);
  const int64_t td = hd < HX_PAY_U32_NULL ? (int64_t)hd : 0;
  HX_CHECK(o[0] >= 0 && o[1] <= c.n_el && o[1] - o[0] == pay_token_words(td, c.dim_t), "payload: corrupt token offsets");
  *head = hd;
  *count = td;
  if (dim_t) *dim_t = c.dim_t;
  const int64_t k = std::min(td, cap);
  if (k <= 0) return 0;
  const uint8_t* base = (const uint8_t*)(c.e0 + o[0]);
  HX_HIP(hipMemcpy(x8_out, base, (size_t)k * c.dim_t, hipMemcpyDeviceToHost));
  HX_HIP(hipMemcpy(scales_out, base + (size_t)td * c.dim_t, (size_t)k * 4, hipMemcpyDeviceToHost));
  HX_CATCH
}

int hx_payload_debug_cell(hx_index* h, int32_t col, int64_t row, void* out_host) {
  HX_TRY
  HX_CHECK(h && out_host, "NULL argument");
  auto& c = pay_col(h, col);
  HX_CHECK(!c.list(), "payload: a list column takes hx_payload_debug_list (column kind)");
  HX_CHECK(!c.text(), "payload: a text column takes hx_payload_debug_text (column kind)");
  HX_CHECK(!c.tokens(), "payload: a token column takes hx_payload_debug_tokens (column kind)");
  HX_CHECK(row >= 0 && row < c.filled, "payload: row out of range");
  h->set_device();
  HX_HIP(hipMemcpy(out_host, c.p0 + row, 4, hipMemcpyDeviceToHost));
  if (c.kind == HX_PAY_F64) HX_HIP(hipMemcpy((uint8_t*)out_host + 4, c.p1 + row, 4, hipMemcpyDeviceToHost));
  HX_CATCH
}

int hx_payload_mask(hx_index* h, const hx_pay_op* ops, int32_t n_ops, const hx_pay_set* sets, int32_t n_sets,
                    uint32_t* mask_dev, int64_t* n_kept, void* stream) {
  HX_TRY
  HX_CHECK(h && ops && (mask_dev || h->n == 0), "NULL argument");
  HX_CHECK(n_ops >= 1 && n_ops <= HX_PAY_MAX_OPS, "payload: a program holds 1 to 4096 ops");
  HX_CHECK(n_sets >= 0 && (sets || n_sets == 0), "payload: bad sets");
  // ---- every refusal, before any device work ----
  std::vector<PayOpDev> prog((size_t)n_ops);
  std::vector<int8_t> set_kind((size_t)n_sets, 0);        // 0 = unused, 1 = uint32, 2 = double, 3 = a pattern blob
  struct TextOp {                                         // one HX_PAY_TEXT_ALL: a k_payload_text launch + PAY_D_BITS
    int at;
    const hx_index::PayCol* c;
    std::vector<PayTextPat> pats;
    size_t pat_off = 0;
  };
  std::vector<TextOp> texts;
  struct NestedOp {                                       // one HX_PAY_NESTED: a k_payload_nested launch + PAY_D_BITS
    int at;
    const int64_t* off;
    PayNestedCols cols;
    std::vector<PayElOpDev> ops;                          // (an IN op: imm = the set's index until the sets are placed)
    size_t op_off = 0;
  };
  std::vector<NestedOp> nests;
  auto use_set = [&](uint64_t idx, int8_t kind) {
    HX_CHECK(idx < (uint64_t)n_sets, "payload: set index out of range");
    HX_CHECK(set_kind[(size_t)idx] == 0 || set_kind[(size_t)idx] == kind, "payload: one set used as uint32 and as double");
    set_kind[(size_t)idx] = kind;
  };
  int depth = 0, n_dev = 0;                               // n_dev = ops of the device program: a nested block becomes one
  for (int i = 0; i < n_ops; ++i) {
    const hx_pay_op& o = ops[i];
    PayOpDev d{0u, 0u, o.imm, nullptr, nullptr, nullptr, nullptr, nullptr, 0ull};
    if (o.op == HX_PAY_NESTED) {       // 
      const hx_index::PayCol& a = pay_col(h, o.col);
      HX_CHECK(a.list(), "payload: the anchor of a nested block must be a list column (column kind)");
      HX_CHECK(a.filled == h->n, "payload: column " + std::to_string(o.col) + " is not filled to the index's row count");
      HX_CHECK(o.imm >= 1 && o.imm <= HX_PAY_NESTED_MAX_OPS, "payload: a nested block holds 1 to 64 element ops");
      const int m = (int)o.imm;
      HX_CHECK(i + m < n_ops, "payload: a nested block runs past the program's end");
      NestedOp nb;
      nb.at = n_dev;
      nb.off = a.off;
      nb.cols = PayNestedCols{};
      int32_t ids[HX_PAY_NESTED_MAX_COLS];
      int edepth = 0;
      for (int j = 1; j <= m; ++j) {
        const hx_pay_op& e = ops[i + j];
        PayElOpDev ed{0u, 0u, 0u, 0u, e.imm, 0ull};
        int epops = 0;
        bool ef64 = false;
        if (e.op >= HX_PAY_EL_EQ && e.op <= HX_PAY_EL_RANGE) {
          const hx_index::PayCol& c = pay_col(h, e.col);
          HX_CHECK(c.list(), "payload: EL_EQ / EL_IN / EL_RANGE need a list column (column kind)");
          HX_CHECK(c.filled == h->n, "payload: column " + std::to_string(e.col) + " is not filled to the index's row count");
          HX_CHECK(c.n_el == a.n_el, "payload: the columns of a nested block hold different numbers of elements");
          ef64 = c.kind == HX_PAY_LIST_F64;
          int slot = 0;
          while (slot < nb.cols.n_cols && ids[slot] != e.col) ++slot;
          if (slot == nb.cols.n_cols) {
            HX_CHECK(slot < HX_PAY_NESTED_MAX_COLS, "payload: a nested block reads at most 8 distinct columns");
            ids[slot] = e.col;
            nb.cols.e0[slot] = c.e0;
            nb.cols.e1[slot] = ef64 ? c.e1 : nullptr;
            ++nb.cols.n_cols;
          }
          ed.slot = (uint32_t)slot;
        }
        switch (e.op) {
          case HX_PAY_TRUE: ed.op = PAY_E_TRUE; break;
          case HX_PAY_FALSE: ed.op = PAY_E_FALSE; break;
          case HX_PAY_AND: ed.op = PAY_E_AND; epops = 2; break;
          case HX_PAY_OR: ed.op = PAY_E_OR; epops = 2; break;
          case HX_PAY_NOT: ed.op = PAY_E_NOT; epops = 1; break;
          case HX_PAY_EL_EQ: ed.op = ef64 ? PAY_E_EQ_F64 : PAY_E_EQ_U32; break;
          case HX_PAY_EL_IN:
            ed.op = ef64 ? PAY_E_IN_F64 : PAY_E_IN_U32;
            use_set(e.imm, ef64 ? 2 : 1);
            break;
          case HX_PAY_EL_RANGE:
            HX_CHECK(ef64, "payload: EL_RANGE needs an F64 list column");
            ed.op = PAY_E_RANGE;
            use_set(e.imm, 2);
            HX_CHECK(sets[e.imm].n == 2, "payload: the set of EL_RANGE holds exactly two doubles, lo <= hi");
            break;
          default: throw Error("payload: op " + std::to_string(e.op) + " is a row op inside a nested block");
        }
        HX_CHECK(edepth >= epops, "payload: element stack underflow at op " + std::to_string(i + j));
        edepth += 1 - epops;
        HX_CHECK(edepth <= HX_PAY_MAX_STACK, "payload: the element stack exceeds 32 entries at op " + std::to_string(i + j));
        nb.ops.push_back(ed);
      }
      HX_CHECK(edepth == 1, "payload: the element program must leave exactly one entry on its stack");
      nests.push_back(std::move(nb));
      d.op = PAY_D_BITS;
      ++depth;
      HX_CHECK(depth <= HX_PAY_MAX_STACK, "payload: the stack exceeds 32 entries at op " + std::to_string(i));
      prog[(size_t)n_dev++] = d;
      i += m;
      continue;
    }
    HX_CHECK(!(o.op >= HX_PAY_EL_EQ && o.op <= HX_PAY_EL_RANGE),
             "payload: op " + std::to_string(o.op) + " is an element op outside a nested block");
    int pops = 0;
    const hx_index::PayCol* c = nullptr;
    const bool list_op = o.op >= HX_PAY_ANY_EQ && o.op <= HX_PAY_IS_EMPTY_LIST;
    const bool reads_col = (o.op >= HX_PAY_IS_MISSING && o.op <= HX_PAY_GE) || list_op || o.op == HX_PAY_TEXT_ALL;
    if (reads_col) {
      c = &pay_col(h, o.col);
      HX_CHECK(c->filled == h->n, "payload: column " + std::to_string(o.col) + " is not filled to the index's row count");
      d.p0 = c->p0;
      d.p1 = c->kind == HX_PAY_F64 ? c->p1 : nullptr;
      if (c->list()) {                 // (filled == hx_count > 0 below: off is allocated; no element = never read)
        d.off = c->off;
        d.e0 = c->e0;
        d.e1 = c->kind == HX_PAY_LIST_F64 ? c->e1 : nullptr;
      }
      if (c->tokens()) d.off = c->off;  // (IS_EMPTY_LIST: head 0 and no word; the words themselves are never read)
      HX_CHECK(!c->text() || (o.op >= HX_PAY_IS_MISSING && o.op <= HX_PAY_PRESENT) || o.op == HX_PAY_TEXT_ALL,
               "payload: a text column takes IS_MISSING / IS_NULL / PRESENT / TEXT_ALL only");
      HX_CHECK(!c->tokens() || (o.op >= HX_PAY_IS_MISSING && o.op <= HX_PAY_PRESENT) || o.op == HX_PAY_IS_EMPTY_LIST,
               "payload: a token column takes IS_MISSING / IS_NULL / PRESENT / IS_EMPTY_LIST only");
      HX_CHECK(!list_op || c->list() || c->tokens(), "payload: ANY_EQ / ANY_IN / ANY_RANGE / IS_EMPTY_LIST need a list column");
      HX_CHECK(!(o.op >= HX_PAY_EQ && o.op <= HX_PAY_GE) || !c->list(),
               "payload: EQ / IN / LT / LE / GT / GE need a scalar column (a list column takes the ANY ops)");
      HX_CHECK(o.op != HX_PAY_TEXT_ALL || c->text(),
               "payload: unknown op " + std::to_string(o.op) + " for this column's kind: TEXT_ALL needs a text column");
    }
    const bool f64 = c && (c->kind == HX_PAY_F64 || c->kind == HX_PAY_LIST_F64);
    switch (o.op) {
      case HX_PAY_TRUE: d.op = PAY_D_TRUE; break;
      case HX_PAY_FALSE: d.op = PAY_D_FALSE; break;
      case HX_PAY_IS_MISSING: d.op = PAY_D_IS_MISSING; break;
      case HX_PAY_IS_NULL: d.op = PAY_D_IS_NULL; break;
      case HX_PAY_PRESENT: d.op = PAY_D_PRESENT; break;
      case HX_PAY_EQ: d.op = f64 ? PAY_D_EQ_F64 : PAY_D_EQ_U32; break;
      case HX_PAY_IN: d.op = f64 ? PAY_D_IN_F64 : PAY_D_IN_U32; break;
      case HX_PAY_LT: d.op = PAY_D_LT; break;
      case HX_PAY_LE: d.op = PAY_D_LE; break;
      case HX_PAY_GT: d.op = PAY_D_GT; break;
      case HX_PAY_GE: d.op = PAY_D_GE; break;
      case HX_PAY_ROW_IN: d.op = PAY_D_ROW_IN; break;
      case HX_PAY_AND: d.op = PAY_D_AND; pops = 2; break;
      case HX_PAY_OR: d.op = PAY_D_OR; pops = 2; break;
      case HX_PAY_NOT: d.op = PAY_D_NOT; pops = 1; break;
      case HX_PAY_ANY_EQ: d.op = f64 ? PAY_D_ANY_EQ_F64 : PAY_D_ANY_EQ_U32; break;
      case HX_PAY_ANY_IN: d.op = f64 ? PAY_D_ANY_IN_F64 : PAY_D_ANY_IN_U32; break;
      case HX_PAY_ANY_RANGE: d.op = PAY_D_ANY_RANGE; break;
      case HX_PAY_IS_EMPTY_LIST: d.op = PAY_D_IS_EMPTY_LIST; break;
      case HX_PAY_TEXT_ALL: {          // the blob: uint32 P, uint32 len[P], the patterns' bytes one after another
        HX_CHECK(o.imm < (uint64_t)n_sets, "payload: set index out of range");
        const hx_pay_set& ps = sets[o.imm];
        HX_CHECK(set_kind[(size_t)o.imm] == 0 || set_kind[(size_t)o.imm] == 3, "payload: one set used as values and as a pattern blob");
        set_kind[(size_t)o.imm] = 3;
        HX_CHECK(ps.vals && ps.n >= 4, "payload: a pattern blob starts with its pattern count");
        const uint8_t* blob = (const uint8_t*)ps.vals;
        uint32_t np = 0;
        std::memcpy(&np, blob, 4);
        HX_CHECK(np >= 1 && np <= HX_PAY_TEXT_MAX_WORDS, "payload: a pattern blob holds 1 to 32 patterns");
        HX_CHECK(ps.n >= 4 + 4 * (int64_t)np, "payload: the pattern blob's size disagrees with its header");
        TextOp t;
        t.at = n_dev;
        t.c = c;
        t.pats.assign(np, PayTextPat{});
        int64_t at = 4 + 4 * (int64_t)np;
        for (uint32_t k = 0; k < np; ++k) {
          uint32_t len = 0;
          std::memcpy(&len, blob + 4 + 4 * k, 4);
          HX_CHECK(len >= 1 && len <= HX_PAY_TEXT_MAX_WORD_BYTES, "payload: a pattern holds 1 to 64 bytes");
          HX_CHECK(at + len <= ps.n, "payload: the pattern blob's size disagrees with its header");
          PayTextPat& pt = t.pats[k];
          pt.len = len;
          pt.fmask = len >= 4 ? 0xFFFFFFFFu : (1u << (8 * len)) - 1u;
          std::memcpy(pt.w, blob + at, len);
          at += len;
        }
        HX_CHECK(at == ps.n, "payload: the pattern blob's size disagrees with its header");
        texts.push_back(std::move(t));
        d.op = PAY_D_BITS;
        d.p0 = nullptr;                // (not a column op on the device: the plane travels in imm)
        d.off = nullptr;
        d.e0 = nullptr;
        break;
      }
      default: throw Error("payload: unknown op " + std::to_string(o.op));
    }
    if (o.op >= HX_PAY_LT && o.op <= HX_PAY_GE) HX_CHECK(f64, "payload: LT / LE / GT / GE need an F64 column");
    if (o.op == HX_PAY_ANY_RANGE) HX_CHECK(f64, "payload: ANY_RANGE needs an F64 list column");
    if (o.op == HX_PAY_IN || o.op == HX_PAY_ROW_IN || o.op == HX_PAY_ANY_IN || o.op == HX_PAY_ANY_RANGE) {
      use_set(o.imm, f64 ? 2 : 1);
      if (o.op == HX_PAY_ANY_RANGE) HX_CHECK(sets[o.imm].n == 2, "payload: the set of ANY_RANGE holds exactly two doubles, lo <= hi");
    }
    HX_CHECK(depth >= pops, "payload: stack underflow at op " + std::to_string(i));
    depth += 1 - pops;
    HX_CHECK(depth <= HX_PAY_MAX_STACK, "payload: the stack exceeds 32 entries at op " + std::to_string(i));
    prog[(size_t)n_dev++] = d;
  }
  HX_CHECK(depth == 1, "payload: the program must leave exactly one entry on the stack");
  const size_t prog_bytes = (size_t)n_dev * sizeof(PayOpDev);
  std::vector<size_t> set_off((size_t)n_sets, 0);
  size_t bytes = prog_bytes;
  for (int s = 0; s < n_sets; ++s) {
    if (!set_kind[(size_t)s] || set_kind[(size_t)s] == 3) continue;   // (a pattern blob travels per op, checked above)
    const int64_t m = sets[s].n;
    HX_CHECK(m >= 0 && m <= 0xFFFFFFFFll && (sets[s].vals || m == 0), "payload: bad set");
    bool ok = true;
    if (set_kind[(size_t)s] == 1) {
      const uint32_t* v = (const uint32_t*)sets[s].vals;
      for (int64_t i = 1; i < m; ++i) ok &= v[i - 1] <= v[i];
    } else {
      const double* v = (const double*)sets[s].vals;
      for (int64_t i = 0; i < m; ++i) ok &= v[i] == v[i] && (i == 0 || v[i - 1] <= v[i]);
    }
    HX_CHECK(ok, "payload: set " + std::to_string(s) + " is not sorted ascending");
    set_off[(size_t)s] = bytes;
    bytes += (size_t)round_up(std::max<int64_t>(m, 1) * (set_kind[(size_t)s] == 1 ? 4 : 8), 8);
  }
  for (auto& t : texts) {
    t.pat_off = bytes;
    bytes += (size_t)round_up((int64_t)(t.pats.size() * sizeof(PayTextPat)), 8);
  }
  for (auto& b : nests) {
    b.op_off = bytes;
    bytes += b.ops.size() * sizeof(PayElOpDev) + sizeof(PayNestedCols);   // (the column table behind the element ops)
  }
  const int64_t n = h->n;
  if (n == 0) {
    if (n_kept) *n_kept = 0;
    return 0;
  }
  // ---- the program, its sets and its patterns: one pinned staging buffer, one copy ----
  h->set_device();
  hipStream_t st = (hipStream_t)stream;
  if (h->pay_ev_pending) {              // the device has taken the previous call's program
    HX_HIP(hipEventSynchronize(h->pay_ev));
    h->pay_ev_pending = false;
  }
  if (bytes > h->pay_pin_cap) {
    if (h->pay_pin) HX_HIP(hipHostFree(h->pay_pin));
    h->pay_pin = nullptr;
    h->pay_pin_cap = 0;
    const size_t want = (size_t)round_up((int64_t)bytes * 2, 4096);
    HX_HIP(hipHostMalloc((void**)&h->pay_pin, want, hipHostMallocDefault));
    h->pay_pin_cap = want;
  }
  if (!h->pay_ev) HX_HIP(hipEventCreateWithFlags(&h->pay_ev, hipEventDisableTiming));
  uint8_t* dev = (uint8_t*)h->ws.get(WS_PAY_PROG, bytes);
  // one packed verdict plane per TEXT_ALL and per NESTED, written by k_payload_text and
  // k_payload_nested (section 26) in front of the mask kernel
  const int64_t plane_words = (n + 31) / 32;
  const size_t n_planes = texts.size() + nests.size();
  uint32_t* planes = n_planes ? (uint32_t*)h->ws.get(WS_PAY_PLANES, n_planes * (size_t)plane_words * 4) : nullptr;
  uint32_t* nplanes = planes + texts.size() * (size_t)plane_words;
  for (size_t t = 0; t < texts.size(); ++t) prog[(size_t)texts[t].at].imm = (uint64_t)(uintptr_t)(planes + t * (size_t)plane_words);
  for (size_t t = 0; t < nests.size(); ++t) {
    prog[(size_t)nests[t].at].imm = (uint64_t)(uintptr_t)(nplanes + t * (size_t)plane_words);
    for (auto& e : nests[t].ops) {
      if (e.op == PAY_E_RANGE) {
        const uint64_t* v = (const uint64_t*)sets[(size_t)e.imm].vals;
        e.imm2 = v[1];
        e.imm = v[0];
      } else if (e.op == PAY_E_IN_U32 || e.op == PAY_E_IN_F64) {
        const size_t s = (size_t)e.imm;
        e.cnt = (uint32_t)sets[s].n;
        e.imm = (uint64_t)(uintptr_t)(dev + set_off[s]);
      }
    }
  }
  for (int i = 0; i < n_dev; ++i) {
    PayOpDev& d = prog[(size_t)i];
    if (d.op == PAY_D_ANY_RANGE) {     // (two doubles, checked above: the closed interval travels in the op itself)
      const uint64_t* v = (const uint64_t*)sets[(size_t)d.imm].vals;
      d.imm = v[0];
      d.imm2 = v[1];
      continue;
    }
    if (d.op != PAY_D_ROW_IN && d.op != PAY_D_IN_U32 && d.op != PAY_D_IN_F64 && d.op != PAY_D_ANY_IN_U32 &&
        d.op != PAY_D_ANY_IN_F64)
      continue;
    const size_t s = (size_t)d.imm;
    d.cnt = (uint32_t)sets[s].n;
    d.imm = (uint64_t)(uintptr_t)(dev + set_off[s]);
  }
  std::memcpy(h->pay_pin, prog.data(), prog_bytes);
  for (int s = 0; s < n_sets; ++s)
    if (set_kind[(size_t)s] && set_kind[(size_t)s] != 3 && sets[s].n > 0)
      std::memcpy(h->pay_pin + set_off[(size_t)s], sets[s].vals, (size_t)sets[s].n * (set_kind[(size_t)s] == 1 ? 4 : 8));
  for (const auto& t : texts) std::memcpy(h->pay_pin + t.pat_off, t.pats.data(), t.pats.size() * sizeof(PayTextPat));
  for (const auto& b : nests) {
    std::memcpy(h->pay_pin + b.op_off, b.ops.data(), b.ops.size() * sizeof(PayElOpDev));
    std::memcpy(h->pay_pin + b.op_off + b.ops.size() * sizeof(PayElOpDev), &b.cols, sizeof(PayNestedCols));
  }
  HX_HIP(hipMemcpyAsync(dev, h->pay_pin, bytes, hipMemcpyHostToDevice, st));
  HX_HIP(hipEventRecord(h->pay_ev, st));
  h->pay_ev_pending = true;
  uint32_t* kept = nullptr;
  if (n_kept) {
    kept = (uint32_t*)h->ws.get(WS_PAY_KEPT, 4);
    HX_HIP(hipMemsetAsync(kept, 0, 4, st));
  }
  for (size_t t = 0; t < texts.size(); ++t)
    launch_payload_text(texts[t].c->p0, texts[t].c->off, texts[t].c->e0, n, (const PayTextPat*)(dev + texts[t].pat_off),
                        (int)texts[t].pats.size(), planes + t * (size_t)plane_words, h->pay_grid, st);
  for (size_t t = 0; t < nests.size(); ++t)
    launch_payload_nested(nests[t].off, n,
                          (const PayNestedCols*)(dev + nests[t].op_off + nests[t].ops.size() * sizeof(PayElOpDev)),
                          (const PayElOpDev*)(dev + nests[t].op_off), (int)nests[t].ops.size(),
                          nplanes + t * (size_t)plane_words, h->pay_grid, st);
  launch_payload_mask((const PayOpDev*)dev, n_dev, n, mask_dev, kept, h->pay_grid, st);
  if (n_kept) {
    uint32_t* pin = (uint32_t*)host_pin(h) + 14;
    HX_HIP(hipMemcpyAsync(pin, kept, 4, hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    *n_kept = pin[0];
  }
  HX_CATCH
}

int hx_payload_same_offsets(hx_index* h, int32_t col_a, int32_t col_b, int32_t* same) {
  HX_TRY
  HX_CHECK(h && same, "NULL argument");
  const auto& a = pay_col(h, col_a);
  const auto& b = pay_col(h, col_b);
  HX_CHECK(a.list() && b.list(), "payload: hx_payload_same_offsets compares two list columns (column kind)");
  if (a.filled != b.filled || a.n_el != b.n_el) {
    *same = 0;
    return 0;
  }
  if (a.filled == 0 || a.id == b.id) {
    *same = 1;
    return 0;
  }
  h->set_device();
  uint32_t* flag = (uint32_t*)h->ws.get(WS_PAY_KEPT, 4);
  const uint32_t one = 1u;
  HX_HIP(hipMemcpy(flag, &one, 4, hipMemcpyHostToDevice));
  launch_payload_same_offsets(a.p0, b.p0, a.off, b.off, a.filled, flag, nullptr);
  uint32_t out = 0u;
  HX_HIP(hipMemcpy(&out, flag, 4, hipMemcpyDeviceToHost));
  *same = (int32_t)out;
  HX_CATCH
}

int hx_payload_facet(hx_index* h, int32_t col, const uint32_t* mask_dev, int64_t mask_rows, uint32_t n_codes,
                     uint32_t* counts_dev, uint64_t* stray_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && counts_dev && stray_dev, "NULL argument");
  const FacetArgs a = facet_args(h, col, mask_dev, mask_rows, n_codes);
  h->set_device();
  facet_count_enqueue(h, a, counts_dev, stray_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_facet_top(hx_index* h, const uint32_t* counts_dev, uint32_t n_codes, const uint32_t* rank_dev, int32_t limit,
                 uint64_t* out_keys_dev, int32_t* out_count_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && counts_dev && out_keys_dev && out_count_dev, "NULL argument");
  facet_top_check(n_codes, limit);
  h->set_device();
  facet_top_enqueue(h, counts_dev, n_codes, rank_dev, limit, out_keys_dev, out_count_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_payload_facet_host(hx_index* h, int32_t col, const uint32_t* mask_host, int64_t mask_rows, uint32_t n_codes,
                          const uint32_t* rank_host, int32_t limit, uint32_t* ranks_or_codes_host, uint32_t* counts_host,
                          int32_t* n_out, uint64_t* stray_host) {
  HX_TRY
  HX_CHECK(h && ranks_or_codes_host && counts_host && n_out && stray_host, "NULL argument");
  facet_top_check(n_codes, limit);
  FacetArgs a = facet_args(h, col, mask_host, mask_rows, n_codes);
  h->set_device();
  hipStream_t st = nullptr;
  const size_t mask_bytes = (size_t)((h->n + 31) / 32) * 4;
  if (mask_host && mask_bytes) {
    uint32_t* m = (uint32_t*)h->ws.get(WS_FACET_MASK, mask_bytes);
    HX_HIP(hipMemcpyAsync(m, mask_host, mask_bytes, hipMemcpyHostToDevice, st));
    a.mask = m;
  } else {
    a.mask = nullptr;
  }
  uint32_t* rank = nullptr;
  if (rank_host) {
    rank = (uint32_t*)h->ws.get(WS_FACET_RANK, (size_t)n_codes * 4);
    HX_HIP(hipMemcpyAsync(rank, rank_host, (size_t)n_codes * 4, hipMemcpyHostToDevice, st));
  }
  uint32_t* counts = (uint32_t*)h->ws.get(WS_FACET_COUNTS, (size_t)n_codes * 4);
  // the results, one block and one copy: [limit keys | the hits (int32, in an 8-byte slot) | stray]
  uint64_t* out = (uint64_t*)h->ws.get(WS_FACET_OUT, ((size_t)limit + 2) * 8);
  facet_count_enqueue(h, a, counts, out + limit + 1, st);
  facet_top_enqueue(h, counts, n_codes, rank, limit, out, (int32_t*)(out + limit), st);
  std::vector<uint64_t> res((size_t)limit + 2);
  HX_HIP(hipMemcpyAsync(res.data(), out, res.size() * 8, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  int32_t hits = 0;
  std::memcpy(&hits, &res[(size_t)limit], 4);
  *n_out = hits;
  *stray_host = res[(size_t)limit + 1];
  for (int32_t i = 0; i < limit; ++i) {
    const uint64_t k = res[(size_t)i];
    ranks_or_codes_host[i] = k ? 0xFFFFFFFFu - (uint32_t)k : 0u;
    counts_host[i] = (uint32_t)(k >> 32);
  }
  HX_CATCH
}

// ---- scroll --------------------------------------------------------------------------------------
int hx_scroll_rows(hx_index* h, const uint32_t* mask_dev, int64_t mask_rows, int64_t start_row, int32_t limit,
                   uint32_t* out_rows_dev, int32_t* out_count_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && out_rows_dev && out_count_dev, "NULL argument");
  scroll_check(h, mask_dev, mask_rows, start_row, limit);
  h->set_device();
  scroll_rows_enqueue(h, mask_dev, start_row, limit, out_rows_dev, out_count_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_payload_order(hx_index* h, int32_t col, const uint32_t* mask_dev, int64_t mask_rows, int32_t direction,
                     int32_t flags, double start_from, double after_value, int64_t after_row, int32_t limit,
                     uint32_t* out_rows_dev, uint64_t* out_bits_dev, int32_t* out_count_dev, void* stream) {
  HX_TRY
  HX_CHECK(h && out_rows_dev && out_bits_dev && out_count_dev, "NULL argument");
  const OrderArgs a = order_args(h, col, mask_dev, mask_rows, direction, flags, start_from, after_value, after_row, limit);
  h->set_device();
  order_enqueue(h, a, out_rows_dev, out_bits_dev, out_count_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_scroll_rows_host(hx_index* h, const uint32_t* mask_host, int64_t mask_rows, int64_t start_row, int32_t limit,
                        uint32_t* out_rows_host, int32_t* out_count_host) {
  HX_TRY
  HX_CHECK(h && out_rows_host && out_count_host, "NULL argument");
  scroll_check(h, mask_host, mask_rows, start_row, limit);
  h->set_device();
  hipStream_t st = nullptr;
  const uint32_t* mask = scroll_mask_up(h, mask_host, st);
  uint32_t* out = (uint32_t*)h->ws.get(WS_SCROLL_OUT, ((size_t)limit * 3 + 2) * 4);
  scroll_rows_enqueue(h, mask, start_row, limit, out, (int32_t*)(out + limit), st);
  std::vector<uint32_t> res((size_t)limit + 1);
  HX_HIP(hipMemcpyAsync(res.data(), out, res.size() * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  std::memcpy(out_rows_host, res.data(), (size_t)limit * 4);
  *out_count_host = (int32_t)res[(size_t)limit];
  HX_CATCH
}

int hx_payload_order_host(hx_index* h, int32_t col, const uint32_t* mask_host, int64_t mask_rows, int32_t direction,
                          int32_t flags, double start_from, double after_value, int64_t after_row, int32_t limit,
                          uint32_t* out_rows_host, uint64_t* out_bits_host, int32_t* out_count_host) {
  HX_TRY
  HX_CHECK(h && out_rows_host && out_bits_host && out_count_host, "NULL argument");
  OrderArgs a = order_args(h, col, mask_host, mask_rows, direction, flags, start_from, after_value, after_row, limit);
  h->set_device();
  hipStream_t st = nullptr;
  a.mask = scroll_mask_up(h, mask_host, st);
  // the results, one block and one copy: [limit cells | limit rows | the hits]
  uint32_t* out = (uint32_t*)h->ws.get(WS_SCROLL_OUT, ((size_t)limit * 3 + 2) * 4);
  order_enqueue(h, a, out + 2 * (size_t)limit, (uint64_t*)out, (int32_t*)(out + 3 * (size_t)limit), st);
  std::vector<uint32_t> res((size_t)limit * 3 + 1);
  HX_HIP(hipMemcpyAsync(res.data(), out, res.size() * 4, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  std::memcpy(out_bits_host, res.data(), (size_t)limit * 8);
  std::memcpy(out_rows_host, res.data() + 2 * (size_t)limit, (size_t)limit * 4);
  *out_count_host = (int32_t)res[3 * (size_t)limit];
  HX_CATCH
}

}  // extern "C"
