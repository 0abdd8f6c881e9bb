// Internal to the host files of libhx -- engine.hip, lifecycle.hip, paystore.hip, poolstage.hip, byexample.hip, spstats.hip
// (DESIGN.md section 3 says what each owns): the state of one collection (struct hx_index) and what one file calls
// in another.
#pragma once
#include "../../include/hx.h"
#include "hx_common.hpp"
#include "kernels.hpp"
#include "replace.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

namespace hx {

struct Workspace {
  std::map<int, std::pair<void*, size_t>> slots;
  void* get(int id, size_t bytes) {
    auto& s = slots[id];
    if (s.second < bytes) {
      if (s.first) HX_HIP(hipFree(s.first));
      s.first = nullptr;
      s.second = 0;
      const size_t want = (bytes + 255) / 256 * 256;
      HX_HIP(hipMalloc(&s.first, want));
      s.second = want;
    }
    return s.first;
  }
  void release() {
    for (auto& kv : slots)
      if (kv.second.first) (void)hipFree(kv.second.first);
    slots.clear();
  }
};

enum WsSlot {
  WS_QN = 1, WS_QH, WS_Q8, WS_RINVQ, WS_CAND, WS_CAND2, WS_CNT, WS_CNT2, WS_OVF, WS_TAU, WS_FAIL,
  WS_NFAIL, WS_QSEL, WS_FB_KEYS, WS_FB_CNT, WS_FB_INCNT, WS_SP_PARTS, WS_SP_PCNT, WS_RAW, WS_RS_TMP,
  WS_T_A, WS_T_ACNT, WS_T_B, WS_T_BCNT, WS_T_C, WS_T_CCNT, WS_T_D, WS_T_DCNT, WS_T_E, WS_T_ECNT,
  WS_T_F, WS_T_FCNT, WS_T_G, WS_T_GCNT, WS_H_QD, WS_H_QIP, WS_H_QIX, WS_H_QV, WS_H_OUT, WS_H_OCNT,
  WS_H_SC, WS_H_ID, WS_SYN_NNZ, WS_RRF_TMP, WS_MISC, WS_SP_CAND, WS_SP_PARK, WS_SP_ORDER, WS_HITLOG, WS_HITCNT, WS_KEPT,
  WS_F_DALL, WS_F_SALL, WS_F_D, WS_F_S, WS_F_DC, WS_F_SC,
  WS_SP_TI0, WS_SP_TI1, WS_SP_QS, WS_SP_MARGIN, WS_SP_FLAG, WS_SP_WORK, WS_SP_FAIL, WS_SP_LIST, WS_SP_LCNT,
  WS_SP_EXACT, WS_SP_ECNT, WS_SP_MM, WS_SP_FTAU, WS_SP_FOVF, WS_SP_QPARTS, WS_SP_SUM,
  WS_ID_IN, WS_LONG_ROWS, WS_Q8S, WS_SQ, WS_EPSQ, WS_TREE_FLAG, WS_DONE,
  WS_M_MASK, WS_M_BLK, WS_M_ROWS, WS_M_FB, WS_ROWS_CHECK, WS_NOM_QBAD, WS_C_LEN, WS_PAY_PROG, WS_PAY_KEPT, WS_PAY_PLANES,
  WS_G_KEYS, WS_G_CODES, WS_G_CNT, WS_MMR_KEYS, WS_MMR_VAL, WS_MMR_CNT, WS_MMR_POOL, WS_MMR_PCNT,
  WS_FACET_A, WS_FACET_B, WS_FACET_CNT, WS_FACET_COUNTS, WS_FACET_MASK, WS_FACET_RANK, WS_FACET_OUT,
  WS_MS_POS, WS_MS_KEYS, WS_MS_CNT, WS_MS_FIRST, WS_MS_Q8, WS_MS_QS, WS_MS_QIP,
  WS_RECO_X, WS_RECO_RAW, WS_RECO_RAWN, WS_RECO_META, WS_RECO_Q, WS_RECO_KEYS, WS_RECO_KCNT, WS_RECO_CAND, WS_RECO_CNT,
  WS_RECO_OVF, WS_RECO_TAU, WS_RECO_TAU0, WS_RECO_MASK, WS_RECO_OUT, WS_RECO_OCNT, WS_RECO_SC, WS_RECO_ID,
  WS_SCROLL_WORK, WS_SCROLL_MASK, WS_SCROLL_OUT,
  WS_FORMULA_PLANES, WS_FORMULA_KEYS, WS_FORMULA_POS, WS_FORMULA_BASE, WS_FORMULA_CNT, WS_FORMULA_DROP,
  WS_MATRIX_ROWS, WS_MATRIX_PLANE, WS_MATRIX_OUT, WS_MATRIX_OCNT, WS_MATRIX_SC, WS_MATRIX_ID,
  WS_DISC_TAU, WS_DISC_TAU0,
  WS_IDF_IDX, WS_IDF_VAL, WS_IDF_DF,
  WS_BIN_Q, WS_BIN_CAND, WS_BIN_CNT, WS_BIN_FLAGS, WS_BIN_TAU, WS_BIN_TAU0,
  WS_ASYM_PLANES, WS_ASYM_TOT
};

template <typename T>
static void grow_copy(T*& p, int64_t old_elems, int64_t new_elems, bool zero_tail) {
  T* np_ = nullptr;
  HX_HIP(hipMalloc((void**)&np_, (size_t)std::max<int64_t>(new_elems, 1) * sizeof(T)));
  if (zero_tail) HX_HIP(hipMemset(np_, 0, (size_t)std::max<int64_t>(new_elems, 1) * sizeof(T)));
  if (p && old_elems > 0) HX_HIP(hipMemcpy(np_, p, (size_t)old_elems * sizeof(T), hipMemcpyDeviceToDevice));
  if (p) HX_HIP(hipFree(p));
  p = np_;
}

struct DevTmp {                      // a temporary of one call
  void* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;    // (owns p)
  void alloc(size_t bytes) { HX_HIP(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
  ~DevTmp() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace hx

using namespace hx;

struct hx_index {
  int dim = 0, dim_pad = 0, dim_pad8 = 0, device = 0;
  int n_pre = 0;
  int psize[3] = {0, 0, 0};
  int64_t id_base = 0;
  int64_t n = 0, cap = 0;
  float* dense = nullptr;
  _Float16* dense_h = nullptr;
  int8_t* q8 = nullptr;
  float* q8_rinv = nullptr;
  float* pre[3] = {nullptr, nullptr, nullptr};
  _Float16* pre_h0 = nullptr;
  // Candidate-pass copy of the normalised rows (DESIGN.md "int8 candidate pass"): rint(x * 127 / max|x|), the
  // row's scale, and -- one device word -- the largest quantisation error ||x - scale * x8|| of any row so far
  // (fp32 bits, rounded up; a rollback leaves it as it is: an upper bound is all the certificate needs).
  int8_t* q8s = nullptr;
  float* q8s_scale = nullptr;
  uint32_t* s8_err = nullptr;
  // 1-bit copy of the normalised rows (hx_binary_enable): bit j & 31 of word j >> 5 of a row =
  // dense[row][j] > 0; bin_words() words per row -- dim_pad8 / 32, at least eight: the kernels that move stored rows take
  // them as two or more 16-byte pieces -- the words past dim_pad / 32 zero.  Derived, never saved; a member of
  // row_arrays() once enabled.
  uint32_t* bits = nullptr;
  bool bin_on = false;
  int bin_words() const { return std::max(dim_pad8 / 32, 8); }
  int cand8 = 1;                      // 0: fp16 candidates only, no int8 copy is kept (HX_DENSE_CAND=f16)
  bool cand8_off = false;             // hx_set_dense_candidates(h, 0): the copy is kept but the fp16 scan nominates
  int64_t cand8_queries = 0, cand8_failed = 0;   // queries the int8 candidate pass took / could not certify
  int64_t tree_redone = 0;            // tree batches run again the synchronous way (a deferred flag was set)
  // Adaptive guards of the two speculative paths (hx_stats): windows of recent outcomes
  int64_t c8_win_q = 0, c8_win_f = 0; // queries / uncertified queries of the current window of the int8 candidate pass
  bool cand8_auto_off = false;        // ... switched off by the guard (hx_set_dense_candidates(h, 1) switches it on again)
  int tree_win_n = 0, tree_win_redone = 0;
  bool tree_spec_off = false;
  int done_zeroed[2] = {0, 0};        // entries of the finish kernel's per-query counters known to be zero (level 0 / retry level)
  bool no_finish_fuse = false;        // HX_DEBUG_NO_FINISH_FUSE (tests): the dense stage's tail always as three launches
  int finish_nb = 0;                  // HX_DEBUG_FINISH_NB (tests): blocks per query of k_dense_finish, 0 = one per four candidates
  // query-tile routing of the scans (read from the environment at hx_create: tests and diagnostics):
  //   B <= 32: k_scan 128 x 32; <= bn64_max: k_scan 128 x 64; <= bn128_max: 128 queries per tile -- the staggered kernel's
  //   256 x 128 form (scan8.hip, HQ) unless no_hq, then k_scan 128 x 128; above: the staggered 256 x 256 kernel
  int bn32_max = 32, bn64_max = 32, bn128_max = 128;
  // second stream of the one-call H1 step: the sparse stage runs beside the dense stage's tail (hybrid_query_dev)
  hipStream_t st2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool overlap_tail = true;           // HX_DEBUG_NO_OVERLAP (diagnostics): everything on the caller's stream
  bool beside = false;                // a stage of this call runs on the second stream while the dense scans run
  int scan_oversub = 4;               // ScanArgs.oversub of those scans (HX_DEBUG_SCAN_OVERSUB)
  int sp_host_late_min_b = 128;       // batches from here on: the host enqueues the dense scans before the sparse stage (HX_DEBUG_SP_HOST_LATE_MIN_B)
  int fork_early_max = 1 << 30;       // batches of at most this many queries start the sparse stage beside the dense SCAN
                                      // (HX_DEBUG_FORK_EARLY_MAX=0: beside the stage's tail only, as round 4 began)
  bool no_hq = false;
  bool no_qs = false;                 // HX_DEBUG_NO_QS (tests): never the query-stationary form of the staggered kernel (k_scan8q)
  // doc-major sparse staging (device)
  int64_t* sp_indptr = nullptr;  // [sp_rows_cap + 1]
  int32_t* sp_idx = nullptr;
  float* sp_val = nullptr;
  int64_t sp_rows = 0, sp_rows_cap = 0, nnz = 0, nnz_cap = 0;
  bool sparse_stale = false;
  // Inverted index = an immutable BASE over documents [0, base.n_docs) plus a TAIL over the documents added
  // since (rebuilt on every finalize from the tail's postings only); the base is rebuilt once the tail has
  // grown to a quarter of it.  Both are searched by the same select kernel; the exact scores come from the
  // document-major CSR, which covers every document.
  struct SparseIx {
    SparseBuildOut sp{};
    int64_t doc0 = 0, n_docs = 0;
    int n_segments = 0;
    int seg_docs = SEG_DOCS_SMALL;
  };
  SparseIx sp_base, sp_tail;
  int seg_docs_force = 0;             // HX_DEBUG_SEG_DOCS (tests): 32768 / 65536, 0 = by size
  int sp_cut_step = 0;                // HX_DEBUG_SP_CUTSTEP (diagnostics): keys between cuts of the select pass, 0 = default
  int64_t tail_min_force = -1;        // HX_DEBUG_TAIL_MIN (tests): documents a tail may hold before the base is rebuilt
  int64_t compact_chunk = 0;          // HX_DEBUG_COMPACT_CHUNK (tests): rows per chunk of hx_retain_rows, 0 = by the bounce buffer's size
  float sp_wmin = 0.f, sp_wmax = 0.f; // range of the document weights (all finite: checked at ingest)
  float sp_wmax_shared = 0.f;         // hx_set_sparse_wmax: the largest weight of any shard of the collection (0: unset)
  bool sp_have_w = false;
  int64_t sparse_fallbacks = 0;       // queries served by the document-at-a-time path
  Workspace ws;
  int64_t dense_fallbacks = 0, i8_fallbacks = 0, retries = 0;
  // max of a per-row scale over every 256-row tile: the int8 scans' column bound (scan8.hip)
  struct TileMax {
    float* v = nullptr;
    int64_t rows = -1, cap = 0;
  };
  TileMax tm_q8, tm_q8s;            // of q8_rinv (the "quantized" stage) and of q8s_scale (the candidate pass)
  int scan_logcap = SCAN8_LOGCAP;   // entries per wave log (HX_DEBUG_SCAN8_LOGCAP shrinks it: tests)
  // optional HIP-event profile of the scan / sparse kernels (hx_profile)
  struct ProfRec { hipEvent_t a, b; int what; double flops, bytes; };
  bool prof = false;
  std::vector<ProfRec> prof_recs;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
  unsigned long long* sp_counter = nullptr;   // postings of the queries' terms (k_sparse_prep) while profiling
  // One host round trip per batch for all the stages' failure flags: the small counters travel into this pinned
  // buffer ([0] a dense stage's failure count, [1..2] the sparse stage's summary) behind ONE synchronisation.
  int* pin = nullptr;
  bool sp_sum_pending = false;        // a sparse_enqueue's summary has not been consumed by sparse_resolve yet
  bool sp_sum_fetched = false;        // ... and is already in sp_sum (a dense stage's flag read took it along)
  int sp_sum[2] = {0, 0};             // flagged-or-failed queries, any invalid query

  // Insertion-order ids under row sharding.  Inside the engine a row's id is id_base + local
  // row.  What crosses the ABI is the row's GLOBAL id: rows arrive in blocks, block k = local rows
  // [row0[k], row0[k + 1]) with global ids gid0[k], gid0[k] + 1, ... (hx_set_next_id names the first id of the next
  // block; without it a block continues the previous one).  Both columns ascend, so the map is monotone: the order
  // (score desc, id asc) of a list is the same in both id spaces, and the remap is one pass over the keys a stage
  // hands out (and over the candidate keys hx_rescore takes in).  One block starting at id_base = the identity.
  struct IdBlocks {
    std::vector<uint32_t> row0, gid0;
    uint32_t* dev = nullptr;          // row0[0, nb) then gid0[0, nb)
    int dev_cap = 0;
    bool dirty = false;
    int64_t next = -1;                // hx_set_next_id: global id of the next appended row (-1: continue)
    int64_t end = -1;                 // global id after the last row (-1: no row yet)
  } ids;

  // Pre-filtered query (hx_hybrid_query_*_masked): while `on`, the whole-collection scans read
  // these gathered copies of the kept rows (view row i = local row rows[i]) and map their candidates back to this index's
  // rows before anything reads rows by id; the sparse stage tests `keep` at harvest.  A copy is gathered on first use in a
  // call (bit of `have`); the buffers hold `cap` rows (a power of two), persist across calls and are freed by
  // hx_release_mask_view or when a call needs more rows.
  struct MaskView {
    bool on = false;
    int64_t n = 0, cap = 0;
    const uint32_t* keep = nullptr;
    const uint32_t* rows = nullptr;
    unsigned have = 0;
    int8_t* q8s = nullptr;
    float* q8s_scale = nullptr;
    _Float16* dense_h = nullptr;
    _Float16* pre_h0 = nullptr;
    int8_t* q8 = nullptr;
    float* q8_rinv = nullptr;
    TileMax tm_q8, tm_q8s;
  } mv;

  // Payload index (hx_payload_*): columns of one (U32) or two (F64: low word, high word) planes of
  // uint32 per row, filled for rows [0, filled), filled <= n.  Ids are never reused.  A program and its sets travel
  // through one pinned staging buffer; pay_ev says when the device has taken the last one.
  // A list column (HX_PAY_LIST_*): p0 = the head plane (missing / null / 0 = a list), off = int64
  // offsets [filled + 1] into the element planes e0 (codes, or the low words of doubles) and e1 (the high words).
  // A text column (HX_PAY_TEXT) is stored the same way: p0 = the head plane (missing / null / the
  // row's byte length), off counts 32-bit words, e0 = the rows' bytes, each row padded with zero bytes to a word.
  // A token column (HX_PAY_TOKENS) likewise: p0 = missing / null / the row's token count Td, e0 =
  // per row Td x dim_t int8, then Td fp32 scales, then zero words up to a multiple of four words.
  struct PayCol {
    int id = 0, kind = 0;
    uint32_t* p0 = nullptr;
    uint32_t* p1 = nullptr;
    int64_t filled = 0, cap = 0;
    int64_t* off = nullptr;
    uint32_t* e0 = nullptr;
    uint32_t* e1 = nullptr;
    int64_t n_el = 0, el_cap = 0;
    int dim_t = 0;                    // HX_PAY_TOKENS: bytes of a token, fixed at creation
    bool list() const { return kind == HX_PAY_LIST_U32 || kind == HX_PAY_LIST_F64; }
    bool text() const { return kind == HX_PAY_TEXT; }
    bool tokens() const { return kind == HX_PAY_TOKENS; }
    bool csr() const { return list() || text() || tokens(); }   // offsets and element planes: what the lifecycle moves
  };
  std::vector<PayCol> pay;
  int reco_chunk0 = 0;                // HX_DEBUG_RECO_CHUNK0 (tests): rows of the first chunk of the recommend scan, 0 = the buffer's capacity
  int reco_cap = 0;                   // HX_DEBUG_RECO_CAP (tests): keys of a request's candidate buffer there, 0 = by the limit
  int discover_chunk0 = 0;            // HX_DEBUG_DISCOVER_CHUNK0 (tests): rows of the first chunk of the discover scan, 0 = the buffer's capacity
  int discover_cap = 0;               // HX_DEBUG_DISCOVER_CAP (tests): keys of a request's candidate buffer there, 0 = by the limit
  int bin_chunk0 = 0;                 // HX_DEBUG_BIN_CHUNK0 (tests): rows of the first chunk of the binary scan, 0 = the buffer's capacity
  int bin_cap = 0;                    // HX_DEBUG_BIN_CAP (tests): keys of a query's candidate buffer there, 0 = by the limit
  int bin_grid = 0;                   // HX_DEBUG_BIN_GRID (tests): the most workgroups of a binary scan launch, 0 = no cap
  int64_t discover_redone = 0;        // hx_discover_redone: requests that went through the overflow redo
  bool matrix_scan_only = false;      // HX_DEBUG_MATRIX_SCAN_ONLY (scripts/matrix_bench.py): hx_search_matrix stops behind k_matrix_scan, the outputs zeroed
  int pay_grid = 0;                   // HX_DEBUG_PAY_GRID (tests): caps the grid of the mask kernel, 0 = no cap
  int pay_next_id = 0;
  uint8_t* pay_pin = nullptr;
  size_t pay_pin_cap = 0;
  hipEvent_t pay_ev = nullptr;
  bool pay_ev_pending = false;

  void set_device() const { HX_HIP(hipSetDevice(device)); }
};

// the frame of every entry of the C ABI: an exception becomes hx_last_error() and the return value 1
#define HX_TRY try {
#define HX_CATCH                                  \
  }                                               \
  catch (const std::exception& e) {               \
    hx::set_last_error(e.what());                 \
    return 1;                                     \
  }                                               \
  catch (...) {                                   \
    hx::set_last_error("unknown error");          \
    return 1;                                     \
  }                                               \
  return 0;

namespace hx {

// ---- engine.hip ---------------------------------------------------------------------------------------------------------
// One stored per-row array.  row_arrays() lists them in the order they are grown and compacted in; the ones with in_file
// set, in that order, are the rows of a saved file.  A new stored copy of a row is added there (and to PrepRowsArgs and
// k_prep_rows, which derive it) and nowhere else in the host code.
struct RowArray {
  void** slot;                       // the field of hx_index that holds the array
  int64_t rb;                        // row bytes; 4 = one scale per row
  bool in_file;                      // hx_save writes it (q8s / q8s_scale are derived: hx_load makes them again)
  size_t arg;                        // where PrepRowsArgs holds the pointer k_prep_rows writes this array through
  void* p() const { void* v; std::memcpy(&v, slot, sizeof v); return v; }
  void set(void* v) const { std::memcpy(slot, &v, sizeof v); }
};
std::vector<RowArray> row_arrays(hx_index* h);
// the arguments of k_prep_rows that write row r onward of arrays laid out as the stored ones: base[i] stands for ra[i]
// (raw, n and nonfinite are the caller's)
PrepRowsArgs prep_rows_args(hx_index* h, const std::vector<RowArray>& ra, void* const* base, int64_t r);
void reserve_rows(hx_index* h, int64_t want);
void reserve_sparse(hx_index* h, int64_t rows, int64_t nnz);
void free_sparse_ix(hx_index::SparseIx& x);
void free_sparse_index(hx_index* h);
// the inverted index brought up to date with the stored sparse rows, as every sparse search does first (spstats.hip)
void sparse_up_to_date(hx_index* h, hipStream_t st);
void track_weights_dev(hx_index* h, const float* val, int64_t n, hipStream_t st);
bool ids_identity(const hx_index* h);
int* host_pin(hx_index* h);
void mask_rows_dev(hx_index* h, const uint32_t* mask_dev, uint32_t*& rows, uint32_t*& count_dev, hipStream_t st);
// the query as the *_host entries of poolstage.hip and byexample.hip run it (the comments are at the definitions)
void check_params(const hx_params* p);
void hybrid_query_dev(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv, int B,
                      const hx_params* p, uint64_t* out_keys, int* out_cnt, hipStream_t st, bool tree_sync = false);
void masked_query_dev(hx_index* h, const float* qd, const int64_t* qip, const int32_t* qix, const float* qv, int B,
                      const hx_params* p, const uint32_t* mask_dev, int64_t count_known, uint64_t* out_keys,
                      int* out_cnt, hipStream_t st);
bool masked_dense_dev(hx_index* h, const float* q_dev, int B, int L, const uint32_t* mask_dev, int64_t count_known,
                      uint64_t* out_keys, int* out_cnt, hipStream_t st);
void rescore(hx_index* h, const float* q_dev, int B, int prefix, const uint64_t* cand, int cstride, const int* ccnt, int L,
             uint64_t* out_keys, int* out_cnt, hipStream_t st);
void remap_out(hx_index* h, uint64_t* keys, int64_t n, hipStream_t st);
const uint64_t* remap_in(hx_index* h, const uint64_t* keys, int64_t n, hipStream_t st, int slot = WS_ID_IN);
void zero_outputs(uint64_t* keys, int* cnt, int B, int L, hipStream_t st);
int64_t host_mask_count(const hx_index* h, const uint32_t* mask_host);
uint32_t* host_mask_upload(hx_index* h, const uint32_t* mask_host, int slot, hipStream_t st);
void results_to_host(hx_index* h, uint64_t* keys, int64_t n, int sc_slot, int id_slot, float* scores, int64_t* ids,
                     hipStream_t st);
int* rows_check_begin(hx_index* h, hipStream_t st);
void rows_check_fetch(hx_index* h, int* w, hipStream_t st);
void rows_check_end(hx_index* h, int* w, hipStream_t st);
void check_sparse_batch_dev(hx_index* h, const int64_t* rows_ip, const int32_t* idx_dev, const float* val_dev, int64_t n,
                            int64_t first, int64_t last, const int64_t* indptr, const int32_t* idx, float* lo, float* hi);

// ---- binscan.hip: what the asymmetric stage (binasym.hip) shares with hx_search_bin --------------------------------------
// every refusal of a stage over the 1-bit copy that needs no device work
void bin_check(hx_index* h, const void* q_dev, int B, int limit, const void* mask_dev, int64_t mask_rows,
               const void* keys_dev, const void* counts_dev);
// What a stage gives the chunked scan loop: `queries` stages the batch as qwords words per query in the workspace slot
// q_slot and counts the non-finite queries in *bad; `scan` launches the scan of a.B queries over [a.row_begin, a.row_end),
// a.qbits being the staged form of the batch's query b0 (0 in the main loop, the flagged query's in the overflow redo).
struct BinStage {
  const char* who = "";              // names the stage in its messages
  int qwords = 0;
  int q_slot = 0;
  std::function<void(uint32_t* qdata, int* bad, hipStream_t st)> queries;
  std::function<void(const BinScanArgs& a, int b0, hipStream_t st)> scan;
};
void bin_stage_search(hx_index* h, const BinStage& s, int B, int L, const uint32_t* mask_dev, uint64_t* out_keys,
                      int* out_cnt, hipStream_t st);

// ---- lifecycle.hip: what a payload column's replace shares with hx_replace_rows -----------------------------------------
// the rows of a replace call -- in [0, limit), unique -- as the uint32 list the kernels read
std::vector<uint32_t> replace_rows_checked(const int64_t* rows_host, int64_t m, int64_t limit, const char* who);
// The splice of a CSR whose documents [f, total) take new lengths (replace.hip): the map document -> batch position,
// the new lengths and their exclusive prefix.  base = the offset of document f (it stays), moved = the postings from f
// on after the call.  splice_plan synchronises `st`.
struct SplicePlan {
  int64_t f = 0, docs = 0, base = 0, moved = 0;
  DevTmp map_, lenoff;
  const uint32_t* map() const { return (const uint32_t*)map_.p; }
  const int64_t* off() const { return (const int64_t*)lenoff.p + (docs + 1); }
};
void splice_plan(SplicePlan& s, const int64_t* indptr, int64_t total, int64_t f, const uint32_t* rows_dev, int64_t m,
                 const int64_t* new_indptr_dev, hipStream_t st);

// ---- formula.hip: every refusal of hx_formula that concerns the program (before any device work), and the program and
// its columns as the kernel's arguments hold them
void formula_lower(hx_index* h, const hx_formula_op* ops, int32_t n_ops, int32_t n_planes, FormulaArgs& a);

// ---- paystore.hip: a payload column as the engine and the lifecycle see it ------------------------------------------------
hx_index::PayCol& pay_col(hx_index* h, int32_t col);      // throws for an unknown id
void pay_free(hx_index::PayCol& c);
void pay_truncate(hx_index* h, int64_t n_rows);          // every column keeps min(filled, n_rows) rows
// hx_retain_rows: what moves with the rows of a column that is filled to the index's n rows -- its planes of one cell per
// row (p1 may be NULL) and, of a list or text column (off != NULL), the offsets and element planes (e1 may be NULL), which
// go the sparse CSR's way; the caller stores the new element count in *n_el.  pay_retained: those columns now hold `count`
// rows, a lagging one (filled < n) is dropped.
struct PayMoved {
  uint32_t *p0, *p1;
  int64_t* off;
  uint32_t *e0, *e1;
  int64_t* n_el;
};
std::vector<PayMoved> pay_moved(hx_index* h, int64_t n);
void pay_retained(hx_index* h, int64_t n, int64_t count);

}  // namespace hx
