// Kernel argument blocks and host-side launch prototypes (libhx, gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hx {

enum { KIND_F16 = 0, KIND_I8 = 1, KIND_F32 = 2 };

// Rigorous bound on |fp16-scan score - spec score| for unit-norm rows and queries
// (DESIGN.md "certificate"): input rounding 2*2^-11 + 2^-22, fp32 accumulation
// (D+19)*2^-24 for D <= 4096, plus the subnormal-half terms; 1.25e-3 has > 10 %
// slack over the sum for D <= 4096.
constexpr float HX_EPS_F16 = 1.25e-3f;

// ---- scan.hip ----------------------------------------------------------------
struct ScanArgs {
  const uint8_t* A;        // corpus matrix (fp16 or int8 rows), stride row_bytes
  const uint8_t* Q;        // query matrix [nq_tiles*BN x row_bytes], zero-padded rows
  int64_t row_bytes;       // multiple of 128
  int64_t row_begin, row_end;  // local rows scanned by this launch
  int B;                   // valid queries
  int nq_tiles;
  const float* tau;        // [B] append threshold (score >= tau passes)
  uint64_t* cand;          // [B x cap] candidate keys
  int* cnt;                // [B] appended so far (may exceed cap)
  int* overflow;           // [B] set when an append was dropped
  int cap;
  int64_t id_base;
  const float* rinv_x;     // i8: 1/||x|| per local row (padded)
  const float* rinv_q;     // i8: 1/||q|| per query (padded)
  const float* rinv_tile_max;  // i8, scan8: max of rinv_x over every 256-row tile (index: local row / 256)
  // scan8 only: per-wave append logs.  A passing (key, query) is stored -- fire and forget -- at
  // hitlog[wave * logcap + i]; launch_scatter_log moves the logs into cand/cnt afterwards.
  // hitlog == NULL (or a launch expected to pass most rows) selects the atomic-append kernel.
  uint4* hitlog;           // [SCAN8_WAVES x logcap x SCAN8_ENTRY]: {query, first row lo, hi, 0} + 16 scores
  int* hitcnt;             // [SCAN8_WAVES] entries written (may exceed logcap: the rest set overflow[q])
  int logcap;
  // k_scan only: tau is -inf and rows_end - row_begin <= cap, so every row has its own slot
  // (row - row_begin, key 0 for a NaN score or a row past n_total) and no counter is touched: the caller presets cnt.
  int all_pass;
  // scan8 only: the 256-row x 128-query form (65..128 queries; Q holds 128-row query tiles)
  int half_q;
  // scan8 only: never the query-stationary form (k_scan8q), whatever the shape (HX_DEBUG_NO_QS: tests)
  int no_qs;
  int oversub;             // k_scan only: k > 1 = k x the resident grid (less 32 workgroups), each with 1 / k of the static share --
                           // for a scan that runs BESIDE another stream's kernels: its two workgroups per CU take the whole LDS, so
                           // a workgroup of the other stream in the way at launch leaves a scan workgroup waiting for a whole
                           // round of its own kernel (measured: 1.2 -> 2.2 ms); queued shares are placed as others retire
  // Scan order.  [row_begin, row_end) are LOGICAL rows: logical 256-row tile t is physical tile
  // (t * perm_mul) mod perm_n (perm_n = 0: identity).  The stride is about 0.618 of the tile count, so every chunk of
  // the geometric scan is an even sample of the whole matrix: a corpus ingested document by document is topically
  // clustered, and a cluster that sat in ONE chunk would push hundreds of rows past a threshold that was set before
  // the scan reached it (buffer overflow, retry, exact path).  Row ids and validity follow the PHYSICAL row:
  // id = id_base + physical row, valid iff physical row < n_total.
  int64_t n_total;
  uint32_t perm_mul, perm_n;
  double perm_inv;         // 1.0 / perm_n
};
// (t * mul) mod n for t, mul < n < 2^24 (row ids are below 2^32, a tile is 256 rows): the product is exact in a
// double, the quotient estimate is off by at most one -- a handful of instructions instead of a 64-bit division
// inside the scan's tile cursor
__host__ __device__ inline uint32_t scan_phys_tile(uint32_t t, uint32_t mul, uint32_t n, double inv_n) {
  if (!n) return t;
  const double x = (double)t * (double)mul, dn = (double)n;
  double r = x - __builtin_floor(x * inv_n) * dn;
  r = r < 0.0 ? r + dn : r;
  r = r >= dn ? r - dn : r;
  return (uint32_t)r;
}
// The walk of one workgroup of k_scan8q (scan8.hip; its grid is always 256: 8 XCDs x 32 workgroups).  Workgroup
// (xcd, i0) keeps query tile i0 mod nq and is stream i0 / nq of nstreams = 32 / nq; it scans the 128-row halves
// u = stream + j * nstreams, j = 0, 1, ..., of its XCD's logical tiles (row_begin / 256 + (u >> 1) * 8 + xcd), each as a
// PAIR of 64-row items.  nstreams is even, so u keeps its parity and the logical tile advances by 4 * nstreams per pair:
// the physical tile advances by the constant step = (4 * nstreams * perm_mul) mod perm_n, one add and one conditional
// subtract in 32-bit integers -- exact, and nothing but SALU inside the item loop.  The modulo itself is taken twice per
// workgroup, for the start tile and for the step, in 64-bit integers (init runs in the kernel's prologue, where a
// division costs nothing that shows; scan_phys_tile's fp64 form gives the same values and stays with the kernels that
// take it once per twelve-phase item).  One code for the kernel and for the host (hx_scan8q_items).
struct Scan8qCursor {
  uint32_t tile;      // physical 256-row tile of the current pair
  uint32_t step;      // added per pair
  uint32_t wrap;      // perm_n, or 2^32 - 1 for the identity order (never reached)
  uint32_t sub;       // first row of the pair's half inside its tile: 0 | 128
  int n_items;        // 64-row items of this workgroup (even; 0: the stream has no rows)
  __host__ __device__ static inline uint32_t mulmod(uint32_t t, uint32_t mul, uint32_t n) {
    return n ? (uint32_t)(((uint64_t)t * (uint64_t)mul) % (uint64_t)n) : t;
  }
  __host__ __device__ inline void init(int64_t row_begin, int64_t row_end, int nq, uint32_t perm_mul, uint32_t perm_n,
                                       int xcd, int i0) {
    const int n_row_tiles = (int)((row_end - row_begin + 255) >> 8);
    const int stream = i0 / nq, nstreams = 32 / nq;
    const int halves_x = 2 * ((n_row_tiles - xcd + 7) >> 3);   // 128-row halves of this XCD's tiles
    n_items = stream < halves_x ? 2 * ((halves_x - stream + nstreams - 1) / nstreams) : 0;
    sub = (uint32_t)(stream & 1) * 128u;
    wrap = perm_n ? perm_n : 0xFFFFFFFFu;
    tile = mulmod((uint32_t)((row_begin >> 8) + (stream >> 1) * 8 + xcd), perm_mul, perm_n);
    step = mulmod((uint32_t)(4 * nstreams), perm_mul, perm_n);
  }
  __host__ __device__ inline uint32_t next_tile() const {
    const uint32_t p = tile + step;
    return p >= wrap ? p - wrap : p;
  }
  __host__ __device__ inline int64_t row0() const { return (int64_t)tile * 256 + sub; }   // odd item of the pair: + 64
};
constexpr int SCAN8_WAVES = 256 * 8;   // waves of the largest scan8 grid
constexpr int SCAN8_LOGCAP = 4096;      // most entries per wave log (expected: a few hundred per launch)
#ifndef HX_S8_TS
#define HX_S8_TS 16                     // MFMA tile side of scan8.hip: 16 (16x16x32) or 32 (32x32x16)
#endif
constexpr int SCAN8_ENTRY = 1 + (64 / HX_S8_TS) * (HX_S8_TS * HX_S8_TS / 64 / 4);   // 16-byte words per log entry
// after_kernel (optional): recorded on `st` right behind the scan kernel itself (before scan8's log scatter)
void launch_scan(const ScanArgs& a, int kind, int bn, hipStream_t st, hipEvent_t after_kernel = nullptr);
// scan8.hip: the 256 x 256 staggered-phase kernel behind launch_scan for large batches
bool scan8_usable(const ScanArgs& a, int bn);
void launch_scan8(const ScanArgs& a, int kind, hipStream_t st, hipEvent_t after_kernel = nullptr);   // includes the log scatter
// whether launch_scan8 takes the query-stationary form k_scan8q for this shape (host arithmetic; ScanArgs.no_qs aside)
bool scan8_qs_form(int kind, int half_q, int64_t row_bytes, int nq_tiles);
// waves that share the appends of a launch over `tiles` 256-row tiles, by form
double scan8_log_waves(int64_t tiles, int nq_tiles, bool qs);

// ---- select.hip --------------------------------------------------------------
// Sort each query's buffer (first min(cnt, stride) keys) best-first, optionally drop
// duplicate keys, keep `keep`; writes out_keys[b*out_stride + r] (may alias `keys`
// when out_stride == stride), out_cnt[b], and tau[b] = score of the keep-th key when
// the list is full, else -inf (tau may be NULL).  in_cnt NULL => all `stride` slots.
// tau_rank (1-based, default keep): rank whose score becomes tau.  kept_io (optional): per-list
// count kept by the previous compaction of the same buffer, updated; with chk_rank > 0 the
// list is flagged in `underflow` when chk_rank + (keys appended since) < keep.
void launch_compact(uint64_t* keys, int stride, const int* in_cnt, int B, int keep, int dedupe,
                    uint64_t* out_keys, int out_stride, int* out_cnt, float* tau,
                    int max_cnt_hint, hipStream_t st, int tau_rank = 0, int chk_rank = 0,
                    int* kept_io = nullptr, int* underflow = nullptr);
// The kernel launch_compact picks for lists of at most list_len (= min(max_cnt_hint, stride)) keys: k_compact_top<nw, e>
// (a wave sorts 64 e keys in registers, nw waves fold), or {0, 0} = k_compact, the LDS sort.  No device, no launch.
struct CompactForm {
  int nw, e;
};
CompactForm compact_form(int list_len, int keep, int dedupe);

// Exact spec score of listed candidates: out_keys[b*stride + i] = key(spec_dot(row, q_b), id)
// for i < min(cnt[b], stride); ids outside [id_base, id_base+n) give key 0.
struct RescoreArgs {
  int kind;                // KIND_F32 (spec_dot over fp32 rows) or KIND_I8
  const void* M;           // matrix base
  int64_t row_stride;      // elements per row
  int dim_pad;             // padded dim (multiple of 64)
  const void* Q;           // prepared queries: f32 [B x dim_pad] or i8 [B x row_stride]
  int64_t q_stride;
  const float* rinv_x;     // i8 only
  const float* rinv_q;     // i8 only
  int64_t n_rows;
  int64_t id_base;
  const uint64_t* cand;    // [B x stride]
  const int* cnt;          // [B] (NULL => stride)
  int stride;
  int B;
  uint64_t* out;           // [B x stride]
  int max_cnt;             // upper bound of cnt[] (0: stride): sizes the grid; slots beyond it are NOT written
};
void launch_rescore_list(const RescoreArgs& a, hipStream_t st);
// as launch_rescore_list for a list that is mostly OTHER shards' rows: only this shard's slots are scored and written
void launch_rescore_own(const RescoreArgs& a, hipStream_t st);
// exact re-score of the (<= 512) candidates of every query + top-L + the certificate of launch_certify, one launch
// (r.out = scratch [B x stride]; done = [B] zeroed counters, left zero).  Returns false when dense_finish_e says the
// sizes do not fit (more than 64 queries, lprime or L above 512): use launch_rescore_list + launch_compact +
// launch_certify.  nb_force > 0: that many blocks per query instead of one per four candidates (tests).
bool launch_dense_finish(const RescoreArgs& r, int lprime, int L, uint64_t* out_keys, int* out_cnt, const int* overflow,
                         float eps, const float* eps_q, int* fail, int* nfail, unsigned int* done, hipStream_t st,
                         int nb_force = 0);
// Keys per lane (2 | 4 | 8) of the k_dense_finish instantiation that serves B queries with lprime candidates and limit
// L, 0 when the three launches serve them.  No device, no launch.
int dense_finish_e(int B, int lprime, int L);

// Exact scores of ALL rows [row_begin,row_end) for the listed queries (fallback path):
// out[qsel[f]*stride + slot0 + (row-row_begin)] = key.
struct RangeArgs {
  RescoreArgs r;           // cand/cnt/out/stride reused: out = buffer, stride = its stride
  const int* qsel;         // [nsel] query indices
  int nsel;
  int64_t row_begin, row_end;
  int slot0;
};
void launch_rescore_range(const RangeArgs& a, hipStream_t st);

// fail[b] = overflow[b] || (approx_cnt[b] >= lprime && !(approx_Lprime_score + eps < exact_L_score))
// eps_q (optional): a radius per query instead of the common `eps`
void launch_certify(const uint64_t* approx_keys, int approx_stride, const int* approx_cnt, int lprime,
                    const uint64_t* exact_keys, int exact_stride, const int* exact_cnt, int L,
                    const int* overflow, float eps, int B, int* fail, int* nfail, hipStream_t st,
                    const float* eps_q = nullptr);

void launch_rrf(const uint64_t* a, int a_stride, const int* a_cnt, const uint64_t* b, int b_stride,
                const int* b_cnt, int B, float k, int rank_base, int limit, uint64_t* out,
                int* out_cnt, hipStream_t st);
// fusion + top-`limit` in one launch when both lists together hold at most 256 keys (returns false otherwise: use
// launch_rrf + launch_compact); out [B x out_stride], out_cnt [B]
bool launch_rrf_top(const uint64_t* a, int a_stride, const int* a_cnt, const uint64_t* b, int b_stride, const int* b_cnt,
                    int B, float k, int rank_base, int limit, uint64_t* out, int out_stride, int* out_cnt, hipStream_t st);
// ---- fuse.hip: N-way fusion (hx_fuse) ------------------------------------------------------------
constexpr int FUSE_MAX_LISTS = 8;        // HX_FUSE_MAX_LISTS
constexpr int FUSE_MAX_SLOTS = 4096;     // HX_FUSE_MAX_SLOTS
constexpr int FUSE_SMALL_SLOTS = 256;    // strides summing to at most this: the one-wave form
struct FuseArgs {
  const uint64_t* keys[FUSE_MAX_LISTS];  // list l of query b: keys[l] + b * stride[l]
  const int* cnt[FUSE_MAX_LISTS];        // [B] each
  int stride[FUSE_MAX_LISTS];
  float w[FUSE_MAX_LISTS];
  int n_lists, method;                   // HX_FUSE_RRF / HX_FUSE_DBSF
  float k;
  int rank_base, limit;
  uint64_t* out;                         // [B x limit]
  int* out_cnt;                          // [B]
};
// 0 = the one-wave form (k_fuse<64, 4>), 1 = the general one (k_fuse<512, 8>): host arithmetic only
int fuse_form(int total_slots);
void launch_fuse(const FuseArgs& a, int B, hipStream_t st);
void launch_unpack(const uint64_t* keys, int64_t n, float* scores, int64_t* ids, hipStream_t st);
// out[b*(sa+sb) ...] = a-list then b-list (empty slots 0)
void launch_concat(const uint64_t* a, int a_stride, const int* a_cnt, const uint64_t* b, int b_stride,
                   const int* b_cnt, int B, uint64_t* out, hipStream_t st);
void launch_regroup(const uint64_t* g, int world, int B, int dl, int sl, uint64_t* d, uint64_t* s, hipStream_t st);
void launch_scan_init(float* tau, int* cnt, int* ovf, int* kept, int B, int cnt0, hipStream_t st);
void launch_fill_f32(float* p, int64_t n, float v, hipStream_t st);
void launch_fill_i32(int* p, int64_t n, int v, hipStream_t st);
void launch_flag_row(const int* nfail, const int* spsum, uint64_t* row, int len, hipStream_t st);
void launch_flag_add(int* acc, const int* add2, hipStream_t st);   // *acc += add2[0] + add2[1]
// internal id (id_base + local row) <-> global insertion-order id through the index's block table (select.hip)
void launch_remap_ids(const uint64_t* in, uint64_t* out, int64_t n, const uint32_t* row0, const uint32_t* gid0, int nb,
                      uint32_t id_base, uint32_t n_rows, int to_global, hipStream_t st);

// ---- shardx.hip: row-sharded H1, candidates exchanged before the exact scores ----------------
void launch_h1x_pack(const uint64_t* cand, int cstride, const int* cnt, const int* ovf, const float* eps, int complete,
                     int k1, const uint64_t* list, int lstride, const int* lcnt, const int* sflag, const int* sfail, int k2,
                     int lout, float wmax, int B, uint64_t* nom, hipStream_t st, const int* qbad = nullptr);
void launch_h1x_union(const uint64_t* g, int world, int B, int k1, int k2, uint64_t* du, uint64_t* su, hipStream_t st);
void launch_h1x_cuts(const uint64_t* g, int world, int B, int k1, int k2, const uint64_t* G, const int* gc, int lp,
                     const uint64_t* ST, const int* sc, int L_s, const int64_t* q_indptr, uint64_t* meta, uint32_t* thr_out,
                     int* q_margin, int* q_flag, hipStream_t st);
void launch_h1x_counts(const uint64_t* priv_cnt, int B, int* out, hipStream_t st);
void launch_h1x_place(const uint64_t* T, const int* tc, const int* ncand, const int* sp_fail, int B, int k3, int world,
                      int rank, uint64_t* se, uint64_t* nc, uint64_t* meta, hipStream_t st);
void launch_h1x_certify(const uint64_t* red, int world, int B, int lp, int k3, const uint64_t* D, const int* Dc, int L,
                        const uint64_t* S, const int* Sc, int L_s, int* fail, int* nfail, hipStream_t st);

// ---- prep.hip ----------------------------------------------------------------
// Derive the stored vectors of rows [0,n) of `raw` (fp32 [n x dim]):
struct PrepRowsArgs {
  const float* raw;        // [n x dim]
  int dim, dim_pad;        // dim_pad = round_up(dim, 64)
  int64_t n;
  float* dense;            // [n x dim_pad] L2-normalised (zero padded)
  _Float16* dense_h;       // [n x dim_pad]
  int8_t* q8;              // [n x dim_pad8] trunc(127*x) of the RAW row
  int dim_pad8;            // round_up(dim, 128)
  float* q8_rinv;          // [n]
  int n_prefix;
  int psize[3];
  float* pre[3];           // [n x psize] normalised prefixes of the RAW row
  _Float16* pre_h0;        // fp16 copy of prefix 0 (may be NULL)
  // candidate-pass copy of the NORMALISED row (may be NULL): rint(x * 127 / max|x|), its scale max|x| / 127, and
  // the running maximum over all rows of the quantisation error ||x - scale * x8||_2 (fp32 bits, rounded up)
  int8_t* q8s;             // [n x dim_pad8]
  float* q8s_scale;        // [n]
  uint32_t* err_max;       // one device word
  int* nonfinite;          // one device word (may be NULL): set to 1 when a row holds a NaN or +-Inf element
  // 1-bit copy of the NORMALISED row (may be NULL): k_prep_rows does not read the field --
  // launch_prep_rows runs k_binarize_rows behind it on the same stream, over the `dense` rows that launch just wrote
  uint32_t* bits;          // [n x bits_words]
  int bits_words;          // words of a row of `bits`: at least dim_pad / 32, a multiple of four
};
void launch_prep_rows(const PrepRowsArgs& a, hipStream_t st);
// bits[r * words + (j >> 5)] bit (j & 31) = dense[r * dim_pad + j] > 0 for j < dim_pad, 0 up to 32 * words
void launch_binarize_rows(const float* dense, int dim_pad, int words, int64_t n, uint32_t* bits, hipStream_t st);
void launch_requant_rows(const float* dense, int dim_pad, int dim_pad8, int64_t n, int8_t* q8s, float* scale,
                         uint32_t* err_max, hipStream_t st);
// candidate-pass form of normalised queries qn [B x dpad]: int8 rows [Bpad x dpad8], scales [Bpad], certificate
// radius per query [B] from the index's largest row quantisation error (*err_max)
void launch_prep_queries_s8(const float* qn, int dpad, int B, int Bpad, int dpad8, int8_t* q8, float* sq, float* eps,
                            const uint32_t* err_max, hipStream_t st);
// out[t] = max of the non-negative floats p[256 t, 256 t + 256) (clipped to n)
void launch_tile_max(const float* p, int64_t n, float* out, hipStream_t st);
void launch_synth_dense(float* raw, int64_t row0_global, int64_t n, int dim, uint32_t seed, hipStream_t st);

// Prepare a query batch for one named vector: normalised fp32 [B x dpad] (+ fp16
// zero-padded to Bpad rows) from raw q[:, :d]; or the int8 copy + rinv.
// bad (optional, device): += the number of queries with a NaN or +-Inf among their q_dim raw elements.
void launch_prep_queries_f(const float* q_raw, int q_dim, int B, int Bpad, int d, int dpad,
                           float* qn, _Float16* qh, hipStream_t st, int* bad = nullptr);
void launch_prep_queries_i8(const float* q_raw, int q_dim, int B, int Bpad, int dpad8, int8_t* q8,
                            float* rinv_q, hipStream_t st, int* bad = nullptr);

// ---- sparse2.hip / sprescore.hip ------------------------------------------------
// K7 in two passes (DESIGN.md "sparse stage"):
//   select  -- term-at-a-time over the inverted index with a 16-bit integer accumulator per document
//              (two documents per LDS word): segments of 32768 / 65536 documents per visit.  The integer
//              score `a` brackets the real one (u = score * scale, a - 1.01 k <= u <= a + 0.01 k for k
//              matching terms), so every document that can reach the exact top-L has a > a_L - M
//              (a_L = L-th best integer score, M = the query's margin): the pass keeps exactly those;
//   rescore -- the exact score of every kept candidate from the document-major CSR in upstream's order
//              (query terms in ascending term id, fp32 mul, fp32 add), then the top-L by key.
// Queries the integer pass cannot serve (a non-positive weight, more than SP_TMAX terms, a candidate
// buffer that overflowed) are flagged and re-run document-at-a-time over all rows (k_sparse_range).
constexpr int SEG_DOCS_SMALL = 32768, SEG_DOCS_LARGE = 65536;
constexpr int SP_TMAX = 64;            // query terms the select pass takes (one lane each)
// Term-major inverted index over the documents [doc0, doc0 + n_docs) of the shard: the postings of live
// term i (ascending document) are post[ptr[i*(n_segments+1) + 0] .. ptr[i*(n_segments+1) + n_segments]);
// ptr[i*(S+1) + s] is the first posting of term i whose document lies in segment s or later.  A posting
// is {the document's place in the select pass's accumulator: byte offset of its 32-bit LDS word (document index
// inside the segment mod seg_docs/2, times 4) | shift of its 16-bit half (0 / 16) << 24, fp32 weight bits}.
struct SparseIndexView {
  const uint2* post;           // [nnz] (+ 16 bytes of padding)
  const uint32_t* ptr;         // [n_live x (n_segments + 1)]
  const uint32_t* uterms;      // [n_live] live term ids, ascending
  int n_live;
  int64_t n_docs;
  int n_segments;
  int seg_docs;                // SEG_DOCS_SMALL or SEG_DOCS_LARGE
  int64_t id_base;             // global id of the view's first document
};
// per-query preparation, one wave per query: validity, scale, margin, live-term index of every term
struct SparsePrepArgs {
  const int64_t* q_indptr;     // [B+1]
  const int32_t* q_idx;        // ascending within a query
  const float* q_val;
  int B;
  SparseIndexView ix[2];       // base index and (optional, n_live = 0) tail index
  float wmax;                  // largest document weight of the shard
  int index_nonpos;            // some document weight is <= 0: the integer pass cannot bracket scores
  int32_t* q_ti[2];            // [B x SP_TMAX] live-term index per view, -1 = absent
  float* q_qs;                 // [B x SP_TMAX] query weight * scale
  int* q_margin;               // [B]
  int* q_flag;                 // [B] 0 ok, 1 = needs the document-at-a-time path, 2 = invalid (non-finite weight),
                               //     3 = invalid (term ids not strictly ascending, or negative)
  unsigned long long* q_work;  // [B] postings of the query's terms (both views): launch order, profile
  unsigned long long* stat_postings;   // optional: += sum of q_work
};
void launch_sparse_prep(const SparsePrepArgs& a, hipStream_t st);
struct SparseSelectArgs {
  SparseIndexView ix;
  const int64_t* q_indptr;
  const int32_t* q_ti;         // [B x SP_TMAX] for THIS view
  const float* q_qs;
  const int* q_margin;
  const int* q_flag;
  int B;
  int parts;                   // most workgroups per query; query q is cut into q_parts[q] of them
  const int* q_parts;          // [B] in [1, parts] (NULL: all `parts`): each owns a contiguous segment range
  const int* items;            // launch plan (NULL: workgroup b = query b / parts, part b % parts): query << 8 | part
  const int* n_items;
  int limit;
  int lout;                    // keys kept per (query, part) at most
  uint64_t* out;               // [B x parts_total x lout] integer-score keys, best first, 0 = empty
  int* out_cnt;                // [B x parts_total]
  int parts_total, part0;      // this launch writes parts [part0, part0 + parts) of every query
  uint64_t* cand;              // [B x parts x (seg_docs + seg_docs/8)] workgroup-private candidate buffers
  int* q_fail;                 // [B] set when a buffer overflowed: the query takes the exact path
  int cut_step;                // keys the buffer grows by between cuts (0: max(1024, 4 * limit))
  const uint32_t* keep;        // row mask of a pre-filtered query (NULL: every row): bit r of keep = local row r
  uint32_t keep_base;          // internal id of local row 0 (the index's id_base)
};
void launch_sparse_select(const SparseSelectArgs& a, hipStream_t st);   // dispatches on a.ix.seg_docs
void launch_sparse_summary(const int* flag, const int* fail, int B, int* out, hipStream_t st);
namespace v32k { void launch_sparse_select_variant(const SparseSelectArgs& a, hipStream_t st); }
namespace v64k { void launch_sparse_select_variant(const SparseSelectArgs& a, hipStream_t st); }
// q_parts[q] in [1, pt_max]: workgroups the query is cut into; items[0, *n_items): query << 8 | part, heaviest first
void launch_sparse_plan(const unsigned long long* q_work, int B, int pt_max, int slots, int* q_parts, int* items,
                        int* n_items, hipStream_t st);
// document-major CSR of the shard (what the ingest path appends)
struct SparseCsr {
  const int64_t* indptr;       // [n_docs + 1]
  const int32_t* idx;
  const float* val;
  int64_t n_docs;
  int64_t id_base;
};
// exact (upstream-order fp32) scores of the kept candidates of every query
struct SparseRescoreArgs {
  SparseCsr d;
  const int64_t* q_indptr;
  const int32_t* q_idx;
  const float* q_val;
  const uint64_t* cand;        // [B x stride] integer-score keys, best first
  const int* cnt;              // [B]
  int stride;
  int B;
  int limit;
  const int* q_margin;
  const int* q_flag;
  uint64_t* out;               // [B x stride] exact keys of the candidates: slots [0, out_cnt[b]) (0 = foreign id)
  int* out_cnt;                // [B] candidates = the prefix of the list within the margin of its L-th key
  int* q_fail;                 // set when the list was cut short of the margin
  int blocks;                  // workgroups (of 4 waves) per query; 0: 32 (a list of ~110 candidates, more when the L-th ties)
  const uint32_t* thr_in;      // optional [B]: the integer-score threshold to apply instead of the list's own
                               // (a shard of the candidates-first exchange applies the GLOBAL one: shardx.hip)
};
void launch_sparse_rescore(const SparseRescoreArgs& a, hipStream_t st);
// out[b] = the parts' lists of query b packed into one run (stride pt * lout), out_cnt[b] = its length
void launch_sparse_pack(const uint64_t* parts, const int* pcnt, int B, int pt, int lout, uint64_t* out, int* out_cnt,
                        hipStream_t st);
// exact scores of ALL documents [row_begin, row_end) for the listed queries (document-at-a-time path).
// tau == NULL: out[f*stride + slot0 + (row - row_begin)] = key, 0 when the document shares no term with the query.
// tau != NULL: keys with score >= tau[f] are appended at out[f*stride + atomicAdd(cnt[f], 1)]; ovf[f] = 1 when full.
struct SparseRangeArgs {
  SparseCsr d;
  const int64_t* q_indptr;
  const int32_t* q_idx;
  const float* q_val;
  const int* qsel;
  int nsel;
  int64_t row_begin, row_end;
  uint64_t* out;
  int stride, slot0;
  const float* tau;
  int* cnt;
  int* ovf;
  const uint32_t* keep;        // row mask of a pre-filtered query (NULL: every row): rows whose bit is clear score nothing
};
void launch_sparse_range(const SparseRangeArgs& a, hipStream_t st);
// {min, max} of val[0, n) merged into mm[0], mm[1] (fp32, device); mm[2] counts non-finite values
void launch_minmax_f32(const float* val, int64_t n, float* mm, hipStream_t st);
// n_rows rows of a device CSR whose offsets start at indptr_rows: *bad |= 1 unless indptr_rows[0] = first, the offsets
// are monotone and indptr_rows[n_rows] = last; *bad |= 2 if an idx in [first, last) is negative
void launch_csr_check(const int64_t* indptr_rows, const int32_t* idx, int64_t n_rows, int64_t first, int64_t last, int* bad,
                      hipStream_t st);
// term ids unique within every row (what hx_add_sparse enforces and k_sparse_rescore's one-ballot-per-term relies
// on): *bad |= 4 on a duplicate.  Rows longer than CSR_UNIQUE_WAVE_MAX terms are not compared on the device: their
// indices go to long_rows[0, *n_long) (at most long_cap are listed; *n_long keeps counting) for the host to check.
constexpr int CSR_UNIQUE_WAVE_MAX = 2048;
void launch_csr_unique(const int64_t* indptr, const int32_t* idx, int64_t n_rows, int* bad, int64_t* long_rows,
                       int long_cap, int* n_long, hipStream_t st);

// ---- mask.hip: row masks of the pre-filtered query (hx_hybrid_query_*_masked) ---------------------------------------
// mask [ceil(n/32) words] -> rows[0, *count) = the kept local rows, ascending; blk = ceil(n/8192) words of scratch.
// Everything enqueued: *count is on the device.
void launch_mask_rows(const uint32_t* mask, int64_t n, uint32_t* blk, uint32_t* rows, uint32_t* count, hipStream_t st);
// dst row i = src row rows[i] (row_bytes a multiple of 16), and the same for one 4-byte value per row
void launch_gather_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                          hipStream_t st);
void launch_gather_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st);
// keys of a scan of the view (internal ids id_base + view row) -> internal ids id_base + rows[view row], in place
void launch_view_ids(uint64_t* keys, int64_t n, const uint32_t* rows, uint32_t count, uint32_t id_base, hipStream_t st);

// ---- compact.hip: per-point deletes (hx_retain_rows) ------------------------------------------------------------------
// dst row i = src row rows[i], i < count (row_bytes a multiple of 16; one 4-byte value per row for _u32).  src and dst
// may be one allocation as long as the launch reads no byte it writes (lifecycle.hip cuts the rows into such chunks).
void launch_compact_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                           hipStream_t st);
void launch_compact_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st);
// plain copies between disjoint buffers (bytes a multiple of 16 / n 4-byte words)
void launch_copy16(const void* src, void* dst, int64_t bytes, hipStream_t st);
void launch_copy_u32(const void* src, void* dst, int64_t n, hipStream_t st);
// document-major CSR: len[j] = postings of document rows[j] (j < m); the segmented copy of those documents' postings
// to idx2 / val2 at off[j] (off = exclusive prefix of len, off[m] = total) with the min / max of the copied weights
// merged into mm[0] / mm[1] (orderable u32, as launch_minmax_f32); indptr[j] = base + off[j] for j <= m
void launch_csr_keep_len(const int64_t* indptr, const uint32_t* rows, int64_t m, int64_t* len, hipStream_t st);
void launch_csr_compact(const int64_t* indptr, const uint32_t* rows, const int64_t* off, int64_t m, const int32_t* idx,
                        const float* val, int32_t* idx2, float* val2, uint32_t* mm, hipStream_t st);
void launch_csr_new_indptr(int64_t* indptr, const int64_t* off, int64_t m, int64_t base, hipStream_t st);

// ---- spbuild.hip -------------------------------------------------------------
struct SparseBuildOut {
  uint2* post;
  uint32_t* ptr;
  uint32_t* uterms;
  int64_t n_live;
  int64_t ptr_entries;
};
// Build the term-major inverted index of documents [doc0, doc0 + n_docs) from the doc-major CSR on the
// device (indptr is the shard's: indptr[doc0] is the first posting taken).
void build_sparse_index(const int64_t* indptr, const int32_t* idx, const float* val, int64_t doc0, int64_t n_docs,
                        int seg_docs, SparseBuildOut* out, hipStream_t st);
// Synthetic docs (oracle synth_sparse_docs): two passes.
void synth_sparse_count(int64_t doc0_global, int64_t n, uint32_t seed, const uint32_t* cdf, int V,
                        const uint16_t* len_tab, int64_t* nnz_per_doc, hipStream_t st);
void synth_sparse_fill(int64_t doc0_global, int64_t n, uint32_t seed, const uint32_t* cdf, int V,
                       const uint16_t* len_tab, const int64_t* indptr, int32_t* idx, float* val,
                       hipStream_t st);
void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, hipStream_t st);  // out[n] = total

// ---- payload.hip: the payload index (hx_payload_mask) ----------------------------------------------
// One op of a program as the kernel reads it: paystore.hip resolves the columns of hx_pay_op to their planes (p0 = the
// cell of a U32 column or the low word of an F64 cell, p1 = its high word or NULL) and the sets to device pointers
// (imm; cnt = entries).  Codes from PAY_D_FIRST_COL on read a column.
// A list column gives p0 = its head plane (p1 = NULL: the head reads as a U32 cell), off = its
// int64 offsets [n + 1] and e0 / e1 = its element planes (e1 = the high words of doubles or NULL).  Codes from
// PAY_D_FIRST_LIST on walk the elements; ANY_RANGE carries its closed interval in imm / imm2 (the bits of two doubles).
// PAY_D_BITS is device-only: imm = a packed verdict plane in the mask's layout, written by
// k_payload_text in front of the mask kernel on the same stream; the op pushes the row's bit of it.
enum PayDevOp : uint32_t {
  PAY_D_TRUE = 0, PAY_D_FALSE, PAY_D_AND, PAY_D_OR, PAY_D_NOT, PAY_D_ROW_IN, PAY_D_BITS,
  PAY_D_FIRST_COL, PAY_D_IS_MISSING = PAY_D_FIRST_COL, PAY_D_IS_NULL, PAY_D_PRESENT, PAY_D_EQ_U32, PAY_D_IN_U32,
  PAY_D_EQ_F64, PAY_D_IN_F64, PAY_D_LT, PAY_D_LE, PAY_D_GT, PAY_D_GE,
  PAY_D_FIRST_LIST, PAY_D_IS_EMPTY_LIST = PAY_D_FIRST_LIST, PAY_D_ANY_EQ_U32, PAY_D_ANY_IN_U32, PAY_D_ANY_EQ_F64,
  PAY_D_ANY_IN_F64, PAY_D_ANY_RANGE
};
struct PayOpDev {
  uint32_t op, cnt;
  uint64_t imm;
  const uint32_t* p0;
  const uint32_t* p1;
  const int64_t* off;
  const uint32_t* e0;
  const uint32_t* e1;
  uint64_t imm2;
};
constexpr int PAY_INLINE_SET = 8;   // sets up to here are compared entry by entry, larger ones searched
// mask[ceil(n / 32)] = the verdicts of the program over rows [0, n) (bits at or past n zero); *kept += their number
// when kept is not NULL (the caller zeroes it).  grid_cap > 0 caps the grid (HX_DEBUG_PAY_GRID: tests).
void launch_payload_mask(const PayOpDev* prog, int n_ops, int64_t n, uint32_t* mask, uint32_t* kept, int grid_cap,
                         hipStream_t st);
// ---- paytext.hip: HX_PAY_TEXT_ALL -------------------------------------------------------------
// One pattern as the kernel reads it: its length in bytes (1 to 64), the mask of its first min(len, 4) bytes and the
// bytes themselves as little-endian words, zero-padded.
struct PayTextPat {
  uint32_t len, fmask;
  uint32_t w[16];
};
// plane[ceil(n / 32)] (the mask's layout, bits at or past n zero): bit r = every one of the n_pats patterns (1 to 32)
// occurs within the bytes of row r of a text column -- head = its head plane (missing, null or the byte length), off =
// its int64 offsets in 32-bit words, text = its word plane (rows padded with zero bytes to a word; below 2^31 words, and
// allocated to a multiple of four words).  grid_cap as launch_payload_mask takes it.
void launch_payload_text(const uint32_t* head, const int64_t* off, const uint32_t* text, int64_t n, const PayTextPat* pats,
                         int n_pats, uint32_t* plane, int grid_cap, hipStream_t st);
// ---- paynested.hip: HX_PAY_NESTED -------------------------------------------------------------
// One ELEMENT op as the kernel reads it: slot = which of the block's distinct columns it reads; a set as a device
// pointer in imm with cnt entries, EL_RANGE's closed interval in imm / imm2 (the bits of two doubles).
enum PayElOp : uint32_t {
  PAY_E_TRUE = 0, PAY_E_FALSE, PAY_E_AND, PAY_E_OR, PAY_E_NOT, PAY_E_EQ_U32, PAY_E_IN_U32, PAY_E_EQ_F64, PAY_E_IN_F64,
  PAY_E_RANGE
};
struct PayElOpDev {
  uint32_t op, slot, cnt, pad;
  uint64_t imm, imm2;
};
constexpr int PAY_NESTED_COLS = 8;    // HX_PAY_NESTED_MAX_COLS
// the element planes of a block's distinct columns (e1 = the high words of doubles or NULL), slots [0, n_cols)
struct PayNestedCols {
  const uint32_t* e0[PAY_NESTED_COLS];
  const uint32_t* e1[PAY_NESTED_COLS];
  int n_cols;
};
// plane[ceil(n / 32)] (the mask's layout, bits at or past n zero): bit r = some element position in
// [off[r], off[r + 1]) makes the element program (1 to 64 ops, leaving one entry) true.  off = the anchor's int64 offsets
// [n + 1]; every plane of `cols` (a table in device memory) holds at least off[n] elements.  grid_cap as launch_payload_mask takes it.
void launch_payload_nested(const int64_t* off, int64_t n, const PayNestedCols* cols, const PayElOpDev* prog, int n_ops,
                           uint32_t* plane, int grid_cap, hipStream_t st);
// *same (the caller sets it to 1) becomes 0 when head_a[r] != head_b[r] for a row r < n or off_a[r] != off_b[r] for r <= n
void launch_payload_same_offsets(const uint32_t* head_a, const uint32_t* head_b, const int64_t* off_a, const int64_t* off_b,
                                 int64_t n, uint32_t* same, hipStream_t st);
// ---- group.hip: grouped search (hx_group) ------------------------------------------------------
constexpr uint32_t HX_GROUP_MISSING = 0xFFFFFFFFu, HX_GROUP_NULL = 0xFFFFFFFEu;   // HX_PAY_U32_MISSING / _NULL of hx.h
// Per query b: the ranked list keys[b * stride + i], i < counts[b] (NULL: stride), 0 = an empty slot; ikeys = the same
// slots with internal ids (id_base + row; the same pointer where the two id spaces are one), which name the row whose
// cell p0[row] is the group.  out[b * G * S + g * S + r] = the r-th hit of the g-th group (a key of `keys`, 0 = empty),
// group_codes[b * G + g] = its code (HX_GROUP_MISSING for a group that was not opened), group_counts[b] = groups opened.
struct GroupArgs {
  const uint64_t* keys;
  const uint64_t* ikeys;
  int stride;              // 1 .. 2048
  const int* counts;
  const uint32_t* p0;      // the cells of rows [0, n_rows)
  int64_t n_rows;
  uint32_t id_base;
  int n_groups, group_size;   // G, S >= 1, G * S <= 2048
  uint64_t* out;
  uint32_t* group_codes;
  int* group_counts;
};
void launch_group_select(const GroupArgs& a, int B, hipStream_t st);
// ---- listkeep.hip: a ranked list filtered by a row mask and / or a score threshold (hx_list_keep)
// Per query b < B: the walk of keys[b * stride + r], r < counts[b] clamped to [0, stride] (NULL: stride), in rank order.
// Slot r is kept when its key is not 0, (mask != NULL) the id of ikeys[b * stride + r] -- the same slot with internal ids,
// id_base + row; the same pointer where the two id spaces are one; 0 = an id of another index -- names a row of [0, n_rows)
// whose bit row & 31 of mask[row >> 5] is set, and (thr != NULL) !(score < thr[b]) in fp32.  out[b * limit + t] = the t-th
// kept key of `keys` as it came, t < limit, 0 after them; out_counts[b] = the keys written.
struct ListKeepArgs {
  const uint64_t* keys;
  const uint64_t* ikeys;
  int stride;              // 1 .. 8192
  const int* counts;
  int B;
  const uint32_t* mask;    // ceil(n_rows / 32) words, or NULL
  int64_t n_rows;
  uint32_t id_base;
  const float* thr;        // B thresholds, or NULL
  int limit;               // 1 .. 8192
  uint64_t* out;
  int* out_counts;
};
void launch_list_keep(const ListKeepArgs& a, hipStream_t st);
// ---- mmr.hip: MMR search (hx_mmr) --------------------------------------------------------------
// Per query b: the ranked pool keys[b * stride + i], i < counts[b] (NULL: stride), 0 = an empty slot; ikeys = the same
// slots with internal ids (id_base + row), which name the fp32 row rows[row * dim_pad ..].  A position is eligible when
// its key is not 0, its row is in [0, n_rows) and (eligible != NULL) bit row & 31 of eligible[row >> 5] is set.
// out_keys[b * limit + t] = the key of pick t as it came, out_values[b * limit + t] = its v; the slots past the picks are
// 0 / 0.0f; out_counts[b] = picks.
struct MmrArgs {
  const uint64_t* keys;
  const uint64_t* ikeys;
  int stride;              // 1 .. 2048
  const int* counts;
  const float* rows;       // the normalised fp32 rows, dim_pad floats each (dim_pad a multiple of 64, at most 4096)
  int dim_pad;
  int64_t n_rows;
  uint32_t id_base;
  const uint32_t* eligible;
  int limit;               // 1 .. 256
  float diversity;         // in [0, 1]
  uint64_t* out_keys;
  float* out_values;
  int* out_counts;
};
void launch_mmr_select(const MmrArgs& a, int B, hipStream_t st);
// ---- maxsim.hip: late-interaction rerank (hx_maxsim) ---------------------------------------------
// Per query b: the pool keys[b * stride + i], i < counts[b] (NULL: stride), 0 = an empty slot; ikeys = the same slots with
// internal ids.  A position is eligible when its key is not 0, its row is in [0, n_rows), the row's head is a token count
// >= 1 and (eligible != NULL) the row's bit is set.  A token row: word off[row] of `words` on, head[row] x dim_t bytes, then
// head[row] fp32 scales (hx.h states the layout and the score).  q8 / qscale / q_indptr: the queries' tokens.
// launch_maxsim_score writes pos_keys[b * stride + i] = orderable(score) << 32 | 0xFFFFFFFF - i, 0 for a position that is
// not eligible (every slot); launch_maxsim_finish turns sorted position keys sorted[b * limit + t] (in place) into
// make_key(score, the id of keys[.. + i]), first[b * limit + t] (may be NULL) = the score keys[.. + i] carried.
struct MaxsimArgs {
  const uint64_t* keys;
  const uint64_t* ikeys;
  int stride;              // 1 .. 2048
  const int* counts;
  const uint32_t* head;
  const int64_t* off;
  const uint32_t* words;
  int dim_t;               // a multiple of 64 in [64, 1024]
  int64_t n_rows;
  uint32_t id_base;
  const uint32_t* eligible;
  const int8_t* q8;
  const float* qscale;
  const int64_t* q_indptr;
  uint64_t* pos_keys;
};
void launch_maxsim_score(const MaxsimArgs& a, int B, hipStream_t st);
void launch_maxsim_finish(const uint64_t* keys, int stride, uint64_t* sorted, float* first, int B, int limit, hipStream_t st);
// ---- facet.hip: payload facets (hx_payload_facet / hx_facet_top) ---------------------------------
// counts[c] += the rows r < n whose bit is set in mask (NULL: every row) and whose cell holds code c < n_codes: p0[r] == c
// for a scalar column (off == NULL), some element of e0[off[r], off[r + 1]) == c for a list column -- a row counts once
// per code.  *stray += the kept cells / elements with a code in [n_codes, HX_PAY_U32_NULL).  The caller zeroes both.
struct FacetArgs {
  const uint32_t* p0;
  const int64_t* off;
  const uint32_t* e0;
  const uint32_t* mask;
  int64_t n;
  uint32_t n_codes;
  uint32_t* counts;
  unsigned long long* stray;
};
// grid_cap as launch_payload_mask takes it
void launch_facet_count(const FacetArgs& a, int grid_cap, hipStream_t st);
// The top stage's first pass: list s = the keys count << 32 | (0xFFFFFFFF - rank) (rank[c], or c when rank is NULL) of the
// non-zero counters among codes [s * FACET_SLICE, (s + 1) * FACET_SLICE), 0 = an empty slot, lists[s * list_len ..]:
// list_len <= 512 = the slice's best list_len keys, sorted; list_len = FACET_SLICE = all of them, in code order.
constexpr int FACET_SLICE = 2048;
void launch_facet_keys(const uint32_t* counts, uint32_t n_codes, const uint32_t* rank, uint64_t* lists, int list_len,
                       hipStream_t st);
// ---- reco.hip: recommend search (hx_recommend) ----------------------------------------------------
// The examples of a call lie in one matrix X [E x dim_pad] of normalised fp32 rows, request by request, inside a request
// the positives in the order given, then the negatives in the order given.
constexpr int RECO_LDS_FLOATS = 32768;   // floats of staged examples per launch: 128 KB of LDS
constexpr int RECO_MAX_EXCL = 32;        // stored examples of a request (HX_RECO_MAX_EXAMPLES)
struct RecoReq {
  int ex0, n_pos, n_ex;    // rows [ex0, ex0 + n_ex) of X; the first n_pos are positives
  int excl0, n_excl;       // excl[excl0 ..]: the request's stored-example rows, ascending, unique
  int slot;                // the request's index in the call: its candidate buffer, counter, threshold and flag
  int lds0;                // first staged example of the request inside its scan launch
};
// X[i] = dense row src[i] (src[i] >= 0), or row -1 - src[i] of raw_n [n_raw x dim_pad] (prepared raw vectors)
void launch_reco_examples(const float* dense, const float* raw_n, const int64_t* src, int E, int dim_pad, float* X,
                          hipStream_t st);
// q [R x dim] = the average-vector query of every request: p + (p - n) with p, n the example-order means (p when a
// request has no negative); every operation one fp32 operation, the sums starting from the first example
void launch_reco_average(const float* X, const RecoReq* req, int R, int dim, int dim_pad, float* q, hipStream_t st);
// out[r * limit ..] = the first `limit` keys of in[r * in_stride ..] (in_cnt[r] of them) whose row is not in the
// request's excl list, 0 past them; out_cnt[r] = their number
void launch_reco_drop(const uint64_t* in, int in_stride, const int* in_cnt, const RecoReq* req, const uint32_t* excl,
                      uint32_t id_base, int R, int limit, uint64_t* out, int* out_cnt, hipStream_t st);
// The exhaustive scan of rows [row_begin, row_end) for the n_req requests req[0 .. n_req) (their examples fit
// RECO_LDS_FLOATS together): a row that is not excluded and whose score is >= tau[slot] is appended to
// cand[slot * cap + atomicAdd(cnt[slot])]; ovf[slot] = 1 when the buffer is full.
struct RecoScanArgs {
  const float* dense;      // the normalised fp32 rows, dim_pad floats each (a multiple of 64, at most 4096)
  int dim_pad;
  int64_t row_begin, row_end;
  const float* X;
  const RecoReq* req;      // device
  int n_req;
  const uint32_t* excl;    // device
  const uint32_t* mask;    // packed row mask, NULL = every row
  int strategy;            // HX_RECO_BEST_SCORE | HX_RECO_SUM_SCORES
  const float* tau;
  uint64_t* cand;
  int* cnt;
  int* ovf;
  int cap;
  uint32_t id_base;
};
// lds_examples = examples staged by the launch (sum of its requests' n_ex): sizes the LDS request and the grid
void launch_reco_scan(const RecoScanArgs& a, int lds_examples, hipStream_t st);
// ---- discover.hip: discovery and context search (hx_discover) ------------------------------------
// The examples lie in reco.hip's matrix X; a request's are its target (RecoReq.n_pos = 1) or none (n_pos = 0), then
// pos_0, neg_0, pos_1, neg_1, ...  The exhaustive scan of rows [row_begin, row_end) for the n_req requests
// req[0 .. n_req): a row that is not excluded and whose KEY make_key(score, id_base + row) is > tau_key[slot] is appended
// to cand[slot * cap + atomicAdd(cnt[slot])]; ovf[slot] = 1 when the buffer is full.
struct DiscoverScanArgs {
  const float* dense;      // the normalised fp32 rows, dim_pad floats each (a multiple of 64, at most 4096)
  int dim_pad;
  int64_t row_begin, row_end;
  const float* X;
  const RecoReq* req;      // device
  int n_req;
  const uint32_t* excl;    // device
  const uint32_t* mask;    // packed row mask, NULL = every row
  const uint64_t* tau_key; // per slot: the limit-th best key so far, 0 = none yet (every key passes)
  uint64_t* cand;
  int* cnt;
  int* ovf;
  int cap;
  uint32_t id_base;
};
void launch_discover_scan(const DiscoverScanArgs& a, int lds_examples, hipStream_t st);
// tau_key[r] = cand[r * cap + limit - 1] when cnt[r] >= limit (lists sorted by launch_compact), else 0; R <= 64
void launch_discover_tau(const uint64_t* cand, int cap, const int* cnt, int R, int limit, uint64_t* tau_key, hipStream_t st);
// ---- matrix.hip: distance matrix search (hx_search_matrix) ----------------------------------------
// The sample is S local rows, rows[0 .. S) on the device; nothing but those rows of `dense` is read.
struct MatrixArgs {
  const float* dense;      // the normalised fp32 rows, dim_pad floats each (a multiple of 64, at most 4096)
  const uint32_t* rows;    // device [S]: the sample's local rows, distinct
  int S;                   // 1 .. HX_MATRIX_MAX_SAMPLE
  int dim_pad;
  float* plane;            // [S x S] plane[i * S + j] = sim(rows[i], rows[j]) (the diagonal included)
};
// staged rows of one workgroup of k_matrix_scan at this width: 48 KB of LDS up to width 1024, eight rows above
int matrix_tile_rows(int dim_pad);
// plane = every sim of the sample: spec_dot in wave_spec_dot's order, + 0.0f
void launch_matrix_scan(const MatrixArgs& a, hipStream_t st);
// Row i of the plane -> out_keys[i * limit ..] = the best `limit` of make_key(plane[i * S + j], id_base + rows[j]) over
// j != i with plane[i * S + j] >= threshold, descending, 0 past them; out_counts[i] = their number
void launch_matrix_select(const MatrixArgs& a, float threshold, uint32_t id_base, int limit, uint64_t* out_keys,
                          int* out_counts, hipStream_t st);
// ---- scroll.hip: scroll (hx_scroll_rows / hx_payload_order) --------------------------------------
// "The first m rows of a predicate, in row order" over contiguous row slices, one per workgroup: a count per slice, an
// exclusive prefix over the slices, and an emit that places a row at prefix + its rank inside the slice.
constexpr int FIRST_MAX_SLICES = 1024;     // slices of one call: what the one-workgroup prefix takes
constexpr int ORDER_BINS = 2048;           // counters of one radix pass
constexpr int ORDER_PASSES = 6;            // digits of 11 / 11 / 10 bits over the high word, then over the low word
struct OrderState {
  uint64_t prefix;         // the digits of the threshold T chosen so far (after the last pass: T)
  uint32_t need;           // rows still to take among those that match the prefix (after the last pass: rows with s == T)
  uint32_t all;            // fewer than `limit` rows are eligible: every one is taken
  uint32_t total;          // eligible rows (written by the first pick)
  uint32_t n_less;         // cursor of the rows with s < T (all: of every eligible row) in the candidate arrays
};
struct OrderArgs {
  const uint32_t* lo;      // the column's planes
  const uint32_t* hi;
  const uint32_t* mask;    // packed row mask, NULL = every row
  int64_t n;
  int desc;                // HX_ORDER_DESC
  int has_start, has_after;
  uint64_t s_start, s_after;   // the order keys s of start_from / after_value
  int64_t after_row;
  int limit;
  uint32_t* hist;          // [ORDER_PASSES x ORDER_BINS]
  OrderState* st;
  uint64_t* cand_s;        // [HX_SCROLL_MAX_LIMIT] the chosen rows' keys and rows, unsorted
  uint32_t* cand_row;
  uint32_t* slice_cnt;     // [FIRST_MAX_SLICES] rows with s == T per slice
  uint32_t* slice_pre;     // ... and their exclusive prefix
};
// slices of a call over n rows under the grid cap of launch_payload_mask (0 = none), and the rows of one slice
int first_slices(int64_t n, int grid_cap, int64_t* slice_rows);
// out_rows [limit] = the first `limit` rows r in [start_row, n) whose mask bit is set (mask NULL: every row), 0 past
// them; *out_count = their number.  slice_cnt / slice_pre: FIRST_MAX_SLICES words each.
void launch_scroll_rows(const uint32_t* mask, int64_t n, int64_t start_row, int limit, uint32_t* slice_cnt,
                        uint32_t* slice_pre, uint32_t* out_rows, int32_t* out_count, int grid_cap, hipStream_t st);
// the whole ordered selection (hx.h states it): out_rows / out_bits [limit], *out_count
void launch_payload_order(const OrderArgs& a, uint32_t* out_rows, uint64_t* out_bits, int32_t* out_count, int grid_cap,
                          hipStream_t st);
// ---- formula.hip: score-boosting search (hx_formula) ------------------------------------------------
// Per query b: the pool keys[b * stride + i], i < counts[b] (NULL: stride), 0 = an empty slot; ikeys = the same slots with
// internal ids.  A position is eligible by the rule of MmrArgs.  The program travels in the kernel arguments (3.7 KB of
// the 4 KB a launch takes; uniform reads): op[i] / arg[i] / imm[i] of hx_formula_op, a VAR's arg = its entry of col_lo /
// col_hi (the low and high words of the column's doubles), a COND's arg = its entry of planes (packed row masks).
// out_keys [B x limit] = make_key(value, the id of keys[.. + i]), 0 past the hits; out_pos = i, -1 past them; out_base
// (may be NULL) = the score keys[.. + i] carried, -inf past them; out_counts [B] = hits; out_dropped [B] = eligible
// positions whose value was not finite.
constexpr int FORMULA_MAX_OPS = 256, FORMULA_MAX_COLS = 64, FORMULA_MAX_PLANES = 8;   // HX_FORMULA_* / HX_PAY_MAX_COLUMNS
struct FormulaArgs {
  const uint64_t* keys;
  const uint64_t* ikeys;
  const int* counts;
  const uint32_t* eligible;
  uint64_t* out_keys;
  int* out_pos;
  float* out_base;
  int* out_counts;
  int* out_dropped;
  int64_t n_rows;
  uint32_t id_base;
  int stride;              // 1 .. 2048
  int limit;               // 1 .. 2048
  int n_ops;               // 1 .. 256
  float threshold;
  int has_threshold;
  const uint32_t* planes[FORMULA_MAX_PLANES];
  const uint32_t* col_lo[FORMULA_MAX_COLS];
  const uint32_t* col_hi[FORMULA_MAX_COLS];
  uint64_t imm[FORMULA_MAX_OPS];
  uint8_t op[FORMULA_MAX_OPS];
  uint8_t arg[FORMULA_MAX_OPS];
};
static_assert(sizeof(FormulaArgs) <= 4096, "the program travels in the kernel arguments");
void launch_formula(const FormulaArgs& a, int B, hipStream_t st);
// compact.hip, a list column's elements: dst[off[j] + k] = src[indptr[rows[j]] + k] for the m kept rows (one 4-byte plane)
void launch_csr_compact_u32(const int64_t* indptr, const uint32_t* rows, const int64_t* off, int64_t m, const uint32_t* src,
                            uint32_t* dst, hipStream_t st);

// ---- spstats.hip: collection term statistics and the IDF modifier (hx_sparse_df / hx_sparse_idf_apply; DESIGN.md
// section 31) --------------------------------------------------------------------------------------------------------
// df[i] = postings of term q_idx[i] in ix[0] plus those in ix[1] (a view with n_live = 0 holds none; a negative id: 0),
// one wave per position
void launch_sparse_df(const SparseIndexView* ix, const int32_t* q_idx, int64_t nnz, int64_t* df, hipStream_t st);
// *n_docs = rows r < rows with indptr[r + 1] > indptr[r] (the launch zeroes *n_docs first; indptr may be NULL when rows = 0)
void launch_sparse_rows_nonempty(const int64_t* indptr, int64_t rows, int64_t* n_docs, hipStream_t st);
// out[i] = q_val[i] * idf(*n_docs, df[i]) in the arithmetic hx.h states; out may be q_val
void launch_sparse_idf(const float* q_val, const int64_t* df, const int64_t* n_docs, int64_t nnz, float* out,
                       hipStream_t st);

// ---- binscan.hip: binary quantization, the Hamming scan stage (hx_search_bin) -------------------
// qbits[b * words + (j >> 5)] bit (j & 31) = q[b * dim + j] > 0 for j < dim, 0 up to 32 * words; *bad += the queries with a
// NaN or +-Inf among their dim elements
void launch_bin_queries(const float* q, int dim, int B, int words, uint32_t* qbits, int* bad, hipStream_t st);
// The exhaustive scan of rows [row_begin, row_end) for B queries: score = dim - 2 popcount(qbits XOR row bits); a row whose
// mask bit is set (mask NULL: every row) and whose KEY make_key(score, id_base + row) is > tau_key[b] is appended to
// cand[b * cap + atomicAdd(cnt[b])]; ovf[b] = 1 when the buffer is full.
struct BinScanArgs {
  const uint32_t* bits;    // the stored rows, `words` words each (a multiple of 4)
  int words;
  int dim;
  int64_t row_begin, row_end;
  const uint32_t* qbits;   // [B x words]
  int B;
  const uint32_t* mask;    // packed row mask, NULL = every row
  const uint64_t* tau_key; // per query: the limit-th best key so far, 0 = none yet (every key passes)
  uint64_t* cand;
  int* cnt;
  int* ovf;
  int cap;
  uint32_t id_base;
  int max_grid;            // HX_DEBUG_BIN_GRID (tests): at most this many workgroups, 0 = what the rows and the CUs give
};
void launch_bin_scan(const BinScanArgs& a, hipStream_t st);
// tau_key[b] = cand[b * cap + limit - 1] when cnt[b] >= limit (lists sorted by launch_compact), else 0
void launch_bin_tau(const uint64_t* cand, int cap, const int* cnt, int B, int limit, uint64_t* tau_key, hipStream_t st);
// the schedule both scans over the 1-bit copy share (k_bin_scan; k_asym_scan in binasym.hip)
constexpr int BIN_NT = 256;              // four waves; a tile is 256 rows, one per lane
constexpr int BIN_PASS_SLOTS = 13;       // 16-byte slots of a row staged at a time: 256 x 13 x 16 B = 52 KB of LDS
constexpr int BIN_MAX_SLOTS = 32;        // of a whole row (dim 4096)
inline uint32_t bin_magic(int slots) {   // ceil(2^32 / slots), slots >= 2
  return slots < 2 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)slots - 1) / (uint64_t)slots);
}

// ---- binasym.hip: the asymmetric stage over the 1-bit copy (hx_search_bin_asym) -----------------
// The queries' codes c = rint(q / max|q| * QMAX), QMAX = 2^(P-1) - 1, as P bit planes of their two's complement:
// planes[(b * P + k) * words + (j >> 5)] bit (j & 31) = bit k of c[b][j] for j < dim, 0 up to 32 * words;
// totals[b] = sum_j c[b][j]; *bad += the queries with a NaN or +-Inf among their dim elements.  P = 4 or 8.
void launch_asym_queries(const float* q, int dim, int B, int words, int P, uint32_t* planes, int* totals, int* bad,
                         hipStream_t st);
// launch_bin_scan's scan with score = 2 S - totals[b], S = the sum of c[b][j] over the row's set bits, taken plane by
// plane: a.qbits = the planes of the launch's first query, totals = its total.
void launch_asym_scan(const BinScanArgs& a, const int* totals, int P, hipStream_t st);

}  // namespace hx
