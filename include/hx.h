/*
 * hx.h -- C ABI of the MI355X-native hybrid retrieval engine (libhx.so).
 *
 * This is the drop-in boundary for the Qdrant-backed search path of
 * VivekMalipatel/RAG_Application.  The reference has no FFI of its own: its
 * seam is the Python class QdrantHandler, which forwards every operation to a
 * Qdrant server over HTTP.  Each entry point below cites the reference call it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the
 * ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from hx_last_error() (thread-local).
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device
 *     memory on the index's device.  `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Device entry points enqueue work on
 *     `stream`; they synchronise it only where stated.
 *   - a ranked list is exchanged between stages as an array of 64-bit KEYS,
 *     `keys[b*stride + r]`, r = rank, sorted best-first, with `counts[b]` valid
 *     entries; key = (orderable(score) << 32) | (0xFFFFFFFF - id), so that the
 *     descending integer order IS the engine's total order (score descending,
 *     id ascending).  0 marks an empty slot.  ids are global row ids, < 2^32 - 1:
 *     id_base + local row, or -- a shard that holds slices of many batches -- the
 *     insertion-order ids named batch by batch with hx_set_next_id.
 *   - no torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef HX_H
#define HX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HX_ABI_VERSION 3   /* 2: hx_set_next_id, hx_add_rows_dev, hx_truncate; max_terms dropped from two entries
                            * 3: the candidates-first sharded H1 (hx_h1_plan / _nominate_async / _rescore_async /
                            *    _finish), hx_sparse_wmax / hx_set_sparse_wmax */

typedef struct hx_index hx_index;

/* The 8-key search_params contract
 * (app/services/agents/hybrid_search_workflow.py:8-19,
 *  app/api/v1/endpoints/mcp/qdrant_search_mcp_endpoint.py:19-28) plus the
 * switches for semantics inherited from Qdrant (oracle/oracle.py names them). */
/* The hybrid entries refuse (before any device work) rrf_k that is non-finite, <= 0 or so small that 2 / rrf_k
 * overflows, and rrf_rank_base outside [0, 2^30]: a document's fused score, the sum of its two contributions
 * 1 / (f32(rank + rrf_rank_base) + rrf_k), then stays finite and positive.  hx_rrf, hx_h1_fuse and
 * hx_h1_finish take the two settings directly and apply the same rule. */
typedef struct hx_params {
  int32_t matryoshka_64_limit;   /* limit of the innermost prefix stage (first matryoshka size)   */
  int32_t matryoshka_128_limit;  /* second prefix stage                                           */
  int32_t matryoshka_256_limit;  /* third prefix stage                                            */
  int32_t dense_limit;
  int32_t quantized_limit;
  int32_t sparse_limit;
  int32_t final_limit;
  int32_t hnsw_ef;               /* accepted, unused: every stage is exact (qdrant_handler.py:369) */
  float   rrf_k;                 /* 2.0  : Qdrant RRF constant; finite, > 0, with 2 / rrf_k finite    */
  int32_t rrf_rank_base;         /* 0    : 0-based ranks; in [0, 2^30]                              */
  int32_t rrf_limit;             /* 10   : default limit of a Prefetch without `limit`              */
  int32_t mode;                  /* HX_MODE_TREE or HX_MODE_H1                                      */
} hx_params;

#define HX_MODE_TREE 0  /* the reference query tree, qdrant_handler.py:305-372                  */
#define HX_MODE_H1   1  /* dense top-dense_limit (+) sparse top-sparse_limit -> RRF -> final_limit */

/* ---- lifecycle ---------------------------------------------------------- */

/* create_collection (qdrant_handler.py:24-117): one index = one user collection
 * holding the named vectors dense / quantized / matryoshka_* and the sparse
 * vector.  `msizes` = matryoshka prefix sizes (ascending, <= 3 of them, each a
 * multiple of 64 and <= dim); n_msizes may be 0.  `id_base` = global id of local
 * row 0 (row sharding).  `device` = HIP device ordinal. */
int hx_create(int32_t dim, const int32_t* msizes, int32_t n_msizes, int32_t device,
              int64_t id_base, hx_index** out);
/* delete_collection (qdrant_handler.py:430-439) */
int hx_destroy(hx_index* h);
const char* hx_last_error(void);
int hx_abi_version(void);

/* ---- ingest: store_document_vectors / store_chat_vectors ------------------
 * (qdrant_handler.py:120-198, 200-267 -> AsyncQdrantClient.upsert :190-193) */

/* optional: pre-size device storage for `n_rows` rows and `nnz` sparse entries */
int hx_reserve(hx_index* h, int64_t n_rows, int64_t nnz);
/* append n raw dense rows [n x dim] (host fp32).  Derives on device, per row:
 * the L2-normalised "dense" vector, the normalised prefixes, the int8
 * "quantized" copy trunc(127*x) (qdrant_handler.py:144-150) and its norm.
 * Every element must be finite: a batch with a NaN or +-Inf element anywhere is refused whole ("finite" in the
 * message), the index stays as it was (count, stored rows, the int8 copy's error bound); the call may consume its ids.
 * A finite row whose squared length overflows to +Inf is valid: it is stored as a zero row.  The same holds for
 * hx_add_dense_dev, hx_add_rows and hx_add_rows_dev (checked on the device while the rows are derived). */
int hx_add_dense(hx_index* h, const float* rows_host, int64_t n);
/* the same for rows already on the device -- the output of an encoder on PyTorch-ROCm
 * (embedding_handler.py:64-99 produces them; qdrant_handler.py:120-198 stores them): read in place,
 * no staging copy.  Returns when the rows are stored. */
int hx_add_dense_dev(hx_index* h, const float* rows_dev, int64_t n, void* stream);
/* append the sparse vectors of the same n rows as doc-major CSR (host):
 * indptr[n+1], idx[nnz] (term ids in [0, 2^31)), val[nnz].  Indices must be
 * unique within a row (Qdrant rejects duplicates).  Rows must be added in the
 * same order as hx_add_dense; a row may be empty.  Values must be finite with
 * |v| <= 1e18 (anything else is refused, nothing is stored).  Sparse vectors are the
 * vectors of the NEXT rows: call it BEFORE hx_add_dense of the same rows (rows that got
 * no sparse vector earlier are padded as empty documents first; a second call before the
 * dense rows of the first arrived is refused). */
int hx_add_sparse(hx_index* h, const int64_t* indptr_host, const int32_t* idx_host,
                  const float* val_host, int64_t n);
/* one chunk batch, dense and sparse together, all or nothing (store_document_vectors builds
 * one PointStruct per chunk carrying both, qdrant_handler.py:152-188): indptr_host NULL = no
 * sparse vectors.  A failure leaves the index exactly as it was. */
int hx_add_rows(hx_index* h, const float* rows_host, const int64_t* indptr_host, const int32_t* idx_host,
                const float* val_host, int64_t n);
/* hx_add_rows for dense rows that already lie on the device (the output of an encoder on PyTorch-ROCm): the same
 * all-or-nothing contract, the sparse CSR still comes from the host (bm25 runs on the host cores). */
int hx_add_rows_dev(hx_index* h, const float* rows_dev, const int64_t* indptr_host, const int32_t* idx_host,
                    const float* val_host, int64_t n, void* stream);
/* Row sharding with insertion-order ids (the reference upserts a collection in MANY batches,
 * app/services/file_processor/text_processor.py:357 -> qdrant_handler.py:190-193; a shard then holds a slice of
 * every batch): the NEXT add call's rows get the global ids first_id, first_id + 1, ...  Ids must ascend with the
 * rows of a shard (first_id >= every id given so far).  Without this call a batch continues the ids of the previous
 * one, starting at hx_create's id_base.  Every key that leaves the index carries global ids, and hx_rescore takes
 * global ids; a failed add consumes the call. */
int hx_set_next_id(hx_index* h, int64_t first_id);
/* Roll the collection back to its first n_rows rows (dense and sparse): how the shards that stored their slice of
 * a batch undo it when another shard could not (one upsert = one request in the reference, :190-193). */
int hx_truncate(hx_index* h, int64_t n_rows);
/* Per-point delete (the reference deletes a file's chunks when its user deletes or re-uploads the file,
 * IndexerAPI/src/api/v1/endpoints/delete.py): keep only the rows of a mask (same layout as hx_hybrid_query_*_masked: bit
 * r = local row r, set = kept; mask_rows must equal hx_count).  *n_removed = rows dropped (n_removed may be NULL).
 * After the call the index is the index one gets by creating a new one and adding the kept rows in their order: row i
 * is the i-th kept row, its id id_base + i; hx_count / hx_nnz are those of the kept rows; every search entry returns
 * (ids and fp32 score bits) what that index returns; later hx_add_* calls continue as on it; hx_save / hx_load round-trip
 * it.  Equivalently: an unmasked call afterwards returns what the masked call with the same mask returned before, ids
 * mapped to their rank among the kept rows.  Every stored copy and the sparse CSR are compacted on the device, in
 * place; the inverted index is dropped and rebuilt by the next search or hx_finalize; the sparse
 * weight range (hx_sparse_wmax) is that of the surviving weights.  Capacities stay as they are.  One figure may differ
 * from the fresh index's: cand8_row_error_max (hx_stats) keeps covering the removed rows -- an upper bound is all the
 * certificate needs, as after hx_truncate.
 * Every row kept: returns 0 with *n_removed = 0, nothing is touched or invalidated, no device work.  No row kept: an
 * empty index that accepts adds.  Refused before anything moves (the index stays as it was): a NULL index, a NULL mask
 * with mask_rows > 0, mask_rows != hx_count, sparse vectors pending for rows not added yet, and an index whose ids
 * were named with hx_set_next_id (a shard of a sharded collection: renumbering is a collective matter).  Synchronises
 * the device (as hx_truncate) and returns when the compaction is done. */
int hx_retain_rows(hx_index* h, const uint32_t* keep_host, int64_t mask_rows, int64_t* n_removed);
/* Upsert by an existing id (client.upsert overwrites the point that already has the id, qdrant_handler.py:190-193):
 * replace stored rows in place.  rows_host[m] = local rows in [0, hx_count), any order, unique; dense_host = [m, dim]
 * raw fp32 in that order; indptr_host / idx_host / val_host = the CSR of the m new sparse vectors in that order.
 * indptr_host NULL = the sparse vectors of those rows stay as they are (the dense-only form: the document-major CSR,
 * the inverted index and the weight range are not touched).
 * After the call the index is the index one gets by creating a new one and adding the final rows in their order:
 * hx_count is unchanged, hx_nnz is the final rows'; every search entry returns (ids and fp32 score bits) what that
 * index returns; hx_debug_row gives its bytes for the replaced rows and the old bytes for every other row; later
 * hx_add_*, hx_retain_rows, hx_truncate, hx_save / hx_load behave as on it.  Every stored copy of a replaced row is
 * derived in a staging block and scattered into place, the CSR is spliced from the first replaced document on
 * (DESIGN.md section 18); the inverted index is dropped and rebuilt by the next search or hx_finalize (not by the
 * dense-only form); the weight range (hx_sparse_wmax) is the final rows'.  Ids, capacities and the hx_stats counters
 * stay; cand8_row_error_max keeps covering the replaced rows and the rows of a refused batch (an upper bound).
 * m == 0: returns 0, nothing is touched.  Refused before any stored byte changes: a NULL index, m < 0, NULL rows_host /
 * dense_host with m > 0, a row outside [0, hx_count), a duplicate row, a NaN / Inf dense element, a sparse batch
 * hx_add_sparse would refuse, sparse vectors pending for rows not added yet, an index whose ids were named with
 * hx_set_next_id.  Synchronises the device at its start and before it returns; its staging buffers (one derived copy
 * of m rows, 8 bytes per posting from the first replaced document on) are freed before it returns. */
int hx_replace_rows(hx_index* h, const int64_t* rows_host, int64_t m, const float* dense_host,
                    const int64_t* indptr_host, const int32_t* idx_host, const float* val_host);
/* build the on-device inverted index over everything added so far; searches
 * call it implicitly when the index is stale. */
int hx_finalize(hx_index* h);
/* get_collection_chunk_count (qdrant_handler.py:441-481) */
int hx_count(hx_index* h, int64_t* n_rows);
int hx_nnz(hx_index* h, int64_t* nnz);

/* fill rows [row0, row0+n) with the synthetic corpus of SURVEY.md 8(d),
 * generated on the device (oracle/oracle.py synth_dense / synth_sparse_docs give
 * the same values).  Global row r = id_base + local row.  cdf_u32[V] and
 * len_u16[256] are the shared lookup tables (host).  with_sparse=0 skips the
 * sparse side. */
int hx_synth_fill(hx_index* h, int64_t n, uint32_t seed_dense, uint32_t seed_sparse,
                  const uint32_t* cdf_u32_host, int32_t V, const uint16_t* len_u16_host,
                  int32_t with_sparse);
/* synthetic query batch on the device: q_dev [B x dim] fp32 rows q0..q0+B-1 */
int hx_synth_queries_dense(int32_t dim, int64_t q0, int32_t B, uint32_t seed,
                           float* q_dev, void* stream);

/* ---- whole-collection stages (device in, device out) ---------------------- */

/* Prefetch(query=dense_vector[:prefix], using="matryoshka_<prefix>"|"dense", limit)
 * (qdrant_handler.py:311-315, 327-329, 366-368).  q_dev: B raw (un-normalised)
 * query rows [B x dim] fp32.  Every element of every query must be finite (all dim of them, whatever the prefix): the
 * call fails for a batch holding a NaN or +-Inf ("finite" in the message), reported at the stage's one host round trip.
 * The same holds for hx_search_i8, hx_h1_local and the hybrid entries; the _async entries and hx_h1_local_async count
 * such a batch's queries as not final (the caller's redo through the synchronous entry then fails), and
 * hx_h1_nominate_async sends the batch flagged.  prefix = 0 searches the full vector.  Output: keys
 * [B x limit] + counts[B].  Synchronises `stream` (exactness certificate). */
int hx_search_dense(hx_index* h, const float* q_dev, int32_t B, int32_t prefix, int32_t limit,
                    uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* Prefetch(query=quantized_query, using="quantized", limit) (qdrant_handler.py:299-302,335-339) */
int hx_search_i8(hx_index* h, const float* q_dev, int32_t B, int32_t limit,
                 uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* Prefetch(query=SparseVector, using="sparse", limit) (qdrant_handler.py:347-354).
 * Query batch as CSR on the device: indptr[B+1] (int64), idx (int32, strictly ascending
 * within a query: the exact score is a running fp32 sum in that order; the device checks it
 * and the call fails for a query that is not), val (fp32, finite). */
int hx_search_sparse(hx_index* h, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                     const float* q_val_dev, int32_t B, int32_t limit,
                     uint64_t* keys_dev, int32_t* counts_dev, void* stream);

/* The three stages above WITHOUT their host round trip (the reference has no multi-device path; these serve the
 * row-sharded form of its query tree, qdrant_handler.py:305-372, where every rank enqueues a level, the ranks exchange
 * the level's lists, and nobody should wait for a flag in between): everything is enqueued on `stream` and the call
 * returns; the number of queries whose lists are NOT final (a stage flagged them for a retry or the exact path) is
 * ADDED to *flag_dev (device).  The caller zeroes the word before the first stage of a batch, reads it when it suits
 * it -- once, behind the whole tree -- and runs the batch again through the synchronous entries when it is not zero. */
int hx_search_dense_async(hx_index* h, const float* q_dev, int32_t B, int32_t prefix, int32_t limit,
                          uint64_t* keys_dev, int32_t* counts_dev, int32_t* flag_dev, void* stream);
int hx_search_i8_async(hx_index* h, const float* q_dev, int32_t B, int32_t limit,
                       uint64_t* keys_dev, int32_t* counts_dev, int32_t* flag_dev, void* stream);
int hx_search_sparse_async(hx_index* h, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                           const float* q_val_dev, int32_t B, int32_t limit,
                           uint64_t* keys_dev, int32_t* counts_dev, int32_t* flag_dev, void* stream);

/* ---- candidate stages ------------------------------------------------------ */

/* outer level of a nested Prefetch / the root query (qdrant_handler.py:307-330,
 * 333-344, 363-372): re-score the candidate ids in cand_keys (scores ignored, ids
 * outside this shard skipped, duplicates merged) with one named vector and keep
 * `limit`. */
int hx_rescore(hx_index* h, const float* q_dev, int32_t B, int32_t prefix,
               const uint64_t* cand_keys_dev, int32_t cand_stride, const int32_t* cand_counts_dev,
               int32_t limit, uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* FusionQuery(Fusion.RRF) over two ranked lists (qdrant_handler.py:357-360) */
int hx_rrf(int32_t device, const uint64_t* a_keys_dev, int32_t a_stride, const int32_t* a_counts_dev,
           const uint64_t* b_keys_dev, int32_t b_stride, const int32_t* b_counts_dev,
           int32_t B, float rrf_k, int32_t rank_base, int32_t limit,
           uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* union / cross-shard merge: per query, top `limit` of the `stride` slots of
 * in_keys (0 = empty), duplicates optionally dropped.  in_counts may be NULL
 * (then every slot is examined). */
int hx_merge(int32_t device, const uint64_t* in_keys_dev, int32_t stride, const int32_t* in_counts_dev,
             int32_t B, int32_t limit, int32_t dedupe,
             uint64_t* keys_dev, int32_t* counts_dev, void* stream);

/* ---- general fusion: FusionQuery(Fusion.RRF | Fusion.DBSF) over N ranked lists ----------------
 * The fusion node of a caller-defined Prefetch tree (client.query_points(prefetch=[...], query=FusionQuery(...))):
 * n_lists ranked lists per query -> one.  hx_rrf is the two-list, unweighted special case and keeps its own kernels.
 * Additive to the ABI: HX_ABI_VERSION stays 3.  No index is involved (device ordinal, as hx_rrf).
 *
 * keys_dev and counts_dev are HOST arrays of n_lists DEVICE pointers: list l of query b is keys_dev[l][b * strides[l] +
 * r], r < n_l = min(max(counts_dev[l][b], 0), strides[l]), best first; every slot below n_l is an entry (id and fp32
 * score as the key carries them).  weights_host: n_lists weights w_l, or NULL = all 1.0f.  The output must not overlap
 * an input.  out_keys_dev [B x limit] holds min(limit, distinct ids) keys (fused score, id) in key order -- fused score
 * descending, id ascending -- and 0 after them; out_counts_dev [B] that number.
 *
 * Refused before any device work: n_lists outside [1, HX_FUSE_MAX_LISTS]; a stride outside [1, 2048] or strides that
 * sum above HX_FUSE_MAX_SLOTS; limit outside [1, 2048]; a weight that is not finite or is negative; an unknown method;
 * for HX_FUSE_RRF the rrf_k / rank_base hx_rrf refuses (HX_FUSE_DBSF ignores both).
 *
 * Arithmetic (exact: rag_application_amd/fusion.py restates it in numpy, bit for bit).  s_r = the fp32 score in the key
 * at rank r of list l; c_l(r) = the contribution of that entry:
 *   HX_FUSE_RRF   c_l(r) = w_l * (1 / (f32(r + rank_base) + rrf_k)): the conversion, the addition, the reciprocal (the
 *                 correctly rounded fp32 quotient 1 / x) and the product are one fp32 round-to-nearest operation each.
 *   HX_FUSE_DBSF  each list is normalised to its mean +- 3 standard deviations (Qdrant's documented rule; its own
 *                 arithmetic is not pinned here).  Statistics in fp64, every step one IEEE double operation (no FMA,
 *                 correctly rounded divide and square root).  T(v) = the sum over a fixed tree: v padded with +0.0 to the
 *                 next power of two P >= n_l, then v[i] += v[i + h] for h = P/2, P/4, ..., 1; T(v) = v[0].
 *                   mean = T(s) / n_l;  var = T((s_r - mean) * (s_r - mean)) / (n_l - 1);  sd = sqrt(var);
 *                 n_l == 1, or sd not > 0 (a NaN included): norm_r = 0.5f for the whole list; otherwise
 *                   norm_r = f32((s_r - (mean - 3 * sd)) / (6 * sd));
 *                 c_l(r) = w_l * norm_r in fp32.
 *   both          fused(id) = 0.0f + c_l1 + c_l2 + ... over the lists that hold the id, added in ascending list order in
 *                 fp32 round-to-nearest (the order of hx_rrf).  A list's FIRST entry of an id counts; a later entry of
 *                 the same id in the same list is ignored -- it still occupies its rank and, for DBSF, still counts in
 *                 the list's statistics. */
#define HX_FUSE_RRF   0
#define HX_FUSE_DBSF  1
#define HX_FUSE_MAX_LISTS 8
#define HX_FUSE_MAX_SLOTS 4096      /* sum of the strides */
int hx_fuse(int32_t device, int32_t method, int32_t n_lists,
            const uint64_t* const* keys_dev, const int32_t* strides_host, const int32_t* const* counts_dev,
            const float* weights_host, int32_t B, float rrf_k, int32_t rank_base, int32_t limit,
            uint64_t* out_keys_dev, int32_t* out_counts_dev, void* stream);
/* Row-sharded H1 query, one process per GPU (the reference has no
 * multi-device path -- these two calls bracket the one all-gather of the step):
 *  hx_h1_local  the shard's dense top-`dense_limit` and sparse top-`sparse_limit` of every
 *               query, side by side in keys_dev [B x (dense_limit + sparse_limit)]
 *               (qdrant_handler.py:347-354 and the dense Prefetch of the H1 configuration;
 *               0 = empty slot, ids are global: id_base + row);
 *  hx_h1_fuse   gathered_dev [world x B x (dense_limit + sparse_limit)] (rank-major, as
 *               all_gather_into_tensor leaves it): per query the global dense and sparse
 *               lists (top of the union of the shards' lists), then RRF as hx_rrf;
 *  hx_h1_local_async  hx_h1_local without its host round trip: everything is enqueued and the
 *               call returns; keys_dev is [(B + 1) x (dense_limit + sparse_limit)], row B holds
 *               in element 0 the number of queries whose lists are NOT final (a stage flagged
 *               them for a retry or the exact path) and zeros after it.  The caller reads that
 *               word when it suits it (it travels through the exchange with the lists, so every
 *               rank sees every rank's word) and redoes the batch through hx_h1_local when any
 *               rank's word is not zero.  Keeps consecutive batches back to back on the device. */
int hx_h1_local(hx_index* h, const float* q_dev, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                const float* q_val_dev, int32_t B, int32_t dense_limit, int32_t sparse_limit,
                uint64_t* keys_dev, void* stream);
int hx_h1_local_async(hx_index* h, const float* q_dev, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                      const float* q_val_dev, int32_t B, int32_t dense_limit, int32_t sparse_limit,
                      uint64_t* keys_dev, void* stream);
int hx_h1_fuse(int32_t device, const uint64_t* gathered_dev, int32_t world, int32_t B,
               int32_t dense_limit, int32_t sparse_limit, int32_t limit, float rrf_k, int32_t rank_base,
               uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* Row-sharded H1 with the exchange BEFORE the exact scores ("candidates first").  What a shard
 * repeats per QUERY whatever its row count -- the exact re-score of L' dense candidates, the exact re-score of the sparse
 * margin set, the compaction of full-size buffers -- is divided by the number of shards: a shard only nominates.
 * Three calls around two collectives per batch, everything enqueued (no host round trip):
 *  hx_h1_plan            list sizes for `world` shards: k1 = dense nominations per shard and query (its binomial share of
 *                        the global L' + 10 sigma), k2 = integer BM25 scores it sends, lp = L' (the global dense
 *                        candidate count the certificate needs for dense_limit), k3 = exact sparse keys it returns,
 *                        lout = the stride of its private integer-score list;
 *  hx_h1_nominate_async  nom_dev [B*k1 dense keys | B*k2 sparse keys | B*2 meta words | B*lout + B private words]: the
 *                        shard's best k1 rows by the int8 candidate score (hx_search_dense's candidate pass, no exact
 *                        score) and its k2 best integer BM25 scores of the select pass (sparse2.hip); the private tail
 *                        (its whole integer-score list) stays on this rank for hx_h1_rescore_async;
 *                        -> all-gather of the first B*(k1+k2+2) words over the shards;
 *  hx_h1_rescore_async   gathered_dev [world x B*(k1+k2+2)] + this rank's own nom_dev: the global cuts (top-lp by int8
 *                        score; the global L-th integer score, hence the margin-set threshold), the check that no
 *                        shard's list was cut above them, and the EXACT scores (spec_dot; upstream-order fp32 sparse sum)
 *                        of THIS shard's rows: res_dev [B*lp dense keys at their positions in the global list |
 *                        B*world*k3 sparse keys, this rank's best k3 in slot `rank` | B*world candidate counts | B*4
 *                        meta], 0 elsewhere;
 *                        -> all-reduce (SUM, as int64) of res_dev: every key slot has one owner, the others hold 0; the
 *                        four meta words per query are the same on every rank and come back multiplied by `world`;
 *  hx_h1_finish          reduced_dev: exact dense top-dense_limit with the certificate m + eps < e_L evaluated once on the
 *                        global list, exact sparse top-sparse_limit, RRF as hx_rrf.  *nfail_dev += queries whose lists
 *                        are not final (a shard's list was cut too short, a buffer overflowed, the certificate does not
 *                        hold): the caller then redoes the batch through hx_h1_local, as after hx_h1_local_async.
 * The integer BM25 scores of different shards are comparable only under one scale: hx_set_sparse_wmax gives every shard
 * the largest document weight of ANY shard (hx_sparse_wmax reads the shard's own; also whether it holds a non-positive
 * weight).  Needs the int8 candidate copy (the default, hx_dense_candidates): a shard whose int8 pass is off does not
 * fail in hx_h1_nominate_async (its peers are already on their way into the all-gather); it sends an empty dense list
 * flagged as overflowed, so every rank sees a flagged batch and redoes it per shard.
 * hx_h1_plan fails (and the caller uses the per-shard exchange, hx_h1_local_async + hx_h1_fuse) when
 *  - dense_limit, rounded up to a multiple of 32, exceeds 8192 / world (also rounded down to 32): a shard's dense list
 *    must hold dense_limit rows, and world x k1 keys are merged in one 8192-key buffer;
 *  - a shard's share of sparse_limit (mean + 10 sigma, to 32) exceeds 256, the most exact sparse keys per query and
 *    shard hx_h1_rescore_async takes (sparse_limit from 257 at world 1, 331 at world 2, 1151 at world 8);
 *  - the arguments are out of range (limits in [1, 2048], world in [1, 64]).
 * Every plan it returns meets the checks of hx_h1_nominate_async, hx_h1_rescore_async and hx_h1_finish: dense_limit <=
 * k1, k1 a share of lp and k2 = k3 a share of sparse_limit (all multiples of 32), world x k <= 8192, k3 <= 256. */
int hx_h1_plan(int32_t dense_limit, int32_t sparse_limit, int32_t world, int32_t* k1, int32_t* k2, int32_t* lp,
               int32_t* k3, int32_t* lout);
/* Which kernels serve the tail of hx_search_dense's full-vector stage for a batch of B queries and limit L (host
 * arithmetic only: no index, no device; the dense stage and its launchers decide by the same functions, so the report
 * cannot differ from what runs).  cand_kind: 1 = int8 candidates, 0 = fp16 candidates (also the first prefix stage, an
 * index without the int8 copy or with it switched off); retry_level: 0 = the first pass, 1 = the re-run of a query the
 * first pass could not certify (always fp16 candidates: cand_kind is ignored there).
 *  lp, cap               L' = candidates kept per query, C = keys of a query's candidate buffer (L <= L', 2 L' <= C);
 *  finish_e              0: exact re-score, top-L and certificate are three launches (k_rescore_list, k_compact_top,
 *                        k_certify); 2 | 4 | 8: one launch, k_dense_finish with that many keys per lane -- B <= 64 and
 *                        L' <= 512; the smallest of 2, 4, 8 with L <= 64 x finish_e;
 *  compact_nw, compact_e the compaction behind every launch of the candidate scan (keep = L' of C keys):
 *                        k_compact_top<compact_nw, compact_e>, or 0, 0 = the sort in LDS (k_compact).
 * It reports the default routing: HX_DEBUG_NO_FINISH_FUSE and HX_DEBUG_FINISH_NB (tests; read by hx_create, per index)
 * force the three launches / a block count for one index and do not change this answer.
 * Fails when B < 1, L is outside [1, 2048], or cand_kind / retry_level is neither 0 nor 1. */
int hx_dense_route(int32_t B, int32_t L, int32_t cand_kind /* 1 int8, 0 fp16 */, int32_t retry_level /* 0 | 1 */,
                   int32_t* lp, int32_t* cap, int32_t* finish_e /* 0 = three launches, else 2 | 4 | 8 */,
                   int32_t* compact_nw, int32_t* compact_e /* 0, 0 = the LDS sort */);
/* Which kernel the whole-collection candidate scan launches for a batch of B queries over rows of row_bytes bytes
 * (kind: 0 fp16, 1 int8), by the default routing; no index and no device are involved.
 *  form  0: k_scan (batches of at most 32 queries, or more than 4096);
 *        1: k_scan8, the staggered 256 x 256 tile;
 *        2: k_scan8 in its 256-row x 128-query form (33..128 queries);
 *        3: k_scan8q, the query-stationary form: int8 rows of 768 bytes and ceil(B / 256) in {1, 2, 4, 8, 16}.
 * HX_DEBUG_NO_QS (read by hx_create, per index) sends form 3 to form 1 for one index and does not change this answer;
 * the first chunk of every scan (the candidate buffer's capacity, a few thousand rows) goes through k_scan whatever B. */
int hx_scan8_form(int32_t B, int64_t row_bytes, int32_t kind, int32_t* form);
/* Waves that share the log appends of one scan launch over `tiles` 256-row tiles and nq_tiles query tiles (qs: the
 * query-stationary form): what the per-wave log capacity is planned by.  Host arithmetic only. */
int hx_scan8_log_waves(int64_t tiles, int32_t nq_tiles, int32_t qs, double* waves);
/* Diagnostic: the walk of workgroup `block` (0 .. 255) of one k_scan8q launch over the logical rows [row_begin, row_end)
 * with nq_tiles query tiles (1, 2, 4, 8 or 16) and the tile permutation (perm_mul, perm_n; perm_n = 0: identity) -- the
 * kernel's own cursor, run on the host; no index and no device are involved.
 *  n_items      64-row items the workgroup scans (0: its stream has no rows);
 *  tiles, rows  [cap] the physical 256-row tile and the first physical row of items 0 .. min(n_items, cap) - 1
 *               (may be NULL when cap is 0). */
int hx_scan8q_items(int64_t row_begin, int64_t row_end, int32_t nq_tiles, uint32_t perm_mul, uint32_t perm_n, int32_t block,
                    int32_t cap, uint32_t* tiles, int64_t* rows, int32_t* n_items);
int hx_sparse_wmax(hx_index* h, float* wmax, int32_t* nonpos);
int hx_set_sparse_wmax(hx_index* h, float wmax);
int hx_h1_nominate_async(hx_index* h, const float* q_dev, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                         const float* q_val_dev, int32_t B, int32_t dense_limit, int32_t sparse_limit, int32_t k1,
                         int32_t k2, uint64_t* nom_dev, void* stream);
int hx_h1_rescore_async(hx_index* h, const float* q_dev, const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                        const float* q_val_dev, int32_t B, const uint64_t* nom_dev, const uint64_t* gathered_dev,
                        int32_t world, int32_t rank, int32_t dense_limit, int32_t sparse_limit, int32_t k1, int32_t k2,
                        int32_t lp, int32_t k3, uint64_t* res_dev, void* stream);
int hx_h1_finish(int32_t device, const uint64_t* reduced_dev, int32_t world, int32_t B, int32_t lp, int32_t k3,
                 int32_t dense_limit, int32_t sparse_limit, int32_t limit, float rrf_k, int32_t rank_base,
                 uint64_t* keys_dev, int32_t* counts_dev, int32_t* nfail_dev, void* stream);
/* keys -> (fp32 score, int64 id); empty slots give (-inf, -1) */
int hx_unpack(int32_t device, const uint64_t* keys_dev, int64_t n, float* scores_dev,
              int64_t* ids_dev, void* stream);

/* ---- whole query, one shard (host in, host out) ----------------------------
 * QdrantHandler.hybrid_search -> query_points (qdrant_handler.py:296-372).
 * q_dense_host [B x dim] raw queries; sparse queries as CSR (indices need not be
 * sorted).  Outputs: scores/ids [B x final_limit], counts[B]. */
int hx_hybrid_query_host(hx_index* h, const float* q_dense_host,
                         const int64_t* q_indptr_host, const int32_t* q_idx_host,
                         const float* q_val_host, int32_t B, const hx_params* p,
                         float* scores_host, int64_t* ids_host, int32_t* counts_host);
/* same, device-resident inputs and outputs (bench path; sparse idx strictly ascending per query, checked) */
int hx_hybrid_query_dev(hx_index* h, const float* q_dense_dev,
                        const int64_t* q_indptr_dev, const int32_t* q_idx_dev,
                        const float* q_val_dev, int32_t B, const hx_params* p,
                        uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* Pre-filtered query (a payload filter evaluated by the caller, applied to EVERY stage -- the prefetches as well as
 * the root): the two calls above restricted to the rows of a mask.  The lists are exactly those of the unmasked call
 * on an index holding only the kept rows, added in the same order (same ids after the map back, same order, same
 * fp32 score bits), in both modes.  mask = ceil(mask_rows / 32) uint32 words, bit r & 31 of word r >> 5 (LSB first)
 * = local row r in insertion order; bits at or past mask_rows are ignored; mask_rows must equal hx_count (an error
 * otherwise).  Every row kept: the unmasked call, the same keys.  No row kept: counts 0, empty slots.  Otherwise the
 * whole-collection dense scans read copies of the kept rows, gathered on the caller's stream (only the copy a scan
 * reads), and the sparse stage tests the mask inside its kernels over this index's inverted index (DESIGN.md section
 * 13).  Synchronisation beyond the unmasked call: the device entry reads the number of kept rows back once (one
 * synchronisation of `stream`; the host entry counts the host mask instead); a call that keeps more rows than any
 * masked call before it synchronises `stream` once more and reallocates the copies' buffers (to the next power of two
 * of the kept rows -- they stay allocated with the index until hx_release_mask_view or hx_destroy); a query no scan
 * can serve (the exact fallback path) gathers its matrix once more.  The mask must stay valid until the call's work on
 * `stream` is done.  Pre-filtered queries do not count toward the int8 guard window (hx_stats). */
int hx_hybrid_query_host_masked(hx_index* h, const float* q_dense_host, const int64_t* q_indptr_host,
                                const int32_t* q_idx_host, const float* q_val_host, int32_t B, const hx_params* p,
                                const uint32_t* mask_host, int64_t mask_rows,
                                float* scores_host, int64_t* ids_host, int32_t* counts_host);
int hx_hybrid_query_dev_masked(hx_index* h, const float* q_dense_dev, const int64_t* q_indptr_dev,
                               const int32_t* q_idx_dev, const float* q_val_dev, int32_t B, const hx_params* p,
                               const uint32_t* mask_dev, int64_t mask_rows,
                               uint64_t* keys_dev, int32_t* counts_dev, void* stream);
/* free the copies of kept rows the pre-filtered queries keep allocated between calls (synchronises the device) */
int hx_release_mask_view(hx_index* h);
/* ONE whole-collection stage restricted to the rows of a mask (a `filter` inside a Prefetch):
 * hx_search_dense / hx_search_i8 / hx_search_sparse with the contract above stated for one stage.  The list is exactly
 * what the unmasked entry returns on an index holding only the kept rows, added in the same order: ids mapped back
 * through the ascending list of kept rows, same order, same fp32 score bits.  Mask layout, mask_rows == hx_count, "every
 * row kept = the unmasked call, same keys", "no row kept = counts 0, empty slots", the synchronisation (one read-back of
 * the kept-row count per call, on top of the stage's own round trip) and the lifetime of the view's buffers are those of
 * hx_hybrid_query_dev_masked.  mask_dev == NULL is the unmasked entry (mask_rows is not read).  A prefix other than the
 * first has no scanned fp16 copy: its masked stage gathers the kept rows of the prefix's fp32 copy and scores them
 * exactly, as the unmasked one scores all of them.  The sparse query weights are used as given: a caller applying an IDF
 * modifier scales them by the WHOLE collection's statistics first (hx_sparse_df), as Qdrant does under a filter.
 * There are no masked _async forms.  Additive to the ABI: HX_ABI_VERSION stays 3. */
int hx_search_dense_masked(hx_index* h, const float* q_dev, int32_t B, int32_t prefix, int32_t limit,
                           const uint32_t* mask_dev, int64_t mask_rows, uint64_t* keys_dev, int32_t* counts_dev,
                           void* stream);
int hx_search_i8_masked(hx_index* h, const float* q_dev, int32_t B, int32_t limit, const uint32_t* mask_dev,
                        int64_t mask_rows, uint64_t* keys_dev, int32_t* counts_dev, void* stream);
int hx_search_sparse_masked(hx_index* h, const int64_t* q_indptr_dev, const int32_t* q_idx_dev, const float* q_val_dev,
                            int32_t B, int32_t limit, const uint32_t* mask_dev, int64_t mask_rows, uint64_t* keys_dev,
                            int32_t* counts_dev, void* stream);

/* ---- binary quantization ----------------------------------
 * Qdrant's BinaryQuantization, the engine's way: an optional 1-bit copy of the stored rows and a whole-collection stage
 * that ranks by Hamming distance.  A caller puts the stage under a dense re-scoring node (hx_rescore) with a limit a few
 * times the final one -- Qdrant's `oversampling` and `rescore`.  Additive to the ABI: HX_ABI_VERSION stays 3.
 *
 * The copy.  hx_binary_enable (idempotent) allocates it at the index's row capacity and derives rows [0, hx_count) from
 * the stored normalised fp32 rows; from then on every entry that adds, replaces, removes or truncates rows carries it.  Bit
 * j & 31 of word j >> 5 of a row is 1 when the STORED normalised value dense[row][j] > 0: +0.0, -0.0, a value that
 * underflowed to zero in normalisation and the padding columns give 0.  It is derived data: hx_save does not write it and
 * hx_load gives an index without it (enable it again; the rows are derived again).  An index on which hx_binary_enable was
 * never called allocates nothing and runs no kernel for it.  hx_binary_debug_row copies the dim_pad / 32 words
 * (dim_pad = dim rounded up to 64) of one row to the host: the tests' hook.
 *
 * The stage.  hx_search_bin / hx_search_bin_masked, B queries q_dev [B x dim] fp32 on the device:
 *   query bits   bit j is 1 when the RAW element q[b][j] > 0 -- no normalisation (the sign does not need it).  Every one of
 *                the dim elements must be finite: a batch holding a NaN or +-Inf fails ("query values must be finite"),
 *                as hx_search_dense's does;
 *   score        of row r for query b = dim - 2 * popcount(query bits XOR row bits) over the padded width: the dot product
 *                of the two +-1 vectors, an integer in [-dim, dim], carried in the key as that fp32 value:
 *                key = (orderable(score) << 32) | (0xFFFFFFFF - id), the engine's key;
 *   order, ids   the best `limit` rows in the engine's total order (score descending, id ascending); counts[b] =
 *                min(limit, rows considered), the slots behind it 0; 1 <= limit <= 2048; ids are global, as every stage's;
 *   mask         the masked form considers exactly the rows whose bit is set: layout and the mask_rows == hx_count rule of
 *                hx_search_dense_masked; mask_dev == NULL is the unmasked entry; no row kept = counts 0, empty slots.  The
 *                mask is read inside the scan: no gathered view of the kept rows is built;
 *   refusals     before any device work: the copy is not enabled ("binary" in the message), B < 1, a limit out of range, a
 *                mask_rows that is not hx_count.  An empty index gives zero counts;
 *   synchronisation  ONE host round trip per call: behind the scan the host reads, together, the count of non-finite
 *                queries and the per-query flags of a candidate buffer that overflowed (such a query -- a corpus ordered
 *                so that every chunk beats the threshold of the rows before it -- is scanned again in fixed chunks, all
 *                enqueued).  The outputs are written by work enqueued on `stream` behind that. */
int hx_binary_enable(hx_index* h);
int hx_binary_enabled(hx_index* h, int32_t* on);
int hx_binary_debug_row(hx_index* h, int64_t row, uint32_t* words_out, int32_t cap_words);
int hx_search_bin(hx_index* h, const float* q_dev, int32_t B, int32_t limit, uint64_t* keys_dev, int32_t* counts_dev,
                  void* stream);
int hx_search_bin_masked(hx_index* h, const float* q_dev, int32_t B, int32_t limit, const uint32_t* mask_dev,
                         int64_t mask_rows, uint64_t* keys_dev, int32_t* counts_dev, void* stream);

/* ---- binary quantization, asymmetric query -----------------
 * Qdrant's BinaryQuantization(query_encoding = scalar4bits | scalar8bits): the stored rows stay at one sign bit per
 * dimension -- the copy of hx_binary_enable, unchanged -- and the QUERY keeps query_bits = 4 or 8 bits per dimension.
 * The stage nominates far better candidates than hx_search_bin at the same list length; like it, it belongs under a
 * dense re-scoring node.  Additive to the ABI: HX_ABI_VERSION stays 3.
 *
 * hx_search_bin_asym / hx_search_bin_asym_masked, B queries q_dev [B x dim] fp32 on the device:
 *   query codes  per query b, QMAX = 127 (8 bits) or 7 (4 bits), over the dim RAW fp32 elements (no normalisation):
 *                m = max_j |q[b][j]|; d_j = q[b][j] / m, ONE correctly rounded fp32 division; t_j = d_j * QMAX, ONE fp32
 *                multiplication; c_j = (int) rintf(t_j), round half to even.  |d_j| <= 1, so |c_j| <= QMAX: no clamp.
 *                m == 0 gives every c_j = 0; the columns from dim up to the padded width have code 0.  Every one of the
 *                dim elements must be finite: a batch holding a NaN or +-Inf fails ("query values must be finite").  A
 *                query whose largest magnitude is subnormal (below 2^-126) is answered without error, but its codes are
 *                outside the bit-exact contract;
 *   score        of row r for query b = sum_{j < dim} c_j * (bit_j(r) ? +1 : -1) over the stored sign bits: an integer of
 *                magnitude at most QMAX * dim <= 127 * 4096 < 2^24, carried in the key as that fp32 value (exact).  It is
 *                computed as 2 S - T: T = sum_j c_j, one integer per query, and S = the sum of c_j over the row's set
 *                bits, from the P = query_bits bit planes of the two's-complement codes:
 *                S = -2^(P-1) popcount(plane_{P-1} & row) + sum_{k < P-1} 2^k popcount(plane_k & row);
 *   order, ids, mask, limits, refusals, synchronisation
 *                exactly hx_search_bin's: the engine's key and total order (score descending, id ascending), counts and
 *                zero slots behind them, global ids, 1 <= limit <= 2048, the mask read inside the scan, the refusals before
 *                any device work (the copy is not enabled, B < 1, a limit out of range, a wrong mask_rows) and, first of
 *                all, a query_bits that is neither 4 nor 8 ("query_bits" in the message); ONE host round trip per call.
 * hx_bin_asym_debug_query (the tests' hook, as hx_binary_debug_row) runs the query kernel alone on the null stream and
 * copies to the host the planes, [B][query_bits][dim_pad / 32] words -- plane k of query b is one run of dim_pad / 32
 * words, bit j & 31 of word j >> 5 is bit k of c_j's two's complement -- and the totals T, [B]; cap_words is the room at
 * planes_out.  It needs no binary copy. */
int hx_search_bin_asym(hx_index* h, const float* q_dev, int32_t B, int32_t limit, int32_t query_bits,
                       uint64_t* keys_dev, int32_t* counts_dev, void* stream);
int hx_search_bin_asym_masked(hx_index* h, const float* q_dev, int32_t B, int32_t limit, int32_t query_bits,
                              const uint32_t* mask_dev, int64_t mask_rows,
                              uint64_t* keys_dev, int32_t* counts_dev, void* stream);
int hx_bin_asym_debug_query(hx_index* h, const float* q_dev, int32_t B, int32_t query_bits,
                            uint32_t* planes_out, int32_t* totals_out, int64_t cap_words);

/* ---- payload index -------------------------------------
 * Qdrant's create_payload_index, the engine's way: indexed payload fields live as columns beside the vectors, a filter
 * arrives as a small postfix program, and one kernel evaluates it over every row and writes the packed row mask of
 * hx_hybrid_query_*_masked / hx_retain_rows.  The engine never sees strings: the caller keeps the dictionaries.
 * A column holds one cell per row, for rows [0, filled), filled <= hx_count:
 *   HX_PAY_U32  a 32-bit code (a keyword's dictionary code, 0 / 1 of a bool); HX_PAY_U32_MISSING / _NULL say so;
 *   HX_PAY_F64  an IEEE double; the two NaN bit patterns HX_PAY_F64_MISSING / _NULL say so (every other NaN must be
 *               kept out by the caller: a NaN cell is equal to nothing and ordered against nothing).
 * Adds leave columns alone: the caller appends the cells of new rows after a successful add.  hx_truncate(n) cuts every
 * column to min(filled, n).  hx_retain_rows compacts every column that is filled to hx_count with the rows (same chunk
 * plan, same hazard rule) and DROPS a column that lags (the caller rebuilds it).  hx_save / hx_load do not store
 * columns (a loaded index has none: they are derived from the payloads); hx_destroy frees them. */
#define HX_PAY_U32 1
#define HX_PAY_F64 2
#define HX_PAY_LIST_U32 3   /* list-valued fields: one state per row -- missing, null, or a list of */
#define HX_PAY_LIST_F64 4   /* k >= 0 elements: U32 codes below HX_PAY_U32_NULL, or doubles that are not NaN              */
#define HX_PAY_TEXT 5       /* text fields: one state per row -- missing, null, or a byte string of     */
                            /* length >= 0 (the caller's lower-cased UTF-8; the engine only ever sees bytes)                   */
#define HX_PAY_U32_MISSING 0xFFFFFFFFu
#define HX_PAY_U32_NULL    0xFFFFFFFEu
#define HX_PAY_F64_MISSING 0x7FF80000FFFFFFFFull
#define HX_PAY_F64_NULL    0x7FF80000FFFFFFFEull
#define HX_PAY_MAX_COLUMNS 64
#define HX_PAY_MAX_STACK   32
#define HX_PAY_MAX_OPS     4096
#define HX_PAY_TEXT_MAX_WORDS 32        /* patterns of one HX_PAY_TEXT_ALL */
#define HX_PAY_TEXT_MAX_WORD_BYTES 64   /* bytes of one pattern */
/* a new empty column; *col = its id (ids are never reused).  Refused when the index holds HX_PAY_MAX_COLUMNS columns. */
int hx_payload_create(hx_index* h, int32_t kind, int32_t* col);
/* an unknown or dropped column is an error, here and in every entry below */
int hx_payload_drop(hx_index* h, int32_t col);
/* the cells of rows [filled, filled + n): n uint32 (HX_PAY_U32) or n doubles (HX_PAY_F64) on the host.  Refused, with
 * the column unchanged, when filled + n > hx_count.  Returns when the cells are stored. */
int hx_payload_append(hx_index* h, int32_t col, const void* cells_host, int64_t n);
int hx_payload_rows(hx_index* h, int32_t col, int64_t* filled);
/* The cells of rows [filled, filled + n) of a LIST column.  heads_host[i] = HX_PAY_U32_MISSING, HX_PAY_U32_NULL or the
 * row's element count (0 = the empty list); values_host = the elements of the rows one after another: n_values uint32
 * (HX_PAY_LIST_U32) or doubles (HX_PAY_LIST_F64).  On the device the column is a head plane (uint32 per row: missing,
 * null, 0 = a list), int64 offsets [filled + 1] and one element plane (two for doubles: low words, high words).
 * Refused, with the column unchanged: filled + n > hx_count, counts that do not sum to n_values, an element that is a
 * reserved code (>= HX_PAY_U32_NULL) or a NaN, a column that is not a list column ("kind" in the message; likewise
 * hx_payload_append on a list column), a column that would hold 2^31 elements or more.  hx_truncate cuts heads and
 * offsets (the elements behind them are dead); hx_retain_rows compacts a list column that is filled to hx_count -- the
 * heads with the rows, offsets and elements as the sparse CSR -- and drops one that lags. */
int hx_payload_append_lists(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const void* values_host,
                            int64_t n_values);
/* The cells of rows that stay where they are (client.upsert of a point whose id exists overwrites its payload,
 * qdrant_handler.py:190-193): rows_host[m] unique rows below `filled`, any order; cells_host = their m new cells, in the
 * encoding of hx_payload_append.  Afterwards the column is the column to which the final cells were appended.  Refused,
 * with the column unchanged: a row at or past `filled`, a duplicate row, a list column.  Synchronises the device. */
int hx_payload_replace(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const void* cells_host);
/* The same for a LIST column (client.upsert, qdrant_handler.py:190-193): heads_host[m] / values_host / n_values in the
 * encoding of hx_payload_append_lists, with its refusals.  The heads are scattered; offsets and elements are spliced
 * from the first replaced row on, as hx_replace_rows splices the sparse CSR. */
int hx_payload_replace_lists(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                             const void* values_host, int64_t n_values);
/* The cells of rows [filled, filled + n) of a TEXT column.  heads_host[i] = HX_PAY_U32_MISSING, HX_PAY_U32_NULL or the
 * row's byte length (0 = the empty string); bytes_host = the rows' bytes one after another, n_bytes of them.  On the device
 * the column is stored as a list column is: a head plane (uint32 per row: missing, null or the byte length), int64 offsets
 * [filled + 1] counting 32-bit words, and one plane of words holding the bytes, every row padded with zero bytes to a
 * multiple of four -- the padding is not text: the head's byte length bounds a match.  Refused, with the column unchanged:
 * filled + n > hx_count, lengths that do not sum to n_bytes, a column that is not a text column ("kind" in the message;
 * likewise hx_payload_append / _append_lists on a text column), a column that would hold 2^31 words (8 GB) or more.
 * hx_truncate, hx_retain_rows, hx_payload_drop and hx_destroy treat it as they treat a list column. */
int hx_payload_append_text(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const void* bytes_host,
                           int64_t n_bytes);
/* hx_payload_replace_lists for a TEXT column: heads_host[m] / bytes_host / n_bytes in the encoding of
 * hx_payload_append_text, with its refusals and those of hx_payload_replace (a row at or past `filled`, a duplicate). */
int hx_payload_replace_text(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                            const void* bytes_host, int64_t n_bytes);
/* The program: postfix over a per-row boolean stack (at most HX_PAY_MAX_STACK deep, exactly one entry at the end).
 *   HX_PAY_TRUE / _FALSE                 push a constant
 *   HX_PAY_IS_MISSING / _IS_NULL / _PRESENT  col   push the cell's state (PRESENT = neither missing nor null)
 *   HX_PAY_EQ  col imm                    cell == imm (U32: the code in the low word; F64: the double's bits, IEEE ==)
 *   HX_PAY_IN  col imm = set index        cell is in the set
 *   HX_PAY_LT / _LE / _GT / _GE  col imm  F64 columns only, IEEE comparison with the double in imm
 *   HX_PAY_ROW_IN  imm = set index        the local row number is in the set (uint32 rows)
 *   HX_PAY_AND / _OR / _NOT               pop two (one), push the result
 * List columns take IS_MISSING / IS_NULL / PRESENT (the row's state) and
 *   HX_PAY_ANY_EQ  col imm                some element equals imm (as EQ compares)
 *   HX_PAY_ANY_IN  col imm = set index    some element is in the set
 *   HX_PAY_ANY_RANGE  col imm = set index HX_PAY_LIST_F64 only; the set is exactly two doubles lo <= hi: some element x
 *                                         has lo <= x <= hi -- ONE element meets both bounds ([1, 10] is not in [4, 6])
 *   HX_PAY_IS_EMPTY_LIST  col             the row holds a list with no element
 * The ANY ops are false on a missing, null or empty row.  EQ / IN / LT / LE / GT / GE are refused on a list column, the
 * four list ops on a scalar column.
 * EQ, IN and the comparisons are false on a missing or null cell.  A set is `n` values on the host, ascending (equal
 * neighbours allowed): uint32 for a U32 column and ROW_IN, doubles (no NaN) for an F64 column.
 * Text columns take IS_MISSING / IS_NULL / PRESENT (the row's state) and
 *   HX_PAY_TEXT_ALL  col imm = set index   every pattern of the set occurs in the row's bytes (a byte-substring test,
 *                                         within the row's byte length); false on a missing or null row
 * Its set is a pattern blob: hx_pay_set.vals points at bytes, n = their number; uint32 P, then uint32 len[P], then the
 * patterns' bytes one after another, 1 <= P <= HX_PAY_TEXT_MAX_WORDS, 1 <= len <= HX_PAY_TEXT_MAX_WORD_BYTES.  Every
 * other column op is refused on a text column, TEXT_ALL on every other column.
 * Nested blocks: list columns that hold ONE element per object of an array of objects, so that
 * position i of every such column speaks of the same object ("aligned": equal heads and offsets for every row)
 *   HX_PAY_NESTED  col imm = m            col = a list column, the block's ANCHOR (its offsets say which element positions
 *                                         a row owns); the next m ops, 1 <= m <= HX_PAY_NESTED_MAX_OPS, are ELEMENT ops.
 *                                         Pushes ONE entry on the row stack: some element position of the row makes the
 *                                         element program true.  False on a missing, null or empty row.
 *   element ops: HX_PAY_TRUE / _FALSE / _AND / _OR / _NOT on a per-ELEMENT boolean stack (at most HX_PAY_MAX_STACK deep,
 *                exactly one entry at the end), and
 *   HX_PAY_EL_EQ  col imm                 the element of `col` at this position == imm (as ANY_EQ compares)
 *   HX_PAY_EL_IN  col imm = set index     ... is in the set
 *   HX_PAY_EL_RANGE  col imm = set index  HX_PAY_LIST_F64 only; the set is exactly two doubles lo <= hi: lo <= x <= hi
 * The columns of a block's EL ops (at most HX_PAY_NESTED_MAX_COLS distinct ones; the anchor counts only when an EL op
 * reads it) must be list columns filled to hx_count that hold as many elements as the anchor: that equality, checked on
 * the host, keeps every element read in bounds.  Alignment proper is the caller's contract (hx_payload_same_offsets
 * checks it): over columns of equal totals but different offsets a block evaluates positions, in bounds, that belong
 * to other rows. */
#define HX_PAY_NESTED_MAX_OPS 64
#define HX_PAY_NESTED_MAX_COLS 8
#define HX_PAY_TRUE 0
#define HX_PAY_FALSE 1
#define HX_PAY_IS_MISSING 2
#define HX_PAY_IS_NULL 3
#define HX_PAY_PRESENT 4
#define HX_PAY_EQ 5
#define HX_PAY_IN 6
#define HX_PAY_LT 7
#define HX_PAY_LE 8
#define HX_PAY_GT 9
#define HX_PAY_GE 10
#define HX_PAY_ROW_IN 11
#define HX_PAY_AND 12
#define HX_PAY_OR 13
#define HX_PAY_NOT 14
#define HX_PAY_ANY_EQ 15
#define HX_PAY_ANY_IN 16
#define HX_PAY_ANY_RANGE 17
#define HX_PAY_IS_EMPTY_LIST 18
#define HX_PAY_TEXT_ALL 19
#define HX_PAY_NESTED 20
#define HX_PAY_EL_EQ 21
#define HX_PAY_EL_IN 22
#define HX_PAY_EL_RANGE 23
typedef struct hx_pay_op {
  int32_t op;
  int32_t col;
  uint64_t imm;
} hx_pay_op;
typedef struct hx_pay_set {
  const void* vals;
  int64_t n;
} hx_pay_set;
/* Evaluate a program over rows [0, hx_count): mask_dev receives ceil(hx_count / 32) words in the layout of
 * hx_hybrid_query_*_masked, bits at or past hx_count zero.  n_kept (may be NULL) receives the number of set bits: the
 * call then synchronises `stream` once; with NULL nothing is read back and the call only enqueues work (the host
 * arguments are copied before it returns).  Refused before any device work: a referenced column that is unknown or not
 * filled to hx_count, a comparison on a U32 column, a list op on a scalar column or a scalar op on a list column,
 * ANY_RANGE on a U32 list column or with a set of other than two entries, TEXT_ALL on a column that is not a text column or
 * any op but the three state ops and TEXT_ALL on one, a pattern blob whose size disagrees with its header or that holds
 * no pattern, more than HX_PAY_TEXT_MAX_WORDS, an empty one or one above HX_PAY_TEXT_MAX_WORD_BYTES, a set index out of
 * range, a set that is not ascending, more than
 * HX_PAY_MAX_OPS ops, a stack that would exceed HX_PAY_MAX_STACK entries or underflow or does not end with exactly one
 * entry.  Of a nested block: m out of range or past the program's end, a row op inside a block or an EL op outside
 * one, a block column that is not a list column or not filled to hx_count, more than HX_PAY_NESTED_MAX_COLS distinct
 * columns, columns of unequal element totals, EL_RANGE on a U32 column or with a set of other than two entries, a set of
 * mixed kind, an element stack that underflows, passes HX_PAY_MAX_STACK entries or does not end at one. */
int hx_payload_mask(hx_index* h, const hx_pay_op* ops, int32_t n_ops, const hx_pay_set* sets_host, int32_t n_sets,
                    uint32_t* mask_dev, int64_t* n_kept, void* stream);
/* *same = 1 when two list columns are aligned: both filled to the same row count, with equal heads and equal offsets
 * for every row (compared on the device; the call synchronises), else 0.  Refused: an unknown column, a column that is
 * not a list column ("kind" in the message). */
int hx_payload_same_offsets(hx_index* h, int32_t col_a, int32_t col_b, int32_t* same);
/* copy one cell to the host (4 bytes of a U32 column, 8 of an F64 column), as hx_debug_row does for vectors; refused on
 * a list or text column */
int hx_payload_debug_cell(hx_index* h, int32_t col, int64_t row, void* out_host);
/* copy one row of a text column to the host: *head = what hx_payload_append_text took for it (missing, null or the byte
 * length), *count = its bytes (0 for a missing or null row), of which the first min(count, cap) go to bytes_out */
int hx_payload_debug_text(hx_index* h, int32_t col, int64_t row, uint32_t* head, void* bytes_out, int64_t cap,
                          int64_t* count);
/* copy one row of a list column to the host: *head = what hx_payload_append_lists took for it (missing, null or the
 * element count), *count = its elements, of which the first min(count, cap) go to values_out (uint32 or doubles) */
int hx_payload_debug_list(hx_index* h, int32_t col, int64_t row, uint32_t* head, void* values_out, int64_t cap,
                          int64_t* count);

/* ---- grouped search ---------------------------------------
 * Qdrant's query_points_groups(group_by, limit, group_size) (additive: the reference calls query_points only,
 * qdrant_handler.py:363-372): the best n_groups groups of a ranked list, at most group_size hits each, a row's group being
 * its cell in an HX_PAY_U32 column (a keyword's code, 0 / 1 of a bool).  The list is walked in rank order: a row whose
 * cell is HX_PAY_U32_MISSING or _NULL is skipped (Qdrant leaves out points without the field); a row whose group is
 * open and holds fewer than group_size hits joins it; a row whose group is not open opens it while fewer than n_groups
 * are open; every other row is dropped.  Groups come out ordered by their best hit, hits inside a group by rank.
 *
 * hx_group is the stage.  keys_dev [B x stride] + counts_dev [B] is a ranked list as the hybrid entries hand it out
 * (global ids, best first); counts_dev NULL = all `stride` slots; a 0 slot inside a list is skipped and keeps its rank.
 * A key whose row is not in this index (another shard's, or past hx_count) is skipped, its cell is not read.
 *   out_keys_dev [B x n_groups x group_size]   slot g * group_size + r = the r-th hit of the g-th group: the input key
 *                                              as it came (same id, same score bits), 0 = empty; every slot is written;
 *   group_codes_dev [B x n_groups]             the g-th group's code, HX_PAY_U32_MISSING for a group that was not opened;
 *   group_counts_dev [B]                       groups opened, at most n_groups.
 * Everything is enqueued on `stream`; nothing is read back.  Refused before any device work: a NULL argument (counts_dev
 * aside), B < 1, stride outside [1, 2048], n_groups or group_size below 1 or n_groups * group_size above 2048, an
 * unknown column, a column whose kind is not HX_PAY_U32 ("kind" in the message), a column not filled to hx_count. */
int hx_group(hx_index* h, int32_t col, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
             int32_t n_groups, int32_t group_size, uint64_t* out_keys_dev, uint32_t* group_codes_dev,
             int32_t* group_counts_dev, void* stream);
/* ---- a ranked list filtered on the device ------------------
 * The filter and the score_threshold of a node of a caller-defined Prefetch tree, applied to the list the node's stage
 * handed out (or, for a re-scoring node's filter, to its candidates before hx_rescore).  Additive to the ABI:
 * HX_ABI_VERSION stays 3.  keys_dev [B x stride] + counts_dev [B] is a ranked list (global ids, best first).  Per query b
 * the list is walked in rank order and slot r is kept when ALL of these hold:
 *   - r < n, n = counts_dev[b] clamped to [0, stride], or stride when counts_dev is NULL;
 *   - the key is not 0 (a 0 slot inside a list is skipped, as hx_rescore and hx_group skip it);
 *   - mask_dev given: the key's id is a row of this index (ids are global: they go through the id map as hx_rescore's
 *     candidates do; an id of another shard, or past hx_count, is dropped) and that row's bit is set.  The mask is that of
 *     hx_hybrid_query_dev_masked: bit r & 31 of word r >> 5 = local row r, bits at or past mask_rows are ignored,
 *     mask_rows must equal hx_count;
 *   - thr_dev given (B floats): !(score < thr_dev[b]) in fp32, score decoded from the key.  A score equal to the threshold
 *     stays; -inf keeps every score, +inf keeps only +inf scores, and a NaN threshold keeps EVERYTHING (the comparison is
 *     false for a NaN).
 * out_keys_dev [B x limit]: the first `limit` kept keys as they came (same id, same score bits), in order, 0 after them;
 * out_counts_dev [B]: the keys written.  A repeated id stays repeated.  Everything is enqueued on `stream`; nothing is
 * read back; the mask and the thresholds must stay valid until the work on `stream` is done.
 * Refused before any device work (the outputs are not touched): a NULL argument other than counts_dev / mask_dev /
 * thr_dev; mask_dev and thr_dev both NULL; B < 1; stride or limit outside [1, 8192] (a re-scoring union is up to 8192
 * wide and is filtered before hx_rescore); mask_rows != hx_count when a mask is given; an output that overlaps the input. */
int hx_list_keep(hx_index* h, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
                 const uint32_t* mask_dev, int64_t mask_rows, const float* thr_dev, int32_t limit,
                 uint64_t* out_keys_dev, int32_t* out_counts_dev, void* stream);
/* The whole grouped query, host in, host out: hx_hybrid_query_host (mask_host NULL) or hx_hybrid_query_host_masked run
 * with final_limit = the POOL size, then hx_group over the pool on the device, then the ids' map, the unpacking and the
 * copy out.  The pool is the ranked list the root hands out: HX_MODE_TREE the re-scored union, at most
 * min(dense_limit + rrf_limit, 2048) rows; HX_MODE_H1 the fused list, at most min(dense_limit + sparse_limit, 2048).
 * group_pool = 0 asks for that maximum, a value in [1, maximum] for a shorter pool; anything else is refused.  p's own
 * final_limit is not used (nor checked), and *p is not modified.  Outputs: scores_host / ids_host [B x n_groups x
 * group_size] in the slot order of hx_group, empty slots (-inf, -1) as hx_unpack gives them; group_codes_host
 * [B x n_groups]; group_counts_host [B].  Refusals: those of the plain call and those of hx_group. */
int hx_hybrid_query_groups_host(hx_index* h, const float* q_dense_host, const int64_t* q_indptr_host,
                                const int32_t* q_idx_host, const float* q_val_host, int32_t B, const hx_params* p,
                                const uint32_t* mask_host, int64_t mask_rows, int32_t col, int32_t group_pool,
                                int32_t n_groups, int32_t group_size, float* scores_host, int64_t* ids_host,
                                uint32_t* group_codes_host, int32_t* group_counts_host);

/* ---- MMR search --------------------------------------------
 * Qdrant's NearestQuery(mmr=Mmr(diversity, candidates_limit)) (additive: the reference calls query_points without it,
 * qdrant_handler.py:363-372; parity unpinned, the semantics below are this project's statement of it): maximal marginal
 * relevance over a ranked pool.  d = diversity as fp32 in [0, 1], a = 1.0f - d; rel_i = the score of the key at pool
 * position i; sim(i, j) = the spec dot product of the normalised fp32 rows of positions i and j over their padded width.
 * Step 0 values position i at v_i = a * rel_i; step t > 0 at v_i = (a * rel_i) - (d * m_i), m_i = the largest sim(i, s)
 * over the picks s so far (no clamp at 0).  Every product, difference and sum is one fp32 operation, round to nearest,
 * never fused; v + 0.0f follows, so that -0 and +0 are one value.  A step picks the eligible, not yet picked position of
 * the largest v, the smaller position on a tie; selection ends after `limit` picks or when no eligible position is left.
 * Not eligible: a 0 slot, a position at or past counts_dev[b], a key whose row is not in this index (another shard's, or
 * past hx_count), a row whose bit is clear in eligible_dev (packed as a row mask: bit r & 31 of word r >> 5 = row r).
 *
 * hx_mmr is the stage.  keys_dev [B x stride] + counts_dev [B] is a pool as the hybrid entries hand it out (global ids);
 * counts_dev NULL = all `stride` slots; eligible_dev NULL = every row.
 *   out_keys_dev [B x limit]     slot t = the input key of pick t as it came (same id, same score bits); the slots past
 *                                the picks are 0, which hx_unpack turns into (-inf, -1); every slot is written;
 *   out_values_dev [B x limit]   slot t = v of pick t; 0.0f past the picks;
 *   out_counts_dev [B]           picks made.
 * Everything is enqueued on `stream`; nothing is read back.  Refused before any device work, every output untouched: a
 * NULL argument (counts_dev and eligible_dev aside), B < 1, stride outside [1, 2048], limit outside [1,
 * HX_MMR_MAX_LIMIT], a diversity that is NaN or outside [0, 1], eligible_rows != hx_count when eligible_dev is given. */
#define HX_MMR_MAX_LIMIT 256
int hx_mmr(hx_index* h, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B, int32_t limit,
           float diversity, const uint32_t* eligible_dev, int64_t eligible_rows, uint64_t* out_keys_dev,
           float* out_values_dev, int32_t* out_counts_dev, void* stream);
/* The whole MMR query, host in, host out.  The plain query runs on a copy of *p with final_limit = the POOL size
 * (HX_MODE_TREE: the root's re-scored union, at most min(dense_limit + rrf_limit, 2048) rows, whose scores are the dense
 * cosines; HX_MODE_H1: the fused list, at most min(dense_limit + sparse_limit, 2048), passed once through the re-score
 * stage -- hx_rescore, full width, limit = the pool -- so that relevance is the dense cosine too: the scores that come
 * back in H1 are those cosines, NOT the fused scores).  candidates_limit = 0 asks for that maximum, a value in [1,
 * maximum] for a shorter pool; anything else is refused.  p's own final_limit is not used (nor checked), *p is not
 * modified.  mask_host NULL = every row; otherwise mask_root_only = 0 runs the pre-filtered query (the mask holds in every
 * stage, as hx_hybrid_query_host_masked) and mask_root_only = 1 runs the query unmasked and hands the mask to hx_mmr as
 * its eligibility plane: the reference's root filter, which filters the union (HX_MODE_TREE only: refused in H1).
 * Then hx_mmr over the pool on the device, the ids' map, the unpacking and the copy out.  Outputs: scores_host / ids_host
 * / values_host [B x limit] in pick order, the slots past the picks (-inf, -1, 0.0f); counts_host [B].  Refusals: those
 * of the plain call and those of hx_mmr. */
int hx_hybrid_query_mmr_host(hx_index* h, const float* q_dense_host, const int64_t* q_indptr_host,
                             const int32_t* q_idx_host, const float* q_val_host, int32_t B, const hx_params* p,
                             const uint32_t* mask_host, int64_t mask_rows, int32_t mask_root_only,
                             int32_t candidates_limit, int32_t limit, float diversity, float* scores_host,
                             int64_t* ids_host, float* values_host, int32_t* counts_host);

/* ---- late-interaction rerank -------------------------------------
 * Qdrant's multivector with comparator=MAX_SIM used as the rescoring query over the hybrid prefetch (additive: the
 * reference's "late interaction reranking" mean-pools one vector per text, qdrant_handler.py:379-382; parity unpinned, the
 * semantics below are this project's statement of it).  Additive to the ABI: HX_ABI_VERSION stays 3.
 *
 * Token form.  A token is dim_t int8 values x8[k] and one fp32 scale s, s finite and s >= 0; dim_t is a multiple of 64 in
 * [64, HX_TOKENS_MAX_DIM].  The HOST quantises, the engine only ever sees bytes (as with text columns); the rule is
 * prep.hip's, in fp32: amax = max|x|, s = amax / 127, x8 = clip(rint(x * (127 / amax)), -127, 127); amax == 0 gives
 * x8 = 0 and s = 0; non-finite input is refused by the quantiser.  Stored tokens and query tokens are quantised
 * identically; a model that emits fewer dimensions zero-pads to a multiple of 64, which changes no dot product.
 *
 * Score of a query with tokens i < Tq, 1 <= Tq <= HX_MAXSIM_MAX_QTOKENS, against a row with tokens j < Td, Td >= 1:
 *   1. I_ij = sum_k q8_i[k] * d8_j[k] in int32.  |I| <= 127^2 * 1024 < 2^24, so (float)I_ij is exact: that is why dim_t
 *      stops at 1024;
 *   2. m_i = max_j ((float)I_ij * sd_j): one fp32 multiply per pair, the max is order-free;
 *   3. t_i = m_i * sq_i;
 *   4. 64 slots: t_0 .. t_{Tq-1}, then +0.0f in every slot >= Tq;
 *   5. the 64 slots are summed by the balanced pairwise tree in index order -- (t0 + t1), (t2 + t3), ..., then pairs of
 *      those, six levels; every add is one fp32 add, round to nearest, nothing is fused;
 *   6. + 0.0f at the end, so that -0 and +0 are one value.
 * (The tree is the order the C/D layout of a 16-row MFMA tile gives without moving data: the registers of a lane, the lane
 * groups, the four tiles.  On float32 numpy arrays it is a = a[0::2] + a[1::2], six times.)  The caller keeps
 * |I| * sd * sq inside the finite range; the engine does not look.
 * Not eligible: a 0 slot, a position at or past counts_dev[b], a key whose row is not in this index, a row whose cell is
 * missing or null or holds no token (a point without the vector is not scored, as in Qdrant), a row whose bit is clear in
 * eligible_dev.  Order: score descending, the smaller pool position first on a tie.
 *
 * Storage: HX_PAY_TOKENS, a sixth column kind, one state per row -- missing, null, or Td >= 0 tokens -- made by
 * hx_payload_create_tokens (hx_payload_create refuses the kind: it has no width to give), dim_t fixed at creation.  On the
 * device it is stored as a text column is: a head plane (uint32 per row: missing, null or Td), int64 offsets [filled + 1]
 * counting 32-bit words, and one word plane.  Inside a row: Td x dim_t bytes (token j at byte j * dim_t), then Td fp32
 * scales, then zero words up to a multiple of four -- a row is dim_t / 4 * Td + 4 * ceil(Td / 4) words, so every row, every
 * token and the scales start on a 16-byte boundary.  hx_truncate, hx_retain_rows, hx_payload_drop and hx_destroy treat it as
 * they treat a list or text column (a column that lags a retain is dropped).  Programs of hx_payload_mask may use
 * IS_MISSING / IS_NULL / PRESENT / IS_EMPTY_LIST on it and nothing else.
 *   hx_payload_append_tokens   the cells of rows [filled, filled + n): heads_host[i] = HX_PAY_U32_MISSING, HX_PAY_U32_NULL
 *                              or Td; x8_host = the rows' tokens one after another, n_tokens x dim_t int8; scales_host
 *                              [n_tokens] fp32.  Refused, with the column unchanged: filled + n > hx_count, counts that do
 *                              not sum to n_tokens, a scale that is negative or not finite, a column of another kind
 *                              ("kind" in the message; likewise the other append entries on a token column), a column that
 *                              would hold 2^31 words or more.
 *   hx_payload_replace_tokens  hx_payload_replace_text for a token column: the heads are scattered, offsets and words are
 *                              spliced from the first replaced row on; the refusals of both.
 *   hx_payload_debug_tokens    the logical content of one row, not its layout: *head = what append took for it, *count =
 *                              its tokens, of which the first min(count, cap) go to x8_out [cap x dim_t] and scales_out
 *                              [cap]; *dim_t (may be NULL) = the column's width.
 *
 * hx_maxsim is the stage.  keys_dev [B x stride] + counts_dev [B] is a pool as the hybrid entries hand it out (global ids);
 * counts_dev NULL = all `stride` slots; eligible_dev NULL = every row.  q8_dev = the queries' tokens one after another,
 * dim_t bytes each, 16-byte aligned; qscale_dev their scales; q_indptr_dev [B + 1] int64 = the first token of every query
 * -- the device copy is what the kernel reads, q_indptr_host [B + 1] the same numbers for the check (nothing is read back).
 *   out_keys_dev [B x limit]   slot t = make_key(MaxSim score, the input id) of the t-th best eligible position, 0 past
 *                              them (hx_unpack turns that into (-inf, -1)); every slot is written;
 *   out_counts_dev [B]         min(limit, eligible positions).
 * Everything is enqueued on `stream`; nothing is read back.  Refused before any device work, every output untouched: a NULL
 * argument (counts_dev and eligible_dev aside), B < 1, stride or limit outside [1, 2048], a query with 0 or more than
 * HX_MAXSIM_MAX_QTOKENS tokens, an unknown column, a column that is not a token column ("kind" in the message), a column
 * not filled to hx_count, eligible_rows != hx_count when eligible_dev is given.
 *
 * hx_hybrid_query_rerank_host is the whole call, host in, host out.  The plain query runs on a copy of *p with
 * final_limit = the POOL size (the maxima of hx_hybrid_query_mmr_host, both modes; candidates_limit = 0 asks for the
 * maximum); the pool is what that query returns -- in H1 the fused list with its fused scores, NOT re-scored.  mask_host /
 * mask_root_only as hx_hybrid_query_mmr_host (a root-only mask becomes the eligibility plane; refused in H1).  Then
 * hx_maxsim, the ids' map, the unpacking and the copy out.  q8_host / qscale_host / q_indptr_host: the query tokens as
 * hx_maxsim takes them, on the host.  Outputs [B x limit], the slots past counts_host[b] (-inf, -1, -inf): scores_host =
 * MaxSim, ids_host, first_scores_host = the score the pool carried.  Refusals: those of the plain call and of hx_maxsim. */
#define HX_PAY_TOKENS 6
#define HX_TOKENS_MAX_DIM 1024
#define HX_MAXSIM_MAX_QTOKENS 64
int hx_payload_create_tokens(hx_index* h, int32_t dim_t, int32_t* col);
int hx_payload_append_tokens(hx_index* h, int32_t col, const uint32_t* heads_host, int64_t n, const int8_t* x8_host,
                             const float* scales_host, int64_t n_tokens);
int hx_payload_replace_tokens(hx_index* h, int32_t col, const int64_t* rows_host, int64_t m, const uint32_t* heads_host,
                              const int8_t* x8_host, const float* scales_host, int64_t n_tokens);
int hx_payload_debug_tokens(hx_index* h, int32_t col, int64_t row, uint32_t* head, int8_t* x8_out, float* scales_out,
                            int64_t cap, int64_t* count, int32_t* dim_t);
int hx_maxsim(hx_index* h, int32_t col, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev, int32_t B,
              const int8_t* q8_dev, const float* qscale_dev, const int64_t* q_indptr_dev, const int64_t* q_indptr_host,
              const uint32_t* eligible_dev, int64_t eligible_rows, int32_t limit, uint64_t* out_keys_dev,
              int32_t* out_counts_dev, void* stream);
int hx_hybrid_query_rerank_host(hx_index* h, const float* q_dense_host, const int64_t* q_indptr_host,
                                const int32_t* q_idx_host, const float* q_val_host, int32_t B, const hx_params* p,
                                const uint32_t* mask_host, int64_t mask_rows, int32_t mask_root_only,
                                int32_t candidates_limit, int32_t col, const int8_t* q8_host, const float* qscale_host,
                                const int64_t* qtok_indptr_host, int32_t limit, float* scores_host, int64_t* ids_host,
                                float* first_scores_host, int32_t* counts_host);

/* ---- recommend search ----------------------------------------------
 * Qdrant's RecommendQuery(positive, negative, strategy) (additive: the reference never calls it; parity unpinned, the
 * semantics below are this project's statement of it): the nearest points to given examples.  Additive to the ABI:
 * HX_ABI_VERSION stays 3.
 *
 * A call carries R requests, 1 <= R <= HX_RECO_MAX_REQUESTS.  Request r has E_r examples, 1 <= E_r <=
 * HX_RECO_MAX_EXAMPLES with E_r * dim_pad <= 32768 floats (dim_pad = dim rounded up to 64: 32 examples up to width
 * 1024, 8 at width 4096), each with a sign, +1 positive or -1 negative.  An example is a STORED ROW -- a local row in
 * [0, hx_count), as hx_replace_rows takes rows; its vector is the normalised fp32 row as stored, bit for bit -- or a RAW
 * VECTOR of dim finite fp32 values, normalised by the rule every dense query is.  p_0 .. p_{P-1} are the positives in the
 * order given, n_0 .. n_{N-1} the negatives in the order given; duplicates are allowed, a row may carry both signs.
 * sim(x, e) = the spec dot product of the stored normalised row x and e over the padded width.  Every product, sum,
 * difference and quotient below is one unfused fp32 operation, round to nearest; every final score gets + 0.0f, so that
 * -0 and +0 are one value.
 *   HX_RECO_AVERAGE     needs P >= 1.  pm[k] = (((p_0[k] + p_1[k]) + ...) + p_{P-1}[k]) / f32(P), nm likewise;
 *                       q[k] = pm[k] + (pm[k] - nm[k]) when N >= 1, else pm[k].  q then IS a raw dense query: the list
 *                       is what hx_search_dense(q, prefix = 0) returns with the excluded rows removed.
 *   HX_RECO_BEST_SCORE  s+ = max_i sim(x, p_i) (-inf when P = 0), s- = max_j sim(x, n_j) (-inf when N = 0);
 *                       score = s+ if s+ > s-, else -(s- * s-).
 *   HX_RECO_SUM_SCORES  acc = +0.0f, then acc = acc + sim(x, p_i) in order, then acc = acc - sim(x, n_j) in order.
 * A row is excluded when it is a stored example of the same request (either sign) or its bit is clear in the optional
 * row mask (the layout of hx_hybrid_query_*_masked; mask_rows must equal hx_count; an example need not be kept by the
 * mask).  Order: score descending, id ascending, as make_key(score, global id).  Request r gets min(limit, rows not
 * excluded) keys, the slots past them are 0; an empty index gives counts 0.
 *
 * ex_indptr_host [R + 1]; ex_rows_host [E] = a local row, or -1 = the next raw vector of ex_vecs_host ([n_raw x dim]
 * fp32, in the order of the -1 entries; may be NULL when there is none); ex_sign_host [E].
 * Refused before any device work, every output untouched: a NULL argument (the mask and an unneeded ex_vecs_host
 * aside), R, E_r, limit or the LDS bound out of range, a sign that is neither +1 nor -1, a row outside [0, hx_count), a
 * non-finite raw element ("finite" in the message), HX_RECO_AVERAGE with P = 0, an unknown strategy, mask_rows !=
 * hx_count with a mask.  hx_recommend synchronises `stream` (the dense stage's certificate; the scan's overflow word,
 * read once behind the scan).  hx_recommend_host adds the unpacking and the copy out: scores_host / ids_host
 * [R x limit], empty slots (-inf, -1); counts_host [R].
 * HX_DEBUG_RECO_CHUNK0 (rows of the scan's first chunk) and HX_DEBUG_RECO_CAP (keys of a request's candidate buffer, at
 * least 2 * limit) are read by hx_create, per index: tests. */
#define HX_RECO_AVERAGE 0
#define HX_RECO_BEST_SCORE 1
#define HX_RECO_SUM_SCORES 2
#define HX_RECO_MAX_REQUESTS 16
#define HX_RECO_MAX_EXAMPLES 32
#define HX_RECO_MAX_LIMIT 1024
int hx_recommend(hx_index* h, int32_t strategy, int32_t R, const int64_t* ex_indptr_host,
                 const int64_t* ex_rows_host, const int8_t* ex_sign_host, const float* ex_vecs_host,
                 const uint32_t* mask_dev, int64_t mask_rows, int32_t limit,
                 uint64_t* keys_dev /* [R x limit] */, int32_t* counts_dev /* [R] */, void* stream);
int hx_recommend_host(hx_index* h, int32_t strategy, int32_t R, const int64_t* ex_indptr_host,
                      const int64_t* ex_rows_host, const int8_t* ex_sign_host, const float* ex_vecs_host,
                      const uint32_t* mask_host, int64_t mask_rows, int32_t limit,
                      float* scores_host, int64_t* ids_host, int32_t* counts_host);

/* ---- discovery and context search ------------------------------------
 * Qdrant's DiscoverQuery(target, context = [ContextPair(positive, negative), ...]) and its target-less sibling
 * ContextQuery (additive: the reference never calls them; parity unpinned, the semantics below are this project's
 * statement of them): every context pair cuts the space in two, and the answer comes from the cell that agrees with the
 * most pairs -- nearest the target there (discovery), or anywhere in it (context).  Additive to the ABI: HX_ABI_VERSION
 * stays 3.
 *
 * A call carries R requests, 1 <= R <= HX_RECO_MAX_REQUESTS.  Request r has an optional target and P_r context pairs;
 * its examples are the target first (when has_target_host[r] = 1), then pos_0, neg_0, pos_1, neg_1, ...: E_r = has_target
 * + 2 P_r of them, 1 <= E_r <= HX_RECO_MAX_EXAMPLES (a target and 15 pairs, or 16 pairs) with E_r * dim_pad <= 32768
 * floats.  P_r >= 1 without a target, P_r >= 0 with one.  An example is a stored row or a raw vector of dim finite fp32
 * values, exactly as in hx_recommend: the same normalisation, sim(x, e) = the spec dot product over the padded width.
 * Every operation below is one unfused fp32 operation, round to nearest; the division is the correctly rounded one.
 *   fast_sigmoid(v) = v / (1.0f + |v|).
 *   With a target (discovery): rank = +0.0f; for each pair in order rank = rank + c, c = +1.0f if sim(x, pos) >
 *     sim(x, neg), -1.0f if it is less, 0.0f if they are equal.  score = rank + 0.5f * (fast_sigmoid(sim(x, target)) +
 *     1.0f), then + 0.0f.
 *   Without a target (context): acc = +0.0f; for each pair in order acc = acc + fast_sigmoid(min((sim(x, pos) -
 *     sim(x, neg)) - 0x1p-23f, 0.0f)).  score = acc + 0.0f: exactly +0 for a row on the positive side of every pair.
 * A row is excluded when it is a stored example of the same request or its bit is clear in the optional row mask (the
 * layout and rules of hx_recommend; an example need not be kept by the mask).  Order: make_key(score, global id)
 * descending -- score descending, id ascending; among the (many) rows a context search scores +0 the smallest ids win.
 * Request r gets min(limit, rows not excluded) keys, the slots past them are 0; 1 <= limit <= HX_RECO_MAX_LIMIT; an empty
 * index gives counts 0.
 *
 * ex_indptr_host [R + 1]; ex_rows_host [E] = a local row, or -1 = the next raw vector of ex_vecs_host ([n_raw x dim]
 * fp32, in the order of the -1 entries; may be NULL when there is none); has_target_host [R] of 0 | 1.
 * Refused before any device work, every output untouched: a NULL argument (the mask and an unneeded ex_vecs_host
 * aside), R, E_r, limit or the LDS bound out of range, a request with neither target nor pair, a pair without its
 * negative, has_target neither 0 nor 1, a row outside [0, hx_count), a non-finite raw element ("finite" in the message),
 * mask_rows != hx_count with a mask.  hx_discover synchronises `stream` (the scan's overflow word, read once behind the
 * scan).  hx_discover_host adds the unpacking and the copy out: scores_host / ids_host [R x limit], empty slots
 * (-inf, -1); counts_host [R].
 * The scan appends a row when its KEY beats the limit-th best key so far, so rows that tie the limit-th score cost
 * nothing; rows ordered so that every chunk beats the threshold overflow a request's buffer, and the request is redone in
 * fixed chunks -- the same list.  hx_discover_redone: how many requests of this index took that redo so far.
 * HX_DEBUG_DISCOVER_CHUNK0 (rows of the scan's first chunk) and HX_DEBUG_DISCOVER_CAP (keys of a request's candidate
 * buffer, at least 2 * limit) are read by hx_create, per index: tests. */
int hx_discover(hx_index* h, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host,
                const float* ex_vecs_host, const int32_t* has_target_host,
                const uint32_t* mask_dev, int64_t mask_rows, int32_t limit,
                uint64_t* keys_dev /* [R x limit] */, int32_t* counts_dev /* [R] */, void* stream);
int hx_discover_host(hx_index* h, int32_t R, const int64_t* ex_indptr_host, const int64_t* ex_rows_host,
                     const float* ex_vecs_host, const int32_t* has_target_host,
                     const uint32_t* mask_host, int64_t mask_rows, int32_t limit,
                     float* scores_host, int64_t* ids_host, int32_t* counts_host);
int hx_discover_redone(hx_index* h, int64_t* requests);

/* ---- distance matrix search ------------------------------------------
 * Qdrant's search_matrix_pairs / search_matrix_offsets (additive: the reference never calls them; parity unpinned, the
 * semantics below are this project's statement of them): for every point of a sample, its nearest neighbours among the
 * OTHER points of the sample.  Additive to the ABI: HX_ABI_VERSION stays 3.
 *
 * The sample is S distinct local rows r_0 .. r_{S-1} in [0, hx_count), in any order, 1 <= S <= HX_MATRIX_MAX_SAMPLE.
 * sim(a, b) = the spec dot product of the stored normalised fp32 rows a and b over the padded width, as hx_recommend
 * defines it: every product and sum one unfused fp32 operation, the result + 0.0f.  sim(a, b) and sim(b, a) are the same
 * bits.  The candidates of r_i are the r_j, j != i, with sim(r_i, r_j) >= score_threshold (a finite fp32, or -inf =
 * none).  Of them the best `limit` are kept, 1 <= limit <= HX_MATRIX_MAX_LIMIT: score descending, id ascending, as
 * make_key(sim, global id of r_j) -- the keys hx_recommend hands out.  Output row i belongs to r_i in the order given:
 * counts[i] = min(limit, candidates of r_i), the slots past it are 0.  S = 1 gives one row with count 0.
 * The engine reads the S sample rows only: the cost depends on S, dim and limit, never on hx_count.  There is no mask:
 * the caller has chosen the rows.
 *
 * Refused before any device work, every output untouched: a NULL argument, S or limit out of range, a row outside
 * [0, hx_count), a row listed twice, a NaN threshold.  hx_search_matrix synchronises `stream`.  hx_search_matrix_host
 * adds the unpacking and the copy out: scores_host / ids_host [S x limit], empty slots (-inf, -1); counts_host [S].
 * HX_DEBUG_MATRIX_SCAN_ONLY=1 (read by hx_create, per index: diagnostics) stops a call behind the scan kernel and zeroes
 * the outputs, so that the scan can be timed alone. */
#define HX_MATRIX_MAX_SAMPLE 4096
#define HX_MATRIX_MAX_LIMIT 1024
int hx_search_matrix(hx_index* h, const int64_t* rows_host, int32_t S, int32_t limit, float score_threshold,
                     uint64_t* keys_dev /* [S x limit] */, int32_t* counts_dev /* [S] */, void* stream);
int hx_search_matrix_host(hx_index* h, const int64_t* rows_host, int32_t S, int32_t limit, float score_threshold,
                          float* scores_host, int64_t* ids_host /* [S x limit] */, int32_t* counts_host);

/* ---- payload facets -------------------------------------------
 * Qdrant's facet(collection, key, facet_filter, limit, exact) (additive: the reference never calls it; parity unpinned, the
 * semantics below are this project's statement of it): for every value of a keyword or bool field, the number of points a
 * filter keeps that hold the value -- a list-valued field holds a value when some element equals it, and a point counts
 * ONCE per value however often its list repeats it; missing, null and [] contribute nothing -- and of those the `limit`
 * values with the largest counts, count descending, value ascending.  The engine sees codes: the caller keeps the
 * dictionary and hands over the position of every code's value in sorted order.
 *
 * hx_payload_facet is the count.  col = an HX_PAY_U32 or HX_PAY_LIST_U32 column filled to hx_count; mask_dev = a packed
 * row mask in the layout of hx_payload_mask, NULL = every row, otherwise mask_rows must equal hx_count;
 *   counts_dev [n_codes] uint32   entry c = the kept rows holding code c; EVERY entry is written, zeros included;
 *   stray_dev [1] uint64          the kept cells / elements (each one, repeats included) whose code is >= n_codes and below
 *                                 HX_PAY_U32_NULL: the engine cannot know the caller's dictionary, a caller that sees a
 *                                 non-zero stray knows its dictionary is out of step with the column.
 * Everything is enqueued on `stream`; nothing is read back.  Refused before any device work, both outputs untouched: a
 * NULL h, counts_dev or stray_dev, n_codes of 0 or above 0xFFFFFFFE, an unknown column, a column of another kind ("kind"
 * in the message), a column not filled to hx_count, mask_rows != hx_count with a mask.
 * n_codes <= HX_FACET_LDS_CODES is counted in a histogram per workgroup in LDS (64 KB: two workgroups per CU), anything
 * above with global atomics; the counts are the same either way.
 *
 * hx_facet_top is the ranking: the at most `limit` codes of counts_dev [n_codes] with a non-zero count, each as a key
 * count << 32 | (0xFFFFFFFF - rank), sorted descending -- rank = rank_dev[code], or the code itself when rank_dev is NULL.
 * rank_dev [n_codes] uint32 is a permutation of [0, n_codes): the position of each code's value in sorted order, which is
 * how the tie order "value ascending" reaches the device without a string crossing the ABI.  out_keys_dev [limit]: every
 * slot is written, the slots past the hits are 0; *out_count_dev (int32) = the hits.  Everything is enqueued on `stream`;
 * the scratch (8 bytes per code at most) is the index's.  Refused before any device work: a NULL h, counts_dev,
 * out_keys_dev or out_count_dev, n_codes of 0 or above 0xFFFFFFFE, limit outside [1, 2048].
 *
 * hx_payload_facet_host is the whole call, host in, host out: mask_host NULL = every row; rank_host NULL or [n_codes];
 * the two stages with scratch from the index, one synchronisation.  ranks_or_codes_host [limit] uint32 = the hits' ranks
 * when rank_host is given, their codes when it is NULL; counts_host [limit] uint32 their counts; both 0 past *n_out
 * (int32) hits; *stray_host as above (a caller that sees it non-zero discards the hits).  Refusals: those of the two
 * stages, and a NULL output. */
#define HX_FACET_LDS_CODES 16384
int hx_payload_facet(hx_index* h, int32_t col, const uint32_t* mask_dev, int64_t mask_rows, uint32_t n_codes,
                     uint32_t* counts_dev, uint64_t* stray_dev, void* stream);
int hx_facet_top(hx_index* h, const uint32_t* counts_dev, uint32_t n_codes, const uint32_t* rank_dev, int32_t limit,
                 uint64_t* out_keys_dev, int32_t* out_count_dev, void* stream);
int hx_payload_facet_host(hx_index* h, int32_t col, const uint32_t* mask_host, int64_t mask_rows, uint32_t n_codes,
                          const uint32_t* rank_host, int32_t limit, uint32_t* ranks_or_codes_host, uint32_t* counts_host,
                          int32_t* n_out, uint64_t* stray_host);

/* ---- scroll -----------------------------------------------------
 * Qdrant's scroll(collection, scroll_filter, limit, offset, order_by) (additive: the reference never calls it; parity
 * unpinned, the semantics below are this project's statement of it): the points a filter keeps, page by page, in row
 * order (the insertion order every tie of this project uses) or in the order of a number field.
 *
 * hx_scroll_rows is the page in row order: the first `limit` local rows r >= start_row whose bit is set in mask_dev (a
 * packed row mask in the layout of hx_payload_mask; NULL = every row, otherwise mask_rows must equal hx_count),
 * ascending.  out_rows_dev [limit] uint32: every slot is written, 0 past *out_count_dev (int32) hits.
 *
 * hx_payload_order is the ordered page: col = an HX_PAY_F64 column filled to hx_count.  The ORDER VALUE of a cell x is
 * x + 0.0 (-0.0 orders as 0.0); as an integer, with b the 64 bits of x + 0.0:  u = b ^ (b >> 63 ? ~0 : 1 << 63), and
 * s = u for HX_ORDER_ASC, ~u for HX_ORDER_DESC.  The order is (s ascending, row ascending) in BOTH directions.  A row is
 * eligible when its mask bit is set (or there is no mask), its cell is neither HX_PAY_F64_MISSING nor HX_PAY_F64_NULL
 * (any other bit pattern, another NaN included, orders by its s), and
 *   HX_ORDER_HAS_START   s(cell) >= s(start_from): the cell is >= start_from ascending, <= start_from descending;
 *   HX_ORDER_HAS_AFTER   (s(cell), row) > (s(after_value), after_row) as a pair: the row lies strictly after the cursor.
 *                        The engine compares the pair and never looks at the cell of after_row (after_row may be any
 *                        value >= 0, past hx_count included).
 * The outputs are the best `limit` eligible rows in that order: out_rows_dev [limit] uint32 the rows, out_bits_dev
 * [limit] uint64 the STORED cells of those rows (a stored -0.0 comes back as -0.0), *out_count_dev (int32) the hits;
 * every slot is written, 0 past the hits.  The result is exact and the same bits on every run.
 *
 * Both entries only enqueue work on `stream` (scratch from the index); nothing is read back.  Refused before any device
 * work, the outputs untouched: a NULL h or a NULL output, limit outside [1, HX_SCROLL_MAX_LIMIT], mask_rows != hx_count
 * with a mask, start_row outside [0, hx_count], an unknown column, a column of another kind ("kind" in the message), a
 * column not filled to hx_count, a direction other than 0 or 1, flag bits other than the two above, a NaN start_from /
 * after_value or a negative after_row when its flag is set.  An empty index gives 0 hits.
 *
 * The _host forms are the whole call, host in, host out: mask_host NULL = every row; the mask goes up, the kernels run
 * and the page comes back behind one synchronisation, scratch from the index.  Same refusals. */
#define HX_ORDER_ASC 0
#define HX_ORDER_DESC 1
#define HX_ORDER_HAS_START 1
#define HX_ORDER_HAS_AFTER 2
#define HX_SCROLL_MAX_LIMIT 2048
int hx_scroll_rows(hx_index* h, const uint32_t* mask_dev, int64_t mask_rows, int64_t start_row, int32_t limit,
                   uint32_t* out_rows_dev, int32_t* out_count_dev, void* stream);
int hx_payload_order(hx_index* h, int32_t col, const uint32_t* mask_dev, int64_t mask_rows, int32_t direction,
                     int32_t flags, double start_from, double after_value, int64_t after_row, int32_t limit,
                     uint32_t* out_rows_dev, uint64_t* out_bits_dev, int32_t* out_count_dev, void* stream);
int hx_scroll_rows_host(hx_index* h, const uint32_t* mask_host, int64_t mask_rows, int64_t start_row, int32_t limit,
                        uint32_t* out_rows_host, int32_t* out_count_host);
int hx_payload_order_host(hx_index* h, int32_t col, const uint32_t* mask_host, int64_t mask_rows, int32_t direction,
                          int32_t flags, double start_from, double after_value, int64_t after_row, int32_t limit,
                          uint32_t* out_rows_host, uint64_t* out_bits_host, int32_t* out_count_host);

/* ---- sparse text provider (host cores) ---------------------------------------
 * EmbeddingHandler.encode_sparse (app/core/embedding/embedding_handler.py:101-142 -> fastembed
 * Qdrant/bm25 :41, :123), batched (the reference's TODO :100): n texts -> CSR of (term id, weight)
 * rows.  texts[i] = lens[i] UTF-8 bytes.  flags[i] = 1 marks a text with non-ASCII bytes: its row
 * is empty and the caller handles it (rag_application_amd/bm25.py).  cap = capacity of idx/val
 * (sum of lens[i]/2 + 1 suffices).  threads <= 0: one per core, at most 16. */
int hx_bm25_embed_batch(const char* const* texts, const int64_t* lens, int64_t n, double k, double b,
                        double avg_len, int32_t threads, int64_t* indptr, int32_t* idx, double* val,
                        int64_t cap, int32_t* flags);

/* ---- score-boosting search -----------------------------------------
 * Qdrant's FormulaQuery ("score boosting") as the rescoring query over the hybrid prefetch (additive: the reference calls
 * query_points without it; parity unpinned, the semantics below are this project's statement of it).  Additive to the ABI:
 * HX_ABI_VERSION stays 3.
 *
 * A formula arrives as a POSTFIX PROGRAM over a stack of doubles, evaluated once per pool position.  Every operation is
 * ONE IEEE double operation, round to nearest, never fused.  `imm` = the bits of a double unless said otherwise:
 *   HX_F_CONST        push imm;
 *   HX_F_SCORE        push (double) of the fp32 score of the pool key at this position;
 *   HX_F_VAR          arg = an HX_PAY_F64 column: push the row's cell, imm (the default) when the cell is
 *                     HX_PAY_F64_MISSING or HX_PAY_F64_NULL;
 *   HX_F_COND         arg = a condition plane in [0, n_planes): push 1.0 when the row's bit is set in it, else 0.0;
 *   HX_F_ADD / _MUL   pop b, pop a, push a + b / a * b;
 *   HX_F_NEG / _ABS   the sign bit of the top entry flipped / cleared;
 *   HX_F_DIV          pop b, pop a; b == 0.0 (either zero): push imm (by_zero_default; a NaN when there is none);
 *                     otherwise push a / b;
 *   HX_F_SQRT         sqrt(a), a NaN for a negative a (-0.0 gives -0.0);
 *   HX_F_EXP          hx_exp(a), below;
 *   HX_F_LIN_DECAY    pop d, t = 1.0 - imm * abs(d), push t < 0.0 ? 0.0 : t (a NaN stays a NaN);
 *                     imm = (1 - midpoint) / scale, computed by the caller;
 *   HX_F_EXP_DECAY    pop d, push hx_exp(imm * abs(d)); imm = ln(midpoint) / scale;
 *   HX_F_GAUSS_DECAY  pop d, push hx_exp(imm * (d * d)); imm = ln(midpoint) / (scale * scale).
 * A decay's d = x - target is compiled as x, target, NEG, ADD.
 * hx_exp(x), the project's own exponential: a NaN gives that NaN; x > 709.0 gives +inf; x < -708.0 gives 0.0 (so no
 * subnormal ever comes out of the ldexp); otherwise k = rint(x * 1.4426950408889634), r = (x - k *
 * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10, p = Horner's rule from degree 13 down over the
 * coefficients (double)(1.0 / i!), every step p = p * r + c_i as two roundings, and the result is ldexp(p, (int)k).
 *
 * The VALUE of a position is the stack's last entry rounded to fp32 (round to nearest even; out of range = +-inf), then
 * + 0.0f (-0 and +0 are one value).  Eligible positions are those of hx_mmr: not a 0 slot, before counts_dev[b], a key
 * whose row is in this index, a row whose bit is set in eligible_dev.  An eligible position whose value is not finite is
 * DROPPED and counted in out_dropped_dev.  With a score_threshold that is not a NaN, positions whose value is < the
 * threshold are cut too (not counted).  The survivors are ordered by value descending, then pool position ascending (a
 * constant formula returns the pool in its own order); the first `limit` come out.
 *
 * hx_formula is the stage.  ops_host [n_ops] is read before the call returns.  planes_dev = a HOST array of n_planes
 * device pointers to packed row masks of plane_rows rows each (NULL when n_planes = 0).  keys_dev [B x stride] +
 * counts_dev [B] is a pool as the hybrid entries hand it out (global ids); counts_dev NULL = all `stride` slots;
 * eligible_dev NULL = every row.
 *   out_keys_dev [B x limit]   slot t = make_key(value, the id of the input key of hit t); 0 past the hits;
 *   out_pos_dev [B x limit]    the pool position of hit t; -1 past the hits;
 *   out_counts_dev [B]         hits;    out_dropped_dev [B]   positions dropped.
 * Everything is enqueued on `stream`; nothing is read back.  Refused before any device work, every output untouched: a
 * NULL argument (counts_dev and eligible_dev aside; planes_dev when n_planes = 0), B < 1, stride or limit outside [1,
 * 2048], n_ops outside [1, HX_FORMULA_MAX_OPS], n_planes outside [0, HX_FORMULA_MAX_PLANES], a program that underflows
 * its stack, holds more than HX_FORMULA_MAX_STACK entries at some point or does not end with exactly one entry, an
 * unknown op, an unknown column, a column that is not HX_PAY_F64 or not filled to hx_count, a plane index outside [0,
 * n_planes), an HX_F_VAR default that is a NaN, plane_rows != hx_count when n_planes > 0, eligible_rows != hx_count when
 * eligible_dev is given. */
#define HX_F_CONST 0
#define HX_F_SCORE 1
#define HX_F_VAR 2
#define HX_F_COND 3
#define HX_F_ADD 4
#define HX_F_MUL 5
#define HX_F_NEG 6
#define HX_F_ABS 7
#define HX_F_DIV 8
#define HX_F_SQRT 9
#define HX_F_EXP 10
#define HX_F_LIN_DECAY 11
#define HX_F_EXP_DECAY 12
#define HX_F_GAUSS_DECAY 13
#define HX_FORMULA_MAX_OPS 256
#define HX_FORMULA_MAX_STACK 16
#define HX_FORMULA_MAX_PLANES 8
typedef struct hx_formula_op {
  int32_t op;
  int32_t arg;
  uint64_t imm;
} hx_formula_op;
int hx_formula(hx_index* h, const hx_formula_op* ops_host, int32_t n_ops, const uint32_t* const* planes_dev,
               int32_t n_planes, int64_t plane_rows, const uint64_t* keys_dev, int32_t stride, const int32_t* counts_dev,
               int32_t B, int32_t limit, float score_threshold, const uint32_t* eligible_dev, int64_t eligible_rows,
               uint64_t* out_keys_dev, int32_t* out_pos_dev, int32_t* out_counts_dev, int32_t* out_dropped_dev,
               void* stream);
/* The whole boosted query, host in, host out.  The plain query runs on a copy of *p with final_limit = the POOL size, as
 * in hx_hybrid_query_mmr_host (candidates_limit, mask_host and mask_root_only mean what they mean there), but the pool
 * keeps the scores its mode hands out -- HX_MODE_TREE: the dense cosines of the root's re-scored union; HX_MODE_H1: the
 * fused RRF scores; there is no extra re-score.  planes_host = n_planes host row masks of hx_count rows each (packed),
 * uploaded as the condition planes.  Then hx_formula over the pool on the device, the ids' map, the unpacking and the
 * copy out.  Outputs [B x limit] in rank order: scores_host = the values, ids_host, base_scores_host = the score the
 * pool carried at the hit's position; (-inf, -1, -inf) past the hits; counts_host [B], dropped_host [B].  Refusals:
 * those of the plain call, of hx_hybrid_query_mmr_host on its pool and mask, and of hx_formula. */
int hx_hybrid_query_formula_host(hx_index* h, const float* q_dense_host, const int64_t* q_indptr_host,
                                 const int32_t* q_idx_host, const float* q_val_host, int32_t B, const hx_params* p,
                                 const uint32_t* mask_host, int64_t mask_rows, int32_t mask_root_only,
                                 int32_t candidates_limit, const hx_formula_op* ops_host, int32_t n_ops,
                                 const uint32_t* const* planes_host, int32_t n_planes, int32_t limit,
                                 float score_threshold, float* scores_host, int64_t* ids_host, float* base_scores_host,
                                 int32_t* counts_host, int32_t* dropped_host);

/* ---- collection term statistics and the sparse IDF modifier --------------------------------------
 * Qdrant's SparseVectorParams(modifier=Modifier.IDF): the server keeps per-term document frequencies and multiplies
 * every query weight by ln(1 + (N - df + 0.5) / (df + 0.5)) at query time.  The statistics are read off the inverted
 * index, so they follow every add, delete, upsert, truncate and load with no bookkeeping of their own.  Parity unpinned
 * (DESIGN.md section 0): Qdrant's own arithmetic is recalled, not run; the arithmetic below is this project's, bit for bit.
 *   df_t  = postings of term t in the base view plus postings in the tail view of the up-to-date inverted index (the
 *           entries bring it up to date as hx_search_sparse does).  A term in neither view, or a negative id: 0.  Row
 *           masks do not enter: a filtered query uses the whole collection's statistics, as in Qdrant.
 *   N     = rows r < hx_count whose document-major CSR row is not empty (indptr[r + 1] > indptr[r]): a point stored
 *           without a sparse vector is not in the sparse index.
 *   x     = 1.0 + ((double)(N - df) + 0.5) / ((double)df + 0.5), N - df in int64 after N = max(N, 0) and df clamped to
 *           [0, N], so x > 1 whatever a caller passes; the add, the divide and the final add are one IEEE double
 *           operation each.
 *   idf   = (float)hx_ln(x), rounded to nearest;  out = q_val * idf, one fp32 multiply.  A non-finite q_val stays
 *           non-finite (the search flags the query as before); idf > 0, so positive weights stay positive unless the
 *           product underflows to 0 -- such a query takes the document-at-a-time path, which is exact.
 *   hx_ln(x), x a positive normal double: (m, e) = frexp(x), m in [0.5, 1); if m < 0.7071067811865476 then m = m * 2,
 *           e = e - 1; s = (m - 1) / (m + 1); z = s * s; p = c_11, then for i = 10 .. 0: p = p * z, p = p + c_i with
 *           c_i = (double)(1.0 / (2 i + 1)) (two roundings a step); t = 2.0 * s, t = t * p; the result is
 *           (double)e * 0.6931471805599453 + t, one multiply and one add.  Within 4 ulp of the correctly rounded
 *           logarithm over the arguments x(N, df) above (DESIGN.md section 31 has the measurement).
 * hx_sparse_df: df_dev [nnz] and *n_docs_dev (one int64 on the device) for the flat array of term ids q_idx_dev [nnz];
 * nnz = 0 writes N only (q_idx_dev and df_dev may then be NULL).  hx_sparse_idf_apply needs no index (as hx_rrf):
 * out_val_dev [nnz] from q_val_dev, df_dev and *n_docs_dev; out_val_dev may be q_val_dev; nnz = 0 does nothing.  Both
 * are enqueued on `stream`; nothing is read back.  hx_sparse_idf_host: host in, host out -- out_val_host [nnz], and when
 * not NULL df_host [nnz] and *n_docs_host.  Refused before any device work, every output untouched: a NULL handle, a
 * NULL pointer (the two optional outputs and the nnz = 0 cases aside), nnz < 0. */
int hx_sparse_df(hx_index* h, const int32_t* q_idx_dev, int64_t nnz, int64_t* df_dev, int64_t* n_docs_dev, void* stream);
int hx_sparse_idf_apply(int32_t device, const float* q_val_dev, const int64_t* df_dev, const int64_t* n_docs_dev,
                        int64_t nnz, float* out_val_dev, void* stream);
int hx_sparse_idf_host(hx_index* h, const int32_t* q_idx_host, const float* q_val_host, int64_t nnz,
                       float* out_val_host, int64_t* df_host, int64_t* n_docs_host);

/* ---- persistence ------------------------------------------------------------
 * The reference asks Qdrant for on-disk vectors (qdrant_handler.py:47-55, 62: on_disk=True,
 * memmap_threshold).  hx_save writes the collection to one file (stored vectors as they stand plus
 * the sparse CSR); hx_load creates a new index from it -- searches return the same lists, bit for
 * bit; the inverted index is rebuilt on the device. */
int hx_save(hx_index* h, const char* path);
int hx_load(const char* path, int32_t device, hx_index** out);

/* ---- introspection (tests, bench) ------------------------------------------ */
typedef struct hx_stats {
  int64_t n_rows, nnz, n_segments;
  int64_t n_groups;       /* live terms of the inverted index */
  int64_t hash_capacity;  /* entries of its [live term x segment] offset table (field names kept from ABI v1) */
  int64_t bytes_dense_f32, bytes_dense_f16, bytes_i8, bytes_prefix, bytes_sparse;
  int64_t dense_fallback_queries;   /* queries whose certificate failed so far */
  int64_t i8_fallback_queries;
  int64_t retry_queries;            /* queries re-run with the safe geometry (overflow, underflow, certificate) */
  int64_t sparse_fallback_queries;  /* sparse queries served document-at-a-time (non-positive weights, > 64 terms, overflow) */
  /* ABI 2: the dense stage's candidate pass on the int8 matrix pipe (a per-row-scaled int8 copy of the normalised rows;
   * final scores stay exact fp32).  Queries it took, queries whose certificate failed (re-run through the fp16 scan). */
  int64_t bytes_i8_cand;
  int64_t cand8_queries;
  int64_t cand8_uncertified_queries;
  double  cand8_row_error_max;      /* largest ||x - scale * x8||_2 of any stored row: what the certificate is built from */
  int64_t tree_batches_redone;      /* HX_MODE_TREE batches whose deferred flag word was set: run again stage by stage */
  /* ABI 3: the two speculative paths switch themselves off on a collection they keep failing on (rows the int8 grid
   * resolves badly make the certificate's radius large for EVERY query; a flagged query costs the whole batch twice):
   * 1 once more than 1 query in 20 of a 4096-query window was uncertified (the fp16 copy nominates from then on),
   * 1 once 4 of 16 consecutive tree batches were redone (the tree reads its stages' flags one by one from then on). */
  int64_t cand8_switched_off;
  int64_t tree_deferral_switched_off;
} hx_stats;
int hx_get_stats(hx_index* h, hx_stats* out);
/* HIP-event profile of the hot kernels, measured on the stream they run on.
 * Index 0 = fp16 scan (k_scan<F16>), 1 = int8 scan of the "quantized" stage (k_scan<I8>), 3 = int8 candidate scan of
 * the dense stage (the same kernel over the per-row-scaled copy), 4 = the ingest kernel (K1/K2: k_prep_rows; bytes =
 * the raw row read once + every derived copy written once), 5 = the preparation of a masked query (hx_hybrid_query_*_masked:
 * the list of kept rows and the gathers of the scanned copies), 2 = sparse scoring
 * (k_sparse_select: the pass over the inverted index; bytes = 8 per posting of the queries' terms).  flops/bytes are ALGORITHMIC: 2*B*rows*D and rows*row_bytes +
 * B*row_bytes per scan launch.  hx_profile_read drains what was recorded
 * since the last read (it synchronises the recorded events). */
#define HX_PROF_SLOTS 6
typedef struct hx_prof {
  int64_t launches[HX_PROF_SLOTS];
  double ms[HX_PROF_SLOTS];
  double flops[HX_PROF_SLOTS];
  double bytes[HX_PROF_SLOTS];
} hx_prof;
/* Which copy nominates the candidates of the full-vector dense stage: 1 = the per-row-scaled int8 copy (the
 * default; a query its certificate does not cover is re-run on the fp16 copy), 0 = the fp16 copy.  The lists are the
 * same either way (final scores are exact fp32): this is a measurement and test switch. */
int hx_set_dense_candidates(hx_index* h, int32_t kind);
/* *kind = 1 when the int8 copy nominates this index's dense candidates now, 0 when the fp16 copy does (switched by
 * hx_set_dense_candidates(h, 0), by the guard that turns the int8 pass off for rows it resolves badly, or an index
 * created without the int8 copy).  The candidates-first sharded H1 exchange needs 1 on every shard. */
int hx_dense_candidates(hx_index* h, int32_t* kind);
/* Where the sparse stage of a hybrid call runs: 1 (the default) = on the index's second stream, beside the dense scans;
 * 0 = every stage on the caller's stream, one kernel at a time -- a measurement switch: a kernel's duration (hx_profile)
 * is its own only when nothing runs beside it.  The lists do not depend on it. */
int hx_set_stream_overlap(hx_index* h, int32_t on);
/* Build the inverted index again from the stored sparse vectors (K9; hx_finalize builds it once and keeps it): a
 * measurement aid for the index-build rate -- the first build of a process also pays for its temporary allocations. */
int hx_rebuild_sparse(hx_index* h);
int hx_profile(hx_index* h, int32_t enable);
int hx_profile_read(hx_index* h, hx_prof* out);
/* copy the derived row `row` (local) of one named vector to the host:
 * which = 0 dense f32 [dim], 1..3 prefix f32 [msizes[which-1]], 4 int8 [dim] (the "quantized" vector),
 * 5 int8 [dim] the candidate-pass copy of the normalised row, 6 f32 [1] its scale */
int hx_debug_row(hx_index* h, int32_t which, int64_t row, void* out_host);

#ifdef __cplusplus
}
#endif
#endif /* HX_H */
