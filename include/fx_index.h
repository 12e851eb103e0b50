/*
 * fx_index.h -- C ABI of the MI355X-native flat (brute-force) vector index.
 *
 * Drop-in boundary for the reference's dense-retrieval hot path.  The
 * reference binds faiss-cpu through SWIG; every call it makes maps to one
 * entry point below (the faiss C-API name of the same operation is given
 * for maintainers who bind through C instead of SWIG):
 *
 *   reference call site                              faiss C API                  this ABI
 *   faiss.IndexFlatL2(d)  faiss_store.py:29,126,     faiss_IndexFlatL2_new_with   fx_index_create
 *                         rag_datastore_manager.py:138
 *   index.add(x)          faiss_store.py:46,         faiss_Index_add              fx_index_add
 *                         rag_datastore_manager.py:173
 *   index.search(x, k)    faiss_store.py:64,         faiss_Index_search           fx_index_search
 *                         rag_datastore_manager.py:218
 *   index.range_search    (score >= s filter of      faiss_Index_range_search     fx_index_range_search
 *     (x, radius)          query.py:42,                                            + fx_index_range_result
 *                          2-cli-rag-search.py:48)
 *   index.search(x, k,    (a query restricted to     faiss_Index_search_with_     fx_index_search_sel
 *     params=...)          one document set; see      params                      + fx_selector_create
 *                          "filtered search" below)
 *   index.remove_ids(sel) (documents re-crawled,     faiss_Index_remove_ids       fx_index_remove_ids
 *                          edited or deleted; see                                  + fx_selector_create
 *                          "row removal" below)
 *   IndexIDMap2(index)    (ids that survive a        faiss_IndexIDMap2_new        (a mode of the index; see
 *     .add_with_ids        removal: one document id  faiss_Index_add_with_ids      "stable ids" below)
 *     (x, ids)             on its chunk rows)                                     fx_index_add_with_ids
 *     .id_map                                        faiss_IndexIDMap_id_map      fx_index_get_ids
 *     .reconstruct(id)                               faiss_Index_reconstruct      fx_index_rows_of_ids
 *                                                                                  + fx_index_reconstruct_n
 *   index.reconstruct_    (the neighbours' vectors   faiss_Index_reconstruct_     fx_index_reconstruct_batch
 *     batch(keys)          for MMR re-ranking; see    batch
 *   index.search_and_      "stored vectors by key"   faiss_Index_search_and_      fx_index_search_and_reconstruct
 *     reconstruct(x, k)    below)                     reconstruct
 *   index.compute_        (re-scoring a candidate    faiss_IndexFlat_compute_     fx_index_compute_distance_subset
 *     distance_subset      set from elsewhere)        distance_subset
 *   (is it an IDMap?)     --                         faiss_IndexIDMap_cast        fx_index_has_ids
 *   IndexIVFFlat(q, d,    (a search over nprobe of   faiss_IndexIVFFlat_new_with  fx_ivf_create, fx_ivf_add,
 *     nlist)               nlist inverted lists; see  _metric                      fx_ivf_search
 *                          "inverted file" below)
 *   IndexScalarQuantizer  (one byte per dimension:   faiss_IndexScalarQuantizer_  fx_sq_create, fx_sq_train,
 *     (d, QT_8bit)         twice the rows per GPU;    new_with                     fx_sq_add, fx_sq_search
 *                          "scalar quantizer" below)
 *   IndexIVFScalarQuant-  (both: nprobe lists of     faiss_IndexIVFScalarQuant-   fx_ivfsq_create, fx_ivfsq_train,
 *     izer(q, d, nlist,    one byte per dimension;    izer_new_with_metric         fx_ivfsq_add, fx_ivfsq_search
 *     QT_8bit)             "inverted file over 8-bit
 *                          codes" below)
 *   index.ntotal          faiss_store.py:53          faiss_Index_ntotal           fx_index_ntotal
 *   (re)IndexFlatL2(d)    faiss_store.py:126         faiss_Index_reset            fx_index_reset
 *   faiss.write_index     faiss_store.py:91,         faiss_write_index_fname      fx_index_write
 *                         rag_datastore_manager.py:186
 *   faiss.read_index      faiss_store.py:106,        faiss_read_index_fname       fx_index_read
 *                         rag_datastore_manager.py:205
 *   (GC of the index)     --                         faiss_Index_free             fx_index_free
 *   (exceptions)          faiss_store.py:79-81,120   faiss_get_last_error         fx_last_error
 *
 * Semantics follow IndexFlatL2 (squared L2, no sqrt, no normalisation,
 * results ascending, ties -> smaller id, missing slots I = -1 and
 * D = FLT_MAX).  Returned ids are bit-exact with the CPU oracle; distances
 * are recomputed exactly (fp64 sum, one rounding to fp32).
 *
 * Conventions: every function returns 0 on success and a negative FX_E*
 * code on failure, with a thread-local message in fx_last_error().  Pointers
 * are plain host or device pointers as flagged by the *_mem arguments; no
 * torch or HIP types appear in the signatures (streams are passed as void*).
 */
#ifndef FX_INDEX_H
#define FX_INDEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FxIndex FxIndex;

/* element types (storage dtype of the index, or dtype of caller buffers) */
enum { FX_F32 = 0, FX_BF16 = 1, FX_F16 = 2 };
/* metrics, numbered as faiss MetricType */
enum { FX_METRIC_INNER_PRODUCT = 0, FX_METRIC_L2 = 1 };
/* where a caller buffer lives */
enum { FX_MEM_HOST = 0, FX_MEM_DEVICE = 1 };

/* error codes */
enum {
    FX_OK = 0,
    FX_E_ARG = -1,      /* invalid argument (faiss: AssertionError in the SWIG wrapper) */
    FX_E_HIP = -2,      /* HIP runtime failure / no device                            */
    FX_E_IO = -3,       /* file open / read / write / format error                     */
    FX_E_UNSUPPORTED = -4,
    FX_E_OOM = -5,
    FX_E_INTEGRITY = -6 /* a host-output search whose candidate lists held row ids outside
                           [0, ntotal): its top-k may be missing rows (never in a correct build) */
};

/* Largest k served by the fused scan path (per query).  fx_index_search
 * itself has no k cap, as faiss's IndexFlatL2::search (faiss_store.py:49,64
 * pass the caller's k): k <= 32 takes the fused scan's fixed candidate lists,
 * 32 < k <= FX_MAX_K a block top-K refine without cross-split pruning, and
 * k > FX_MAX_K the exact sort path (every (query, row) distance exactly,
 * one radix sort per query; HBM-bound, for the rare caller that asks).
 * fx_merge_shards takes any k the same way. */
#define FX_MAX_K 1024

const char* fx_last_error(void);
int fx_device_count(int* out);

/* faiss.IndexFlatL2(d) (faiss_store.py:29).  storage_dtype FX_F32 keeps the
 * reference's fp32 codes; FX_BF16 / FX_F16 halve HBM bytes per row.
 * device: HIP device ordinal the corpus is resident on. */
int fx_index_create(int d, int storage_dtype, int metric, int device, FxIndex** out);
void fx_index_free(FxIndex* index);

/* Opt-in row L2 normalisation applied at add time (cosine / IP mode; the
 * reference default is off: SURVEY.md section 8a a8). */
int fx_index_set_normalize(FxIndex* index, int on);
/* Run the index's kernels on `stream` (a hipStream_t; NULL = the index's own
 * stream, which is a blocking stream and therefore ordered with work on the
 * legacy null stream).  Lets a caller order index work after its own
 * producers.  Switching streams keeps the index's calls in order: the new
 * stream waits (on the device, no host sync) for the work already enqueued on
 * the previous one. */
int fx_index_set_stream(FxIndex* index, void* stream);
/* Per-index tuning option (name -> integer value).  Initial
 * values come from the FX_* environment variables, read once at index
 * creation; nothing on the search path reads the environment.  Names and
 * accepted values: "search_graph" 0/1 (default 0; 1: replay small host searches
 * as one hipGraph), "scan_place" -1/0/1, "scan_sx" >= 0, "reduce_cand" 0/1/2 (small
 * batches over many splits: 1, the default, one 16-wave workgroup refine per
 * query; 2 a separate merge of 16 splits' lists first; 0 neither),
 * "f32_split" 0/1, "centre" 0/1, "scan_pub" 0/1, "prune_rank" 0..32,
 * "compact_at" 0 (= 48) or 33..64 (list fill that triggers a compaction), "union_w"
 * 0/16/32/64 (splits per union-bound window), "union_defer" 0/1 (default 1:
 * a compaction's union bound fetched by LDS-DMA and bounded a tile later
 * instead of waited for), "union_inplace" -1..64 (at most this many lists
 * per compaction bounded by the union in place beyond the deferred ones; -1,
 * the default: 0 with union_defer, all without), "tight_at" -1/0 (off) or 33..64 (a list that took
 * entries and holds at least this many gets its threshold re-bounded between
 * compactions), "cold_bound" -1/0/1 (an empty list's first record tile bounds its
 * threshold from the per-lane group minima; -1, the default: on for corpus
 * splits of <= 256 tiles), "scan_v5" 0/1/2 (default 1: the 64-row-tile scan
 * for 16-bit rows of 512 / 768 / 1536 B where it adds no padding work; 2
 * wherever it has the shape), "refine_waves" 4/8/16,
 * "convoy" 0/1 (k_scan_v5 blocks start their split where its running blocks
 * are), "convoy_every" 1/2/4/8,
 * "host_spin" 0/1, "range_cap" 0 (= 1,048,576) or 1 .. 2^30 (entries, 8 B
 * each, the range_search candidate buffer starts with; a call whose scan
 * emits more grows it to the emitted count and scans a second time; setting
 * the option drops a grown buffer), "remove_stage" 0 (= 256 MiB) or row
 * bytes .. 2^32 (bytes of the staging buffer fx_index_remove_ids gathers
 * overlapping chunks of rows into; a smaller one means more, smaller
 * chunks), "kmeans_chunk" 0 (= 131,072) or 1 .. 2^30 (rows per chunk of
 * fx_kmeans_step / fx_kmeans_update; the chunk order is part of a k-means
 * result's summation order, so this one may change the last bits of the
 * centroids).  None of the others changes results, only
 * speed.  Unknown name or out-of-range value: FX_E_ARG.  (The diagnostic
 * build libfx_index_diag.so adds test hooks -- "force_fallback",
 * "scan_dbg" -- that the product library does not have.) */
int fx_index_set_option(FxIndex* index, const char* name, int64_t value);
/* Global id of local row 0 (row-sharded multi-GPU: shard offset).  A non-zero
 * offset on a labelled index ("stable ids" below): FX_E_ARG. */
int fx_index_set_id_offset(FxIndex* index, int64_t offset);

int fx_index_dim(const FxIndex* index, int* out);
int fx_index_ntotal(const FxIndex* index, int64_t* out);
int fx_index_storage_dtype(const FxIndex* index, int* out);
int fx_index_metric(const FxIndex* index, int* out);

/* Pre-size HBM for n rows (optional; add grows geometrically). */
int fx_index_reserve(FxIndex* index, int64_t n);

/* index.add(x) (faiss_store.py:46): append n rows of x[n][d] (row-major,
 * dtype x_dtype, host or device); rows get ids ntotal .. ntotal+n-1.
 * With FX_MEM_DEVICE it is stream-ordered (returns without waiting for the
 * device, unless the code matrix has to grow). */
int fx_index_add(FxIndex* index, int64_t n, const void* x, int x_dtype, int x_mem);

/* index.search(x, k) (faiss_store.py:64): q[nq][d] -> D[nq][k] (f32),
 * I[nq][k] (int64), out buffers caller-allocated on out_mem.  k >= 1 (any
 * k; past ntotal I = -1, D = +-FLT_MAX as faiss pads).  Blocks until results are in host memory when out_mem is
 * FX_MEM_HOST; with FX_MEM_DEVICE (queries and results on the device) it
 * is stream-ordered: it enqueues its work and returns without waiting for
 * the device (the re-scan and exact fallback for uncertified queries are
 * enqueued always and decided on the device).  A host-output search returns
 * through one packed device-to-host copy [D | I | counters] and enqueues
 * that chain only when the copy says a query was uncertified (then copies
 * again).  Workspace growth (first search of a larger shape) may
 * synchronise through hipMalloc / hipFree; so does a k > FX_MAX_K search
 * whose sort workspace exceeds 512 MiB (it is released after the call, a
 * smaller one is kept for the next). */
int fx_index_search(FxIndex* index, int64_t nq, const void* q, int q_dtype, int q_mem,
                    int k, float* D, int64_t* I, int out_mem);

/* index.range_search(x, radius) (faiss IndexFlat::range_search): for every
 * query row of q[nq][d], every row y with D(q, y) < radius (L2 index;
 * IP index: q.y > radius), both strict.  D is the library's exact distance
 * (fp64 sum over the stored row, one rounding to fp32), compared as fp32
 * with the fp32 radius: membership is exact, whatever the options.  lims is
 * a host array of nq + 1: query i owns entries lims[i] .. lims[i+1] of the
 * result, ordered by ascending row id (ids carry id_offset).  The result
 * stays in index-owned device buffers until the next range search, reset or
 * free; fx_index_range_result copies it out.  Blocks in both memory modes
 * (it returns sizes).  NaN radius: FX_E_ARG.  L2 with radius <= 0, or an
 * empty index: all-zero lims.  nq == 0: FX_OK (lims[0] = 0).  At most 2^31-1
 * queries, and 2^31-1 pairs passing the MFMA filter, per call
 * (FX_E_UNSUPPORTED beyond); FX_E_OOM when the buffers cannot be allocated;
 * FX_E_INTEGRITY when a candidate word named a row outside [0, ntotal)
 * (counted in fx_index_last_dropped_candidates; never in a correct build). */
int fx_index_range_search(FxIndex* index, int64_t nq, const void* q, int q_dtype, int q_mem,
                          float radius, int64_t* lims);
/* Copy the last range search's lims[nq] results to caller buffers (host or
 * device): D f32, I int64.  FX_E_ARG when no result is stored. */
int fx_index_range_result(FxIndex* index, float* D, int64_t* I, int out_mem);
/* Of the last range search: (query, row) pairs the MFMA scan emitted (>= the
 * result count; the exact pass removed the rest) and scan passes run (1, or
 * 2 when the candidate buffer had to grow; 0 when no scan was needed). */
int fx_index_last_range_stats(FxIndex* index, int64_t* candidates, int* passes);

/* ---- filtered search: faiss IDSelector / SearchParameters ---------------
 *
 *   faiss (Python)                                  faiss C API                        this ABI
 *   IDSelectorBatch / IDSelectorArray(ids)          faiss_IDSelectorBatch_new          fx_selector_create(FX_SEL_IDS)
 *   IDSelectorBitmap(n, bitmap)                     faiss_IDSelectorBitmap_new         fx_selector_create(FX_SEL_BITMAP)
 *   IDSelectorRange(imin, imax)                     faiss_IDSelectorRange_new          fx_selector_create(FX_SEL_RANGE)
 *   IDSelectorNot(sel)                              faiss_IDSelectorNot_new            the `invert` argument
 *   SearchParameters(sel=...)                       faiss_SearchParameters_new         (the selector handle itself)
 *   index.search(x, k, params=...)                  faiss_Index_search_with_params     fx_index_search_sel
 *   (GC of the selector)                            faiss_IDSelector_free              fx_selector_free
 *
 * Ids are the ids search returns: local row r has id r + id_offset
 * (fx_index_set_id_offset).  A selector is a SNAPSHOT of the index's rows
 * [0, ntotal) at creation: it owns a device row mask (one bit per row) and the
 * ascending list of the 128-row tiles that hold a selected row; the filtered
 * scan visits those tiles only, and rows that are not selected never become
 * candidates.  After rows are added or removed or the index is reset the
 * snapshot no longer describes the index: create a new selector. */
typedef struct FxSelector FxSelector;
enum { FX_SEL_BITMAP = 0, FX_SEL_IDS = 1, FX_SEL_RANGE = 2 };

/* kind FX_SEL_BITMAP: data = n bytes; id i is a member iff
 *   data[i >> 3] & (1 << (i & 7)); ids >= 8 n are not members (IDSelectorBitmap).
 * kind FX_SEL_IDS: data = n int64 ids; duplicates and ids outside the index
 *   are ignored (IDSelectorArray / IDSelectorBatch).
 * kind FX_SEL_RANGE: data = two int64 {imin, imax} in HOST memory whatever
 *   data_mem says (n is ignored); members are imin <= id < imax
 *   (IDSelectorRange).
 * invert != 0 selects the complement within the index's rows (IDSelectorNot).
 * data_mem: FX_MEM_HOST, or FX_MEM_DEVICE -- device data is read stream-ordered
 * on the index's stream and must stay valid until that work has run.  data may
 * be NULL when n == 0 (bitmap, ids).  FX_E_ARG: null index / out, a kind other
 * than the three (named in the message), n < 0, imax < imin. */
int fx_selector_create(FxIndex* index, int kind, const void* data, int64_t n, int data_mem, int invert,
                       FxSelector** out);
/* May be called after the index was freed. */
void fx_selector_free(FxSelector* sel);
/* Selected rows and live 128-row tiles of the snapshot (synchronises with the
 * selector's build when it was created from device data). */
int fx_selector_stats(const FxSelector* sel, int64_t* rows, int64_t* tiles);
/* fx_index_search over the selector's rows only: the k nearest SELECTED rows
 * of every query; with fewer than k selected rows the missing slots hold
 * I = -1, D = +-FLT_MAX, as an index with that many rows returns; an empty
 * selection pads every slot (no scan is launched).  Argument rules (nq == 0,
 * k <= 0, dtypes, buffers) and the host / device output modes are
 * fx_index_search's; results are exact in the same sense (every stage --
 * scan, certification, re-scan, exact fallback -- sees the same subset).
 * FX_E_ARG: a selector created on another index, or a stale one (the index's
 * ntotal differs from the snapshot's: rows were added or the index reset
 * since).  k > FX_MAX_K: FX_E_UNSUPPORTED (the exact sort path takes no
 * selector).  Never replayed from a search graph.  The fx_index_last_*
 * calls report a filtered search like any other. */
int fx_index_search_sel(FxIndex* index, const FxSelector* sel, int64_t nq, const void* q, int q_dtype, int q_mem,
                        int k, float* D, int64_t* I, int out_mem);

/* ---- row removal: faiss IndexFlatCodes::remove_ids -----------------------
 *
 * IndexFlatCodes::remove_ids (faiss_Index_remove_ids): remove the selector's
 * rows.  Any selector of fx_selector_create (bitmap, ids, range, inverted)
 * that is a current snapshot of this index; one created on another index or
 * a stale one: FX_E_ARG, as fx_index_search_sel.  The kept rows keep their
 * relative order and are renumbered densely (local row r again has id
 * r + id_offset), ntotal drops by the count and *n_removed receives it.  The
 * rows are compacted where they lie (no second copy of the corpus: a staging
 * buffer of at most "remove_stage" bytes, 4 bytes per staged row for the
 * norms, and one word per 32 rows of prefix data).  Blocks.  Nothing
 * selected: FX_OK, *n_removed = 0, nothing changes and the selector stays
 * valid.  Otherwise every selector from before the call, the one passed in
 * included, is stale afterwards (also once later adds restore the old
 * ntotal), and the stored range-search result is dropped. */
int fx_index_remove_ids(FxIndex* index, const FxSelector* sel, int64_t* n_removed);
/* The plan of the last removal that removed a row (no faiss counterpart; for
 * benchmarks): the first removed row, the kept rows above it that one launch
 * moved in place (read once, written once) and those gathered into staging
 * and copied into place (read and written twice), and the chunks launched.
 * All 0 before the first removal. */
int fx_index_last_remove_stats(FxIndex* index, int64_t* first, int64_t* direct_rows, int64_t* staged_rows,
                               int64_t* chunks);

/* ---- stable ids: faiss IndexIDMap / IndexIDMap2 ---------------------------
 *
 *   faiss (Python)                                  faiss C API                        this ABI
 *   IndexIDMap(index) / IndexIDMap2(index)          faiss_IndexIDMap_new /             (the mode below)
 *                                                   faiss_IndexIDMap2_new
 *   index.add_with_ids(x, ids)                      faiss_Index_add_with_ids           fx_index_add_with_ids
 *   index.id_map                                    faiss_IndexIDMap_id_map            fx_index_get_ids
 *   IndexIDMap2.rev_map / reconstruct(id)           faiss_Index_reconstruct            fx_index_rows_of_ids
 *   (downcast test)                                 faiss_IndexIDMap_cast              fx_index_has_ids
 *
 * An index may carry a LABEL ARRAY: one caller-chosen int64 per row, resident
 * on the device, grown with the rows and compacted with them by
 * fx_index_remove_ids, so the ids a caller holds survive removals.  It is a
 * mode of the index, decided by the first add into an EMPTY index:
 * fx_index_add_with_ids turns it on, fx_index_add leaves (or turns) it off;
 * on a non-empty index the add of the other mode is FX_E_ARG (faiss: "add does
 * not make sense with IndexIDMap" / "add_with_ids not implemented for this
 * type of index").  fx_index_reset empties the index and clears the mode.
 * Labels and id_offset exclude each other: fx_index_add_with_ids with a
 * non-zero offset set, and fx_index_set_id_offset(non-zero) on a labelled
 * index, are FX_E_ARG.
 *
 * Labels are arbitrary int64: negative values, values above 2^32 and
 * duplicates are legal (one document id on several chunk rows).  -1 is legal
 * too but cannot be told from the "missing slot" marker in results.
 *
 * On a labelled index
 *   - fx_index_search, fx_index_search_sel and fx_index_range_search /
 *     fx_index_range_result return labels in I (empty slots stay -1).  Ranking
 *     stays by (distance, ROW), as faiss's IndexIDMap (the inner index ranks,
 *     then ids are translated): ties break on insertion order, not on label,
 *     and a range result stays ordered by ascending row within a query;
 *   - fx_selector_create takes the same three kinds, whose ids, range bounds
 *     and bitmap bit positions now mean LABELS: a row is selected iff its label
 *     is a member.  Bitmap membership is faiss's: (uint64_t)label >> 3 < n and
 *     the bit set, so negative labels are never members.  `invert`, the
 *     snapshot and the staleness rules are unchanged;
 *   - fx_index_remove_ids keeps its contract; the labels move with their rows;
 *   - fx_index_write writes faiss's IndexIDMap2 file: fourcc "IxM2", then the
 *     header fields of IxF2 (i32 d, i64 ntotal, i64 1<<20, i64 1<<20, u8
 *     is_trained, i32 metric), then the complete IxF2 file as the sub-index,
 *     then i64 n and n int64 labels.  (This restates faiss's write_index for
 *     IndexIDMap2 as remembered; it is not checked against a faiss build.)
 *     fx_index_read accepts "IxF2", "IxMp" (IndexIDMap) and "IxM2"; a file cut
 *     short anywhere is FX_E_IO and no index is returned. */

/* index.add_with_ids(x, ids) (IndexIDMap::add_with_ids): fx_index_add of the
 * n rows of x, row i labelled ids[i].  ids: n int64 on ids_mem.  With
 * FX_MEM_DEVICE rows and ids it is stream-ordered like fx_index_add.  n == 0:
 * FX_OK and nothing changes (the mode included).  FX_E_ARG: null x or ids with
 * n > 0, an unlabelled index that has rows, a non-zero id_offset. */
int fx_index_add_with_ids(FxIndex* index, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids,
                          int ids_mem);
/* *out = 1 when the index is in the labelled mode, else 0. */
int fx_index_has_ids(const FxIndex* index, int* out);
/* IndexIDMap::id_map: the labels of rows [i0, i0 + n) -> out (host or
 * device; a host copy blocks).  FX_E_ARG: an index without labels, a range
 * outside [0, ntotal]. */
int fx_index_get_ids(FxIndex* index, int64_t i0, int64_t n, int64_t* out, int out_mem);
/* IndexIDMap2::rev_map: rows[i] = the LAST row (the one added last) whose
 * label is ids[i], -1 when no row carries it; repeated entries of ids each
 * get the answer.  ids and rows: n int64 each, host or device (device buffers
 * are read / written stream-ordered; a host `rows` blocks).  One pass over the
 * label array whatever n.  FX_E_ARG on an index without labels;
 * FX_E_UNSUPPORTED for n > 2^31-1. */
int fx_index_rows_of_ids(FxIndex* index, const int64_t* ids, int64_t n, int ids_mem, int64_t* rows, int rows_mem);

/* Number of queries of the last search whose top-k could not be certified
 * from the scan's candidate margin and were re-scanned with a wide candidate
 * set (after an FX_MEM_DEVICE search this synchronises the index stream). */
int fx_index_last_fallbacks(FxIndex* index, int64_t* out);
/* Of those, the queries the re-scan could not certify either, re-ranked by
 * the exact fp64 scan of every row. */
int fx_index_last_exact_fallbacks(FxIndex* index, int64_t* out);
/* Candidate-list integrity of the last search: entries the exact re-rank
 * dropped because their row id (other than the empty-slot -1) lay outside
 * [0, ntotal).  Always 0 unless a scan list was corrupted; the dropped
 * entries are never gathered, so a non-zero count means the top-k may be
 * missing rows (faiss itself cannot return such a result: faiss_store.py:64).
 * A host-output search (FX_MEM_HOST) checks it itself and returns
 * FX_E_INTEGRITY; after a device-resident search the caller must read it
 * (this call synchronises the index stream). */
int fx_index_last_dropped_candidates(FxIndex* index, int64_t* out);

/* The scan plan of the last search (no faiss counterpart: which scan kernel
 * ran, for benchmarks and profiles): tile_rows 128 = k_scan_v4, 64 =
 * k_scan_v5; query_tile = queries per workgroup; splits = corpus splits per
 * query tile.  All 0 before the first search. */
int fx_index_last_scan_plan(FxIndex* index, int* tile_rows, int* query_tile, int* splits);

/* IndexFlatL2 reset (faiss_store.py:124-128). Keeps the HBM allocation. */
int fx_index_reset(FxIndex* index);

/* Copy rows [i0, i0+n) back as fp32 (host).  Used by write_index. */
int fx_index_reconstruct_n(FxIndex* index, int64_t i0, int64_t n, float* out);

/* ---- stored vectors by key: faiss reconstruct_batch / search_and_reconstruct /
 * ---- compute_distance_subset ---------------------------------------------
 *
 *   faiss (Python)                                  faiss C API                              this ABI
 *   index.reconstruct(key) / reconstruct_batch(keys) faiss_Index_reconstruct_batch           fx_index_reconstruct_batch
 *   index.search_and_reconstruct(x, k)              faiss_Index_search_and_reconstruct       fx_index_search_and_reconstruct
 *   index.compute_distance_subset(x, labels)        faiss_IndexFlat_compute_distance_subset  fx_index_compute_distance_subset
 *
 * Keys are the ids search returns: row + id_offset, or labels on a labelled
 * index ("stable ids" above: the LAST row added with a label answers for it;
 * one pass over the label array whatever n).  On the device every key is
 * checked against the index's rows before an address is formed, and a key that
 * names no row -- -1, the missing slot of a search result, included -- reads
 * no memory:
 *   - the NaN rule: its vector is a row of NaN, every bit set (fp32
 *     0xFFFFFFFF, 16-bit 0xFFFF: faiss's memset(-1) of a missing result);
 *   - the +-FLT_MAX rule: its distance is the missing slot's value, FLT_MAX
 *     on an L2 index and -FLT_MAX on an IP index, so
 *     compute_distance_subset(x, I) reproduces a padded search result.
 * Vectors come back dense [n][d] as fp32 (the exact widening of bf16 / fp16
 * rows) or in the index's storage dtype (the stored bytes). */

/* out[i][0..d) = the stored vector of keys[i]; keys: n int64 on keys_mem, out
 * on out_mem.  out_dtype: FX_F32 or the index's storage dtype (else
 * FX_E_UNSUPPORTED).  HOST keys of an unlabelled index are validated first:
 * any key outside [id_offset, id_offset + ntotal) is FX_E_ARG (faiss asserts
 * key < ntotal), the message names the first bad key and nothing is written.
 * DEVICE keys are read stream-ordered and cannot be validated without a sync:
 * a bad key gives a NaN row.  On a labelled index an unknown label gives a NaN
 * row in both modes (no sync in this layer).  With device keys and a device
 * out the call is stream-ordered; a host out goes through a bounded stage
 * buffer in chunks and blocks.  n == 0: FX_OK.  n > 2^31-1:
 * FX_E_UNSUPPORTED. */
int fx_index_reconstruct_batch(FxIndex* index, int64_t n, const int64_t* keys, int keys_mem,
                               void* out, int out_dtype, int out_mem);
/* fx_index_search (sel NULL; any k) or fx_index_search_sel (k <= FX_MAX_K,
 * else FX_E_UNSUPPORTED) with the neighbours' vectors: D and I are exactly
 * what those calls return, argument rules and error codes included, and
 * R[i][j][0..d) (dtype r_dtype: FX_F32 or the storage dtype) is the stored
 * vector of the ROW that ranked j for query i -- on a labelled index too, where
 * I[i][j] is that row's label and labels may repeat.  Missing slots (I = -1)
 * hold NaN.  With FX_MEM_DEVICE queries and results the whole call is
 * stream-ordered: the gather is enqueued behind the device-decided re-scan and
 * exact-fallback chain, no host sync.  Never recorded into or replayed from a
 * search graph. */
int fx_index_search_and_reconstruct(FxIndex* index, const FxSelector* sel, int64_t nq,
                                    const void* q, int q_dtype, int q_mem, int k,
                                    float* D, int64_t* I, void* R, int r_dtype, int out_mem);
/* D[i][j] = the library's exact distance (fp64 sum over the stored row, one
 * rounding to fp32; the arithmetic of the search's certified path, so the
 * value search returns for that pair) of query i and the row keys[i][j]; k is
 * the per-query candidate count, any positive value; keys [nq][k] int64 on
 * keys_mem.  A key that names no row: +-FLT_MAX (above).  Stream-ordered when
 * queries, keys and D are on the device.  nq == 0: FX_OK.  More than 2^31-1
 * pairs per call: FX_E_UNSUPPORTED. */
int fx_index_compute_distance_subset(FxIndex* index, int64_t nq, const void* q, int q_dtype, int q_mem,
                                     int k, const int64_t* keys, int keys_mem, float* D, int out_mem);

/* ---- k-means: faiss Kmeans / Clustering ------------------------------------
 *
 *   faiss (Python)                      faiss C++ / C API                               this ABI
 *   faiss.Kmeans(d, k).train(x)         Clustering::train / faiss_Clustering_train      fx_kmeans_step + fx_kmeans_finish, per iteration
 *   kmeans.index.search(x, 1)           Index::assign / faiss_Index_assign              fx_index_search (k = 1) on the centroid index
 *
 * One iteration of Lloyd's algorithm over a centroid index (an unlabelled flat
 * index with id offset 0 whose k = ntotal rows are the centroids).  The
 * assignment is the index's own k = 1 search, so its ids are bit-exact; the
 * update is bitwise reproducible: member lists from a stable radix sort of
 * (cluster << 32 | row) keys, fp64 sums in a fixed order, no floating-point
 * atomics.  Two runs of the same calls give the same bits; the result depends
 * on the rows, the assignment and the chunking only.
 *
 * Buffers: sums [k][d] fp64, counts [k] int64, obj one fp64, assign [n] int64,
 * dist [n] fp32, centroids_out [k][d] fp32 and n_split one int64 are always
 * DEVICE memory; x is on x_mem.  With FX_MEM_DEVICE x every call here is
 * stream-ordered on the index's stream (workspace growth may synchronise
 * through hipMalloc / hipFree); host x is staged through a bounded pinned
 * buffer (64 MiB) chunk by chunk and the call blocks.  Large n is cut into
 * chunks of the option "kmeans_chunk" rows (default 131,072: the search
 * workspace of a chunk stays near 1 GiB at d = 768 whatever n is), and the
 * chunks' results are accumulated in chunk order.
 *
 * An assign[i] outside [0, k) -- a padded search's -1 included -- forms no
 * key and no address: the row is skipped and counted.  A host-x call returns
 * FX_E_INTEGRITY when it skipped one; after device-x calls fx_kmeans_status
 * reports the count.
 *
 * Errors of the three calls: FX_E_ARG for a null index, an empty centroid
 * index, n < 0, a dtype outside the three, a bad x_mem, or null sums /
 * counts / obj (fx_kmeans_finish: any null buffer); FX_E_UNSUPPORTED for a
 * labelled centroid index, a non-zero id offset, or k > 2^31-1.  n == 0 is
 * FX_OK and changes nothing.  Never recorded into a search graph. */

/* assign / dist <- the k = 1 search of x[n][d] over the centroids (NULL: kept
 * in the library's workspace), then sums[c] = the fp64 sum of the rows
 * assigned to c, counts[c] = their number, obj = the fp64 sum of their
 * distances (L2 index: squared distances; IP index: inner products).
 * accumulate != 0 adds to what sums / counts / obj hold (a training set passed
 * in several calls); 0 overwrites them. */
int fx_kmeans_step(FxIndex* centroids, int64_t n, const void* x, int x_dtype, int x_mem,
                   int64_t* assign, float* dist,      /* device, n each; NULL = library workspace   */
                   double* sums, int64_t* counts,     /* device, [k][d] and [k]                     */
                   double* obj,                       /* device, one fp64                           */
                   int accumulate);
/* The update half alone, from the caller's assignment (device, n int64;
 * dist: device, n fp32, or NULL: obj gets 0 added).  What fx_kmeans_step runs
 * after its search. */
int fx_kmeans_update(FxIndex* centroids, int64_t n, const void* x, int x_dtype, int x_mem,
                     const int64_t* assign, const float* dist, double* sums, int64_t* counts,
                     double* obj, int accumulate);
/* centroids_out[c] = (float)(sums[c] / counts[c]) where counts[c] > 0; an
 * empty cluster keeps the row the index stores and is then repaired as
 * faiss's split_clusters does, except for the donor: faiss draws it at random
 * in proportion to the cluster sizes, here it is the cluster with the largest
 * working count (ties: the smaller index), so a training is reproducible.
 * For each empty ci in ascending order, with donor cj: c[ci] = c[cj]; for
 * even j c[ci][j] *= 1 + EPS and c[cj][j] *= 1 - EPS, for odd j the signs
 * swapped (EPS = 1/1024, fp32); working counts h[ci] = h[cj] / 2, h[cj] -=
 * h[ci].  *n_split = the repairs.  spherical != 0 then divides every centroid
 * by its L2 norm (an fp64 sum; each element rounded once).  Last, the index
 * is reset and the k new centroids are added to it, stream-ordered, so the
 * next fx_kmeans_step / search sees them (selectors built before are stale). */
int fx_kmeans_finish(FxIndex* centroids, const double* sums, const int64_t* counts, int spherical,
                     float* centroids_out /* device [k][d] */, int64_t* n_split /* device */);
/* Waits for the index's stream; *bad_assign = the assignments outside [0, k)
 * skipped since the last read (then 0 again).  FX_E_INTEGRITY when non-zero. */
int fx_kmeans_status(FxIndex* centroids, int64_t* bad_assign);
/* With fx_index_profile on, the k-means calls record events around their
 * parts; this waits and returns the milliseconds since the last read: the
 * searches, key build + sort + segments, sum + fold, and the finishes. */
int fx_kmeans_profile_read(FxIndex* centroids, double* assign_ms, double* sort_ms, double* sum_ms,
                           double* finish_ms);

/* ---- inverted file: faiss IndexIVFFlat ---------------------------------------
 *
 *   faiss (Python)                      faiss C++ / C API                               this ABI
 *   IndexIVFFlat(quantizer, d, nlist)   faiss_IndexIVFFlat_new_with_metric              fx_ivf_create
 *   index.is_trained                    faiss_Index_is_trained                          (quantizer ntotal == nlist)
 *   index.train(x)                      faiss_Index_train                               the k-means calls above, then
 *                                                                                       fx_index_add on the quantizer
 *   index.add(x) / add_with_ids(x, ids) faiss_Index_add / faiss_Index_add_with_ids      fx_ivf_add
 *   index.nprobe; index.search(x, k)    faiss_IndexIVF_set_nprobe / faiss_Index_search  fx_ivf_search
 *   index.reset()                       faiss_Index_reset                               fx_ivf_reset
 *   index.ntotal                        faiss_Index_ntotal                              fx_ivf_ntotal
 *   invlists.list_size(l)               faiss_IndexIVF_get_list_size                    fx_ivf_list_sizes
 *   invlists.get_ids(l)                 faiss_IndexIVF_invlists_get_ids                 fx_ivf_list_ids
 *   (GC of the index)                   faiss_Index_free                                fx_ivf_free
 *
 * The quantizer is an unlabelled flat index with id offset 0 on the same
 * device, BORROWED: the caller keeps it alive as long as the IVF index.  The
 * index is trained as soon as the quantizer holds nlist rows (the centroids),
 * however they got there; an add or a search before that is FX_E_ARG.
 *
 * Row i of an add goes to list quantizer.search(x_i, 1): the quantizer's own
 * metric and tie rule (the smaller centroid number).  Rows are stored in the
 * storage dtype exactly as the flat index stores them, in LIST ORDER: list l
 * owns a run of rows, in insertion order.  An add appends to the tail and the
 * next search (or list accessor) regroups: a stable device sort of
 * list << 32 | row keys and a gather into second buffers, which needs a
 * second copy of the rows while it runs (released once the buffers are
 * swapped) and is O(ntotal) per add-then-search cycle (merging only the tail
 * is future work), and reads the longest list's length
 * back to the host once (the one synchronisation of a search after an add).
 *
 * A search probes, per query, the min(nprobe, nlist) lists of
 * quantizer.search(q, nprobe), and returns the k best rows among them under
 * the index metric, ranked by (exact fp32 distance, list number, insertion
 * order within the list), i.e. by position in the list-ordered store (faiss's
 * own IVF tie order is an artefact of its heap).  Within the probed lists the
 * result is exact as the flat index's is: ids bit-exact, distances the fp64 sum
 * rounded once; with nprobe = nlist it is the flat index's result (up to the
 * tie rule).  Missing slots: I = -1, D = +-FLT_MAX.  I holds the ids of
 * fx_ivf_add: sequential from 0 in insertion order when ids was NULL, else the
 * caller's int64 (any value, duplicates included); the two may not be mixed on
 * a non-empty index (FX_E_ARG, as fx_index_add / fx_index_add_with_ids).
 *
 * Errors: FX_E_ARG for a null handle, d different from the quantizer's,
 * nlist < 1, a labelled quantizer or one with an id offset, add or search on an
 * untrained index, k < 1, nprobe < 1, a bad dtype or mem; FX_E_UNSUPPORTED for
 * k > FX_MAX_K, nq * nprobe >= 2^31, min(nprobe, nlist) > FX_MAX_K (the coarse
 * search's k), ntotal >= 2^31; FX_E_INTEGRITY when a row was assigned outside
 * [0, nlist) (it belongs to no list; counted as k-means counts them) and for a
 * host-output search whose candidate lists or probe lists held ids outside the
 * index (never in a correct build).  nq == 0 and n == 0 are FX_OK.
 *
 * Out of scope: writing / reading an IVF index (faiss's "IwFl" layout cannot
 * be checked here: persist the quantizer as IxF2 and re-add the rows),
 * remove_ids, range_search, selectors, reconstruct*, search_preassigned,
 * sharding across GPUs, the search graph (8-bit lists: "inverted file over
 * 8-bit codes" below; product-quantized lists: "inverted file over
 * product-quantized codes"). */
typedef struct FxIvf FxIvf;
int fx_ivf_create(FxIndex* quantizer, int d, int64_t nlist, int storage_dtype, int metric, FxIvf** out);
void fx_ivf_free(FxIvf* ivf);
/* ids NULL: sequential ids ntotal .. ntotal + n - 1.  Device x (and ids) is
 * stream-ordered; host x blocks. */
int fx_ivf_add(FxIvf* ivf, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem);
/* Host results block; device queries and results are stream-ordered (the first
 * search after an add synchronises once for the regroup).  k <= 32: the fused
 * path (MFMA list scan, exact refine, exact fallback for uncertified queries,
 * all decided on the device); 32 < k <= FX_MAX_K: the exact list scan.
 * Limitation: the refine certifies a query from the room between its k-th and
 * its 32nd candidate key, so as k nears 32 more queries are uncertified, and at
 * k = 32 every query whose probed lists hold 32 rows or more is; those are
 * re-ranked by the exact list scan (one thread per row, fp64), which is
 * correct but much slower than the MFMA path.  Fast for small k (k = 10: none
 * flagged on the test and benchmark corpora); a wider candidate set for k near
 * 32, as the flat index's re-scan has, is future work. */
int fx_ivf_search(FxIvf* ivf, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe,
                  float* D, int64_t* I, int out_mem);
/* Empties the lists, keeps the quantizer (and so the training). */
int fx_ivf_reset(FxIvf* ivf);
int fx_ivf_ntotal(const FxIvf* ivf, int64_t* out);
/* out: host [nlist]. */
int fx_ivf_list_sizes(FxIvf* ivf, int64_t* out);
/* *n = rows of `list`; out (host, cap entries; may be NULL with cap 0)
 * receives the first min(*n, cap) ids in insertion order. */
int fx_ivf_list_ids(FxIvf* ivf, int64_t list, int64_t* out, int64_t cap, int64_t* n);
int fx_ivf_set_stream(FxIvf* ivf, void* stream);
/* Of the last search (after a device-output one this synchronises): queries the
 * refine could not certify (re-ranked by the exact list scan, so both counts
 * are equal), and candidate / probe ids outside the index (0 in a correct
 * build). */
int fx_ivf_last_counts(FxIvf* ivf, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped);
/* With profiling on, every pass of a search records events around its parts;
 * _read waits and returns the milliseconds summed since the last read: the
 * coarse search, pairs + query preparation, the list scan (exact path: the
 * exact scan), refine + exact fallback, and the passes they cover. */
int fx_ivf_profile(FxIvf* ivf, int enable);
int fx_ivf_profile_read(FxIvf* ivf, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                        int64_t* passes);
/* The plan of the last search: path 0 fused / 1 exact, tile chunks per list,
 * candidate slots per query (nprobe * chunks), queries per pass, and the list
 * scan's launch-grid bound. */
int fx_ivf_last_plan(FxIvf* ivf, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid);

/* ---- scalar quantizer: faiss IndexScalarQuantizer (8-bit) --------------------
 *
 *   faiss (Python)                      faiss C++ / C API                               this ABI
 *   IndexScalarQuantizer(d, qtype)      faiss_IndexScalarQuantizer_new_with             fx_sq_create
 *   index.train(x)                      faiss_Index_train                               fx_sq_train
 *   index.is_trained                    faiss_Index_is_trained                          fx_sq_is_trained
 *   index.sq.trained                    ScalarQuantizer::trained                        fx_sq_get_trained / _set_trained
 *   index.add(x)                        faiss_Index_add                                 fx_sq_add
 *   index.search(x, k)                  faiss_Index_search                              fx_sq_search
 *   index.reset()                       faiss_Index_reset                               fx_sq_reset
 *   index.ntotal                        faiss_Index_ntotal                              fx_sq_ntotal
 *   index.reconstruct_n(i0, n)          faiss_Index_reconstruct_n                       fx_sq_reconstruct_n
 *   index.reconstruct_batch(keys)       faiss_Index_reconstruct_batch                   fx_sq_reconstruct_batch
 *   index.sa_encode(x) / sa_decode(c)   faiss_Index_sa_encode / faiss_Index_sa_decode   fx_sq_encode / fx_sq_decode
 *   (GC of the index)                   faiss_Index_free                                fx_sq_free
 *
 * This restates faiss's ScalarQuantizer from memory; it is NOT checked against
 * a faiss build (as the IxM2 note above).  qtype is faiss's QuantizerType
 * number: 0 QT_8bit (per dimension, RS_minmax, rangestat_arg 0: vmin_j = min_i
 * x_ij, vdiff_j = max_i x_ij - vmin_j) or 2 QT_8bit_uniform (one global min and
 * max, held as the same two arrays with equal entries).  trained is [vmin[d] |
 * vdiff[d]] in fp32 (QT_8bit_uniform reads back as [vmin, vdiff], 2 floats).
 *
 *   encode (fp32, each operation rounded once, no FMA contraction):
 *     xi = vdiff_j != 0 ? clamp((x_j - vmin_j) / vdiff_j, 0, 1) : 0,  c_j = (int)(255.f * xi) in [0, 255]
 *   decode:  y_j = vmin_j + ((c_j + 0.5f) / 255.f) * vdiff_j  (two rounded fp32
 *     operations on the table value: bitwise a numpy fp32 expression)
 *
 * The index stores the signed code c' = c - 128 (faiss's byte XOR 0x80, the
 * int8 MFMA operand) in rows of roundup(d, 128) bytes plus one fp32 constant
 * per row; fx_sq_encode / fx_sq_decode speak faiss's UNSIGNED bytes [n][d].
 *
 * A search has the flat index's contract applied to the DECODED rows: per query
 * the k rows that minimise sum (x_j - y_j)^2 (L2) or maximise sum x_j y_j (IP)
 * over the decoded fp32 y, the sum in fp64 rounded once to fp32, ranked by (that
 * value, row); missing slots I = -1, D = +-FLT_MAX; ids are row numbers in
 * insertion order.  k <= 32: the fused path (query preparation, the int8 MFMA
 * scan, exact refine + certification, the exact scan for uncertified queries,
 * all decided on the device); 32 < k <= FX_MAX_K: the exact scan for the whole
 * search.  Limitation (as the inverted file's): the exact scan is one fp64 pass
 * over every decoded row per query, correct but slow, and as k nears 32 more
 * queries fall to it (at k = 32 every query of an index with 32 rows or more).
 *
 * Errors: FX_E_ARG for a null handle, a bad dtype / mem / qtype / metric, add or
 * search before training, train or set_trained on an index that holds rows,
 * non-finite training data, k < 1; FX_E_UNSUPPORTED for k > FX_MAX_K and ntotal
 * >= 2^31; FX_E_INTEGRITY for a host-output search whose candidate lists held
 * ids outside the index (never in a correct build).  nq == 0 and n == 0 are
 * FX_OK.
 *
 * Out of scope: the 4-bit, 6-bit, fp16 / bf16 and direct qtypes and rangestat
 * other than min/max; selectors, remove_ids, range_search, IndexIDMap over it,
 * id offsets; write_index / read_index (faiss's "IxSQ" layout cannot be checked
 * here); sharding and the search graph; a re-scan stage with wider candidate
 * lists; scanning with k_scan_v5's ring (8-bit codes in inverted lists:
 * "inverted file over 8-bit codes" below). */
typedef struct FxSq FxSq;
int fx_sq_create(int d, int qtype, int metric, int device, FxSq** out);
void fx_sq_free(FxSq* sq);
/* Per-dimension min / max of x [n][d] in one pass (bitwise reproducible).  more
 * != 0: the call only accumulates (a training set handed over in chunks) and
 * the index stays untrained; the call with more == 0 finishes.  Any non-finite
 * input fails the training with FX_E_ARG (the index stays untrained). */
int fx_sq_train(FxSq* sq, int64_t n, const void* x, int x_dtype, int x_mem, int more);
int fx_sq_is_trained(const FxSq* sq, int* out);
/* out / trained: host [2 d] floats, [vmin | vdiff]. */
int fx_sq_get_trained(FxSq* sq, float* out);
int fx_sq_set_trained(FxSq* sq, const float* trained);
/* Ids are the row numbers ntotal .. ntotal + n - 1.  Device x is stream-ordered;
 * host x blocks. */
int fx_sq_add(FxSq* sq, int64_t n, const void* x, int x_dtype, int x_mem);
/* Host results block; device queries and results are stream-ordered. */
int fx_sq_search(FxSq* sq, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem);
/* Empties the index, keeps the training. */
int fx_sq_reset(FxSq* sq);
int fx_sq_ntotal(const FxSq* sq, int64_t* out);
/* out [n][d] fp32 (out_mem) <- the decoded rows [i0, i0 + n) / the rows keys[i]
 * (int64, keys_mem; a key outside [0, ntotal): a row of NaN, as the flat index). */
int fx_sq_reconstruct_n(FxSq* sq, int64_t i0, int64_t n, float* out, int out_mem);
int fx_sq_reconstruct_batch(FxSq* sq, int64_t n, const int64_t* keys, int keys_mem, float* out, int out_mem);
/* sa_encode / sa_decode: x [n][d] (x_dtype) <-> faiss's unsigned codes [n][d],
 * all three buffers in `mem`. */
int fx_sq_encode(FxSq* sq, int64_t n, const void* x, int x_dtype, uint8_t* codes, int mem);
int fx_sq_decode(FxSq* sq, int64_t n, const uint8_t* codes, float* out, int mem);
int fx_sq_set_stream(FxSq* sq, void* stream);
/* Of the last search (after a device-output one this synchronises): queries the
 * refine could not certify (all re-ranked by the exact scan, so both counts are
 * equal) and candidate ids outside the index (0 in a correct build). */
int fx_sq_last_counts(FxSq* sq, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped);
/* The plan of the last search: path 0 fused / 1 exact, query tiles of a pass,
 * corpus splits per query tile, splits of the exact scan, queries per pass, and
 * the scan's workgroups. */
int fx_sq_last_plan(FxSq* sq, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid);
/* With profiling on, every pass of a search records events around its parts;
 * _read waits and returns the milliseconds summed since the last read: query
 * preparation, the scan (exact path: the exact scan), refine + exact fallback,
 * and the passes they cover. */
int fx_sq_profile(FxSq* sq, int enable);
int fx_sq_profile_read(FxSq* sq, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes);

/* ---- product quantizer: faiss IndexPQ (8-bit) ---------------------------------
 *
 *   faiss (Python)                      faiss C++ / C API                               this ABI
 *   IndexPQ(d, M, nbits, metric)        faiss_IndexPQ_new_with_metric                   fx_pq_create
 *   index.train(x)                      faiss_Index_train                               M k-means runs (the k-means calls
 *                                                                                       above), then fx_pq_set_centroids
 *   index.is_trained                    faiss_Index_is_trained                          fx_pq_is_trained
 *   index.pq.centroids                  ProductQuantizer::centroids                     fx_pq_get_centroids / _set_centroids
 *   index.add(x)                        faiss_Index_add                                 fx_pq_add
 *   index.search(x, k)                  faiss_Index_search                              fx_pq_search
 *   index.reset()                       faiss_Index_reset                               fx_pq_reset
 *   index.ntotal                        faiss_Index_ntotal                              fx_pq_ntotal
 *   index.reconstruct_n(i0, n)          faiss_Index_reconstruct_n                       fx_pq_reconstruct_n
 *   index.reconstruct_batch(keys)       faiss_Index_reconstruct_batch                   fx_pq_reconstruct_batch
 *   index.sa_encode(x) / sa_decode(c)   faiss_Index_sa_encode / faiss_Index_sa_decode   fx_pq_encode / fx_pq_decode
 *   index.codes                         IndexPQ::codes                                  fx_pq_get_codes
 *   (GC of the index)                   faiss_Index_free                                fx_pq_free
 *
 * This restates faiss's ProductQuantizer from memory; it is NOT checked against
 * a faiss build (as the IxM2 note above).  d = M dsub; sub-quantizer m owns the
 * dimensions [m dsub, (m + 1) dsub) and 256 fp32 centroids of dsub values;
 * centroids is faiss's flat array [M][256][dsub].
 *
 *   encode:  code_m = argmin_j sum_e (x_{m dsub + e} - c_{m j e})^2, the sum in fp64 over e
 *     ascending, every operation rounded once (no FMA contraction), the lowest j on a tie
 *   decode:  y_{m dsub + e} = c_{m code_m e}  (a gather: bitwise)
 *
 * The index stores roundup(M, 16) code bytes and one fp32 constant (|decode|^2)
 * per row; fx_pq_encode / _decode / _get_codes speak faiss's row-major [n][M]
 * uint8.
 *
 * A search has the flat index's contract applied to the DECODED rows, exactly
 * as the scalar quantizer's above: the k rows that minimise sum (x_j - y_j)^2
 * (L2) or maximise sum x_j y_j (IP), the sum in fp64 rounded once to fp32,
 * ranked by (that value, row); rows with equal codes tie exactly and rank by
 * row.  k <= 32 and dsub % 8 == 0: the fused path (query preparation, the
 * gather scan on the bf16 MFMA, exact refine + certification, the exact scan
 * for uncertified queries).  32 < k <= FX_MAX_K, and every index whose dsub is
 * no multiple of 8: the exact scan for the whole search, one fp64 pass over
 * every decoded row per query -- correct but slow; fx_pq_last_plan reports it.
 *
 * Errors: FX_E_ARG for a null handle, a bad dtype / mem / metric, d % M != 0,
 * add or search before the centroids are set, set_centroids on an index that
 * holds rows, non-finite centroids, k < 1; FX_E_UNSUPPORTED for nbits != 8, k >
 * FX_MAX_K and ntotal >= 2^31; FX_E_INTEGRITY as the scalar quantizer's.  nq ==
 * 0 and n == 0 are FX_OK.
 *
 * Out of scope: nbits != 8, fast-scan 4-bit codes, OPQ, polysemous
 * and symmetric (SDC) search, selectors, remove_ids, range_search, IndexIDMap
 * over it, write_index / read_index, sharding and the search graph. */
typedef struct FxPq FxPq;
int fx_pq_create(int d, int M, int nbits, int metric, int device, FxPq** out);
void fx_pq_free(FxPq* pq);
int fx_pq_is_trained(const FxPq* pq, int* out);
/* out / centroids: host [M][256][dsub] floats.  Setting them (an index without
 * rows only) rebuilds the scan image and marks the index trained. */
int fx_pq_get_centroids(FxPq* pq, float* out);
int fx_pq_set_centroids(FxPq* pq, const float* centroids);
/* Ids are the row numbers ntotal .. ntotal + n - 1.  Device x is stream-ordered;
 * host x blocks. */
int fx_pq_add(FxPq* pq, int64_t n, const void* x, int x_dtype, int x_mem);
/* Host results block; device queries and results are stream-ordered. */
int fx_pq_search(FxPq* pq, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem);
/* Empties the index, keeps the centroids. */
int fx_pq_reset(FxPq* pq);
int fx_pq_ntotal(const FxPq* pq, int64_t* out);
/* out [n][d] fp32 (out_mem) <- the decoded rows [i0, i0 + n) / the rows keys[i]
 * (int64, keys_mem; a key outside [0, ntotal): a row of NaN, as the flat index). */
int fx_pq_reconstruct_n(FxPq* pq, int64_t i0, int64_t n, float* out, int out_mem);
int fx_pq_reconstruct_batch(FxPq* pq, int64_t n, const int64_t* keys, int keys_mem, float* out, int out_mem);
/* sa_encode / sa_decode: x [n][d] (x_dtype) <-> codes [n][M], all three buffers
 * in `mem`. */
int fx_pq_encode(FxPq* pq, int64_t n, const void* x, int x_dtype, uint8_t* codes, int mem);
int fx_pq_decode(FxPq* pq, int64_t n, const uint8_t* codes, float* out, int mem);
/* out [n][M] (out_mem) <- the codes of the rows [i0, i0 + n). */
int fx_pq_get_codes(FxPq* pq, int64_t i0, int64_t n, uint8_t* out, int out_mem);
int fx_pq_set_stream(FxPq* pq, void* stream);
/* As fx_sq_last_counts / fx_sq_last_plan / fx_sq_profile / fx_sq_profile_read. */
int fx_pq_last_counts(FxPq* pq, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped);
int fx_pq_last_plan(FxPq* pq, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid);
int fx_pq_profile(FxPq* pq, int enable);
int fx_pq_profile_read(FxPq* pq, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes);

/* ---- inverted file over 8-bit codes: faiss IndexIVFScalarQuantizer ------------
 *
 *   faiss (Python)                               faiss C++ / C API                          this ABI
 *   IndexIVFScalarQuantizer(quantizer, d, nlist, faiss_IndexIVFScalarQuantizer_new_with_    fx_ivfsq_create
 *       qtype, metric, by_residual)                  metric
 *   index.train(x)                               faiss_Index_train                          the k-means calls above and fx_index_add
 *                                                                                           on the quantizer, then fx_ivfsq_train
 *   index.is_trained                             faiss_Index_is_trained                     fx_ivfsq_is_trained (and the quantizer's rows)
 *   index.sq.trained                             ScalarQuantizer::trained                   fx_ivfsq_get_trained / _set_trained
 *   index.add(x) / add_with_ids(x, ids)          faiss_Index_add / _add_with_ids            fx_ivfsq_add
 *   index.nprobe; index.search(x, k)             faiss_IndexIVF_set_nprobe / _Index_search  fx_ivfsq_search
 *   index.reset()                                faiss_Index_reset                          fx_ivfsq_reset
 *   index.ntotal                                 faiss_Index_ntotal                         fx_ivfsq_ntotal
 *   invlists.list_size(l) / get_ids(l)           faiss_IndexIVF_get_list_size / ..get_ids   fx_ivfsq_list_sizes / _list_ids
 *   invlists.get_codes(l)                        InvertedLists::get_codes                   fx_ivfsq_list_codes
 *   (GC of the index)                            faiss_Index_free                           fx_ivfsq_free
 *
 * Like the two sections it joins ("inverted file", "scalar quantizer"), this
 * restates faiss from memory and is NOT checked against a faiss build.  One
 * difference is known and deliberate: faiss ranks a row of list l by
 * |fl(x - c_l) - decode(code)|^2 (the distance between residuals), while this
 * contract ranks by the decoded row that reconstruct would return, below.
 *
 * Lists.  The quantizer is a borrowed unlabelled flat index; a row's list is its
 * exact k = 1 search; rows are kept in list order and regrouped by the next
 * search (or list accessor) after an add; ids are sequential or the caller's
 * int64; the probe set of a query is quantizer.search(q, min(nprobe, nlist)):
 * all as the "inverted file" section says.
 *
 * Encoding.  qtype is 0 QT_8bit or 2 QT_8bit_uniform.  With by_residual != 0
 * (faiss's default) the encoded vector of a row of list l is r = fl32(x - c_l),
 * one rounded fp32 subtraction per dimension against the fp32 centroid the
 * quantizer reconstructs (as it was when the tables were trained); otherwise r =
 * x.  The code is the "scalar quantizer" section's encode(r), bitwise.  The
 * tables [vmin | vdiff] are one min / max pass over the r of the training rows.
 *
 * Decoded row.  y = fl32(c_l + decode(code)), or decode(code) without
 * by_residual: every operation rounded once, no FMA contraction, so a numpy fp32
 * expression gives the same bits.
 *
 * Search.  Per query the k rows of its probed lists that minimise sum (x_j -
 * y_j)^2 (L2) or maximise sum x_j y_j (IP) over the decoded fp32 y, the sum in
 * fp64 rounded once to fp32, ranked by (that value, list number, insertion order
 * within the list); missing slots I = -1, D = +-FLT_MAX.  k <= 32: the fused path
 * (operand preparation per (query, probe) pair, the int8 MFMA list scan, exact
 * refine + certification, the exact list scan for uncertified queries, all
 * decided on the device); 32 < k <= FX_MAX_K: the exact list scan (one fp64 pass
 * over the decoded rows of the probed lists: correct, slow; the limitation of
 * both parent sections as k nears 32 holds here too).
 *
 * Errors: those of fx_ivf_* and fx_sq_*, with the same limits.  FX_E_ARG also for
 * training or set_trained while the quantizer does not hold nlist centroids or
 * the index holds rows, and for add or search before the tables are trained.
 *
 * Out of scope: write_index / read_index (faiss's "IwSQ" layout cannot be checked
 * here), remove_ids, range_search, selectors, reconstruct* by id, sharding, the
 * search graph, the other qtypes. */
typedef struct FxIvfSq FxIvfSq;
int fx_ivfsq_create(FxIndex* quantizer, int d, int64_t nlist, int qtype, int metric, int by_residual, FxIvfSq** out);
void fx_ivfsq_free(FxIvfSq* ivfsq);
/* Assigns x [n][d] to lists, forms r, and feeds the min / max pass (bitwise
 * reproducible).  more != 0: the call only accumulates and the index stays
 * untrained; the call with more == 0 finishes (fx_sq_train's protocol). */
int fx_ivfsq_train(FxIvfSq* ivfsq, int64_t n, const void* x, int x_dtype, int x_mem, int more);
int fx_ivfsq_is_trained(const FxIvfSq* ivfsq, int* out);
/* out / trained: host [2 d] floats, [vmin | vdiff]. */
int fx_ivfsq_get_trained(FxIvfSq* ivfsq, float* out);
int fx_ivfsq_set_trained(FxIvfSq* ivfsq, const float* trained);
/* ids NULL: sequential ids ntotal .. ntotal + n - 1.  Device x (and ids) is
 * stream-ordered; host x blocks. */
int fx_ivfsq_add(FxIvfSq* ivfsq, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem);
/* Host results block; device queries and results are stream-ordered (the first
 * search after an add synchronises once for the regroup). */
int fx_ivfsq_search(FxIvfSq* ivfsq, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D,
                    int64_t* I, int out_mem);
/* Empties the lists; the quantizer and the tables (both trainings) stay. */
int fx_ivfsq_reset(FxIvfSq* ivfsq);
int fx_ivfsq_ntotal(const FxIvfSq* ivfsq, int64_t* out);
/* out: host [nlist]. */
int fx_ivfsq_list_sizes(FxIvfSq* ivfsq, int64_t* out);
/* *n = rows of `list`; out (host, cap entries; may be NULL with cap 0) receives
 * the first min(*n, cap) ids / code rows in insertion order.  Codes are faiss's
 * unsigned bytes [.][d]. */
int fx_ivfsq_list_ids(FxIvfSq* ivfsq, int64_t list, int64_t* out, int64_t cap, int64_t* n);
int fx_ivfsq_list_codes(FxIvfSq* ivfsq, int64_t list, uint8_t* out, int64_t cap, int64_t* n);
int fx_ivfsq_set_stream(FxIvfSq* ivfsq, void* stream);
/* As fx_ivf_last_counts / _last_plan / _profile / _profile_read (pairs_ms: the
 * pair grouping and the per-pair operand preparation). */
int fx_ivfsq_last_counts(FxIvfSq* ivfsq, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped);
int fx_ivfsq_last_plan(FxIvfSq* ivfsq, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid);
int fx_ivfsq_profile(FxIvfSq* ivfsq, int enable);
int fx_ivfsq_profile_read(FxIvfSq* ivfsq, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                          int64_t* passes);

/* ---- inverted file over product-quantized codes: faiss IndexIVFPQ (8-bit) ------
 *
 *   faiss (Python)                               faiss C++ / C API                          this ABI
 *   IndexIVFPQ(quantizer, d, nlist, M, nbits,    faiss_IndexIVFPQ_new_with_metric           fx_ivfpq_create
 *       metric); index.by_residual
 *   index.train(x)                               faiss_Index_train                          the k-means calls above and fx_index_add
 *                                                                                           on the quantizer, fx_ivfpq_residuals, M
 *                                                                                           k-means runs, fx_ivfpq_set_centroids
 *   index.is_trained                             faiss_Index_is_trained                     fx_ivfpq_is_trained (and the quantizer's rows)
 *   index.pq.centroids                           ProductQuantizer::centroids                fx_ivfpq_get_centroids / _set_centroids
 *   quantizer.compute_residual_n                 Index::compute_residual_n                  fx_ivfpq_residuals
 *   index.add(x) / add_with_ids(x, ids)          faiss_Index_add / _add_with_ids            fx_ivfpq_add
 *   index.nprobe; index.search(x, k)             faiss_IndexIVF_set_nprobe / _Index_search  fx_ivfpq_search
 *   index.reset()                                faiss_Index_reset                          fx_ivfpq_reset
 *   index.ntotal                                 faiss_Index_ntotal                         fx_ivfpq_ntotal
 *   invlists.list_size(l) / get_ids(l)           faiss_IndexIVF_get_list_size / ..get_ids   fx_ivfpq_list_sizes / _list_ids
 *   invlists.get_codes(l)                        InvertedLists::get_codes                   fx_ivfpq_list_codes
 *   (GC of the index)                            faiss_Index_free                           fx_ivfpq_free
 *
 * Like the sections it joins ("inverted file", "product quantizer"), this
 * restates faiss from memory and is NOT checked against a faiss build.  The
 * deliberate difference the section above names holds here too: faiss ranks a
 * row of list l by the distance between the query's residual and the decoded
 * residual (through its distance tables), this contract by the decoded row.
 *
 * Lists.  The quantizer, a row's list, the regroup after an add, the ids
 * (sequential or the caller's int64, never mixed), the probe set
 * quantizer.search(q, min(nprobe, nlist)) and the missing slots I = -1, D =
 * +-FLT_MAX: all exactly as the "inverted file" section says.
 *
 * Encoded vector.  With by_residual != 0 (faiss's default) the encoded vector of
 * a row of list l is r = fl32(x - c_l), one rounded fp32 subtraction per
 * dimension against the fp32 centroid the quantizer reconstructs (as it was when
 * the codebook was set); otherwise r = x.  The code is the "product quantizer"
 * section's encode(r), bitwise: fp64 argmin, dimensions ascending, no
 * contraction, the lowest j on a tie.
 *
 * Decoded row.  y = fl32(c_l + decode(code)), or decode(code) without
 * by_residual: the gather is bitwise and the addition is rounded once.
 *
 * Search.  Per query the k rows of its probed lists that minimise sum (x_j -
 * y_j)^2 (L2) or maximise sum x_j y_j (IP) over the decoded fp32 y, the sum in
 * fp64 rounded once to fp32, ranked by (that value, list number, insertion order
 * within the list).  k <= 32 and dsub % 8 == 0: the fused path (operand
 * preparation per (query, probe) pair, the gather list scan on the bf16 MFMA,
 * exact refine + certification, the exact list scan for uncertified queries, all
 * decided on the device).  32 < k <= FX_MAX_K, and every index whose dsub is no
 * multiple of 8: the exact list scan for the whole search (one fp64 pass over the
 * decoded rows of the probed lists: correct, slow).  fx_ivfpq_last_plan reports
 * which path ran.
 *
 * Errors: those of fx_ivf_* and fx_pq_*, with the same limits.  FX_E_ARG also for
 * set_centroids while the quantizer does not hold nlist centroids or the index
 * holds rows, and for add or search before the codebook is set;
 * FX_E_UNSUPPORTED for nbits != 8.
 *
 * Out of scope: precomputed tables, polysemous search, nbits != 8, OPQ, fast-scan,
 * write_index / read_index, remove_ids, range_search, selectors, reconstruct* by
 * id, sharding, the search graph. */
typedef struct FxIvfPq FxIvfPq;
int fx_ivfpq_create(FxIndex* quantizer, int d, int64_t nlist, int M, int nbits, int metric, int by_residual,
                    FxIvfPq** out);
void fx_ivfpq_free(FxIvfPq* ivfpq);
int fx_ivfpq_is_trained(const FxIvfPq* ivfpq, int* out);
/* out / centroids: host [M][256][dsub] floats.  Setting them (a trained
 * quantizer, an index without rows) reads the quantizer's centroids, rebuilds
 * the scan image and marks the index trained. */
int fx_ivfpq_get_centroids(FxIvfPq* ivfpq, float* out);
int fx_ivfpq_set_centroids(FxIvfPq* ivfpq, const float* centroids);
/* faiss's compute_residual_n: out [n][d] fp32 (out_mem) <- fl32(x_i - c_l), l the
 * list of row i (the quantizer's k = 1 search); a copy of x widened to fp32
 * without by_residual.  What the codebook is trained on. */
int fx_ivfpq_residuals(FxIvfPq* ivfpq, int64_t n, const void* x, int x_dtype, int x_mem, float* out, int out_mem);
/* ids NULL: sequential ids ntotal .. ntotal + n - 1.  Device x (and ids) is
 * stream-ordered; host x blocks. */
int fx_ivfpq_add(FxIvfPq* ivfpq, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem);
/* Host results block; device queries and results are stream-ordered (the first
 * search after an add synchronises once for the regroup). */
int fx_ivfpq_search(FxIvfPq* ivfpq, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D,
                    int64_t* I, int out_mem);
/* Empties the lists; the quantizer and the codebook stay. */
int fx_ivfpq_reset(FxIvfPq* ivfpq);
int fx_ivfpq_ntotal(const FxIvfPq* ivfpq, int64_t* out);
/* out: host [nlist]. */
int fx_ivfpq_list_sizes(FxIvfPq* ivfpq, int64_t* out);
/* *n = rows of `list`; out (host, cap entries; may be NULL with cap 0) receives
 * the first min(*n, cap) ids / code rows in insertion order.  Codes are faiss's
 * [.][M] uint8. */
int fx_ivfpq_list_ids(FxIvfPq* ivfpq, int64_t list, int64_t* out, int64_t cap, int64_t* n);
int fx_ivfpq_list_codes(FxIvfPq* ivfpq, int64_t list, uint8_t* out, int64_t cap, int64_t* n);
int fx_ivfpq_set_stream(FxIvfPq* ivfpq, void* stream);
/* As fx_ivfsq_last_counts / _last_plan / _profile / _profile_read. */
int fx_ivfpq_last_counts(FxIvfPq* ivfpq, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped);
int fx_ivfpq_last_plan(FxIvfPq* ivfpq, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid);
int fx_ivfpq_profile(FxIvfPq* ivfpq, int enable);
int fx_ivfpq_profile_read(FxIvfPq* ivfpq, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                          int64_t* passes);

/* faiss.write_index / faiss.read_index on the IxF2 format (faiss_store.py:
 * 91,106): fourcc "IxF2", i32 d, i64 ntotal, i64 1<<20, i64 1<<20,
 * u8 is_trained, i32 metric, i64 ntotal*d, f32 codes.  A labelled index is
 * written as "IxM2" around that file, and read back labelled ("stable ids"
 * above). */
int fx_index_write(FxIndex* index, const char* path);
int fx_index_read(const char* path, int storage_dtype, int device, FxIndex** out);

/* ---- row-sharded multi-GPU support (one process per GPU) --------------- */

/* Merge G per-shard result lists (device pointers, layout [G][nq][k], global
 * ids, each list ordered) into D_out/I_out [nq][k] under the index order
 * (L2: ascending; IP: descending; ties -> smaller id).  `stream` may be NULL.
 * k > FX_MAX_K merges at most 64 shards (FX_E_UNSUPPORTED beyond). */
int fx_merge_shards(int metric, int nshards, int64_t nq, int k, const float* D_in,
                    const int64_t* I_in, float* D_out, int64_t* I_out, int device, void* stream);

/* ---- synthetic corpora (bench / tests) -------------------------------- */

/* out[r][c] for rows [row0, row0+n) of the counter-based generator shared
 * with oracle/flat_l2.c (exact in fp32/bf16/fp16).  Device memory. */
int fx_synth_fill(void* out, int64_t row0, int64_t n, int d, int dtype, uint64_t seed,
                  int device, void* stream);

/* ---- kernel timing for the roofline report ---------------------------- */

/* When enabled, every search records HIP events around its scan kernel
 * (on the stream it is launched on).  _read synchronises and returns the
 * summed scan-kernel milliseconds and the number of launches since reset. */
int fx_index_profile(FxIndex* index, int enable);
int fx_index_profile_read(FxIndex* index, double* scan_ms, double* merge_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* FX_INDEX_H */
