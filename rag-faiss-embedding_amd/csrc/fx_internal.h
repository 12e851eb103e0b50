// fx_internal.h -- shared between the HIP translation units (fx_kernels.hip,
// fx_scan.hip, fx_scan5.hip, fx_hugek.hip, fx_range.hip, fx_select.hip, fx_remove.hip, fx_idmap.hip, fx_recon.hip, fx_kmeans.hip, fx_ivf.hip, fx_sq.hip, fx_ivfsq.hip, fx_pq.hip, fx_ivfpq.hip) and the host C ABI
// (fx_index.cpp, fx_api_*.cpp, fx_plan.cpp; their own header: fx_host.h):
// tiling constants, kernel parameter blocks, the launchers' prototypes and
// their host-side helpers.  Not part of the public ABI (include/fx_index.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace fx {

// ---- tiling of the fused scan kernel (see DESIGN.md "scan kernel") --------
constexpr int TILE_R = 128;   // corpus rows per tile (MFMA M side)
constexpr int TILE_Q = 128;   // queries per tile      (MFMA N side)
constexpr int STAGE_B = 128;  // bytes of each row's K staged per pipeline stage
constexpr int KP = 32;        // candidates kept per (query, corpus split)
constexpr int FX_BIG_K = 1024;  // largest k of the scan path (k > KP: k_refine_big; == FX_MAX_K of the
                                // ABI); larger k: fx_hugek.hip
constexpr int CAP = 64;       // LDS candidate-list capacity per query (2*KP)
constexpr int ROW_ALIGN = 128;  // row stride alignment in bytes (== STAGE_B)
constexpr int SCAN_THREADS = 256;

// dynamic LDS carve of the scan kernel (all in ONE extern array: see
// cdna_hip_programming.md 5.4 item 4(a))
constexpr int LDS_STAGE = 2 * (TILE_R + TILE_Q) * STAGE_B;   // 64 KiB double buffer
constexpr int LDS_NORM_OFF = LDS_STAGE;                       // 2 x 512 B row norms
constexpr int LDS_LD_OFF = LDS_NORM_OFF + 2 * TILE_R * 4;    // lst_d [TILE_Q][CAP] f32
constexpr int LDS_LI_OFF = LDS_LD_OFF + TILE_Q * CAP * 4;    // lst_i [TILE_Q][CAP] i32
constexpr int LDS_CNT_OFF = LDS_LI_OFF + TILE_Q * CAP * 4;   // cnt   [TILE_Q] i32
constexpr int LDS_TAU_OFF = LDS_CNT_OFF + TILE_Q * 4;        // tau   [TILE_Q] f32
constexpr int LDS_FLAG_OFF = LDS_TAU_OFF + TILE_Q * 4;       // overflow flag (16 B)
constexpr int LDS_SCAN_BYTES = LDS_FLAG_OFF + 16;

enum Dtype { F32 = 0, BF16 = 1, F16 = 2,
             // scan-only operand format of an fp32 index (FX_F32_SPLIT=1): every
             // value v as bf16 hi = rn(v) and lo = rn(v - hi), rows laid out
             // [hi plane | lo plane] in the fp32 row's bytes; the scan sums
             // hi*hi + hi*lo + lo*hi with bf16 MFMAs (never a storage dtype)
             F32S = 3 };
enum Metric { IP = 0, L2 = 1 };

inline int dtype_size(int dt) { return dt == F32 ? 4 : 2; }

struct ScanParams {
    const char* codes;     // [cap_rows][row_bytes] storage dtype, zero padded
    const float* norms;    // [cap_rows] |y|^2 (fp32, of stored values)
    int64_t ntotal;
    int row_bytes;
    const char* qop;       // [nq_pad][row_bytes] queries in storage dtype
    int64_t nq;
    int n_qtiles;
    int n_ctiles;          // corpus tiles (ceil(ntotal / TILE_R))
    int splits;            // corpus splits per query tile
    int qt_per_xcd;        // query tiles assigned per XCD group
    float* cand_d;         // [n_qtiles][splits][TILE_Q][KP]
    int* cand_i;
    int dbg;               // ablation switches (FX_SCAN_DBG; 0 in production)
    unsigned* gtau;        // [n_qtiles * TILE_Q] order-preserving bits of the best
                           // known KP-th key per query across splits (atomicMin)
    unsigned long long* trace;  // diagnostics only (FX_SCAN_TRACE): per block
                                // {xcc | hw_id << 8 | qtile << 32, split, t_start, t_end}
    unsigned* dbgbuf;           // diagnostics only (FX_SCAN_DBG & 32): operand self-check
    int share;                  // 1: splits publish their KP-th key to gtau and prune with it
                                // (k <= KP); 0: no cross-split pruning (k > KP, k_refine_big)
    int place;                  // block placement (map_tile): 0 query-tile groups per XCD, 1
                                // corpus-partitioned (XCD x owns splits [x sx, (x+1) sx))
    int sx;                     // place 1: corpus splits per XCD (splits = 8 sx)
    int grid;                   // workgroups of the scan launch
    int prune_rank;             // rank of the union bound published to gtau (compact_wave)
    int union_w;                // union bound window: 16, 32 or 64 splits (their first 256 / union_w keys)
    int compact_at;             // a list is compacted once it holds this many entries (KP < v <= CAP;
                                // the threshold only improves at a compaction)
    float* pub;                 // k_scan_v4 with share: [n_qtiles * TILE_Q][splits][KP] each split's
                                // last compacted top-KP keys per query (null: not used)
    unsigned long long* stamps; // diagnostics only (FX_SCAN_STAMPS, -DFX_ABLATION builds):
                                // [grid][4 waves][16] per-wave cycle sums of the scan's phases
    const int* nq_dev;          // non-null (the re-scan of uncertified queries): the live query
                                // count is min(*nq_dev, nq), known only on the device
    int union_defer;            // 1: a compaction's union bound is fetched by LDS-DMA and bounded at
                                // the next tile's epilogue (compact_regs); 0: waited for in place
    int tight_at;               // > 0: a list that took entries in a tile and holds >= tight_at (below
                                // the compaction trigger) gets its threshold re-bounded (tighten_list)
    int union_inplace;          // most lists per compaction call bounded in place by the union (those
                                // past the deferred slots); the rest publish only their own bound
    int cold_bound;             // 1: a still-empty list's first record tile bounds its threshold by the
                                // prune_rank-th of the tile's group minima before pushing
    int qt;                     // queries per scan tile (the candidate layout's [qtile][split][qt][KP]):
                                // TILE_Q (k_scan_v4 / k_scan_topk) or 256 (k_scan_v5)
    int tr;                     // corpus rows per scan tile: TILE_R, or 64 (k_scan_v5)
    unsigned* conv;             // convoy words of k_scan_v4 / v5, one line per split (null: every block starts at its
                                // split's first tile): blocks publish the split-relative tile they scan,
                                // and a starting block begins there (circularly), so blocks of one split
                                // read the same rows at the same time whenever they started
    int conv_every;             // publish every conv_every tiles (power of 2)
};
// convoy splits per index (splits above this scan without them); one 64-B
// line (16 words) per split
constexpr int CONV_MAX = 4096;
constexpr int CONV_WORDS = CONV_MAX * 16;

// queries are zero-padded to a multiple of QPAD (the scan's query tile)
constexpr int QPAD = TILE_Q;

struct RefineParams {
    const float* cand_d;   // scan output (approx keys)
    const int* cand_i;
    int splits;
    int64_t nq;
    int k;
    const char* codes;
    int row_bytes;
    int kdim;
    const float* qf32;     // [nq_pad][kdim] fp32 queries, zero padded
    const float* qeps;     // [nq] E: query-wide bound on |approx key + shift - exact|
    const float* qrho;     // [nq] rho = |x - mu - x_op| (the scan operand's rounding): the bound adds
                           // 2 rho sqrt(D) for a row at exact distance D (L2, 16-bit / fp32 rows)
    const double* qshift;  // [nq] s_q: approx key + s_q estimates the exact distance
    int64_t id_offset;
    const int64_t* labels; // non-null (a labelled index, fx_idmap.hip): I = labels[row]; null: row + id_offset
    float* D;              // [nq][k]
    int64_t* I;
    int* n_flag;           // uncertified counter
    int* flag_list;        // [nq] uncertified query ids
    int prefetch;          // > 1: phase-1 loads issued 4 chunks at a time (small-batch scan)
    int k1;                // k > KP: approx candidates re-ranked exactly (2k, <= 2 FX_BIG_K)
    int force_fb;          // test hook (FX_FORCE_FALLBACK=1): flag every query -> exact fallback
    const unsigned* gtau;  // k <= KP: the scan's final shared thresholds (ordered bits): every row a split
                           // dropped lies above it, so it caps the certification bound; null: unused
    const int* nq_dev;     // non-null: live query count min(*nq_dev, nq) (the re-scan)
    const int* out_idx;    // non-null: query q's results go to row out_idx[q] of D / I, and an
                           // uncertified q is flagged as out_idx[q] (the re-scan's gathered queries)
    int64_t ntotal;        // rows of the index: a candidate row id outside [0, ntotal) is never gathered
    int* n_drop;           // ... and counted here (ids other than -1 outside [0, ntotal): a corrupted
                           // candidate list), read back by fx_index_last_dropped_candidates
    int qt;                // queries per scan tile of the candidate layout (ScanParams.qt)
    int wg;                // > 0: small batches over many splits (k <= KP): one workgroup of wg (4, 8, 16) waves per query
                           // (k_refine_wg: the waves share the walk over splits * KP candidates); 0: k_refine
};
// waves of k_refine_wg's workgroup (one query per workgroup) unless the
// index's option refine_waves says otherwise (4, 8 or 16)
constexpr int REFINE_WG_WAVES = 16;

// exact fallback (k_fb_scan / k_fb_merge): corpus splits per flagged query,
// decided on the device from the flagged count nf; items nf * fbs <=
// max(4096, nf), so the candidate buffer is max(4096, nq) * k entries
constexpr int FB_SCAN_GRID = 1024, FB_MERGE_GRID = 256;
__host__ __device__ inline int fb_splits_for(int nf, int64_t ntotal) {
    int s = nf >= 4096 ? 1 : 4096 / (nf > 0 ? nf : 1);
    if (s > 256) s = 256;
    const int64_t by_rows = ntotal / 1024 > 0 ? ntotal / 1024 : 1;
    if (s > by_rows) s = (int)by_rows;
    return s < 1 ? 1 : s;
}

// the re-scan of uncertified queries takes them in chunks of at most this
// many (its workspace is sized for one chunk)
constexpr int64_t RESCAN_MAX = 2048;
// counts[c] = live queries of re-scan chunk c: the flagged queries
// [c cap, min(n_flag[0], (c+1) cap)); device-gated like the fallbacks
hipError_t launch_rescan_chunks(const int* n_flag, int cap, int nchunks, int* counts, hipStream_t s);

// True on a thread that is capturing a search into a hipGraph (fx_api_search.cpp
// graph_build): the scan launchers then skip hipFuncSetAttribute, which the
// do_search right before the capture has already applied for the same kernel.
extern thread_local bool g_graph_capture;

// Launch of a kernel with more than 64 KiB of dynamic LDS: the opt-in (per
// device; cheap to repeat; skipped while capturing, see above), the launch,
// its error.
template <class... P, class... A>
hipError_t launch_with_lds(void (*kernel)(P...), int grid, int block, int lds_bytes, hipStream_t s, const A&... args) {
    if (!g_graph_capture) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, s, args...);
    return hipGetLastError();
}

// (dtype, metric) as compile-time constants: f(integral_constant<int, DT>,
// integral_constant<int, METRIC>) -> hipError_t for the run-time pair, with f
// instantiated for the dtypes of ALLOWED only.  A dtype outside ALLOWED is
// hipErrorInvalidValue (every caller has validated it by then: the storage
// dtype at fx_index_create, the scan dtype by image_kind); a metric other than
// L2 is IP.
constexpr unsigned DT_16BIT = 1u << BF16 | 1u << F16;  // k_scan_v5, the centred norms
constexpr unsigned DT_STORED = DT_16BIT | 1u << F32;   // what an index stores
constexpr unsigned DT_SCAN = DT_STORED | 1u << F32S;   // ... and what k_scan_v4 also reads
template <unsigned ALLOWED, int DT, int METRIC, class F>
hipError_t dispatch_one(F&& f) {
    if constexpr ((ALLOWED >> DT & 1u) != 0)
        return f(std::integral_constant<int, DT>{}, std::integral_constant<int, METRIC>{});
    else
        return hipErrorInvalidValue;
}
template <unsigned ALLOWED, class F>
hipError_t dispatch_dt_metric(int dt, int metric, F&& f) {
    // The order of these branches is the order in which f is instantiated, and so
    // the order in which a translation unit's kernels are emitted: F32S first, then
    // metric-major.  Keep it: comparing the device assembly of fx_scan.hip and
    // fx_scan5.hip with an earlier commit's (the check that a change did not
    // reach the hot kernels) relies on the kernels keeping their places.
    if (dt == F32S) return metric == L2 ? dispatch_one<ALLOWED, F32S, L2>(f) : dispatch_one<ALLOWED, F32S, IP>(f);
    if (metric == L2) {
        if (dt == F32) return dispatch_one<ALLOWED, F32, L2>(f);
        if (dt == BF16) return dispatch_one<ALLOWED, BF16, L2>(f);
        if (dt == F16) return dispatch_one<ALLOWED, F16, L2>(f);
    } else {
        if (dt == F32) return dispatch_one<ALLOWED, F32, IP>(f);
        if (dt == BF16) return dispatch_one<ALLOWED, BF16, IP>(f);
        if (dt == F16) return dispatch_one<ALLOWED, F16, IP>(f);
    }
    return hipErrorInvalidValue;
}

// launchers (stream-ordered, no host sync) -- fx_kernels.hip
hipError_t launch_convert_rows(const void* x, int x_dt, int64_t n, int d, void* codes_row0, int st_dt,
                               int kdim, float* norms_row0, unsigned* max_sq_bits, int normalize,
                               hipStream_t s);
// search(): query preparation (k_prep_queries): fp32 copy for the exact
// refine, the scan operand, and the per-query certification terms
struct PrepParams {
    const void* q;          // [nq][d] caller queries, dtype q_dt, on the device
    int q_dt;
    int64_t nq, nq_pad;
    int d, kdim;
    int st_dt;              // scan dtype (F32, BF16, F16, F32S)
    int metric;
    float* qf32;            // [nq_pad][kdim] fp32 queries, zero padded
    void* qop;              // [nq_pad][row_bytes] scan operand (x - mu in the scan dtype, pre-scaled)
    float* qeps;            // [nq] E
    float* qrho;            // [nq] rho
    double* qshift;         // [nq] s_q
    const unsigned* mbits;     // max |y|^2 of the stored rows (float bits)
    const unsigned* img_bits;  // max srcC of the scan image (= mbits without an image)
    const float* mu;        // centre of the scan image (null: none)
    const int* qidx;        // non-null: row r of the batch is row qidx[r] of q (the re-scan's gather)
    const int* nq_dev;      // non-null: live query count min(*nq_dev, nq); later rows are padding
    // the search's resets, folded into this first kernel instead of memsets:
    unsigned* gtau;         // non-null: [nq_pad] the scan's shared thresholds, set to ord(+inf)
    int* zero[3];           // non-null entries: counters set to 0 (dropped ids, flagged, exact)
    float* pub;             // non-null: the scan's published lists, npub floats set to +inf
    int64_t npub;
};
hipError_t launch_prep_queries(const PrepParams& p, hipStream_t s);
hipError_t launch_scan(int st_dt, int metric, const ScanParams& p, hipStream_t s);
// fx_scan.hip: the MFMA scan; *handled = false when it has no kernel for p.row_bytes
hipError_t launch_scan_mfma(int st_dt, int metric, const ScanParams& p, hipStream_t s, bool* handled);
hipError_t launch_refine(int st_dt, int metric, const RefineParams& p, hipStream_t s);
// small batches: merge each 16 splits' candidate lists of a query into their
// top KP (k_reduce_cand); *ngroups = ceil(splits / 16) lists per query after
hipError_t launch_reduce_cand(const float* cd, const int* ci, int splits, int64_t nq, int qt, float* od,
                              int* oi, int* ngroups, int64_t ntotal, int* n_drop, hipStream_t s);
// fx_scan5.hip: the 64-row-tile, 256-query scan (k_scan_v5) and the shapes it has
int scan_v5_qt(int st_dt, int row_bytes);  // its queries per workgroup for these rows (0: no shape)
hipError_t launch_scan_v5(int st_dt, int metric, const ScanParams& p, hipStream_t s);
constexpr int V5_TR = 64;
// both fallback launches, always enqueued; they read the flagged count at
// n_flag[0] (list at n_flag + 1) and do nothing when it is 0.  row_mask
// non-null (a filtered search): only rows whose mask bit is set are ranked
hipError_t launch_exact_fallback(int st_dt, int metric, const char* codes, int row_bytes, int kdim,
                                 int64_t ntotal, const float* qf32, const int* n_flag, int k,
                                 int64_t id_offset, float* cand_d, int* cand_i, float* D, int64_t* I,
                                 hipStream_t s, const uint32_t* row_mask = nullptr,
                                 const int64_t* labels = nullptr);
hipError_t launch_merge_shards(int metric, int nshards, int64_t nq, int k, const float* D_in,
                               const int64_t* I_in, float* D_out, int64_t* I_out, hipStream_t s);
// k > FX_BIG_K (fx_hugek.hip): exact key of every (query, row) pair, a radix
// sort per query, the first k -> D / I (faiss padding past ntotal)
struct HugeKParams {
    const char* codes;     // [ntotal][row_bytes] stored rows (storage dtype st_dt)
    int row_bytes, kdim, d, st_dt, metric;
    int64_t ntotal;
    const void* q;         // [nq][d] queries on the device, dtype q_dt
    int q_dt;
    int64_t nq;
    int k;
    int64_t id_offset;
    const int64_t* labels; // non-null: I = labels[row] (null: row + id_offset)
    float* D;              // [nq][k] on the device
    int64_t* I;
};
// queries per batch, and the workspace bytes a batch of qb queries needs
int hugek_batch(int64_t ntotal, int64_t nq);
hipError_t hugek_workspace(int64_t ntotal, int kdim, int qb, size_t* bytes);
hipError_t launch_hugek_search(const HugeKParams& p, void* ws, size_t ws_bytes, int qb, hipStream_t s);
// fx_merge_shards for k > FX_BIG_K: per query, a G-way merge of the gathered
// lists (each in the index order); at most FX_HUGEK_MAX_SHARDS shards
constexpr int FX_HUGEK_MAX_SHARDS = 64;
hipError_t launch_merge_shards_sort(int metric, int nshards, int64_t nq, int k, const float* D_in,
                                    const int64_t* I_in, float* D_out, int64_t* I_out, hipStream_t s);
// range_search (fx_range.hip).  thr[q] = T_q, the largest scan key a row
// within `radius` of query q can have (from k_prep_queries' E, rho, s_q).
hipError_t launch_range_thr(int64_t nq, int metric, float radius, const float* qeps, const float* qrho,
                            const double* qshift, float* thr, hipStream_t s);
// the MFMA filter over the stored rows (p.codes / p.norms = the index's own,
// p.qt = TILE_Q, p.tr = TILE_R, placement fields as map_block reads them):
// every (query, row) pair with key <= thr[query] -> cand[] as query << 32 | row
// at positions reserved from *counter, which counts past `cap` (entries at
// or past cap are not stored).  *counter must be 0 before the launch.
hipError_t launch_range_scan(int st_dt, int metric, const ScanParams& p, const float* thr, uint64_t* cand,
                             uint64_t cap, uint64_t* counter, hipStream_t s);
// exact verification, compaction and unpacking of n candidate words
struct RangeFinish {
    uint64_t* words;       // [n] candidates (overwritten: failing ones -> all ones)
    int64_t n;             // 1 .. INT_MAX
    const char* codes;     // stored rows (storage dtype st_dt)
    int row_bytes, kdim, st_dt, metric;
    int64_t ntotal;
    const float* qf32;     // [nq][kdim] fp32 queries, zero padded
    int64_t nq;
    float radius;
    int64_t id_offset;
    const int64_t* labels; // non-null: I = labels[row] (null: row + id_offset)
    float* dist;           // [n] scratch: exact distance of words[i]
    uint64_t* sorted;      // [n] scratch: words in (query, row) order, sentinels last
    void* temp;            // rocPRIM temporaries (range_sort_temp_bytes)
    size_t temp_bytes;
    int* n_drop;           // words naming a query / row outside the index are counted here, never gathered
    int64_t* lims;         // out [nq + 1]
    float* D;              // out [n]: the first lims[nq] are the results
    int64_t* I;            // out [n]
};
hipError_t range_sort_temp_bytes(int64_t n, int64_t nq, size_t* bytes);
hipError_t launch_range_finish(const RangeFinish& f, hipStream_t s);
// filtered search (fx_select.hip).  A selector's device image: the row mask
// (bit r & 31 of word r >> 5 set: local row r is selected; 4 words per 128-row
// tile, zero past ntotal), the ascending list of the tiles with a selected
// row, and their counts.
struct SelCounts {
    long long rows;  // selected rows
    int tiles;       // live tiles (entries of the tile list)
    int pad;
};
inline int64_t sel_mask_words(int64_t ntotal) { return (ntotal + TILE_R - 1) / TILE_R * (TILE_R / 32); }
// mask builders over rows [0, ntotal) (ids = row + id_offset); invert != 0:
// the complement within those rows.  Each writes every word of the mask.
//   bitmap: id i is a member iff bits[i >> 3] & (1 << (i & 7)), i < 8 nbytes
//   ids:    n int64 ids (duplicates and ids outside the index ignored)
//   range:  local rows [lo, hi), 0 <= lo <= hi <= ntotal
hipError_t launch_sel_bitmap(const uint8_t* bits, int64_t nbytes, int64_t id_offset, int64_t ntotal, int invert,
                             uint32_t* mask, hipStream_t s);
hipError_t launch_sel_ids(const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal, int invert,
                          uint32_t* mask, hipStream_t s);
hipError_t launch_sel_range(int64_t lo, int64_t hi, int64_t ntotal, int invert, uint32_t* mask, hipStream_t s);
// tiles[0, cnt->tiles) <- the tiles of the mask with a set bit, ascending; cnt <- the counts
hipError_t launch_sel_tiles(const uint32_t* mask, int64_t ntotal, int* tiles, SelCounts* cnt, hipStream_t s);
// k_scan_topk over the selector's live tiles and selected rows only (p as
// launch_range_scan's: the stored rows, qt = TILE_Q, tr = TILE_R); the same
// [qtile][split][TILE_Q][KP] candidate lists, every split's written
hipError_t launch_scan_sel(int st_dt, int metric, const ScanParams& p, const uint32_t* mask, const int* tiles,
                           const SelCounts* cnt, hipStream_t s);
// remove_ids (fx_remove.hip): the in-place compaction of codes / norms under a
// selector's row mask (a set bit: the row is REMOVED).
// launch_keep_prefix: prefix[w] = kept rows before mask word w (sel_mask_words
// words), gp[g] = the same at row 1024 g (rm_groups entries), bsum:
// rm_prefix_blocks words of scratch, info[0] = the first removed row
// (0xffffffff: none), info[1] = the kept total.
constexpr int RM_WORDS_PER_BLOCK = 256;  // mask words per workgroup of the prefix kernels
constexpr int64_t RM_GROUP_ROWS = 1024;  // rows per gp entry (32 mask words)
inline int64_t rm_prefix_blocks(int64_t ntotal) {
    return (sel_mask_words(ntotal) + RM_WORDS_PER_BLOCK - 1) / RM_WORDS_PER_BLOCK;
}
inline int64_t rm_groups(int64_t ntotal) { return (sel_mask_words(ntotal) + 31) / 32; }
hipError_t launch_keep_prefix(const uint32_t* mask, int64_t ntotal, unsigned* prefix, unsigned* gp, unsigned* bsum,
                              unsigned* info, hipStream_t s);
// kept rows r of the source rows [s0, s1) (and their norms) -> row prefix(r) -
// dbase of dst_codes / dst_norms.  The caller orders the launches (DESIGN.md
// "row removal"): dst is the index's own arrays only when every destination
// row lies below s0, else a staging buffer.
hipError_t launch_move_rows(const char* codes, const float* norms, const uint32_t* mask, const unsigned* prefix,
                            int64_t ntotal, int row_bytes, int64_t s0, int64_t s1, char* dst_codes, float* dst_norms,
                            int64_t dbase, hipStream_t s);
// stable external ids (fx_idmap.hip): a labelled index carries one int64 label
// per row (FxIndex::labels); these are the label -> row direction.
// Selector masks by label over rows [0, ntotal): a row is selected iff its
// label is a member (invert: the complement within the rows); each writes
// every word of the mask.
//   range:  imin <= label < imax
//   bitmap: (uint64_t)label >> 3 < nbytes and the label's bit set (negative labels: never)
//   ids:    label in ids[0, n) -- ids is sorted on the device first, into
//           ws (idmap_sort_bytes(n, false) bytes), then every row binary-searches it
hipError_t launch_sel_range_lbl(const int64_t* labels, int64_t imin, int64_t imax, int64_t ntotal, int invert,
                                uint32_t* mask, hipStream_t s);
hipError_t launch_sel_bitmap_lbl(const int64_t* labels, const uint8_t* bits, int64_t nbytes, int64_t ntotal,
                                 int invert, uint32_t* mask, hipStream_t s);
hipError_t idmap_sort_bytes(int64_t n, bool pairs, size_t* bytes);
hipError_t launch_sel_ids_lbl(const int64_t* labels, const int64_t* ids, int64_t n, int64_t ntotal, int invert,
                              uint32_t* mask, void* ws, size_t ws_bytes, hipStream_t s);
// rows[i] <- the LAST row whose label is ids[i], -1 when none (n <= INT_MAX;
// ws: idmap_sort_bytes(n, true) bytes): the (id, position) pairs sorted, every
// row's label binary-searched, atomicMax of the row into the id's first sorted
// slot, then the runs' answers scattered back to input order
hipError_t launch_rows_of_labels(const int64_t* labels, int64_t ntotal, const int64_t* ids, int64_t n, int64_t* rows,
                                 void* ws, size_t ws_bytes, hipStream_t s);
// remove_ids: dst[prefix(r)] <- labels[r] for the rows r the mask keeps (a set
// bit: removed), out of place (prefix: launch_keep_prefix's words)
hipError_t launch_compact_labels(const int64_t* labels, const uint32_t* mask, const unsigned* prefix, int64_t ntotal,
                                 int64_t* dst, hipStream_t s);
// stored vectors and exact distances by key (fx_recon.hip).  A key names local
// row key - id_offset; one outside [id_offset, id_offset + ntotal) is checked
// before any address is formed and reads no memory.
// out[i][0..d) <- the stored row keys[i] (keys null: the implicit key key0 + i),
// dense [n][d] of out_dt = F32 (exact widening) or st_dt (byte copy); a key
// naming no row: a row of all-ones bits (NaN)
hipError_t launch_gather_rows(const char* codes, int st_dt, int row_bytes, int64_t ntotal, const int64_t* keys,
                              int64_t key0, int64_t id_offset, int64_t n, int d, void* out, int out_dt,
                              hipStream_t s);
// D[i][j] <- the refine's exact distance of query i (qf32: [nq][kdim] fp32, zero
// padded) and row keys[i][j]; a key naming no row: FLT_MAX (L2) / -FLT_MAX (IP)
hipError_t launch_subset_dist(int st_dt, int metric, const char* codes, int row_bytes, int kdim, int64_t ntotal,
                              const float* qf32, int64_t nq, int k, const int64_t* keys, int64_t id_offset, float* D,
                              hipStream_t s);
// I[i] <- labels[I[i]] for rows 0 <= I[i] < ntotal, else -1
hipError_t launch_label_ids(const int64_t* labels, int64_t ntotal, int64_t n, int64_t* I, hipStream_t s);
// k-means (fx_kmeans.hip): one Lloyd update from (x, assign), bitwise
// reproducible (fp64 sums in a fixed order, no floating-point atomics).
constexpr int KM_M = 128;  // members of a cluster summed by one workgroup of k_km_sum
struct KmUpdate {
    const void* x;          // [n][d] dense rows on the device, dtype x_dt
    int x_dt;
    int64_t n;              // 1 .. 2^31-1 rows (one chunk)
    int d;
    int64_t k;              // clusters, 1 .. 2^31-1
    const int64_t* assign;  // [n] cluster of every row; one outside [0, k) is counted in *bad and skipped
    const float* dist;      // [n] the rows' distances (summed into obj), or null
    double* sums;           // [k][d]
    int64_t* counts;        // [k]
    double* obj;            // one fp64
    int accumulate;         // != 0: add to sums / counts / obj (an earlier chunk's), else overwrite
    unsigned long long* bad;  // device counter of the skipped entries (never reset here)
};
// bytes of the workspace launch_km_update needs for a chunk of n rows
hipError_t km_workspace(int64_t n, int64_t k, int d, size_t* bytes);
// mid non-null: recorded between (keys, sort, segments) and (sum, fold)
hipError_t launch_km_update(const KmUpdate& u, void* ws, size_t ws_bytes, hipStream_t s, hipEvent_t mid = nullptr);
struct KmFinish {
    const double* sums;     // [k][d]
    const int64_t* counts;  // [k]
    int64_t k;
    int d;
    const char* codes;      // the centroid index's stored rows (an empty cluster keeps its row)
    int st_dt, row_bytes;
    int spherical;          // != 0: every centroid L2-normalised
    float* cent;            // out [k][d] fp32
    int64_t* h;             // [k] scratch: the repair's working counts
    int64_t* n_split;       // out: empty clusters repaired
};
hipError_t launch_km_finish(const KmFinish& f, hipStream_t s);
// inverted file (fx_ivf.hip): IndexIVFFlat over a list-ordered payload.
// Regroup: rows [0, n) of (codes, norms, labels, row_list) -> the same rows in
// list order (stable: insertion order within a list) in the dst arrays;
// list_off[l] = first row of list l (list_off[nlist] = rows with a valid list),
// *max_rows = the longest list.  A row_list entry outside [0, nlist) sorts last,
// past list_off[nlist].  ws: ivf_regroup_bytes(n, nlist).
struct IvfRegroup {
    int64_t n, nlist;  // n <= 2^31-1
    int row_bytes;
    const char* codes;
    const float* norms;
    const int64_t* labels;
    const int* row_list;
    char* dst_codes;
    float* dst_norms;
    int64_t* dst_labels;
    int* dst_row_list;
    int* list_off;  // [nlist + 1]
    int* max_rows;  // one word
};
hipError_t ivf_regroup_bytes(int64_t n, int64_t nlist, size_t* bytes);
hipError_t launch_ivf_regroup(const IvfRegroup& r, void* ws, size_t ws_bytes, hipStream_t s);
// row_list[i] = (int)assign[i] for i < n; an assignment outside [0, nlist) is stored as nlist and counted in *bad
hipError_t launch_ivf_record(const int64_t* assign, int64_t n, int64_t nlist, int* row_list, unsigned long long* bad,
                             hipStream_t s);
// ids[i] = first + i
hipError_t launch_ivf_iota(int64_t* ids, int64_t n, int64_t first, hipStream_t s);
// The (query, probed list) pairs of a pass, grouped by list on the device:
// pair p = q * np + j probes list coarse[p]; sorted = the pairs as list << 32 |
// p ordered by list (stable); seg[l] = first sorted position of list l, gbase =
// exclusive scan of ceil(count_l / TILE_Q) over the NON-EMPTY lists (a list
// without rows forms no group), so gbase[nlist] is the pass's group total.  A
// coarse entry outside [0, nlist) forms no pair and is counted in *bad.
struct IvfPairs {
    const int64_t* coarse;  // [npairs]
    int64_t npairs;         // <= 2^31-1
    int64_t nlist;
    const int* list_off;    // [nlist + 1]
    uint64_t* keys;         // [npairs] scratch
    uint64_t* sorted;       // [npairs]
    int* seg;               // [nlist + 1]
    int* ngrp;              // [nlist + 1] scratch
    int* gbase;             // [nlist + 1]
    int* bad;               // one counter (added to)
};
hipError_t ivf_pairs_temp_bytes(int64_t npairs, int64_t nlist, size_t* bytes);
hipError_t launch_ivf_pairs(const IvfPairs& p, void* temp, size_t temp_bytes, hipStream_t s);
// k_ivf_scan: one workgroup per (query group, chunk): the MFMA tile loop over
// the chunk's tiles of the group's list against the group's <= TILE_Q queries,
// fetched through the sorted pairs; the sorted top-KP of (item, query) ->
// cand[q][j * C + chunk][KP].  cand_i must hold -1 wherever no block writes.
struct IvfScan {
    const char* codes;    // the payload in list order
    const float* norms;
    int row_bytes;
    const int* list_off;
    int64_t nlist;
    const char* qop;      // [nq_pad][row_bytes] prepared query operands of the pass
    int np, C;            // probes per query, chunks per list
    const uint64_t* sorted;
    const int* seg;
    const int* gbase;
    float* cand_d;        // [nq][np * C][KP]
    int* cand_i;
    int64_t grid;
};
hipError_t launch_ivf_scan(int st_dt, int metric, const IvfScan& p, hipStream_t s);
// k_ivf_exact + k_ivf_merge: the exact fp64 ranking of the probed lists' rows
// for the queries n_flag[1 ..] (count n_flag[0], read on the device: nothing
// runs when it is 0).  Item (flagged f, probe j, chunk c) -> cd / ci[item][k];
// the merge ranks a query's np * C lists under (key, row) -> D / I.
struct IvfExact {
    const char* codes;
    int row_bytes, kdim;
    const int* list_off;
    int64_t nlist;
    const int64_t* coarse;  // [nq][np]
    int np, C;
    const float* qf32;      // [nq][kdim]
    const int* n_flag;
    int k;
    float* cd;              // [flagged * np * C][k]
    int* ci;
    const int64_t* labels;
    float* D;               // [nq][k]
    int64_t* I;
};
hipError_t launch_ivf_exact(int st_dt, int metric, const IvfExact& p, hipStream_t s);
// k_ivf_merge alone: the per-query merge of cd / ci lists another exact scan wrote (fx_ivfsq.hip)
hipError_t launch_ivf_merge(int metric, const IvfExact& p, hipStream_t s);
// *bad += the entries of coarse[0, n) outside [0, nlist) (the exact path of a whole pass, which forms no pairs)
hipError_t launch_ivf_count_bad(const int64_t* coarse, int64_t n, int64_t nlist, int* bad, hipStream_t s);
// flag[0] = n, flag[1 + i] = i (the exact path of a whole pass)
hipError_t launch_ivf_flag_all(int* flag, int64_t n, hipStream_t s);
// *total += *n_flag
hipError_t launch_ivf_accum(int* total, const int* n_flag, hipStream_t s);
// queries [n][d] (dtype q_dt, on the device) -> fp32 [n][kdim], zero padded (fx_hugek.hip: k_hk_queries)
hipError_t launch_f32_queries(const void* q, int q_dt, int64_t n, int d, int kdim, float* out, hipStream_t s);
// bits[0] <- max(bits[0], float bits of the largest of norms[0, n)) (atomicMax)
hipError_t launch_norm_max(const float* norms, int64_t n, unsigned* bits, hipStream_t s);
// fp32 code rows [r0, r1) -> their F32S scan image (same row stride)
// (centred by mu when non-null), with the image rows' |v|^2 -> cnorms and their
// maximum -> cmax_bits (atomicMax)
hipError_t launch_split_rows(const float* codes, int kdim, int64_t r0, int64_t r1, const float* mu, void* split,
                             float* cnorms, unsigned* cmax_bits, hipStream_t s);
// mu[kdim] <- mean of a strided sample of <= MU_SAMPLE of the n stored rows
// (dtype dt, row stride row_bytes; part: 2 * MU_GROUPS * kdim doubles of
// scratch).  min_ratio > 0: mu is set to 0 when |mu|^2 < min_ratio * the
// sample's mean |y|^2 (no common direction to remove)
constexpr int64_t MU_SAMPLE = 1 << 20;
constexpr int MU_GROUPS = 64;
hipError_t launch_mu(const char* codes, int dt, int row_bytes, int d, int64_t n, double* part, float* mu,
                     float min_ratio, hipStream_t s);
// 16-bit rows [r0, r1) -> cnorms = |y - mu|^2 (fp64 sum, one rounding; mu null:
// |y|^2), their maximum -> cmax_bits (atomicMax)
hipError_t launch_centre_norms(const char* codes, int dt, int row_bytes, int64_t r0, int64_t r1, const float* mu,
                               float* cnorms, unsigned* cmax_bits, hipStream_t s);
// scalar quantizer (fx_sq.hip): faiss's IndexScalarQuantizer with 8-bit codes.
// trained = [vmin[d] | vdiff[d]] fp32.  A stored row is row_bytes = roundup(d,
// 128) signed codes c' = c - 128 (padding 0); nc[row] = sum_j (s_j c'_j)^2 with
// s_j = vdiff_j / 255 (fp64 sum, rounded once).
constexpr int SQ_P = 3;          // int8 digit planes of the query operand
constexpr int SQ_STAGE_B = 64;   // bytes of each row's K staged per pipeline stage (one MFMA k-chunk)
constexpr int SQ_EXACT_GRID = 1024, SQ_MERGE_GRID = 256;
// index-wide constants on the device: float bits of max n_c, the integer max
// sum c'^2, float bits of rho_dec (the decode's rounding: |y_fp32 - (m + s c')|
// over any row), 1 word spare
enum { SQ_W_MAXNC = 0, SQ_W_MAXC2 = 1, SQ_W_RHO = 2, SQ_WORDS = 4 };
// mm = [min[d] | max[d]] as order-preserving uints (0xffffffff / 0 before the
// first row); *bad counts non-finite inputs
hipError_t launch_sq_minmax(const void* x, int x_dt, int64_t n, int d, unsigned* mm, unsigned long long* bad,
                            hipStream_t s);
hipError_t launch_sq_minmax_reset(unsigned* mm, int d, unsigned long long* bad, hipStream_t s);
// trained <- mm (uniform != 0: one global min / max in every entry)
hipError_t launch_sq_finish(const unsigned* mm, int d, int uniform, float* trained, hipStream_t s);
// words[SQ_W_RHO] <- the decode rounding bound of `trained`
hipError_t launch_sq_consts(const float* trained, int d, unsigned* words, hipStream_t s);
// rows x [n][d] -> signed codes at codes_row0 (stride row_bytes, padding
// zeroed), their n_c, and the two running maxima
hipError_t launch_sq_encode(const void* x, int x_dt, int64_t n, int d, const float* trained, int row_bytes,
                            char* codes_row0, float* nc_row0, unsigned* words, hipStream_t s);
// rows x [n][d] -> faiss's unsigned bytes [n][d]
hipError_t launch_sq_encode_u8(const void* x, int x_dt, int64_t n, int d, const float* trained, uint8_t* out,
                               hipStream_t s);
// out[i][0..d) fp32 <- decode of source row r_i: keys null: r_i = key0 + i; flip
// = 0x80 for caller bytes [.][stride] of faiss's unsigned codes, 0 for stored
// rows.  A key outside [0, nrows): a row of all-ones bits (NaN), nothing read.
hipError_t launch_sq_decode(const char* codes, int stride, int flip, int64_t nrows, const int64_t* keys, int64_t key0,
                            int64_t n, int d, const float* trained, float* out, hipStream_t s);
struct SqPrep {
    const void* q;        // [nq][d] on the device
    int q_dt, metric, d, row_bytes;
    int64_t nq, nq_pad;
    const float* trained;
    const unsigned* words;
    float* qf32;          // [nq_pad][row_bytes] fp32 queries, zero padded
    char* planes;         // [SQ_P][nq_pad][row_bytes]
    float* sigma;         // [nq_pad]
    float* qeps;          // [nq] E
    float* qrho;          // [nq] rho' = |w - w_op| (reported; the bound uses it inside E)
    double* qshift;       // [nq] |z|^2 (L2), -x.m (IP): scan key + shift estimates the exact key
    int* zero[2];         // counters set to 0 (flagged, dropped)
};
hipError_t launch_sq_prep(const SqPrep& p, hipStream_t s);
struct SqScan {
    const char* codes;
    const float* nc;
    int64_t ntotal;
    int row_bytes;
    const char* planes;
    const float* sigma;
    int64_t nq, nq_pad;
    int n_qtiles, n_ctiles, splits;
    float* cand_d;        // [n_qtiles][splits][TILE_Q][KP]
    int* cand_i;
};
hipError_t launch_sq_scan(int metric, const SqScan& p, hipStream_t s);
struct SqRefine {
    const float* cand_d;
    const int* cand_i;
    int splits;
    int64_t nq, ntotal;
    int k, d, row_bytes;
    const char* codes;
    const float* trained;
    const unsigned* words;
    const float* qf32;
    const float* qeps;
    const double* qshift;
    float* D;
    int64_t* I;
    int* n_flag;          // [0] count, [1 ..] flagged queries
    int* n_drop;
    int force_fb;
};
hipError_t launch_sq_refine(int metric, const SqRefine& p, hipStream_t s);
// k_sq_exact + k_sq_merge for the queries n_flag[1 ..] (count n_flag[0], read on
// the device): item (flagged f, split c of xs) -> cd / ci[item][k], merged under
// (key, row) -> D / I
struct SqExact {
    const char* codes;
    int row_bytes, d;
    int64_t ntotal;
    const float* trained;
    const float* qf32;
    const int* n_flag;
    int k, xs;
    float* cd;
    int* ci;
    float* D;
    int64_t* I;
};
hipError_t launch_sq_exact(int metric, const SqExact& p, hipStream_t s);
// inverted file over 8-bit codes (fx_ivfsq.hip): faiss's IndexIVFScalarQuantizer.  The payload is
// the inverted file's (list order, list_off, row_list) with the scalar quantizer's rows (signed
// codes, n_c); with by_residual a code encodes fl32(x - c_l) and the row decodes to fl32(c_l +
// decode(code)).  cent is the fp32 centroids [nlist][d], or null without by_residual.
// out[i][0..d) <- fl32(x[i] - cent[row_list[i]]) (a list number outside [0, nlist): x[i] itself)
hipError_t launch_ivfsq_residual(const void* x, int x_dt, int64_t n, int d, const int* row_list, int64_t nlist,
                                 const float* cent, float* out, hipStream_t s);
// words[SQ_W_RHO] <- the rounding bound of a decoded row: launch_sq_consts' per-dimension term plus
// u (max_l |c_lj| + max |decode_j|) for the addition of the centroid (cent null: launch_sq_consts)
hipError_t launch_ivfsq_consts(const float* trained, int d, const float* cent, int64_t nlist, unsigned* words,
                               hipStream_t s);
// out[i][0..d) <- faiss's unsigned bytes of stored rows [r0, r0 + n)
hipError_t launch_ivfsq_codes_u8(const char* codes, int row_bytes, int64_t r0, int64_t n, int d, uint8_t* out,
                                 hipStream_t s);
// Operand preparation per (query, probe) pair p = q * np + j (the list's centroid folded in):
//   L2  z = x - c_l - m, w = z o s, |x - y|^2 = |z|^2 - 2 w.c' + n_c      shift |z|^2
//   IP  w = x o s,                  x.y       = x.(c_l + m) + w.c'        shift -x.(c_l + m)
// planes, sigma, shift (fp32: the scan adds it to the key) and the pair's bound E.
struct IvfSqPrep {
    const void* q;          // [nq][d] on the device
    int q_dt, metric, d, row_bytes;
    int64_t nq;
    int np;
    int64_t pairs_pad;      // >= nq * np; rows past nq * np are written as zero operands
    const int64_t* coarse;  // [nq][np] probed lists
    int64_t nlist;
    const float* cent;      // [nlist][d] or null
    const float* trained;
    const unsigned* words;
    float* qf32;            // [nq][row_bytes] fp32 queries, zero padded
    char* planes;           // [SQ_P][pairs_pad][row_bytes]
    float* sigma;           // [pairs_pad]
    float* peps;            // [pairs_pad] E of the pair, the rounding of the shift and its addition included
    float* pshift;          // [pairs_pad]
    int* zero[2];           // counters set to 0
};
hipError_t launch_ivfsq_prep(const IvfSqPrep& p, hipStream_t s);
// k_ivfsq_scan: k_ivf_scan's grid and list logic around k_sq_scan's int8 tile loop; the B planes
// are fetched by pair number.  key = fl(fl(n_c - 2 sigma S) + shift) (IP: fl(-sigma S + shift)).
struct IvfSqScan {
    const char* codes;    // [rows][row_bytes] signed codes in list order, a whole tile past the end
    const float* nc;
    int row_bytes;
    const int* list_off;
    int64_t nlist;
    const char* planes;   // [SQ_P][pairs_pad][row_bytes]
    const float* sigma;   // [pairs_pad]
    const float* pshift;  // [pairs_pad]
    int64_t pairs_pad;
    int np, C;
    const uint64_t* sorted;
    const int* seg;
    const int* gbase;
    float* cand_d;        // [nq][np * C][KP]
    int* cand_i;
    int64_t grid;
};
hipError_t launch_ivfsq_scan(int metric, const IvfSqScan& p, hipStream_t s);
// k_sq_refine's three phases over [nq][slots][KP]; candidate keys carry their pair's shift, so the
// certification runs with shift 0 and E = the largest of the query's pairs'
struct IvfSqRefine {
    const float* cand_d;
    const int* cand_i;
    int slots, np;
    int64_t nq, ntotal;
    int k, d, row_bytes;
    const char* codes;
    const int* row_list;    // [ntotal] the rows' lists
    int64_t nlist;
    const float* cent;      // or null
    const float* trained;
    const unsigned* words;
    const float* qf32;      // [nq][row_bytes]
    const float* peps;      // [nq * np]
    const int64_t* labels;
    float* D;
    int64_t* I;
    int* n_flag;
    int* n_drop;
    int force_fb;
};
hipError_t launch_ivfsq_refine(int metric, const IvfSqRefine& p, hipStream_t s);
// k_ivfsq_exact (k_ivf_exact over decoded rows: decode plus centroid) + k_ivf_merge
struct IvfSqExact {
    IvfExact ex;            // codes: the signed codes; kdim: the fp32 queries' stride (row_bytes)
    int d;
    const float* trained;
    const float* cent;      // or null
};
hipError_t launch_ivfsq_exact(int metric, const IvfSqExact& p, hipStream_t s);
// product quantizer (fx_pq.hip): faiss's IndexPQ with 8-bit codes.  cb = the fp32 centroids
// [M][256][dsub].  A stored row is pq_stride(M) = roundup(M, 16) code bytes (padding 0) plus ny[row]
// = |decode|^2 (fp64 sum in dimension order, rounded once).  The scan image of the centroids (dsub %
// 8 == 0 only) is two bf16 planes [hi | lo] of pq_plane_bytes each: plane[(m * 256 + j) * dsub + e],
// then one 16-B piece of zeros, which the stage pieces past d gather.
constexpr int PQ_KSUB = 256;
constexpr int PQ_STAGE_D = 32;  // dimensions of each row staged per pipeline stage (64 B per plane: one MFMA k-chunk)
constexpr int PQ_STAGE_BYTES = 2 * (TILE_R + TILE_Q) * PQ_STAGE_D * 2;  // [A hi | A lo | B hi | B lo]
static_assert(2 * PQ_STAGE_BYTES == LDS_STAGE, "the gather stages fill k_scan_topk's double buffer");
constexpr int PQ_EXACT_GRID = 1024, PQ_MERGE_GRID = 256;
inline int pq_stride(int M) { return (M + 15) / 16 * 16; }
inline int pq_kpad(int d) { return (d + PQ_STAGE_D - 1) / PQ_STAGE_D * PQ_STAGE_D; }
inline int64_t pq_plane_bytes(int M, int dsub) { return ((int64_t)M * PQ_KSUB * dsub + 8) * 2; }
// out[r * stride + m] <- argmin_j |x[r][m dsub ..] - cb[m][j]|^2 (fp64, dimensions ascending, every
// operation rounded once, the lowest j on a tie); bytes m >= M of a row are not written
hipError_t launch_pq_encode(const void* x, int x_dt, int64_t n, int d, int M, int dsub, const float* cb, uint8_t* out,
                            int stride, hipStream_t s);
hipError_t launch_pq_ny(const uint8_t* codes, int stride, int64_t n, int M, int dsub, const float* cb, float* ny,
                        hipStream_t s);
// out[i][0..d) fp32 <- the centroids of source row r_i of codes [nrows][stride] (keys null: r_i = key0 +
// i).  A key outside [0, nrows): a row of all-ones bits (NaN), nothing read.
hipError_t launch_pq_decode(const uint8_t* codes, int stride, int64_t nrows, const int64_t* keys, int64_t key0,
                            int64_t n, int M, int dsub, const float* cb, float* out, hipStream_t s);
struct PqPrep {
    const void* q;        // [nq][d] on the device
    int q_dt, metric, d, kp;
    int64_t nq, nq_pad;
    double Y, Ry, Yl;     // index constants: max |decode|, max |y - y_hi - y_lo|, max |y_lo| over any code row
    float* qf32;          // [nq_pad][kp] fp32 queries, zero padded
    uint16_t* planes;     // [2][nq_pad][kp] bf16 hi / lo of -2 x (IP: -x)
    float* qeps;          // [nq] E
    float* qrho;          // [nq] |x' - x'_hi - x'_lo| (reported; the bound uses it inside E)
    double* qshift;       // [nq] |x|^2 (L2), 0 (IP)
    int* zero[2];         // counters set to 0
};
hipError_t launch_pq_prep(const PqPrep& p, hipStream_t s);
struct PqScan {
    const uint8_t* codes; // [cap_rows][stride], a whole tile past the last row, padding rows code 0
    const float* ny;
    int64_t ntotal;
    int stride, M, dsub, d, kp;
    const char* img;      // the scan image
    int64_t plane_bytes;
    const uint16_t* planes;
    int64_t nq, nq_pad;
    int n_qtiles, n_ctiles, splits;
    float* cand_d;        // [n_qtiles][splits][TILE_Q][KP]
    int* cand_i;
};
hipError_t launch_pq_scan(int metric, const PqScan& p, hipStream_t s);
struct PqRefine {
    const float* cand_d;
    const int* cand_i;
    int splits;
    int64_t nq, ntotal;
    int k, d, kp, M, dsub, stride;
    const uint8_t* codes;
    const float* cb;
    const float* qf32;
    const float* qeps;
    const double* qshift;
    float* D;
    int64_t* I;
    int* n_flag;          // [0] count, [1 ..] flagged queries
    int* n_drop;
    int force_fb;
};
hipError_t launch_pq_refine(int metric, const PqRefine& p, hipStream_t s);
// k_pq_exact + k_pq_merge for the queries n_flag[1 ..] (count n_flag[0], read on the device)
struct PqExact {
    const uint8_t* codes;
    int stride, M, dsub, d, kp;
    int64_t ntotal;
    const float* cb;
    const float* qf32;
    const int* n_flag;
    int k, xs;
    float* cd;
    int* ci;
    float* D;
    int64_t* I;
};
hipError_t launch_pq_exact(int metric, const PqExact& p, hipStream_t s);
// inverted file over product-quantized codes (fx_ivfpq.hip): faiss's IndexIVFPQ with 8-bit codes.  The
// payload is the inverted file's (list order, list_off, row_list) with the product quantizer's rows
// (pq_stride(M) code bytes, n_y = |decode|^2); with by_residual a code encodes fl32(x - c_l) and the row
// decodes to fl32(c_l + decode(code)).  cent is the fp32 centroids [nlist][d], or null without by_residual.
// Operand preparation.  per_pair != 0 (L2 with by_residual): operand row = pair p = q * np + j, x' = -2
// fl32(x - c_l), shift |x - c_l|^2.  Otherwise the operand row = the query (IP: -x; L2 without
// by_residual: -2 x) and only shift (IP: -(x . c_l); else |x|^2 / 0) and E are per pair.
struct IvfPqPrep {
    const void* q;          // [nq][d] on the device
    int q_dt, metric, d, kp;
    int64_t nq;
    int np, per_pair;
    int64_t op_rows;        // plane rows: >= nq * np (per_pair) or >= nq; rows past the live ones are zero operands
    const int64_t* coarse;  // [nq][np] probed lists
    int64_t nlist;
    const float* cent;      // [nlist][d] or null
    double Y, Ry, Yl, rho_dec;  // FxPq's constants, and the rounding bound of fl32(c_l + decode) (0 without by_residual)
    float* qf32;            // [nq][kp] fp32 queries, zero padded
    uint16_t* planes;       // [2][op_rows][kp] bf16 hi / lo
    float* peps;            // [nq * np] E of the pair
    float* pshift;          // [nq * np] fl32(shift)
    int* zero[2];           // counters set to 0
};
hipError_t launch_ivfpq_prep(const IvfPqPrep& p, hipStream_t s);
// k_ivfpq_scan: k_ivfsq_scan's grid and list logic around k_pq_scan's gather tile loop; the B planes
// are fetched by operand row pair / bdiv.  key = fl(fl(n_y + S) + shift) (IP: fl(S + shift)).
struct IvfPqScan {
    const uint8_t* codes; // [rows][stride] in list order, a whole zero tile past the last row
    const float* ny;
    int stride, M, dsub, d, kp;
    const char* img;      // the codebook's scan image
    int64_t plane_bytes;
    const int* list_off;
    int64_t nlist;
    const uint16_t* planes;  // [2][op_rows][kp]
    int64_t op_rows;
    int bdiv;             // operand row of pair p: p / bdiv (1: per pair; np: per query)
    const float* pshift;  // [nq * np]
    int np, C;
    const uint64_t* sorted;
    const int* seg;
    const int* gbase;
    float* cand_d;        // [nq][np * C][KP]
    int* cand_i;
    int64_t grid;
};
hipError_t launch_ivfpq_scan(int metric, const IvfPqScan& p, hipStream_t s);
// k_ivfsq_refine's three phases; the exact recomputation gathers the fp32 centroids and adds the list's
struct IvfPqRefine {
    const float* cand_d;
    const int* cand_i;
    int slots, np;
    int64_t nq, ntotal;
    int k, d, kp, dsub, stride;
    const uint8_t* codes;
    const float* cb;        // [M][256][dsub]
    const int* row_list;    // [ntotal] the rows' lists
    int64_t nlist;
    const float* cent;      // or null
    double rho_dec;
    const float* qf32;      // [nq][kp]
    const float* peps;      // [nq * np]
    const int64_t* labels;
    float* D;
    int64_t* I;
    int* n_flag;
    int* n_drop;
    int force_fb;
};
hipError_t launch_ivfpq_refine(int metric, const IvfPqRefine& p, hipStream_t s);
// k_ivfpq_exact (k_ivf_exact over decoded rows: gather plus centroid) + k_ivf_merge
struct IvfPqExact {
    IvfExact ex;            // codes: the code bytes; row_bytes: their stride; kdim: the fp32 queries' stride (kp)
    int d, dsub;
    const float* cb;
    const float* cent;      // or null
};
hipError_t launch_ivfpq_exact(int metric, const IvfPqExact& p, hipStream_t s);
hipError_t launch_synth(void* out, int64_t row0, int64_t n, int d, int dtype, uint64_t seed,
                        hipStream_t s);
hipError_t launch_to_f32(const void* codes, int st_dt, int row_bytes, int64_t n, int d, float* out,
                         hipStream_t s);

}  // namespace fx
