// fx_index.cpp -- host implementation of the C ABI declared in
// include/fx_index.h.  Owns HBM (code matrix, row norms, search workspace),
// sequences the kernels of fx_kernels.hip on one HIP stream per index, and
// reproduces faiss's IndexFlatL2 API contract (faiss_store.py:29-128,
// rag_datastore_manager.py:138-218) at the C level.
#include "../../include/fx_index.h"

#include <float.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "fx_internal.h"

using namespace fx;

namespace {

thread_local std::string g_err;

int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return set_err(FX_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                             \
    } while (0)

// Restores the caller's current device on scope exit (torch keeps its own
// notion of the current device per thread).
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        const size_t grow = std::max(want, bytes + bytes / 2);
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, grow);
        if (e == hipSuccess) bytes = grow;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// range_search's candidate buffer: entries it starts with unless the option
// range_cap says otherwise (8 B each, plus 24 B per candidate actually found
// for the exact distances, the sort and the result), and the option's limit
constexpr int RANGE_CAP_DEFAULT = 1 << 20, RANGE_CAP_MAX = 1 << 30;
// remove_ids' staging buffer in bytes unless the option remove_stage says
// otherwise (one row .. REMOVE_STAGE_MAX)
constexpr int64_t REMOVE_STAGE_DEFAULT = 256ll << 20, REMOVE_STAGE_MAX = 1ll << 32;

// rows per chunk of fx_kmeans_step unless the option kmeans_chunk says
// otherwise: the k = 1 search of a chunk keeps ~ (8 + 2 row_bytes) B of
// workspace per row plus its candidate lists, so 131,072 rows of d = 768 stay
// near 1 GiB whatever n is; the option's limit keeps a chunk's member blocks
// (<= rows / KM_M + rows) below 2^31
constexpr int KMEANS_CHUNK_DEFAULT = 1 << 17, KMEANS_CHUNK_MAX = 1 << 30;

// Per-index tuning options.  Initial values come from the FX_* environment
// variables, read ONCE when the index is created (never on the search path);
// fx_index_set_option changes them afterwards (range-checked: opt_range).
// Test hooks and diagnostic dumps exist only in the diagnostic build
// (-DFX_DIAG: libfx_index_diag.so, make diag / abl), never in libfx_index.so.
struct Options {
    int search_graph = 0;    // FX_SEARCH_GRAPH: replay small host searches as one hipGraph (round 5: -7 %
                             // per one-query call, r5r; off since round 6: with the call down to three
                             // kernels and one packed copy, the eager enqueue is 3-7 % faster: 97-101 vs
                             // 104 us on a 100k x 384 fp32 index, profiles/r6/latency_graph_r6f.jsonl)
    int place = -1;          // FX_SCAN_PLACE: scan block placement (-1 automatic, 0, 1)
    int sx = 0;              // FX_SCAN_SX: corpus splits per XCD under placement 1 (0 automatic)
    int reduce_cand = 1;     // FX_REDUCE_CAND: small nq over many splits: 1 one 16-wave workgroup refine per
                             // query (k_refine_wg), 2 merge 16 splits' lists first (k_reduce_cand, round 3),
                             // 0 the one-wave-per-query refine
    int f32_split = 1;       // FX_F32_SPLIT: fp32 indexes scan their split-bf16 image
    int centre = 1;          // FX_CENTER: L2 scan images are centred on a row sample's mean
    int pub = 1;             // FX_SCAN_PUB: union threshold over published per-split lists
    int prune_rank = 0;      // FX_PRUNE_RANK: rank of the shared threshold (0: max(6k/5, 12))
    int compact_at = 0;      // FX_COMPACT_AT: list fill that triggers a compaction (0: default 48, KP < v <= CAP)
    int union_w = 0;         // FX_UNION_W: splits per union-bound window (16, 32, 64; 0: by split count)
    int union_defer = 1;     // FX_UNION_DEFER: union bounds fetched by LDS-DMA, bounded a tile later (0: in place)
    int union_inplace = -1;  // FX_UNION_INPLACE: most lists per compaction call bounded in place beyond the
                             // deferred ones (-1: 0 with union_defer, all without; r5v: 0 is -1.4 % on the
                             // N = 8 shard and (b), (d) unchanged)
    int tight_at = -1;       // FX_TIGHT_AT: a list that took entries and holds >= this many gets its threshold
                             // re-bounded without a compaction (-1 default, 0 off, KP < v <= CAP)
    int cold_bound = -1;     // FX_COLD_BOUND: an empty list's first record tile bounds its threshold by the
                             // rank-th of the tile's group minima before pushing (0 off, 1 on, -1: on for
                             // splits of <= 256 tiles).  tight_at measured slower and off
                             // (profiles/r5/ab/r5h_tight_cold.txt); cold_bound -1.8 % on (b), -1 % on (d)
                             // at nq = 256 (short splits), +0.5-0.9 % on the long splits of (d) and the
                             // N = 8 shard (r5h, r5i, r5k)
    int graph_verbose = 0;   // FX_SEARCH_GRAPH_VERBOSE
    int refine_waves = REFINE_WG_WAVES;  // FX_REFINE_WAVES: waves of k_refine_wg's workgroup (4, 8, 16)
    int scan_v5 = 1;         // FX_SCAN_V5: 16-bit rows of 512 / 768 / 1,536 B scan with k_scan_v5 (64-row
                             // tiles, 256 / 192 queries per workgroup; fx_scan5.hip) where it adds no
                             // padding work; 2: wherever it has the shape (tests); 0: k_scan_v4
    int convoy = 1;          // FX_CONVOY: k_scan_v5 blocks start where the other blocks of their split
                             // are (ScanParams.conv); 0: at the split's first tile
    int convoy_every = 4;    // FX_CONVOY_EVERY: a block publishes its tile every this many tiles (1/2/4/8;
                             // 1: (d) 1.8x slower -- every block of a split writing one line each tile)
    int range_cap = 0;       // FX_RANGE_CAP: entries the range_search candidate buffer starts with (0: the
                             // default RANGE_CAP_DEFAULT; a call that finds more grows it and scans again)
    int64_t remove_stage = 0;  // FX_REMOVE_STAGE: bytes of remove_ids' staging buffer (0: REMOVE_STAGE_DEFAULT;
                               // row_bytes .. REMOVE_STAGE_MAX, checked by fx_index_set_option / at use)
    int kmeans_chunk = 0;    // FX_KMEANS_CHUNK: rows per chunk of fx_kmeans_step / fx_kmeans_update (0: the
                             // default KMEANS_CHUNK_DEFAULT; 1 .. 2^30)
    int host_spin = 1;       // FX_HOST_SPIN: a host-output search waits for its results by polling the
                             // stream (1) instead of a blocking hipStreamSynchronize (0)
#ifdef FX_DIAG
    int force_fallback = 0;  // FX_FORCE_FALLBACK: flag every query (1: -> re-scan, 2: -> exact scan)
    int scan_dbg = 0;        // FX_SCAN_DBG: ablation switches of -DFX_ABLATION builds / key dump (32)
    std::string trace, stamps, cand, keys;  // FX_SCAN_TRACE / _STAMPS / _CAND / _KEYS dump paths
#else
    static constexpr int force_fallback = 0, scan_dbg = 0;
#endif

    void from_env() {
        auto num = [](const char* name, int& v) {
            if (const char* e = getenv(name); e && *e) v = atoi(e);
        };
        auto str = [](const char* name, std::string& v) {
            if (const char* e = getenv(name); e && *e) v = e;
        };
        num("FX_SEARCH_GRAPH", search_graph);
        num("FX_SCAN_PLACE", place);
        num("FX_SCAN_SX", sx);
        num("FX_REDUCE_CAND", reduce_cand);
        num("FX_F32_SPLIT", f32_split);
        num("FX_CENTER", centre);
        num("FX_SCAN_PUB", pub);
        num("FX_PRUNE_RANK", prune_rank);
        num("FX_COMPACT_AT", compact_at);
        num("FX_UNION_W", union_w);
        num("FX_UNION_DEFER", union_defer);
        num("FX_UNION_INPLACE", union_inplace);
        num("FX_TIGHT_AT", tight_at);
        num("FX_COLD_BOUND", cold_bound);
        num("FX_SEARCH_GRAPH_VERBOSE", graph_verbose);
        num("FX_HOST_SPIN", host_spin);
        num("FX_SCAN_V5", scan_v5);
        num("FX_CONVOY", convoy);
        num("FX_CONVOY_EVERY", convoy_every);
        num("FX_REFINE_WAVES", refine_waves);
        num("FX_RANGE_CAP", range_cap);
        if (range_cap < 0 || range_cap > RANGE_CAP_MAX) range_cap = 0;
        num("FX_KMEANS_CHUNK", kmeans_chunk);
        if (kmeans_chunk < 0 || kmeans_chunk > KMEANS_CHUNK_MAX) kmeans_chunk = 0;
        if (const char* e = getenv("FX_REMOVE_STAGE"); e && *e) remove_stage = atoll(e);
        if (remove_stage < 0 || remove_stage > REMOVE_STAGE_MAX) remove_stage = 0;
        if (refine_waves != 4 && refine_waves != 8 && refine_waves != 16) refine_waves = REFINE_WG_WAVES;
        (void)str;
#ifdef FX_DIAG
        num("FX_FORCE_FALLBACK", force_fallback);
        num("FX_SCAN_DBG", scan_dbg);
        str("FX_SCAN_TRACE", trace);
        str("FX_SCAN_STAMPS", stamps);
        str("FX_SCAN_CAND", cand);
        str("FX_SCAN_KEYS", keys);
#endif
    }
    // option name -> its slot and accepted range [lo, hi] (allowed: a value
    // list when `set` is non-null)
    struct Slot {
        const char* name;
        int* v;
        int lo, hi;
        const int* set;
        int nset;
    };
    int* find(const char* name, int64_t value, const char** why) {
        static const int kWindows[] = {0, 16, 32, 64};
        static const int kWaves[] = {4, 8, 16};
        const Slot slots[] = {
            {"search_graph", &search_graph, 0, 1, nullptr, 0},
            {"scan_place", &place, -1, 1, nullptr, 0},
            {"scan_sx", &sx, 0, 1 << 16, nullptr, 0},
            {"reduce_cand", &reduce_cand, 0, 2, nullptr, 0},
            {"f32_split", &f32_split, 0, 1, nullptr, 0},
            {"centre", &centre, 0, 1, nullptr, 0},
            {"scan_pub", &pub, 0, 1, nullptr, 0},
            {"prune_rank", &prune_rank, 0, KP, nullptr, 0},
            {"compact_at", &compact_at, 0, CAP, nullptr, 0},
            {"union_w", &union_w, 0, 64, kWindows, 4},
            {"union_defer", &union_defer, 0, 1, nullptr, 0},
            {"union_inplace", &union_inplace, -1, 64, nullptr, 0},
            {"tight_at", &tight_at, -1, CAP, nullptr, 0},
            {"cold_bound", &cold_bound, -1, 1, nullptr, 0},
            {"host_spin", &host_spin, 0, 1, nullptr, 0},
            {"scan_v5", &scan_v5, 0, 2, nullptr, 0},
            {"convoy", &convoy, 0, 1, nullptr, 0},
            {"convoy_every", &convoy_every, 1, 8, nullptr, 0},
            {"refine_waves", &refine_waves, 4, 16, kWaves, 3},
            {"range_cap", &range_cap, 0, RANGE_CAP_MAX, nullptr, 0},
            {"kmeans_chunk", &kmeans_chunk, 0, KMEANS_CHUNK_MAX, nullptr, 0},
#ifdef FX_DIAG
            {"force_fallback", &force_fallback, 0, 2, nullptr, 0},
            {"scan_dbg", &scan_dbg, 0, 1 << 20, nullptr, 0},
#endif
        };
        for (const Slot& sl : slots) {
            if (strcmp(name, sl.name) != 0) continue;
            bool ok = value >= sl.lo && value <= sl.hi;
            if (ok && sl.set) {
                ok = false;
                for (int i = 0; i < sl.nset; ++i) ok |= value == sl.set[i];
            }
            // compact_at: 0 (default) or a fill in (KP, CAP]
            if (ok && sl.v == &compact_at) ok = value == 0 || value > KP;
            // tight_at: -1 (default), 0 (off) or a fill in (KP, CAP]
            if (ok && sl.v == &tight_at) ok = value <= 0 || value > KP;
            *why = ok ? nullptr : "value out of range";
            return sl.v;
        }
        *why = "unknown option";
        return nullptr;
    }
};

// scan image of the index (what the MFMA scan streams, and its row constants)
enum ImageKind {
    IMG_NONE = 0,  // the stored rows with srcC = |y|^2 (IP: no row constant)
    IMG_F32S = 1,  // fp32 index: [hi | lo] bf16 planes of fl(y - mu), srcC = |y - mu|^2
    IMG_C16 = 2,   // bf16 / fp16 L2 index: the stored rows, srcC = |y - mu|^2 (the query operand is x - mu)
};

}  // namespace

namespace {

// The device-side plan of one search: scan, refine and fallback parameters
// over the index's workspace.  Sizes the workspace (a no-op when it is large
// enough already, as it is for a graph capture right after do_search).
struct SearchPlan {
    int64_t nq = 0, nq_pad = 0;
    int k = 0, q_dtype = F32, scan_dt = F32;
    ScanParams sp{};
    RefineParams rp{};
    PrepParams pp{};
    bool reduce = false;
    size_t ncand = 0;
    // the re-scan of the queries pass 1 left uncertified (plan_rescan)
    ScanParams sp2{};
    RefineParams rp2{};
    PrepParams pp2{};
    int* n_exact = nullptr;  // queries the re-scan left uncertified too (-> exact scan)
    int nchunks = 0;         // re-scan chunks of <= RESCAN_MAX flagged queries each
    const FxSelector* sel = nullptr;  // non-null: a filtered search (fx_index_search_sel): the plain plan over
                                      // the stored rows, every scan through k_scan_topk_sel
    int* chunk_cnt = nullptr;  // [nchunks] live queries of each chunk (k_rescan_chunks, on the device)
    bool row_ids = false;  // a labelled index reports row numbers, not labels (fx_index_search_and_reconstruct
                           // gathers by row and translates I afterwards)
};

}  // namespace

struct FxIndex {
    int d = 0, dtype = F32, metric = L2, device = 0, normalize = 0;
    int row_bytes = 0, kdim = 0;
    int64_t ntotal = 0, cap_rows = 0, id_offset = 0;
    char* codes = nullptr;
    float* norms = nullptr;
    // stable ids (fx_idmap.hip): in the labelled mode (has_ids) row r's label is
    // labels[r]; the buffer holds label_cap >= cap_rows entries (grow_labels).
    // labels_alt: the second buffer a removal compacts into, then swapped in.
    bool has_ids = false;
    int64_t* labels = nullptr;
    int64_t* labels_alt = nullptr;
    int64_t label_cap = 0, label_alt_cap = 0;
    DevBuf idm_ws;  // sort workspace of a selector's id list / rows_of_ids, staged host ids
    // device words: [0] max |y|^2 of the stored rows, [1] max srcC of the scan
    // image (F32S / C16), as float bits (non-negative floats order as uints)
    unsigned* max_sq_bits = nullptr;
    hipStream_t own_stream = nullptr;
    hipStream_t user_stream = nullptr;
    hipEvent_t switch_ev = nullptr;  // orders the work of a stream the index leaves before the next one's
    Options opt;
    // search workspace
    DevBuf qin, qf32, qop, qeps, qrho, cand_d, cand_i, cand2_d, cand2_i, dws, iws, flag, fbc_d, fbc_i, stage, gtau,
        trace, dbgbuf, stamps, pub;
    // the re-scan of uncertified queries (plan_rescan): its own query
    // operands, thresholds, candidate lists and flagged list
    DevBuf rq_f32, rq_op, rq_eps, rq_rho, rq_shift, rq_gtau, rq_cand_d, rq_cand_i, rq_flag;
    // k > FX_BIG_K (fx_hugek.hip): query batch, sort keys, rocPRIM temporaries
    DevBuf hk_ws;
    // scan image (ImageKind; rows [0, img_rows) current).  L2 images are
    // centred (Options.centre): mu = mean of a row sample, recomputed (and the
    // image rebuilt) whenever ntotal has doubled since (mu_rows), so the
    // centre follows the data at O(1) amortised cost per added row.
    //   F32S: split = [hi | lo] bf16 planes of fl(y - mu), cnorms = |y - mu|^2
    //   C16:  cnorms = |y - mu|^2 of the stored bf16 / fp16 rows (no copy of
    //         the codes; a 16-bit centre whose norm is small next to the rows'
    //         is set to 0 on the device: k_mu_finish)
    DevBuf split, cnorms, centre, mu_part, qshift;
    int64_t img_rows = 0, mu_rows = 0;
    int img_kind = IMG_NONE;
    bool centred = false;
    // search_graph: the search of a small host batch (the reference's one-query
    // call form) replayed as one hipGraph per shape, over pinned host staging;
    // `gkey` = the shape and every buffer the graph captured
    hipGraphExec_t gexec = nullptr;
    std::vector<uint64_t> gkey;
    bool gfailed = false;
    void* ghq = nullptr;
    char* ghout = nullptr;  // pinned mirror of hout for the graph's one D2H copy
    size_t ghq_bytes = 0, ghout_bytes = 0;
    SearchPlan gplan;       // the captured search's plan (its fallback chain runs eagerly when needed)
    // host-output searches: ONE packed device buffer [D | I | n_drop | n_flag |
    // flag list] (host_out_layout) and its pinned mirror, so the common case
    // returns through one D2H copy
    DevBuf hout;
    char* hpin = nullptr;
    size_t hpin_bytes = 0;
    char* qpin = nullptr;   // pinned staging of a host-output search's host queries (<= QPIN_MAX)
    size_t qpin_bytes = 0;
    int64_t last_fallbacks = 0;
    // uncertified count of the last search, copied stream-ordered into pinned
    // memory; read (after a stream sync) only when asked for (fb_pending)
    int* pin_nf = nullptr;  // [0] queries re-scanned, [1] queries sent to the exact scan, [2] dropped ids
    bool fb_pending = false;
    int64_t last_exact = 0;
    // candidate entries the refine dropped for a row id outside [0, ntotal)
    // (a corrupted candidate list; 0 unless something is broken)
    int64_t last_dropped = 0;
    int* dev_drop = nullptr;  // its device word, zeroed at the start of every search
    // range_search (fx_range.hip): its own query operands and thresholds (none
    // of them a buffer a search graph captured), the candidate words, and the
    // last call's result (lims / D / I), kept until the next range search,
    // reset or free
    DevBuf rg_qin, rg_qf32, rg_qop, rg_eps, rg_rho, rg_shift, rg_thr, rg_cnt, rg_cand, rg_dist, rg_sorted, rg_temp,
        rg_lims, rg_D, rg_I;
    int64_t rg_nq = -1;       // queries of the stored result (-1: none)
    int64_t rg_total = 0;     // its lims[nq]
    int64_t rg_cands = 0;     // pairs the MFMA scan emitted
    int rg_passes = 0;        // scan passes run (0: no scan was needed)
    // remove_ids (fx_remove.hip): [prefix | gp | block sums | info | staged norms] (remove_rows)
    DevBuf rm_ws;
    // the last removal's plan: first removed row, rows moved in place / through staging, chunks launched
    int64_t rm_stats[4] = {0, 0, 0, 0};
    // reconstruct_batch / search_and_reconstruct / compute_distance_subset (fx_recon.hip): staged host
    // keys and queries, a labelled index's keys as rows, the fp32 queries, device results of a host
    // output -- none of them a buffer a search graph captured
    DevBuf rc_in, rc_rows, rc_qf32, rc_out;
    // k-means (fx_kmeans.hip): the update's workspace, the assignment / distances of a chunk when the
    // caller keeps none, staged host rows (device and pinned), the repair's working counts, and the
    // device counter of assignments outside [0, k) with its pinned mirror
    DevBuf km_ws, km_out, km_x, km_h;
    char* km_pin = nullptr;
    size_t km_pin_bytes = 0;
    unsigned long long* km_bad = nullptr;
    unsigned long long* km_bad_pin = nullptr;
    std::vector<hipEvent_t> km_ev, km_ev_fin;  // profiling: 4 events per chunk of a step, 2 per finish
    DevBuf conv;  // k_scan_v5 convoy words (CONV_WORDS; zeroed once, then only hints)
    int last_plan[3] = {0, 0, 0};  // the last search's scan plan: tile rows (128 k_scan_v4, 64 k_scan_v5), qt, splits
    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_scan, ev_merge;
    std::mutex mu;

    uint64_t epoch = 0;  // bumped by reset and by a removal: a selector (a snapshot of the rows) from before is stale

    hipStream_t stream() const { return user_stream ? user_stream : own_stream; }
};

// A selector (include/fx_index.h): the device image fx_select.hip builds of a
// subset of `index`'s rows [0, ntotal) as they were at creation.
struct FxSelector {
    const FxIndex* index = nullptr;  // identity only (never dereferenced: the index may be freed first)
    int device = 0;
    int64_t ntotal = 0;
    uint64_t epoch = 0;
    uint32_t* mask = nullptr;   // sel_mask_words(ntotal) words
    int* tiles = nullptr;       // [ceil(ntotal / TILE_R)] ascending live tiles
    SelCounts* cnt = nullptr;   // device counts (the scan reads cnt->tiles)
    // the counts on the host: copied stream-ordered into pinned memory after
    // the build, read (after `ready`) the first time someone asks
    SelCounts* pin = nullptr;
    hipEvent_t ready = nullptr;
    mutable bool known = false;
    mutable int64_t rows = 0, ntiles = 0;
    mutable std::mutex mu;
};

namespace {

int check_dtype(int dt) { return dt == FX_F32 || dt == FX_BF16 || dt == FX_F16; }

// the labelled mode's buffer follows the rows' capacity (a no-op without
// labels, or when it is large enough): the ntotal labels are carried over
hipError_t grow_labels(FxIndex* h) {
    if (!h->has_ids || (h->labels && h->label_cap >= h->cap_rows)) return hipSuccess;
    const int64_t cap = std::max<int64_t>(h->cap_rows, TILE_R);
    int64_t* labels = nullptr;
    hipError_t e = hipMalloc((void**)&labels, (size_t)cap * 8);
    if (e != hipSuccess) return e;
    hipStream_t s = h->stream();
    if (h->labels && h->ntotal > 0)
        e = hipMemcpyAsync(labels, h->labels, (size_t)h->ntotal * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (searches in flight still read the old buffer)
    if (e != hipSuccess) {
        (void)hipFree(labels);
        return e;
    }
    if (h->labels) (void)hipFree(h->labels);
    h->labels = labels;
    h->label_cap = cap;
    return hipSuccess;
}

hipError_t grow(FxIndex* h, int64_t need_rows) {
    if (need_rows <= h->cap_rows) return grow_labels(h);
    int64_t cap = round_up(std::max<int64_t>(need_rows, h->cap_rows + h->cap_rows / 2), TILE_R);
    char* codes = nullptr;
    float* norms = nullptr;
    hipError_t e = hipMalloc(&codes, (size_t)cap * h->row_bytes);
    if (e != hipSuccess) return e;
    e = hipMalloc(&norms, (size_t)cap * sizeof(float));
    if (e != hipSuccess) {
        (void)hipFree(codes);
        return e;
    }
    hipStream_t s = h->stream();
    // zero-fill: padding rows of the last tile must be finite
    e = hipMemsetAsync(codes + (size_t)h->ntotal * h->row_bytes, 0, (size_t)(cap - h->ntotal) * h->row_bytes, s);
    // padding rows: |y|^2 = +inf keeps them out of the scan's candidate lists
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(norms + h->ntotal), 0x7f800000u, (size_t)(cap - h->ntotal), s);
    if (e == hipSuccess && h->ntotal > 0) {
        e = hipMemcpyAsync(codes, h->codes, (size_t)h->ntotal * h->row_bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(norms, h->norms, (size_t)h->ntotal * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(codes);
        (void)hipFree(norms);
        return e;
    }
    if (h->codes) (void)hipFree(h->codes);
    if (h->norms) (void)hipFree(h->norms);
    h->codes = codes;
    h->norms = norms;
    h->cap_rows = cap;
    return grow_labels(h);
}

// split count whose live workgroups (one per CU: the scan's LDS) fill whole
// rounds of 256 CUs best, with >= ~4 rounds and >= min_tiles tiles per split
int fill_splits(int live_tiles, int eff_tiles, int n_ctiles, int min_tiles) {
    const int max_splits = std::max(1, n_ctiles / min_tiles);
    const int s0 = std::max(1, std::min(max_splits, (1024 + eff_tiles - 1) / eff_tiles));
    int best = s0;
    double best_eff = 0.0;
    for (int s = s0; s <= std::min(max_splits, 4 * s0); ++s) {
        const double live = (double)live_tiles * s;
        const double rounds = std::ceil(live / 256.0);
        const double eff = live / (rounds * 256.0);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
        if (eff > 0.985) break;
    }
    return best;
}

// The shape-only part of a scan's grid (map_tile's fields), for ntl query
// tiles and nct corpus tiles with >= min_tiles tiles per split.  partition:
// corpus-partitioned placement is admissible (taken once every XCD gets
// min_tiles tiles); group_qtiles: placement 0 gives each XCD a fixed group of
// query tiles when there are >= 8.  No index and no option enters.
struct SplitPlan {
    int place, sx, splits, qt_per_xcd;
    int qslots;  // workgroups per split: ntl, or 8 qt_per_xcd
    void store(ScanParams& p) const {
        p.place = place;
        p.sx = sx;
        p.splits = splits;
        p.qt_per_xcd = qt_per_xcd;
        p.grid = qslots * splits;
    }
};
SplitPlan plan_splits(int ntl, int nct, int min_tiles, bool partition, bool group_qtiles) {
    SplitPlan s = {0, 0, 1, 0, ntl};
    if (partition && nct >= 8 * min_tiles) {
        // XCD x owns 1/8 of the corpus for every query tile; sx splits per
        // XCD so that its ntl * sx blocks fill whole rounds of its 32 CUs
        s.place = 1;
        const int max_sx = std::max(1, nct / (8 * min_tiles));
        double best_eff = 0.0;
        for (int sx = 1; sx <= std::min(max_sx, std::max(16, 128 / ntl)); ++sx) {
            const double live = (double)ntl * sx;
            const double eff = live / (std::ceil(live / 32.0) * 32.0);
            if (eff > best_eff + 1e-9) { best_eff = eff; s.sx = sx; }
            if (eff > 0.985 && live >= 128) break;
        }
        s.splits = 8 * s.sx;
    } else {
        s.qt_per_xcd = group_qtiles && ntl >= 8 ? (ntl + 7) / 8 : 0;
        if (s.qt_per_xcd > 0) s.qslots = 8 * s.qt_per_xcd;
        s.splits = fill_splits(ntl, s.qslots, nct, min_tiles);
    }
    return s;
}

// the scan's grid: corpus splits per query tile and block placement.
// k > KP: no cross-split pruning (ScanParams.share = 0) and at least k/4
// splits, so that a split's KP-list rarely holds fewer than all of its top-k
// rows and the certification bound (the smallest full split's KP-th key)
// lies far beyond the k-th distance
void plan_scan(const FxIndex* h, int64_t nq, int k, ScanParams& p) {
    // the scan's shape: k_scan_v5 (64-row tiles x 256 queries) for the 16-bit
    // rows it has (not with the key-matrix dump, whose layout is k_scan_v4's)
    const int sdt = h->img_kind == IMG_F32S ? (int)F32S : h->dtype;
    // ... when its wider query tiles add no padding work: v5 query slots within
    // 5 % of k_scan_v4's (nq = 256 on 1,536-B rows would scan 384 slots for
    // 256 queries: 5.59 against 3.61 ms, profiles/r6/ab_v5_d_r6e.txt; one-query
    // calls keep k_scan_v4's 128-query tile)
    const int v5qt = h->opt.scan_v5 != 0 && !(h->opt.scan_dbg & 32) ? scan_v5_qt(sdt, h->row_bytes) : 0;
    const int64_t slots4 = (nq + TILE_Q - 1) / TILE_Q * TILE_Q;
    const bool v5 = v5qt > 0 && (h->opt.scan_v5 == 2 || (nq + v5qt - 1) / v5qt * v5qt * 20 <= slots4 * 21);
    p.qt = v5 ? v5qt : TILE_Q;
    p.tr = v5 ? V5_TR : TILE_R;
    p.n_qtiles = (int)((nq + p.qt - 1) / p.qt);
    p.n_ctiles = (int)((h->ntotal + p.tr - 1) / p.tr);
    p.pub = nullptr;
    p.prune_rank = KP;
    // default 48: with the union bound deferred a compaction is cheap enough
    // that tightening the threshold 16 entries earlier pays (same-box sweep,
    // profiles/r4/ab/compact_r4c.txt: (d) -1.1 %, (b) and the N = 8 shard -0.2 %)
    p.compact_at = h->opt.compact_at > KP && h->opt.compact_at <= CAP ? h->opt.compact_at : 48;
    p.share = k <= KP ? 1 : 0;
    p.union_w = 16;
    p.union_defer = h->opt.union_defer;
    p.union_inplace = h->opt.union_inplace >= 0 ? h->opt.union_inplace : p.union_defer ? 0 : (1 << 30);
    // list re-bounding between compactions (k <= KP only; -1: the default)
    p.tight_at = p.share && h->opt.tight_at > KP ? h->opt.tight_at : 0;
    p.cold_bound = 0;  // below, once the split count is known
    const int ntl = p.n_qtiles, nct = p.n_ctiles;
    // >= 3 tiles per split: a 100k-row index (782 tiles) then fills all 256
    // CUs with one query tile (256 splits; 192 at 4 tiles)
    constexpr int min_tiles = 3;
    // placement (map_tile): corpus-partitioned by default (config (d): 257 vs
    // 742 GB fetched past L2 per launch, ~2 % faster); scan_place = 0 forces
    // the query-tile groups of round 1.  Also for fewer than 8 query tiles:
    // the ntl blocks of one split then run side by side on one XCD, so the
    // split is fetched past L2 once for all of them (nq = 256: once instead
    // of twice)
    const int place = h->opt.place >= 0 ? h->opt.place : 1;
    SplitPlan sp = plan_splits(ntl, nct, min_tiles, place == 1, true);
    if (sp.place == 1) {
        const int max_sx = std::max(1, nct / (8 * min_tiles));
        if (h->opt.sx > 0) sp.sx = std::max(1, std::min(max_sx, h->opt.sx));  // placement A/B runs only
        if (k > KP) sp.sx = std::max(sp.sx, std::min(max_sx, ((k + 3) / 4 + 7) / 8));
        sp.splits = 8 * sp.sx;
    } else if (k > KP) {
        sp.splits = std::max(sp.splits, std::min(std::max(1, nct / min_tiles), (k + 3) / 4));
    }
    sp.store(p);
    // union-bound window (compact_regs): as many splits as there are, up to
    // 64, each contributing its first 256 / window published keys
    const int uw = h->opt.union_w;
    p.union_w = uw == 16 || uw == 32 || uw == 64 ? uw : p.splits <= 16 ? 16 : p.splits <= 32 ? 32 : 64;
    // cold-start bound: pays on short splits, where a block's first record
    // tiles are a large share of its work
    const int cb = h->opt.cold_bound;
    p.cold_bound = !p.share ? 0 : cb >= 0 ? cb : ((int64_t)(nct + p.splits - 1) / p.splits) * p.tr <= 256 * TILE_R ? 1 : 0;
    if (v5) p.tight_at = 0;  // (k_scan_v5 has no between-compaction re-bound)
}

// The plan of a filtered search (k_scan_topk_sel), whatever the index's scan
// image: 128 x 128 tiles over the stored rows, sized and placed from the
// shape alone as the range filter's grid is (plan_range_scan) -- over ALL the
// index's tiles, an upper bound of the selector's live ones, which the kernel
// divides among the splits on the device.  No cross-split sharing; k > KP
// takes at least k/4 splits like plan_scan, so that the splits' KP-entry
// lists can hold k results.
void plan_sel_scan(const FxIndex* h, int64_t nq, int k, ScanParams& p) {
    p.qt = TILE_Q;
    p.tr = TILE_R;
    p.n_qtiles = (int)((nq + TILE_Q - 1) / TILE_Q);
    p.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
    constexpr int min_tiles = 3;
    SplitPlan sp = plan_splits(p.n_qtiles, p.n_ctiles, min_tiles, true, false);
    if (k > KP) {
        if (sp.place == 1) {
            const int max_sx = std::max(1, p.n_ctiles / (8 * min_tiles));
            sp.sx = std::max(sp.sx, std::min(max_sx, ((k + 3) / 4 + 7) / 8));
            sp.splits = 8 * sp.sx;
        } else {
            sp.splits = std::max(sp.splits, std::min(std::max(1, p.n_ctiles / min_tiles), (k + 3) / 4));
        }
    }
    sp.store(p);
    p.share = 0;
    p.pub = nullptr;
    p.prune_rank = KP;
    p.compact_at = CAP;
    p.union_w = 16;
    p.union_defer = p.union_inplace = p.tight_at = p.cold_bound = 0;
}

// k > KP: approx candidates the refine re-ranks exactly (k_refine_big)
int big_k1(int k) { return k > KP ? std::max(2 * k, 64) : 0; }

// small batches over many splits (k <= KP, nq <= 256, >= 64 splits): the
// candidate walk is shared by the waves of one workgroup per query
// (reduce_cand 1, k_refine_wg) or by a separate merge of 16 splits' lists at a
// time before the refine (reduce_cand 2, k_reduce_cand)
bool small_many(int k, int64_t nq, int splits) { return k <= KP && nq <= 256 && splits >= 64; }

hipError_t ensure_pinned_count(FxIndex* h) {
    if (h->pin_nf) return hipSuccess;
    hipError_t e = hipHostMalloc((void**)&h->pin_nf, 3 * sizeof(int), hipHostMallocDefault);
    if (e == hipSuccess) h->pin_nf[0] = h->pin_nf[1] = h->pin_nf[2] = 0;
    return e;
}

// which scan image the index's current options call for
int image_kind(const FxIndex* h) {
    const int rb64 = h->row_bytes / 64;
    if (h->dtype == F32)
        return h->opt.f32_split != 0 && h->row_bytes % 64 == 0 && (rb64 == 8 || rb64 == 12 || rb64 == 16 || rb64 == 24)
                   ? IMG_F32S
                   : IMG_NONE;
    return h->metric == L2 && h->opt.centre != 0 ? IMG_C16 : IMG_NONE;
}

// bring the scan image up to date (rows appended since the last search)
hipError_t update_scan_image(FxIndex* h) {
    const int kind = image_kind(h);
    hipStream_t s = h->stream();
    hipError_t e = hipSuccess;
    if (kind == IMG_NONE) {
        h->img_kind = IMG_NONE;
        return hipSuccess;
    }
    const void* old = h->split.p;
    const void* old_n = h->cnorms.p;
    if (kind == IMG_F32S && (e = h->split.ensure((size_t)h->cap_rows * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->cnorms.ensure((size_t)h->cap_rows * 4)) != hipSuccess) return e;
    bool rebuild = h->split.p != old || h->cnorms.p != old_n || h->img_rows > h->ntotal || kind != h->img_kind;
    const bool centre = h->metric == L2 && h->opt.centre != 0;
    if (centre != h->centred) rebuild = true;
    if (centre && (h->mu_rows == 0 || h->ntotal >= 2 * h->mu_rows || kind != h->img_kind)) {
        // (re)centre on the current rows
        if ((e = h->centre.ensure((size_t)h->kdim * 4)) != hipSuccess) return e;
        if ((e = h->mu_part.ensure((size_t)2 * MU_GROUPS * h->kdim * 8)) != hipSuccess) return e;
        // 16-bit rows: a centre whose norm is below 0.1 of the rows' mean
        // square norm (no common direction) is dropped (mu = 0), which keeps
        // 16-bit-exact queries exact in the scan operand
        if ((e = launch_mu(h->codes, h->dtype, h->row_bytes, h->d, h->ntotal, (double*)h->mu_part.p,
                           (float*)h->centre.p, kind == IMG_C16 ? 0.1f : 0.0f, s)) != hipSuccess)
            return e;
        h->mu_rows = h->ntotal;
        rebuild = true;
    }
    h->centred = centre;
    h->img_kind = kind;
    if (rebuild) {  // zero image (finite padding rows), +inf padding norms
        if (kind == IMG_F32S && (e = hipMemsetAsync(h->split.p, 0, h->split.bytes, s)) != hipSuccess) return e;
        if ((e = hipMemsetD32Async((hipDeviceptr_t)h->cnorms.p, 0x7f800000u, h->cnorms.bytes / 4, s)) != hipSuccess)
            return e;
        if ((e = hipMemsetAsync(h->max_sq_bits + 1, 0, 4, s)) != hipSuccess) return e;
        h->img_rows = 0;
    }
    const float* mu = centre ? (const float*)h->centre.p : nullptr;
    if (kind == IMG_F32S)
        e = launch_split_rows((const float*)h->codes, h->kdim, h->img_rows, h->ntotal, mu, h->split.p,
                              (float*)h->cnorms.p, h->max_sq_bits + 1, s);
    else
        e = launch_centre_norms(h->codes, h->dtype, h->row_bytes, h->img_rows, h->ntotal, mu, (float*)h->cnorms.p,
                                h->max_sq_bits + 1, s);
    if (e == hipSuccess) h->img_rows = h->ntotal;
    return e;
}


// The re-scan of the queries pass 1 could not certify (rows flag_list[0 ..
// n_flag) of the batch, gathered on the device): the same MFMA scan over
// them without cross-split pruning and with ~k1/4 corpus splits, then
// k_refine_big re-ranking k1 = max(512, 4k) approx candidates exactly, so the
// certification bound sits near the k1-th key instead of the ~2k-th.  Its
// uncertified queries go to the exact scan.  Launched always; every kernel
// reads the flagged count and exits at once when it is 0.
// The re-scan's workspace is sized for RESCAN_MAX flagged queries whatever
// the batch (its lists are k1/4 splits wide); a batch that could flag more
// runs it in ceil(nq / RESCAN_MAX) chunks over the flagged list, each chunk's
// live count decided on the device (k_rescan_chunks: empty chunks exit at
// once), so a large batch never pays for a workspace it almost never uses
// and never sends re-scannable queries to the exact scan.
hipError_t plan_rescan(FxIndex* h, SearchPlan& P) {
    hipError_t e;
    const int64_t nq = std::min<int64_t>(P.nq, RESCAN_MAX);
    const int k1 = std::min(2 * FX_BIG_K, std::max(512, 4 * P.k));
    int* n_flag = P.rp.n_flag;
    ScanParams& sp = P.sp2;
    sp = P.sp;
    sp.nq = nq;
    if (P.sel) plan_sel_scan(h, nq, k1, sp);  // (a filtered search re-scans with its own kernel)
    else plan_scan(h, nq, k1, sp);  // k1 > KP: share = 0, >= k1/4 splits
    const int64_t nq_pad = round_up(nq, std::max<int64_t>(QPAD, sp.qt));
    if ((e = h->rq_f32.ensure((size_t)nq_pad * h->kdim * 4)) != hipSuccess) return e;
    if ((e = h->rq_op.ensure((size_t)nq_pad * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->rq_eps.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->rq_rho.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->rq_shift.ensure((size_t)nq * 8)) != hipSuccess) return e;
    if ((e = h->rq_gtau.ensure((size_t)nq_pad * 4)) != hipSuccess) return e;
    P.nchunks = (int)((P.nq + RESCAN_MAX - 1) / RESCAN_MAX);
    // [count | every query may go exact | the chunks' live counts]
    if ((e = h->rq_flag.ensure((size_t)(P.nq + 1 + P.nchunks) * 4)) != hipSuccess) return e;
    PrepParams& pp = P.pp2;
    pp = P.pp;
    pp.nq = nq;
    pp.nq_pad = nq_pad;
    pp.q = h->qf32.p;  // pass 1's fp32 copy of the batch, rows padded to kdim
    pp.q_dt = F32;
    pp.d = h->kdim;
    pp.qidx = P.rp.flag_list;
    pp.nq_dev = n_flag;
    pp.qf32 = (float*)h->rq_f32.p;
    pp.qop = h->rq_op.p;
    pp.qeps = (float*)h->rq_eps.p;
    pp.qrho = (float*)h->rq_rho.p;
    pp.qshift = (double*)h->rq_shift.p;
    sp.qop = (const char*)h->rq_op.p;
    sp.gtau = (unsigned*)h->rq_gtau.p;
    sp.pub = nullptr;
    sp.prune_rank = KP;
    sp.dbg = 0;
    sp.trace = nullptr;
    sp.dbgbuf = nullptr;
    sp.stamps = nullptr;
    sp.nq_dev = n_flag;
    const size_t ncand = (size_t)sp.n_qtiles * sp.splits * sp.qt * KP;
    if ((e = h->rq_cand_d.ensure(ncand * 4)) != hipSuccess) return e;
    if ((e = h->rq_cand_i.ensure(ncand * 4)) != hipSuccess) return e;
    sp.cand_d = (float*)h->rq_cand_d.p;
    sp.cand_i = (int*)h->rq_cand_i.p;
    RefineParams& rp = P.rp2;
    rp = P.rp;
    rp.nq = nq;
    rp.cand_d = sp.cand_d;
    rp.cand_i = sp.cand_i;
    rp.splits = sp.splits;
    rp.qt = sp.qt;
    rp.qf32 = pp.qf32;
    rp.qeps = pp.qeps;
    rp.qrho = pp.qrho;
    rp.qshift = pp.qshift;
    rp.k1 = k1;
    rp.gtau = nullptr;
    rp.nq_dev = n_flag;
    rp.out_idx = P.rp.flag_list;
    P.n_exact = (int*)h->rq_flag.p;
    P.chunk_cnt = P.n_exact + 1 + P.nq;
    rp.n_flag = P.n_exact;
    rp.flag_list = P.n_exact + 1;
    rp.force_fb = h->opt.force_fallback == 2;
    rp.wg = 0;
    return hipSuccess;
}

// words (non-null: a host-output search): [n_drop | n_flag | flag list[nq]]
// inside the packed output buffer; otherwise the index's own counter words
hipError_t plan_search(FxIndex* h, int64_t nq, const void* qdev, int q_dtype, int k, float* Dd, int64_t* Id,
                       int* words, SearchPlan& P) {
    hipError_t e;
    P.nq = nq;
    P.k = k;
    P.q_dtype = q_dtype;
    // a filtered search scans the stored rows themselves (no image)
    const int img_kind = P.sel ? (int)IMG_NONE : h->img_kind;
    P.scan_dt = img_kind == IMG_F32S ? (int)F32S : h->dtype;
    ScanParams& sp = P.sp;
    if (P.sel) plan_sel_scan(h, nq, k, sp);
    else plan_scan(h, nq, k, sp);
    h->last_plan[0] = sp.tr;
    h->last_plan[1] = sp.qt;
    h->last_plan[2] = sp.splits;
    P.nq_pad = round_up(nq, std::max<int64_t>(QPAD, sp.qt));  // whole scan tiles of (zero) queries
    const bool img = img_kind != IMG_NONE;
    if ((e = h->qf32.ensure((size_t)P.nq_pad * h->kdim * 4)) != hipSuccess) return e;
    if ((e = h->qop.ensure((size_t)P.nq_pad * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->qeps.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->qrho.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->qshift.ensure((size_t)nq * 8)) != hipSuccess) return e;

    PrepParams& pp = P.pp;
    pp.q = qdev;
    pp.q_dt = q_dtype;
    pp.nq = nq;
    pp.nq_pad = P.nq_pad;
    pp.d = h->d;
    pp.kdim = h->kdim;
    pp.st_dt = P.scan_dt;
    pp.metric = h->metric;
    pp.qf32 = (float*)h->qf32.p;
    pp.qop = h->qop.p;
    pp.qeps = (float*)h->qeps.p;
    pp.qrho = (float*)h->qrho.p;
    pp.qshift = (double*)h->qshift.p;
    pp.mbits = h->max_sq_bits;
    pp.img_bits = img ? h->max_sq_bits + 1 : h->max_sq_bits;
    pp.mu = img && h->centred ? (const float*)h->centre.p : nullptr;
    pp.qidx = nullptr;
    pp.nq_dev = nullptr;

    sp.codes = img_kind == IMG_F32S ? (const char*)h->split.p : h->codes;
    sp.norms = img ? (const float*)h->cnorms.p : h->norms;
    sp.ntotal = h->ntotal;
    sp.row_bytes = h->row_bytes;
    sp.qop = (const char*)h->qop.p;
    sp.nq = nq;
    sp.dbg = P.sel ? 0 : h->opt.scan_dbg;
    if ((e = h->gtau.ensure((size_t)P.nq_pad * 4)) != hipSuccess) return e;
    sp.gtau = (unsigned*)h->gtau.p;
    sp.conv = nullptr;
    // (only grids of more than one dispatch round: a single round's blocks
    // start together, and the word's read would only add a round trip to
    // the one-query call)
    if (!P.sel && h->opt.convoy != 0 && sp.grid > 256 && sp.splits <= CONV_MAX) {
        if (!h->conv.p) {
            if ((e = h->conv.ensure((size_t)CONV_WORDS * 4)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(h->conv.p, 0, (size_t)CONV_WORDS * 4, h->stream())) != hipSuccess) return e;
        }
        sp.conv = (unsigned*)h->conv.p;
    }
    {
        const int ce = h->opt.convoy_every;
        sp.conv_every = ce >= 8 ? 8 : ce >= 4 ? 4 : ce >= 2 ? 2 : 1;
    }
    // k_scan_v4's published per-split lists (the union threshold, see
    // compact_wave): slow-path tiles 25.7 -> 16.5 %, config (d) -3 %
    if (sp.share && sp.splits > 1 && h->opt.pub != 0) {
        const size_t npub = (size_t)sp.n_qtiles * sp.qt * sp.splits * KP;
        if ((e = h->pub.ensure(npub * 4)) != hipSuccess) return e;
        sp.pub = (float*)h->pub.p;
        // union bound taken at rank max(6k/5, 12) (<= KP): tighter pruning;
        // the refine's certification bound is capped by the final threshold.
        // (k = 10: 12, was 20 -- config (b) -4.5 %, (d) -1 %, 0 fallbacks in
        // every certification stress case; profiles/r3/ab/prune_rank*)
        sp.prune_rank = h->opt.prune_rank > 0 ? h->opt.prune_rank : std::max(6 * k / 5, 12);
        sp.prune_rank = std::max(k, std::min(KP, sp.prune_rank));
    }
    P.ncand = (size_t)sp.n_qtiles * sp.splits * sp.qt * KP;
    if ((e = h->cand_d.ensure(P.ncand * 4)) != hipSuccess) return e;
    if ((e = h->cand_i.ensure(P.ncand * 4)) != hipSuccess) return e;
    sp.cand_d = (float*)h->cand_d.p;
    sp.cand_i = (int*)h->cand_i.p;
    sp.trace = nullptr;
    sp.dbgbuf = nullptr;
    sp.stamps = nullptr;
    sp.nq_dev = nullptr;

    if ((e = h->flag.ensure((size_t)(nq + 1) * 4)) != hipSuccess) return e;
    RefineParams& rp = P.rp;
    rp.cand_d = sp.cand_d;
    rp.cand_i = sp.cand_i;
    rp.splits = sp.splits;
    rp.qt = sp.qt;
    rp.nq = nq;
    rp.ntotal = h->ntotal;
    rp.k = k;
    rp.codes = h->codes;
    rp.row_bytes = h->row_bytes;
    rp.kdim = h->kdim;
    rp.qf32 = pp.qf32;
    rp.qeps = pp.qeps;
    rp.qrho = pp.qrho;
    rp.qshift = pp.qshift;
    rp.id_offset = h->id_offset;
    rp.labels = h->has_ids && !P.row_ids ? h->labels : nullptr;
    rp.D = Dd;
    rp.I = Id;
    rp.n_flag = words ? words + 1 : (int*)h->flag.p;
    rp.flag_list = rp.n_flag + 1;
    rp.n_drop = words ? words : h->dev_drop;
    // small batches: one wave per query walks splits * KP candidates (256 splits
    // at nq = 1); issue 4 chunks of loads at a time (nq = 1: 0.84 -> ~0.3 ms)
    rp.prefetch = nq <= 256 ? 4 : 1;
    rp.k1 = big_k1(k);
    rp.force_fb = h->opt.force_fallback != 0;
    rp.gtau = sp.share ? sp.gtau : nullptr;
    rp.nq_dev = nullptr;
    rp.out_idx = nullptr;
    P.reduce = small_many(k, nq, sp.splits) && h->opt.reduce_cand == 2;
    rp.wg = small_many(k, nq, sp.splits) && h->opt.reduce_cand == 1 ? h->opt.refine_waves : 0;
    if (P.reduce) {
        const size_t nred = (size_t)sp.n_qtiles * ((sp.splits + 15) / 16) * sp.qt * KP;
        if ((e = h->cand2_d.ensure(nred * 4)) != hipSuccess) return e;
        if ((e = h->cand2_i.ensure(nred * 4)) != hipSuccess) return e;
    }
    const size_t nfb = (size_t)std::max<int64_t>(4096, nq) * k;
    if ((e = h->fbc_d.ensure(nfb * 4)) != hipSuccess) return e;
    if ((e = h->fbc_i.ensure(nfb * 4)) != hipSuccess) return e;
    return plan_rescan(h, P);
}

// the scan of a plan (pass 1's or the re-scan's parameters): the filtered
// kernel when the search has a selector
hipError_t run_scan(const FxIndex* h, const SearchPlan& P, const ScanParams& sp, hipStream_t s) {
    if (P.sel) return launch_scan_sel(h->dtype, h->metric, sp, P.sel->mask, P.sel->tiles, P.sel->cnt, s);
    return launch_scan(P.scan_dt, h->metric, sp, s);
}

// Enqueue the planned search on s up to its certification: query preparation
// (which also resets the shared thresholds, the published lists and the
// search's counters: one kernel instead of memsets), scan, refine +
// certification (small batches over many splits: one workgroup per query,
// or the separate candidate reduction when asked for).  No host sync: the
// same sequence is what a search graph captures.
hipError_t enqueue_main(FxIndex* h, SearchPlan& P, hipStream_t s, bool timed, hipEvent_t* ev) {
    hipError_t e;
    PrepParams pp1 = P.pp;
    pp1.gtau = P.sp.gtau;
    pp1.zero[0] = P.rp.n_drop;
    pp1.zero[1] = P.rp.n_flag;
    pp1.zero[2] = P.n_exact;
    pp1.pub = P.sp.pub;  // only live queries publish: nq rows of [splits][KP]
    pp1.npub = P.sp.pub ? P.nq * P.sp.splits * KP : 0;
    if ((e = launch_prep_queries(pp1, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
    if ((e = run_scan(h, P, P.sp, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
    RefineParams rp = P.rp;
    if (P.reduce) {
        int ng = 0;
        if ((e = launch_reduce_cand(P.sp.cand_d, P.sp.cand_i, P.sp.splits, P.nq, P.sp.qt, (float*)h->cand2_d.p,
                                    (int*)h->cand2_i.p, &ng, P.rp.ntotal, P.rp.n_drop, s)) != hipSuccess)
            return e;
        rp.cand_d = (const float*)h->cand2_d.p;
        rp.cand_i = (const int*)h->cand2_i.p;
        rp.splits = ng;
    }
    if ((e = launch_refine(h->dtype, h->metric, rp, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
    return hipSuccess;
}

// The chain for the queries the refine could not certify (rare: only when the
// candidate margin is inside the scan's rounding bound): a re-scan with a
// wide candidate set (plan_rescan), then the exact scan for what that still
// cannot certify.  Device-gated: every kernel reads the flagged count and
// exits at once when it is 0.  A device-resident search enqueues it always
// (no host round trip inside the search); a host-output search enqueues it
// only when its packed result says some query was flagged (finish_host_out).
hipError_t enqueue_fallback(FxIndex* h, SearchPlan& P, hipStream_t s) {
    hipError_t e;
#ifdef FX_ABLATION
    if ((P.sp.dbg & ~32) != 0) return hipSuccess;  // ablated scans: results invalid, no fallback chain
#endif
    if ((e = launch_rescan_chunks(P.rp.n_flag, (int)RESCAN_MAX, P.nchunks, P.chunk_cnt, s)) != hipSuccess) return e;
    for (int c = 0; c < P.nchunks; ++c) {  // chunk c: flagged queries [c RESCAN_MAX, ...)
        const int* list = P.rp.flag_list + (size_t)c * RESCAN_MAX;
        PrepParams pp = P.pp2;
        pp.qidx = list;
        pp.nq_dev = P.chunk_cnt + c;
        pp.zero[0] = pp.zero[1] = pp.zero[2] = nullptr;
        pp.pub = nullptr;
        pp.npub = 0;
        ScanParams sp = P.sp2;
        pp.gtau = sp.gtau;  // reset by the chunk's query preparation
        sp.nq_dev = P.chunk_cnt + c;
        RefineParams rp2 = P.rp2;
        rp2.nq_dev = P.chunk_cnt + c;
        rp2.out_idx = list;
        if ((e = launch_prep_queries(pp, s)) != hipSuccess) return e;
        if ((e = run_scan(h, P, sp, s)) != hipSuccess) return e;
        if ((e = launch_refine(h->dtype, h->metric, rp2, s)) != hipSuccess) return e;
    }
    return launch_exact_fallback(h->dtype, h->metric, h->codes, h->row_bytes, h->kdim, h->ntotal, P.rp.qf32,
                                 P.n_exact, P.k, h->id_offset, (float*)h->fbc_d.p, (int*)h->fbc_i.p, P.rp.D, P.rp.I,
                                 s, P.sel ? P.sel->mask : nullptr, P.rp.labels);
}

// Host-output searches (the reference's call form) return through ONE packed
// device buffer, copied back with one D2H:
//   [D: nq k f32 | I: nq k i64 | n_drop | n_flag | flag list: nq i32]
// (the copy covers D .. n_flag; the flag list stays on the device for the
// fallback chain)
struct HostOut {
    size_t offI = 0, offW = 0, copy_bytes = 0, bytes = 0;
};
HostOut host_out_layout(int64_t nq, int k) {
    HostOut L;
    L.offI = (size_t)round_up(nq * k * 4, 8);
    L.offW = L.offI + (size_t)nq * k * 8;
    L.copy_bytes = L.offW + 8;
    L.bytes = L.offW + (size_t)(2 + nq) * 4;
    return L;
}

hipError_t ensure_pinned(char*& p, size_t& have, size_t want) {
    if (want <= have) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    const size_t grow = std::max(want, have + have / 2);
    hipError_t e = hipHostMalloc((void**)&p, grow, hipHostMallocDefault);
    if (e == hipSuccess) have = grow;
    return e;
}

#ifdef FX_DIAG
template <typename T>
hipError_t dump_device(const std::string& path, const void* dev, size_t n) {
    std::vector<T> v(n);
    hipError_t e = hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    if (FILE* f = fopen(path.c_str(), "ab")) {
        fwrite(v.data(), sizeof(T), n, f);
        fclose(f);
    }
    return hipSuccess;
}
#endif

// a host-output search whose refine dropped candidate ids outside [0, ntotal)
// (a corrupted scan list): the top-k may be missing rows, so it is an error
// (include/fx_index.h, fx_index_last_dropped_candidates)
int integrity_error(const FxIndex* h) {
    return set_err(FX_E_INTEGRITY, "search: %lld candidate row ids outside [0, %lld) were dropped (corrupted scan list)",
                   (long long)h->last_dropped, (long long)h->ntotal);
}

// Wait for a host-output search's results.  The one-query call is latency
// bound: polling the stream (host_spin) returns as soon as the D2H copy is
// done, where a blocking synchronise adds the runtime's wake-up latency.
hipError_t wait_results(const FxIndex* h, hipStream_t s) {
    if (!h->opt.host_spin) return hipStreamSynchronize(s);
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
    }
}

// A host-output search after its packed copy landed in `pin` (the stream is
// synchronised): when the refine flagged queries, run their fallback chain
// now and copy the results again (rare); then hand D / I to the caller.
int finish_host_out(FxIndex* h, SearchPlan& P, const HostOut& L, char* pin, float* D, int64_t* I) {
    hipStream_t s = h->stream();
    const int nflag = ((const int*)(pin + L.offW))[1];
    h->last_exact = 0;
    if (nflag > 0) {
        HIP_TRY(ensure_pinned_count(h));
        HIP_TRY(enqueue_fallback(h, P, s));
        HIP_TRY(hipMemcpyAsync(pin, P.rp.D, L.copy_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 1, P.n_exact, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->last_exact = h->pin_nf[1];
    }
    const int* w = (const int*)(pin + L.offW);
    memcpy(D, pin, (size_t)P.nq * P.k * 4);
    memcpy(I, pin + L.offI, (size_t)P.nq * P.k * 8);
    h->last_fallbacks = nflag;
    h->last_dropped = w[0];
    h->fb_pending = false;
    return h->last_dropped > 0 ? integrity_error(h) : FX_OK;
}

// host queries of a host-output search up to this size go through pinned
// staging (a memcpy and an async DMA instead of the runtime's pageable path:
// the one-query call is latency bound); the call waits for its results, so
// the staging buffer is free again when it returns
constexpr size_t QPIN_MAX = (size_t)4 << 20;

int do_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
              int out_mem, const FxSelector* sel = nullptr, bool row_ids = false) {
    hipStream_t s = h->stream();
    const int qes = dtype_size(q_dtype);
    // queries -> device
    const void* qdev = q;
    if (q_mem == FX_MEM_HOST) {
        const size_t qb = (size_t)nq * h->d * qes;
        HIP_TRY(h->qin.ensure(qb));
        if (out_mem == FX_MEM_HOST && qb <= QPIN_MAX && ensure_pinned(h->qpin, h->qpin_bytes, qb) == hipSuccess) {
            memcpy(h->qpin, q, qb);
            HIP_TRY(hipMemcpyAsync(h->qin.p, h->qpin, qb, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(h->qin.p, q, qb, hipMemcpyHostToDevice, s));
        }
        qdev = h->qin.p;
    }
    // host results: the packed output buffer (host_out_layout)
    const bool host_out = out_mem == FX_MEM_HOST;
    HostOut L;
    float* Dd = D;
    int64_t* Id = I;
    int* words = nullptr;
    if (host_out) {
        L = host_out_layout(nq, k);
        HIP_TRY(h->hout.ensure(L.bytes));
        HIP_TRY(ensure_pinned(h->hpin, h->hpin_bytes, L.copy_bytes));
        Dd = (float*)h->hout.p;
        Id = (int64_t*)((char*)h->hout.p + L.offI);
        words = (int*)((char*)h->hout.p + L.offW);
    }
    if (!sel) HIP_TRY(update_scan_image(h));  // (a filtered search reads no image)
    SearchPlan P;
    P.sel = sel;
    P.row_ids = row_ids;
    HIP_TRY(plan_search(h, nq, qdev, q_dtype, k, Dd, Id, words, P));
#ifdef FX_DIAG
    // diagnostics (Options): per-block placement/timing, phase stamps, the
    // scan's key matrix, raw candidate lists -> binary files
    const size_t grid = (size_t)P.sp.grid;
    if (!h->opt.stamps.empty()) {
        HIP_TRY(h->stamps.ensure(grid * 4 * 128));
        HIP_TRY(hipMemsetAsync(h->stamps.p, 0, grid * 4 * 128, s));
        P.sp.stamps = (unsigned long long*)h->stamps.p;
    }
    const size_t nkeys = (size_t)P.sp.n_qtiles * P.sp.qt * P.sp.n_ctiles * P.sp.tr;
    if ((P.sp.dbg & 32) && nkeys <= (size_t)1 << 26) {
        HIP_TRY(h->dbgbuf.ensure(nkeys * 4));
        HIP_TRY(hipMemsetAsync(h->dbgbuf.p, 0xff, nkeys * 4, s));
        P.sp.dbgbuf = (unsigned*)h->dbgbuf.p;
    }
    if (!h->opt.trace.empty()) {
        HIP_TRY(h->trace.ensure(grid * 32));
        HIP_TRY(hipMemsetAsync(h->trace.p, 0, grid * 32, s));
        P.sp.trace = (unsigned long long*)h->trace.p;
    }
#endif
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (h->profile)
        for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
    HIP_TRY(enqueue_main(h, P, s, h->profile, ev));
    if (h->profile) {
        h->ev_scan.emplace_back(ev[0], ev[1]);
        h->ev_merge.emplace_back(ev[1], ev[2]);
    }
    if (!host_out) {
        // device results: the uncertified queries' chain is enqueued always and
        // decided on the device; the counts follow stream-ordered into pinned
        // memory, read only when asked for (read_counts)
        HIP_TRY(enqueue_fallback(h, P, s));
        HIP_TRY(ensure_pinned_count(h));
        HIP_TRY(hipMemcpyAsync(h->pin_nf, P.rp.n_flag, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 1, P.n_exact, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 2, P.rp.n_drop, 4, hipMemcpyDeviceToHost, s));
        h->fb_pending = true;
    }
#ifdef FX_DIAG
    if (!h->opt.cand.empty()) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(dump_device<float>(h->opt.cand, P.sp.cand_d, P.ncand));
        HIP_TRY(dump_device<int>(h->opt.cand, P.sp.cand_i, P.ncand));
    }
    if (P.sp.dbgbuf) {  // the scan's key matrix [n_qtiles*128][n_ctiles*128]
        HIP_TRY(hipStreamSynchronize(s));
        const std::string path = h->opt.keys.empty() ? std::string("/tmp/fx_keys.bin") : h->opt.keys;
        if (FILE* f = fopen(path.c_str(), "wb")) fclose(f);  // truncate: one dump per search
        HIP_TRY(dump_device<float>(path, P.sp.dbgbuf, nkeys));
    }
    if (P.sp.stamps) {
        HIP_TRY(hipStreamSynchronize(s));
        if (FILE* f = fopen(h->opt.stamps.c_str(), "wb")) fclose(f);
        HIP_TRY(dump_device<unsigned long long>(h->opt.stamps, P.sp.stamps, grid * 4 * 16));
    }
    if (P.sp.trace) {
        HIP_TRY(hipStreamSynchronize(s));
        if (FILE* f = fopen(h->opt.trace.c_str(), "wb")) fclose(f);
        HIP_TRY(dump_device<unsigned long long>(h->opt.trace, P.sp.trace, grid * 4));
    }
#endif
    if (!host_out) return FX_OK;
    // host results: ONE packed D2H copy [D | I | n_drop | n_flag]
    HIP_TRY(hipMemcpyAsync(h->hpin, h->hout.p, L.copy_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(wait_results(h, s));
    return finish_host_out(h, P, L, h->hpin, D, I);
}

// k > FX_BIG_K: exact keys of every (query, row) pair and a radix sort per
// query (fx_hugek.hip).  Every result is exact, so no query is "uncertified".
constexpr size_t HK_KEEP_BYTES = (size_t)512 << 20;
int do_search_hugek(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                    int out_mem, bool row_ids = false) {
    hipStream_t s = h->stream();
    const void* qdev = q;
    if (q_mem == FX_MEM_HOST) {
        HIP_TRY(h->qin.ensure((size_t)nq * h->d * dtype_size(q_dtype)));
        HIP_TRY(hipMemcpyAsync(h->qin.p, q, (size_t)nq * h->d * dtype_size(q_dtype), hipMemcpyHostToDevice, s));
        qdev = h->qin.p;
    }
    float* Dd = D;
    int64_t* Id = I;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->dws.ensure((size_t)nq * k * 4));
        HIP_TRY(h->iws.ensure((size_t)nq * k * 8));
        Dd = (float*)h->dws.p;
        Id = (int64_t*)h->iws.p;
    }
    const int qb = hugek_batch(h->ntotal, nq);
    size_t ws = 0;
    HIP_TRY(hugek_workspace(h->ntotal, h->kdim, qb, &ws));
    HIP_TRY(h->hk_ws.ensure(ws));
    HugeKParams p{};
    p.codes = h->codes;
    p.row_bytes = h->row_bytes;
    p.kdim = h->kdim;
    p.d = h->d;
    p.st_dt = h->dtype;
    p.metric = h->metric;
    p.ntotal = h->ntotal;
    p.q = qdev;
    p.q_dt = q_dtype;
    p.nq = nq;
    p.k = k;
    p.id_offset = h->id_offset;
    p.labels = h->has_ids && !row_ids ? h->labels : nullptr;
    p.D = Dd;
    p.I = Id;
    HIP_TRY(launch_hugek_search(p, h->hk_ws.p, h->hk_ws.bytes, qb, s));
    // the sort keys + rocPRIM temporaries stay cached for the next call up to
    // HK_KEEP_BYTES; a larger workspace (up to 2 GiB of keys) is released
    // after the call, which waits for the stream (hipFree would anyway)
    if (h->hk_ws.bytes > HK_KEEP_BYTES) {
        HIP_TRY(hipStreamSynchronize(s));
        h->hk_ws.release();
    }
    h->last_fallbacks = 0;
    h->last_exact = 0;
    h->last_dropped = 0;
    h->fb_pending = false;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

// Shape + options + every device buffer a captured search touches: the graph
// is valid while all of them are unchanged
std::vector<uint64_t> graph_key(const FxIndex* h, int64_t nq, int q_dtype, int k) {
    const Options& o = h->opt;
    return {(uint64_t)nq, (uint64_t)q_dtype, (uint64_t)k, (uint64_t)h->ntotal, (uint64_t)h->id_offset,
            (uint64_t)h->img_kind, (uint64_t)h->centred, (uint64_t)h->img_rows,
            (uint64_t)o.force_fallback, (uint64_t)o.place, (uint64_t)o.sx, (uint64_t)o.reduce_cand,
            (uint64_t)o.pub, (uint64_t)o.prune_rank, (uint64_t)o.compact_at, (uint64_t)o.union_w,
            (uint64_t)o.union_defer, (uint64_t)(int64_t)o.union_inplace, (uint64_t)(int64_t)o.tight_at, (uint64_t)o.cold_bound,
            (uint64_t)o.reduce_cand, (uint64_t)o.scan_v5, (uint64_t)o.refine_waves, (uint64_t)o.convoy, (uint64_t)o.convoy_every,
            (uint64_t)(uintptr_t)h->codes, (uint64_t)(uintptr_t)h->norms, (uint64_t)(uintptr_t)h->split.p,
            (uint64_t)(uintptr_t)h->cnorms.p, (uint64_t)(uintptr_t)h->centre.p, (uint64_t)(uintptr_t)h->qshift.p,
            (uint64_t)(uintptr_t)h->qin.p, (uint64_t)(uintptr_t)h->qf32.p, (uint64_t)(uintptr_t)h->qop.p,
            (uint64_t)(uintptr_t)h->qeps.p, (uint64_t)(uintptr_t)h->qrho.p, (uint64_t)(uintptr_t)h->gtau.p,
            (uint64_t)(uintptr_t)h->pub.p, (uint64_t)(uintptr_t)h->cand_d.p, (uint64_t)(uintptr_t)h->cand_i.p,
            (uint64_t)(uintptr_t)h->cand2_d.p, (uint64_t)(uintptr_t)h->cand2_i.p,
            (uint64_t)(uintptr_t)h->hout.p, (uint64_t)(uintptr_t)h->conv.p,
            (uint64_t)(uintptr_t)h->flag.p, (uint64_t)(uintptr_t)h->fbc_d.p, (uint64_t)(uintptr_t)h->fbc_i.p,
            (uint64_t)(uintptr_t)h->rq_f32.p, (uint64_t)(uintptr_t)h->rq_op.p, (uint64_t)(uintptr_t)h->rq_eps.p,
            (uint64_t)(uintptr_t)h->rq_rho.p, (uint64_t)(uintptr_t)h->rq_shift.p, (uint64_t)(uintptr_t)h->rq_gtau.p,
            (uint64_t)(uintptr_t)h->rq_cand_d.p, (uint64_t)(uintptr_t)h->rq_cand_i.p,
            (uint64_t)(uintptr_t)h->rq_flag.p,
            // the label buffer the refine reads (null without labels): growth and a removal's swap replace it
            (uint64_t)(uintptr_t)(h->has_ids ? h->labels : nullptr)};
}

void graph_release(FxIndex* h) {
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
    h->gkey.clear();
}

// Record the stream-ordered search of do_search (host queries, host results,
// no diagnostics) into h->gexec: the query's H2D copy, enqueue_main (prep,
// scan, refine: no fallback chain) and the packed result's one D2H copy.
// Runs right after a do_search of the same shape, so every workspace is
// sized and every kernel attribute set.
hipError_t graph_build(FxIndex* h, int64_t nq, int q_dtype, int k) {
    graph_release(h);
    hipStream_t s = h->stream();
    const size_t qb = (size_t)nq * h->d * dtype_size(q_dtype);
    const HostOut L = host_out_layout(nq, k);
    hipError_t e = hipSuccess;
    if (qb > h->ghq_bytes) {
        if (h->ghq) (void)hipHostFree(h->ghq);
        h->ghq = nullptr;
        h->ghq_bytes = 0;
        if ((e = hipHostMalloc(&h->ghq, qb, hipHostMallocDefault)) != hipSuccess) return e;
        h->ghq_bytes = qb;
    }
    if ((e = ensure_pinned(h->ghout, h->ghout_bytes, L.copy_bytes)) != hipSuccess) return e;
    if ((e = h->hout.ensure(L.bytes)) != hipSuccess) return e;  // (sized by the do_search before)
    char* hb = (char*)h->hout.p;
    SearchPlan& P = h->gplan;
    P = SearchPlan{};
    if ((e = plan_search(h, nq, h->qin.p, q_dtype, k, (float*)hb, (int64_t*)(hb + L.offI), (int*)(hb + L.offW),
                         P)) != hipSuccess)
        return e;
    P.sp.dbg = 0;

    if ((e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal)) != hipSuccess) return e;
    g_graph_capture = true;
    hipError_t ce = hipMemcpyAsync(h->qin.p, h->ghq, qb, hipMemcpyHostToDevice, s);
    if (ce == hipSuccess) ce = enqueue_main(h, P, s, false, nullptr);
    if (ce == hipSuccess) ce = hipMemcpyAsync(h->ghout, hb, L.copy_bytes, hipMemcpyDeviceToHost, s);
    g_graph_capture = false;
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(s, &graph);  // always end the capture: the stream must leave capture mode
    if (ce != hipSuccess) e = ce;
    if (e == hipSuccess) e = hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (e != hipSuccess) {
        h->gexec = nullptr;
        (void)hipGetLastError();
        return e;
    }
    h->gkey = graph_key(h, nq, q_dtype, k);
    return hipSuccess;
}

// Small host batches under search_graph: replay the captured search; its
// fallback chain runs eagerly only when the packed result flags a query
// (finish_host_out).  On a shape / buffer / option change run do_search and
// re-capture.
int graph_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int k, float* D, int64_t* I) {
    HIP_TRY(update_scan_image(h));
    if (h->gexec && graph_key(h, nq, q_dtype, k) == h->gkey) {
        hipStream_t s = h->stream();
        memcpy(h->ghq, q, (size_t)nq * h->d * dtype_size(q_dtype));
        HIP_TRY(hipGraphLaunch(h->gexec, s));
        HIP_TRY(wait_results(h, s));
        return finish_host_out(h, h->gplan, host_out_layout(nq, k), h->ghout, D, I);
    }
    const int rc = do_search(h, nq, q, q_dtype, FX_MEM_HOST, k, D, I, FX_MEM_HOST);
    if (rc == FX_OK && !h->gfailed) {
        const hipError_t e = graph_build(h, nq, q_dtype, k);
        if (e != hipSuccess) {  // stay on do_search for this index
            h->gfailed = true;
            if (h->opt.graph_verbose) fprintf(stderr, "fx: search graph capture failed: %s\n", hipGetErrorString(e));
        } else if (h->opt.graph_verbose) {
            fprintf(stderr, "fx: search graph captured (nq=%lld k=%d)\n", (long long)nq, k);
        }
    }
    return rc;
}

// every slot missing (I = -1, D = FLT_MAX; IP: -FLT_MAX): the search of an
// empty index, or of an empty selection
int fill_missing(FxIndex* h, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
    const float dfill = h->metric == L2 ? FLT_MAX : -FLT_MAX;
    if (out_mem == FX_MEM_HOST) {
        std::fill(D, D + (size_t)nq * k, dfill);
        std::fill(I, I + (size_t)nq * k, (int64_t)-1);
    } else {  // stream-ordered fills: -1 is all ones in two's complement
        uint32_t bits;
        memcpy(&bits, &dfill, 4);
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)D, bits, (size_t)nq * k, h->stream()));
        HIP_TRY(hipMemsetAsync(I, 0xff, (size_t)nq * k * 8, h->stream()));
    }
    h->last_fallbacks = 0;
    h->last_exact = 0;
    h->last_dropped = 0;
    h->fb_pending = false;
    return FX_OK;
}

// the selector's counts on the host (waits for its build once)
int selector_counts(const FxSelector* sel) {
    std::lock_guard<std::mutex> lk(sel->mu);
    if (sel->known) return FX_OK;
    DeviceGuard g(sel->device);
    HIP_TRY(hipEventSynchronize(sel->ready));
    sel->rows = sel->pin->rows;
    sel->ntiles = sel->pin->tiles;
    sel->known = true;
    return FX_OK;
}

// ---- remove_ids (fx_remove.hip): the host's chunk plan ----------------------

// Kept rows before row r, for the rows the plan asks about: any row (the
// prefix and mask words on the host; only for a staging buffer smaller than
// RM_GROUP_ROWS rows) or the multiples of RM_GROUP_ROWS, the first removed
// row and ntotal (the device's gp words).
struct KeptPrefix {
    int64_t ntotal = 0, first = 0, kept = 0;
    int64_t g = RM_GROUP_ROWS;  // the plan's boundary granule: RM_GROUP_ROWS (gp) or 1 (words + mask)
    std::vector<unsigned> gp, words, mask;
    int64_t at(int64_t r) const {
        if (r >= ntotal) return kept;
        if (r <= first) return r;  // no row below the first removed one is removed
        if (g == 1) return (int64_t)words[r >> 5] + __builtin_popcount(~mask[r >> 5] & ((1u << (r & 31)) - 1u));
        return gp[r / RM_GROUP_ROWS];
    }
};

struct RemoveChunk {
    int64_t s0, s1;  // source rows
    int64_t d0, kept;  // its kept rows go to rows [d0, d0 + kept)
    bool direct;     // d0 + kept <= s0: moved in place by one launch; else gathered into staging, then copied
};

// Ascending chunks of source rows from the first removed row to ntotal, cut at
// multiples of P.g.  From s0 (kept rows before it: d0) the candidates are the
// longest direct chunk (the largest boundary s1 with prefix(s1) <= s0) and the
// longest staged one (prefix(s1) - d0 <= stage_rows); the direct one is taken
// when it is at least half as long (a staged row moves twice), so small
// shifts do not turn into many small launches.  Chunks without a kept row are
// skipped.  false: a boundary step holds more kept rows than the staging
// buffer (never: the caller picks g <= stage_rows).
bool plan_remove(const KeptPrefix& P, int64_t stage_rows, std::vector<RemoveChunk>& out) {
    const int64_t g = P.g, nt = P.ntotal;
    const int64_t nb = (nt + g - 1) / g;  // boundary i is row min(nt, i g)
    auto row = [&](int64_t i) { return std::min(nt, i * g); };
    int64_t s0 = P.first;
    while (s0 < nt) {
        const int64_t d0 = P.at(s0);
        const int64_t i0 = s0 / g + 1;  // the first boundary above s0
        // the largest boundary in [i0, nb] where pred holds (pred: true up to some row, false after); i0 - 1: none
        auto last = [&](auto pred) {
            int64_t lo = i0 - 1, hi = nb;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo + 1) / 2;
                if (pred(row(mid))) lo = mid;
                else hi = mid - 1;
            }
            return lo;
        };
        const int64_t id = last([&](int64_t r) { return P.at(r) <= s0; });
        const int64_t is = last([&](int64_t r) { return P.at(r) - d0 <= stage_rows; });
        if (is < i0) return false;
        const int64_t s1d = id >= i0 ? row(id) : s0, s1s = row(is);
        const bool direct = s1d > s0 && (s1d - s0) * 2 >= s1s - s0;
        const int64_t s1 = direct ? s1d : s1s;
        const int64_t kept = P.at(s1) - d0;
        if (kept > 0) out.push_back({s0, s1, d0, kept, direct});
        s0 = s1;
    }
    return true;
}

// The compaction itself: the index's rows under sel's mask (sel->rows > 0 of
// them removed), then the invariants of grow() / fx_index_reset on the freed
// tail, the recomputed norm maximum and the scan image's bookkeeping.
int remove_rows(FxIndex* h, const FxSelector* sel) {
    hipStream_t s = h->stream();
    const int64_t nt = h->ntotal, rb = h->row_bytes;
    const int64_t nw = sel_mask_words(nt), ngp = rm_groups(nt), nblk = rm_prefix_blocks(nt);
    int64_t stage_bytes = h->opt.remove_stage;
    if (stage_bytes < rb || stage_bytes > REMOVE_STAGE_MAX) stage_bytes = REMOVE_STAGE_DEFAULT;
    const int64_t stage_rows = std::min(std::max<int64_t>(stage_bytes / rb, 1), nt);
    HIP_TRY(h->rm_ws.ensure((size_t)(nw + ngp + nblk + 4 + stage_rows) * 4));
    unsigned* prefix = (unsigned*)h->rm_ws.p;
    unsigned* gp = prefix + nw;
    unsigned* bsum = gp + ngp;
    unsigned* info = bsum + nblk;
    float* nstage = (float*)(info + 4);
    HIP_TRY(launch_keep_prefix(sel->mask, nt, prefix, gp, bsum, info, s));
    unsigned hinfo[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(hinfo, info, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    KeptPrefix P;
    P.ntotal = nt;
    P.first = hinfo[0];
    P.kept = hinfo[1];
    if (P.first >= nt || P.kept != nt - sel->rows)
        return set_err(FX_E_INTEGRITY, "remove_ids: the mask's scan gives first removed row %lld, %lld kept of %lld rows; "
                       "the selector counted %lld selected", (long long)P.first, (long long)P.kept, (long long)nt,
                       (long long)sel->rows);
    P.g = stage_rows < std::min<int64_t>(RM_GROUP_ROWS, nt) ? 1 : RM_GROUP_ROWS;
    if (P.g == 1) {
        P.words.resize((size_t)nw);
        P.mask.resize((size_t)nw);
        HIP_TRY(hipMemcpyAsync(P.words.data(), prefix, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(P.mask.data(), sel->mask, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
    } else {
        P.gp.resize((size_t)ngp);
        HIP_TRY(hipMemcpyAsync(P.gp.data(), gp, (size_t)ngp * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<RemoveChunk> plan;
    if (!plan_remove(P, stage_rows, plan)) return set_err(FX_E_INTEGRITY, "remove_ids: no chunk plan within the staging buffer");
    int64_t staged_max = 0;
    for (const RemoveChunk& c : plan)
        if (!c.direct) staged_max = std::max(staged_max, c.kept);
    if (staged_max > stage_rows) return set_err(FX_E_INTEGRITY, "remove_ids: a staged chunk exceeds the staging buffer");
    if (staged_max > 0) HIP_TRY(h->stage.ensure((size_t)staged_max * rb));
    h->rm_stats[0] = P.first;
    h->rm_stats[1] = h->rm_stats[2] = 0;
    h->rm_stats[3] = (int64_t)plan.size();
    for (const RemoveChunk& c : plan) h->rm_stats[c.direct ? 1 : 2] += c.kept;
    for (const RemoveChunk& c : plan) {
        if (c.direct) {
            HIP_TRY(launch_move_rows(h->codes, h->norms, sel->mask, prefix, nt, (int)rb, c.s0, c.s1, h->codes, h->norms, 0, s));
        } else {
            HIP_TRY(launch_move_rows(h->codes, h->norms, sel->mask, prefix, nt, (int)rb, c.s0, c.s1, (char*)h->stage.p,
                                     nstage, c.d0, s));
            HIP_TRY(hipMemcpyAsync(h->codes + (size_t)c.d0 * rb, h->stage.p, (size_t)c.kept * rb, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h->norms + c.d0, nstage, (size_t)c.kept * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    const int64_t newn = P.kept;
    if (h->has_ids) {
        // the labels follow their rows: compacted out of place into the second buffer, which takes over
        // (searches enqueued before this call are done with the old one: the sync below precedes any reuse)
        if (!h->labels_alt || h->label_alt_cap < h->label_cap) {
            if (h->labels_alt) (void)hipFree(h->labels_alt);
            h->labels_alt = nullptr;
            h->label_alt_cap = 0;
            HIP_TRY(hipMalloc((void**)&h->labels_alt, (size_t)h->label_cap * 8));
            h->label_alt_cap = h->label_cap;
        }
        HIP_TRY(launch_compact_labels(h->labels, sel->mask, prefix, nt, h->labels_alt, s));
        std::swap(h->labels, h->labels_alt);
        std::swap(h->label_cap, h->label_alt_cap);
    }
    // the freed tail: zero rows, +inf norms (grow / fx_index_reset)
    HIP_TRY(hipMemsetAsync(h->codes + (size_t)newn * rb, 0, (size_t)(nt - newn) * rb, s));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(h->norms + newn), 0x7f800000u, (size_t)(nt - newn), s));
    // max |y|^2 over the kept rows (a removed outlier's would keep the certification bound E wide for good)
    HIP_TRY(hipMemsetAsync(h->max_sq_bits, 0, 4, s));
    HIP_TRY(launch_norm_max(h->norms, newn, h->max_sq_bits, s));
    // scan image: rows below the first removed one stay valid for the unchanged centre; update_scan_image
    // rebuilds the rest at the next search.  Its freed tail: +inf row constants, zero F32S rows.
    h->img_rows = std::min(h->img_rows, P.first);
    if (h->cnorms.p) {
        const int64_t hi = std::min<int64_t>(nt, (int64_t)(h->cnorms.bytes / 4));
        if (newn < hi)
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)((float*)h->cnorms.p + newn), 0x7f800000u, (size_t)(hi - newn), s));
        if (h->img_kind != IMG_NONE) {  // ... and its maximum over the rows that stay
            HIP_TRY(hipMemsetAsync(h->max_sq_bits + 1, 0, 4, s));
            HIP_TRY(launch_norm_max((const float*)h->cnorms.p, std::min<int64_t>(h->img_rows, hi), h->max_sq_bits + 1, s));
        }
    }
    if (h->split.p) {
        const int64_t hi = std::min<int64_t>(nt, (int64_t)(h->split.bytes / rb));
        if (newn < hi) HIP_TRY(hipMemsetAsync((char*)h->split.p + (size_t)newn * rb, 0, (size_t)(hi - newn) * rb, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->ntotal = newn;
    if (newn == 0) h->mu_rows = 0;  // as fx_index_reset leaves it
    ++h->epoch;
    h->rg_nq = -1;  // the last range search's result named the old rows
    h->rg_total = 0;
    graph_release(h);  // (its key would not notice a removal followed by an add of as many rows)
    return FX_OK;
}

}  // namespace

extern "C" {

const char* fx_last_error(void) { return g_err.c_str(); }

int fx_device_count(int* out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return set_err(FX_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out = n;
    return FX_OK;
}

int fx_index_create(int d, int storage_dtype, int metric, int device, FxIndex** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (!check_dtype(storage_dtype)) return set_err(FX_E_ARG, "bad storage dtype %d", storage_dtype);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT)
        return set_err(FX_E_ARG, "bad metric %d", metric);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(FX_E_HIP, "device %d not available (%d devices)", device, n);
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    FxIndex* h = new FxIndex();
    h->d = d;
    h->dtype = storage_dtype;
    h->metric = metric;
    h->device = device;
    h->row_bytes = (int)round_up((int64_t)d * dtype_size(storage_dtype), ROW_ALIGN);
    h->kdim = h->row_bytes / dtype_size(storage_dtype);
    h->opt.from_env();
    // A BLOCKING stream: work on the legacy null stream (torch's default
    // stream, cuda_stream == 0) is ordered before and after it, so a caller
    // that binds "stream 0" (fx_index_set_stream(h, NULL)) stays ordered.
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&h->max_sq_bits, 16);
    if (e == hipSuccess) e = hipMemset(h->max_sq_bits, 0, 16);
    if (e == hipSuccess) e = hipMalloc(&h->dev_drop, 16);
    if (e == hipSuccess) e = hipMemset(h->dev_drop, 0, 16);
    if (e != hipSuccess) {
        fx_index_free(h);
        return set_err(FX_E_HIP, "index init: %s", hipGetErrorString(e));
    }
    *out = h;
    return FX_OK;
}

void fx_index_free(FxIndex* h) {
    if (!h) return;
    {
        DeviceGuard g(h->device);
        if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
        if (h->user_stream) (void)hipStreamSynchronize(h->user_stream);
        if (h->codes) (void)hipFree(h->codes);
        if (h->norms) (void)hipFree(h->norms);
        if (h->labels) (void)hipFree(h->labels);
        if (h->labels_alt) (void)hipFree(h->labels_alt);
        h->idm_ws.release();
        if (h->max_sq_bits) (void)hipFree(h->max_sq_bits);
        if (h->dev_drop) (void)hipFree(h->dev_drop);
        for (DevBuf* b : {&h->qin, &h->qf32, &h->qop, &h->qeps, &h->cand_d, &h->cand_i, &h->dws, &h->iws, &h->flag,
                          &h->fbc_d, &h->fbc_i, &h->stage, &h->gtau, &h->trace, &h->dbgbuf, &h->split, &h->cnorms,
                          &h->centre, &h->mu_part, &h->qshift, &h->qrho, &h->stamps, &h->pub, &h->cand2_d,
                          &h->cand2_i, &h->rq_f32, &h->rq_op, &h->rq_eps, &h->rq_rho, &h->rq_shift, &h->rq_gtau,
                          &h->rq_cand_d, &h->rq_cand_i, &h->rq_flag, &h->hk_ws, &h->hout, &h->conv, &h->rg_qin,
                          &h->rg_qf32, &h->rg_qop, &h->rg_eps, &h->rg_rho, &h->rg_shift, &h->rg_thr, &h->rg_cnt,
                          &h->rg_cand, &h->rg_dist, &h->rg_sorted, &h->rg_temp, &h->rg_lims, &h->rg_D, &h->rg_I,
                          &h->rm_ws, &h->rc_in, &h->rc_rows, &h->rc_qf32, &h->rc_out, &h->km_ws, &h->km_out, &h->km_x,
                          &h->km_h})
            b->release();
        graph_release(h);
        if (h->ghq) (void)hipHostFree(h->ghq);
        if (h->ghout) (void)hipHostFree(h->ghout);
        if (h->hpin) (void)hipHostFree(h->hpin);
        if (h->qpin) (void)hipHostFree(h->qpin);
        if (h->pin_nf) (void)hipHostFree(h->pin_nf);
        if (h->km_pin) (void)hipHostFree(h->km_pin);
        if (h->km_bad) (void)hipFree(h->km_bad);
        if (h->km_bad_pin) (void)hipHostFree(h->km_bad_pin);
        for (hipEvent_t e : h->km_ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : h->km_ev_fin) (void)hipEventDestroy(e);
        for (auto& pr : h->ev_scan) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (auto& pr : h->ev_merge) (void)hipEventDestroy(pr.second);
        if (h->switch_ev) (void)hipEventDestroy(h->switch_ev);
        if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    }
    delete h;
}

int fx_index_set_normalize(FxIndex* h, int on) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    h->normalize = on ? 1 : 0;
    return FX_OK;
}

int fx_index_set_stream(FxIndex* h, void* stream) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    const hipStream_t prev = h->stream();
    h->user_stream = (hipStream_t)stream;
    const hipStream_t next = h->stream();
    if (next != prev) {
        // the index's work stays in call order across a stream switch: the new
        // stream waits (on the device) for everything enqueued on the old one
        DeviceGuard g(h->device);
        HIP_TRY(hipEventRecord(h->switch_ev, prev));
        HIP_TRY(hipStreamWaitEvent(next, h->switch_ev, 0));
    }
    return FX_OK;
}

int fx_index_set_option(FxIndex* h, const char* name, int64_t value) {
    if (!h || !name) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (strcmp(name, "remove_stage") == 0) {  // (bytes: the one option wider than an int)
        if (value != 0 && (value < h->row_bytes || value > REMOVE_STAGE_MAX))
            return set_err(FX_E_ARG, "option 'remove_stage': value out of range (%lld; 0 or %d .. %lld bytes)",
                           (long long)value, h->row_bytes, (long long)REMOVE_STAGE_MAX);
        h->opt.remove_stage = value;
        return FX_OK;
    }
    const char* why = nullptr;
    int* slot = h->opt.find(name, value, &why);
    if (!slot) return set_err(FX_E_ARG, "unknown option '%s'", name);
    if (why) return set_err(FX_E_ARG, "option '%s': %s (%lld)", name, why, (long long)value);
    if (slot == &h->opt.range_cap && h->rg_cand.p) {
        // the next range search starts from the new capacity
        DeviceGuard g(h->device);
        HIP_TRY(hipStreamSynchronize(h->stream()));
        h->rg_cand.release();
    }
    *slot = (int)value;
    return FX_OK;
}

int fx_index_set_id_offset(FxIndex* h, int64_t off) {
    if (!h || off < 0) return set_err(FX_E_ARG, "bad index/offset");
    std::lock_guard<std::mutex> lk(h->mu);
    if (off != 0 && h->has_ids)
        return set_err(FX_E_ARG, "set_id_offset: the index carries labels (add_with_ids); ids are the labels, not row + offset");
    h->id_offset = off;
    return FX_OK;
}

int fx_index_dim(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->d;
    return FX_OK;
}
int fx_index_ntotal(const FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->ntotal;
    return FX_OK;
}
int fx_index_storage_dtype(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->dtype;
    return FX_OK;
}
int fx_index_metric(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->metric;
    return FX_OK;
}

int fx_index_reserve(FxIndex* h, int64_t n) {
    if (!h || n < 0) return set_err(FX_E_ARG, "bad reserve");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(grow(h, n));
    return FX_OK;
}

// the append of fx_index_add / fx_index_add_with_ids (arguments validated, the
// index locked): rows [ntotal, ntotal + n) <- x; ntotal is the caller's to advance
static int append_rows(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    hipStream_t s = h->stream();
    HIP_TRY(grow(h, h->ntotal + n));
    const size_t xes = dtype_size(x_dtype);
    if (x_mem == FX_MEM_DEVICE) {
        HIP_TRY(launch_convert_rows(x, x_dtype, n, h->d, h->codes + (size_t)h->ntotal * h->row_bytes, h->dtype,
                                    h->kdim, h->norms + h->ntotal, h->max_sq_bits, h->normalize, s));
    } else {
        // stream host rows through a bounded staging buffer (<= 256 MiB)
        const int64_t chunk = std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * xes));
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t nr = std::min(chunk, n - r0);
            HIP_TRY(h->stage.ensure((size_t)nr * h->d * xes));
            HIP_TRY(hipMemcpyAsync(h->stage.p, (const char*)x + (size_t)r0 * h->d * xes, (size_t)nr * h->d * xes,
                                   hipMemcpyHostToDevice, s));
            HIP_TRY(launch_convert_rows(h->stage.p, x_dtype, nr, h->d,
                                        h->codes + (size_t)(h->ntotal + r0) * h->row_bytes, h->dtype, h->kdim,
                                        h->norms + h->ntotal + r0, h->max_sq_bits, h->normalize, s));
            HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
        }
    }
    return FX_OK;
}

static int check_add_args(const FxIndex* h, int64_t n, const void* x, int x_dtype) {
    if (!x) return set_err(FX_E_ARG, "null x");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if ((int64_t)h->ntotal + n >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "more than 2^31-1 rows per shard");
    return FX_OK;
}

int fx_index_add(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (n == 0) return FX_OK;
    if (const int rc = check_add_args(h, n, x, x_dtype); rc != FX_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->has_ids && h->ntotal > 0)
        return set_err(FX_E_ARG, "add does not make sense on an index with labels: use add_with_ids");
    h->has_ids = false;  // the first add into an empty index decides the mode
    DeviceGuard g(h->device);
    if (const int rc = append_rows(h, n, x, x_dtype, x_mem); rc != FX_OK) return rc;
    h->ntotal += n;
    return FX_OK;
}

// ---- stable ids (fx_idmap.hip) ----------------------------------------------

int fx_index_add_with_ids(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids,
                          int ids_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (n == 0) return FX_OK;
    if (!ids) return set_err(FX_E_ARG, "add_with_ids: null ids");
    if (ids_mem != FX_MEM_HOST && ids_mem != FX_MEM_DEVICE) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (const int rc = check_add_args(h, n, x, x_dtype); rc != FX_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids && h->ntotal > 0)
        return set_err(FX_E_ARG, "add_with_ids not implemented for an index that holds rows without labels");
    if (h->id_offset != 0)
        return set_err(FX_E_ARG, "add_with_ids: the index has id offset %lld; labels and an id offset exclude each other",
                       (long long)h->id_offset);
    DeviceGuard g(h->device);
    const bool was = h->has_ids;
    h->has_ids = true;  // (grow carries / allocates the label buffer from here on)
    int rc = append_rows(h, n, x, x_dtype, x_mem);
    if (rc == FX_OK) {
        hipStream_t s = h->stream();
        hipError_t e = hipMemcpyAsync(h->labels + h->ntotal, ids, (size_t)n * 8,
                                      ids_mem == FX_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s);
        // (host ids: the caller's array may go when the call returns)
        if (e == hipSuccess && ids_mem == FX_MEM_HOST) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = set_err(FX_E_HIP, "add_with_ids: copying the labels: %s", hipGetErrorString(e));
    }
    if (rc != FX_OK) {
        h->has_ids = was;
        return rc;
    }
    h->ntotal += n;
    return FX_OK;
}

int fx_index_has_ids(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->has_ids ? 1 : 0;
    return FX_OK;
}

int fx_index_get_ids(FxIndex* h, int64_t i0, int64_t n, int64_t* out, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (i0 < 0 || n < 0) return set_err(FX_E_ARG, "get_ids: negative range");
    if (out_mem != FX_MEM_HOST && out_mem != FX_MEM_DEVICE) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids) return set_err(FX_E_ARG, "get_ids: the index carries no labels (it was not filled by add_with_ids)");
    if (i0 > h->ntotal || n > h->ntotal - i0)
        return set_err(FX_E_ARG, "get_ids: rows [%lld, %lld) outside the index's %lld", (long long)i0,
                       (long long)(i0 + n), (long long)h->ntotal);
    if (n == 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(out, h->labels + i0, (size_t)n * 8,
                           out_mem == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_rows_of_ids(FxIndex* h, const int64_t* ids, int64_t n, int ids_mem, int64_t* rows, int rows_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if ((ids_mem != FX_MEM_HOST && ids_mem != FX_MEM_DEVICE) || (rows_mem != FX_MEM_HOST && rows_mem != FX_MEM_DEVICE))
        return set_err(FX_E_ARG, "bad ids_mem / rows_mem");
    if (n > 0 && (!ids || !rows)) return set_err(FX_E_ARG, "null buffer");
    if (n > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "rows_of_ids: more than 2^31-1 ids per call");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids) return set_err(FX_E_ARG, "rows_of_ids: the index carries no labels (it was not filled by add_with_ids)");
    if (n == 0) return FX_OK;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    // workspace: [sort | staged host ids | device rows of a host output]
    size_t sort_bytes = 0;
    HIP_TRY(idmap_sort_bytes(n, true, &sort_bytes));
    const size_t nb = (size_t)round_up(n * 8, 256);
    HIP_TRY(h->idm_ws.ensure(sort_bytes + 2 * nb));
    char* base = (char*)h->idm_ws.p;
    const int64_t* dids = ids;
    if (ids_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(base + sort_bytes, ids, (size_t)n * 8, hipMemcpyHostToDevice, s));
        dids = (const int64_t*)(base + sort_bytes);
    }
    int64_t* drows = rows_mem == FX_MEM_HOST ? (int64_t*)(base + sort_bytes + nb) : rows;
    HIP_TRY(launch_rows_of_labels(h->labels, h->ntotal, dids, n, drows, base, sort_bytes, s));
    if (rows_mem == FX_MEM_HOST) HIP_TRY(hipMemcpyAsync(rows, drows, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    // (host buffers on either side: the call is done with them when it returns)
    if (rows_mem == FX_MEM_HOST || ids_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                    int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    static_assert(FX_MAX_K == FX_BIG_K, "ABI k limit of the scan path = the big-k refine's");
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (h->ntotal > 0 && k > FX_MAX_K) return do_search_hugek(h, nq, q, q_dtype, q_mem, k, D, I, out_mem);
    if (h->ntotal == 0) return fill_missing(h, nq, k, D, I, out_mem);  // faiss: empty index -> every slot missing
    const Options& o = h->opt;
#ifdef FX_DIAG
    const bool diag = o.scan_dbg != 0 || !o.trace.empty() || !o.cand.empty() || !o.stamps.empty();
#else
    constexpr bool diag = false;
#endif
    if (o.search_graph == 1 && q_mem == FX_MEM_HOST && out_mem == FX_MEM_HOST && nq <= 64 && !h->profile && !diag &&
        h->user_stream == nullptr)
        return graph_search(h, nq, q, q_dtype, k, D, I);
    return do_search(h, nq, q, q_dtype, q_mem, k, D, I, out_mem);
}

// ---- filtered search (fx_select.hip) ---------------------------------------

void fx_selector_free(FxSelector* sel) {
    if (!sel) return;
    {
        DeviceGuard g(sel->device);
        if (sel->ready) {
            (void)hipEventSynchronize(sel->ready);
            (void)hipEventDestroy(sel->ready);
        }
        if (sel->mask) (void)hipFree(sel->mask);
        if (sel->tiles) (void)hipFree(sel->tiles);
        if (sel->cnt) (void)hipFree(sel->cnt);
        if (sel->pin) (void)hipHostFree(sel->pin);
    }
    delete sel;
}

int fx_selector_create(FxIndex* h, int kind, const void* data, int64_t n, int data_mem, int invert,
                       FxSelector** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (kind != FX_SEL_BITMAP && kind != FX_SEL_IDS && kind != FX_SEL_RANGE)
        return set_err(FX_E_ARG, "bad selector kind %d (FX_SEL_BITMAP 0, FX_SEL_IDS 1, FX_SEL_RANGE 2)", kind);
    if (!h) return set_err(FX_E_ARG, "null index");
    if (data_mem != FX_MEM_HOST && data_mem != FX_MEM_DEVICE) return set_err(FX_E_ARG, "bad data_mem %d", data_mem);
    int64_t imin = 0, imax = 0;
    if (kind == FX_SEL_RANGE) {
        if (!data) return set_err(FX_E_ARG, "selector: null range");
        memcpy(&imin, data, 8);
        memcpy(&imax, (const char*)data + 8, 8);
        if (imax < imin)
            return set_err(FX_E_ARG, "selector: range with imax %lld < imin %lld", (long long)imax, (long long)imin);
    } else {
        if (n < 0) return set_err(FX_E_ARG, "selector: negative n");
        if (n > 0 && !data) return set_err(FX_E_ARG, "selector: null data");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    FxSelector* sel = new FxSelector();
    sel->index = h;
    sel->device = h->device;
    sel->ntotal = h->ntotal;
    sel->epoch = h->epoch;
    const int64_t nt = h->ntotal, off = h->id_offset;
    const int64_t nwords = sel_mask_words(nt), ntiles = nwords / (TILE_R / 32);
    void* staged = nullptr;  // host data on the device for the build
    hipError_t e = hipMalloc((void**)&sel->mask, (size_t)std::max<int64_t>(nwords, 4) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&sel->tiles, (size_t)std::max<int64_t>(ntiles, 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&sel->cnt, sizeof(SelCounts));
    if (e == hipSuccess) e = hipHostMalloc((void**)&sel->pin, sizeof(SelCounts), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sel->ready, hipEventDisableTiming);
    // a labelled index (fx_idmap.hip): ids, range bounds and bitmap bits mean labels
    const int64_t* labels = h->has_ids ? h->labels : nullptr;
    if (e == hipSuccess && labels && nt > 0) {
        if (kind == FX_SEL_RANGE) {
            e = launch_sel_range_lbl(labels, imin, imax, nt, invert != 0, sel->mask, s);
        } else {
            const size_t bytes = (size_t)n * (kind == FX_SEL_IDS ? 8 : 1);
            // index-owned scratch: [sort workspace of the id list | host data staged for the build]
            size_t sort_bytes = 0;
            if (kind == FX_SEL_IDS && n > 0) {
                if (n > (int64_t)INT32_MAX) e = hipErrorInvalidValue;
                else e = idmap_sort_bytes(n, false, &sort_bytes);
            }
            const bool stage = data_mem == FX_MEM_HOST && n > 0;
            if (e == hipSuccess && sort_bytes + (stage ? bytes : 0) > 0)
                e = h->idm_ws.ensure(sort_bytes + (stage ? bytes : 0));
            const void* dev = data;
            if (e == hipSuccess && stage) {
                dev = (char*)h->idm_ws.p + sort_bytes;
                e = hipMemcpyAsync((void*)dev, data, bytes, hipMemcpyHostToDevice, s);
            }
            if (e == hipSuccess)
                e = kind == FX_SEL_IDS
                        ? launch_sel_ids_lbl(labels, (const int64_t*)dev, n, nt, invert != 0, sel->mask, h->idm_ws.p,
                                             sort_bytes, s)
                        : launch_sel_bitmap_lbl(labels, (const uint8_t*)dev, n, nt, invert != 0, sel->mask, s);
            // (host data: the pageable copy above has to be out of the caller's array before the call returns)
            if (e == hipSuccess && stage) e = hipStreamSynchronize(s);
        }
    } else if (e == hipSuccess && kind == FX_SEL_RANGE) {
        // ids -> local rows, clamped to the index (id_offset >= 0; differences of int64 ids may not overflow)
        auto local = [&](int64_t id) { return id <= off ? (int64_t)0 : std::min(id - off, nt); };
        e = launch_sel_range(local(imin), local(imax), nt, invert != 0, sel->mask, s);
    } else if (e == hipSuccess) {
        const size_t bytes = (size_t)n * (kind == FX_SEL_IDS ? 8 : 1);
        const void* dev = data;
        if (data_mem == FX_MEM_HOST && n > 0) {
            e = hipMalloc(&staged, bytes);
            if (e == hipSuccess) e = hipMemcpyAsync(staged, data, bytes, hipMemcpyHostToDevice, s);
            dev = staged;
        }
        if (e == hipSuccess)
            e = kind == FX_SEL_IDS ? launch_sel_ids((const int64_t*)dev, n, off, nt, invert != 0, sel->mask, s)
                                   : launch_sel_bitmap((const uint8_t*)dev, n, off, nt, invert != 0, sel->mask, s);
    }
    if (e == hipSuccess) e = launch_sel_tiles(sel->mask, nt, sel->tiles, sel->cnt, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sel->pin, sel->cnt, sizeof(SelCounts), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(sel->ready, s);
    if (staged) {  // host data: the build has to finish before the staging copy goes
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(staged);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fx_selector_free(sel);
        return set_err(FX_E_HIP, "selector build: %s", hipGetErrorString(e));
    }
    *out = sel;
    return FX_OK;
}

int fx_selector_stats(const FxSelector* sel, int64_t* rows, int64_t* tiles) {
    if (!sel || !rows || !tiles) return set_err(FX_E_ARG, "null argument");
    const int rc = selector_counts(sel);
    if (rc != FX_OK) return rc;
    *rows = sel->rows;
    *tiles = sel->ntiles;
    return FX_OK;
}

int fx_index_search_sel(FxIndex* h, const FxSelector* sel, int64_t nq, const void* q, int q_dtype, int q_mem, int k,
                        float* D, int64_t* I, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (!sel) return set_err(FX_E_ARG, "null selector");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (sel->index != h) return set_err(FX_E_ARG, "search: the selector was created on another index");
    if (k > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "search with a selector supports k <= %d (got %d): the exact sort path takes none",
                       FX_MAX_K, k);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (sel->ntotal != h->ntotal || sel->epoch != h->epoch)
        return set_err(FX_E_ARG, "search: stale selector: it is a snapshot of %lld rows, the index now has %lld "
                       "(rows were added or the index was reset since it was created)",
                       (long long)sel->ntotal, (long long)h->ntotal);
    DeviceGuard g(h->device);
    {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    // nothing selected (or an empty index): every slot missing, no scan
    if (h->ntotal == 0 || sel->rows == 0) return fill_missing(h, nq, k, D, I, out_mem);
    return do_search(h, nq, q, q_dtype, q_mem, k, D, I, out_mem, sel);
}

// ---- remove_ids (fx_remove.hip) --------------------------------------------

int fx_index_remove_ids(FxIndex* h, const FxSelector* sel, int64_t* n_removed) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (!sel) return set_err(FX_E_ARG, "null selector");
    if (!n_removed) return set_err(FX_E_ARG, "null n_removed");
    *n_removed = 0;
    if (sel->index != h) return set_err(FX_E_ARG, "remove_ids: the selector was created on another index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (sel->ntotal != h->ntotal || sel->epoch != h->epoch)
        return set_err(FX_E_ARG, "remove_ids: stale selector: it is a snapshot of %lld rows, the index now has %lld "
                       "(rows were added or removed, or the index was reset since it was created)",
                       (long long)sel->ntotal, (long long)h->ntotal);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    if (h->ntotal == 0 || sel->rows == 0) return FX_OK;  // nothing selected: nothing changes, the selector stays valid
    const int rc = remove_rows(h, sel);
    if (rc != FX_OK) return rc;
    *n_removed = sel->rows;
    return FX_OK;
}

int fx_index_last_remove_stats(FxIndex* h, int64_t* first, int64_t* direct_rows, int64_t* staged_rows, int64_t* chunks) {
    if (!h || !first || !direct_rows || !staged_rows || !chunks) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *first = h->rm_stats[0];
    *direct_rows = h->rm_stats[1];
    *staged_rows = h->rm_stats[2];
    *chunks = h->rm_stats[3];
    return FX_OK;
}

// the counts of the last search (after a device-resident one: synchronises the
// index stream, which is ordered after every stream the index used before)
static int read_counts(FxIndex* h) {
    if (h->fb_pending) {
        DeviceGuard g(h->device);
        HIP_TRY(hipStreamSynchronize(h->stream()));
        h->last_fallbacks = h->pin_nf[0];
        h->last_exact = h->pin_nf[1];
        h->last_dropped = h->pin_nf[2];
        h->fb_pending = false;
        if (h->last_dropped > 0) return integrity_error(h);
    }
    return FX_OK;
}

int fx_index_last_dropped_candidates(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_dropped;
    return FX_OK;
}

int fx_index_last_fallbacks(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_fallbacks;
    return FX_OK;
}

int fx_index_last_scan_plan(FxIndex* h, int* tile_rows, int* query_tile, int* splits) {
    if (!h || !tile_rows || !query_tile || !splits) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *tile_rows = h->last_plan[0];
    *query_tile = h->last_plan[1];
    *splits = h->last_plan[2];
    return FX_OK;
}

int fx_index_last_exact_fallbacks(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_exact;
    return FX_OK;
}

// ---- range_search (fx_range.hip) ------------------------------------------

// the range scan's grid: 128-query tiles x corpus splits, sized and placed by
// plan_splits as plan_scan's 128-row scans are (>= 3 tiles per split; corpus-
// partitioned over the XCDs once there are 8 x 3 tiles), from the shape
// alone -- no option enters, so none can change a result
static void plan_range_scan(const FxIndex* h, int64_t nq, ScanParams& p) {
    p.qt = TILE_Q;
    p.tr = TILE_R;
    p.n_qtiles = (int)((nq + TILE_Q - 1) / TILE_Q);
    p.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
    plan_splits(p.n_qtiles, p.n_ctiles, 3, true, false).store(p);
}

static int range_store_empty(FxIndex* h, int64_t nq, int64_t* lims) {
    // no row can qualify: all-zero lims on the host and on the device
    HIP_TRY(h->rg_lims.ensure((size_t)(nq + 1) * 8));
    HIP_TRY(hipMemsetAsync(h->rg_lims.p, 0, (size_t)(nq + 1) * 8, h->stream()));
    HIP_TRY(hipStreamSynchronize(h->stream()));
    std::fill(lims, lims + nq + 1, (int64_t)0);
    h->rg_nq = nq;
    h->rg_total = 0;
    return FX_OK;
}

// DevBuf growth of the range path: an allocation failure is FX_E_OOM
#define RG_ALLOC(buf, want)                                                                          \
    do {                                                                                             \
        if ((buf).ensure(want) != hipSuccess) {                                                      \
            (void)hipGetLastError();                                                                 \
            return set_err(FX_E_OOM, "range_search: cannot allocate %zu bytes (%s)", (size_t)(want), #buf); \
        }                                                                                            \
    } while (0)

int fx_index_range_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, float radius,
                          int64_t* lims) {
    if (radius != radius) return set_err(FX_E_ARG, "range_search: radius is NaN");
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (nq >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "range_search: more than 2^31-1 queries per call");
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!lims) return set_err(FX_E_ARG, "null lims");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    {   // the counts of a device-resident search still in flight are read first:
        // this call reuses the dropped-ids word
        const int rc = read_counts(h);
        if (rc != FX_OK) return rc;
    }
    h->rg_nq = -1;
    h->rg_total = 0;
    h->rg_cands = 0;
    h->rg_passes = 0;
    if (nq == 0) {
        lims[0] = 0;
        h->rg_nq = 0;
        return FX_OK;
    }
    if (!q) return set_err(FX_E_ARG, "null buffer");
    // L2 distances are >= 0 and the test is strict: radius <= 0 takes no row
    if (h->ntotal == 0 || (h->metric == L2 && radius <= 0.0f)) return range_store_empty(h, nq, lims);

    hipStream_t s = h->stream();
    const void* qdev = q;
    if (q_mem == FX_MEM_HOST) {
        const size_t qb = (size_t)nq * h->d * dtype_size(q_dtype);
        RG_ALLOC(h->rg_qin, qb);
        HIP_TRY(hipMemcpyAsync(h->rg_qin.p, q, qb, hipMemcpyHostToDevice, s));
        qdev = h->rg_qin.p;
    }
    const int64_t nq_pad = round_up(nq, QPAD);
    RG_ALLOC(h->rg_qf32, (size_t)nq_pad * h->kdim * 4);
    RG_ALLOC(h->rg_qop, (size_t)nq_pad * h->row_bytes);
    RG_ALLOC(h->rg_eps, (size_t)nq * 4);
    RG_ALLOC(h->rg_rho, (size_t)nq * 4);
    RG_ALLOC(h->rg_shift, (size_t)nq * 8);
    RG_ALLOC(h->rg_thr, (size_t)nq * 4);
    RG_ALLOC(h->rg_cnt, 8);
    RG_ALLOC(h->rg_lims, (size_t)(nq + 1) * 8);
    const uint64_t want_cap = h->opt.range_cap > 0 ? (uint64_t)h->opt.range_cap : (uint64_t)RANGE_CAP_DEFAULT;
    RG_ALLOC(h->rg_cand, (size_t)want_cap * 8);

    // query preparation in its no-image mode: the operand of the stored rows'
    // dtype, uncentred, bound terms against max |y|^2
    PrepParams pp{};
    pp.q = qdev;
    pp.q_dt = q_dtype;
    pp.nq = nq;
    pp.nq_pad = nq_pad;
    pp.d = h->d;
    pp.kdim = h->kdim;
    pp.st_dt = h->dtype;
    pp.metric = h->metric;
    pp.qf32 = (float*)h->rg_qf32.p;
    pp.qop = h->rg_qop.p;
    pp.qeps = (float*)h->rg_eps.p;
    pp.qrho = (float*)h->rg_rho.p;
    pp.qshift = (double*)h->rg_shift.p;
    pp.mbits = h->max_sq_bits;
    pp.img_bits = h->max_sq_bits;
    pp.zero[0] = h->dev_drop;
    HIP_TRY(launch_prep_queries(pp, s));
    HIP_TRY(launch_range_thr(nq, h->metric, radius, pp.qeps, pp.qrho, pp.qshift, (float*)h->rg_thr.p, s));

    ScanParams sp{};
    sp.codes = h->codes;
    sp.norms = h->norms;
    sp.ntotal = h->ntotal;
    sp.row_bytes = h->row_bytes;
    sp.qop = (const char*)h->rg_qop.p;
    sp.nq = nq;
    plan_range_scan(h, nq, sp);

    // the scan; when it counted more candidates than the buffer holds, the
    // buffer grows to the count and the scan runs once more (the count does
    // not depend on the capacity, so the second pass fits)
    uint64_t count = 0;
    for (int pass = 1; pass <= 2; ++pass) {
        const uint64_t cap = h->rg_cand.bytes / 8;
        HIP_TRY(hipMemsetAsync(h->rg_cnt.p, 0, 8, s));
        HIP_TRY(launch_range_scan(h->dtype, h->metric, sp, (const float*)h->rg_thr.p, (uint64_t*)h->rg_cand.p, cap,
                                  (uint64_t*)h->rg_cnt.p, s));
        HIP_TRY(hipMemcpyAsync(&count, h->rg_cnt.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->rg_passes = pass;
        if (count <= cap) break;
        if (pass == 2)
            return set_err(FX_E_INTEGRITY, "range_search: the second scan pass counted %llu candidates for %llu slots",
                           (unsigned long long)count, (unsigned long long)cap);
        if (count > (uint64_t)INT32_MAX)
            return set_err(FX_E_UNSUPPORTED, "range_search: %llu candidate pairs in one call (limit 2^31-1): "
                           "search fewer queries per call", (unsigned long long)count);
        RG_ALLOC(h->rg_cand, (size_t)count * 8);
    }
    h->rg_cands = (int64_t)count;
    if (count == 0) return range_store_empty(h, nq, lims);

    RangeFinish f{};
    f.n = (int64_t)count;
    HIP_TRY(range_sort_temp_bytes(f.n, nq, &f.temp_bytes));
    RG_ALLOC(h->rg_dist, (size_t)count * 4);
    RG_ALLOC(h->rg_sorted, (size_t)count * 8);
    RG_ALLOC(h->rg_temp, std::max<size_t>(f.temp_bytes, 16));
    RG_ALLOC(h->rg_D, (size_t)count * 4);
    RG_ALLOC(h->rg_I, (size_t)count * 8);
    f.words = (uint64_t*)h->rg_cand.p;
    f.codes = h->codes;
    f.row_bytes = h->row_bytes;
    f.kdim = h->kdim;
    f.st_dt = h->dtype;
    f.metric = h->metric;
    f.ntotal = h->ntotal;
    f.qf32 = pp.qf32;
    f.nq = nq;
    f.radius = radius;
    f.id_offset = h->id_offset;
    f.labels = h->has_ids ? h->labels : nullptr;
    f.dist = (float*)h->rg_dist.p;
    f.sorted = (uint64_t*)h->rg_sorted.p;
    f.temp = h->rg_temp.p;
    f.n_drop = h->dev_drop;
    f.lims = (int64_t*)h->rg_lims.p;
    f.D = (float*)h->rg_D.p;
    f.I = (int64_t*)h->rg_I.p;
    HIP_TRY(launch_range_finish(f, s));
    int dropped = 0;
    HIP_TRY(hipMemcpyAsync(lims, f.lims, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&dropped, h->dev_drop, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->last_dropped = dropped;
    if (dropped > 0) return integrity_error(h);
    h->rg_nq = nq;
    h->rg_total = lims[nq];
    return FX_OK;
}
#undef RG_ALLOC

int fx_index_range_result(FxIndex* h, float* D, int64_t* I, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->rg_nq < 0) return set_err(FX_E_ARG, "range_result: no range search result is stored");
    if (h->rg_total == 0) return FX_OK;
    if (!D || !I) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const hipMemcpyKind kind = out_mem == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(D, h->rg_D.p, (size_t)h->rg_total * 4, kind, s));
    HIP_TRY(hipMemcpyAsync(I, h->rg_I.p, (size_t)h->rg_total * 8, kind, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_last_range_stats(FxIndex* h, int64_t* candidates, int* passes) {
    if (!h || !candidates || !passes) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *candidates = h->rg_cands;
    *passes = h->rg_passes;
    return FX_OK;
}

int fx_index_reset(FxIndex* h) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    HIP_TRY(hipMemset(h->max_sq_bits, 0, 8));
    if (h->codes && h->cap_rows > 0) {
        HIP_TRY(hipMemset(h->codes, 0, (size_t)h->cap_rows * h->row_bytes));
        HIP_TRY(hipMemsetD32((hipDeviceptr_t)h->norms, 0x7f800000u, (size_t)h->cap_rows));
    }
    h->ntotal = 0;
    h->has_ids = false;  // the next add decides the mode again (the label buffer stays allocated)
    ++h->epoch;
    h->img_rows = 0;
    h->mu_rows = 0;
    h->rg_nq = -1;  // the last range search's result goes with the rows
    h->rg_total = 0;
    return FX_OK;
}

// ---- stored vectors and distances by key (fx_recon.hip) ---------------------

namespace {

// bytes of the bounded stage buffer a host read-back goes through per chunk
constexpr int64_t RECON_STAGE_BYTES = 128ll << 20;

// Rows by key -> host `out`, in chunks through the stage buffer (one gather,
// one device-to-host copy and one wait per chunk).  keys: n int64 on the
// device, or null for the implicit keys key0 + i.
int gather_to_host(FxIndex* h, const int64_t* keys, int64_t key0, int64_t id_offset, int64_t n, void* out,
                   int out_dtype) {
    hipStream_t s = h->stream();
    const int64_t rowb = (int64_t)h->d * dtype_size(out_dtype);
    const int64_t chunk = std::max<int64_t>(1, RECON_STAGE_BYTES / rowb);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        HIP_TRY(h->stage.ensure((size_t)(nr * rowb)));
        HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, keys ? keys + r0 : nullptr, key0 + r0,
                                   id_offset, nr, h->d, h->stage.p, out_dtype, s));
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)(r0 * rowb), h->stage.p, (size_t)(nr * rowb), hipMemcpyDeviceToHost,
                               s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

// the keys of a labelled index (n <= INT_MAX labels on the device) as rows in
// h->rc_rows: the last row of a label, -1 when none; one pass over the labels
int rows_of_keys(FxIndex* h, const int64_t* dkeys, int64_t n, const int64_t** rows) {
    size_t sort_bytes = 0;
    HIP_TRY(idmap_sort_bytes(n, true, &sort_bytes));
    HIP_TRY(h->idm_ws.ensure(sort_bytes));
    HIP_TRY(h->rc_rows.ensure((size_t)n * 8));
    HIP_TRY(launch_rows_of_labels(h->labels, h->ntotal, dkeys, n, (int64_t*)h->rc_rows.p, h->idm_ws.p, sort_bytes,
                                  h->stream()));
    *rows = (const int64_t*)h->rc_rows.p;
    return FX_OK;
}

}  // namespace

int fx_index_reconstruct_n(FxIndex* h, int64_t i0, int64_t n, float* out) {
    if (!h || !out || i0 < 0 || n < 0) return set_err(FX_E_ARG, "bad reconstruct range");
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 > h->ntotal || n > h->ntotal - i0) return set_err(FX_E_ARG, "bad reconstruct range");
    if (n == 0) return FX_OK;
    DeviceGuard g(h->device);
    // the implicit keys i0 + i of rows [i0, i0 + n)
    return gather_to_host(h, nullptr, i0, 0, n, out, FX_F32);
}

int fx_index_reconstruct_batch(FxIndex* h, int64_t n, const int64_t* keys, int keys_mem, void* out, int out_dtype,
                               int out_mem) {
    if (!check_dtype(out_dtype))
        return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: out_dtype %d is neither FX_F32 nor a storage dtype", out_dtype);
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if ((keys_mem != FX_MEM_HOST && keys_mem != FX_MEM_DEVICE) || (out_mem != FX_MEM_HOST && out_mem != FX_MEM_DEVICE))
        return set_err(FX_E_ARG, "bad keys_mem / out_mem");
    if (n > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: more than 2^31-1 keys per call");
    std::lock_guard<std::mutex> lk(h->mu);
    if (out_dtype != FX_F32 && out_dtype != h->dtype)
        return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: out_dtype %d is neither FX_F32 nor the index's storage dtype %d",
                       out_dtype, h->dtype);
    if (n == 0) return FX_OK;
    if (!keys || !out) return set_err(FX_E_ARG, "null buffer");
    // host keys of an unlabelled index are checked here, before anything is written (faiss asserts
    // key < ntotal); device keys cannot be without a sync: a bad one yields a NaN row
    if (keys_mem == FX_MEM_HOST && !h->has_ids)
        for (int64_t i = 0; i < n; ++i)
            if (keys[i] < h->id_offset || keys[i] - h->id_offset >= h->ntotal)
                return set_err(FX_E_ARG, "reconstruct_batch: key %lld (entry %lld) outside the index's ids [%lld, %lld)",
                               (long long)keys[i], (long long)i, (long long)h->id_offset,
                               (long long)(h->id_offset + h->ntotal));
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const int64_t* dkeys = keys;
    if (keys_mem == FX_MEM_HOST) {
        HIP_TRY(h->rc_in.ensure((size_t)n * 8));
        HIP_TRY(hipMemcpyAsync(h->rc_in.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, s));
        dkeys = (const int64_t*)h->rc_in.p;
    }
    int64_t id_offset = h->id_offset;
    if (h->has_ids) {  // labels -> rows (an unknown label: -1 -> a NaN row)
        const int rc = rows_of_keys(h, dkeys, n, &dkeys);
        if (rc != FX_OK) return rc;
        id_offset = 0;
    }
    if (out_mem == FX_MEM_HOST) return gather_to_host(h, dkeys, 0, id_offset, n, out, out_dtype);
    HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, dkeys, 0, id_offset, n, h->d, out,
                               out_dtype, s));
    // (host keys: the call is done with the caller's array when it returns)
    if (keys_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_search_and_reconstruct(FxIndex* h, const FxSelector* sel, int64_t nq, const void* q, int q_dtype,
                                    int q_mem, int k, float* D, int64_t* I, void* R, int r_dtype, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if ((q_mem != FX_MEM_HOST && q_mem != FX_MEM_DEVICE) || (out_mem != FX_MEM_HOST && out_mem != FX_MEM_DEVICE))
        return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (!check_dtype(r_dtype))
        return set_err(FX_E_UNSUPPORTED, "search_and_reconstruct: r_dtype %d is neither FX_F32 nor a storage dtype", r_dtype);
    if (sel && sel->index != h) return set_err(FX_E_ARG, "search: the selector was created on another index");
    if (sel && k > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "search with a selector supports k <= %d (got %d): the exact sort path takes none",
                       FX_MAX_K, k);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I || !R) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (r_dtype != FX_F32 && r_dtype != h->dtype)
        return set_err(FX_E_UNSUPPORTED, "search_and_reconstruct: r_dtype %d is neither FX_F32 nor the index's storage "
                       "dtype %d", r_dtype, h->dtype);
    if (sel && (sel->ntotal != h->ntotal || sel->epoch != h->epoch))
        return set_err(FX_E_ARG, "search: stale selector: it is a snapshot of %lld rows, the index now has %lld "
                       "(rows were added or the index was reset since it was created)",
                       (long long)sel->ntotal, (long long)h->ntotal);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    if (sel) {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    hipStream_t s = h->stream();
    const bool host_out = out_mem == FX_MEM_HOST;
    const size_t nres = (size_t)nq * k, rbytes = nres * h->d * dtype_size(r_dtype);
    // nothing to rank: every slot missing, every vector NaN
    if (h->ntotal == 0 || (sel && sel->rows == 0)) {
        const int rc = fill_missing(h, nq, k, D, I, out_mem);
        if (rc != FX_OK) return rc;
        if (host_out) memset(R, 0xff, rbytes);
        else HIP_TRY(hipMemsetAsync(R, 0xff, rbytes, s));
        return FX_OK;
    }
    // The search itself, device-resident and eager (never a search graph), reporting ROWS (+ id_offset)
    // also on a labelled index: the gather must read the row that ranked, and labels may repeat.
    float* Dd = D;
    int64_t* Id = I;
    const size_t offI = (size_t)round_up((int64_t)nres * 4, 256);
    if (host_out) {
        HIP_TRY(h->rc_out.ensure(offI + nres * 8));
        Dd = (float*)h->rc_out.p;
        Id = (int64_t*)((char*)h->rc_out.p + offI);
    }
    const int rc = !sel && k > FX_MAX_K
                       ? do_search_hugek(h, nq, q, q_dtype, q_mem, k, Dd, Id, FX_MEM_DEVICE, true)
                       : do_search(h, nq, q, q_dtype, q_mem, k, Dd, Id, FX_MEM_DEVICE, sel, true);
    if (rc != FX_OK) return rc;
    // the gather follows the re-scan / exact-fallback chain on the stream; a missing slot's -1 is no row: NaN
    if (host_out) {
        const int rg = gather_to_host(h, Id, 0, h->id_offset, (int64_t)nres, R, r_dtype);
        if (rg != FX_OK) return rg;
    } else {
        HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, Id, 0, h->id_offset, (int64_t)nres,
                                   h->d, R, r_dtype, s));
    }
    if (h->has_ids) HIP_TRY(launch_label_ids(h->labels, h->ntotal, (int64_t)nres, Id, s));
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(D, Dd, nres * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(I, Id, nres * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return read_counts(h);  // (a host result checks the candidate lists' integrity itself, as search does)
    } else if (q_mem == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(s));  // (host queries: done with the caller's array on return)
    }
    return FX_OK;
}

int fx_index_compute_distance_subset(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k,
                                     const int64_t* keys, int keys_mem, float* D, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if ((q_mem != FX_MEM_HOST && q_mem != FX_MEM_DEVICE) || (keys_mem != FX_MEM_HOST && keys_mem != FX_MEM_DEVICE) ||
        (out_mem != FX_MEM_HOST && out_mem != FX_MEM_DEVICE))
        return set_err(FX_E_ARG, "bad q_mem / keys_mem / out_mem");
    if (nq == 0) return FX_OK;
    if (!q || !keys || !D) return set_err(FX_E_ARG, "null buffer");
    if (nq > (int64_t)INT32_MAX / k)
        return set_err(FX_E_UNSUPPORTED, "compute_distance_subset: more than 2^31-1 (query, key) pairs per call");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const int64_t n = nq * k;
    // host inputs staged in one buffer: [queries | keys]
    const size_t qbytes = (size_t)nq * h->d * dtype_size(q_dtype), koff = (size_t)round_up((int64_t)qbytes, 256);
    const bool stage_q = q_mem == FX_MEM_HOST, stage_k = keys_mem == FX_MEM_HOST;
    if (stage_q || stage_k) HIP_TRY(h->rc_in.ensure(koff + (size_t)n * 8));
    const void* qdev = q;
    const int64_t* dkeys = keys;
    if (stage_q) {
        HIP_TRY(hipMemcpyAsync(h->rc_in.p, q, qbytes, hipMemcpyHostToDevice, s));
        qdev = h->rc_in.p;
    }
    if (stage_k) {
        HIP_TRY(hipMemcpyAsync((char*)h->rc_in.p + koff, keys, (size_t)n * 8, hipMemcpyHostToDevice, s));
        dkeys = (const int64_t*)((char*)h->rc_in.p + koff);
    }
    // the queries once as padded fp32 [nq][kdim], in a buffer of this call's own (not a search's)
    HIP_TRY(h->rc_qf32.ensure((size_t)nq * h->kdim * 4));
    HIP_TRY(launch_f32_queries(qdev, q_dtype, nq, h->d, h->kdim, (float*)h->rc_qf32.p, s));
    int64_t id_offset = h->id_offset;
    if (h->has_ids) {
        const int rc = rows_of_keys(h, dkeys, n, &dkeys);
        if (rc != FX_OK) return rc;
        id_offset = 0;
    }
    float* Dd = D;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->rc_out.ensure((size_t)n * 4));
        Dd = (float*)h->rc_out.p;
    }
    HIP_TRY(launch_subset_dist(h->dtype, h->metric, h->codes, h->row_bytes, h->kdim, h->ntotal,
                               (const float*)h->rc_qf32.p, nq, k, dkeys, id_offset, Dd, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_mem == FX_MEM_HOST || stage_q || stage_k) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

// ---- k-means (fx_kmeans.hip) -------------------------------------------------

namespace {

// pinned staging of host training rows, per chunk
constexpr int64_t KMEANS_PIN_BYTES = 64ll << 20;

int km_check_index(const FxIndex* h, const char* who) {
    if (h->ntotal <= 0) return set_err(FX_E_ARG, "%s: the centroid index is empty", who);
    if (h->has_ids) return set_err(FX_E_UNSUPPORTED, "%s: the centroid index carries labels (add_with_ids)", who);
    if (h->id_offset != 0)
        return set_err(FX_E_UNSUPPORTED, "%s: the centroid index has id offset %lld", who, (long long)h->id_offset);
    if (h->ntotal > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "%s: more than 2^31-1 centroids", who);
    return FX_OK;
}

hipError_t km_ensure_bad(FxIndex* h) {
    if (h->km_bad) return hipSuccess;
    hipError_t e = hipMalloc((void**)&h->km_bad, 8);
    if (e == hipSuccess) e = hipMemset(h->km_bad, 0, 8);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->km_bad_pin, 8, hipHostMallocDefault);
    return e;
}

// the skipped-assignment count since the last read (waits for the stream), then 0 again
int km_read_bad(FxIndex* h, int64_t* out) {
    *out = 0;
    if (!h->km_bad) return FX_OK;
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(h->km_bad_pin, h->km_bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(h->km_bad, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)*h->km_bad_pin;
    return FX_OK;
}

int km_bad_error(int64_t bad, int64_t k) {
    return set_err(FX_E_INTEGRITY, "kmeans: %lld assignments outside [0, %lld) were skipped", (long long)bad,
                   (long long)k);
}

// fx_kmeans_step (search) / fx_kmeans_update: the rows in chunks, each chunk's
// assignment (searched, or the caller's) and its update, accumulated in chunk order
int km_run(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, int64_t* assign, float* dist, bool search,
           double* sums, int64_t* counts, double* obj, int accumulate) {
    hipStream_t s = h->stream();
    const int64_t k = h->ntotal;
    const int64_t rowb = (int64_t)h->d * dtype_size(x_dtype);
    const bool host = x_mem == FX_MEM_HOST;
    int64_t chunk = h->opt.kmeans_chunk > 0 ? h->opt.kmeans_chunk : (int)KMEANS_CHUNK_DEFAULT;
    if (host) chunk = std::min(chunk, std::max<int64_t>(1, KMEANS_PIN_BYTES / rowb));
    chunk = std::min(chunk, n);
    HIP_TRY(km_ensure_bad(h));
    if (search && (!assign || !dist)) HIP_TRY(h->km_out.ensure((size_t)chunk * 12));
    if (host) {
        HIP_TRY(h->km_x.ensure((size_t)(chunk * rowb)));
        HIP_TRY(ensure_pinned(h->km_pin, h->km_pin_bytes, (size_t)(chunk * rowb)));
    }
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        size_t ws_bytes = 0;  // (per chunk: the sort's temporaries need not grow with the rows)
        HIP_TRY(km_workspace(nr, k, h->d, &ws_bytes));
        HIP_TRY(h->km_ws.ensure(ws_bytes));
        const void* xd = (const char*)x + r0 * rowb;
        if (host) {
            memcpy(h->km_pin, xd, (size_t)(nr * rowb));
            HIP_TRY(hipMemcpyAsync(h->km_x.p, h->km_pin, (size_t)(nr * rowb), hipMemcpyHostToDevice, s));
            xd = h->km_x.p;
        }
        int64_t* a = assign ? assign + r0 : (int64_t*)h->km_out.p;
        float* dd = dist ? dist + r0 : (search ? (float*)((char*)h->km_out.p + (size_t)chunk * 8) : nullptr);
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (h->profile) {
            for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
            h->km_ev.insert(h->km_ev.end(), ev, ev + 4);
            HIP_TRY(hipEventRecord(ev[0], s));
        }
        if (search) {
            // the index's own device-output k = 1 search: every plan, the re-scan and the exact fallback
            const int rc = do_search(h, nr, xd, x_dtype, FX_MEM_DEVICE, 1, dd, a, FX_MEM_DEVICE);
            if (rc != FX_OK) return rc;
        }
        if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
        KmUpdate u{};
        u.x = xd;
        u.x_dt = x_dtype;
        u.n = nr;
        u.d = h->d;
        u.k = k;
        u.assign = a;
        u.dist = dd;
        u.sums = sums;
        u.counts = counts;
        u.obj = obj;
        u.accumulate = accumulate != 0 || r0 > 0;
        u.bad = h->km_bad;
        HIP_TRY(launch_km_update(u, h->km_ws.p, h->km_ws.bytes, s, ev[2]));
        if (h->profile) HIP_TRY(hipEventRecord(ev[3], s));
        if (host) HIP_TRY(hipStreamSynchronize(s));  // (the staging buffers are free again)
    }
    if (!host) return FX_OK;
    // a host call has waited for its work: its skipped entries are known now
    int64_t bad = 0;
    if (const int rc = km_read_bad(h, &bad); rc != FX_OK) return rc;
    return bad > 0 ? km_bad_error(bad, k) : FX_OK;
}

int km_check_args(const FxIndex* h, int64_t n, int x_dtype, int x_mem, const double* sums, const int64_t* counts,
                  const double* obj) {
    // (the index last: the other checks are then reachable without a device)
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (x_mem != FX_MEM_HOST && x_mem != FX_MEM_DEVICE) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    if (!sums || !counts || !obj) return set_err(FX_E_ARG, "null sums / counts / obj");
    if (!h) return set_err(FX_E_ARG, "null index");
    return FX_OK;
}

}  // namespace

int fx_kmeans_step(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, int64_t* assign, float* dist,
                   double* sums, int64_t* counts, double* obj, int accumulate) {
    if (const int rc = km_check_args(h, n, x_dtype, x_mem, sums, counts, obj); rc != FX_OK) return rc;
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_step"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    return km_run(h, n, x, x_dtype, x_mem, assign, dist, true, sums, counts, obj, accumulate);
}

int fx_kmeans_update(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* assign,
                     const float* dist, double* sums, int64_t* counts, double* obj, int accumulate) {
    if (const int rc = km_check_args(h, n, x_dtype, x_mem, sums, counts, obj); rc != FX_OK) return rc;
    if (n == 0) return FX_OK;
    if (!x || !assign) return set_err(FX_E_ARG, "null x / assign");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_update"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    return km_run(h, n, x, x_dtype, x_mem, const_cast<int64_t*>(assign), const_cast<float*>(dist), false, sums, counts,
                  obj, accumulate);
}

int fx_kmeans_finish(FxIndex* h, const double* sums, const int64_t* counts, int spherical, float* centroids_out,
                     int64_t* n_split) {
    if (!sums || !counts || !centroids_out || !n_split) return set_err(FX_E_ARG, "null buffer");
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_finish"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const int64_t k = h->ntotal;
    HIP_TRY(h->km_h.ensure((size_t)k * 8));
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (h->profile) {
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        h->km_ev_fin.insert(h->km_ev_fin.end(), ev, ev + 2);
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    KmFinish f{};
    f.sums = sums;
    f.counts = counts;
    f.k = k;
    f.d = h->d;
    f.codes = h->codes;
    f.st_dt = h->dtype;
    f.row_bytes = h->row_bytes;
    f.spherical = spherical;
    f.cent = centroids_out;
    f.h = (int64_t*)h->km_h.p;
    f.n_split = n_split;
    HIP_TRY(launch_km_finish(f, s));
    // fx_index_reset and a device-side fx_index_add of the k new rows, both
    // stream-ordered: the rows [0, k) are rewritten in place (nothing grows, the
    // rows past k keep their zero codes and +inf norms), the scan image and
    // its centre are rebuilt by the next search, selectors from before are stale
    HIP_TRY(hipMemsetAsync(h->max_sq_bits, 0, 8, s));
    h->ntotal = 0;
    ++h->epoch;
    h->img_rows = 0;
    h->mu_rows = 0;
    h->rg_nq = -1;
    h->rg_total = 0;
    if (const int rc = append_rows(h, k, centroids_out, FX_F32, FX_MEM_DEVICE); rc != FX_OK) return rc;
    h->ntotal = k;
    if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
    return FX_OK;
}

int fx_kmeans_status(FxIndex* h, int64_t* bad_assign) {
    if (!h || !bad_assign) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (const int rc = km_read_bad(h, bad_assign); rc != FX_OK) return rc;
    return *bad_assign > 0 ? km_bad_error(*bad_assign, h->ntotal) : FX_OK;
}

int fx_kmeans_profile_read(FxIndex* h, double* assign_ms, double* sort_ms, double* sum_ms, double* finish_ms) {
    if (!h || !assign_ms || !sort_ms || !sum_ms || !finish_ms) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    double ms[4] = {0, 0, 0, 0};
    float v = 0;
    for (size_t i = 0; i + 3 < h->km_ev.size(); i += 4)
        for (int p = 0; p < 3; ++p) {
            HIP_TRY(hipEventElapsedTime(&v, h->km_ev[i + p], h->km_ev[i + p + 1]));
            ms[p] += v;
        }
    for (size_t i = 0; i + 1 < h->km_ev_fin.size(); i += 2) {
        HIP_TRY(hipEventElapsedTime(&v, h->km_ev_fin[i], h->km_ev_fin[i + 1]));
        ms[3] += v;
    }
    for (hipEvent_t e : h->km_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->km_ev_fin) (void)hipEventDestroy(e);
    h->km_ev.clear();
    h->km_ev_fin.clear();
    *assign_ms = ms[0];
    *sort_ms = ms[1];
    *sum_ms = ms[2];
    *finish_ms = ms[3];
    return FX_OK;
}

// the header fields an IxF2 file and an IxM2 / IxMp wrapper share, after the fourcc
static bool write_index_header(FILE* f, int32_t d, int64_t nt) {
    const int32_t metric = FX_METRIC_L2;
    const int64_t dummy = 1 << 20;
    const uint8_t trained = 1;
    return fwrite(&d, 4, 1, f) == 1 && fwrite(&nt, 8, 1, f) == 1 && fwrite(&dummy, 8, 1, f) == 1 &&
           fwrite(&dummy, 8, 1, f) == 1 && fwrite(&trained, 1, 1, f) == 1 && fwrite(&metric, 4, 1, f) == 1;
}
static bool read_index_header(FILE* f, int32_t* d, int64_t* nt, int32_t* metric) {
    int64_t d1 = 0, d2 = 0;
    uint8_t trained = 0;
    return fread(d, 4, 1, f) == 1 && fread(nt, 8, 1, f) == 1 && fread(&d1, 8, 1, f) == 1 && fread(&d2, 8, 1, f) == 1 &&
           fread(&trained, 1, 1, f) == 1 && fread(metric, 4, 1, f) == 1;
}

int fx_index_write(FxIndex* h, const char* path) {
    if (!h || !path) return set_err(FX_E_ARG, "null argument");
    if (h->metric != FX_METRIC_L2) return set_err(FX_E_UNSUPPORTED, "IxF2 writer supports METRIC_L2 only");
    FILE* f = fopen(path, "wb");
    if (!f) return set_err(FX_E_IO, "cannot open %s for writing", path);
    const int32_t d = h->d;
    const int64_t nt = h->ntotal, count = h->ntotal * (int64_t)h->d;
    const bool labelled = h->has_ids;
    bool ok = true;
    // a labelled index: faiss's IndexIDMap2 file -- its own header, the flat index as the sub-index, the labels
    if (labelled) ok = fwrite("IxM2", 1, 4, f) == 4 && write_index_header(f, d, nt);
    ok = ok && fwrite("IxF2", 1, 4, f) == 4 && write_index_header(f, d, nt) && fwrite(&count, 8, 1, f) == 1;
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)h->d * 4));
    std::vector<float> buf;
    for (int64_t r0 = 0; ok && r0 < nt; r0 += chunk) {
        const int64_t nr = std::min(chunk, nt - r0);
        buf.resize((size_t)nr * h->d);
        int rc = fx_index_reconstruct_n(h, r0, nr, buf.data());
        if (rc != FX_OK) {
            fclose(f);
            return rc;
        }
        ok = fwrite(buf.data(), 4, buf.size(), f) == buf.size();
    }
    if (ok && labelled) {
        std::vector<int64_t> ids((size_t)nt);
        const int rc = fx_index_get_ids(h, 0, nt, ids.data(), FX_MEM_HOST);
        if (rc != FX_OK) {
            fclose(f);
            return rc;
        }
        ok = fwrite(&nt, 8, 1, f) == 1 && fwrite(ids.data(), 8, ids.size(), f) == ids.size();
    }
    if (fclose(f) != 0) ok = false;
    if (!ok) return set_err(FX_E_IO, "short write to %s", path);
    return FX_OK;
}

int fx_index_read(const char* path, int storage_dtype, int device, FxIndex** out) {
    if (!path || !out) return set_err(FX_E_ARG, "null argument");
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return set_err(FX_E_IO, "could not open %s for reading", path);
    char fourcc[4];
    int32_t d = 0, metric = 0;
    int64_t nt = 0, count = 0;
    bool ok = fread(fourcc, 1, 4, f) == 4;
    // IndexIDMap ("IxMp") / IndexIDMap2 ("IxM2"): a header of their own around the flat sub-index
    const bool labelled = ok && (memcmp(fourcc, "IxM2", 4) == 0 || memcmp(fourcc, "IxMp", 4) == 0);
    int32_t wd = 0, wmetric = 0;
    int64_t wnt = 0;
    if (labelled) ok = read_index_header(f, &wd, &wnt, &wmetric) && fread(fourcc, 1, 4, f) == 4;
    ok = ok && read_index_header(f, &d, &nt, &metric) && fread(&count, 8, 1, f) == 1;
    if (!ok) {
        fclose(f);
        return set_err(FX_E_IO, "%s: truncated IxF2 header", path);
    }
    if (memcmp(fourcc, "IxF2", 4) != 0) {
        fclose(f);
        return set_err(FX_E_IO, "%s: unsupported index fourcc (only IxF2 / IndexFlatL2, alone or inside IxMp / IxM2)", path);
    }
    if (d <= 0 || nt < 0 || metric != FX_METRIC_L2 || count != nt * (int64_t)d ||
        (labelled && (wd != d || wnt != nt || wmetric != metric))) {
        fclose(f);
        return set_err(FX_E_IO, "%s: inconsistent IxF2 header", path);
    }
    FxIndex* h = nullptr;
    int rc = fx_index_create(d, storage_dtype, FX_METRIC_L2, device, &h);
    if (rc != FX_OK) {
        fclose(f);
        return rc;
    }
    rc = fx_index_reserve(h, nt);
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)d * 4));
    std::vector<float> buf;
    for (int64_t r0 = 0; rc == FX_OK && r0 < nt; r0 += chunk) {
        const int64_t nr = std::min(chunk, nt - r0);
        buf.resize((size_t)nr * d);
        if (fread(buf.data(), 4, buf.size(), f) != buf.size()) {
            rc = set_err(FX_E_IO, "%s: truncated IxF2 codes", path);
            break;
        }
        rc = fx_index_add(h, nr, buf.data(), FX_F32, FX_MEM_HOST);
    }
    if (rc == FX_OK && labelled) {
        // i64 n, n labels: attached to the rows just added (the index becomes a labelled one)
        int64_t n = -1;
        std::vector<int64_t> ids;
        if (fread(&n, 8, 1, f) != 1 || n != nt) {
            rc = set_err(FX_E_IO, "%s: truncated or inconsistent id map (%lld ids for %lld rows)", path, (long long)n,
                         (long long)nt);
        } else {
            ids.resize((size_t)n);
            if (n > 0 && fread(ids.data(), 8, ids.size(), f) != ids.size()) rc = set_err(FX_E_IO, "%s: truncated id map", path);
        }
        if (rc == FX_OK) {
            std::lock_guard<std::mutex> lk(h->mu);
            DeviceGuard g(h->device);
            h->has_ids = true;
            hipError_t e = grow_labels(h);
            if (e == hipSuccess && n > 0) e = hipMemcpy(h->labels, ids.data(), (size_t)n * 8, hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = set_err(FX_E_HIP, "%s: storing the id map: %s", path, hipGetErrorString(e));
        }
    }
    fclose(f);
    if (rc != FX_OK) {
        fx_index_free(h);
        return rc;
    }
    *out = h;
    return FX_OK;
}

int fx_merge_shards(int metric, int nshards, int64_t nq, int k, const float* D_in, const int64_t* I_in, float* D_out,
                    int64_t* I_out, int device, void* stream) {
    if (nshards <= 0 || nq < 0 || k <= 0) return set_err(FX_E_ARG, "bad merge shape");
    if (!D_in || !I_in || !D_out || !I_out) return set_err(FX_E_ARG, "null buffer");
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric");
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    if (k > FX_MAX_K && nshards > FX_HUGEK_MAX_SHARDS)
        return set_err(FX_E_UNSUPPORTED, "merge of k = %d > %d lists supports at most %d shards (got %d)", k, FX_MAX_K,
                       FX_HUGEK_MAX_SHARDS, nshards);
    if (k > FX_MAX_K)  // stream-ordered sort merge (fx_hugek.hip)
        HIP_TRY(launch_merge_shards_sort(metric, nshards, nq, k, D_in, I_in, D_out, I_out, (hipStream_t)stream));
    else
        HIP_TRY(launch_merge_shards(metric, nshards, nq, k, D_in, I_in, D_out, I_out, (hipStream_t)stream));
    return FX_OK;
}

int fx_synth_fill(void* out, int64_t row0, int64_t n, int d, int dtype, uint64_t seed, int device, void* stream) {
    if (!out || n < 0 || d <= 0 || row0 < 0 || !check_dtype(dtype)) return set_err(FX_E_ARG, "bad synth args");
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    HIP_TRY(launch_synth(out, row0, n, d, dtype, seed, (hipStream_t)stream));
    return FX_OK;
}

int fx_index_profile(FxIndex* h, int enable) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    for (auto& pr : h->ev_scan) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : h->ev_merge) (void)hipEventDestroy(pr.second);
    h->ev_scan.clear();
    h->ev_merge.clear();
    h->profile = enable != 0;
    return FX_OK;
}

int fx_index_profile_read(FxIndex* h, double* scan_ms, double* merge_ms, int64_t* launches) {
    if (!h || !scan_ms || !merge_ms || !launches) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    double a = 0, b = 0;
    for (size_t i = 0; i < h->ev_scan.size(); ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_scan[i].first, h->ev_scan[i].second));
        a += ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_merge[i].first, h->ev_merge[i].second));
        b += ms;
    }
    *scan_ms = a;
    *merge_ms = b;
    *launches = (int64_t)h->ev_scan.size();
    return FX_OK;
}

}  // extern "C"
