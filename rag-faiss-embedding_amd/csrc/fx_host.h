// fx_host.h -- internal header of the host side of the C ABI (fx_index.cpp,
// fx_api_*.cpp, fx_plan.cpp; never a .hip file): error reporting, the owning
// buffers, the index's options and state, and the few helpers that cross files.
// Each feature's state is a member struct of FxIndex, declared here beside the
// prototypes of the file that owns it; the other index handles are built from
// the shared parts of fx_api_handle.cpp (Handle, SearchStats, CodeRows).
#pragma once
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

namespace fx {

// sets the calling thread's fx_last_error() text; returns code (fx_index.cpp)
int set_err(int code, const char* fmt, ...);

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

// Device memory that frees itself.  The owner's destructor must run with the
// buffer's device current (fx_index_free / fx_selector_free delete inside
// their DeviceGuard).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        const size_t grow = std::max(want, bytes + bytes / 2);
        release();
        hipError_t e = hipMalloc(&p, grow);
        if (e == hipSuccess) bytes = grow;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
};

// Its pinned host counterpart (grows by 1.5x like DevBuf: the growth is taken
// from the old capacity, before that is given up).
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        const size_t grow = std::max(want, bytes + bytes / 2);
        release();
        hipError_t e = hipHostMalloc(&p, grow, hipHostMallocDefault);
        if (e == hipSuccess) bytes = grow;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// A buffer read as an array of T: `buf + r`, `buf[i]` and a T* argument work
// as on the pointer it holds.
template <class Buf, class T>
struct ArrOf : Buf {
    operator T*() const { return (T*)this->p; }
};
template <class T>
using DevArr = ArrOf<DevBuf, T>;
template <class T>
using PinArr = ArrOf<PinBuf, T>;

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline bool check_dtype(int dt) { return dt == FX_F32 || dt == FX_BF16 || dt == FX_F16; }
inline bool valid_mem(int mem) { return mem == FX_MEM_HOST || mem == FX_MEM_DEVICE; }

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
    std::string sq_cand, ivf_cand;  // FX_SQ_CAND / FX_IVF_CAND: the scan lists of fx_sq_search / fx_ivf_search, per pass
    std::string ivfsq_cand;         // FX_IVFSQ_CAND: the scan lists and pair operands of fx_ivfsq_search, per pass
    std::string pq_cand;            // FX_PQ_CAND: the scan lists, query operands and row constants of fx_pq_search, per pass
    std::string ivfpq_cand;         // FX_IVFPQ_CAND: the scan lists, pair operands and rows of fx_ivfpq_search, per pass
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
        str("FX_SQ_CAND", sq_cand);
        str("FX_IVF_CAND", ivf_cand);
        str("FX_IVFSQ_CAND", ivfsq_cand);
        str("FX_PQ_CAND", pq_cand);
        str("FX_IVFPQ_CAND", ivfpq_cand);
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

#ifdef FX_DIAG
// n elements of device memory appended to the file `path` (the diagnostic dumps; the caller has
// synchronised the stream that wrote them)
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

// scan image of the index (what the MFMA scan streams, and its row constants)
enum ImageKind {
    IMG_NONE = 0,  // the stored rows with srcC = |y|^2 (IP: no row constant)
    IMG_F32S = 1,  // fp32 index: [hi | lo] bf16 planes of fl(y - mu), srcC = |y - mu|^2
    IMG_C16 = 2,   // bf16 / fp16 L2 index: the stored rows, srcC = |y - mu|^2 (the query operand is x - mu)
};

// what the planners (fx_plan.h) read of an index
struct IndexShape {
    int64_t ntotal;
    int row_bytes, dtype, metric, img_kind;
};

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

// the query operands of one scan: k_prep_queries' outputs (PrepParams)
struct QueryBufs {
    DevBuf f32, op, eps, rho, shift;
};

// ---- fx_index.cpp: lifecycle, add, reset, files ------------------------------

// rows [ntotal, ntotal + n) <- x (arguments validated, the index locked);
// ntotal is the caller's to advance
int append_rows(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem);
int check_add_args(const FxIndex* h, int64_t n, const void* x, int x_dtype);
// rows [r0, r1) of the code matrix <- what a row that holds nothing looks like:
// zero codes (padding rows of the last tile must be finite) and |y|^2 = +inf
// (which keeps them out of the scan's candidate lists)
hipError_t blank_rows(FxIndex* h, int64_t r0, int64_t r1, hipStream_t s);
// Input of a call -> where the kernels read it: device memory is used where it
// lies (*dev = src); host memory is copied, on stream s, into `buf` (grown to
// offset + bytes) at `offset`.
hipError_t stage_in(hipStream_t s, DevBuf& buf, const void* src, size_t bytes, int mem, const void** dev,
                    size_t offset = 0);

// ---- fx_api_search.cpp ---------------------------------------------------------

// the re-scan of uncertified queries (plan_rescan): its own query operands,
// thresholds, candidate lists and flagged list
struct RescanState : QueryBufs {
    DevBuf gtau, cand_d, cand_i, flag;
};
// search_graph: the search of a small host batch (the reference's one-query
// call form) replayed as one hipGraph per shape, over pinned host staging;
// `key` = the shape and every buffer the graph captured
struct GraphState {
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;
    bool failed = false;
    PinBuf hq;    // the captured H2D copy's source
    PinBuf hout;  // pinned mirror of hout for the graph's one D2H copy
    SearchPlan plan;  // the captured search's plan (its fallback chain runs eagerly when needed)
};
// k > FX_BIG_K (fx_hugek.hip): query batch, sort keys, rocPRIM temporaries
struct HugeKState {
    DevBuf ws;
};
int do_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem,
              const FxSelector* sel = nullptr, bool row_ids = false);
int do_search_hugek(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                    int out_mem, bool row_ids = false);
int fill_missing(FxIndex* h, int64_t nq, int k, float* D, int64_t* I, int out_mem);
int read_counts(FxIndex* h);
int integrity_error(const FxIndex* h);
hipError_t update_scan_image(FxIndex* h);
void graph_release(FxIndex* h);
// the fields of a query preparation / a scan that every caller sets alike:
// the batch, the index's shape, the operand buffers; the scan reads the
// stored rows, or the scan image of img_kind
void base_prep(const FxIndex* h, const QueryBufs& b, const void* q, int q_dtype, int64_t nq, int64_t nq_pad, int st_dt,
               PrepParams& pp);
void base_scan(const FxIndex* h, int img_kind, const QueryBufs& b, int64_t nq, ScanParams& sp);

// ---- fx_api_select.cpp ---------------------------------------------------------

// the selector's counts on the host (waits for its build once)
int selector_counts(const FxSelector* sel);
// A selector handed to a call `who` on h: made on h and, with `since` non-null
// (the index locked), still a snapshot of its rows; `since` names what may have
// happened to them, which differs between a search and a removal.
int check_selector(const FxIndex* h, const FxSelector* sel, const char* who, const char* since);

// ---- fx_api_range.cpp ----------------------------------------------------------

// range_search (fx_range.hip): its own query operands and thresholds (none of
// them a buffer a search graph captured), the candidate words, and the last
// call's result (lims / D / I), kept until the next range search, reset or free
struct RangeState : QueryBufs {
    DevBuf qin, thr, cnt, cand, dist, sorted, temp, lims, D, I;
    int64_t nq = -1;    // queries of the stored result (-1: none)
    int64_t total = 0;  // its lims[nq]
    int64_t cands = 0;  // pairs the MFMA scan emitted
    int passes = 0;     // scan passes run (0: no scan was needed)
};

// ---- fx_api_remove.cpp ---------------------------------------------------------

struct RemoveState {
    DevBuf ws;  // [prefix | gp | block sums | info | staged norms] (remove_rows)
    // the last removal's plan: first removed row, rows moved in place / through staging, chunks launched
    int64_t stats[4] = {0, 0, 0, 0};
};

// ---- fx_api_idmap.cpp ----------------------------------------------------------

// stable ids (fx_idmap.hip): in the labelled mode (FxIndex::has_ids) row r's
// label is labels[r]; the buffer holds at least cap_rows entries (grow_labels).
struct IdMapState {
    DevArr<int64_t> labels;
    DevArr<int64_t> labels_alt;  // the second buffer a removal compacts into, then swapped in
    DevBuf ws;  // sort workspace of a selector's id list / rows_of_ids, staged host ids
};

// ---- fx_api_recon.cpp ----------------------------------------------------------

// reconstruct_batch / search_and_reconstruct / compute_distance_subset (fx_recon.hip): staged host
// keys and queries, a labelled index's keys as rows, the fp32 queries, device results of a host
// output -- none of them a buffer a search graph captured
struct ReconState {
    DevBuf in, rows, qf32, out;
};

// ---- fx_api_kmeans.cpp ---------------------------------------------------------

// k-means (fx_kmeans.hip): the update's workspace, the assignment / distances of a chunk when the
// caller keeps none, staged host rows (device and pinned), the repair's working counts, and the
// device counter of assignments outside [0, k) with its pinned mirror
struct KmeansState {
    DevBuf ws, out, x, h;
    PinBuf pin;
    DevArr<unsigned long long> bad;
    PinArr<unsigned long long> bad_pin;
    std::vector<hipEvent_t> ev, ev_fin;  // profiling: 4 events per chunk of a step, 2 per finish
};

}  // namespace fx

struct FxIndex {
    int d = 0, dtype = fx::F32, metric = fx::L2, device = 0, normalize = 0;
    int row_bytes = 0, kdim = 0;
    int64_t ntotal = 0, cap_rows = 0, id_offset = 0;
    fx::DevArr<char> codes;
    fx::DevArr<float> norms;
    bool has_ids = false;
    fx::IdMapState idm;
    // device words: [0] max |y|^2 of the stored rows, [1] max srcC of the scan
    // image (F32S / C16), as float bits (non-negative floats order as uints)
    fx::DevArr<unsigned> max_sq_bits;
    hipStream_t own_stream = nullptr;
    hipStream_t user_stream = nullptr;
    hipEvent_t switch_ev = nullptr;  // orders the work of a stream the index leaves before the next one's
    fx::Options opt;
    // search workspace
    fx::QueryBufs qw;
    fx::DevBuf qin, cand_d, cand_i, cand2_d, cand2_i, dws, iws, flag, fbc_d, fbc_i, stage, gtau, trace, dbgbuf, stamps,
        pub;
    fx::RescanState rq;
    fx::HugeKState hk;
    // scan image (ImageKind; rows [0, img_rows) current).  L2 images are
    // centred (Options.centre): mu = mean of a row sample, recomputed (and the
    // image rebuilt) whenever ntotal has doubled since (mu_rows), so the
    // centre follows the data at O(1) amortised cost per added row.
    //   F32S: split = [hi | lo] bf16 planes of fl(y - mu), cnorms = |y - mu|^2
    //   C16:  cnorms = |y - mu|^2 of the stored bf16 / fp16 rows (no copy of
    //         the codes; a 16-bit centre whose norm is small next to the rows'
    //         is set to 0 on the device: k_mu_finish)
    fx::DevBuf split, cnorms, centre, mu_part;
    int64_t img_rows = 0, mu_rows = 0;
    int img_kind = fx::IMG_NONE;
    bool centred = false;
    fx::GraphState graph;
    // host-output searches: ONE packed device buffer [D | I | n_drop | n_flag |
    // flag list] (host_out_layout) and its pinned mirror, so the common case
    // returns through one D2H copy
    fx::DevBuf hout;
    fx::PinBuf hpin;
    fx::PinBuf qpin;  // pinned staging of a host-output search's host queries (<= QPIN_MAX)
    int64_t last_fallbacks = 0;
    // uncertified count of the last search, copied stream-ordered into pinned
    // memory; read (after a stream sync) only when asked for (fb_pending)
    fx::PinArr<int> pin_nf;  // [0] queries re-scanned, [1] queries sent to the exact scan, [2] dropped ids
    bool fb_pending = false;
    int64_t last_exact = 0;
    // candidate entries the refine dropped for a row id outside [0, ntotal)
    // (a corrupted candidate list; 0 unless something is broken)
    int64_t last_dropped = 0;
    fx::DevArr<int> dev_drop;  // its device word, zeroed at the start of every search
    fx::RangeState rg;
    fx::RemoveState rm;
    fx::ReconState rc;
    fx::KmeansState km;
    fx::DevBuf conv;  // k_scan_v5 convoy words (CONV_WORDS; zeroed once, then only hints)
    int last_plan[3] = {0, 0, 0};  // the last search's scan plan: tile rows (128 k_scan_v4, 64 k_scan_v5), qt, splits
    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_scan, ev_merge;
    std::mutex mu;

    uint64_t epoch = 0;  // bumped by reset and by a removal: a selector (a snapshot of the rows) from before is stale

    hipStream_t stream() const { return user_stream ? user_stream : own_stream; }
    // the label buffer the kernels translate rows with (null: ids are row + id_offset)
    const int64_t* label_ptr() const { return has_ids ? (const int64_t*)idm.labels : nullptr; }
    fx::IndexShape shape() const { return {ntotal, row_bytes, dtype, metric, img_kind}; }
};

// The quantizer's searches run on the borrowing index's stream for the duration
// of a call (the quantizer locked): both directions ordered on the device, as
// fx_index_set_stream orders a switch.
struct BorrowQuant {
    FxIndex* q;
    hipStream_t s, prev_user, prev;
    std::unique_lock<std::mutex> lk;
    BorrowQuant(FxIndex* quant, hipStream_t stream) : q(quant), s(stream), lk(quant->mu) {
        prev_user = q->user_stream;
        prev = q->stream();
    }
    hipError_t begin() {
        hipError_t e = hipSuccess;
        if (prev != s) {
            e = hipEventRecord(q->switch_ev, prev);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, q->switch_ev, 0);
        }
        q->user_stream = s;
        return e;
    }
    ~BorrowQuant() {
        q->user_stream = prev_user;
        if (prev != s && hipEventRecord(q->switch_ev, s) == hipSuccess) (void)hipStreamWaitEvent(prev, q->switch_ev, 0);
    }
};

// ---- fx_api_handle.cpp: what the indexes beside the flat one share -------------
//
// FxSq, FxPq, FxIvfSq and FxIvfPq are a Handle (stream, options, lock, counts,
// profile) over CodeRows (their payload); FxSq and FxPq share FlatCodes and its
// search driver (fx_flat_codes.h); FxIvf, FxIvfSq and FxIvfPq share IvfLists
// (fx_ivf_lists.h).

namespace fx {

// D / I of a search over an empty index, written through host vectors (FxIndex
// fills with memsets: fx_api_search.cpp)
int fill_missing(hipStream_t s, int metric, int64_t nq, int k, float* D, int64_t* I, int out_mem);
// where a call's result is computed: the caller's device memory, or `io` for a host caller ...
hipError_t out_buf(DevBuf& io, void* out, size_t bytes, int out_mem, void** od);
// ... and its way back: copied out and waited for (wait: a host input the call staged must be waited for too)
int finish_out(hipStream_t s, void* out, const void* od, size_t bytes, int out_mem, bool wait = false);
// "<kind> <call>: the index is not trained"
int need_trained(bool trained, const char* kind, const char* call);
// the checks of a call that takes rows x [n][d] (the handle's own check comes after them)
int check_rows(int64_t n, int x_dtype, int x_mem);
// a trained table [vmin | vdiff] as the scalar quantizers accept it
int sq_check_tables(const char* kind, int d, const float* trained);
// What a product quantizer derives from its centroids [M][256][dsub] on the host (fx_api_pq.cpp): the
// scan image (dsub % 8 == 0: two bf16 planes [hi | lo] of pq_plane_bytes each, else empty) and the
// bound's constants max |decode|, max |y - y_hi - y_lo|, max |y_lo| over any code row.  FX_E_ARG for a
// non-finite centroid or norms outside the fp32 range.
struct PqCodebook {
    std::vector<uint16_t> img;
    double Y = 0, Ry = 0, Yl = 0;
};
int pq_codebook(const char* kind, int M, int dsub, const float* centroids, PqCodebook& out);

// Rows x [n][d] through the bounded staging buffer `in` (<= 256 MiB a chunk, or
// `chunk` rows): body(xd, r0, nr) per chunk, and one synchronisation per chunk
// when x is host memory (the staging buffer is reused).
template <class Body>
int staged_rows(hipStream_t s, DevBuf& in, int64_t n, const void* x, size_t row_bytes, int x_mem, int64_t chunk,
                Body body) {
    if (chunk <= 0)
        chunk = x_mem == FX_MEM_DEVICE ? std::max<int64_t>(n, 1) : std::max<int64_t>(1, (256ll << 20) / (int64_t)row_bytes);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* xd = nullptr;
        HIP_TRY(stage_in(s, in, (const char*)x + (size_t)r0 * row_bytes, (size_t)nr * row_bytes, x_mem, &xd));
        if (const int rc = body(xd, r0, nr); rc != FX_OK) return rc;
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

// The counts and the profile of a handle's searches.  cnt: [0] dropped
// candidate ids, [1] queries flagged, [2] inverted files: coarse entries
// outside the lists; copied stream-ordered into pin_cnt by a search and read
// (after a synchronisation) when someone asks.  ev: `per_pass` events of every
// profiled pass (4: start, prep, scan, refine + exact; inverted files 5:
// start, coarse, pairs + prep, list scan, refine + exact).
struct SearchStats {
    DevArr<int> cnt;
    PinArr<int> pin_cnt;
    bool counts_pending = false;
    int64_t last_fallbacks = 0, last_dropped = 0, last_bad_probe = 0;
    bool profile = false;
    std::vector<hipEvent_t> ev;

    hipError_t init_counts();
    void clear_counts() {
        counts_pending = false;
        last_fallbacks = last_dropped = last_bad_probe = 0;
    }
    // a profiled pass's n events, the first recorded
    hipError_t begin_pass(hipEvent_t* pass_ev, int n, hipStream_t s);
    hipError_t mark(hipEvent_t e, hipStream_t s) { return profile ? hipEventRecord(e, s) : hipSuccess; }
    void destroy_events();
    // quant: the borrowed coarse quantizer, whose own integrity count is read with these
    int read_counts(int device, hipStream_t s, FxIndex* quant = nullptr);
    // ms[per_pass - 1] <- the summed parts of the passes since the last read
    int profile_read(int device, hipStream_t s, int per_pass, double* const* ms, int64_t* passes);
};

struct Handle : SearchStats {
    int device = 0;
    hipStream_t own_stream = nullptr, user_stream = nullptr;
    hipEvent_t switch_ev = nullptr;  // orders the work of a stream the index leaves before the next one's
    Options opt;  // (force_fallback and the dump paths of the diagnostic build, read from the environment at creation)
    std::mutex mu;
    hipStream_t stream() const { return user_stream ? user_stream : own_stream; }
    hipError_t init();  // the options, the stream, the event, the counts (the device current)
};
// the event hand-over of a stream switch, as fx_index_set_stream's
int handle_set_stream(Handle* h, const char* kind, void* stream);

// the calls every handle type H (a SearchStats with device, stream() and mu) answers alike
template <class H>
void handle_free(H* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->user_stream) (void)hipStreamSynchronize(h->user_stream);
    h->destroy_events();
    if (h->switch_ev) (void)hipEventDestroy(h->switch_ev);
    const hipStream_t own = h->own_stream;
    delete h;  // its buffers, with the device current and before the stream goes
    if (own) (void)hipStreamDestroy(own);
}
template <class H>
int handle_profile(H* h, const char* kind, int enable) {
    if (!h) return set_err(FX_E_ARG, "null %s index", kind);
    std::lock_guard<std::mutex> lk(h->mu);
    h->profile = enable != 0;
    return FX_OK;
}
template <class H, size_t N>
int handle_profile_read(H* h, double* const (&ms)[N], int64_t* passes) {
    if (!h) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    return h->profile_read(h->device, h->stream(), (int)N + 1, ms, passes);
}
// (a flagged query goes straight to the exact scan: both fallback counts are the same)
template <class H>
int handle_last_counts(H* h, FxIndex* quant, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    if (!h || !fallbacks || !exact_fallbacks || !dropped) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = h->read_counts(h->device, h->stream(), quant); rc != FX_OK) return rc;
    *fallbacks = h->last_fallbacks;
    *exact_fallbacks = h->last_fallbacks;
    *dropped = h->last_dropped + h->last_bad_probe;
    return FX_OK;
}

// Codes [cap_rows][stride] and the rows' constants (n_c of the scalar
// quantizers, n_y of the product quantizer), with a whole tile past the last
// row; `lists`: the rows' labels and lists beside them (FxIvfSq).  Rows past
// ntotal hold code 0 and constant 0: the scans mask them by row number.
struct CodeRows {
    int stride = 0;
    int64_t ntotal = 0, cap_rows = 0;
    bool lists = false;
    DevArr<char> codes;
    DevArr<float> nc;
    DevArr<int64_t> labels;
    DevArr<int> row_list;
    // capacity for n rows (1.5x steps), the ntotal rows carried over; synchronises before the swap
    hipError_t grow(int64_t n, hipStream_t s);
    // codes and constants <- 0 (a reset)
    hipError_t zero(hipStream_t s);
};

// What FxSq and FxPq share: the search driver's workspace and the last plan (fx_flat_codes.h)
struct FlatCodes : Handle, CodeRows {
    int d = 0, metric = L2;
    bool trained = false;
    // workspace of add / search / the codec
    DevBuf in, qf32, planes, eps, rho, shift, cand_d, cand_i, flag, outD, outI, io;
    int last_plan[4] = {0, 0, 0, 0};  // path, query tiles, splits, exact splits
    int64_t last_qbatch = 0, last_grid = 0;
};

// The list state of an inverted file and its search workspace (fx_ivf_lists.h).
// `quant` is the caller's coarse quantizer (borrowed).  row_list[r] is the list
// of payload row r (nlist: an assignment outside the lists); the rows are in
// list order once `dirty` is false.
struct IvfLists {
    FxIndex* quant = nullptr;
    int64_t nlist = 0;
    bool dirty = false;         // rows were appended since the last regroup
    bool sequential = false;    // ids are ntotal .. (an add without ids); decided by the first add
    int64_t max_list_rows = 0;  // of the last regroup
    std::vector<int> h_off;     // list_off on the host, read back with it ([nlist + 1])
    DevArr<int> list_off, max_rows;
    DevBuf rws;                 // the regroup's sort workspace
    DevBuf assign;              // a chunk's k = 1 search results
    // search workspace
    DevBuf qin, coarse_d, coarse_i, pkeys, psorted, seg, ngrp, gbase, ptemp, cand_d, cand_i, flag, outD, outI;
    int last_plan[3] = {0, 0, 0};  // path, chunks, slots
    int64_t last_qbatch = 0, last_grid = 0;
};

}  // namespace fx

// An inverted-file index (include/fx_index.h, fx_ivf.hip).  `pay` is the payload
// it owns: a labelled flat index, on whose stream and device everything runs.
struct FxIvf : fx::SearchStats, fx::IvfLists {
    FxIndex* pay = nullptr;
    int device = 0;  // pay's
    fx::DevArr<int> row_list;
    fx::DevBuf ids;  // sequential ids of an add
    fx::DevArr<unsigned long long> bad;  // assignments outside [0, nlist) since the last read
    fx::QueryBufs qb;
    std::mutex mu;
    hipStream_t stream() const { return pay->stream(); }
};

// A scalar-quantizer index (include/fx_index.h, fx_sq.hip): 8-bit signed codes
// (stride: the padded row), the rows' constants n_c, the trained tables
// [vmin | vdiff] and the index-wide bound words.
struct FxSq : fx::FlatCodes {
    int qtype = 0;
    bool train_open = false;  // fx_sq_train calls with more != 0 have accumulated min / max
    fx::DevArr<float> tables;
    fx::DevArr<unsigned> words, mm;
    fx::DevArr<unsigned long long> bad;
    fx::DevBuf sigma;
};

// A product quantizer index (include/fx_index.h "product quantizer", fx_pq.hip).  The fp32 centroids
// are the truth; the scan image and the three constants of the bound are rebuilt from them on the
// host whenever they are set.  Rows: stride = roundup(M, 16) code bytes and one fp32 n_y (nc) each.
struct FxPq : fx::FlatCodes {
    int M = 0, dsub = 0, kp = 0;
    std::vector<float> h_cb;     // [M][256][dsub], the host copy fx_pq_get_centroids returns
    double Y = 0, Ry = 0, Yl = 0;  // max |decode|, max |y - y_hi - y_lo|, max |y_lo| over any code row
    fx::DevArr<float> cb;
    fx::DevArr<char> img;        // dsub % 8 == 0: [hi | lo] bf16 planes of pq_plane_bytes each
    uint8_t* u8() const { return (uint8_t*)codes.p; }
};

// An inverted file over 8-bit codes (include/fx_index.h, fx_ivfsq.hip).  The payload is FxSq's rows
// with their labels and lists.  cent holds the quantizer's centroids widened to fp32 as they were
// when the tables were trained (by_residual only).
struct FxIvfSq : fx::Handle, fx::CodeRows, fx::IvfLists {
    int d = 0, qtype = 0, metric = fx::L2, by_residual = 1;
    bool trained = false, train_open = false;
    fx::DevArr<float> tables, cent;
    fx::DevArr<unsigned> words, mm;
    fx::DevArr<unsigned long long> bad;  // [0] non-finite training values, [1] assignments outside [0, nlist)
    // workspace of train / add / the accessors, and the search's pair operands
    fx::DevBuf in, tlist, resid, io, qf32, planes, sigma, peps, pshift;
};

// An inverted file over product-quantized codes (include/fx_index.h, fx_ivfpq.hip).  The payload is
// FxPq's rows with their labels and lists; the codebook, its scan image and constants are FxPq's.
// cent holds the quantizer's centroids widened to fp32 as they were when the codebook was set
// (by_residual only), rho_dec the rounding bound of fl32(c_l + decode) they give.
struct FxIvfPq : fx::Handle, fx::CodeRows, fx::IvfLists {
    int d = 0, M = 0, dsub = 0, kp = 0, metric = fx::L2, by_residual = 1;
    bool trained = false;
    std::vector<float> h_cb;     // [M][256][dsub], the host copy fx_ivfpq_get_centroids returns
    double Y = 0, Ry = 0, Yl = 0, rho_dec = 0;
    fx::DevArr<float> cb, cent;
    fx::DevArr<char> img;        // dsub % 8 == 0: [hi | lo] bf16 planes of pq_plane_bytes each
    fx::DevArr<unsigned long long> bad;  // [1] assignments outside [0, nlist) ([0] unused, as FxIvfSq's layout)
    // workspace of add / residuals / the accessors, and the search's operands
    fx::DevBuf in, tlist, resid, io, qf32, planes, peps, pshift;
    uint8_t* u8() const { return (uint8_t*)codes.p; }
};

// A selector (include/fx_index.h): the device image fx_select.hip builds of a
// subset of `index`'s rows [0, ntotal) as they were at creation.
struct FxSelector {
    const FxIndex* index = nullptr;  // identity only (never dereferenced: the index may be freed first)
    int device = 0;
    int64_t ntotal = 0;
    uint64_t epoch = 0;
    fx::DevArr<uint32_t> mask;      // sel_mask_words(ntotal) words
    fx::DevArr<int> tiles;          // [ceil(ntotal / TILE_R)] ascending live tiles
    fx::DevArr<fx::SelCounts> cnt;  // device counts (the scan reads cnt->tiles)
    // the counts on the host: copied stream-ordered into pinned memory after
    // the build, read (after `ready`) the first time someone asks
    fx::PinArr<fx::SelCounts> pin;
    hipEvent_t ready = nullptr;
    mutable bool known = false;
    mutable int64_t rows = 0, ntiles = 0;
    mutable std::mutex mu;
};
