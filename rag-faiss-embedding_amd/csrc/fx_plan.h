// fx_plan.h -- the launch planners (fx_plan.cpp): pure integer logic over an
// index's shape (IndexShape) and options.  They decide every grid shape and
// chunk plan the host launches, make no HIP call, and are checked against a
// golden on the CPU (tests/test_plan_golden.py).
#pragma once
#include "fx_host.h"

namespace fx {

// split count whose live workgroups (one per CU: the scan's LDS) fill whole
// rounds of 256 CUs best, with >= ~4 rounds and >= min_tiles tiles per split
int fill_splits(int live_tiles, int eff_tiles, int n_ctiles, int min_tiles);

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
SplitPlan plan_splits(int ntl, int nct, int min_tiles, bool partition, bool group_qtiles);

// The scan's grid (fx_plan.cpp has the reasoning at each definition).  v5_qt:
// k_scan_v5's query tile for the rows' scan dtype (scan_v5_qt; 0: it has no
// shape for them) -- passed in, so that this file needs no kernel object.
void plan_scan(const IndexShape& ix, const Options& o, int64_t nq, int k, int v5_qt, ScanParams& p);
void plan_sel_scan(const IndexShape& ix, int64_t nq, int k, ScanParams& p);
void plan_range_scan(const IndexShape& ix, int64_t nq, ScanParams& p);
int big_k1(int k);
bool small_many(int k, int64_t nq, int splits);
// which scan image the shape (dtype, row_bytes, metric) and options call for
int image_kind(const IndexShape& ix, const Options& o);

// Host-output searches (the reference's call form) return through ONE packed
// device buffer, copied back with one D2H:
//   [D: nq k f32 | I: nq k i64 | n_drop | n_flag | flag list: nq i32]
// (the copy covers D .. n_flag; the flag list stays on the device for the
// fallback chain)
struct HostOut {
    size_t offI = 0, offW = 0, copy_bytes = 0, bytes = 0;
};
HostOut host_out_layout(int64_t nq, int k);

// ---- inverted file (fx_ivf.hip): the plan of one IndexIVFFlat search ---------

// path: the fused MFMA list scan + refine (k <= KP), or the exact list scan
// (k_ivf_exact) for the whole search.
enum { IVF_PATH_FUSED = 0, IVF_PATH_EXACT = 1 };
struct IvfPlan {
    int path = IVF_PATH_FUSED;
    int chunks = 1;           // C: tile chunks per probed list
    int tiles_per_chunk = 1;  // ceil(tiles of the longest list / C): an upper bound for checks only -- the
                              // kernel divides each list's own tiles by C itself
    int slots = 1;            // candidate lists per query: nprobe_eff * C
    int64_t q_batch = 1;      // queries per pass
    int64_t grid = 0;         // upper bound of the list scan's workgroups in a pass
};
// candidate bytes a pass may hold (entries of 8 B: key + row)
constexpr int64_t IVF_CAND_BYTES = 1ll << 30;
// A list of r rows whose start is aligned down to 4 rows touches up to
// ceil(r / 128) + 1 tiles.  C > 1 only when a pass has fewer than 256 (query,
// list) pairs: then the pairs alone cannot fill the CUs, and each list is cut
// into chunks of >= 4 tiles until ~512 workgroups exist (at most 64 chunks).
// q_batch: the most queries whose candidate lists (slots * KP entries each;
// exact path: slots * k) fit IVF_CAND_BYTES.  grid: a pass of P = q_batch *
// nprobe_eff pairs forms sum_l ceil(c_l / 128) <= P / 128 + min(nlist, P) query
// groups, each scanned by C workgroups.
IvfPlan plan_ivf(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k,
                 int row_bytes);

// ---- scalar quantizer (fx_sq.hip): the plan of one IndexScalarQuantizer search

// path: the fused int8 MFMA scan + refine (k <= KP), or the exact scan
// (k_sq_exact) for the whole search.
enum { SQ_PATH_FUSED = 0, SQ_PATH_EXACT = 1 };
struct SqPlan {
    int path = SQ_PATH_FUSED;
    int qtiles = 1;       // query tiles of a full pass: ceil(q_batch / 128)
    int splits = 1;       // corpus splits per query tile (fused), <= corpus tiles
    int xsplits = 1;      // corpus splits per query of the exact scan: the whole search on the exact
                          // path, the flagged queries on the fused one (then <= splits, so that the
                          // fused pass's candidate buffer holds them)
    int64_t q_batch = 1;  // queries per pass
    int64_t grid = 0;     // workgroups of a full pass's scan (fused: qtiles * splits; exact: the fixed grid)
    int64_t cand_bytes = 0;  // candidate bytes of a full pass (entries of 8 B: key + row)
};
constexpr int64_t SQ_CAND_BYTES = 1ll << 30;
// Fused: the splits of fill_splits (>= 3 tiles each, whole rounds of 256 CUs, ~1,024 workgroups for a
// small batch), and the most queries per pass whose [qtile][split][128][KP] lists fit SQ_CAND_BYTES.
// Exact: up to 64 splits of >= 1,024 rows, and the most queries whose [query][xsplit][k] lists fit.
SqPlan plan_sq(int64_t nq, int64_t ntotal, int k, int row_bytes);

// ---- product quantizer (fx_pq.hip): the plan of one IndexPQ search

// plan_sq's plan with one more reason for the exact path: the fused gather scan stages 16-B pieces of
// a centroid, so it needs dsub % 8 == 0; any other dsub takes the exact scan (k_pq_exact) at every k.
SqPlan plan_pq(int64_t nq, int64_t ntotal, int k, int M, int dsub);

// ---- inverted file over 8-bit codes (fx_ivfsq.hip): the plan of one IndexIVFScalarQuantizer search

// plan_ivf's path, chunks, slots and grid; q_batch additionally keeps the pass's operand planes
// (SQ_P * pairs_pad * row_bytes, one operand per (query, probe) pair) plus its candidate lists
// within IVFSQ_PASS_BYTES.
struct IvfSqPlan : IvfPlan {
    int64_t pairs_pad = 0;    // roundup(q_batch * nprobe_eff, 128): plane rows of a full pass
    int64_t plane_bytes = 0;  // SQ_P * pairs_pad * row_bytes (exact path: 0, it prepares no operand)
    int64_t cand_bytes = 0;   // q_batch * slots * (KP or k) * 8
};
constexpr int64_t IVFSQ_PASS_BYTES = 1ll << 30;
IvfSqPlan plan_ivfsq(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k,
                     int row_bytes);

// ---- inverted file over product-quantized codes (fx_ivfpq.hip): the plan of one IndexIVFPQ search

// plan_ivfsq with the product quantizer's operands and one more reason for the exact path: path is
// exact for k > KP and for every dsub that is no multiple of 8 (plan_pq's rule).  An operand is two
// bf16 planes of kpad(d) = roundup(d, 32) values, 4 kpad(d) bytes; per_pair != 0 (L2 with by_residual)
// there is one per (query, probe) pair, otherwise one per query.  q_batch keeps the operand planes
// plus the candidate lists of a pass within IVFPQ_PASS_BYTES.
struct IvfPqPlan : IvfPlan {
    int64_t pairs_pad = 0;    // roundup(q_batch * nprobe_eff, 128)
    int64_t op_rows = 0;      // plane rows of a full pass: pairs_pad, or roundup(q_batch, 128) (exact path: 0)
    int64_t plane_bytes = 0;  // 2 * op_rows * kpad(d) * 2 (exact path: 0, it prepares no operand)
    int64_t cand_bytes = 0;   // q_batch * slots * (KP or k) * 8
};
constexpr int64_t IVFPQ_PASS_BYTES = 1ll << 30;
IvfPqPlan plan_ivfpq(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k, int d,
                     int dsub, int per_pair);

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
bool plan_remove(const KeptPrefix& P, int64_t stage_rows, std::vector<RemoveChunk>& out);

}  // namespace fx
