// fx_plan.cpp -- the launch planners: every grid shape, split count and chunk plan the host decides, as pure
// integer functions of the index's shape and options.  No HIP call: links without any kernel object
// (tests/native/plan_check.cpp, tests/test_plan_golden.py).
#include "fx_plan.h"

namespace fx {

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
void plan_scan(const IndexShape& ix, const Options& o, int64_t nq, int k, int v5_qt, ScanParams& p) {
    // the scan's shape: k_scan_v5 (64-row tiles x 256 queries) for the 16-bit
    // rows it has (not with the key-matrix dump, whose layout is k_scan_v4's)
    // ... when its wider query tiles add no padding work: v5 query slots within
    // 5 % of k_scan_v4's (nq = 256 on 1,536-B rows would scan 384 slots for
    // 256 queries: 5.59 against 3.61 ms, profiles/r6/ab_v5_d_r6e.txt; one-query
    // calls keep k_scan_v4's 128-query tile)
    const int v5qt = o.scan_v5 != 0 && !(o.scan_dbg & 32) ? v5_qt : 0;
    const int64_t slots4 = (nq + TILE_Q - 1) / TILE_Q * TILE_Q;
    const bool v5 = v5qt > 0 && (o.scan_v5 == 2 || (nq + v5qt - 1) / v5qt * v5qt * 20 <= slots4 * 21);
    p.qt = v5 ? v5qt : TILE_Q;
    p.tr = v5 ? V5_TR : TILE_R;
    p.n_qtiles = (int)((nq + p.qt - 1) / p.qt);
    p.n_ctiles = (int)((ix.ntotal + p.tr - 1) / p.tr);
    p.pub = nullptr;
    p.prune_rank = KP;
    // default 48: with the union bound deferred a compaction is cheap enough
    // that tightening the threshold 16 entries earlier pays (same-box sweep,
    // profiles/r4/ab/compact_r4c.txt: (d) -1.1 %, (b) and the N = 8 shard -0.2 %)
    p.compact_at = o.compact_at > KP && o.compact_at <= CAP ? o.compact_at : 48;
    p.share = k <= KP ? 1 : 0;
    p.union_w = 16;
    p.union_defer = o.union_defer;
    p.union_inplace = o.union_inplace >= 0 ? o.union_inplace : p.union_defer ? 0 : (1 << 30);
    // list re-bounding between compactions (k <= KP only; -1: the default)
    p.tight_at = p.share && o.tight_at > KP ? o.tight_at : 0;
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
    const int place = o.place >= 0 ? o.place : 1;
    SplitPlan sp = plan_splits(ntl, nct, min_tiles, place == 1, true);
    if (sp.place == 1) {
        const int max_sx = std::max(1, nct / (8 * min_tiles));
        if (o.sx > 0) sp.sx = std::max(1, std::min(max_sx, o.sx));  // placement A/B runs only
        if (k > KP) sp.sx = std::max(sp.sx, std::min(max_sx, ((k + 3) / 4 + 7) / 8));
        sp.splits = 8 * sp.sx;
    } else if (k > KP) {
        sp.splits = std::max(sp.splits, std::min(std::max(1, nct / min_tiles), (k + 3) / 4));
    }
    sp.store(p);
    // union-bound window (compact_regs): as many splits as there are, up to
    // 64, each contributing its first 256 / window published keys
    const int uw = o.union_w;
    p.union_w = uw == 16 || uw == 32 || uw == 64 ? uw : p.splits <= 16 ? 16 : p.splits <= 32 ? 32 : 64;
    // cold-start bound: pays on short splits, where a block's first record
    // tiles are a large share of its work
    const int cb = o.cold_bound;
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
void plan_sel_scan(const IndexShape& ix, int64_t nq, int k, ScanParams& p) {
    p.qt = TILE_Q;
    p.tr = TILE_R;
    p.n_qtiles = (int)((nq + TILE_Q - 1) / TILE_Q);
    p.n_ctiles = (int)((ix.ntotal + TILE_R - 1) / TILE_R);
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

// the range scan's grid: 128-query tiles x corpus splits, sized and placed by
// plan_splits as plan_scan's 128-row scans are (>= 3 tiles per split; corpus-
// partitioned over the XCDs once there are 8 x 3 tiles), from the shape
// alone -- no option enters, so none can change a result
void plan_range_scan(const IndexShape& ix, int64_t nq, ScanParams& p) {
    p.qt = TILE_Q;
    p.tr = TILE_R;
    p.n_qtiles = (int)((nq + TILE_Q - 1) / TILE_Q);
    p.n_ctiles = (int)((ix.ntotal + TILE_R - 1) / TILE_R);
    plan_splits(p.n_qtiles, p.n_ctiles, 3, true, false).store(p);
}

// which scan image the index's current options call for
int image_kind(const IndexShape& ix, const Options& o) {
    const int rb64 = ix.row_bytes / 64;
    if (ix.dtype == F32)
        return o.f32_split != 0 && ix.row_bytes % 64 == 0 && (rb64 == 8 || rb64 == 12 || rb64 == 16 || rb64 == 24)
                   ? IMG_F32S
                   : IMG_NONE;
    return ix.metric == L2 && o.centre != 0 ? IMG_C16 : IMG_NONE;
}

HostOut host_out_layout(int64_t nq, int k) {
    HostOut L;
    L.offI = (size_t)round_up(nq * k * 4, 8);
    L.offW = L.offI + (size_t)nq * k * 8;
    L.copy_bytes = L.offW + 8;
    L.bytes = L.offW + (size_t)(2 + nq) * 4;
    return L;
}

IvfPlan plan_ivf(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k,
                 int row_bytes) {
    // ntotal and row_bytes are part of the planner's signature but do not enter today: the chunk count
    // follows the longest list's tiles, whatever a tile costs.  `tiles` below is the planner's upper
    // bound on a list's tiles (tiles_per_chunk: for checks); k_ivf_scan divides each list's own tile
    // count by C, so only C, slots, q_batch and grid reach the launch.
    (void)ntotal;
    (void)row_bytes;
    IvfPlan P;
    P.path = k <= KP ? IVF_PATH_FUSED : IVF_PATH_EXACT;
    const int64_t np = std::max(1, nprobe_eff);
    const int64_t tiles = (std::max<int64_t>(max_list_rows, 0) + TILE_R - 1) / TILE_R + 1;
    const int64_t pairs = std::max<int64_t>(nq, 1) * np;
    int64_t C = 1;
    if (pairs < 256) {
        C = (512 + pairs - 1) / pairs;
        C = std::min<int64_t>(C, std::max<int64_t>(1, tiles / 4));
        C = std::min<int64_t>(C, 64);
    }
    P.chunks = (int)C;
    P.tiles_per_chunk = (int)((tiles + C - 1) / C);
    P.slots = (int)(np * C);
    const int64_t per_query = (int64_t)P.slots * (P.path == IVF_PATH_FUSED ? KP : k) * 8;
    P.q_batch = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(nq, 1), IVF_CAND_BYTES / per_query));
    const int64_t bp = P.q_batch * np;
    P.grid = (bp / TILE_Q + std::min<int64_t>(nlist, bp)) * C;
    return P;
}

IvfSqPlan plan_ivfsq(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k,
                     int row_bytes) {
    IvfSqPlan P;
    static_cast<IvfPlan&>(P) = plan_ivf(nq, nprobe_eff, nlist, max_list_rows, ntotal, k, row_bytes);
    const int64_t np = std::max(1, nprobe_eff);
    const int64_t rb = std::max(1, row_bytes);
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t cand_q = (int64_t)P.slots * (fused ? KP : k) * 8;
    if (fused) {
        // a query costs its np operands and its lists; the padding of the pair count costs < 128 operands
        const int64_t per_query = (int64_t)SQ_P * np * rb + cand_q;
        const int64_t room = IVFSQ_PASS_BYTES - (int64_t)SQ_P * (TILE_Q - 1) * rb;
        P.q_batch = std::max<int64_t>(1, std::min<int64_t>(P.q_batch, room / per_query));
        const int64_t bp = P.q_batch * np;
        P.grid = (bp / TILE_Q + std::min<int64_t>(nlist, bp)) * P.chunks;
        P.pairs_pad = (bp + TILE_Q - 1) / TILE_Q * TILE_Q;
        P.plane_bytes = (int64_t)SQ_P * P.pairs_pad * rb;
    }
    P.cand_bytes = P.q_batch * cand_q;
    return P;
}

// the exact scan for a whole search: xs corpus splits per query, the most queries whose [query][xsplit][k]
// lists fit SQ_CAND_BYTES
static SqPlan sq_exact_plan(int64_t nq, int xs, int k) {
    SqPlan P;
    P.path = SQ_PATH_EXACT;
    P.xsplits = xs;
    P.splits = 1;
    P.q_batch = std::max<int64_t>(1, std::min<int64_t>(nq, SQ_CAND_BYTES / ((int64_t)xs * k * 8)));
    P.qtiles = (int)((P.q_batch + TILE_Q - 1) / TILE_Q);
    P.grid = SQ_EXACT_GRID;
    P.cand_bytes = P.q_batch * xs * k * 8;
    return P;
}

SqPlan plan_sq(int64_t nq, int64_t ntotal, int k, int row_bytes) {
    // row_bytes is part of the signature but does not enter today: a tile's cost does not change how
    // many workgroups fill the CUs
    (void)row_bytes;
    SqPlan P;
    P.path = k <= KP ? SQ_PATH_FUSED : SQ_PATH_EXACT;
    nq = std::max<int64_t>(nq, 1);
    const int nct = (int)std::max<int64_t>(1, (ntotal + TILE_R - 1) / TILE_R);
    const int xs = (int)std::max<int64_t>(1, std::min<int64_t>(64, ntotal / 1024));
    if (P.path == SQ_PATH_EXACT) return sq_exact_plan(nq, xs, k);
    constexpr int min_tiles = 3;
    const int64_t per_list = (int64_t)TILE_Q * KP * 8;
    int64_t qb = nq;
    for (;;) {
        const int ntl = (int)((qb + TILE_Q - 1) / TILE_Q);
        const int splits = fill_splits(ntl, ntl, nct, min_tiles);
        P.qtiles = ntl;
        P.splits = splits;
        P.q_batch = qb;
        P.cand_bytes = (int64_t)ntl * splits * per_list;
        if (P.cand_bytes <= SQ_CAND_BYTES || ntl == 1) break;
        qb = (int64_t)(ntl / 2) * TILE_Q;
    }
    P.xsplits = std::min(P.splits, xs);
    P.grid = (int64_t)P.qtiles * P.splits;
    return P;
}

SqPlan plan_pq(int64_t nq, int64_t ntotal, int k, int M, int dsub) {
    // M does not enter: a tile's cost does not change how many workgroups fill the CUs
    (void)M;
    if (dsub % 8 == 0) return plan_sq(nq, ntotal, k, 0);
    const int xs = (int)std::max<int64_t>(1, std::min<int64_t>(64, ntotal / 1024));
    return sq_exact_plan(std::max<int64_t>(nq, 1), xs, k);
}

IvfPqPlan plan_ivfpq(int64_t nq, int nprobe_eff, int64_t nlist, int64_t max_list_rows, int64_t ntotal, int k, int d,
                     int dsub, int per_pair) {
    IvfPqPlan P;
    static_cast<IvfPlan&>(P) = plan_ivf(nq, nprobe_eff, nlist, max_list_rows, ntotal, k, 0);
    const int64_t np = std::max(1, nprobe_eff);
    if (dsub <= 0 || dsub % 8 != 0) P.path = IVF_PATH_EXACT;
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t cand_q = (int64_t)P.slots * (fused ? KP : k) * 8;
    // (plan_ivf sized q_batch for the fused lists; the exact path's are slots * k entries)
    P.q_batch = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(nq, 1), IVF_CAND_BYTES / cand_q));
    if (fused) {
        // a query costs its operands (np, or one) and its lists; the padding costs < 128 operands
        const int64_t op = 4 * (int64_t)pq_kpad(std::max(1, d));
        const int64_t per_query = (per_pair ? np : 1) * op + cand_q;
        const int64_t room = IVFPQ_PASS_BYTES - (TILE_Q - 1) * op;
        P.q_batch = std::max<int64_t>(1, std::min<int64_t>(P.q_batch, room / per_query));
        const int64_t bp = P.q_batch * np;
        P.pairs_pad = (bp + TILE_Q - 1) / TILE_Q * TILE_Q;
        P.op_rows = per_pair ? P.pairs_pad : (P.q_batch + TILE_Q - 1) / TILE_Q * TILE_Q;
        P.plane_bytes = P.op_rows * op;
    }
    const int64_t bp = P.q_batch * np;
    P.grid = (bp / TILE_Q + std::min<int64_t>(nlist, bp)) * P.chunks;
    P.cand_bytes = P.q_batch * cand_q;
    return P;
}

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

}  // namespace fx
