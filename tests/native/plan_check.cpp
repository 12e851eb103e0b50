// plan_check.cpp -- prints what the launch planners of csrc/fx_plan.cpp decide
// for a fixed grid of shapes, one JSON line per case.  Pure host code: built
// from fx_plan.cpp alone (make plan), runs without a GPU.
// tests/test_plan_golden.py compares every line with tests/golden/scan_plans.json.
//
// The calls below the PLAN_CHECK_PLANNERS seam are all this file needs from the
// planners; the golden was recorded by compiling this same case list against
// the planners of the commit before they moved into fx_plan.cpp.
#include <stdio.h>

#include <string>
#include <vector>

#ifndef PLAN_CHECK_PLANNERS
#include "fx_plan.h"
using namespace fx;

// queries per k_scan_v5 workgroup for these rows: fx_scan5.hip's scan_v5_qt
// (a kernel object, which this program does not link)
static int v5_qt_of(int st_dt, int row_bytes) {
    if (st_dt != BF16 && st_dt != F16) return 0;
    return row_bytes == 512 || row_bytes == 768 ? 256 : row_bytes == 1536 ? 192 : 0;
}
static void call_plan_scan(const IndexShape& ix, const Options& o, int64_t nq, int k, ScanParams& p) {
    plan_scan(ix, o, nq, k, v5_qt_of(ix.img_kind == IMG_F32S ? (int)F32S : ix.dtype, ix.row_bytes), p);
}
static void call_plan_sel_scan(const IndexShape& ix, int64_t nq, int k, ScanParams& p) { plan_sel_scan(ix, nq, k, p); }
static void call_plan_range_scan(const IndexShape& ix, int64_t nq, ScanParams& p) { plan_range_scan(ix, nq, p); }
static int call_image_kind(const IndexShape& ix, const Options& o) { return image_kind(ix, o); }
#endif

namespace {

struct Row {
    const char* name;
    int dtype, d, img_kind;
};
const Row kRows[] = {
    {"f32 d=384", F32, 384, IMG_F32S}, {"f32 d=100", F32, 100, IMG_NONE},  {"bf16 d=256", BF16, 256, IMG_C16},
    {"f16 d=384", F16, 384, IMG_C16},  {"bf16 d=768", BF16, 768, IMG_C16}, {"bf16 d=100", BF16, 100, IMG_C16},
};
const int64_t kNtotal[] = {1, 128, 129, 383, 384, 1535, 1536, 3071, 3072, 100000, 1000000, 10000000};
const int64_t kNq[] = {1, 128, 129, 192, 193, 256, 257, 1024, 1025, 2048, 4096};
// k, then the re-scan's k1 = min(2048, max(512, 4k)) of those k
const int kK[] = {1, 10, 32, 33, 100, 1024, 512, 2048};
// the option cases run on this thinned grid
const int64_t kNtotalThin[] = {129, 3072, 100000, 10000000};
const int64_t kNqThin[] = {1, 193, 1024, 4096};
const int kKThin[] = {10, 100, 512};

struct OptCase {
    const char* name;
    void (*set)(Options&);
};
const OptCase kOpts[] = {
    {"scan_place=0", [](Options& o) { o.place = 0; }},     {"scan_sx=3", [](Options& o) { o.sx = 3; }},
    {"scan_v5=0", [](Options& o) { o.scan_v5 = 0; }},      {"scan_v5=2", [](Options& o) { o.scan_v5 = 2; }},
    {"union_w=32", [](Options& o) { o.union_w = 32; }},    {"cold_bound=0", [](Options& o) { o.cold_bound = 0; }},
    {"cold_bound=1", [](Options& o) { o.cold_bound = 1; }}, {"compact_at=40", [](Options& o) { o.compact_at = 40; }},
    {"tight_at=40", [](Options& o) { o.tight_at = 40; }},
};

IndexShape shape(const Row& r, int64_t ntotal) {
    IndexShape ix{};
    ix.ntotal = ntotal;
    ix.row_bytes = (int)round_up((int64_t)r.d * dtype_size(r.dtype), ROW_ALIGN);
    ix.dtype = r.dtype;
    ix.metric = L2;
    ix.img_kind = r.img_kind;
    return ix;
}

void print_scan(const std::string& group, int64_t nq, int k, const ScanParams& p) {
    printf("{\"group\": \"%s\", \"nq\": %lld, \"k\": %d, \"qt\": %d, \"tr\": %d, \"n_qtiles\": %d, \"n_ctiles\": %d, "
           "\"place\": %d, \"sx\": %d, \"splits\": %d, \"qt_per_xcd\": %d, \"grid\": %d, \"share\": %d, \"union_w\": %d, "
           "\"compact_at\": %d, \"tight_at\": %d, \"cold_bound\": %d, \"union_defer\": %d, \"union_inplace\": %d}\n",
           group.c_str(), (long long)nq, k, p.qt, p.tr, p.n_qtiles, p.n_ctiles, p.place, p.sx, p.splits, p.qt_per_xcd,
           p.grid, p.share, p.union_w, p.compact_at, p.tight_at, p.cold_bound, p.union_defer, p.union_inplace);
}

template <size_t NN, size_t NQ, size_t NK>
void scan_cases(const char* opt_name, const Options& o, const int64_t (&ntotals)[NN], const int64_t (&nqs)[NQ],
                const int (&ks)[NK]) {
    for (const Row& r : kRows)
        for (int64_t nt : ntotals) {
            const std::string group = std::string("plan_scan|") + r.name + "|" + opt_name + "|ntotal=" + std::to_string(nt);
            for (int64_t nq : nqs)
                for (int k : ks) {
                    ScanParams p{};
                    call_plan_scan(shape(r, nt), o, nq, k, p);
                    print_scan(group, nq, k, p);
                }
        }
}

// ---- plan_remove: the chunk plan of a mask (a set bit: the row is removed) ----

struct Mask {
    const char* name;
    bool (*removed)(int64_t r, int64_t nt);
};
const Mask kMasks[] = {
    {"first", [](int64_t r, int64_t) { return r == 0; }},
    {"last", [](int64_t r, int64_t nt) { return r == nt - 1; }},
    {"every-other", [](int64_t r, int64_t) { return r % 2 == 1; }},
    {"middle-block", [](int64_t r, int64_t nt) { return r >= nt / 3 && r < nt / 3 + std::max<int64_t>(1, nt / 4); }},
    {"all-but-one", [](int64_t r, int64_t nt) { return r != nt / 2; }},
};

void remove_cases() {
    const int64_t G = RM_GROUP_ROWS;
    for (int64_t nt : {(int64_t)1, (int64_t)33, G - 1, G + 1, 3 * G + 5})
        for (const Mask& m : kMasks) {
            // what remove_rows reads back from the device: the kept rows before every mask word and group
            const int64_t nw = sel_mask_words(nt), ngp = rm_groups(nt);
            std::vector<unsigned> words((size_t)nw, 0u), mask((size_t)nw, 0u), gp((size_t)ngp, 0u);
            int64_t kept = 0, first = nt;
            for (int64_t r = 0; r < nw * 32; ++r) {
                if (r % 32 == 0) words[(size_t)(r / 32)] = (unsigned)kept;
                if (r % G == 0) gp[(size_t)(r / G)] = (unsigned)kept;
                if (r >= nt) continue;
                if (m.removed(r, nt)) {
                    mask[(size_t)(r / 32)] |= 1u << (r % 32);
                    first = std::min(first, r);
                } else {
                    ++kept;
                }
            }
            if (first == nt) continue;  // (nothing removed: remove_ids returns before it plans)
            int64_t last_stage = 0;
            for (int64_t want : {(int64_t)1, (int64_t)7, G, nt}) {
                const int64_t stage_rows = std::min(want, nt);
                if (stage_rows == last_stage) continue;
                last_stage = stage_rows;
                KeptPrefix P;
                P.ntotal = nt;
                P.first = first;
                P.kept = kept;
                P.g = stage_rows < std::min<int64_t>(G, nt) ? 1 : G;
                if (P.g == 1) {
                    P.words = words;
                    P.mask = mask;
                } else {
                    P.gp = gp;
                }
                std::vector<RemoveChunk> plan;
                const bool ok = plan_remove(P, stage_rows, plan);
                printf("{\"group\": \"plan_remove|ntotal=%lld|%s\", \"stage_rows\": %lld, \"first\": %lld, \"kept\": %lld, "
                       "\"ok\": %d, \"chunks\": [",
                       (long long)nt, m.name, (long long)stage_rows, (long long)first, (long long)kept, ok ? 1 : 0);
                for (size_t i = 0; i < plan.size(); ++i)
                    printf("%s[%lld, %lld, %lld, %lld, %d]", i ? ", " : "", (long long)plan[i].s0, (long long)plan[i].s1,
                           (long long)plan[i].d0, (long long)plan[i].kept, plan[i].direct ? 1 : 0);
                printf("]}\n");
            }
        }
}

}  // namespace

int main() {
    const Options dflt;
    scan_cases("default", dflt, kNtotal, kNq, kK);
    for (const OptCase& oc : kOpts) {
        Options o;
        oc.set(o);
        scan_cases(oc.name, o, kNtotalThin, kNqThin, kKThin);
    }
    // the filtered scan's and the range scan's plans read the shape alone (128-row tiles over the stored rows)
    for (int64_t nt : kNtotal) {
        const IndexShape ix = shape(kRows[4], nt);
        for (int64_t nq : kNq) {
            for (int k : kK) {
                ScanParams p{};
                call_plan_sel_scan(ix, nq, k, p);
                print_scan("plan_sel_scan|ntotal=" + std::to_string(nt), nq, k, p);
            }
            ScanParams p{};
            call_plan_range_scan(ix, nq, p);
            print_scan("plan_range_scan|ntotal=" + std::to_string(nt), nq, 0, p);
        }
    }
    for (const Row& r : kRows) {
        Options off;
        off.f32_split = 0;
        off.centre = 0;
        printf("{\"group\": \"image_kind|%s\", \"default\": %d, \"off\": %d}\n", r.name,
               call_image_kind(shape(r, 1000), dflt), call_image_kind(shape(r, 1000), off));
    }
    for (int k : kK)
        printf("{\"group\": \"big_k1\", \"k\": %d, \"k1\": %d, \"small_many\": [%d, %d, %d]}\n", k, big_k1(k),
               (int)small_many(k, 256, 64), (int)small_many(k, 257, 64), (int)small_many(k, 1, 63));
    const int64_t ho[][2] = {{1, 1}, {1, 10}, {3, 5}, {64, 1024}};
    for (const auto& c : ho) {
        const HostOut L = host_out_layout(c[0], (int)c[1]);
        printf("{\"group\": \"host_out_layout\", \"nq\": %lld, \"k\": %lld, \"offI\": %zu, \"offW\": %zu, \"copy_bytes\": %zu, "
               "\"bytes\": %zu}\n", (long long)c[0], (long long)c[1], L.offI, L.offW, L.copy_bytes, L.bytes);
    }
    remove_cases();
    return 0;
}
