// ivf_plan_check.cpp -- prints what plan_ivf (csrc/fx_plan.cpp) decides over a
// fixed grid of shapes, one JSON line per case.  Pure host code: built from
// fx_plan.cpp alone (make ivfplan), runs without a GPU; the second build of the
// same program runs under AddressSanitizer + UBSan.  tests/test_ivf_plan.py
// checks every line against what follows from the planner's definition.
#include <stdio.h>

#include "fx_plan.h"

int main() {
    const long long kNq[] = {1, 16, 256, 10000};
    const int kNprobe[] = {1, 8, 128, 1024};
    const long long kNlist[] = {16, 1024, 65536};
    const long long kMaxRows[] = {0, 1, 127, 129, 100000};
    const int kK[] = {1, 32, 33, 1024};
    int n = 0;
    for (long long nq : kNq)
        for (int nprobe : kNprobe)
            for (long long nlist : kNlist)
                for (long long mr : kMaxRows)
                    for (int k : kK) {
                        const int np = (int)(nprobe < nlist ? nprobe : nlist);
                        const fx::IvfPlan P = fx::plan_ivf(nq, np, nlist, mr, mr * nlist, k, 1536);
                        printf("{\"nq\": %lld, \"nprobe\": %d, \"nprobe_eff\": %d, \"nlist\": %lld, \"max_list_rows\": %lld, "
                               "\"k\": %d, \"path\": %d, \"chunks\": %d, \"tiles_per_chunk\": %d, \"slots\": %d, "
                               "\"q_batch\": %lld, \"grid\": %lld}\n",
                               nq, nprobe, np, nlist, mr, k, P.path, P.chunks, P.tiles_per_chunk, P.slots,
                               (long long)P.q_batch, (long long)P.grid);
                        ++n;
                    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
