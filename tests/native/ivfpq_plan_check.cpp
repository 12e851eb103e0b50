// ivfpq_plan_check.cpp -- prints what plan_ivfpq (csrc/fx_plan.cpp) decides over a fixed grid of
// shapes, one JSON line per case.  Pure host code: built from fx_plan.cpp alone (make ivfpqplan),
// runs without a GPU; the second build of the same program runs under AddressSanitizer + UBSan.
// tests/test_ivfpq_plan.py checks every line against what follows from the planner's definition.
#include <stdio.h>

#include "fx_plan.h"

int main() {
    const long long kNq[] = {1, 5, 37, 10000, 200000};
    const int kNprobe[] = {1, 8, 128, 1024};
    const long long kNlist[] = {16, 1024};
    const long long kMaxRows[] = {0, 129, 1000, 100000};
    const int kK[] = {1, 32, 33, 1024};
    const int kShape[][2] = {{16, 8}, {768, 8}, {1096, 8}, {20, 4}};  // d, dsub
    int n = 0;
    for (long long nq : kNq)
        for (int nprobe : kNprobe)
            for (long long nlist : kNlist)
                for (long long mr : kMaxRows)
                    for (int k : kK)
                        for (const auto& sh : kShape)
                            for (int per_pair = 0; per_pair < 2; ++per_pair) {
                                const int np = (int)(nprobe < nlist ? nprobe : nlist);
                                const fx::IvfPqPlan P =
                                    fx::plan_ivfpq(nq, np, nlist, mr, mr * nlist, k, sh[0], sh[1], per_pair);
                                const fx::IvfPlan Q = fx::plan_ivf(nq, np, nlist, mr, mr * nlist, k, 0);
                                printf("{\"nq\": %lld, \"nprobe\": %d, \"nprobe_eff\": %d, \"nlist\": %lld, "
                                       "\"max_list_rows\": %lld, \"k\": %d, \"d\": %d, \"dsub\": %d, \"per_pair\": %d, "
                                       "\"path\": %d, \"chunks\": %d, \"slots\": %d, \"q_batch\": %lld, \"grid\": %lld, "
                                       "\"pairs_pad\": %lld, \"op_rows\": %lld, \"plane_bytes\": %lld, "
                                       "\"cand_bytes\": %lld, \"ivf_chunks\": %d}\n",
                                       nq, nprobe, np, nlist, mr, k, sh[0], sh[1], per_pair, P.path, P.chunks, P.slots,
                                       (long long)P.q_batch, (long long)P.grid, (long long)P.pairs_pad,
                                       (long long)P.op_rows, (long long)P.plane_bytes, (long long)P.cand_bytes, Q.chunks);
                                ++n;
                            }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
