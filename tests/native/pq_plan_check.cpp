// pq_plan_check.cpp -- prints what plan_pq (csrc/fx_plan.cpp) decides over a
// fixed grid of shapes, one JSON line per case.  Pure host code: built from
// fx_plan.cpp alone (make pqplan), runs without a GPU; the second build of the
// same program runs under AddressSanitizer + UBSan.  tests/test_pq_plan.py
// checks every line against what follows from the planner's definition.
#include <stdio.h>

#include "fx_plan.h"

int main() {
    const long long kNq[] = {1, 16, 128, 129, 10000, 8000000};
    const long long kRows[] = {1, 127, 128, 129, 1000, 20000, 1000000, 100000000};
    const int kK[] = {1, 10, 32, 33, 1024};
    const int kShape[][2] = {{96, 8}, {8, 4}, {2, 8}, {6, 16}, {16, 3}};  // (M, dsub)
    int n = 0;
    for (long long nq : kNq)
        for (long long rows : kRows)
            for (int k : kK)
                for (const auto& sh : kShape) {
                    const fx::SqPlan P = fx::plan_pq(nq, rows, k, sh[0], sh[1]);
                    printf("{\"nq\": %lld, \"ntotal\": %lld, \"k\": %d, \"M\": %d, \"dsub\": %d, \"path\": %d, "
                           "\"qtiles\": %d, \"splits\": %d, \"xsplits\": %d, \"q_batch\": %lld, \"grid\": %lld, "
                           "\"cand_bytes\": %lld}\n",
                           nq, rows, k, sh[0], sh[1], P.path, P.qtiles, P.splits, P.xsplits, (long long)P.q_batch,
                           (long long)P.grid, (long long)P.cand_bytes);
                    ++n;
                }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
