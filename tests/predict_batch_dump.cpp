// Prints plan_predict_batch (voice_activity_detection_amd/csrc/savad_schedule.h) for ONE case named on the command line:
//     predict_batch_dump precision row_mode F chunk half jump N_0 N_1 ...      (N_c = rows of clip c; "-" in place of the lengths: C = 0)
//     predict_batch_dump ... table v_0 v_1 ...                                  (the table itself, for tables that are none)
// One line: the plan's fields, the forwards it runs as first:count pairs, and the workspace each of them asks for
// (tests/test_predict_batch_host.py checks the line against its own arithmetic).  Host C++ only.
#include "savad_schedule.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace savad::sched;

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    Knobs k;
    k.precision = atoi(argv[1]);
    k.row_mode = atoi(argv[2]);
    k.feature_size = atoi(argv[3]);
    k.FP = (k.feature_size + 15) / 16 * 16;
    k.num_layers = 3;
    const int chunk = atoi(argv[4]), half = atoi(argv[5]), jump = atoi(argv[6]);
    std::vector<int32_t> table;
    if (!strcmp(argv[7], "table")) {
        for (int i = 8; i < argc; ++i) table.push_back((int32_t)atol(argv[i]));
    } else if (strcmp(argv[7], "-")) {
        table.push_back(0);
        for (int i = 7; i < argc; ++i) table.push_back((int32_t)(table.back() + atol(argv[i])));
    }
    const int C = (int)table.size() - 1;
    const PredictBatchPlan p = plan_predict_batch(k, table.empty() ? nullptr : table.data(), C, half, jump, chunk);
    if (p.err) {
        printf("err %d '%s'\n", p.err, p.msg ? p.msg : "");
        return 0;
    }
    printf("W %d C %d rows %d items %d chunk %d items_first %zu logp %zu windows %zu fwd %zu fwd_bytes %zu total %zu :", p.W, p.C, p.rows,
           p.n_items, p.chunk, p.items_first, p.logp, p.windows, p.fwd, p.fwd_bytes, p.total);
    for (int first = 0; first < p.n_items; first += p.chunk) {
        const int count = p.n_items - first < p.chunk ? p.n_items - first : p.chunk;
        printf(" %d:%d:%zu", first, count, plan_forward(k, count, p.W, false, 0).total);
    }
    printf("\n");
    return 0;
}
