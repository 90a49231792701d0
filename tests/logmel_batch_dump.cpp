// Prints the host plan of the log-mel front-end over a clip table (voice_activity_detection_amd/csrc/savad_logmel_batch_plan.h) and the
// pad rule it shares with savad_logmel_span and the kernels (mel::pad_rule, mel::pad_source in savad_audio_host.h):
//     logmel_batch_dump plan audio_count first:count first:count ...      ("-" in place of the clips: C = 0)
//         one line: rows, tiles, the workspace offsets, then clip_first and tiles_first; or err CODE 'message'
//     logmel_batch_dump rule n_lo n_hi
//         one line per signal length n: the whole signal's rule, then the sample each element of stretch A and of stretch B stands for
// (tests/test_logmel_batch_host.py checks both against its own arithmetic).  Host C++ only.
#include "savad_logmel_batch_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace savad;

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "rule")) {
        for (long n = atol(argv[2]); n <= atol(argv[3]); ++n) {
            const mel::PadRule r = mel::pad_rule(n, 0, melbatch::frames_of(n));
            printf("%ld %ld %d %ld %ld %d %ld %ld :", n, r.a_j0, r.a_count, r.a_end, r.b_j0, r.b_count, r.j_first, r.j_last);
            for (int k = 0; k < r.a_count; ++k) printf(" %ld", mel::pad_source(r.a_j0 + k, n));
            printf(" :");
            for (int k = 0; k < r.b_count; ++k) printf(" %ld", mel::pad_source(r.b_j0 + k, n));
            printf("\n");
        }
        return 0;
    }
    if (argc < 4 || strcmp(argv[1], "plan")) return 2;
    const int64_t audio_count = atoll(argv[2]);
    std::vector<melbatch::Clip> clips;
    if (strcmp(argv[3], "-"))
        for (int i = 3; i < argc; ++i) {
            const char* colon = strchr(argv[i], ':');
            if (!colon) return 2;
            clips.push_back(melbatch::Clip{atoll(argv[i]), atoll(colon + 1)});
        }
    const int C = (int)clips.size();
    std::vector<int32_t> clip_first((size_t)C + 1), tiles_first((size_t)C + 1);
    const melbatch::Plan p = melbatch::plan(clips.empty() ? nullptr : clips.data(), C, audio_count, clip_first.data(), tiles_first.data());
    if (p.err) {
        printf("err %d '%s'\n", p.err, p.msg);
        return 0;
    }
    printf("C %d rows %lld tiles %lld tiles_first %zu head %zu tail %zu total %zu head_slot %d tail_slot %d :", p.C, (long long)p.rows,
           (long long)p.tiles, p.tiles_first, p.head, p.tail, p.total, melbatch::HEAD_SLOT, melbatch::TAIL_SLOT);
    for (int32_t v : clip_first) printf(" %d", v);
    printf(" :");
    for (int32_t v : tiles_first) printf(" %d", v);
    printf("\n");
    return 0;
}
