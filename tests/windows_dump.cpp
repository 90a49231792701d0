// Prints the window geometry rules of voice_activity_detection_amd/csrc/savad_windows.h, which this program includes alone
// (tests/test_window_geometry_host.py checks every line against numpy and the rules' one-line definitions).  Host C++ only.
//     windows_dump offsets HALF_MAX JUMP_MAX     "o half jump W refused : off_0 off_1 ..." (the offsets as a caller's int32_t[64] receives them)
//     windows_dump rules                         "i rows half items", "c chunk n_items even_chunk at_most_items", "l ... layout"
#include "savad_windows.h"

#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

using namespace savad;

int main(int argc, char** argv) {
    if (argc == 4 && argv[1][0] == 'o') {
        for (int half = 0; half <= atoi(argv[2]); ++half)
            for (int jump = 1; jump <= atoi(argv[3]); ++jump) {
                int32_t off[windows::MAX_FRAMES + 1];
                off[windows::MAX_FRAMES] = 12345;  // the guard: never written
                const long W = windows::offsets(half, jump, off);
                if (W != windows::offsets(half, jump, nullptr) || off[windows::MAX_FRAMES] != 12345) return 3;
                printf("o %d %d %ld '%s' :", half, jump, W, W > windows::MAX_FRAMES ? windows::TOO_LONG : "");
                for (long i = 0; i < W && i < windows::MAX_FRAMES; ++i) printf(" %d", off[i]);
                printf("\n");
            }
        return 0;
    }
    if (argc == 2 && argv[1][0] == 'r') {
        for (long rows : {0L, 1L, 37L, 38L, 39L, 40L, 1000L, 2147483647L})
            for (long half : {0L, 1L, 19L, 20L, 500L}) printf("i %ld %ld %ld\n", rows, half, windows::items(rows, half));
        for (long chunk : {1L, 2L, 3L, 7L, 8L, 999L, 1000L, 16384L, 2147483647L})
            for (int n : {0, 1, 2, 3, 7, 8, 9, 1000, 1001, 16384, 2147483647})
                printf("c %ld %d %d %d\n", chunk, n, windows::even_chunk(chunk, n), windows::at_most_items(chunk, n));
        const size_t cases[][6] = {{0, 1, 0, 7, 80, 0}, {0, 962, 962, 7, 80, 1000}, {65, 1, 1, 3, 13, 256}, {4, 5000, 1024, 63, 80, 123457}, {0, 96, 32, 7, 80, 4096}};
        for (const auto& c : cases) {
            const windows::Layout l = windows::layout(c[0], c[1], c[2], (int)c[3], (int)c[4], c[5]);
            printf("l %zu %zu %zu %zu %zu %zu : %zu %zu %zu %zu %zu\n", c[0], c[1], c[2], c[3], c[4], c[5], l.items_first, l.logp, l.windows, l.fwd, l.total);
        }
        return 0;
    }
    return 2;
}
