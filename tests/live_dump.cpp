// Prints the host plan of the live mode (voice_activity_detection_amd/csrc/savad_live_plan.h) for tests/test_live_host.py.  Host C++ only.
//   live_dump counts <half> <n_max>                                   one line per n: n K E N rows_at_finish
//   live_dump sim <streams> <max_push> <half> <jump> <tick> ...       a tick is slot:count[f][,slot:count[f]...]; a slot opens at its
//                                                                     first mention (and again after a finish); per tick the tables
#include "savad_live_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace savad::live;

int main(int argc, char** argv) {
    if (argc >= 4 && std::string(argv[1]) == "counts") {
        const int half = atoi(argv[2]);
        const long n_max = atol(argv[3]);
        for (long n = 0; n <= n_max; ++n) {
            const long K = ready_frames(n), N = total_frames(n);
            printf("%ld %ld %ld %ld %ld %ld\n", n, K, final_rows(K, half), N, N - final_rows(K, half), keep_from(n));
        }
        return 0;
    }
    if (argc < 6 || std::string(argv[1]) != "sim") return 2;
    const Geometry g = geometry(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (g.err) {
        printf("X %d %s\n", g.err, g.msg);
        return 0;
    }
    printf("G %d %d %d %d %d %d %d %zu %d %d\n", g.W, g.P, g.max_new, g.max_rows, g.feat_cap, g.logp_cap, g.sample_cap, g.stride, g.max_tiles(),
           g.max_items());
    std::vector<Slot> slots(g.streams, Slot{0, 0, 0, 0});
    const uint64_t state = 1ull << 32;
    for (int a = 6; a < argc; ++a) {
        std::vector<Push> pushes;
        for (const char* s = argv[a]; *s;) {
            char* end;
            Push p{};
            p.slot = (int32_t)strtol(s, &end, 10);
            if (*end != ':') return 2;
            p.count = (int32_t)strtol(end + 1, &end, 10);
            p.dtype = 1;
            p.data = 1ull << 40;
            if (*end == 'f') p.finish = 1, ++end;
            if (*end == ',') ++end;
            s = end;
            if (p.slot >= 0 && p.slot < g.streams && !slots[p.slot].open) slots[p.slot] = Slot{0, 0, 1, 0};
            pushes.push_back(p);
        }
        std::vector<char> table(table_bytes(g, (int)pushes.size()));
        std::vector<int64_t> rows(2 * pushes.size() + 2);
        const PlanResult r = plan_tick(g, slots.data(), pushes.data(), (int)pushes.size(), state, table.data(), table.size(), rows.data());
        if (r.err) {
            printf("X %d %s\n", r.err, r.msg);
            continue;
        }
        const Header* h = header(table.data());
        printf("T %d %d %d %d %d %d\n", h->n_entries, h->n_tiles, h->n_items, h->n_rows, h->total, h->max_append);
        const Entry* e = entries(table.data());
        const Tile* t = (const Tile*)(table.data() + h->o_tiles);
        const Item* it = (const Item*)(table.data() + h->o_items);
        const int32_t* ro = (const int32_t*)(table.data() + h->o_rows);
        for (int i = 0; i < h->n_entries; ++i)
            printf("E %d %d %ld %ld %ld %ld %d %d %ld %d %d %d %d %d %d %d %d %d %d %ld %ld %d\n", e[i].slot, e[i].finish, (long)e[i].n_before,
                   (long)e[i].n_after, (long)e[i].base_before, (long)e[i].base_after, e[i].keep_off, e[i].keep_count, (long)e[i].row_first, e[i].row_count,
                   e[i].row_out, e[i].n_frames, e[i].frame_first_mod, e[i].n_windows, e[i].win_first_mod, e[i].win_kept, e[i].item0, e[i].head_write,
                   e[i].tail_count, (long)e[i].tail_j0, (long)rows[2 * i], ro[i] == e[i].row_out && rows[2 * i + 1] == e[i].row_count);
        for (int i = 0; i < h->n_tiles; ++i)
            printf("L %d %d %ld %ld %ld %ld %ld\n", t[i].entry, t[i].count, (long)t[i].J0, (long)t[i].j_last, (long)t[i].jA_end, (long)t[i].jB0,
                   (long)((t[i].out - e[t[i].entry].feat) / (sizeof(float) * g.F)));
        for (int i = 0; i < h->n_items; ++i) printf("I %d %d %d\n", i, it[i].entry, it[i].centre);
        const PlanResult c = check_table(g, table.data(), slots.data());
        if (c.err) printf("X %d %s\n", c.err, c.msg);
        commit(table.data(), slots.data());
    }
    return 0;
}
