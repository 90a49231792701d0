// Prints the launch schedule (voice_activity_detection_amd/csrc/savad_schedule.h) of a fixed list of cases, one line each with every
// field of the plan: tests/test_schedule_host.py compares the output with tests/golden/schedule_table.txt, which was recorded from
// the decision logic as it stood before it moved into that header.  Host C++ only.
#include "savad_schedule.h"

#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>

using namespace savad::sched;

static Knobs knobs(int precision, int row_mode, int F = 80, int L = 2, int n_cu = 256) {
    Knobs k;
    k.precision = precision;
    k.row_mode = row_mode;
    k.n_cu = n_cu;
    k.num_layers = L;
    k.feature_size = F;
    k.FP = (F + 15) / 16 * 16;
    return k;
}

static Knobs generic(int d_model, int F = 80, int L = 2, int splits = 0) {
    Knobs k = knobs(0, 0, F, L);
    k.generic = true;
    k.d_model = d_model;
    k.FP = F;
    k.splits = splits;
    return k;
}

static void print_knobs(const char* tag, const Knobs& k) {
    printf("%s p%d m%d s%d i%d c%d L%d f%d/%d g%d d%d", tag, k.precision, k.row_mode, k.splits, (int)k.batch_invariant, k.n_cu, k.num_layers,
           k.feature_size, k.FP, (int)k.generic, k.d_model);
}

// a field at zero is left out of the line
static void field(const char* name, long long v) {
    if (v) printf(" %s%lld", name, v);
}

static void fwd(const Knobs& k, int B, int T, bool x_is_bf16 = false, long xbs_in = 0) {
    const ForwardPlan p = plan_forward(k, B, T, x_is_bf16, xbs_in);
    print_knobs("F", k);
    printf(" B%d T%d x%d xs%ld : fam%d form%d", B, T, (int)x_is_bf16, xbs_in, p.family, p.form);
    if (p.err || p.msg) printf(" err%d '%s'", p.err, p.msg ? p.msg : "");
    const struct { const char* name; long long v; } f[] = {
        {"pad", p.pad}, {"msplit", p.msplit}, {"fused", p.fused}, {"S", p.S}, {"wide", p.wide}, {"inp", p.input_p}, {"ksc", p.KSC}, {"attn", p.attn},
        {"var", p.variant}, {"fv", p.fold_v}, {"rows", (long long)p.rows}, {"rpad", (long long)p.rows_pad}, {"nblk", p.nblk}, {"npad", p.nblk_pad},
        {"NG", p.NG}, {"cb", p.cb}, {"tq", p.tq}, {"h", (long long)p.h}, {"n", (long long)p.n}, {"q", (long long)p.q}, {"k", (long long)p.k},
        {"v", (long long)p.v}, {"q2:", (long long)p.q2}, {"k2:", (long long)p.k2}, {"v2:", (long long)p.v2}, {"op", (long long)p.opart},
        {"ml", (long long)p.ml}, {"ctx", (long long)p.ctx}, {"ff", (long long)p.ff}, {"sc", (long long)p.scores}, {"xp", (long long)p.xpad},
        {"total", (long long)p.total}};
    for (const auto& e : f) field(e.name, e.v);
    printf("\n");
}

static void pred(const Knobs& k, int N, int half, int jump, int chunk) {
    const PredictPlan p = plan_predict(k, N, half, jump, chunk);
    print_knobs("P", k);
    printf(" N%d h%d j%d c%d :", N, half, jump, chunk);
    if (p.err || p.msg) printf(" err%d '%s'", p.err, p.msg ? p.msg : "");
    const struct { const char* name; long long v; } f[] = {
        {"W", p.W}, {"items", p.n_items}, {"chunk", p.chunk}, {"win", p.windowed}, {"f32s", p.f32s}, {"fam", p.family}, {"var", p.variant},
        {"last", p.variant_last}, {"logp", (long long)p.logp}, {"windows", (long long)p.windows}, {"fwd", (long long)p.fwd},
        {"fwdbytes", (long long)p.fwd_bytes}, {"total", (long long)p.total}};
    for (const auto& e : f) field(e.name, e.v);
    printf("\n");
}

template <int N>
static void shapes(const Knobs& k, const int (&bt)[N][2]) {
    for (int i = 0; i < N; ++i) fwd(k, bt[i][0], bt[i][1]);
}

static Knobs with(Knobs k, int splits, bool batch_invariant = false) {
    k.splits = splits;
    k.batch_invariant = batch_invariant;
    return k;
}

int main(int argc, char** argv) {
    // `schedule_dump windows HALF_MAX JUMP_MAX`: one line "half jump W" per geometry (tests/test_window_geometry_host.py); without
    // arguments the recorded table below
    if (argc == 4 && argv[1][0] == 'w') {
        for (int half = 0; half <= atoi(argv[2]); ++half)
            for (int jump = 1; jump <= atoi(argv[3]); ++jump) printf("%d %d %ld\n", half, jump, window_count(half, jump));
        return 0;
    }
    // ---- general: every sequence length under the automatic schedule, every row_mode at a short and a long one, a large batch
    for (int precision = 0; precision < 3; ++precision) {
        for (int T : {1, 7, 20, 32, 33, 50, 96, 800, 3200}) fwd(knobs(precision, 0), 5, T);
        for (int mode = 1; mode <= 8; ++mode)
            for (int T : {7, 96}) fwd(knobs(precision, mode), 5, T);
        for (int T : {7, 96, 800}) fwd(knobs(precision, 0), 600, T);
    }
    fwd(knobs(0, 0), 0, 7);
    fwd(knobs(1, 0), 3, 0);

    // ---- fp32
    {
        const int single[][2] = {{4096, 7}, {4097, 7},                        // tiles_packed 1024 / 1025
                                 {2340, 7}, {2341, 7},                        // tiles_dense 512 / 513
                                 {256, 20}, {257, 20}, {400, 20}, {410, 20}};  // the 92 / 45 + 110 round model
        const int msplit[][2] = {{20, 800}, {21, 800}, {327, 50}, {328, 50}, {81, 200}, {82, 200},   // rows_pad / 32 at 512 / 516
                                 {512, 50}, {128, 200}, {64, 400}, {32, 800}};   // ragged and full query-block groups in the M-split regime
        const int splits[][2] = {{1, 800}, {2, 800}, {4, 800}, {8, 800}, {1, 3200}, {3, 96}};
        shapes(knobs(0, 0), single);
        shapes(knobs(0, 4), single);
        shapes(knobs(0, 0), msplit);
        shapes(knobs(0, 3), msplit);
        shapes(knobs(0, 2), {{20, 800}, {512, 50}});
        shapes(knobs(0, 0), splits);
        shapes(knobs(0, 1), splits);
        for (int forced : {2, 64})
            for (int mode : {0, 1, 3}) shapes(with(knobs(0, mode), forced), {{2, 20}, {2, 96}, {64, 800}});
        for (int L : {8, 9})
            for (int mode : {0, 4}) fwd(knobs(0, mode, 80, L), 1000, 7);
        for (int F : {16, 40, 240, 256})
            for (int mode : {0, 1}) fwd(knobs(0, mode, F), 3, mode ? 96 : 20);
        for (int mode : {0, 3}) fwd(knobs(0, mode, 80, 2, 128), 32, 800);
    }

    // ---- bf16
    {
        const int fuse[][2] = {{256, 50}, {257, 50}, {1024, 50}, {1025, 50},       // ragged groups at 256 / 257, 1024 / 1025
                               {256, 128}, {257, 128}, {1024, 128}, {1025, 128},   // full groups
                               {36, 800}, {37, 800}, {146, 800}, {147, 800}};
        const int pw[][2] = {{96, 800}, {128, 800}, {160, 800}, {192, 800}, {224, 800}, {256, 800}, {320, 800}, {512, 800},   // the pw_pays sweep
                             {256, 1000}, {128, 1600}, {64, 3200}, {512, 400}, {1100, 256}, {2048, 256}, {2000, 200}};
        const int input[][2] = {{9, 800}, {10, 800}, {5, 800}, {6, 800}};           // nblk_pad below and at n_cu (256, 128)
        const int single[][2] = {{1024, 7}, {1025, 7}, {512, 7}, {513, 7},          // nblk at n_cu / n_cu + 1
                                 {2048, 7}, {2049, 7}, {1000, 7}, {4000, 7}};       // (nblk + 3) / 4 around n_cu / 2
        shapes(knobs(1, 0), fuse);
        shapes(knobs(1, 3), {{1025, 50}, {147, 800}});
        shapes(knobs(1, 1), {{256, 50}, {36, 800}});
        shapes(knobs(1, 0), pw);
        shapes(with(knobs(1, 0), 0, true), {{160, 800}, {512, 800}, {128, 1600}, {512, 400}, {1100, 256}, {2048, 256}});
        shapes(knobs(1, 5), {{96, 800}, {2000, 200}});
        shapes(with(knobs(1, 5), 0, true), {{96, 800}, {2000, 200}});
        for (int n_cu : {256, 128}) {
            shapes(knobs(1, 0, 80, 2, n_cu), input);
            shapes(knobs(1, 0, 80, 2, n_cu), single);
            shapes(knobs(1, 5, 80, 2, n_cu), {{9, 800}, {10, 800}, {1024, 7}});
        }
        for (int F : {80, 16, 240, 256, 40})
            for (int mode : {0, 1})
                for (bool xb : {false, true}) {
                    fwd(knobs(1, mode, F), 32, 800, xb);
                    if (F == 80 || F == 40) fwd(knobs(1, mode, F), 1000, 7, xb);
                }
        for (int L : {6, 7})
            for (int mode : {0, 8})
                for (bool xb : {false, true}) fwd(knobs(1, mode, 80, L), 1000, 7, xb);
    }

    // ---- fp32s
    {
        const int handoff[][2] = {{128, 64}, {129, 64}, {85, 96}, {86, 96}, {64, 64}, {65, 64}, {10, 800}, {11, 800}, {5, 800}, {6, 800}};   // blocks around n_cu
        const int single[][2] = {{2048, 7}, {2049, 7}, {1024, 7}, {1025, 7}, {8, 32}, {600, 32}};                                          // nblk around 2 n_cu
        for (int n_cu : {256, 128}) {
            shapes(knobs(2, 0, 80, 2, n_cu), handoff);
            shapes(knobs(2, 0, 80, 2, n_cu), single);
        }
        shapes(knobs(2, 0, 80, 2, 255), {{85, 96}, {128, 64}});   // exactly n_cu and n_cu + 1 blocks
        shapes(knobs(2, 3), {{128, 64}, {5, 800}, {8, 32}, {8, 33}, {600, 33}});
        shapes(knobs(2, 0), {{8, 33}, {600, 33}});
        shapes(knobs(2, 7), {{1024, 7}, {8, 32}});
        shapes(knobs(2, 8), {{2049, 7}, {600, 32}});
        shapes(knobs(2, 3, 80, 2, 128), {{128, 64}, {1024, 7}});
        for (int L : {3, 4})
            for (int mode : {0, 1, 8}) fwd(knobs(2, mode, 80, L), 1000, 7);
        for (int F : {16, 40})
            for (int mode : {0, 3}) shapes(knobs(2, mode, F), {{3, 20}, {2, 96}, {600, 96}});
    }

    // ---- any d_model
    for (int dm : {64, 256})
        for (int forced : {0, 2, 7})
            for (int T : {7, 800}) fwd(generic(dm, 80, 2, forced), 3, T);
    fwd(generic(64, 40, 3), 70000, 7);
    fwd(generic(64), 1, 6000);   // T * T beyond the score tile
    fwd(generic(64), 2, 96, false, 96 * 80);

    // ---- sequence stride: honoured, and each refusal
    for (int precision = 0; precision < 3; ++precision)
        for (int mode : {0, 1, 3})
            for (int F : {80, 40})
                for (int T : {20, 96})
                    if (mode < 3 || (F == 80 && T == 96)) fwd(knobs(precision, mode, F), mode ? 3 : 600, T, false, 48 * (long)F);
    fwd(knobs(1, 0), 3, 96, true, 48 * 80);
    fwd(knobs(1, 0, 80, 7), 3, 20, true, 48 * 80);

    // ---- predict
    for (int precision = 0; precision < 3; ++precision)
        for (int mode : {0, 1, 4, 8}) {
            const Knobs k = knobs(precision, mode);
            pred(k, 98, 19, 9, 16384);
            pred(k, 4097 + 38, 19, 9, 16384);
            if (mode >= 4) continue;   // (the pinned single-launch modes: the windowed sizes only)
            for (int N : {0, 38, 4096 + 38}) pred(k, N, 19, 9, 16384);
            pred(k, 98, 19, 9, 15);
            pred(k, 2000, 40, 1, 256);   // W = 81: refused
            pred(k, 100000, 19, 9, 4095);
            pred(k, 2000, 20, 1, 256);   // W = 41
            pred(k, 2000, 16, 1, 255);   // W = 33
            pred(knobs(precision, mode, 40), 1062, 19, 9, 16384);   // padded features: gathered
            pred(knobs(precision, mode, 80, 9), 1062, 19, 9, 16384);
            pred(knobs(precision, mode, 80, 2, 128), (1 << 22) + 38 + 100, 19, 9, 16384);   // two launches, the last of 100 windows
        }
    pred(generic(64), 1062, 19, 9, 16384);
    pred(generic(64, 80, 2, 2), 1062, 19, 9, 15);
    return 0;
}
