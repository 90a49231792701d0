// savad_schedule.h -- the launch schedule of a forward, decided once: which kernel family runs a shape, in which form and variant,
// how many blocks or tiles it covers and where every buffer of its workspace lies.  plan_forward / plan_predict are pure functions
// of the handle's settings (Knobs) and the shape; savad.hip sizes workspaces from their totals and launches what they name, and
// tests/schedule_dump.cpp prints them case by case (tests/golden/schedule_table.txt).  Plain C++17: no HIP, no device code.
// Every threshold of the schedule, with the measurements behind it, is in this file.
#pragma once

#include <stddef.h>

#include "../../include/savad.h"
#include "savad_dims.h"
#include "savad_windows.h"

// ---- experiment-build knobs (-D on the compile line; the product is built with the defaults)
#ifndef SAVAD_INPUT_PERSISTENT
#define SAVAD_INPUT_PERSISTENT 1   // 0: experiment builds that keep the ring form of the bf16 input stage everywhere (scripts/ubench/input_p_ab.py)
#endif
#ifndef SAVAD_NS_MAX_ROUNDS
#define SAVAD_NS_MAX_ROUNDS 1   // blocks per CU up to which one block per workgroup beats four (scripts/ubench/packed_bf16_bench.py)
#endif
#ifndef SAVAD_F32S_NS_MAX_ROUNDS
#define SAVAD_F32S_NS_MAX_ROUNDS 2   // blocks per CU up to which one block per workgroup beats a wave per block (scripts/ubench/f32s_check_t7.py)
#endif
#ifndef SAVAD_F32S_PACKED_MIN_BLOCKS
#define SAVAD_F32S_PACKED_MIN_BLOCKS 0
#endif
#ifndef SAVAD_F32S_MIN_BLOCKS_PER_CU
#define SAVAD_F32S_MIN_BLOCKS_PER_CU 1
#endif

namespace savad {
namespace sched {

// what a handle's settings contribute to the schedule (savad.hip: knobs_of)
struct Knobs {
    int precision = 0;  // 0 = fp32 MFMA, 1 = bf16 MFMA operands, 2 = "fp32s" (three bf16 pieces per operand)
    int row_mode = 0;   // savad_set_row_mode, 0 - 8 (include/savad.h)
    int splits = 0;     // savad_set_attention_splits, 0 = automatic
    bool batch_invariant = false;
    int n_cu = 256;
    int num_layers = 0, feature_size = 0;
    int FP = 0;  // feature size rounded up to the kernels' K granularity
    bool generic = false;
    int d_model = D;
};

enum Family { GENERIC, F32, BF16, F32S };  // savad_generic.h | savad_kernels.h | savad_kernels_bf16.h + savad_packed_bf16.h | savad_kernels_f32s.h
enum Form { SINGLE, FUSED, SEPARATE };     // the whole forward in one launch | attention + row chain in one launch per layer | a launch each
enum Attention { ATTN_NONE, ATTN_PACKED, ATTN_FIRST, ATTN_PW, ATTN_PW_NOSPLIT };  // the attention launch of Form SEPARATE
enum { VARIANT_WAVE_PER_BLOCK = 4, VARIANT_LATENCY = 8 };                         // ForwardPlan::variant in the fp32s family

struct ForwardPlan {
    int family = F32, form = SEPARATE;
    int err = SAVAD_OK;  // a sequence stride (xbs_in > 0) no kernel of this schedule takes: the code and message of the refusal
    const char* msg = nullptr;
    bool pad = false;  // the features are zero-padded to FP columns first (into xpad)
    // fp32
    bool msplit = false;  // row-wise stages on 128-row tiles with the weight stream shared through LDS
    bool fused = false;   // attention + row chain in one launch per layer when the per-layer launches run (q/k/v double-buffered: q2, k2, v2)
    int S = 1;            // key splits of the attention kernel
    // bf16
    bool wide = false;     // 8-wave workgroups with the 4-deep ring
    bool input_p = false;  // the persistent weights-resident input stage
    int KSC = 0;           // ... its compile-time K-step count (5, or 0 = any)
    int attn = ATTN_NONE;
    // single launch: bf16 5 / 6 / 7 / 8 (savad.hip: launch_single), fp32s VARIANT_LATENCY / VARIANT_WAVE_PER_BLOCK; 0 otherwise
    int variant = 0;
    bool fold_v = false;  // fp32s: the launches read the Q/K/V images with the out-projection folded into V
    size_t rows = 0, rows_pad = 0;      // fp32: B * T and whole 128-row tiles
    int nblk = 0, nblk_pad = 0, NG = 0;  // 32-row blocks (tiles of the fp32 single launch), whole workgroups of them, query-block groups per sequence
    int cb = 0, tq = 0;                  // generic: sequences and query rows per score tile
    size_t h = 0, n = 0, q = 0, k = 0, v = 0, q2 = 0, k2 = 0, v2 = 0, opart = 0, ml = 0, ctx = 0, ff = 0, scores = 0, xpad = 0;  // byte offsets
    size_t total = 0;  // bytes
};

struct PredictPlan {
    int err = SAVAD_OK;
    const char* msg = nullptr;
    int W = 0, n_items = 0, chunk = 0;
    bool windowed = false;  // the single-launch forward reads its windows straight out of the feature matrix
    bool f32s = false;      // ... and it is the fp32s one (precision 2 from SAVAD_F32S_PACKED_MIN_BLOCKS blocks up; shorter clips: the exact-fp32 one)
    int family = F32;       // windowed: the family whose single-launch kernel serves the windows
    int variant = 0, variant_last = 0;  // ... and its variant for a launch of `chunk` windows and for the shorter last one
    size_t logp = 0, windows = 0, fwd = 0, total = 0;  // byte offsets into the workspace
    size_t fwd_bytes = 0;                              // the ForwardPlan total of a chunk-sized forward (gathered path)
};

constexpr const char* STRIDE_REFUSED = "strided input: no kernel takes the stride for this shape";

inline long window_count(int half, int jump) { return windows::offsets(half, jump, nullptr); }  // W, as tests/schedule_dump.cpp prints it

// packed blocks of a T <= 32 batch: floor(32 / T) sequences share a 32-row block
inline long packed_blocks(int B, int T) { return ((long)B + 32 / T - 1) / (32 / T); }

inline int choose_splits(const Knobs& m, int B, int T) {
    if (T <= 32) return 1;
    const int NT = (T + 31) / 32, QB = NT;
    if (m.splits > 0) return m.splits < NT ? m.splits : NT;
    // Work quantisation model (MFMA-bound): a workgroup puts one wave on each SIMD of a CU, so a
    // CU that receives n workgroups needs n * ceil(NT/S) tile-times whether or not they are
    // co-resident; prologue + epilogue + partial write/re-read cost about 1.5 tile-times per
    // workgroup.  Measured at B=32, T=800: S=1 120 us, S=2 119 us (+4 us in the row kernel), S=5
    // 121 us (+25 us): splitting only pays when it fills idle CUs (small batches).
    auto cost = [&](int S) {
        const long wgs = (long)B * ((QB + 3) / 4) * S;
        return (double)((wgs + 255) / 256) * ((NT + S - 1) / S + 1.5);
    };
    const double cost1 = cost(1);
    double best = cost1;
    int bestS = 1;
    for (int S = 2; S <= 8 && S <= NT; ++S) {
        const double cs = cost(S);
        if (cs < 0.93 * cost1 && cs < best) {
            best = cs;
            bestS = S;
        }
    }
    return bestS;
}

// T <= 32 with bf16 operands: the whole forward in one launch (savad_packed_bf16.h); a wave per packed block, NW blocks per
// workgroup.
inline bool single_bf16_applies(const Knobs& m, int T) {
    // row_mode 0 (automatic) and 4: picked by the number of blocks; 5 - 7: a fixed variant (launch_single; tuning
    // knobs at T <= 32, where the persistent attention kernel that 5 selects for long sequences does not exist); 1 - 3 keep
    // the per-layer launches (the cross-check of the tests)
    return T <= 32 && m.num_layers <= bf::PACKED_BF16_MAX_LAYERS && (m.row_mode == 0 || m.row_mode >= 4);
}
inline int single_bf16_variant(const Knobs& m, long nblk) {
    // variant: row_mode 5 = 8-wave workgroups, 6 = 4 waves + 4 that move the weight stream through a 4-slot ring, 7 = 4 waves +
    // 2 slots; automatic: 6 while the 4-block workgroups fill at most half of the CUs ([1000,7,80], 63 workgroups: 0.044 against 0.049 ms;
    // [4000,7,80], 250 workgroups: 0.059 against 0.053; scripts/ubench/packed_bf16_bench.py)
    // 8 = the latency variant: ONE block per workgroup, its four waves split the output features (savad_packed_bf16.h)
    return m.row_mode >= 5 ? m.row_mode : (nblk <= SAVAD_NS_MAX_ROUNDS * m.n_cu ? 8 : ((nblk + 3) / 4 <= m.n_cu / 2 ? 6 : 7));
}

// T <= 32 in precision 2: ONE launch for the whole forward -- the latency variant (one packed block per workgroup, its four waves
// splitting every GEMM's output features; round 6) while the blocks fill the CUs at most SAVAD_F32S_NS_MAX_ROUNDS times, the
// wave-per-block kernel (four blocks per workgroup share the weight stream through the LDS ring; a block's chain is 7 320 bf16 MFMAs)
// beyond.  (Until the latency variant existed, short clips ran the exact-fp32 kernels of precision 0: SAVAD_F32S_PACKED_MIN_BLOCKS.)
inline bool single_f32s_applies(const Knobs& m, int B, int T) {
    // row_mode 0 (automatic) and 4: the single launch in the variant the number of blocks suggests (launch_single);
    // 5 - 7: the wave-per-block variant, 8: the latency variant (one block per workgroup); 1 - 3 keep the per-layer launches
    // (the cross-check of the tests).  SAVAD_F32S_PACKED_MIN_BLOCKS > 0 (experiment builds): exact-fp32 kernels below that many blocks
    if (T > 32 || m.num_layers > fs::PACKED_F32S_MAX_LAYERS) return false;
    const long nblk = packed_blocks(B, T);
    return m.row_mode >= 4 || (m.row_mode == 0 && nblk >= SAVAD_F32S_PACKED_MIN_BLOCKS);
}
inline int single_f32s_variant(const Knobs& m, long nblk) {
    // the latency variant (one block per workgroup, its four waves splitting the output features) up to SAVAD_F32S_NS_MAX_ROUNDS blocks
    // per CU; beyond, a wave per block with the weight stream shared through the LDS ring
    const bool ns = m.row_mode >= 5 ? m.row_mode == 8 : nblk <= SAVAD_F32S_NS_MAX_ROUNDS * m.n_cu;
    return ns ? VARIANT_LATENCY : VARIANT_WAVE_PER_BLOCK;
}
// precision 2 shapes that run the exact-fp32 kernels under the automatic schedule ("fp32s" promises the fp32 result at the best speed
// the library has, not a particular instruction): sequences longer than 32 frames in batches of at most SAVAD_F32S_MIN_BLOCKS_PER_CU
// 32-row blocks per CU.  There a forward's time is the latency of ONE block's chain, and the exact-fp32 kernels split a block's
// GEMMs over the four waves of a workgroup where the fp32s fused launch gives a block to one wave: same-box sweep
// (scripts/ubench/f32s_vs_f32_sweep.py, us, exact fp32 / fp32s): [1,800] 208 / 295, [8,800] 253 / 300, [12,800] 371 / 301,
// [2,3200] 403 / 668, [4,3200] 747 / 673, [64,100] 187 / 203, [24,400] 340 / 246 -- the crossing sits at one block per CU for every T.
// Any non-zero row_mode keeps the fp32s kernels (3: its fused launches at every size -- the tests' way to reach them, and the way
// to results that do not depend on the batch a sequence arrives in: the two kernel families agree to fp32 rounding, not bit for bit).
inline bool f32s_uses_exact_fp32(const Knobs& m, int B, int T) {
    if (m.row_mode != 0) return false;
    if (T <= 32) return !single_f32s_applies(m, B, T);
    return (long)B * ((T + 31) / 32) <= (long)SAVAD_F32S_MIN_BLOCKS_PER_CU * m.n_cu;
}

// The persistent attention kernel (one 4 x 64-row workgroup per CU walking (sequence, 8 query blocks) items) against the
// first-generation one: a cost model of both, from the sweep scripts/ubench/pw_sweep.py (round 4, us per launch, first-generation /
// persistent): [96,800] 43.4 / 50.1, [128,800] 52.6 / 52.0, [160,800] 67.3 / 58.3, [192,800] 77.9 / 74.1, [224,800] 90.8 / 78.1,
// [256,800] 97.7 / 82.4, [512,800] 193.3 / 163.7, [256,1000] 143.7 / 117.7, [128,1600] 176.1 / 144.3, [64,3200] 333.9 / 284.5,
// [512,400] 65.3 / 63.8.  Persistent: the busiest workgroup's items (the cursor of scripts/gen_attn_pw.py restated: full groups
// with a stride of 32 per XCD, a sequence's tail group attached to one of them; a key-split tail costs 0.55 of a full item) times
// 0.62 us per key block + 7 us per item, + 5 us per launch.  First generation: 0.54 ns per (query block x key block) + 2.5 ns per
// query block, per sequence.  The persistent kernel is picked unless the model has it more than 5 % behind.
inline bool pw_pays(bool ks_tail /* key-split tail items (0.55 of a full item) or ordinary ones (a full item's time) */, int Bq, int Tq) {
    const int QBq = (Tq + 31) / 32, NGFq = QBq >> 3, TQq = QBq & 7;
    if (NGFq == 0) return false;
    const int wg = bf::PW_GRID / 8;
    auto ff1 = [](int x) { return __builtin_ctz((unsigned)x); };
    const int t0 = ff1(NGFq) < ff1(wg) ? ff1(NGFq) : ff1(wg), sh = ff1(wg) - t0, mask = (1 << t0) - 1;
    const int S = (Bq + 7) / 8;  // sequences of the fullest XCD
    const double ctail = TQq == 0 ? 0.0 : (TQq <= 2 && ks_tail ? 0.55 : 1.0);
    double busiest = 0.0;
    for (int j = 0; j < wg; ++j) {
        double n = 0.0;
        for (long i = j; i / NGFq < S; i += wg) {
            const int bi = (int)(i / NGFq), g = (int)(i % NGFq);
            n += 1.0 + ((TQq && g == ((bi >> sh) & mask)) ? ctail : 0.0);
        }
        busiest = n > busiest ? n : busiest;
    }
    const double t_pw = busiest * (0.62 * QBq + 7.0) + 5.0;
    const double t_first = (double)Bq * (5.4e-4 * QBq * QBq + 2.5e-3 * QBq);
    return t_pw < 1.05 * t_first;   // (the busiest-workgroup figure errs on the high side when the last round is thin: [320,800] 106.6 measured, 119.7 priced)
}

namespace detail {

struct Bump {  // the workspace as consecutive buffers
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += bytes;
        return o;
    }
};

inline void refuse(ForwardPlan& p, const char* msg) {
    p.err = SAVAD_E_UNSUPPORTED;
    p.msg = msg;
}

// 32-row blocks of the fragment-major families: ceil(T / 32) per sequence, or floor(32 / T) sequences packed into one
inline int blocks(int B, int T) { return T > 32 ? B * ((T + 31) / 32) : (B + (32 / T) - 1) / (32 / T); }

// fp32 (savad_kernels.h): float buffers h | q | k | v | [q2 | k2 | v2] | opart | ml | [xpad]
inline void plan_f32(ForwardPlan& w, const Knobs& m, int B, int T, long xbs_in) {
    const size_t f = sizeof(float);
    if (xbs_in > 0 && (w.pad || T <= 32)) refuse(w, STRIDE_REFUSED);
    w.rows = (size_t)B * T;
    w.rows_pad = (w.rows + 127) / 128 * 128;  // whole 128-row tiles (M-split kernels); also a multiple of TILE
    w.S = choose_splits(m, B, T);
    // Row-wise stages: 128-row tiles with the weight stream shared through LDS (M split) when that
    // fills the chip; 32-row tiles with the output features split over the 4 waves (N split) when
    // the batch is small and the critical path per workgroup matters more than weight traffic.
    // N-split works through ceil(tiles / 256) rounds of ~45 us, M-split through one round of ~118 us per 256 workgroups
    // of 128 rows: M wins from the third N-split round on (more than 512 tiles of 32 rows).  Measured at T=800: B=20
    // (500 tiles) N 0.504 / M 0.648 ms; B=24 (600 tiles) N 0.611 / M 0.589 ms.
    const int row_mode = m.row_mode == 4 ? 0 : m.row_mode;  // 4 only differs from automatic for T <= 32 (savad_forward)
    w.msplit = row_mode == 2 || row_mode == 3 || (row_mode == 0 && w.rows_pad / 32 > 512);
    // In the M-split regime without key splits the attention stage and the row chain of a query-block group
    // run back to back in one workgroup (attention_row_kernel).  row_mode 2 keeps them as separate launches.
    // Automatic: only when a query-block group keeps at least 80 % of its 4 wave slots busy -- waves without a
    // query block sit out the whole row chain (measured: T=50, two blocks per group, B=512: 0.63 ms fused against
    // 0.42 ms separate; T=200 (7 blocks in 2 groups) 0.434 / 0.453; T=400 (13 in 4) 0.508 / 0.524; T=800 (25 in
    // 7) 0.640 / 0.668).
    const int QBp = (T + 31) / 32, NGp = (QBp + 3) / 4;
    const bool ragged = QBp * 5 < NGp * 4 * 4;  // QB / (4 NG) < 0.8
    w.fused = w.msplit && T > 32 && w.S == 1 && (row_mode == 3 || (row_mode != 2 && !ragged));
    w.NG = NGp;
    // T <= 32 in the small-batch regime (the reference pipeline's 7-frame windows): the whole forward is ONE launch,
    // a workgroup per packed tile of floor(32/T) sequences keeps every activation on its CU (packed_forward_kernel).
    // Automatic up to 1024 tiles (four rounds of the 256 CUs); beyond that the 128-row M-split tiles, which fetch the
    // weight stream once per 128 rows instead of once per tile, are ahead.  Measured at T=7, ms per forward, single
    // launch / per-layer N-split launches / M-split: 250 tiles 0.100 / 0.156 / 0.356; 512 tiles 0.186 / 0.272 / 0.364;
    // 1024 tiles 0.366 / 0.506 / 0.383; 2048 tiles 0.728 / 0.878 / 0.699; 4096 tiles (the predictor's 16384-window
    // batches) 1.454 / 1.736 / 1.346.  row_mode 4 forces the single launch for any T <= 32 batch.
    // A packed tile holds floor(32/T)*T of 32 rows (28 at T=7, 20 at T=20, 17 at T=17): while the DENSE 32-row tiles of the
    // per-layer N-split launches still fit fewer rounds of the CUs, those win (T=20, B=400: 400 packed / 250 dense tiles,
    // 0.184 against 0.160 ms).  Round model fitted to scripts/ubench/policy_sweep.py: 92 us per round of packed tiles, 45 +
    // 110 us per round of dense tiles.
    const long tiles_packed = T <= 32 ? packed_blocks(B, T) : 0, tiles_dense = ((long)B * T + 31) / 32;
    const bool one_launch = tiles_packed <= 1024 &&
                            (tiles_dense > 512 || 92 * ((tiles_packed + 255) / 256) <= 45 + 110 * ((tiles_dense + 255) / 256));
    w.nblk = (int)tiles_packed;
    if (T <= 32 && m.num_layers <= PACKED_MAX_LAYERS && (m.row_mode == 4 || (m.row_mode == 0 && one_launch)))
        w.form = SINGLE;
    else if (w.fused)
        w.form = FUSED;
    else
        w.attn = T <= 32 ? ATTN_PACKED : ATTN_FIRST;
    Bump b;
    w.h = b.take(w.rows_pad * D * f);
    w.q = b.take((w.rows_pad + TILE) * D * f);  // +32 rows of slack: key/value tiles may over-read the last block
    w.k = b.take((w.rows_pad + TILE) * D * f);
    w.v = b.take((w.rows_pad + TILE) * D * f);
    w.q2 = w.k2 = w.v2 = b.off;
    if (w.fused) {
        w.q2 = b.take((w.rows_pad + TILE) * D * f);
        w.k2 = b.take((w.rows_pad + TILE) * D * f);
        w.v2 = b.take((w.rows_pad + TILE) * D * f);
    }
    w.opart = b.take((size_t)w.S * w.rows_pad * D * f);
    w.ml = b.take((size_t)w.S * w.rows_pad * 2 * f);
    w.xpad = b.off;
    if (w.pad) b.take(w.rows * (size_t)m.FP * f);  // zero-padded features
    w.total = b.off;
}

// block space of the bf16 path (savad_kernels_bf16.h): h | q | k | v^T | ctx | [q2 | k2 | v^T2] | [xpad]
inline void plan_bf16(ForwardPlan& p, const Knobs& m, int B, int T, bool x_is_bf16, long xbs_in) {
    const bool single = single_bf16_applies(m, T);
    if (xbs_in > 0 && (p.pad || single)) refuse(p, STRIDE_REFUSED);
    p.nblk = blocks(B, T);
    p.nblk_pad = (p.nblk + 7) / 8 * 8;  // whole workgroups for both the 4- and the 8-wave kernels
    // 4-wave workgroups (two per CU, 2-slot ring) by default.  row_mode 2 selects the 8-wave variant with a
    // 4-deep ring (half the DMA stream per data row, one workgroup per CU): measured SLOWER on MI355X at
    // every size tried (B=256, T=800: 0.86 vs 0.75 ms), kept as a tuning knob and covered by the tests.
    // row_mode 0 / 3 fuse attention and row chain per layer when T > 32; 1 / 2 keep them apart.
    p.wide = m.row_mode == 2;
    // row_mode 1 / 2 keep attention and row chain as separate launches (4- / 8-wave workgroups), 3 fuses them.
    // Automatic: fused up to ~4 workgroups per CU.  Measured on MI355X at T=800 (fused vs separate, ms per
    // forward): B=32 0.128 / 0.142, B=64 0.197 / 0.204, B=128 0.355 / 0.370, B=192 0.509 / 0.501, B=256 0.642 /
    // 0.641 -- with more work per CU the wave slots a ragged query-block group leaves idle (3 of 28 at T=800) cost
    // the row chain as much as the context round trip and the extra launches cost the separate form.
    const int QBp = (T + 31) / 32, NG4 = (QBp + 3) / 4, NW = p.wide ? 8 : 4;
    const long groups = T > 32 ? (long)B * NG4 : 0;
    const bool ragged = QBp * 5 < NG4 * 4 * 4;  // fewer than 80 % of a group's wave slots hold a query block
    // (below one workgroup per CU the forward is launch / latency bound and fusing wins even with idle slots:
    // B=64, T=50: 0.070 / 0.074 ms; B=32, T=160: 0.072 / 0.080 ms)
    const bool automatic = m.row_mode == 0 || m.row_mode == 4;
    const bool fused = T > 32 && (m.row_mode == 3 || (automatic && groups <= 1024 && (!ragged || groups <= 256)));
    p.NG = (QBp + NW - 1) / NW;  // query-block groups of the launches' own workgroup width (NW waves, a query block each)
    if (single && !(x_is_bf16 && !p.pad)) {  // (the single launch reads fp32 features; the padded copy is fp32)
        p.form = SINGLE;
        p.variant = single_bf16_variant(m, p.nblk);
    } else {
        p.form = fused ? FUSED : SEPARATE;
        // Persistent weights-resident form of the stage (input_qkv_kernel_bf16_p) in the automatic schedules and in 5, from one block per
        // CU up (scripts/ubench/input_p_ab.py, us per launch ring / persistent, fp32 features at T = 800: B=16 19.4 / 17.1, 32 20.5 / 19.1,
        // 64 22.4 / 22.7, 128 39.9 / 33.2, 256 79.6 / 64.9, 512 151.4 / 114.6; the same bits); row_mode 1 - 3 keep the ring kernel.
        const int KSx = m.FP / 16;
        p.input_p = SAVAD_INPUT_PERSISTENT && (automatic || m.row_mode == 5) && KSx >= 1 && KSx <= 15 && p.nblk_pad >= m.n_cu;
        p.KSC = p.input_p && KSx == 5 ? 5 : 0;
        if (!fused) {
            if (T <= 32)
                p.attn = ATTN_PACKED;
            else if (m.row_mode == 5 || (automatic && pw_pays(!m.batch_invariant, B, T)))  // persistent 4 x 64-row attention (savad_attn_pw_bf16.h)
                p.attn = m.batch_invariant ? ATTN_PW_NOSPLIT : ATTN_PW;
            else
                p.attn = ATTN_FIRST;
        }
    }
    Bump b;
    p.h = b.take((size_t)p.nblk_pad * bf::HBLK_FLOATS * bf::HRES_BYTES);
    const size_t fb = (size_t)(p.nblk_pad + 1) * bf::BLK_BYTES;  // +1 block: a 2-block key stage may over-read
    p.q = b.take(fb);
    p.k = b.take(fb);
    p.v = b.take(fb);
    p.ctx = b.take(fb);
    p.q2 = p.k2 = p.v2 = b.off;
    if (fused) {
        p.q2 = b.take(fb);
        p.k2 = b.take(fb);
        p.v2 = b.take(fb);
    }
    p.xpad = b.off;
    if (p.pad) b.take((size_t)B * T * m.FP * sizeof(float));
    p.total = b.off;
}

// block space of the fp32s path (savad_kernels_f32s.h): fp32 residual blocks, Q / K / V^T as triples, double-buffered between
// layers (the fused launch of layer l writes layer l + 1's Q / K / V^T while other workgroups still read layer l's)
inline void plan_f32s(ForwardPlan& p, const Knobs& m, int B, int T, long xbs_in) {
    if (xbs_in > 0 && (p.pad || T <= 32)) refuse(p, STRIDE_REFUSED);
    p.nblk = blocks(B, T);
    p.nblk_pad = (p.nblk + 3) / 4 * 4;
    p.NG = ((T + 31) / 32 + 3) / 4;
    if (single_f32s_applies(m, B, T)) {
        p.form = SINGLE;
        p.variant = single_f32s_variant(m, p.nblk);
    } else {
        p.form = FUSED;
        // T > 32: V is projected with Wo Wv' (prepare_frags), so that P V already is the out-projected context -- the fused launch's row
        // chain has no out-projection.  The T <= 32 form of the launch keeps the plain images and its out-projection.
        p.fold_v = T > 32;
    }
    Bump b;
    p.h = b.take((size_t)p.nblk_pad * fs::HBLK_BYTES);
    const size_t fb = (size_t)p.nblk_pad * fs::BLK3_BYTES;
    size_t* slots[6] = {&p.q, &p.k, &p.v, &p.q2, &p.k2, &p.v2};
    for (size_t* s : slots) *s = b.take(fb);
    p.xpad = b.off;
    if (p.pad) b.take((size_t)B * T * m.FP * sizeof(float));
    p.total = b.off;
}

// any d_model (savad_generic.h): h | n | q | k | v | ctx (rows x d_model each), ff (rows x 4 d_model), one score tile
inline void plan_generic(ForwardPlan& p, const Knobs& m, int B, int T, long xbs_in) {
    if (xbs_in > 0) refuse(p, "strided input needs the d_model=128 kernels");
    const int force_query_tiles = m.splits;
    const size_t md = (size_t)B * T * m.d_model;
    Bump b;
    auto take = [&](size_t n) { return b.take(((n + 63) & ~size_t(63)) * sizeof(float)); };
    p.h = take(md);
    p.n = take(md);
    p.q = take(md);
    p.k = take(md);
    p.v = take(md);
    p.ctx = take(md);
    p.ff = take(4 * md);
    const size_t tt = (size_t)T * T;
    if (force_query_tiles > 1 || tt > gen::SCORE_CAP) {
        p.cb = 1;
        long tq = force_query_tiles > 1 ? (T + force_query_tiles - 1) / force_query_tiles : (long)(gen::SCORE_CAP / T);
        p.tq = (int)(tq < 1 ? 1 : (tq > T ? T : tq));
    } else {
        size_t cb = gen::SCORE_CAP / tt;
        cb = cb > 65535 ? 65535 : cb;  // cb is a grid.z of the score GEMMs (HIP: at most 65535); the b0 loop takes the rest
        p.cb = (int)(cb > (size_t)B ? (size_t)B : cb);
        p.tq = T;
    }
    p.scores = take((size_t)p.cb * p.tq * T);
    p.total = b.off;
}

}  // namespace detail

// The schedule of one forward of B sequences of T frames.  x_is_bf16: bf16 features (bf16 precision only); xbs_in: elements between
// consecutive sequences of x (savad_forward_strided), 0 = T * F -- it travels as an ARGUMENT to the one kernel per family that reads
// the features, and every schedule that cannot honour it carries the refusal (err, msg).  B == 0 or T == 0: nothing to run, total 0.
inline ForwardPlan plan_forward(const Knobs& m, int B, int T, bool x_is_bf16, long xbs_in) {
    ForwardPlan p;
    p.family = m.generic ? GENERIC : m.precision == 1 ? BF16 : F32;
    if (B <= 0 || T <= 0) return p;
    if (m.precision == 2 && !m.generic && !f32s_uses_exact_fp32(m, B, T)) p.family = F32S;
    p.pad = !m.generic && m.FP != m.feature_size;
    switch (p.family) {
        case GENERIC: detail::plan_generic(p, m, B, T, xbs_in); break;
        case BF16: detail::plan_bf16(p, m, B, T, x_is_bf16, xbs_in); break;
        case F32S: detail::plan_f32s(p, m, B, T, xbs_in); break;
        default: detail::plan_f32(p, m, B, T, xbs_in); break;
    }
    return p;
}

// The schedule of savad_predict_probabilities over N feature frames (vad/predictor.py:159-262): windows of W frames around each of
// n_items positions, `chunk` of them per forward.
inline PredictPlan plan_predict(const Knobs& m, int N, int half, int jump, int chunk) {
    PredictPlan pp;
    PredictPlan* p = &pp;
    const long Wl = windows::offsets(half, jump, nullptr);
    p->W = (int)(Wl < 65 ? Wl : 65);
    if (Wl > windows::MAX_FRAMES) {
        p->err = SAVAD_E_UNSUPPORTED;
        p->msg = windows::TOO_LONG;
        return pp;
    }
    p->n_items = (int)windows::items(N, half);
    const int F = m.feature_size;
    // windowed: the whole clip in ONE single-launch forward (up to 1024 packed tiles = 4096 windows of 7 frames, ~41 s of
    // audio: savad_forward's own limit for that kernel); longer inputs go through `chunk`-sized M-split forwards, which
    // are ~9 % faster per window than 4096-window launches (5.27 vs 5.36 ms for 10 min of audio)
    // (bf16 operands: the single launch amortises the weight stream over the workgroup's blocks, so it takes any number of windows)
    p->f32s = m.precision == 2 && !m.generic && p->W <= 32 && m.FP == F && p->n_items > 0 && single_f32s_applies(m, p->n_items, p->W);
    if (m.precision == 1)
        p->windowed = !m.generic && p->W <= 32 && m.FP == F && single_bf16_applies(m, p->W);
    else if (p->f32s)   // (the fp32s single launch takes any number of windows)
        p->windowed = true;
    else
        p->windowed = !m.generic && p->W <= 32 && m.num_layers <= PACKED_MAX_LAYERS && m.FP == F &&
                      (m.row_mode == 4 || (m.row_mode == 0 && p->n_items <= 1024 * (32 / p->W)));
    p->family = m.generic ? GENERIC : m.precision == 1 ? BF16 : p->f32s ? F32S : F32;
    p->chunk = p->windowed ? windows::at_most_items(m.precision == 1 || p->f32s ? (1 << 22) : 1024 * (32 / p->W), p->n_items)
                           : windows::even_chunk(chunk, p->n_items);
    if (p->windowed && p->n_items > 0 && p->family != F32) {
        auto variant = [&](int count) {
            const long nblk = packed_blocks(count, p->W);
            return p->family == BF16 ? single_bf16_variant(m, nblk) : single_f32s_variant(m, nblk);
        };
        const int last = p->n_items % p->chunk;
        p->variant = variant(p->chunk);
        p->variant_last = last ? variant(last) : p->variant;
    }
    p->fwd_bytes = p->windowed ? 0 : plan_forward(m, p->chunk, p->W, false, 0).total;
    const windows::Layout l = windows::layout(0, p->n_items > 0 ? p->n_items : 1, p->windowed ? 0 : p->chunk, p->W, F, p->fwd_bytes);
    p->logp = l.logp, p->windows = l.windows, p->fwd = l.fwd, p->total = l.total;
    return pp;
}

// The schedule of savad_predict_probabilities_batch: C clips in one concatenated feature matrix, clip c = rows [clip_first[c],
// clip_first[c + 1]) with n_c = max(0, rows - 2 half) windows of its own (savad_batch_kernels.h).
struct PredictBatchPlan {
    int err = SAVAD_OK;
    const char* msg = nullptr;
    int W = 0, C = 0, rows = 0, n_items = 0, chunk = 0;  // rows = the matrix's, n_items = the sum of n_c: global items [0, n_items), `chunk` per forward
    size_t items_first = 0, logp = 0, windows = 0, fwd = 0, total = 0;  // byte offsets into the workspace
    size_t fwd_bytes = 0;                                               // the ForwardPlan total of a chunk-sized forward
};

constexpr long BATCH_INDEX_LIMIT = 2147483647L;  // rows of the matrix (an int32 table holds no more) and n_items * W: 32-bit indices

// what the HOST copy of a clip table says: validated (C >= 1, clip_first[0] = 0, non-decreasing, the window geometry, the index
// limits) and counted
struct ClipTotals {
    int err = SAVAD_OK;
    const char* msg = nullptr;
    int W = 0, rows = 0, n_items = 0;
};
inline ClipTotals clip_totals(const int32_t* clip_first, int C, int half, int jump) {
    ClipTotals t;
    auto refuse = [&](int err, const char* msg) {
        t.err = err;
        t.msg = msg;
        return t;
    };
    if (!clip_first || C < 1) return refuse(SAVAD_E_INVALID, "clip table: at least one clip");
    if (half < 0 || jump <= 0) return refuse(SAVAD_E_INVALID, "half must not be negative, jump must be positive");
    const long Wl = windows::offsets(half, jump, nullptr);
    if (Wl > windows::MAX_FRAMES) return refuse(SAVAD_E_UNSUPPORTED, windows::TOO_LONG);
    t.W = (int)Wl;
    if (clip_first[0] != 0) return refuse(SAVAD_E_INVALID, "clip table: clip_first[0] must be 0");
    long items = 0;
    for (int c = 0; c < C; ++c) {
        const long n = (long)clip_first[c + 1] - clip_first[c];
        if (n < 0) return refuse(SAVAD_E_INVALID, "clip table: clip_first must not decrease");
        items += windows::items(n, half);
    }
    t.rows = clip_first[C];  // (an int32 table cannot name more than BATCH_INDEX_LIMIT rows)
    if (items * t.W > BATCH_INDEX_LIMIT) return refuse(SAVAD_E_UNSUPPORTED, "windows x frames of all clips exceed the 32-bit index range");
    t.n_items = (int)items;
    return t;
}

// The plan of the one call from the HOST copy of the table: validates it, counts the items and lays the
// workspace out: items_first [C + 1] int32 | logp [n_items, W, 2] | windows [chunk, W, F] | the chunk-sized forward's workspace.  The
// windows are always copied and every chunk is a savad_forward of its own, in every precision and row mode (the packed kernels
// read windows in place at ONE row pitch; a chunk of a ragged matrix has none).
inline PredictBatchPlan plan_predict_batch(const Knobs& m, const int32_t* clip_first, int C, int half, int jump, int chunk) {
    PredictBatchPlan p;
    const ClipTotals t = clip_totals(clip_first, C, half, jump);
    p.err = t.err;
    p.msg = t.msg;
    if (!p.err && chunk <= 0) {
        p.err = SAVAD_E_INVALID;
        p.msg = "chunk must be positive";
    }
    if (p.err) return p;
    p.W = t.W;
    p.C = C;
    p.rows = t.rows;
    p.n_items = t.n_items;
    p.chunk = windows::even_chunk(chunk, p.n_items);
    p.fwd_bytes = plan_forward(m, p.chunk, p.W, false, 0).total;
    const windows::Layout l = windows::layout((size_t)C + 1, p.n_items > 0 ? p.n_items : 1, p.chunk, p.W, m.feature_size, p.fwd_bytes);
    p.items_first = l.items_first, p.logp = l.logp, p.windows = l.windows, p.fwd = l.fwd, p.total = l.total;
    return p;
}

}  // namespace sched
}  // namespace savad
