// savad_live_plan.h -- the host plan of the live mode (audio fed as it arrives, many streams per tick), free of HIP: every count of a
// tick, the per-stream state sizes, and the tables the kernels of savad_live.h read.  Plain integer arithmetic; savad.hip launches
// from it and never reads a count back from the device; tests/live_dump.cpp includes this header alone.
//
// Shipped front-end, 16 kHz mono: frame f reads samples 160 f - 208 ... 160 f + 207 (the 400 samples under the window sit inside
// that 416-sample stretch).  After n samples of an OPEN stream
//   ready frames  K(n) = 0 for n < 257 (the offline minimum: the left reflection reads samples 1 .. 208 and the front-end refuses
//                 less), else (n - 208) / 160 + 1: frame f < K(n) reads only samples that exist, so it is the finished recording's
//   ready windows centres half .. K - 1 - half: max(0, K - 2 half) of them, window j has centre j + half
//   final rows    E(n) = max(0, K - 2 half): row f needs windows up to f (slot (f, w) holds window f - half - off[w])
// and at finish N = 1 + n / 160 frames exist, the last of them through the right-hand reflection.
//
// State of a stream (caller-owned device memory, one stride per slot):
//   samples   two buffers of sample_cap floats, used alternately: a tick copies the samples its not-yet-ready frames still read
//             (from keep_from(n), a multiple of 16) to the front of the other buffer and writes the push behind them -- compacted
//             linear, so a tile's samples are one contiguous, 16-byte aligned stretch (position == index mod 4), and no lane moves
//             data inside a buffer another lane reads
//   head/tail the mirrored stretches of the padded signal: indices [48, 256) once the first frames are ready, and the stretch past
//             the last sample at finish
//   feature   a ring of 2 half + max_new_frames rows: row r of the recording at r mod cap (the rows a tick keeps, K - 2 half .. K - 1,
//             and the ones it adds never meet; a log-mel tile is cut where the ring wraps)
//   logp      a ring of 2 half + max_new_frames windows' (log p0, log p1) [W], window j at j mod cap
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "savad_audio_host.h"
#include "savad_windows.h"   // the window offsets, the item rule

namespace savad {
namespace live {

constexpr int HOP = mel::HOP, N_MELS = mel::N_MELS;
constexpr int READ_BEFORE = 208;     // frame f reads samples [160 f - 208, 160 f + 208)
constexpr int MIN_SAMPLES = mel::N_FFT / 2 + 1;
constexpr int HEAD_J0 = 48, HEAD_FLOATS = mel::N_FFT / 2 - HEAD_J0;   // padded indices [48, 256)
constexpr int TAIL_FLOATS = 224;     // at most 212 are used
constexpr long NEVER = 1L << 40;
constexpr uint32_t TABLE_MAGIC = 0x4c495645u;

inline long ready_frames(long n) { return n < MIN_SAMPLES ? 0 : (n - READ_BEFORE) / HOP + 1; }
inline long total_frames(long n) { return 1 + n / HOP; }
inline long final_rows(long frames, int half) { return windows::items(frames, half); }
// first sample the frames that are not ready after n samples still read
inline long keep_from(long n) {
    const long s = (long)HOP * ready_frames(n) - READ_BEFORE;
    return s > 0 ? s : 0;
}

struct Geometry {
    int err = 0;
    const char* msg = nullptr;
    int streams = 0, max_push = 0, half = 0, jump = 0, F = N_MELS, W = 0, P = 1;
    int32_t off[windows::MAX_FRAMES];
    int max_new = 0;                       // frames (hence windows) one tick adds to a stream at most
    int max_rows = 0;                       // rows one tick emits for a stream at most (finish)
    int feat_cap = 0, logp_cap = 0, sample_cap = 0;
    size_t o_samples = 0, o_head = 0, o_tail = 0, o_feat = 0, o_logp = 0, stride = 0;   // bytes inside a slot's state
    size_t state_bytes() const { return stride * (size_t)streams; }
    int max_tiles() const { return (max_new + 31) / 32 + 1; }         // per stream and tick (+ 1: the ring wrap)
    int max_items() const { return max_new + 2 * (P - 1); }           // per stream and tick (slot padding either side)
};

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

inline Geometry geometry(int streams, int max_push, int half, int jump) {
    Geometry g;
    if (streams < 1 || max_push < 1 || half < 0 || jump < 1) {
        g.err = -1;
        g.msg = "streams, max_push_samples and jump must be >= 1, half >= 0";
        return g;
    }
    if (max_push > (1 << 24) || streams > (1 << 20)) {
        g.err = -2;
        g.msg = "more than 2^24 samples per push or 2^20 streams";
        return g;
    }
    const long W = windows::offsets(half, jump, g.off);
    if (W > windows::MAX_FRAMES) {
        g.err = -2;
        g.msg = windows::TOO_LONG;
        return g;
    }
    g.W = (int)W;
    g.streams = streams, g.max_push = max_push, g.half = half, g.jump = jump;
    g.P = g.W <= 32 ? 32 / g.W : 1;
    // K(n + p) - K(n) <= p / 160 + 2 (from K = 0), N(n + p) - K(n) <= p / 160 + 3
    g.max_new = max_push / HOP + 3;
    g.max_rows = g.max_new + 2 * half;
    g.feat_cap = g.logp_cap = 2 * half + g.max_new;
    g.sample_cap = (2 * READ_BEFORE - 1 + max_push + 3) & ~3;   // n - keep_from(n) <= 415
    size_t o = 0;
    g.o_samples = o, o += up16(sizeof(float) * 2 * (size_t)g.sample_cap);
    g.o_head = o, o += up16(sizeof(float) * HEAD_FLOATS);
    g.o_tail = o, o += up16(sizeof(float) * TAIL_FLOATS);
    g.o_feat = o, o += up16(sizeof(float) * (size_t)g.feat_cap * g.F);
    g.o_logp = o, o += up16(sizeof(float) * (size_t)g.logp_cap * g.W * 2);
    g.stride = (o + 255) & ~(size_t)255;
    return g;
}

// HOST state of a slot (caller-owned; all zero = closed)
struct Slot {
    int64_t n;        // samples pushed so far
    int64_t base;     // sample index at position 0 of the current sample buffer
    int32_t open;
    int32_t phase;    // which of the two sample buffers holds [base, n)
};

struct Push {
    int32_t slot, count, dtype /* 0 int16 PCM, 1 float32 (SAVAD_PCM_*) */, finish;
    uint64_t data;    // DEVICE address of the chunk when the tick's kernels run
};

// ---- the tables (one blob; host and device copies hold the same bytes) --------------------------------------------------------
struct Header {
    uint32_t magic;
    int32_t n_entries, n_tiles, n_items, n_rows;
    int32_t o_entries, o_tiles, o_items, o_rows;   // byte offsets
    int32_t total;
    int32_t max_append;                            // largest element count an entry's append moves
    int32_t pad[5];
};
static_assert(sizeof(Header) == 64, "Header");

// one stream of the tick
struct Entry {
    int32_t slot, finish, dtype, push;
    uint64_t src, buf_old, buf_new, head, tail, feat, logp;
    int64_t n_before, n_after, base_before, base_after, tail_j0;
    int32_t keep_off, keep_count;          // old positions [keep_off, + keep_count) -> new [0, keep_count)
    int32_t head_write, tail_count;
    int32_t frame_first_mod, n_frames;     // new feature rows: ring positions from frame_first_mod on
    int32_t win_first_mod, n_windows;      // new windows: ring positions from win_first_mod on
    int32_t win_kept;                      // windows before the new ones that the ring still holds (<= 2 half)
    int32_t item0;                         // item of the first new window
    int32_t row_count, row_out;            // rows emitted, first row in the compact output
    int64_t row_first;                     // first emitted row's index in the recording
    int32_t phase_after, pad;
};
static_assert(sizeof(Entry) % 8 == 0, "Entry");

// one log-mel tile: FftWhere of savad_logmel.h, frames, output rows
struct Tile {
    uint64_t srcA, srcB, srcY;
    int64_t J0, j_last, jA_end, jB0;
    uint64_t out;
    int32_t count, entry;
};
static_assert(sizeof(Tile) == 72, "Tile");

struct Item {
    int32_t entry;     // -1: a dummy (zeros, result dropped)
    int32_t centre;    // ring position of the window's centre row
};

inline size_t table_bytes(const Geometry& g, int max_entries) {
    size_t o = sizeof(Header);
    o += up16(sizeof(Entry) * (size_t)max_entries);
    o += up16(sizeof(Tile) * (size_t)max_entries * g.max_tiles());
    o += up16(sizeof(Item) * (size_t)max_entries * g.max_items());
    o += up16(sizeof(int32_t) * ((size_t)max_entries + 1));
    return o;
}

struct PlanResult {
    int err = 0;
    char msg[160] = {0};
};

inline PlanResult refuse(int err, const char* fmt, long a = 0, long b = 0, long c = 0) {
    PlanResult r;
    r.err = err;
    snprintf(r.msg, sizeof r.msg, fmt, a, b, c);
    return r;
}

// The tick of `pushes` (each slot at most once) against the slots as they stand: fills `table` (table_bytes(g, n_pushes) bytes at
// least) and, when given, rows[2 i] / rows[2 i + 1] = first row index in the recording / row count of push i.  Changes no slot:
// commit() does, once the tick has been launched.  state_dev is only turned into addresses, never read.
inline PlanResult plan_tick(const Geometry& g, const Slot* slots, const Push* pushes, int n_pushes, uint64_t state_dev, void* table,
                            size_t table_size, int64_t* rows) {
    if (g.err) {
        PlanResult r;
        r.err = g.err;
        snprintf(r.msg, sizeof r.msg, "%s", g.msg ? g.msg : "bad geometry");
        return r;
    }
    if (!slots || !table || (n_pushes > 0 && !pushes) || n_pushes < 0) return refuse(-1, "null table or slots");
    if (table_size < table_bytes(g, n_pushes)) return refuse(-1, "table too small: %ld < %ld bytes", (long)table_size, (long)table_bytes(g, n_pushes));
    for (int i = 0; i < n_pushes; ++i) {
        const Push& p = pushes[i];
        if (p.slot < 0 || p.slot >= g.streams) return refuse(-1, "push %ld names slot %ld of %ld", i, p.slot, g.streams);
        if (!slots[p.slot].open) return refuse(-1, "push %ld names slot %ld, which is closed", i, p.slot);
        if (p.count < 0 || p.count > g.max_push) return refuse(-1, "push %ld holds %ld samples, the declared maximum is %ld", i, p.count, g.max_push);
        if (p.dtype < 0 || p.dtype > 1) return refuse(-1, "push %ld: sample type %ld (0 int16, 1 float32)", i, p.dtype);
        if (p.count > 0 && (!p.data || (p.data & (p.dtype ? 3 : 1)))) return refuse(-1, "push %ld: null or misaligned samples", i);
        if (p.finish && slots[p.slot].n + p.count < MIN_SAMPLES)
            return refuse(-1, "finish of slot %ld after %ld samples: the front-end needs %ld", p.slot, (long)(slots[p.slot].n + p.count), MIN_SAMPLES);
        for (int k = 0; k < i; ++k)
            if (pushes[k].slot == p.slot) return refuse(-1, "slot %ld appears twice in one tick", p.slot);
    }
    char* tb = (char*)table;
    Header h;
    memset(&h, 0, sizeof h);
    h.magic = TABLE_MAGIC;
    h.n_entries = n_pushes;
    size_t o = sizeof(Header);
    h.o_entries = (int32_t)o, o += up16(sizeof(Entry) * (size_t)n_pushes);
    h.o_tiles = (int32_t)o, o += up16(sizeof(Tile) * (size_t)n_pushes * g.max_tiles());
    h.o_items = (int32_t)o, o += up16(sizeof(Item) * (size_t)n_pushes * g.max_items());
    h.o_rows = (int32_t)o, o += up16(sizeof(int32_t) * ((size_t)n_pushes + 1));
    h.total = (int32_t)o;
    Entry* entries = (Entry*)(tb + h.o_entries);
    Tile* tiles = (Tile*)(tb + h.o_tiles);
    Item* items = (Item*)(tb + h.o_items);
    int32_t* row_out = (int32_t*)(tb + h.o_rows);
    const int half = g.half;
    for (int i = 0; i < n_pushes; ++i) {
        const Push& p = pushes[i];
        const Slot& s = slots[p.slot];
        const uint64_t st = state_dev + g.stride * (uint64_t)p.slot;
        Entry e;
        memset(&e, 0, sizeof e);
        e.slot = p.slot, e.finish = p.finish ? 1 : 0, e.dtype = p.dtype, e.push = p.count;
        e.src = p.data;
        e.buf_old = st + g.o_samples + sizeof(float) * (size_t)g.sample_cap * (s.phase & 1);
        e.buf_new = st + g.o_samples + sizeof(float) * (size_t)g.sample_cap * ((s.phase & 1) ^ 1);
        e.head = st + g.o_head, e.tail = st + g.o_tail, e.feat = st + g.o_feat, e.logp = st + g.o_logp;
        e.n_before = s.n, e.n_after = s.n + p.count;
        e.base_before = s.base, e.base_after = keep_from(s.n);
        e.keep_off = (int32_t)(e.base_after - s.base), e.keep_count = (int32_t)(s.n - e.base_after);
        e.phase_after = (s.phase & 1) ^ 1;
        const long K0 = ready_frames(s.n), K1 = e.finish ? total_frames(e.n_after) : ready_frames(e.n_after);
        const long E0 = final_rows(K0, half), E1 = final_rows(K1, half);
        e.head_write = K0 == 0 && K1 > 0;
        const long j_last = (long)HOP * (K1 - 1) + 460;   // the last 16-byte chunk the new frames read (padded index)
        long jb = NEVER;
        if (e.finish) {
            jb = (e.n_after + 253 + 3) & ~3L;   // first chunk that runs past the last sample
            if (j_last >= jb) e.tail_count = (int32_t)(j_last + 4 - jb);
            else jb = NEVER;
        }
        e.tail_j0 = jb;
        e.frame_first_mod = (int32_t)(K0 % g.feat_cap), e.n_frames = (int32_t)(K1 - K0);
        e.win_first_mod = (int32_t)(E0 % g.logp_cap), e.n_windows = (int32_t)(E1 - E0);
        e.win_kept = (int32_t)(E0 < 2L * half ? E0 : 2L * half);
        e.row_first = E0, e.row_count = (int32_t)((e.finish ? K1 : E1) - E0);
        e.row_out = h.n_rows;
        row_out[i] = h.n_rows;
        h.n_rows += e.row_count;
        if (rows) rows[2 * i] = E0, rows[2 * i + 1] = e.row_count;
        // log-mel tiles: at most 32 frames, rows contiguous in the ring
        for (long f = K0; f < K1;) {
            const long pos = f % g.feat_cap;
            long cnt = K1 - f < 32 ? K1 - f : 32;
            if (pos + cnt > g.feat_cap) cnt = g.feat_cap - pos;
            Tile t;
            memset(&t, 0, sizeof t);
            t.srcA = e.head - 4 * (uint64_t)HEAD_J0;
            t.srcB = e.tail - 4 * (uint64_t)(jb == NEVER ? 0 : jb);
            t.srcY = e.buf_new - 4 * (uint64_t)(e.base_after + mel::N_FFT / 2);
            t.J0 = (long)HOP * f + 48, t.j_last = j_last, t.jA_end = mel::N_FFT / 2, t.jB0 = jb;
            t.out = e.feat + sizeof(float) * (size_t)pos * g.F;
            t.count = (int32_t)cnt, t.entry = i;
            tiles[h.n_tiles++] = t;
            f += cnt;
        }
        // items: window j of the stream at slot j mod P of its packed block
        if (e.n_windows > 0) {
            for (long k = 0; k < E0 % g.P; ++k) items[h.n_items++] = Item{-1, 0};
            e.item0 = h.n_items;
            for (long j = E0; j < E1; ++j) items[h.n_items++] = Item{i, (int32_t)((j + half) % g.feat_cap)};
            while (h.n_items % g.P) items[h.n_items++] = Item{-1, 0};
        }
        const int moved = e.keep_count + e.push;
        if (moved > h.max_append) h.max_append = moved;
        entries[i] = e;
    }
    row_out[n_pushes] = h.n_rows;
    memcpy(tb, &h, sizeof h);
    return PlanResult{};
}

inline const Header* header(const void* table) { return (const Header*)table; }
inline const Entry* entries(const void* table) { return (const Entry*)((const char*)table + header(table)->o_entries); }

// the table still describes the slots: every entry's stream is open and stands where the plan found it
inline PlanResult check_table(const Geometry& g, const void* table, const Slot* slots) {
    if (!table) return refuse(-1, "null table");
    const Header* h = header(table);
    if (h->magic != TABLE_MAGIC || h->n_entries < 0 || h->n_entries > g.streams) return refuse(-1, "not a live table");
    if (slots) {
        const Entry* e = entries(table);
        for (int i = 0; i < h->n_entries; ++i) {
            if (e[i].slot < 0 || e[i].slot >= g.streams) return refuse(-1, "entry %ld names slot %ld", i, e[i].slot);
            const Slot& s = slots[e[i].slot];
            if (!s.open) return refuse(-1, "the table names slot %ld, which is closed", e[i].slot);
            if (s.n != e[i].n_before || s.base != e[i].base_before || (s.phase & 1) == e[i].phase_after)
                return refuse(-1, "the table was planned for another state of slot %ld", e[i].slot);
        }
    }
    return PlanResult{};
}

// the tick has been launched: the slots move on
inline void commit(const void* table, Slot* slots) {
    const Header* h = header(table);
    const Entry* e = entries(table);
    for (int i = 0; i < h->n_entries; ++i) {
        Slot& s = slots[e[i].slot];
        s.n = e[i].n_after, s.base = e[i].base_after, s.phase = e[i].phase_after;
        if (e[i].finish) s = Slot{0, 0, 0, 0};
    }
}

// forward calls of a tick: `chunk` items each, a multiple of the packed block's slots (and even: a chunk's log-probs start 16-byte aligned)
inline int chunk_items(const Geometry& g, int chunk) {
    const int unit = g.P % 2 ? 2 * g.P : g.P;
    const int c = chunk / unit * unit;
    return c < unit ? unit : c;
}

}  // namespace live
}  // namespace savad
