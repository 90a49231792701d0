// savad_windows.h -- the window geometry of the predictor (vad/predictor.py:159-262), written once: which frames a window reads, how
// many windows a recording has, how many of them one forward takes, and where the pieces of a prediction's workspace lie.  The
// single-clip plan, the clip-table plan (savad_schedule.h), the live plan (savad_live_plan.h) and savad.hip all read it from here;
// tests/windows_dump.cpp includes this header alone (tests/test_window_geometry_host.py).  Plain C++17: no HIP, no device code
// (the rules are constexpr, so a kernel may call them).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace savad {

// consecutive 256-byte-aligned regions of a caller's workspace or of one device allocation
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

namespace windows {

constexpr int MAX_FRAMES = 64;  // what WindowOffsets (savad_device.h) and live::Geometry hold
constexpr const char* TOO_LONG = "window longer than 64 frames";

// The frames of a window, relative to its centre: arange(-half, 0, jump) ++ [0] ++ arange(1, half + 1, jump) (vad/predictor.py:186-212).
// Both aranges have n = ceil(half / jump) entries.  Writes the first min(W, cap) offsets when `off` is given and returns W; the
// caller refuses W > MAX_FRAMES (TOO_LONG) wherever the offsets go into a fixed int32_t[MAX_FRAMES].  half >= 0, jump >= 1.
inline long offsets(int half, int jump, int32_t* off, long cap = MAX_FRAMES) {
    const long n = ((long)half + jump - 1) / jump, W = 2 * n + 1;
    for (long i = 0; off && i < W && i < cap; ++i) off[i] = (int32_t)(i < n ? -half + i * jump : i == n ? 0 : 1 + (i - n - 1) * jump);
    return W;
}

// windows of `rows` feature frames: one per centre that has `half` frames on either side (vad/predictor.py:169)
constexpr long items(long rows, long half) { return rows > 2 * half ? rows - 2 * half : 0; }

// items per forward: at most n_items, at least 1 ...
constexpr int at_most_items(long chunk, int n_items) { return chunk <= n_items ? (int)chunk : (n_items > 0 ? n_items : 1); }
// ... and for the chunk a caller names, even: a chunk's log-probs start at logp + first * W * 2 floats and savad_forward wants 16-byte
// aligned pointers, which an even `first` gives whatever W is (windows are independent: the chunking never changes a result)
constexpr int even_chunk(long chunk, int n_items) { return at_most_items(chunk + (chunk & 1), n_items); }

// [items_first [table_ints] int32] | logp [logp_items, W, 2] | windows [chunk, W, F] | the chunk-sized forward's workspace; a piece of
// no bytes takes no room (no table: the single clip and the live tick; no windows and no forward: the single-launch forwards that
// read their windows in place)
struct Layout {
    size_t items_first = 0, logp = 0, windows = 0, fwd = 0, total = 0;  // byte offsets
};
inline Layout layout(size_t table_ints, size_t logp_items, size_t chunk, int W, int F, size_t fwd_bytes) {
    Layout l;
    Arena a;
    l.items_first = a.take(sizeof(int32_t) * table_ints);
    l.logp = a.take(sizeof(float) * logp_items * W * 2);
    l.windows = a.take(sizeof(float) * chunk * W * F);
    l.fwd = a.take(fwd_bytes);
    l.total = a.off;
    return l;
}

}  // namespace windows
}  // namespace savad
