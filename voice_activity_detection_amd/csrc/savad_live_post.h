// savad_live_post.h -- the post-processing of a LIVE stream on the device: the rows a tick made final -> boosted mean -> threshold
// -> trim -> sample classes -> START / END events, as soon as no continuation of the recording can change them.  The events of a
// stream, concatenated, are the segments of the offline path (savad_post_device.h) over the finished recording, index for index.
// Shipped geometry only (hop 160, window 400 samples, 16 kHz), as the live mode itself.
//
// The arithmetic comes from the inlines of savad_post_device.h (row_mean, above, cover_of), and the streaming rules are stated once
// below as __host__ __device__ inlines: the kernel and the host twin (savad_live_post_host) run the same code.
//
// WHAT IS BUILT: an automaton per stream, not the 64-lane edge scans of the offline path.  A pass of trim edits whole runs: pass 0
// fills a run of zeros between two ones that is shorter than v, pass 1 flattens a run of ones between two zeros that is shorter
// than h, pass 2 turns the first o zeros after a fall and the last b zeros before a rise into ones.  A run's length saturates at the
// threshold it is compared with, and the frames of a run that is still undecided all have ONE value, so a COUNTER stands for the
// undetermined tail of each pass: the state of a stream is 64 bytes whatever v, h, b and o are, and a step touches no array.  With
// typically one to ten rows per stream and tick there is nothing for 64 lanes to scan; the wave's lanes compute the row means (the
// part that reads memory), a ballot turns 64 rows into one mask, and lane 0 steps the automaton over the mask.
//
// Pass 0 (valley), input raw r, output p0.  A 1 is final.  A 0 before the first 1 is final (leading zeros are never filled).  A 0
//   after a 1 waits: zrun = zeros of the open valley, held back while zrun < v; at zrun == v they are final zeros, as is every further
//   zero of that valley; a 1 while 0 < zrun < v makes them ones.                                             held back: <= v - 1
// Pass 1 (hill), input p0, output p1.  A 0 is final.  A 1 before the first 0 is final (a leading hill is never flattened).  A 1 after
//   a 0 waits: orun = ones of the open hill, held back while orun < h; at orun == h they are final ones; a 0 while 0 < orun < h
//   makes them zeros.                                                                                        held back: <= h - 1
// Pass 2 (hang), input p1, only when b > 0 (the reference's `hang_before > 0 or hang_before > 0`).  A 1 is final.  A 0 among the
//   first o of a run that follows a 1 is a final 1.  Any other 0 waits among the last `pend` <= b zeros: one more zero makes the
//   oldest of b waiting zeros a final 0, a 1 makes all of them ones.                                         held back: <= b
// A skipped pass (v == 0, h == 0, b == 0) hands its input on.  At finish every pass, in order, releases what it holds with "no next
// edge": zeros stay zeros, ones stay ones.  So after R rows D2 >= R - (v + h + b) frames are final.
//
// Samples: frame f covers samples [160 f, 160 f + 400), so sample 160 k + r is covered by frames k - 2 .. k for r < 80 and by
// k - 1 .. k for r >= 80 (clipped to the frames that exist): the class is constant on half hops, and a final frame f makes the
// two pieces [160 f, 160 f + 80) and [160 f + 80, 160 f + 160) final.  Each piece's class comes from cover_of (the exact predicate)
// at its first sample with n = f + 1 frames, over the last three final frames.  At finish with N frames three more pieces follow,
// up to sample (N - 1) 160 + 400.  The segment machine is convert_samples_to_segments over the pieces.
#pragma once
#include "savad_live_plan.h"
#include "savad_post_device.h"

namespace savad {
namespace livepost {

#define SAVAD_HD __host__ __device__ inline

constexpr int START = 0, END = 1;   // SAVAD_LIVE_EVENT_*
constexpr int HOP = 160, PIECE = 80;

struct Event {   // savad_live_event
    int64_t sample;
    int32_t slot, kind;
};
static_assert(sizeof(Event) == 16, "Event");

struct Params {
    int W;
    float threshold;
    int v, h, b, o;
};

// a stream's state: needs no initialisation (an entry with row_first == 0 resets it)
struct State {
    int64_t next_row;     // rows fed so far = the row_first the next entry must have; -1 after a finish
    int64_t frames_out;   // D2: frames whose trimmed value is final
    int32_t seen_one, zrun;          // pass 0: a 1 has come; zeros of the open valley (<= v)
    int32_t seen_zero, orun;         // pass 1: a 0 has come; ones of the open hill (<= h)
    int32_t hang_one, zpos, pend;    // pass 2: a 1 has come; zeros of the open run (<= o); zeros held back (<= b)
    int32_t f0, f1, f2;              // the final frames D2 - 1, D2 - 2, D2 - 3
    int32_t in_voice;
    int32_t pad;
};
static_assert(sizeof(State) == 64, "State");

// where a tick's events go: slot k of `out` while k < cap; n counts all of them
struct Sink {
    Event* out;
    int cap, n;
    int32_t slot;
};

// events one entry can emit: an event needs a class change ONE <-> ZERO, which takes four pieces = two frames; a finish adds three
// pieces and the END of an open segment
SAVAD_HD int event_cap(int row_count, const Params& p) { return (row_count + p.v + p.h + p.b) / 2 + 4; }

SAVAD_HD void emit(Sink& k, int kind, int64_t sample) {
    if (k.n < k.cap) k.out[k.n] = Event{sample, k.slot, kind};
    ++k.n;
}

SAVAD_HD postdev::Geometry shipped_geometry() { return postdev::make_geometry(1, 16000, 10.0, 25.0); }

// class of the piece that starts at sample i, with g.n final frames of which the last three are s.f0, s.f1, s.f2
SAVAD_HD uint8_t piece_class(const State& s, const postdev::Geometry& g, long i) {
    long first;
    const int count = postdev::cover_of(g, i, &first);
    int ones = 0;
    for (int k = 0; k < count; ++k) {
        const long back = g.n - 1 - (first + k);   // 0, 1 or 2
        ones += back == 0 ? s.f0 : back == 1 ? s.f1 : s.f2;
    }
    if (ones == 0) return postdev::ZERO;
    return ones == count ? postdev::ONE : postdev::MID;
}

SAVAD_HD void piece(State& s, Sink& k, const postdev::Geometry& g, long i) {
    const uint8_t cls = piece_class(s, g, i);
    if (cls == postdev::ONE && !s.in_voice) {
        emit(k, START, i);
        s.in_voice = 1;
    } else if (cls == postdev::ZERO && s.in_voice) {
        emit(k, END, i - 1);
        s.in_voice = 0;
    }
}

// frame D2 is final with value x
SAVAD_HD void frame_out(State& s, Sink& k, postdev::Geometry& g, int x) {
    const long f = (long)s.frames_out;
    s.f2 = s.f1, s.f1 = s.f0, s.f0 = x;
    s.frames_out = f + 1;
    g.n = (int)(f + 1);
    piece(s, k, g, f * HOP);
    piece(s, k, g, f * HOP + PIECE);
}

SAVAD_HD void hang_in(State& s, Sink& k, postdev::Geometry& g, const Params& p, int x) {
    if (p.b <= 0) return frame_out(s, k, g, x);
    if (x) {
        for (; s.pend > 0; --s.pend) frame_out(s, k, g, 1);   // a rise within hang_before of them
        frame_out(s, k, g, 1);
        s.hang_one = 1, s.zpos = 0;
    } else if (s.hang_one && s.zpos < p.o) {                   // within hang_over of the fall
        ++s.zpos;
        frame_out(s, k, g, 1);
    } else if (s.pend >= p.b) {
        frame_out(s, k, g, 0);                                 // the oldest waiting zero: b zeros behind it and no rise
    } else {
        ++s.pend;
    }
}

SAVAD_HD void hill_in(State& s, Sink& k, postdev::Geometry& g, const Params& p, int x) {
    if (p.h <= 0) return hang_in(s, k, g, p, x);
    if (x) {
        if (!s.seen_zero || s.orun >= p.h) return hang_in(s, k, g, p, 1);
        if (++s.orun >= p.h)
            for (int j = 0; j < p.h; ++j) hang_in(s, k, g, p, 1);
    } else {
        if (s.orun < p.h)
            for (int j = 0; j < s.orun; ++j) hang_in(s, k, g, p, 0);   // a hill shorter than h
        s.orun = 0, s.seen_zero = 1;
        hang_in(s, k, g, p, 0);
    }
}

SAVAD_HD void valley_in(State& s, Sink& k, postdev::Geometry& g, const Params& p, int x) {
    if (p.v <= 0) return hill_in(s, k, g, p, x);
    if (x) {
        if (s.zrun < p.v)
            for (int j = 0; j < s.zrun; ++j) hill_in(s, k, g, p, 1);   // a valley shorter than v
        s.zrun = 0, s.seen_one = 1;
        hill_in(s, k, g, p, 1);
    } else {
        if (!s.seen_one || s.zrun >= p.v) return hill_in(s, k, g, p, 0);
        if (++s.zrun >= p.v)
            for (int j = 0; j < p.v; ++j) hill_in(s, k, g, p, 0);
    }
}

// the entry continues the state (or starts a recording)?  A state that never saw a reset may hold anything: its counters are
// brought into their ranges, so that no loop below runs longer than its threshold.
SAVAD_HD bool begin(State& s, int64_t row_first, const Params& p) {
    if (row_first == 0) {
        s = State{};
        return true;
    }
    if (row_first < 0 || s.next_row != row_first) return false;
    s.zrun = s.zrun < 0 ? 0 : s.zrun > p.v ? p.v : s.zrun;
    s.orun = s.orun < 0 ? 0 : s.orun > p.h ? p.h : s.orun;
    s.pend = s.pend < 0 ? 0 : s.pend > p.b ? p.b : s.pend;
    s.zpos = s.zpos < 0 ? 0 : s.zpos > p.o ? p.o : s.zpos;
    return true;
}

// rows next_row .. next_row + n - 1 (n <= 64): bit j of `bits` = the thresholded mean of row j
SAVAD_HD void feed_bits(State& s, Sink& k, postdev::Geometry& g, const Params& p, uint64_t bits, int n) {
    for (int j = 0; j < n; ++j) valley_in(s, k, g, p, (int)((bits >> j) & 1));
    s.next_row += n;
}

// the recording ends: every pass releases what it holds, the last pieces follow, an open segment ends at the last sample
SAVAD_HD void finish(State& s, Sink& k, postdev::Geometry& g, const Params& p) {
    if (p.v > 0 && s.zrun < p.v)
        for (int j = 0; j < s.zrun; ++j) hill_in(s, k, g, p, 0);
    s.zrun = 0;
    if (p.h > 0 && s.orun < p.h)
        for (int j = 0; j < s.orun; ++j) hang_in(s, k, g, p, 1);
    s.orun = 0;
    for (; s.pend > 0; --s.pend) frame_out(s, k, g, 0);
    const long N = (long)s.frames_out;
    if (N > 0) {
        g.n = (int)N;
        for (int j = 0; j < 3; ++j) piece(s, k, g, N * HOP + j * PIECE);
        if (s.in_voice) emit(k, END, (N - 1) * HOP + 400 - 1);
    }
    s.in_voice = 0;
    s.next_row = -1;
}

// ---- host twin: one entry of one stream in plain loops ------------------------------------------------------------------------
// returns the number of events (those beyond cap are counted, not written), or -1 where the entry does not continue the state
inline int run_host(State* state, const Params& p, int32_t slot, int64_t row_first, int row_count, int fin, const float* probs, Event* out, int cap) {
    State s = *state;
    if (!begin(s, row_first, p)) return -1;
    Sink k{out, cap, 0, slot};
    postdev::Geometry g = shipped_geometry();
    for (int base = 0; base < row_count; base += 64) {
        const int n = row_count - base < 64 ? row_count - base : 64;
        uint64_t bits = 0;
        for (int j = 0; j < n; ++j)
            bits |= (uint64_t)postdev::above(postdev::row_mean(probs + (size_t)(base + j) * p.W, p.W), p.threshold) << j;
        feed_bits(s, k, g, p, bits, n);
    }
    if (fin) finish(s, k, g, p);
    *state = s;
    return k.n;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------

// One wave per entry of the tick.  The lanes take a row each (64 rows a turn), the ballot of their thresholded means is the mask
// lane 0 steps the automaton over.  Events go to the entry's own stretch of `raw` (cap slots), their number to counts[entry]
// (-1: the entry does not continue its stream's state, which is left as it is).
__global__ void __launch_bounds__(64) post_kernel(const live::Entry* __restrict__ entries, int n_entries, int streams, const float* __restrict__ probs,
                                                  Params p, State* __restrict__ states, Event* __restrict__ raw, int cap, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < n_entries; e += gridDim.x) {
        const int32_t slot = entries[e].slot;
        const int64_t row_first = entries[e].row_first;
        const int row_count = entries[e].row_count, row_out = entries[e].row_out, fin = entries[e].finish;
        if (slot < 0 || slot >= streams) {
            if (lane == 0) counts[e] = -1;
            continue;
        }
        State s = states[slot];
        if (!begin(s, row_first, p)) {
            if (lane == 0) counts[e] = -1;
            continue;
        }
        Sink k{raw + (size_t)e * cap, cap, 0, slot};
        postdev::Geometry g = shipped_geometry();
        for (int base = 0; base < row_count; base += 64) {
            const int n = row_count - base < 64 ? row_count - base : 64;
            int bit = 0;
            if (lane < n) bit = postdev::above(postdev::row_mean(probs + ((size_t)row_out + base + lane) * p.W, p.W), p.threshold);
            const uint64_t bits = __ballot(bit);
            if (lane == 0) feed_bits(s, k, g, p, bits, n);
        }
        if (lane == 0) {
            if (fin) finish(s, k, g, p);
            states[slot] = s;
            counts[e] = k.n < cap ? k.n : cap;
        }
    }
}

struct OpSum {
    typedef int T;
    __device__ static T identity() { return 0; }
    __device__ static T combine(T a, T b) { return a + b; }
};

// One workgroup: offsets = the exclusive scan of the entries' event counts (a -1 counts as none), counts_out = the counts as they
// are, events = the entries' events one after the other.  A thread moves the events of its entries: a tick has few.
__global__ void __launch_bounds__(256) compact_kernel(const Event* __restrict__ raw, int cap, const int32_t* __restrict__ counts, int n_entries,
                                                      int32_t* __restrict__ offsets, int32_t* __restrict__ counts_out, Event* __restrict__ events,
                                                      long events_cap) {
    int carry = 0;
    for (int base = 0; base < n_entries; base += 256) {
        const int e = base + (int)threadIdx.x;
        const int c = e < n_entries ? counts[e] : 0;
        const int own = c > 0 ? c : 0;
        int total;
        const int at = carry + postdev::block_exclusive<OpSum>(own, &total);
        if (e < n_entries) {
            offsets[e] = at;
            counts_out[e] = c;
            for (int j = 0; j < own; ++j)
                if ((long)at + j < events_cap) events[at + j] = raw[(size_t)e * cap + j];
        }
        carry += total;
        __syncthreads();   // block_exclusive's wave totals are read before the next turn writes them
    }
    if (threadIdx.x == 0) offsets[n_entries] = carry;
}

#undef SAVAD_HD

}  // namespace livepost
}  // namespace savad
