// savad_post_batch.h -- the device post-processing of savad_post_device.h for EVERY CLIP OF A BATCH at once: probabilities
// [sum N, W] and a clip table -> every clip's segments, with a number of launches that does not depend on the number of clips.
// The per-element arithmetic is savad_post_device.h's (row_mean, above, edge_index, trim_pass_value, cover_of, sample_class);
// what is new is the clip handling, stated once below as __host__ __device__ inlines that the kernels and the host twin
// (savad_post_batch_frames_host) both run.  The scans are the generic scan_run: the only ordering between workgroups is the
// boundary between launches; no atomics, no polling.
//
// Frames.  Rows keep their GLOBAL index.  An edge never exists at a clip's first row (its predecessor belongs to another clip),
// so the edge scans run over the whole matrix as they are, and the apply step clamps what they answer against the row's clip
// [lo, hi): a "last edge <= i" before lo is none, a "first edge > i" at or after hi is none.  What remains are the clip's own
// edges, and a pass only uses differences of indices.  A row finds its clip once (frames kernel: upper_bound - 1 in the table;
// empty clips make entries repeat, so the LAST entry <= i is the owner) and leaves lo and hi beside it.
//
// Samples.  The clips' sample domains lie one after the other as SLOTS: clip c with n_c > 0 frames owns make_geometry(n_c).num
// samples and one CLOSING slot behind them (where a segment still open after the last sample ends); a clip without rows owns
// nothing.  slot_first [C + 1] is the exclusive prefix sum.  A slot's class comes from its own clip's frames and geometry; the
// closing slot has the class CLOSE, which the state scan reads as ZERO: "voice before sample i" therefore restarts at every
// clip's first sample whatever that sample's class is.  (Under geometry_supported sample 0 of a clip is covered by frame 0
// alone -- frame f >= 1 starts at f * hop >= 1 -- so it is never MID and the scan would restart by itself; the closing slot
// makes the restart independent of that.)
//
// Segments.  Output slots are the global prefix sums of the start and of the end flags; indices are written LOCAL to the
// clip.  The closing slot of clip c records the running count (clip_total[c]); the host turns those into seg_first [C + 1].
// A last launch over the segments flags the clips that hold one longer than max_samples (one byte per clip; racing stores of
// the same value).
#pragma once
#include "savad_post_device.h"

namespace savad {
namespace postdev {

#define SAVAD_HD __host__ __device__ inline

constexpr uint8_t CLOSE = 3;   // class of a clip's closing slot

// the clip that owns element i of a table first[0 .. C] (non-decreasing, first[0] = 0, 0 <= i < first[C]): the LAST c with
// first[c] <= i (upper_bound - 1; repeated entries are empty clips, which own nothing)
template <class T>
SAVAD_HD int clip_of(const T* first, int C, long i) {
    int lo = 0, hi = C;   // first[lo] <= i < first[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long)first[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// edge index of global row i whose clip starts at row lo: none at the clip's first row
SAVAD_HD int edge_index_clip(const uint8_t* s, int i, int kind, int none, int lo) { return i == lo ? none : edge_index(s, i, kind, none); }

// what the whole-matrix scans answer, seen from a row of the clip [lo, hi)
SAVAD_HD int clamp_last(int last, int lo) { return last < lo ? -1 : last; }
SAVAD_HD int clamp_next(int next, int hi) { return next >= hi ? INT_MAX : next; }

// slots of a clip of n frames: its samples and the closing slot; none without frames
SAVAD_HD long clip_slots(int n, int sample_rate, double hop_ms, double window_ms) {
    return n > 0 ? make_geometry(n, sample_rate, hop_ms, window_ms).num + 1 : 0;
}

// class of slot `local` of a clip of n frames `frames`
SAVAD_HD uint8_t slot_class(const uint8_t* frames, int n, long local, int sample_rate, double hop_ms, double window_ms) {
    const Geometry g = make_geometry(n, sample_rate, hop_ms, window_ms);
    return local == g.num ? CLOSE : sample_class(frames, g, local);
}

// ---- host twins ------------------------------------------------------------------------------------------------------------

// row -> its clip's [lo, hi), by the search the frames kernel runs
inline void clip_bounds_host(const int32_t* clip_first, int C, int N, int* row_lo, int* row_hi) {
    for (int i = 0; i < N; ++i) {
        const int c = clip_of(clip_first, C, i);
        row_lo[i] = clip_first[c];
        row_hi[i] = clip_first[c + 1];
    }
}

// trim_host over the whole matrix with the clip rules: scans of global indices, clamped per row
inline void trim_batch_host(uint8_t* s, int N, const int* row_lo, const int* row_hi, int min_vally, int min_hill, int hang_before, int hang_over,
                            int* last, int* next) {
    for (int pass = 0; pass < 3; ++pass) {
        if ((pass == 0 && min_vally <= 0) || (pass == 1 && min_hill <= 0) || (pass == 2 && hang_before <= 0)) continue;
        const int k_last = pass == 1 ? 0 : 1, k_next = pass == 1 ? 1 : 0;
        int run = -1;
        for (int i = 0; i < N; ++i) {
            const int e = edge_index_clip(s, i, k_last, -1, row_lo[i]);
            run = e > run ? e : run;
            last[i] = run;
        }
        run = INT_MAX;
        for (int i = N - 1; i >= 0; --i) {   // next[i] = first edge > i
            next[i] = run;
            const int e = edge_index_clip(s, i, k_next, INT_MAX, row_lo[i]);
            run = e < run ? e : run;
        }
        for (int i = 0; i < N; ++i)
            s[i] = trim_pass_value(pass, s[i], i, clamp_last(last[i], row_lo[i]), clamp_next(next[i], row_hi[i]), min_vally, min_hill, hang_before,
                                   hang_over);
    }
}

inline void slot_table_host(const int32_t* clip_first, int C, int sample_rate, double hop_ms, double window_ms, long* slot_first) {
    slot_first[0] = 0;
    for (int c = 0; c < C; ++c) slot_first[c + 1] = slot_first[c] + clip_slots(clip_first[c + 1] - clip_first[c], sample_rate, hop_ms, window_ms);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

__global__ void frames_batch_kernel(const float* __restrict__ probs, const int32_t* __restrict__ clip_first, int C, int N, int W, float threshold,
                                    float* __restrict__ boosted, uint8_t* __restrict__ s, int* __restrict__ row_lo, int* __restrict__ row_hi) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const float m = row_mean(probs + i * W, W);
        boosted[i] = m;
        s[i] = above(m, threshold);
        const int c = clip_of(clip_first, C, i);
        row_lo[i] = clip_first[c];
        row_hi[i] = clip_first[c + 1];
    }
}

__global__ void trim_apply_batch_kernel(uint8_t* s, int N, int pass, const int* __restrict__ last, const int* __restrict__ next_incl,
                                        const int* __restrict__ row_lo, const int* __restrict__ row_hi, int min_vally, int min_hill, int hang_before,
                                        int hang_over) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const int next = i + 1 < N ? next_incl[i + 1] : INT_MAX;
        s[i] = trim_pass_value(pass, s[i], (int)i, clamp_last(last[i], row_lo[i]), clamp_next(next, row_hi[i]), min_vally, min_hill, hang_before,
                               hang_over);
    }
}

__global__ void slot_class_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ clip_first, const long* __restrict__ slot_first,
                                  int C, long slots, int sample_rate, double hop_ms, double window_ms, uint8_t* __restrict__ cls) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (long)gridDim.x * blockDim.x) {
        const int c = clip_of(slot_first, C, j);
        const int lo = clip_first[c];
        cls[j] = slot_class(frames + lo, clip_first[c + 1] - lo, j - slot_first[c], sample_rate, hop_ms, window_ms);
    }
}

// a clip with a segment longer than max_samples; seg_clip[k] = the clip of segment k
__global__ void long_flag_kernel(const long* __restrict__ starts, const long* __restrict__ ends, const int* __restrict__ seg_clip,
                                 const long* __restrict__ totals, long cap, long max_samples, uint8_t* flags) {
    const long count = totals[0] < cap ? totals[0] : cap;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (long)gridDim.x * blockDim.x)
        if (ends[k] + 1 - starts[k] > max_samples) flags[seg_clip[k]] = 1;
}

// ---- the scans' inputs and outputs -----------------------------------------------------------------------------------------

struct OpSumL {
    typedef long T;
    __device__ static T identity() { return 0; }
    __device__ static T combine(T a, T b) { return a + b; }
};

// slot_first[c + 1] = the inclusive sum of the clips' slots
struct SlotCountLoad {
    const int32_t* clip_first;
    int sample_rate;
    double hop_ms, window_ms;
    __device__ long operator()(long c) const { return clip_slots(clip_first[c + 1] - clip_first[c], sample_rate, hop_ms, window_ms); }
};
struct SlotFirstStore {
    long* slot_first;
    __device__ void operator()(long c, long v) const {
        if (c == 0) slot_first[0] = 0;
        slot_first[c + 1] = v;
    }
};

struct EdgeLoadBatch {   // EdgeLoad with the clip rule
    const uint8_t* s;
    const int* row_lo;
    int n, kind, reverse;
    __device__ int operator()(long j) const {
        const int i = reverse ? n - 1 - (int)j : (int)j;
        return edge_index_clip(s, i, kind, reverse ? INT_MAX : -1, row_lo[i]);
    }
};

struct ClassLoadBatch {   // the closing slot ends whatever was open: ZERO to the state scan
    const uint8_t* cls;
    __device__ int operator()(long j) const {
        const uint8_t c = cls[j];
        return c == CLOSE ? ZERO : c;
    }
};

// start / end flags of slot j: state[j] = the last non-MID class up to and including j (ZERO at a closing slot, so never ONE
// in front of a clip's first sample)
struct FlagLoadBatch {
    const uint8_t* cls;
    const uint8_t* state;
    __device__ Long2 operator()(long j) const {
        const bool voice = j > 0 && state[j - 1] == ONE;
        const uint8_t c = cls[j];
        if (c == CLOSE) return Long2{0, voice ? 1 : 0};
        return Long2{(c == ONE && !voice) ? 1 : 0, (c == ZERO && voice) ? 1 : 0};
    }
};
// scatter: the k-th start / end of the batch to slot k of `cap`-slot buffers, as indices local to the clip; a closing slot
// leaves the running count in clip_total[its clip]; the last slot the totals
struct SegmentStoreBatch {
    FlagLoadBatch flags;
    const long* slot_first;
    int C;
    long slots;
    long* starts;
    long* ends;
    int* seg_clip;
    long cap;
    long* clip_total;
    long* totals;
    __device__ void operator()(long j, Long2 v) const {
        const Long2 f = flags(j);
        const bool closing = flags.cls[j] == CLOSE;
        if (f.a || f.b || closing) {
            const int c = clip_of(slot_first, C, j);
            const long local = j - slot_first[c];
            if (f.a && v.a - 1 < cap) {
                starts[v.a - 1] = local;
                seg_clip[v.a - 1] = c;
            }
            if (f.b && v.b - 1 < cap) ends[v.b - 1] = local - 1;
            if (closing) clip_total[c] = v.a;
        }
        if (j == slots - 1) {
            totals[0] = v.a;
            totals[1] = v.b;
        }
    }
};

#undef SAVAD_HD

}  // namespace postdev
}  // namespace savad
