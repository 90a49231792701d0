// savad_eval_batch.h -- the device metrics of savad_eval_device.h for EVERY CLIP OF A BATCH at once: probabilities [rows, W] with
// their clip table, one concatenated label array with a table of its own -> every clip's counter block and boundary records, with
// a number of launches that does not depend on the number of clips.  The per-frame arithmetic is savad_eval_device.h's (key_of,
// count_frame, is_start / is_end, start_counts / end_counts, u2_term) and the scans are savad_post_device.h's scan_run; what is new
// is the clip handling.  The specification is evaldev::counts_host on each clip's slice (counts_host_batch below).
//
// Elements.  Clip c works on n_c = min(rows_c, labels_c) frames.  The frames of all clips lie one after the other as ELEMENTS:
// elem_first [C + 1] is the exclusive prefix sum of n_c, element e of clip c is row clip_first[c] + (e - elem_first[c]) of the
// matrix and label label_first[c] + (e - elem_first[c]).  The frames kernel leaves keys, labels and both predictions in element
// order and the element's clip beside them, so every later step hands the inline functions a pointer to the clip's first
// element, a LOCAL index and n_c: an edge, a boundary window or a tie group cannot see another clip.
//
// Counters.  A frame adds 0 or 1 to a counter, so a wave counts with ballots: the lanes of a wave hold consecutive elements, the
// lanes of one clip are a run of them, and the first lane of a run adds the set bits of ITS run to the clip's slot (one atomic
// per counter, clip and wave; integer sums, any order).  The rank sum's terms are not flags: a segmented shuffle scan adds them
// up within a run and the run's last lane adds the sum.
//
// Sort.  savad_eval_device.h's LSD radix passes with SORT BLOCKS THAT NEVER SPAN TWO CLIPS: clip c owns ceil(n_c / block)
// blocks (block_first [C + 1]).  The digit table is laid out clip-major, then digit-major, then by the clip's blocks, so ONE plain
// scan_run<OpSumU> over the whole table yields global positions: clip c's entries sum to n_c, so clip c + 1's positions begin at
// its own first element.  Four passes, none over clip ids, each stable within a clip.
//
// Rank sum.  The head / negatives scan runs over all elements with a group head at every clip's first element; a group's
// "negatives before" is taken relative to the count in front of its clip.
//
// Boundaries.  The start / end ranks under OpSum2 over all elements ARE the record indices in clip order, then segment order.
#pragma once
#include "savad_eval_device.h"
#include "savad_post_batch.h"

namespace savad {
namespace evalbatch {

namespace pd = savad::postdev;
namespace ed = savad::evaldev;

#define SAVAD_HD __host__ __device__ inline

SAVAD_HD long clip_frames(const int32_t* clip_first, const int32_t* label_first, long c) {
    const long rows = (long)clip_first[c + 1] - clip_first[c], labels = (long)label_first[c + 1] - label_first[c];
    return rows < labels ? rows : labels;
}

SAVAD_HD long blocks_of(long n, int block) { return (n + block - 1) / block; }

// ---- host twin -------------------------------------------------------------------------------------------------------------

// counters [C][COUNTERS], records in clip order then segment order (up to seg_cap of them), seg_first [C + 1]; returns the batch's
// true-segment count.  A clip without frames has zero counters.
inline long counts_host_batch(const float* probs, const int32_t* clip_first, const uint8_t* labels, const int32_t* label_first, int C, int W,
                              float threshold, int L, long* counters, uint8_t* seg, long seg_cap, long* seg_first) {
    long total = 0;
    seg_first[0] = 0;
    std::vector<uint8_t> records;
    for (int c = 0; c < C; ++c) {
        const int n = (int)clip_frames(clip_first, label_first, c);
        records.resize((size_t)ed::SEG_BYTES * (size_t)((n + 1) / 2) + 1);
        const long got = ed::counts_host(probs + (size_t)clip_first[c] * W, W, labels + label_first[c], n, threshold, L, counters + (size_t)c * ed::COUNTERS,
                                         records.data(), (n + 1) / 2);
        for (long k = 0; k < got; ++k)
            if (total + k < seg_cap) memcpy(seg + (size_t)(total + k) * ed::SEG_BYTES, records.data() + (size_t)k * ed::SEG_BYTES, ed::SEG_BYTES);
        total += got;
        seg_first[c + 1] = total;
    }
    return total;
}

// ---- the tables ------------------------------------------------------------------------------------------------------------

// elem_first[c + 1], block_first[c + 1] = the inclusive sums of the clips' frames and of their sort blocks
struct ClipCountLoad {
    const int32_t* clip_first;
    const int32_t* label_first;
    int block;
    __device__ pd::Long2 operator()(long c) const {
        const long n = clip_frames(clip_first, label_first, c);
        return pd::Long2{n, blocks_of(n, block)};
    }
};
struct ClipFirstStore {
    long* elem_first;
    long* block_first;
    __device__ void operator()(long c, pd::Long2 v) const {
        if (c == 0) elem_first[0] = 0, block_first[0] = 0;
        elem_first[c + 1] = v.a;
        block_first[c + 1] = v.b;
    }
};

// ---- counting within a wave, clip by clip ------------------------------------------------------------------------------------

// Every lane of the wave calls these.  clip: the lane's clip, -1 for a lane without an element; the lanes of a clip are a run.
struct WaveRuns {
    unsigned long long mine;   // the lanes of this lane's run
    bool first, last;          // this lane opens / closes its run (never for a lane without an element)
};
__device__ inline WaveRuns wave_runs(int clip) {
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(clip, 1, 64);
    const bool head = lane == 0 || before != clip;
    const unsigned long long heads = __ballot(head);
    const unsigned long long from = ~0ull << lane;                       // this lane and the ones above it
    const unsigned long long up_to = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // this lane and the ones below it
    const int start = 63 - __clzll(heads & up_to);                       // the head of this lane's run (lane 0 is always a head)
    const unsigned long long later = lane == 63 ? 0ull : (heads & (from << 1));   // heads above this lane
    const int end = later ? __ffsll((long long)later) - 1 : 64;          // one past the run's last lane
    WaveRuns r;
    r.mine = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & (~0ull << start);
    r.first = clip >= 0 && lane == start;
    r.last = clip >= 0 && lane == end - 1;
    return r;
}
__device__ inline void run_add_flag(const WaveRuns& r, long* counter, bool flag) {   // counter: the clip's slot
    const unsigned long long set = __ballot(flag) & r.mine;
    if (r.first && set) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(set));
}
__device__ inline void run_add(const WaveRuns& r, int clip, long* counter, long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long other = pd::shfl_up_words(v, d);
        const int other_clip = __shfl_up(clip, d, 64);
        if (lane >= d && other_clip == clip) v += other;   // (runs are contiguous: the same clip d lanes below is the same run)
    }
    if (r.last && v != 0) atomicAdd((unsigned long long*)counter, (unsigned long long)v);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

// (a) element e -> its clip, sort key, both predictions and label; NaN scores and labels above 1 counted per clip.  One element
// per lane and trip; every lane of a wave makes the same number of trips.
__global__ void frames_kernel(const float* __restrict__ probs, const int32_t* __restrict__ clip_first, const uint8_t* __restrict__ labels,
                              const int32_t* __restrict__ label_first, const long* __restrict__ elem_first, int C, long E, int W, float threshold,
                              int* __restrict__ elem_clip, uint32_t* __restrict__ keys, uint8_t* __restrict__ y, uint8_t* __restrict__ spred,
                              uint8_t* __restrict__ bpred, long* counters) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e0 = (long)blockIdx.x * blockDim.x; e0 < E; e0 += stride) {
        const long e = e0 + threadIdx.x;
        int c = -1;
        bool nan = false, bad = false;
        if (e < E) {
            c = pd::clip_of(elem_first, C, e);
            const long local = e - elem_first[c];
            const float* row = probs + ((long)clip_first[c] + local) * W;
            const float boosted = pd::row_mean(row, W), single = row[W / 2];
            bpred[e] = pd::above(boosted, threshold);
            spred[e] = pd::above(single, threshold);
            keys[e] = ed::key_of(boosted);
            const uint8_t l = labels[(long)label_first[c] + local];
            y[e] = l ? 1 : 0;
            elem_clip[e] = c;
            nan = ed::is_nan(boosted) || ed::is_nan(single);
            bad = l > 1;
        }
        const WaveRuns r = wave_runs(c);
        long* mine = counters + (long)(c < 0 ? 0 : c) * ed::COUNTERS;
        run_add_flag(r, mine + ed::C_NAN, nan);
        run_add_flag(r, mine + ed::C_BAD_LABEL, bad);
    }
}

// (d) the confusion and edge counts, per clip
__global__ void counts_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ spred, const uint8_t* __restrict__ bpred,
                              const int* __restrict__ elem_clip, const long* __restrict__ elem_first, long E, long* counters) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e0 = (long)blockIdx.x * blockDim.x; e0 < E; e0 += stride) {
        const long e = e0 + threadIdx.x;
        int c = -1;
        int acc[ed::FRAME_SLOTS];
#pragma unroll
        for (int s = 0; s < ed::FRAME_SLOTS; ++s) acc[s] = 0;
        if (e < E) {
            c = elem_clip[e];
            const long first = elem_first[c];
            ed::count_frame(y + first, spred + first, bpred + first, (int)(e - first), acc);
        }
        const WaveRuns r = wave_runs(c);
        long* mine = counters + (long)(c < 0 ? 0 : c) * ed::COUNTERS;
#pragma unroll
        for (int s = 0; s < ed::FRAME_SLOTS; ++s) run_add_flag(r, mine + ed::slot_counter(s), acc[s] != 0);
    }
}

// ---- radix sort, clip by clip ----------------------------------------------------------------------------------------------

// where sort block b lies: its clip, its elements [base, end) (end = the clip's), its column of the clip's share of the table
struct SortBlock {
    long base, end, first, table;   // first: the clip's first element; table: index of (digit 0, this block)
    long stride;                    // the clip's blocks: distance between two digits of the table
};
__device__ inline SortBlock sort_block(const long* elem_first, const long* block_first, int C, int block, long b) {
    const int c = pd::clip_of(block_first, C, b);
    const long lb = b - block_first[c];
    SortBlock s;
    s.first = elem_first[c];
    s.base = s.first + lb * block;
    s.end = elem_first[c + 1];
    s.stride = block_first[c + 1] - block_first[c];
    s.table = (long)ed::RADIX * block_first[c] + lb;
    return s;
}

// ed::sort_hist_kernel for sort block blockIdx.x of the batch
__global__ void __launch_bounds__(ed::SORT_THREADS) sort_hist_kernel(const uint32_t* __restrict__ keys, const long* __restrict__ elem_first,
                                                                     const long* __restrict__ block_first, int C, int shift, int block,
                                                                     unsigned* __restrict__ table) {
    __shared__ unsigned hist[ed::RADIX];
    for (int d = threadIdx.x; d < ed::RADIX; d += blockDim.x) hist[d] = 0;
    __syncthreads();
    const SortBlock s = sort_block(elem_first, block_first, C, block, blockIdx.x);
    for (int j = threadIdx.x; j < block; j += blockDim.x)
        if (s.base + j < s.end) atomicAdd(&hist[(keys[s.base + j] >> shift) & (ed::RADIX - 1)], 1u);
    __syncthreads();
    for (int d = threadIdx.x; d < ed::RADIX; d += blockDim.x) table[s.table + (long)d * s.stride] = hist[d];
}

// ed::sort_scatter_kernel for sort block blockIdx.x of the batch: the same ranking; the block's elements end at its clip's end, its
// column of the table is the clip's, and a position outside the clip is not written
__global__ void __launch_bounds__(ed::SORT_THREADS) sort_scatter_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labels,
                                                                        const long* __restrict__ elem_first, const long* __restrict__ block_first,
                                                                        int C, int shift, int block, const unsigned* __restrict__ table,
                                                                        uint32_t* __restrict__ keys_out, uint8_t* __restrict__ labels_out) {
    __shared__ uint16_t count[ed::SORT_VWAVES_MAX * ed::RADIX];   // [round * waves + wave][digit]: a wave's count, then the count of the rows before it
    __shared__ unsigned first[ed::RADIX];                         // where the workgroup's first element of a digit goes
    const int threads = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = threads >> 6;
    const int rounds = block / threads, rows = rounds * waves;
    const SortBlock s = sort_block(elem_first, block_first, C, block, blockIdx.x);
    for (int j = threadIdx.x; j < rows * ed::RADIX; j += threads) count[j] = 0;
    __syncthreads();
    uint32_t key[ed::SORT_ROUNDS_MAX];
    int rank[ed::SORT_ROUNDS_MAX];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < ed::SORT_ROUNDS_MAX; ++k) {
        if (k < rounds) {   // (uniform over the workgroup: every lane of a wave takes part in the ballots)
            const long idx = s.base + (long)k * threads + threadIdx.x;
            const bool valid = idx < s.end;
            key[k] = valid ? keys[idx] : 0u;
            const int d = (key[k] >> shift) & (ed::RADIX - 1);
            unsigned long long peers = __ballot(valid);   // the valid lanes of this wave with this lane's digit
#pragma unroll
            for (int bit = 0; bit < ed::RADIX_BITS; ++bit) {
                const bool set = (d >> bit) & 1;
                const unsigned long long with = __ballot(set);
                peers &= set ? with : ~with;
            }
            rank[k] = __popcll(peers & below);
            if (valid && rank[k] == 0) count[(k * waves + wave) * ed::RADIX + d] = (uint16_t)__popcll(peers);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < ed::RADIX; d += threads) {
        unsigned run = 0;
        for (int r = 0; r < rows; ++r) {
            const unsigned c = count[r * ed::RADIX + d];
            count[r * ed::RADIX + d] = (uint16_t)run;
            run += c;
        }
        first[d] = table[s.table + (long)d * s.stride] - run;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ed::SORT_ROUNDS_MAX; ++k) {
        if (k < rounds) {
            const long idx = s.base + (long)k * threads + threadIdx.x;
            if (idx < s.end) {
                const int d = (key[k] >> shift) & (ed::RADIX - 1);
                const long pos = (long)first[d] + count[(k * waves + wave) * ed::RADIX + d] + rank[k];
                if (pos >= s.first && pos < s.end) {
                    keys_out[pos] = key[k];
                    labels_out[pos] = labels[idx];
                }
            }
        }
    }
}

// entries of the digit table at the SMALLEST block, from the host tables (so that the knob never outgrows a workspace)
inline long sort_table_elems(const int32_t* clip_first_host, const int32_t* label_first_host, int C) {
    long blocks = 0;
    for (int c = 0; c < C; ++c) blocks += blocks_of(clip_frames(clip_first_host, label_first_host, c), pd::SCAN_BLOCK_MIN);
    return (long)ed::RADIX * blocks;
}

// every clip's (keys_a, labels_in) sorted by key among themselves, stably, into (keys_a, labels_a); `blocks`: the sort blocks of
// all clips at `block`.  Launches only.
inline void sort_run(hipStream_t st, long blocks, int block, const long* elem_first, const long* block_first, int C, uint32_t* keys_a, uint32_t* keys_b,
                     const uint8_t* labels_in, uint8_t* labels_a, uint8_t* labels_b, unsigned* table, unsigned* sums) {
    if (blocks <= 0) return;
    const int threads = block < ed::SORT_THREADS ? block : ed::SORT_THREADS;
    for (int pass = 0; pass < ed::PASSES; ++pass) {
        const uint32_t* kin = pass % 2 ? keys_b : keys_a;
        uint32_t* kout = pass % 2 ? keys_a : keys_b;
        const uint8_t* lin = pass == 0 ? labels_in : (pass % 2 ? labels_b : labels_a);
        uint8_t* lout = pass % 2 ? labels_a : labels_b;
        const int shift = pass * ed::RADIX_BITS;
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, kin, elem_first, block_first, C, shift, block, table);
        pd::scan_run<ed::OpSumU>(st, (long)ed::RADIX * blocks, block, pd::PtrLoad<unsigned>{table}, pd::PtrStore<unsigned>{table}, sums);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, kin, lin, elem_first, block_first, C, shift, block,
                           (const unsigned*)table, kout, lout);
    }
}

// ---- rank sum --------------------------------------------------------------------------------------------------------------

struct HeadNegLoad {   // ed::HeadNegLoad with a group head at every clip's first element
    const uint32_t* keys;
    const uint8_t* labels;
    const int* elem_clip;
    __device__ ed::HeadNeg operator()(long i) const {
        const bool head = i == 0 || elem_clip[i] != elem_clip[i - 1] || keys[i] != keys[i - 1];
        return ed::HeadNeg{head ? (int)i : -1, labels[i] ? 0 : 1};
    }
};

// every group's term, at its last element, onto its clip's counter; the negatives in front of the clip do not count
__global__ void u2_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labels, const ed::HeadNeg* __restrict__ scan,
                          const int* __restrict__ elem_clip, const long* __restrict__ elem_first, long E, long* counters) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e0 = (long)blockIdx.x * blockDim.x; e0 < E; e0 += stride) {
        const long i = e0 + threadIdx.x;
        int c = -1;
        long term = 0;
        if (i < E) {
            c = elem_clip[i];
            const long first = elem_first[c];
            if (i == E - 1 || elem_clip[i + 1] != c || keys[i + 1] != keys[i]) {
                const long head = scan[i].head;
                if (head >= first && head <= i) {
                    const long in_front = first > 0 ? scan[first - 1].neg : 0;
                    const long before = scan[head].neg - (labels[head] ? 0 : 1), q = scan[i].neg - before;
                    term = ed::u2_term((i - head + 1) - q, q, before - in_front);
                }
            }
        }
        const WaveRuns r = wave_runs(c);
        run_add(r, c, counters + (long)(c < 0 ? 0 : c) * ed::COUNTERS + ed::C_U2, term);
    }
}

// ---- boundaries ------------------------------------------------------------------------------------------------------------

struct BoundaryLoad {   // ed::BoundaryLoad on the element's own clip
    const uint8_t* y;
    const int* elem_clip;
    const long* elem_first;
    __device__ pd::Long2 operator()(long e) const {
        const int c = elem_clip[e];
        const long first = elem_first[c];
        const int n = (int)(elem_first[c + 1] - first);
        return pd::Long2{ed::is_start(y + first, (int)(e - first)) ? 1 : 0, ed::is_end(y + first, (int)(e - first), n) ? 1 : 0};
    }
};
// the k-th start / end of the batch writes its counts into record k of a `cap`-record buffer
struct BoundaryStore {
    BoundaryLoad flags;
    const uint8_t* spred;
    const uint8_t* bpred;
    int L;
    uint8_t* seg;
    long cap;
    __device__ void operator()(long e, pd::Long2 v) const {
        const pd::Long2 f = flags(e);
        if (!f.a && !f.b) return;
        const int c = flags.elem_clip[e];
        const long first = flags.elem_first[c];
        const int n = (int)(flags.elem_first[c + 1] - first), i = (int)(e - first);
        const uint8_t* y = flags.y + first;
        if (f.a && v.a - 1 < cap) {
            uint8_t* r = seg + (v.a - 1) * ed::SEG_BYTES;
            ed::start_counts(y, spred + first, i, n, L, r + 0, r + 1);
            ed::start_counts(y, bpred + first, i, n, L, r + 4, r + 5);
        }
        if (f.b && v.b - 1 < cap) {
            uint8_t* r = seg + (v.b - 1) * ed::SEG_BYTES;
            ed::end_counts(y, spred + first, i, L, r + 2, r + 3);
            ed::end_counts(y, bpred + first, i, L, r + 6, r + 7);
        }
    }
};

#undef SAVAD_HD

}  // namespace evalbatch
}  // namespace savad
