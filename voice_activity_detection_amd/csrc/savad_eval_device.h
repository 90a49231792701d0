// savad_eval_device.h -- the metrics of the evaluate command on the DEVICE: per-frame probabilities [N, W] + 0/1 labels -> the integers
// every one of evaluate.file_metrics' 18 values is a float64 expression of (metrics.metrics_from_counts): confusion counts, edge
// counts, a rank sum and per-boundary hit counts.  What returns to the host is a fixed block of int64 counters and 8 bytes per true
// segment; no float leaves the device, so the host expressions see the integers the numpy path sees and give its bits.
//
// The arithmetic is stated once, as __host__ __device__ inlines (first half of this file): the kernels (second half) and the host
// twin the CPU suite calls (savad_eval_counts_host) run the same code.  Row mean and threshold are savad_post_device.h's.
//
// Sort key: the float32 bits of a boosted score mapped to a uint32 whose unsigned order is the order of the values (sign bit
// flipped for positives, all bits for negatives); -0.0 is folded onto +0.0 first, because the host compares values.
//
// Sort: LSD radix, 8-bit digits, four passes, each stable.  A pass = a digit histogram per block of elements; the [256 x blocks]
// table scanned digit-major by savad_post_device.h's scan_run; a scatter in which a workgroup ranks its elements per digit: within
// a wave by a match loop over ballots, across the waves (and the rounds of a workgroup that holds several elements per lane) by an
// LDS table of per-wave digit counts.  A block's elements of one digit land next to each other, in their order.  Payload: the label.
//
// Rank sum: over the sorted pairs a group is a run of equal keys.  One scan carries (index of the last group head, negatives so
// far); at a group's last element that gives its negatives q, positives p and the negatives before it, and
// U2 = sum p * (2 * negatives_before + q) = 2 * (rank sum of the positives with mid-ranks - n_pos (n_pos + 1) / 2), an integer.
//
// Boundaries: a thread per frame; a start / end boundary of the labels reads its at most L + 1 neighbours directly; its output
// slot is its rank under OpSum2 over the start and end flags, so the output is in boundary order with no atomic append.
//
// Workgroups: as in savad_post_device.h THE ONLY ORDERING BETWEEN WORKGROUPS IS THE BOUNDARY BETWEEN LAUNCHES.  The counters are
// integer sums: every wave adds its share with one atomic add per counter, whose order does not matter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "savad_post_device.h"

namespace savad {
namespace evaldev {

namespace pd = savad::postdev;

#define SAVAD_HD __host__ __device__ inline

// slots of the counter block (include/savad.h: SAVAD_EVAL_*)
constexpr int C_N = 0, C_POS = 1, C_TRUE = 2, C_NAN = 3, C_BAD_LABEL = 4, C_U2 = 5, C_PRED = 6;
constexpr int P_TP = 0, P_FP = 1, P_FN = 2, P_TN = 3, P_NPRED = 4, PRED_STRIDE = 5;   // per prediction: 0 = single, 1 = boosted
constexpr int COUNTERS = C_PRED + 2 * PRED_STRIDE;
constexpr int FRAME_SLOTS = 2 + 2 * PRED_STRIDE;   // what count_frame adds to: C_POS, C_TRUE, then the two predictions' five
constexpr int SEG_BYTES = 8;                       // per true segment: (num_s, den_s, num_e, den_e) of single, then of boosted
constexpr int L_MAX = 254;                         // a denominator is at most L + 1 and travels in a byte

constexpr int RADIX = 256, RADIX_BITS = 8, PASSES = 4;
constexpr int SORT_BLOCK_DEFAULT = pd::SCAN_BLOCK_DEFAULT;   // elements per workgroup: 256 lanes x 8 rounds
constexpr int SORT_THREADS = pd::SCAN_THREADS;
constexpr int SORT_ROUNDS_MAX = SORT_BLOCK_DEFAULT / SORT_THREADS;
constexpr int SORT_VWAVES_MAX = SORT_BLOCK_DEFAULT / 64;     // (round, wave) pairs of a workgroup: rows of the LDS count table

// ---- arithmetic shared by host and device ---------------------------------------------------------------------------------

SAVAD_HD uint32_t key_of(float f) {
    uint32_t u = 0;   // +0.0 and -0.0
    if (!(f == 0.0f)) memcpy(&u, &f, sizeof(u));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

SAVAD_HD float key_value(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

SAVAD_HD bool is_nan(float f) { return f != f; }

SAVAD_HD int slot_counter(int slot) { return slot < 2 ? C_POS + slot : C_PRED + (slot - 2); }

// what frame i adds to the counters: acc[FRAME_SLOTS].  y, spred, bpred: 0 / 1
template <class Acc>
SAVAD_HD void count_frame(const uint8_t* y, const uint8_t* spred, const uint8_t* bpred, int i, Acc* acc) {
    const int t = y[i];
    acc[0] += t;
    acc[1] += (t && (i == 0 || !y[i - 1])) ? 1 : 0;
    for (int p = 0; p < 2; ++p) {
        const uint8_t* pred = p ? bpred : spred;
        const int v = pred[i];
        Acc* a = acc + 2 + p * PRED_STRIDE;
        a[P_TP] += (t && v) ? 1 : 0;
        a[P_FP] += (!t && v) ? 1 : 0;
        a[P_FN] += (t && !v) ? 1 : 0;
        a[P_TN] += (!t && !v) ? 1 : 0;
        a[P_NPRED] += (v && (i == 0 || !pred[i - 1])) ? 1 : 0;
    }
}

SAVAD_HD bool is_start(const uint8_t* y, int i) { return y[i] && (i == 0 || !y[i - 1]); }
SAVAD_HD bool is_end(const uint8_t* y, int i, int n) { return y[i] && (i == n - 1 || !y[i + 1]); }

// start boundary b: the frames [b, min(b + L, n)) and how many of them the prediction has right
SAVAD_HD void start_counts(const uint8_t* y, const uint8_t* pred, int b, int n, int L, uint8_t* num, uint8_t* den) {
    const int hi = (long)b + L < (long)n ? b + L : n;
    int m = 0;
    for (int j = b; j < hi; ++j) m += pred[j] == y[j] ? 1 : 0;
    *num = (uint8_t)m;
    *den = (uint8_t)(hi - b);
}

// end boundary e: the frames [max(e - L, 0), e]
SAVAD_HD void end_counts(const uint8_t* y, const uint8_t* pred, int e, int L, uint8_t* num, uint8_t* den) {
    const int lo = e - L > 0 ? e - L : 0;
    int m = 0;
    for (int j = lo; j <= e; ++j) m += pred[j] == y[j] ? 1 : 0;
    *num = (uint8_t)m;
    *den = (uint8_t)(e - lo + 1);
}

// a tie group of p positives and q negatives with neg_before negatives below it
SAVAD_HD long u2_term(long p, long q, long neg_before) { return p * (2 * neg_before + q); }

// ---- host twin -------------------------------------------------------------------------------------------------------------

// counters[COUNTERS] and up to seg_cap boundary records from host pointers; returns the number of true segments
inline long counts_host(const float* probs, int W, const uint8_t* labels, int n, float threshold, int L, long* counters, uint8_t* seg, long seg_cap) {
    std::vector<uint32_t> keys((size_t)n);
    std::vector<uint8_t> y((size_t)n), spred((size_t)n), bpred((size_t)n);
    for (int k = 0; k < COUNTERS; ++k) counters[k] = 0;
    counters[C_N] = n;
    for (int i = 0; i < n; ++i) {
        const float* row = probs + (size_t)i * W;
        const float boosted = pd::row_mean(row, W);
        bpred[i] = pd::above(boosted, threshold);
        spred[i] = pd::above(row[W / 2], threshold);
        keys[i] = key_of(boosted);
        y[i] = labels[i] ? 1 : 0;
        counters[C_NAN] += is_nan(boosted) || is_nan(row[W / 2]) ? 1 : 0;
        counters[C_BAD_LABEL] += labels[i] > 1 ? 1 : 0;
    }
    long acc[FRAME_SLOTS] = {0};
    for (int i = 0; i < n; ++i) count_frame(y.data(), spred.data(), bpred.data(), i, acc);
    for (int s = 0; s < FRAME_SLOTS; ++s) counters[slot_counter(s)] = acc[s];
    long n_start = 0, n_end = 0;
    for (int i = 0; i < n; ++i) {
        for (int p = 0; p < 2; ++p) {
            const uint8_t* pred = p ? bpred.data() : spred.data();
            if (is_start(y.data(), i) && n_start < seg_cap) start_counts(y.data(), pred, i, n, L, seg + n_start * SEG_BYTES + p * 4, seg + n_start * SEG_BYTES + p * 4 + 1);
            if (is_end(y.data(), i, n) && n_end < seg_cap) end_counts(y.data(), pred, i, L, seg + n_end * SEG_BYTES + p * 4 + 2, seg + n_end * SEG_BYTES + p * 4 + 3);
        }
        n_start += is_start(y.data(), i) ? 1 : 0;
        n_end += is_end(y.data(), i, n) ? 1 : 0;
    }
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] < keys[b]; });
    long u2 = 0, neg_before = 0;
    for (int lo = 0; lo < n;) {
        int hi = lo;
        long q = 0;
        while (hi < n && keys[order[hi]] == keys[order[lo]]) q += y[order[hi++]] ? 0 : 1;
        u2 += u2_term((hi - lo) - q, q, neg_before);
        neg_before += q;
        lo = hi;
    }
    counters[C_U2] = u2;
    return n_start;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

// the sum of v over the wave, valid in lane 0
__device__ inline long wave_sum(long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_down((int)(v & 0xffffffffL), d, 64), hi = __shfl_down((int)(v >> 32), d, 64);
        v += (long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}

__device__ inline void wave_add(long* counter, long v) {   // every lane of the wave calls it
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd((unsigned long long*)counter, (unsigned long long)v);
}

// (a) frame i -> sort key of the boosted score, both predictions, the label as 0 / 1; NaN scores and labels above 1 counted
__global__ void frames_kernel(const float* __restrict__ probs, int W, const uint8_t* __restrict__ labels, int n, float threshold,
                              uint32_t* __restrict__ keys, uint8_t* __restrict__ y, uint8_t* __restrict__ spred, uint8_t* __restrict__ bpred,
                              long* counters) {
    long nan = 0, bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float* row = probs + i * W;
        const float boosted = pd::row_mean(row, W), single = row[W / 2];
        bpred[i] = pd::above(boosted, threshold);
        spred[i] = pd::above(single, threshold);
        keys[i] = key_of(boosted);
        const uint8_t l = labels[i];
        y[i] = l ? 1 : 0;
        nan += is_nan(boosted) || is_nan(single) ? 1 : 0;
        bad += l > 1 ? 1 : 0;
    }
    wave_add(counters + C_NAN, nan);
    wave_add(counters + C_BAD_LABEL, bad);
}

// (d) the confusion and edge counts
__global__ void counts_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ spred, const uint8_t* __restrict__ bpred, int n, long* counters) {
    long acc[FRAME_SLOTS];
#pragma unroll
    for (int s = 0; s < FRAME_SLOTS; ++s) acc[s] = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) count_frame(y, spred, bpred, (int)i, acc);
#pragma unroll
    for (int s = 0; s < FRAME_SLOTS; ++s) wave_add(counters + slot_counter(s), acc[s]);
}

// savad_eval_sort: float keys <-> sort keys
__global__ void keys_kernel(const float* __restrict__ values, long n, uint32_t* __restrict__ keys) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) keys[i] = key_of(values[i]);
}
__global__ void values_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labels, long n, float* __restrict__ values,
                              uint8_t* __restrict__ labels_out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        values[i] = key_value(keys[i]);
        labels_out[i] = labels[i];
    }
}

// ---- radix sort ------------------------------------------------------------------------------------------------------------

struct OpSumU {   // the digit table's prefix sums: below 2^31 elements in all
    typedef unsigned T;
    __device__ static T identity() { return 0u; }
    __device__ static T combine(T a, T b) { return a + b; }
};

// workgroup b: the digit counts of elements [b * block, (b + 1) * block) -> table[digit * blocks + b]
__global__ void __launch_bounds__(SORT_THREADS) sort_hist_kernel(const uint32_t* __restrict__ keys, long n, int shift, int block, long blocks,
                                                                 unsigned* __restrict__ table) {
    __shared__ unsigned hist[RADIX];
    for (int d = threadIdx.x; d < RADIX; d += blockDim.x) hist[d] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * block;
    for (int j = threadIdx.x; j < block; j += blockDim.x)
        if (base + j < n) atomicAdd(&hist[(keys[base + j] >> shift) & (RADIX - 1)], 1u);
    __syncthreads();
    for (int d = threadIdx.x; d < RADIX; d += blockDim.x) table[(long)d * blocks + blockIdx.x] = hist[d];
}

// workgroup b scatters its elements; table = the INCLUSIVE digit-major prefix sums of the histograms.  Element order within the
// workgroup: round k, then wave, then lane (element index base + k * threads + thread: ascending), so a rank that counts the
// equal digits of earlier (round, wave) rows and of lower lanes is the stable one.
__global__ void __launch_bounds__(SORT_THREADS) sort_scatter_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labels, long n,
                                                                    int shift, int block, long blocks, const unsigned* __restrict__ table,
                                                                    uint32_t* __restrict__ keys_out, uint8_t* __restrict__ labels_out) {
    __shared__ uint16_t count[SORT_VWAVES_MAX * RADIX];   // [round * waves + wave][digit]: a wave's count, then the count of the rows before it
    __shared__ unsigned first[RADIX];                     // where the workgroup's first element of a digit goes
    const int threads = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = threads >> 6;
    const int rounds = block / threads, rows = rounds * waves;
    const long base = (long)blockIdx.x * block;
    for (int j = threadIdx.x; j < rows * RADIX; j += threads) count[j] = 0;
    __syncthreads();
    uint32_t key[SORT_ROUNDS_MAX];
    int rank[SORT_ROUNDS_MAX];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < SORT_ROUNDS_MAX; ++k) {
        if (k < rounds) {   // (uniform over the workgroup: every lane of a wave takes part in the ballots)
            const long idx = base + (long)k * threads + threadIdx.x;
            const bool valid = idx < n;
            key[k] = valid ? keys[idx] : 0u;
            const int d = (key[k] >> shift) & (RADIX - 1);
            unsigned long long peers = __ballot(valid);   // the valid lanes of this wave with this lane's digit
#pragma unroll
            for (int bit = 0; bit < RADIX_BITS; ++bit) {
                const bool set = (d >> bit) & 1;
                const unsigned long long with = __ballot(set);
                peers &= set ? with : ~with;
            }
            rank[k] = __popcll(peers & below);
            if (valid && rank[k] == 0) count[(k * waves + wave) * RADIX + d] = (uint16_t)__popcll(peers);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < RADIX; d += threads) {
        unsigned run = 0;
        for (int r = 0; r < rows; ++r) {
            const unsigned c = count[r * RADIX + d];
            count[r * RADIX + d] = (uint16_t)run;
            run += c;
        }
        first[d] = table[(long)d * blocks + blockIdx.x] - run;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SORT_ROUNDS_MAX; ++k) {
        if (k < rounds) {
            const long idx = base + (long)k * threads + threadIdx.x;
            if (idx < n) {
                const int d = (key[k] >> shift) & (RADIX - 1);
                const long pos = (long)first[d] + count[(k * waves + wave) * RADIX + d] + rank[k];
                if (pos < n) {
                    keys_out[pos] = key[k];
                    labels_out[pos] = labels[idx];
                }
            }
        }
    }
}

// elements of the digit table of a sort of n elements at the SMALLEST block (so that the knob never outgrows a workspace)
inline long sort_table_elems(long n) { return (long)RADIX * ((n + pd::SCAN_BLOCK_MIN - 1) / pd::SCAN_BLOCK_MIN); }

// (keys_a, labels_in) sorted by key, stably, into (keys_a, labels_a); keys_b / labels_b: the other side of the ping-pong.  labels_in
// is only read (it may be labels_a).  Launches only.
inline void sort_run(hipStream_t st, long n, int block, uint32_t* keys_a, uint32_t* keys_b, const uint8_t* labels_in, uint8_t* labels_a,
                     uint8_t* labels_b, unsigned* table, unsigned* sums) {
    if (n <= 0) return;
    const int threads = block < SORT_THREADS ? block : SORT_THREADS;
    const long blocks = (n + block - 1) / block;
    for (int pass = 0; pass < PASSES; ++pass) {
        const uint32_t* kin = pass % 2 ? keys_b : keys_a;
        uint32_t* kout = pass % 2 ? keys_a : keys_b;
        const uint8_t* lin = pass == 0 ? labels_in : (pass % 2 ? labels_b : labels_a);
        uint8_t* lout = pass % 2 ? labels_a : labels_b;
        const int shift = pass * RADIX_BITS;
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, kin, n, shift, block, blocks, table);
        pd::scan_run<OpSumU>(st, (long)RADIX * blocks, block, pd::PtrLoad<unsigned>{table}, pd::PtrStore<unsigned>{table}, sums);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, kin, lin, n, shift, block, blocks, (const unsigned*)table,
                           kout, lout);
    }
}

// ---- rank sum --------------------------------------------------------------------------------------------------------------

struct HeadNeg {
    int head, neg;   // index of the last group head so far (-1: none), negatives so far
};
struct OpHeadNeg {
    typedef HeadNeg T;
    __device__ static T identity() { return HeadNeg{-1, 0}; }
    __device__ static T combine(T a, T b) { return HeadNeg{a.head > b.head ? a.head : b.head, a.neg + b.neg}; }
};
struct HeadNegLoad {
    const uint32_t* keys;
    const uint8_t* labels;
    __device__ HeadNeg operator()(long i) const { return HeadNeg{(i == 0 || keys[i] != keys[i - 1]) ? (int)i : -1, labels[i] ? 0 : 1}; }
};

// every group's term, at its last element
__global__ void u2_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labels, const HeadNeg* __restrict__ scan, int n, long* counters) {
    long acc = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (i == n - 1 || keys[i + 1] != keys[i]) {
            const int head = scan[i].head;
            if (head >= 0 && head <= i) {
                const long neg_before = scan[head].neg - (labels[head] ? 0 : 1), q = scan[i].neg - neg_before;
                acc += u2_term((i - head + 1) - q, q, neg_before);
            }
        }
    }
    wave_add(counters + C_U2, acc);
}

// ---- boundaries ------------------------------------------------------------------------------------------------------------

struct BoundaryLoad {
    const uint8_t* y;
    int n;
    __device__ pd::Long2 operator()(long i) const { return pd::Long2{is_start(y, (int)i) ? 1 : 0, is_end(y, (int)i, n) ? 1 : 0}; }
};
// the k-th start / end writes its counts into record k of a `cap`-record buffer
struct BoundaryStore {
    BoundaryLoad flags;
    const uint8_t* spred;
    const uint8_t* bpred;
    int L;
    uint8_t* seg;
    long cap;
    __device__ void operator()(long i, pd::Long2 v) const {
        const pd::Long2 f = flags(i);
        if (f.a && v.a - 1 < cap) {
            uint8_t* r = seg + (v.a - 1) * SEG_BYTES;
            start_counts(flags.y, spred, (int)i, flags.n, L, r + 0, r + 1);
            start_counts(flags.y, bpred, (int)i, flags.n, L, r + 4, r + 5);
        }
        if (f.b && v.b - 1 < cap) {
            uint8_t* r = seg + (v.b - 1) * SEG_BYTES;
            end_counts(flags.y, spred, (int)i, L, r + 2, r + 3);
            end_counts(flags.y, bpred, (int)i, L, r + 6, r + 7);
        }
    }
};

#undef SAVAD_HD

}  // namespace evaldev
}  // namespace savad
