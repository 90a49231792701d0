// savad_post_device.h -- the post-processing of the predict path on the DEVICE: per-frame probabilities [N, W] -> boosted mean ->
// threshold -> trim -> sample classes -> segments (-> optimal split), and the per-sample probabilities of return_probs.  An
// alternative to the host functions of savad_post.h with THEIR results, bit for bit; what returns to the host is a segment
// count and count x 2 sample indices.
//
// The arithmetic is stated once, as __host__ __device__ inlines (first half of this file): the kernels (second half) and the
// host twins the CPU suite calls (savad_post_frames_host, savad_post_sample_class_host) run the same code.
//
// Row mean: numpy's float32 mean(axis=1) of a C-contiguous matrix = its pairwise sum of a row (eight accumulators for 8 <= W
// <= 128, left to right below 8), divided by float(W).  Only adds and one IEEE division: nothing to contract or re-associate.
//
// Trim: each of the reference's three passes reads a snapshot and only writes, so a pass is a function of the snapshot:
// with rise[i] = s[i-1]==0 && s[i]==1 and fall[i] = s[i-1]==1 && s[i]==0 (i >= 1), "last edge <= i" is a prefix max and "first
// edge > i" a suffix min of edge indices, and a frame's new value follows from those two and its old value.
//
// Samples: frame f covers sample i iff (long)(f*hop) <= i < (long)(f*hop + win).  The device path takes geometries whose hop is a
// whole number of samples (>= 1) with (n-1)*hop + win < 2^52 only: then the reference's repeated `start += hop` is f*hop
// exactly, and a contracted fma(f, hop, win) rounds as the two-step expression does.  A sample finds its highest candidate
// frame by integer division and walks down while the exact predicate holds.
//
// Segments: "is_voice before sample i" = the last non-MID class before i is ONE = a scan under combine(a, b) = b != MID ? b : a;
// the output slots are prefix sums of the start and of the end flags, so the output is sorted with no atomic append.
//
// Scans: ONE generic reduce-then-scan over workgroup-sized blocks (block reduce; the block sums scanned by the same routine
// until one block is left; block scan with the carry).  THE ONLY ORDERING BETWEEN WORKGROUPS IS THE BOUNDARY BETWEEN
// LAUNCHES: no kernel waits on, polls or spins for another workgroup.  Within a wave: 64-lane shuffles.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

namespace savad {
namespace postdev {

#define SAVAD_HD __host__ __device__ inline

constexpr int W_MAX = 128;                 // numpy's pairwise sum recurses above 128 elements: another order
constexpr uint8_t ZERO = 0, ONE = 1, MID = 2;   // class of a sample
constexpr int SCAN_BLOCK_DEFAULT = 2048;   // elements per workgroup block of the scans: 256 lanes x 8
constexpr int SCAN_BLOCK_MIN = 64;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS_MAX = SCAN_BLOCK_DEFAULT / SCAN_THREADS;
constexpr int ARGMIN_GRID = 1024;          // workgroups (at most) of the range argmin's first stage

// ---- arithmetic shared by host and device ---------------------------------------------------------------------------------

SAVAD_HD float div_f32(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// numpy float32 mean of a contiguous row of W <= 128 elements
SAVAD_HD float row_mean(const float* a, int W) {
#pragma clang fp contract(off)
    float s;
    if (W < 8) {
        s = a[0];
        for (int i = 1; i < W; ++i) s = s + a[i];
    } else {
        float r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
        const int full = W - W % 8;
        int i = 8;
        for (; i < full; i += 8) {
            r0 = r0 + a[i + 0];
            r1 = r1 + a[i + 1];
            r2 = r2 + a[i + 2];
            r3 = r3 + a[i + 3];
            r4 = r4 + a[i + 4];
            r5 = r5 + a[i + 5];
            r6 = r6 + a[i + 6];
            r7 = r7 + a[i + 7];
        }
        s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < W; ++i) s = s + a[i];
    }
    return div_f32(s, (float)W);
}

SAVAD_HD uint8_t above(float boosted, float threshold) { return boosted > threshold ? 1 : 0; }

// edge index of frame i: i where the edge is, `none` elsewhere.  kind 0 = rising (0 -> 1), 1 = falling (1 -> 0)
SAVAD_HD int edge_index(const uint8_t* s, int i, int kind, int none) {
    if (i < 1) return none;
    const uint8_t before = kind ? 1 : 0, after = kind ? 0 : 1;
    return (s[i - 1] == before && s[i] == after) ? i : none;
}

// one trim pass for frame i.  last = the last edge <= i of the pass's first kind (-1: none), next = the first edge > i of its
// second kind (INT_MAX: none).  pass 0 = valley (fall, rise), 1 = hill (rise, fall), 2 = hang (fall, rise).
SAVAD_HD uint8_t trim_pass_value(int pass, uint8_t s, int i, int last, int next, int min_vally, int min_hill, int hang_before, int hang_over) {
    const bool has_last = last >= 0, has_next = next != INT_MAX;
    if (pass == 0) return (s == 0 && has_last && has_next && next - last < min_vally) ? 1 : s;
    if (pass == 1) return (s == 1 && has_last && has_next && next - last < min_hill) ? 0 : s;
    return ((has_next && next - i <= hang_before) || (has_last && i - last < hang_over)) ? 1 : s;
}

struct Geometry {
    double hop, win;   // samples
    long hop_l;        // hop as an integer (the device path takes whole hops only)
    long num;          // samples of n frames: (long)((n-1)*hop + win), never negative
    int n;             // frames
};

SAVAD_HD Geometry make_geometry(int n, int sample_rate, double hop_ms, double window_ms) {
    Geometry g;
    g.hop = sample_rate * hop_ms / 1000;
    g.win = sample_rate * window_ms / 1000;
    g.hop_l = (long)g.hop;
    const long num = (long)((n - 1) * g.hop + g.win);
    g.num = num > 0 ? num : 0;
    g.n = n;
    return g;
}

// does frame f cover sample i?  (the reference's slice [int(start), int(start + win)) with start = f * hop)
SAVAD_HD bool covers(const Geometry& g, long f, long i) { return (long)((double)f * g.hop) <= i && i < (long)((double)f * g.hop + g.win); }

// the covering frames of sample i are [*first, *first + count): candidates by arithmetic, each confirmed with the exact predicate
SAVAD_HD int cover_of(const Geometry& g, long i, long* first) {
    long hi = i / g.hop_l;
    if (hi > g.n - 1) hi = g.n - 1;
    long lo = hi + 1;
    while (lo - 1 >= 0 && covers(g, lo - 1, i)) --lo;
    *first = lo;
    return (int)(hi + 1 - lo);
}

// value of sample i of convert_frames_to_samples(x): the covering frames summed in ascending order in double / their number
SAVAD_HD double sample_value(const float* x, const Geometry& g, long i) {
    long first;
    const int count = cover_of(g, i, &first);
    double s = 0.0;
    for (int k = 0; k < count; ++k) s = s + (double)x[first + k];
    return s / (count == 0 ? 1.0 : (double)count);
}

// class of sample i for 0/1 frames: ONE where the value is 1.0, ZERO where it is 0.0, MID otherwise
SAVAD_HD uint8_t sample_class(const uint8_t* frames, const Geometry& g, long i) {
    long first;
    const int count = cover_of(g, i, &first);
    int ones = 0;
    for (int k = 0; k < count; ++k) ones += frames[first + k] ? 1 : 0;
    if (ones == 0) return ZERO;
    return ones == count ? ONE : MID;
}

// the conditions of the device path (savad_post_supported)
inline bool geometry_supported(int sample_rate, double hop_ms, double window_ms, int n_frames) {
    if (sample_rate <= 0 || n_frames < 0 || !(hop_ms > 0) || !(window_ms > 0)) return false;
    const double hop = sample_rate * hop_ms / 1000, win = sample_rate * window_ms / 1000;
    if (!(hop >= 1.0) || !(hop < 4503599627370496.0) || hop != (double)(long)hop) return false;
    const double span = (n_frames > 0 ? (double)(n_frames - 1) : 0.0) * hop + win;
    return span < 4503599627370496.0;   // 2^52
}

// ---- host twins ------------------------------------------------------------------------------------------------------------

// the trim passes in a plain loop over the same inlines; s: n values in {0, 1}, edited in place; last / next: n ints of scratch
inline void trim_host(uint8_t* s, int n, int min_vally, int min_hill, int hang_before, int hang_over, int* last, int* next) {
    for (int pass = 0; pass < 3; ++pass) {
        if ((pass == 0 && min_vally <= 0) || (pass == 1 && min_hill <= 0) || (pass == 2 && hang_before <= 0)) continue;
        const int k_last = pass == 1 ? 0 : 1, k_next = pass == 1 ? 1 : 0;
        int run = -1;
        for (int i = 0; i < n; ++i) {
            const int e = edge_index(s, i, k_last, -1);
            run = e > run ? e : run;
            last[i] = run;
        }
        run = INT_MAX;
        for (int i = n - 1; i >= 0; --i) {   // next[i] = first edge > i
            next[i] = run;
            const int e = edge_index(s, i, k_next, INT_MAX);
            run = e < run ? e : run;
        }
        for (int i = 0; i < n; ++i) s[i] = trim_pass_value(pass, s[i], i, last[i], next[i], min_vally, min_hill, hang_before, hang_over);
    }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

__global__ void frames_kernel(const float* __restrict__ probs, int N, int W, float threshold, float* __restrict__ boosted, uint8_t* __restrict__ s) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const float m = row_mean(probs + i * W, W);
        boosted[i] = m;
        s[i] = above(m, threshold);
    }
}

// s[i] <- its value after one trim pass; last[i] = last edge <= i, next_incl[i] = first edge >= i (so "first edge > i" = next_incl[i + 1])
__global__ void trim_apply_kernel(uint8_t* s, int N, int pass, const int* __restrict__ last, const int* __restrict__ next_incl, int min_vally,
                                  int min_hill, int hang_before, int hang_over) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const int next = i + 1 < N ? next_incl[i + 1] : INT_MAX;
        s[i] = trim_pass_value(pass, s[i], (int)i, last[i], next, min_vally, min_hill, hang_before, hang_over);
    }
}

__global__ void sample_class_kernel(const uint8_t* __restrict__ frames, Geometry g, uint8_t* __restrict__ cls) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g.num; i += (long)gridDim.x * blockDim.x) cls[i] = sample_class(frames, g, i);
}

__global__ void sample_probs_kernel(const float* __restrict__ boosted, Geometry g, double* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g.num; i += (long)gridDim.x * blockDim.x) out[i] = sample_value(boosted, g, i);
}

// class ZERO at every break of the optimal split
__global__ void breaks_kernel(const long* __restrict__ breaks, int n_breaks, long num, uint8_t* cls) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_breaks && breaks[k] >= 0 && breaks[k] < num) cls[breaks[k]] = ZERO;
}

// ---- generic scan ----------------------------------------------------------------------------------------------------------

struct Long2 {
    long a, b;
};

struct OpMax {   // prefix max of edge indices (-1: none so far)
    typedef int T;
    __device__ static T identity() { return -1; }
    __device__ static T combine(T a, T b) { return a > b ? a : b; }
};
struct OpMin {   // (suffix) min of edge indices (INT_MAX: none)
    typedef int T;
    __device__ static T identity() { return INT_MAX; }
    __device__ static T combine(T a, T b) { return a < b ? a : b; }
};
struct OpLast {   // the last non-MID class: associative, not commutative
    typedef int T;
    __device__ static T identity() { return MID; }
    __device__ static T combine(T a, T b) { return b != MID ? b : a; }
};
struct OpSum2 {   // two long sums at once: the start flags and the end flags
    typedef Long2 T;
    __device__ static T identity() { return Long2{0, 0}; }
    __device__ static T combine(T a, T b) { return Long2{a.a + b.a, a.b + b.b}; }
};

template <class T>
__device__ inline T shfl_up_words(T v, int delta) {   // a 64-lane __shfl_up of any value made of 32-bit words
    static_assert(sizeof(T) % 4 == 0, "whole words");
    int w[sizeof(T) / 4];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int j = 0; j < (int)(sizeof(T) / 4); ++j) w[j] = __shfl_up(w[j], delta, 64);
    memcpy(&v, w, sizeof(T));
    return v;
}

// in: this lane's own total, lanes in order.  Returns the combination of all EARLIER lanes' totals of the workgroup (identity for
// lane 0); *total = the whole workgroup's (valid in every lane).  Workgroups are whole waves: 64, 128 or 256 lanes.
template <class Op>
__device__ inline typename Op::T block_exclusive(typename Op::T own, typename Op::T* total) {
    typedef typename Op::T T;
    __shared__ T wave_total[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    T incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T other = shfl_up_words(incl, d);
        if (lane >= d) incl = Op::combine(other, incl);
    }
    if (lane == 63) wave_total[wave] = incl;
    T excl = shfl_up_words(incl, 1);
    if (lane == 0) excl = Op::identity();
    __syncthreads();
    T before = Op::identity(), all = Op::identity();
    for (int j = 0; j < waves; ++j) {
        if (j < wave) before = Op::combine(before, wave_total[j]);
        all = Op::combine(all, wave_total[j]);
    }
    *total = all;
    return Op::combine(before, excl);
}

// block b of `items * blockDim.x` consecutive elements -> sums[b]
template <class Op, class Load>
__global__ void scan_reduce_kernel(long n, int items, Load load, typename Op::T* __restrict__ sums) {
    typedef typename Op::T T;
    const long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * items;
    T acc = Op::identity();
    for (int k = 0; k < items; ++k)
        if (base + k < n) acc = Op::combine(acc, load(base + k));
    T total;
    block_exclusive<Op>(acc, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// inclusive scan of block b with the carry carry[b - 1] (the inclusive scan of the block sums; null: one block)
template <class Op, class Load, class Store>
__global__ void scan_block_kernel(long n, int items, Load load, const typename Op::T* __restrict__ carry, Store store) {
    typedef typename Op::T T;
    const long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * items;
    T v[SCAN_ITEMS_MAX];
    T acc = Op::identity();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS_MAX; ++k) {
        if (k < items && base + k < n) acc = Op::combine(acc, load(base + k));
        v[k] = acc;
    }
    T total;
    T before = block_exclusive<Op>(acc, &total);
    if (carry && blockIdx.x > 0) before = Op::combine(carry[blockIdx.x - 1], before);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS_MAX; ++k)
        if (k < items && base + k < n) store(base + k, Op::combine(before, v[k]));
}

template <class T>
struct PtrLoad {
    const T* p;
    __device__ T operator()(long i) const { return p[i]; }
};
template <class T>
struct PtrStore {
    T* p;
    __device__ void operator()(long i, T v) const { p[i] = v; }
};

// number of block sums all levels of a scan of n elements need, at the SMALLEST block (so that the knob never outgrows a workspace)
inline long scan_sums_elems(long n) {
    long total = 0;
    while (n > 1) {
        n = (n + SCAN_BLOCK_MIN - 1) / SCAN_BLOCK_MIN;
        total += n;
    }
    return total + 1;
}

// inclusive scan of load(0 .. n-1) under Op, results handed to store(i, value).  Launches only; `sums` holds scan_sums_elems(n).
template <class Op, class Load, class Store>
inline void scan_run(hipStream_t st, long n, int block, Load load, Store store, typename Op::T* sums) {
    typedef typename Op::T T;
    if (n <= 0) return;
    const int threads = block < SCAN_THREADS ? block : SCAN_THREADS, items = block / threads;
    const long blocks = (n + block - 1) / block;
    if (blocks == 1) {
        hipLaunchKernelGGL((scan_block_kernel<Op, Load, Store>), dim3(1), dim3(threads), 0, st, n, items, load, (const T*)nullptr, store);
        return;
    }
    hipLaunchKernelGGL((scan_reduce_kernel<Op, Load>), dim3((unsigned)blocks), dim3(threads), 0, st, n, items, load, sums);
    scan_run<Op>(st, blocks, block, PtrLoad<T>{sums}, PtrStore<T>{sums}, sums + blocks);   // the block sums, in place
    hipLaunchKernelGGL((scan_block_kernel<Op, Load, Store>), dim3((unsigned)blocks), dim3(threads), 0, st, n, items, load, (const T*)sums, store);
}

// ---- the scans' inputs and outputs -----------------------------------------------------------------------------------------

// element j of the edge scans.  Forward: the edge index of frame j (-1: none).  Reverse (for the suffix min): of frame n-1-j (INT_MAX: none)
struct EdgeLoad {
    const uint8_t* s;
    int n, kind, reverse;
    __device__ int operator()(long j) const { return edge_index(s, reverse ? n - 1 - (int)j : (int)j, kind, reverse ? INT_MAX : -1); }
};
struct EdgeStore {
    int* out;
    int n, reverse;
    __device__ void operator()(long j, int v) const { out[reverse ? n - 1 - j : j] = v; }
};

struct ClassLoad {
    const uint8_t* cls;
    __device__ int operator()(long i) const { return cls[i]; }
};
struct ClassStore {
    uint8_t* state;
    __device__ void operator()(long i, int v) const { state[i] = (uint8_t)v; }
};

// start / end flags of sample i in [0, num]: state[i] = the last non-MID class up to and including i.  Element `num` is the
// end of a segment still open after the last sample.
struct FlagLoad {
    const uint8_t* cls;
    const uint8_t* state;
    long num;
    __device__ Long2 operator()(long i) const {
        const bool voice = i > 0 && state[i - 1] == ONE;
        if (i == num) return Long2{0, voice ? 1 : 0};
        const uint8_t c = cls[i];
        return Long2{(c == ONE && !voice) ? 1 : 0, (c == ZERO && voice) ? 1 : 0};
    }
};
// scatter: the k-th start / end goes to slot k - first of a `cap`-slot buffer; the totals to totals[0..1]
struct SegmentStore {
    FlagLoad flags;
    long* starts;
    long* ends;
    long first, cap;
    long* totals;
    __device__ void operator()(long i, Long2 v) const {
        const Long2 f = flags(i);
        if (f.a) {
            const long k = v.a - 1 - first;
            if (k >= 0 && k < cap) starts[k] = i;
        }
        if (f.b) {
            const long k = v.b - 1 - first;
            if (k >= 0 && k < cap) ends[k] = i - 1;
        }
        if (i == flags.num) {
            totals[0] = v.a;
            totals[1] = v.b;
        }
    }
};

// ---- range argmin ----------------------------------------------------------------------------------------------------------

struct MinKey {
    double value;
    long index;
};

__device__ inline MinKey min_key(MinKey a, MinKey b) {   // the lower index wins ties (np.argmin: the first minimum)
    if (b.index < 0) return a;
    if (a.index < 0) return b;
    if (b.value < a.value || (b.value == a.value && b.index < a.index)) return b;
    return a;
}

__device__ inline MinKey block_min_key(MinKey k) {
    __shared__ MinKey wave_min[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const MinKey other = shfl_up_words(k, d);
        if (lane >= d) k = min_key(k, other);
    }
    if (lane == 63) wave_min[wave] = k;
    __syncthreads();
    MinKey best = wave_min[0];
    for (int j = 1; j < waves; ++j) best = min_key(best, wave_min[j]);
    return best;
}

// stage 1: every workgroup's minimum of value(i; boosted) over its share of [a, b)
__global__ void argmin_stage1_kernel(const float* __restrict__ boosted, Geometry g, long a, long b, MinKey* __restrict__ partial) {
    MinKey k{0.0, -1};
    for (long i = a + (long)blockIdx.x * blockDim.x + threadIdx.x; i < b; i += (long)gridDim.x * blockDim.x)
        k = min_key(k, MinKey{sample_value(boosted, g, i), i});
    k = block_min_key(k);
    if (threadIdx.x == 0) partial[blockIdx.x] = k;
}

// stage 2: one workgroup over the partial minima
__global__ void argmin_stage2_kernel(const MinKey* __restrict__ partial, int n, MinKey* __restrict__ out) {
    MinKey k{0.0, -1};
    for (int i = threadIdx.x; i < n; i += blockDim.x) k = min_key(k, partial[i]);
    k = block_min_key(k);
    if (threadIdx.x == 0) *out = k;
}

#undef SAVAD_HD

}  // namespace postdev
}  // namespace savad
