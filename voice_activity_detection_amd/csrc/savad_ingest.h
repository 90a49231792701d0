// savad_ingest.h -- audio ingest on the device: what AudioData.load does on the host before the first feature
// (vad/data_models/audio_data.py:18-34): channel average (:26) and librosa.resample(audio, sr, 16000, res_type="kaiser_fast")
// (:27-30) = resampy 0.2.x core.resample / interpn.resample_f with the "kaiser_fast" filter, then librosa's fix_length.
//
// Resampler: ONE LANE PER OUTPUT SAMPLE, walking the taps in resampy's order (left wing x[n], x[n-1], ..., then right wing
// x[n+1], x[n+2], ...) with resampy's arithmetic: the weight  win[idx] + eta * delta[idx]  and the product  weight * x  in
// float64, the accumulator rounded to float32 after every tap.  Nothing is re-associated and no multiply-add is contracted
// (plain operators under `#pragma clang fp contract(off)`: hipcc contracts device code by default, and the __dmul_rn / __dadd_rn
// wrappers are themselves compiled contractable, so after inlining they fuse all the same), so an output sample has the bits of resampy's loop.
//
// Layout: a workgroup of BLOCK lanes owns BLOCK consecutive outputs; their taps read one contiguous input span of
// about BLOCK * rate / 16000 + 2 * taps samples, staged in LDS as float32.  The filter's half window (8193 float64 entries,
// scaled by the ratio when downsampling) is kept in LDS next to it, interleaved with its first differences as
// (win[i], delta[i]) pairs of 16 bytes: one ds_read_b128 per tap.  A workgroup loads the table once and then walks blocks
// of outputs (grid-stride), so the 128 KiB of table traffic per workgroup is paid once.  128 KiB + span <= 160 KiB bounds
// the source rate (RATE_MAX).  TABLE_IN_LDS = false reads the pairs through the cache instead (the A/B of
// scripts/ubench/ingest_bench.py).
//
// Time register: resampy advances it by repeated float64 addition (time_register += 1 / ratio), and  k * increment  is
// NOT that value.  But while t stays inside one binade [2^e, 2^(e+1)) and the increment c is not exactly half way between
// two multiples of ulp(t), every addition moves t by the same exactly representable amount  s = fl(t + c) - t  (c rounded to
// a multiple of ulp(t)), so  t_k = t_0 + (k - k_0) * s  holds exactly (product and sum are multiples of ulp(t) below
// 2^53 ulp(t): no rounding).  time_segments() walks the binades on the host -- one true addition at every binade crossing
// and for every step inside a tie binade -- and yields a few dozen (k_0, t_0, s) segments; a lane finds its segment by
// binary search.  No per-sample array of times exists anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "savad_audio_host.h"   // constants, Seg, Plan, time_segments: pure host code

namespace savad {
namespace ingest {

__device__ inline double seg_time(const Seg* __restrict__ segs, int nseg, long long k) {
#pragma clang fp contract(off)
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].k0 <= k) lo = mid; else hi = mid;
    }
    return segs[lo].t0 + (double)(k - segs[lo].k0) * segs[lo].s;  // exact: see the head of this file
}

// outputs [o0, o0 + count) of the resampled signal; x points at input sample in_first and holds in_count samples (every
// sample the span reads and the signal has must be inside: checked on the host); outputs at or past n_out are zero
// (librosa's fix_length).  tab: NWIN (win, delta) pairs.
template <bool TABLE_IN_LDS>
__global__ __launch_bounds__(BLOCK) void resample_kernel(const float* __restrict__ x, long long in_first, long long in_count, long long n_in,
                                                         long long o0, long long count, long long n_out,
                                                         const double2* __restrict__ tab, const Seg* __restrict__ segs, int nseg,
                                                         double scale, int step, int taps, int span_cap, float* __restrict__ y) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double2* const ltab = reinterpret_cast<double2*>(lds);
    float* const xs = reinterpret_cast<float*>(lds + (TABLE_IN_LDS ? (size_t)NWIN * 16 : 0));
    const int tid = threadIdx.x;
    if (TABLE_IN_LDS)
        for (int i = tid; i < NWIN; i += BLOCK) ltab[i] = tab[i];
    const double2* const w = TABLE_IN_LDS ? ltab : tab;
    const long long o1 = o0 + count;
    const long long blocks = (count + BLOCK - 1) / BLOCK;
    for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
        const long long kb = o0 + b * BLOCK;
        long long ke = kb + BLOCK < o1 ? kb + BLOCK : o1;  // this pass's outputs: [kb, ke)
        const long long kc = ke < n_out ? ke : n_out;      // ... of which [kb, kc) are computed
        long long lo = 0;
        __syncthreads();  // the table is in place / the previous pass has finished with xs
        if (kc > kb) {
            const long long n_first = (long long)seg_time(segs, nseg, kb), n_last = (long long)seg_time(segs, nseg, kc - 1);
            lo = n_first - taps + 1;
            long long len = n_last + taps + 1 - lo;
            if (len > span_cap) len = span_cap;  // (never: span_cap is the bound of plan_for)
            for (int j = tid; j < (int)len; j += BLOCK) {
                const long long g = lo + j, r = g - in_first;
                xs[j] = (g >= 0 && g < n_in && r >= 0 && r < in_count) ? x[r] : 0.0f;
            }
        }
        __syncthreads();
        const long long k = kb + tid;
        if (k >= ke) continue;
        float acc = 0.0f;
        if (k < kc) {
            const double t = seg_time(segs, nseg, k);
            const long long n = (long long)t;
            double frac = scale * (t - (double)n);
            double index_frac = frac * (double)NUM_TABLE;
            int offset = (int)index_frac;
            double eta = index_frac - (double)offset;
            long long lim = (NWIN - offset) / step;
            int i_max = (int)(n + 1 < lim ? n + 1 : lim);
            const float* xl = xs + (n - lo);
            for (int i = 0; i < i_max; ++i) {  // left wing
                const double2 e = w[offset + i * step];
                const double weight = e.x + eta * e.y;
                acc = (float)((double)acc + weight * (double)xl[-i]);
            }
            frac = scale - frac;
            index_frac = frac * (double)NUM_TABLE;
            offset = (int)index_frac;
            eta = index_frac - (double)offset;
            lim = (NWIN - offset) / step;
            const long long room = n_in - n - 1;
            const int k_max = (int)(room < lim ? room : lim);
            for (int i = 0; i < k_max; ++i) {  // right wing
                const double2 e = w[offset + i * step];
                const double weight = e.x + eta * e.y;
                acc = (float)((double)acc + weight * (double)xl[i + 1]);
            }
        }
        y[k - o0] = acc;
    }
}

// interleaved [n_frames][C] int16 or float32 -> float32 mono with the bits of the host loader: sample / 32768 for int16, then
// numpy's .reshape(-1, C).mean(axis=1) in float32 = the left-to-right float32 sum divided by float32(C) (numpy adds a row of
// fewer than 8 elements in order; int16 sources: every partial sum of up to 256 values k / 32768 is exact, any order gives
// the same bits).
template <typename T>
__device__ inline float ingest_sample(T v);
template <>
__device__ inline float ingest_sample<short>(short v) { return (float)v * (1.0f / 32768.0f); }
template <>
__device__ inline float ingest_sample<float>(float v) { return v; }

template <typename T>
__global__ void downmix_kernel(const T* __restrict__ raw, int C, long long n_frames, float* __restrict__ mono) {
#pragma clang fp contract(off)
    const float fc = (float)C;
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_frames; f += (long long)gridDim.x * blockDim.x) {
        const T* p = raw + f * C;
        float s = ingest_sample<T>(p[0]);
        for (int c = 1; c < C; ++c) s = s + ingest_sample<T>(p[c]);
        mono[f] = __fdiv_rn(s, fc);
    }
}

}  // namespace ingest
}  // namespace savad
