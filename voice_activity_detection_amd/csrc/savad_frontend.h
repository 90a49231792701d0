// savad_frontend.h -- the feature front-end for every transform a reference config can name
// (vad/acoustics/transforms/transform_factory.py:13-59, vad/acoustics/feature_extractor.py:122-147), with runtime geometry.
// savad_logmel.h keeps the tuned kernel of the one shipped geometry; this path is generic:
//
//   stft_kernel   DFT as one GEMM on the exact-fp32 MFMA (the rounds 1-4 design of mel::logmel_kernel): A operand = host-built
//                 window-folded cos / sin rows (re and im of a bin in adjacent rows: |X|^2 and |X| are lane-local), B operand =
//                 the frames' samples read from the reflect-padded signal (centred transforms) or the signal (spectrogram).
//                 The table's K range starts at the 4-aligned sample at or below the window's first one, with zero weights
//                 before it and after its end, so that every B read is one 16-byte load.  Power (mel / log-mel / mfcc) goes to
//                 a [frames][bins] workspace, magnitude (spectrogram) straight to the feature matrix.
//   fe_gemm_kernel  the mel filterbank and the DCT as small LDS-tiled GEMMs (the shape of gen::gemm_kernel) with the epilogues
//                 none / log(x + 1e-6) / power_to_db (10 log10(max(1e-10, x)), and the maximum over the call as an atomic max
//                 on an order-preserving integer image of the float: deterministic) and, for the DCT, the top_db clamp on the
//                 operand it reads (x < max - 80 -> max - 80).
//   delta_kernel  librosa.feature.delta(width 9, order 1 and 2) = Savitzky-Golay filters along time (mode "interp": the first
//                 and last 4 frames are the polynomial fitted to the first / last 9 frames, evaluated there): columns F..3F of
//                 an [N][3F] matrix whose first F columns the transform wrote.
#pragma once
#include <hip/hip_runtime.h>

#include "savad_audio_host.h"   // geometry, tables and workspace layout: pure host code
#include "savad_device.h"

namespace savad {
namespace fe {

enum { EPI_NONE = 0, EPI_LOG = 1, EPI_DB = 2 };

constexpr int FT = 2;         // 32-frame tiles per workgroup

// ---- device ------------------------------------------------------------------------------------------------------------

// ypad[j] = y[reflect(j - n_fft / 2)] for j in [0, n + n_fft + SLACK) (numpy.pad(mode="reflect"); indices past the padded
// signal read the clamped edge: finite values under zero weights)
__global__ void fe_reflect_pad_kernel(const float* __restrict__ y, long n, int half, long total, float* __restrict__ ypad) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (long)gridDim.x * blockDim.x) {
        long i = j - half;
        if (i < 0) i = -i;
        if (i >= n) i = 2L * (n - 1) - i;
        if (i < 0) i = 0;
        if (i >= n) i = n - 1;
        ypad[j] = y[i];
    }
}

// dst[j] = y[j] for j < n, 0 for j in [n, total): the aligned copy of an unaligned (or too short to over-read) signal
__global__ void fe_copy_kernel(const float* __restrict__ y, long n, long total, float* __restrict__ dst) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (long)gridDim.x * blockDim.x) dst[j] = j < n ? y[j] : 0.0f;
}

__device__ __forceinline__ int float_key(float v) {  // order-preserving: a < b <=> key(a) < key(b) (as signed ints)
    const int i = __float_as_int(v);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

struct StftArgs {
    const float* src;   // frame f reads src[hop f + k0 + c], c in [0, kr)
    const float* tab;   // dft_fragments
    float* out;         // power: [frames][ld] (bins 0..nb-1), or magnitude
    int* gmax;          // reset to key(-inf) by workgroup 0 (the MFCC maximum of this call), or null
    int n_frames, hop, kg, rblocks, nb, n_fft, ld;
    int magnitude;
};

// One workgroup = FT 32-frame tiles; wave w runs the row-block groups w, w + 4, ... (RB blocks each) over the whole K range:
// per k-group of 8 samples RB A fragments and FT sample float4s, RB * FT * 4 MFMAs.  VEC: frames start on 16-byte boundaries
// (hop and k0 multiples of 4, src aligned).
template <bool VEC>
__global__ __launch_bounds__(256, 2) void stft_kernel(StftArgs a) {
    const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (a.gmax && blockIdx.x == 0 && threadIdx.x == 0) *a.gmax = float_key(-INFINITY);
    const float* xp[FT];
    int fr[FT];
#pragma unroll
    for (int t = 0; t < FT; ++t) {
        int f = (blockIdx.x * FT + t) * 32 + m;
        fr[t] = f;
        if (f >= a.n_frames) f = a.n_frames - 1;  // lanes past the last frame redo it; their results are not stored
        xp[t] = a.src + (size_t)a.hop * f + 4 * h;
    }
    const int groups = a.rblocks / RB;
    for (int grp = wv; grp < groups; grp += 4) {
        f32x16 acc[RB][FT];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int t = 0; t < FT; ++t) acc[r][t] = zero16();
        const float* ap = a.tab + (size_t)grp * RB * a.kg * 256 + lane * 4;
        auto load_x = [&](int t, int G) -> f32x4 {
            if constexpr (VEC) return ld4(xp[t] + 8 * G);
            else return f32x4{xp[t][8 * G], xp[t][8 * G + 1], xp[t][8 * G + 2], xp[t][8 * G + 3]};
        };
        f32x4 an[RB], xn[FT];
#pragma unroll
        for (int r = 0; r < RB; ++r) an[r] = ld4(ap + (size_t)r * a.kg * 256);
#pragma unroll
        for (int t = 0; t < FT; ++t) xn[t] = load_x(t, 0);
        for (int G = 0; G < a.kg; ++G) {
            f32x4 ac[RB], xc[FT];
#pragma unroll
            for (int r = 0; r < RB; ++r) ac[r] = an[r];
#pragma unroll
            for (int t = 0; t < FT; ++t) xc[t] = xn[t];
            if (G + 1 < a.kg) {  // the next k-group's operands are requested before this one's MFMAs
#pragma unroll
                for (int r = 0; r < RB; ++r) an[r] = ld4(ap + ((size_t)r * a.kg + G + 1) * 256);
#pragma unroll
                for (int t = 0; t < FT; ++t) xn[t] = load_x(t, G + 1);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int t = 0; t < FT; ++t) acc[r][t] = SAVAD_MFMA(ac[r][e], xc[t][e], acc[r][t]);
        }
        // register pair p = (2p, 2p + 1) holds rows 2 b, 2 b + 1 of the block: bin b = 16 rb + 4 (p >> 1) + 2 h + (p & 1)
#pragma unroll
        for (int t = 0; t < FT; ++t) {
            if (fr[t] >= a.n_frames) continue;
            float* op = a.out + (size_t)fr[t] * a.ld;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int rb = grp * RB + r;
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const float x0 = acc[r][t][2 * p], x1 = acc[r][t][2 * p + 1];
                    const int b = 16 * rb + 4 * (p >> 1) + 2 * h + (p & 1);
                    if (b == 0) {  // rows 0 / 1: re(bin 0), re(bin n_fft / 2)
                        op[0] = a.magnitude ? fabsf(x0) : x0 * x0;
                        if (!(a.n_fft & 1)) op[a.n_fft / 2] = a.magnitude ? fabsf(x1) : x1 * x1;
                    } else if (b < a.nb && !(b == a.n_fft / 2 && !(a.n_fft & 1))) {
                        const float pw = x0 * x0 + x1 * x1;
                        op[b] = a.magnitude ? sqrtf(pw) : pw;
                    }
                }
            }
        }
    }
}

// C[m][n] = sum_k pro(A[m][k]) * W[n][k], then epi; A row-major (lda), W row-major [N][K] (nn.Linear form), C with row stride
// ldc.  PRO: the top_db clamp x -> max(x, key_float(*gmax) - 80).  EPI_DB also folds the maximum of its outputs into *gmax.
struct FeGemm {
    const float* A;
    long lda;
    const float* W;
    float* C;
    long ldc;
    int M, N, K;
    int* gmax;
};

constexpr int GT = 64, GK = 16;

template <int EPI, bool PRO>
__global__ __launch_bounds__(256) void fe_gemm_kernel(FeGemm g) {
    __shared__ float As[GK][GT + 1];
    __shared__ float Ws[GK][GT + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const long m0 = (long)blockIdx.y * GT;
    const int n0 = blockIdx.x * GT;
    float floor_db = 0.0f;
    if constexpr (PRO) floor_db = key_float(*g.gmax) - 80.0f;
    f32x16 acc = zero16();
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    const int kh = lane >> 5, l31 = lane & 31;
    for (int k0 = 0; k0 < g.K; k0 += GK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long m = m0 + ar;
            const int k = k0 + ak + e, n = n0 + ar;
            float v = (m < g.M && k < g.K) ? g.A[m * g.lda + k] : 0.0f;
            if constexpr (PRO) v = fmaxf(v, floor_db);
            As[ak + e][ar] = (m < g.M && k < g.K) ? v : 0.0f;
            Ws[ak + e][ar] = (n < g.N && k < g.K) ? g.W[(long)n * g.K + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GK; k += 2) acc = SAVAD_MFMA(Ws[k + kh][wn * 32 + l31], As[k + kh][wm * 32 + l31], acc);
        __syncthreads();
    }
    // lane: output row m, registers: columns n0 + 32 wn + 8 (r >> 2) + 4 kh + (r & 3)
    const long m = m0 + wm * 32 + l31;
    float mx = -INFINITY;
    if (m < g.M) {
        float* C = g.C + m * g.ldc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wn * 32 + acc_row(r, kh);
            if (n >= g.N) continue;
            float v = acc[r];
            if constexpr (EPI == EPI_LOG) v = logf(v + 1e-6f);
            if constexpr (EPI == EPI_DB) {
                v = 10.0f * log10f(fmaxf(1e-10f, v));
                mx = fmaxf(mx, v);
            }
            C[n] = v;
        }
    }
    if constexpr (EPI == EPI_DB) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0 && mx > -INFINITY) atomicMax(g.gmax, float_key(mx));
    }
}

// X = columns [0, F) of an [N][ld] matrix; columns [F, 2F) and [2F, 3F) get the first and second Savitzky-Golay derivatives
// along the frames: frame t uses the 9 frames from s = clamp(t - 4, 0, N - 9), row u = t - s of each order's table
__global__ void delta_kernel(float* __restrict__ x, int N, int F, long ld, const float* __restrict__ sg) {
    const long total = (long)N * F;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i / F), c = (int)(i % F);
        int s = t - DELTA_W / 2;
        if (s < 0) s = 0;
        if (s > N - DELTA_W) s = N - DELTA_W;
        const float* r1 = sg + (t - s) * DELTA_W;
        const float* r2 = sg + (DELTA_W + t - s) * DELTA_W;
        float d1 = 0.0f, d2 = 0.0f;
#pragma unroll
        for (int j = 0; j < DELTA_W; ++j) {
            const float v = x[(long)(s + j) * ld + c];
            d1 = fmaf(r1[j], v, d1);
            d2 = fmaf(r2[j], v, d2);
        }
        x[(long)t * ld + F + c] = d1;
        x[(long)t * ld + 2 * F + c] = d2;
    }
}

}  // namespace fe
}  // namespace savad
