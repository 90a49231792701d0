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
#include <math.h>

#include <vector>

#include "savad_device.h"

namespace savad {
namespace fe {

enum { SPECTROGRAM = 0, MEL = 1, LOGMEL = 2, MFCC = 3 };
enum { EPI_NONE = 0, EPI_LOG = 1, EPI_DB = 2 };

constexpr int RB = 4;         // DFT row blocks (32 rows each) per wave pass
constexpr int FT = 2;         // 32-frame tiles per workgroup
constexpr int SLACK = 64;     // floats of readable (finite) slack after a padded signal: the K range may end past the frame
constexpr int DELTA_W = 9;    // librosa.feature.delta(width=9)

// geometry of one configuration (host and device agree on it; every field derives from the config)
struct Geo {
    int n_fft, hop, win, lpad;  // lpad = (n_fft - win) / 2: librosa pad_center / torch.stft's window placement
    int k0, kr, kg;             // K range: frame samples [k0, k0 + kr), k0 = lpad rounded down to 4, kr = 8 kg
    int rows, rblocks;          // DFT rows (2 ceil(n_fft / 2)) and row blocks padded to a multiple of RB
    int nb, nbs;                // bins (n_fft / 2 + 1) and the power workspace's row stride (multiple of 4)
};

inline Geo geometry(int n_fft, int hop, int win) {
    Geo g;
    g.n_fft = n_fft;
    g.hop = hop;
    g.win = win;
    g.lpad = (n_fft - win) / 2;
    g.k0 = g.lpad & ~3;
    g.kg = (g.lpad + win - g.k0 + 7) / 8;
    g.kr = 8 * g.kg;
    g.rows = 2 * ((n_fft + 1) / 2);
    g.rblocks = (g.rows + 32 * RB - 1) / (32 * RB) * RB;
    g.nb = n_fft / 2 + 1;
    g.nbs = (g.nb + 3) & ~3;
    return g;
}

// ---- host tables (float64 arithmetic, stored as fp32) ------------------------------------------------------------------

// Plain DFT matrix [rblocks * 32][kr]: row 0 = re(bin 0), row 1 = re(bin n_fft / 2) for an even n_fft (both imaginary parts
// vanish; a zero row for an odd one), rows 2b / 2b + 1 = re / im of bin b; column c = frame sample k0 + c.  Window: periodic
// Hann (librosa's "hann", scipy get_window(fftbins=True)) for the centred transforms, periodic Hamming (torch.hamming_window)
// for the spectrogram, placed at lpad inside the n_fft-sample frame.
inline std::vector<float> dft_plain(const Geo& g, bool hamming) {
    const double PI = 3.14159265358979323846;
    const int R = g.rblocks * 32;
    std::vector<float> t((size_t)R * g.kr, 0.0f);
    for (int r = 0; r < R && r < g.rows; ++r) {
        int bin = r >> 1;
        bool im = r & 1;
        if (r == 1) {
            if (g.n_fft & 1) continue;
            bin = g.n_fft / 2;
            im = false;
        }
        for (int c = 0; c < g.kr; ++c) {
            const int kp = g.k0 + c, j = kp - g.lpad;
            if (j < 0 || j >= g.win) continue;
            const double w = hamming ? 0.54 - 0.46 * cos(2.0 * PI * j / g.win) : 0.5 - 0.5 * cos(2.0 * PI * j / g.win);
            const double ph = 2.0 * PI * (double)((long)bin * kp % g.n_fft) / g.n_fft;
            t[(size_t)r * g.kr + c] = (float)(w * (im ? -sin(ph) : cos(ph)));
        }
    }
    return t;
}

// The same in the A-operand fragment order of stft_kernel: [row block][k-group][lane 64][4], element e of lane (i, h) =
// row 32 rb + i, column 8 G + 4 h + e
inline std::vector<float> dft_fragments(const Geo& g, const std::vector<float>& plain) {
    std::vector<float> t((size_t)g.rblocks * g.kg * 256);
    for (int rb = 0; rb < g.rblocks; ++rb)
        for (int G = 0; G < g.kg; ++G)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e)
                    t[(((size_t)rb * g.kg + G) * 64 + lane) * 4 + e] = plain[(size_t)(32 * rb + (lane & 31)) * g.kr + 8 * G + 4 * (lane >> 5) + e];
    return t;
}

inline double hz_to_mel_slaney(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
inline double mel_to_hz_slaney(double mm) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return mm >= min_log_mel ? min_log_hz * exp(logstep * (mm - min_log_mel)) : f_sp * mm;
}

// librosa.filters.mel(sr=16000, n_fft, n_mels, fmin=0, fmax=8000, htk=False, norm="slaney"): [n_mels][nb]
inline std::vector<float> mel_filterbank(int n_fft, int n_mels) {
    const int nb = n_fft / 2 + 1;
    std::vector<double> mel_f(n_mels + 2);
    const double m_lo = hz_to_mel_slaney(0.0), m_hi = hz_to_mel_slaney(8000.0);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz_slaney(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    std::vector<float> M((size_t)n_mels * nb, 0.0f);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int b = 0; b < nb; ++b) {
            const double fr = nb > 1 ? 8000.0 * b / (nb - 1) : 0.0;  // fft_frequencies = linspace(0, sr / 2, nb)
            const double lower = (fr - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1]);
            M[(size_t)i * nb + b] = (float)(fmax(0.0, fmin(lower, upper)) * enorm);
        }
    }
    return M;
}

// DCT-II, norm="ortho": [n_mfcc][n_mels]
inline std::vector<float> dct_ortho(int n_mels, int n_mfcc) {
    const double PI = 3.14159265358979323846;
    std::vector<float> D((size_t)n_mfcc * n_mels);
    for (int k = 0; k < n_mfcc; ++k)
        for (int n = 0; n < n_mels; ++n)
            D[(size_t)k * n_mels + n] = (float)(sqrt((k == 0 ? 1.0 : 2.0) / n_mels) * cos(PI * k * (2 * n + 1) / (2.0 * n_mels)));
    return D;
}

// Savitzky-Golay rows [order - 1][u][j]: the order-th derivative at position u (0..8) of the degree-`order` least-squares
// polynomial through 9 points at positions 0..8 = sum_j row[j] x[j].  u = 4 is the interior filter (scipy savgol_coeffs),
// u = 0..3 / 5..8 the edge rows of mode="interp".
inline std::vector<float> savgol_rows() {
    std::vector<float> out(2 * DELTA_W * DELTA_W);
    for (int order = 1; order <= 2; ++order) {
        const int P = order + 1;  // polynomial coefficients
        // normal equations: (V^T V) a = V^T x, V[j][k] = j^k; row(u) = d(u)^T (V^T V)^-1 V^T
        double A[3][3] = {{0}}, inv[3][3] = {{0}};
        for (int r = 0; r < P; ++r)
            for (int c = 0; c < P; ++c)
                for (int j = 0; j < DELTA_W; ++j) A[r][c] += pow((double)j, r + c);
        for (int r = 0; r < P; ++r) inv[r][r] = 1.0;
        for (int c = 0; c < P; ++c) {  // Gauss-Jordan (symmetric positive definite: no pivoting needed)
            const double p = A[c][c];
            for (int k = 0; k < P; ++k) {
                A[c][k] /= p;
                inv[c][k] /= p;
            }
            for (int r = 0; r < P; ++r)
                if (r != c) {
                    const double f = A[r][c];
                    for (int k = 0; k < P; ++k) {
                        A[r][k] -= f * A[c][k];
                        inv[r][k] -= f * inv[c][k];
                    }
                }
        }
        for (int u = 0; u < DELTA_W; ++u) {
            double d[3] = {0, 0, 0};  // d/du^order of u^k
            for (int k = order; k < P; ++k) {
                double f = 1.0;
                for (int q = 0; q < order; ++q) f *= (k - q);
                d[k] = f * pow((double)u, k - order);
            }
            for (int j = 0; j < DELTA_W; ++j) {
                double v = 0.0;
                for (int r = 0; r < P; ++r)
                    for (int c = 0; c < P; ++c) v += d[r] * inv[r][c] * pow((double)j, c);
                out[((size_t)(order - 1) * DELTA_W + u) * DELTA_W + j] = (float)v;
            }
        }
    }
    return out;
}

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
