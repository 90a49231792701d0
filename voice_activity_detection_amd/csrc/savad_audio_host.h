// savad_audio_host.h -- the host side of the audio paths, free of HIP: every table the log-mel kernels (savad_logmel.h), the
// general front-end (savad_frontend.h) and the resampler (savad_ingest.h) read, the geometry those kernels share with their
// tables, and where each entry point's workspace pieces lie.  savad.hip uploads and launches; tests/audio_tables_dump.cpp
// includes this header alone and pins every table and layout bit for bit (tests/test_audio_tables_host.py).
// Tables are computed in float64 and stored as fp32.
#pragma once
#include <math.h>
#include <stddef.h>

#include <utility>
#include <vector>

#include "savad_windows.h"   // Arena

namespace savad {

// ---- Slaney mel scale and filterbank (librosa htk=False, norm="slaney", fmin 0, fmax 8 kHz @16 kHz) ---------------------------

constexpr double PI = 3.14159265358979323846;
constexpr double F_SP = 200.0 / 3, MIN_LOG_HZ = 1000.0, MIN_LOG_MEL = MIN_LOG_HZ / F_SP;   // linear below 1 kHz, log above
inline double hz_to_mel(double f) { return f >= MIN_LOG_HZ ? MIN_LOG_MEL + log(f / MIN_LOG_HZ) / (log(6.4) / 27.0) : f / F_SP; }
inline double mel_to_hz(double mm) { return mm >= MIN_LOG_MEL ? MIN_LOG_HZ * exp(log(6.4) / 27.0 * (mm - MIN_LOG_MEL)) : F_SP * mm; }

// How a filter weight  w * enorm  (both float64) becomes fp32.  The two paths were written apart and each is pinned bit for bit by
// its own tests, so both roundings stay: at (n_fft 512, 80 mels) they differ, by one rounding, in about a third of the non-zero weights.
//   ROUND_FACTORS  fp32(w) * fp32(enorm)   the log-mel kernels of the shipped geometry (mel::fft_tables, mel::mel_fragments)
//   ROUND_PRODUCT  fp32(w * enorm)         the general front-end (savad_frontend's table 1)
enum MelRounding { ROUND_FACTORS, ROUND_PRODUCT };

// librosa.filters.mel(sr=16000, n_fft, n_mels): M[mel][bin], n_mels x (n_fft / 2 + 1)
inline std::vector<float> mel_filterbank(int n_fft, int n_mels, MelRounding rounding) {
    const int nb = n_fft / 2 + 1;
    std::vector<double> mel_f(n_mels + 2);
    const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(8000.0);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    std::vector<float> M((size_t)n_mels * nb, 0.0f);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int b = 0; b < nb; ++b) {
            const double fr = nb > 1 ? 8000.0 * b / (nb - 1) : 0.0;  // fft_frequencies = linspace(0, sr / 2, nb)
            const double lower = (fr - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1]);
            const double wgt = fmax(0.0, fmin(lower, upper));
            M[(size_t)i * nb + b] = rounding == ROUND_FACTORS ? (float)wgt * (float)enorm : (float)(wgt * enorm);
        }
    }
    return M;
}

// ---- log-mel of the shipped geometry (kernels and operand layouts: savad_logmel.h) --------------------------------------------
namespace mel {

constexpr int N_FFT = 512, HOP = 160, WIN = 400, N_MELS = 80, LPAD = (N_FFT - WIN) / 2;  // LPAD = 56
constexpr int KG = WIN / 8;                    // 50 k-groups of 8 samples
constexpr int DFT_FRAG_FLOATS = 16 * KG * 256;  // [row block 16][G 50][lane 64][4]
constexpr int MEL_FRAG_FLOATS = 4 * 3 * 4 * 2 * 256;  // [pass 4][mel block 3][row block 4][g pair 2][lane 64][4]
constexpr int FFT_T1_FLOATS = 4 * 13 * 256;   // [wave 4][k-step 13][lane 64][n2 & 3]
constexpr int FFT_T3_FLOATS = 16 * 4 * 256;   // [group 16][n2 >> 2][lane 64][n2 & 3]
constexpr int FFT_TM_FLOATS = 16 * 3 * 256;   // [group 16][t >> 2][lane 64][t & 3], t = 0..9 (10, 11 unused)

// A operands of logmel_fft_kernel (algorithm 0).  False when a filter weight falls outside the kernel's fixed
// (register pair -> mel block) pattern, which would be a bug in the bin ordering.
inline bool fft_tables(std::vector<float>& t1, std::vector<float>& t3, std::vector<float>& tm) {
    const int NB = N_FFT / 2 + 1;
    t1.assign(FFT_T1_FLOATS, 0.0f);
    t3.assign(FFT_T3_FLOATS, 0.0f);
    tm.assign(FFT_TM_FLOATS, 0.0f);
    // step 1: row i = lane & 31 of the output tile is (k1 = 4 (i >> 3) + (i & 3), re | im = (i >> 2) & 1); k-step s of
    // lane half h is n1 = 3 + 2 s + h; the slot of im(k1 = 0) carries re(k1 = 16)
    for (int w = 0; w < 4; ++w)
        for (int s = 0; s < 13; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int i = lane & 31, h = lane >> 5, n1 = 3 + 2 * s + h, n2 = 4 * w + e, n = 16 * n1 + n2;
                    const bool re16 = i == 4;   // (k1 = 0, im): the slot of re(k1 = 16)
                    const int k1 = re16 ? 16 : 4 * (i >> 3) + (i & 3);
                    const bool im = !re16 && ((i >> 2) & 1);
                    float win = 0.0f;
                    if (n >= LPAD && n < LPAD + WIN) win = (float)(0.5 - 0.5 * cos(2.0 * PI * (n - LPAD) / WIN));  // periodic Hann(400), float32 as librosa's
                    const double ph = 2.0 * PI * (double)(n1 * k1 % 32) / 32.0;
                    t1[(((size_t)w * 13 + s) * 64 + lane) * 4 + e] = (float)(win * (im ? -sin(ph) : cos(ph)));
                }
    // bins of a group, lowest first.  kind 0: bin K = 32 k2 from Y[0] (real, low lane half); kind 1: K = 16 + 32 k2 from
    // Y[16] (real, high lane half); kind 2: K = k1 + 32 k2 from the complex Y[k1].  label = the bin below 257 with the same power.
    struct Bin {
        int kind, K, label;
    };
    std::vector<std::vector<Bin>> groups(16);
    for (int grp = 0; grp < 16; ++grp) {
        std::vector<Bin>& g = groups[grp];
        if (grp == 0) {
            for (int k2 = 1; k2 < 8; ++k2) g.push_back({0, 32 * k2, 32 * k2});
            for (int k2 = 0; k2 < 8; ++k2) g.push_back({1, 16 + 32 * k2, 16 + 32 * k2});
        } else {
            for (int k2 = 0; k2 < 16; ++k2) {
                const int K = grp + 32 * k2;
                g.push_back({2, K, K <= 256 ? K : 512 - K});
            }
        }
        for (size_t a = 1; a < g.size(); ++a)  // insertion sort by label
            for (size_t b = a; b > 0 && g[b].label < g[b - 1].label; --b) std::swap(g[b], g[b - 1]);
    }
    // step 3: row i of the output tile is (register pair p = 2 (i >> 3) + ((i & 3) >> 1), lane half hD = (i >> 2) & 1,
    // re | im = i & 1) = bin number 2 p + hD of the group; k-step n2 of lane half h multiplies re (h = 0) / im (h = 1) of Y
    for (int grp = 0; grp < 16; ++grp)
        for (int n2 = 0; n2 < 16; ++n2)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const int p = 2 * (i >> 3) + ((i & 3) >> 1), hD = (i >> 2) & 1, ro = i & 1, idx = 2 * p + hD;
                float v = 0.0f;
                if (idx < (int)groups[grp].size()) {
                    const Bin& b = groups[grp][idx];
                    const double th = 2.0 * PI * (double)((long)n2 * b.K % N_FFT) / N_FFT, c = cos(th), sn = sin(th);
                    // X = sum (Yre + i Yim)(c - i sn):  re = Yre c + Yim sn,  im = Yim c - Yre sn
                    if (b.kind == 2)
                        v = (float)(h == 0 ? (ro == 0 ? c : -sn) : (ro == 0 ? sn : c));
                    else if (b.kind == h)
                        v = (float)(ro == 0 ? c : -sn);
                }
                t3[(((size_t)grp * 4 + (n2 >> 2)) * 64 + lane) * 4 + (n2 & 3)] = v;
            }
    // mel: entry t of a group = (pair, mel block) in the kernel's fixed order
    static const int PAIR[10] = {0, 1, 1, 2, 3, 4, 4, 5, 6, 7}, BLOCK[10] = {0, 0, 1, 1, 1, 1, 2, 2, 2, 2};
    const std::vector<float> M = mel_filterbank(N_FFT, N_MELS, ROUND_FACTORS);
    std::vector<char> covered((size_t)N_MELS * NB, 0);
    for (int grp = 0; grp < 16; ++grp)
        for (int t = 0; t < 10; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = lane & 31, h = lane >> 5, idx = 2 * PAIR[t] + h, ml = 32 * BLOCK[t] + j;
                if (idx < (int)groups[grp].size() && ml < N_MELS) {
                    const int label = groups[grp][idx].label;
                    tm[(((size_t)grp * 3 + (t >> 2)) * 64 + lane) * 4 + (t & 3)] = M[(size_t)ml * NB + label];
                    covered[(size_t)ml * NB + label] = 1;
                }
            }
    for (size_t q = 0; q < M.size(); ++q)
        if (M[q] != 0.0f && !covered[q]) return false;
    return true;
}

// A operand of logmel_kernel (algorithm 1): the window-folded DFT rows in fragment order [row block 16][G 50][lane 64][4]:
// row 0 = re(bin 0), row 1 = re(bin 256) (both imaginary parts are identically 0), row 2b / 2b+1 = re / im of bin b
inline std::vector<float> dft_fragments() {
    std::vector<float> dft((size_t)DFT_FRAG_FLOATS);
    for (int rb = 0; rb < 16; ++rb)
        for (int G = 0; G < KG; ++G)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int n = lane & 31, hh = lane >> 5, row = 32 * rb + n, kk = 8 * G + 4 * hh + e;
                    const double win = 0.5 - 0.5 * cos(2.0 * PI * kk / WIN);  // periodic Hann(400)
                    const int kp = kk + LPAD;                                  // position inside the 512-sample frame
                    const int bin = row == 1 ? 256 : row >> 1;
                    const bool im = row != 1 && (row & 1);
                    const double ph = 2.0 * PI * (double)((long)bin * kp % N_FFT) / N_FFT;
                    dft[(((size_t)rb * KG + G) * 64 + lane) * 4 + e] = (float)((float)win * (im ? -sin(ph) : cos(ph)));
                }
    return dft;
}

// its mel fragments [pass 4][mel block 3][row block 4][g pair 2][lane 64][4]; element e -> g = 2gp + (e>>1), bin
// 64 pass + 16 rbl + 4 g + 2 h + (e&1).  Bins 0 and 256 have zero weight in every filter (fmin 0, fmax 8 kHz).
inline std::vector<float> mel_fragments() {
    const int NB = N_FFT / 2 + 1;
    const std::vector<float> M = mel_filterbank(N_FFT, N_MELS, ROUND_FACTORS);
    std::vector<float> melf((size_t)MEL_FRAG_FLOATS, 0.0f);
    for (int pass = 0; pass < 4; ++pass)
        for (int mb = 0; mb < 3; ++mb)
            for (int rbl = 0; rbl < 4; ++rbl)
                for (int gp = 0; gp < 2; ++gp)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int n = lane & 31, hh = lane >> 5, g = 2 * gp + (e >> 1);
                            const int bin = 64 * pass + 16 * rbl + 4 * g + 2 * hh + (e & 1);
                            const int ml_ = 32 * mb + n;
                            float v = 0.0f;
                            if (ml_ < N_MELS && bin >= 1 && bin < 256) v = M[(size_t)ml_ * NB + bin];
                            melf[(((((size_t)pass * 3 + mb) * 4 + rbl) * 2 + gp) * 64 + lane) * 4 + e] = v;
                        }
    return melf;
}

// samples [first, first + count) of the signal that frames [frame_first, frame_first + frame_count) read, reflections
// at the signal's ends included; first is rounded down to a multiple of 4 (16-byte alignment of the direct reads)
inline void span_samples(long n, int frame_first, int frame_count, long* first, long* count) {
    const long lo = (long)HOP * frame_first - 208, hi = (long)HOP * (frame_first + frame_count - 1) + 208;  // [lo, hi)
    long a = lo < 0 ? 0 : lo, b = hi > n ? n : hi;
    if (lo < 0 && -lo + 1 > b) b = -lo + 1;
    if (hi > n && 2 * (n - 1) - (hi - 1) < a) a = 2 * (n - 1) - (hi - 1);
    if (a < 0) a = 0;
    if (b > n) b = n;
    a &= ~3L;
    *first = a;
    *count = b - a;
}

// Which padded indices j (ypad[j] = y[reflect(j - 256)]) frames [frame_first, frame_first + frame_count) of an n-sample signal read,
// in 16-byte chunks: [j_first, j_last + 4).  On the direct path (aligned audio) the chunks below a_end = 256 come from stretch A =
// padded indices [a_j0, a_j0 + a_count), the mirrored head; the chunks from b_j0 on from stretch B = [b_j0, b_j0 + b_count), the
// run past the last sample; everything between straight from the audio.  A stretch the frames do not touch has count 0 and its
// bound is PAD_NEVER away.  Written once, for the host (savad_logmel_span, the plans) and for the kernels that place the stretches
// themselves (savad_logmel_batch.h): __host__ __device__ under hipcc, plain C++ anywhere else.
#if defined(__HIPCC__)
#define SAVAD_PAD_HD __host__ __device__
#else
#define SAVAD_PAD_HD
#endif
constexpr long PAD_NEVER = 1L << 40;
constexpr int PAD_A_MAX = 208, PAD_B_MAX = 212;   // floats a stretch holds at most
struct PadRule {
    long j_first, j_last;
    long a_j0, a_end, b_j0;
    int a_count, b_count;
};
SAVAD_PAD_HD inline PadRule pad_rule(long n, long frame_first, long frame_count) {
    PadRule r{};
    r.j_first = (long)HOP * frame_first + 48;
    r.j_last = (long)HOP * (frame_first + frame_count - 1) + 460;
    r.a_end = -PAD_NEVER;
    r.b_j0 = PAD_NEVER;
    if (r.j_first < N_FFT / 2) {  // the stretch that mirrors the head of the signal
        r.a_j0 = r.j_first;
        r.a_count = (int)((r.j_last + 4 < N_FFT / 2 ? r.j_last + 4 : N_FFT / 2) - r.j_first);
        r.a_end = N_FFT / 2;
    }
    const long jb = (n + 253 + 3) & ~3L;  // first chunk that runs past the last sample
    if (r.j_last >= jb) {
        r.b_j0 = jb;
        r.b_count = (int)(r.j_last + 4 - jb);  // <= 212
    }
    return r;
}
// the sample padded index j stands for: one reflection at either end (numpy.pad(mode="reflect")), then the clamps for signals
// shorter than the padding -- the index rule of reflect_pad_segments_kernel (savad_logmel.h).  That kernel keeps its own statement:
// calling this inline there gave it another register allocation (54 VGPRs for 52, other instruction order), and its code is pinned
SAVAD_PAD_HD inline long pad_source(long j, long n) {
    long i = j - N_FFT / 2;
    if (i < 0) i = -i;
    if (i >= n) i = 2L * (n - 1) - i;
    if (i < 0) i = 0;
    if (i >= n) i = n - 1;
    return i;
}
#undef SAVAD_PAD_HD

// Workspace of savad_logmel (n samples) and savad_logmel_span (frame_count frames), in bytes.  Algorithm 1 and an unaligned
// audio pointer fill it from offset 0 with the padded signal / the padded span; aligned audio materialises only the two
// edge stretches (the mirrored head, at most 208 floats, and the run past the last sample, at most 212), one PAD_SEG each.
constexpr size_t PAD_SEG_BYTES = 256 * sizeof(float);
constexpr size_t SPAN_SLACK_BYTES = 8 * PAD_SEG_BYTES;   // what a span's workspace holds beyond its padded samples
static_assert(2 * PAD_SEG_BYTES <= SPAN_SLACK_BYTES && 2 * PAD_SEG_BYTES <= (N_FFT + 64) * sizeof(float), "both edge stretches fit every workspace");
struct Workspace { size_t pad_a, pad_b, total; };
inline Workspace workspace(size_t signal_floats, size_t slack_bytes) {
    Arena a;
    const size_t pad_a = a.take(PAD_SEG_BYTES), pad_b = a.take(PAD_SEG_BYTES);
    return Workspace{pad_a, pad_b, (signal_floats + N_FFT + 64) * sizeof(float) + slack_bytes};
}
inline Workspace workspace_whole(int n_samples) { return workspace((size_t)n_samples, 0); }
inline Workspace workspace_span(int frame_count) { return workspace((size_t)HOP * (frame_count > 0 ? frame_count : 0), SPAN_SLACK_BYTES); }

}  // namespace mel

// ---- general front-end (kernels: savad_frontend.h) ------------------------------------------------------------------------------
namespace fe {

enum { SPECTROGRAM = 0, MEL = 1, LOGMEL = 2, MFCC = 3 };

constexpr int RB = 4;         // DFT row blocks (32 rows each) per wave pass
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
    const int lpad = (n_fft - win) / 2, k0 = lpad & ~3, kg = (lpad + win - k0 + 7) / 8, rows = 2 * ((n_fft + 1) / 2), nb = n_fft / 2 + 1;
    return Geo{n_fft, hop, win, lpad, k0, 8 * kg, kg, rows, (rows + 32 * RB - 1) / (32 * RB) * RB, nb, (nb + 3) & ~3};
}

// Config below: any struct with the fields of savad_frontend_config (include/savad.h: transform, n_fft, hop, win, n_mels, n_mfcc, deltas)
template <class Config>
Geo geometry(const Config& c) { return geometry(c.n_fft, c.hop, c.win); }

// frames and features of a call on n samples.  need: the fewest samples the transform takes (n_fft / 2 + 1 under reflect
// padding, n_fft for the spectrogram's center=False); frames counts the n_fft-sample window over the signal (padded by
// n_fft / 2 per side when centred): 1 + n / hop for an even n_fft.  The refusals (n < need, frames < DELTA_W with deltas)
// are savad.hip's.
struct Shape { long need, frames; int feats; };
template <class Config>
Shape shape(const Config& c, long n) {
    const bool centred = c.transform != SPECTROGRAM;
    const int F = c.transform == SPECTROGRAM ? c.n_fft / 2 + 1 : c.transform == MFCC ? c.n_mfcc : c.n_mels;
    return Shape{centred ? c.n_fft / 2 + 1 : c.n_fft, 1 + (n + (centred ? 2 * (c.n_fft / 2) : 0) - c.n_fft) / c.hop, c.deltas ? 3 * F : F};
}

// workspace of savad_frontend (bytes): MFCC maximum | padded / copied signal | power [N][nbs] | dB mel [N][n_mels]
struct Workspace { size_t gmax, sig, spec, db, total; };
template <class Config>
Workspace workspace(const Config& c, long n, long frames) {
    Arena a;
    const size_t gmax = a.take(sizeof(int)), sig = a.take(((size_t)n + c.n_fft + SLACK) * sizeof(float));
    const size_t spec = a.take(c.transform == SPECTROGRAM ? 0 : (size_t)frames * geometry(c).nbs * sizeof(float));
    const size_t db = a.take(c.transform == MFCC ? (size_t)frames * c.n_mels * sizeof(float) : 0);
    return Workspace{gmax, sig, spec, db, a.off};
}

// Plain DFT matrix [rblocks * 32][kr]: row 0 = re(bin 0), row 1 = re(bin n_fft / 2) for an even n_fft (both imaginary parts
// vanish; a zero row for an odd one), rows 2b / 2b + 1 = re / im of bin b; column c = frame sample k0 + c.  Window: periodic
// Hann (librosa's "hann", scipy get_window(fftbins=True)) for the centred transforms, periodic Hamming (torch.hamming_window)
// for the spectrogram, placed at lpad inside the n_fft-sample frame.
inline std::vector<float> dft_plain(const Geo& g, bool hamming) {
    const int R = g.rblocks * 32;
    std::vector<float> t((size_t)R * g.kr, 0.0f);
    for (int r = 0; r < R && r < g.rows; ++r) {
        if (r == 1 && (g.n_fft & 1)) continue;
        const int bin = r == 1 ? g.n_fft / 2 : r >> 1;
        const bool im = r != 1 && (r & 1);
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

// DCT-II, norm="ortho": [n_mfcc][n_mels]
inline std::vector<float> dct_ortho(int n_mels, int n_mfcc) {
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

// table `which` of a configuration as savad_frontend_tables_host hands it out: 0 = plain DFT, 1 = mel filterbank,
// 2 = DCT, 3 = Savitzky-Golay rows; empty where the transform has no such table
template <class Config>
std::vector<float> host_table(const Config& c, int which) {
    if (which == 0) return dft_plain(geometry(c), c.transform == SPECTROGRAM);
    if (which == 1) return c.transform == SPECTROGRAM ? std::vector<float>() : mel_filterbank(c.n_fft, c.n_mels, ROUND_PRODUCT);
    if (which == 2) return c.transform == MFCC ? dct_ortho(c.n_mels, c.n_mfcc) : std::vector<float>();
    return savgol_rows();
}

}  // namespace fe

// ---- resampler (kernels and the time register's story: savad_ingest.h) --------------------------------------------------------
namespace ingest {

constexpr int NWIN = 8193;        // resampy "kaiser_fast": 16 zero crossings x 512 entries + 1
constexpr int NUM_TABLE = 512;    // entries per zero crossing (precision 9)
constexpr int TARGET = 16000;
constexpr int BLOCK = 1024;       // outputs per workgroup pass: 16 waves, 4 per SIMD, around one table in LDS
constexpr int MAX_SEGS = 256;     // time-register segments (44.1 kHz needs 49 for 2^45 input samples)
constexpr int RATE_MIN = 1000, RATE_MAX = 100000;
constexpr int LDS_BYTES_MAX = 160 * 1024;
constexpr double T_END = 35184372088832.0;  // 2^45 input samples: where the segment walk stops

struct Seg {
    long long k0;  // first output sample of the segment
    double t0;     // its time register
    double s;      // exact step between consecutive time registers inside the segment
};

struct Plan {
    double ratio, scale, inc;  // 16000 / rate; min(1, ratio); 1 / ratio  (resampy: sample_ratio, scale, time_increment)
    int step;                  // int(scale * 512): table stride of one tap
    int taps;                  // upper bound of a wing's length: 8193 / step
    int span;                  // LDS floats of a block's input span
};

inline Plan plan_for(int rate) {
    const double ratio = (double)TARGET / (double)rate, scale = ratio < 1.0 ? ratio : 1.0, inc = 1.0 / ratio;
    const int step = (int)(scale * NUM_TABLE), taps = NWIN / step;
    // span: n(last lane) - n(first lane) <= ceil((BLOCK - 1) * inc) + 1 (the register's rounding stays far below one sample)
    return Plan{ratio, scale, inc, step, taps, (int)ceil((BLOCK - 1) * inc) + 2 + 2 * taps + 2};
}

inline size_t lds_bytes(const Plan& p, bool table_in_lds) {
    return (table_in_lds ? (size_t)NWIN * 16 : 0) + (size_t)p.span * sizeof(float);
}

// the caller's half window as a rate's kernel reads it: scaled by the ratio when downsampling (resampy: interp_win *=
// sample_ratio), and its first differences (np.diff; delta[last] = 0)
inline void scaled_window(const Plan& p, const std::vector<double>& half_window, std::vector<double>& win, std::vector<double>& delta) {
    win = half_window;
    if (p.ratio < 1.0)
        for (double& v : win) v = v * p.ratio;
    delta.assign(NWIN, 0.0);
    for (int i = 0; i + 1 < NWIN; ++i) delta[i] = win[i + 1] - win[i];
}

// (k_0, t_0, s) segments of the time register for increment c, up to T_END; *k_end = the first output NOT covered.
// Empty when more than MAX_SEGS segments would be needed (a tie binade that holds many steps).
inline std::vector<Seg> time_segments(double c, long long* k_end) {
    std::vector<Seg> v;
    volatile double t = 0.0;  // (volatile: every addition below is the float64 addition resampy makes, never folded)
    long long k = 0;
    while (t < T_END) {
        if ((int)v.size() >= MAX_SEGS) {
            v.clear();
            break;
        }
        const double tc = t;
        volatile double t1 = tc + c;
        if (tc <= 0.0) {
            v.push_back(Seg{k, tc, c});
            k += 1;
            t = t1;
            continue;
        }
        const int e = ilogb(tc);
        const double u = ldexp(1.0, e - 52), hi = ldexp(1.0, e + 1);
        const double q = c / (0.5 * u);  // exact (a power of two): c in half ulps of t
        const bool tie = q == floor(q) && fmod(q, 2.0) == 1.0;
        const double s = t1 - tc;  // exact
        if (t1 >= hi || tie || s <= 0.0) {
            if (s <= 0.0) break;  // (increment below half an ulp: beyond T_END for every supported rate)
            v.push_back(Seg{k, tc, s});
            k += 1;
            t = t1;
            continue;
        }
        const long long T = (long long)(tc / u), S = (long long)(s / u), H = 1LL << 53;
        const long long m = (H - 1 - T) / S;  // t_0 + j s stays below 2^(e+1) for j = 0 .. m
        v.push_back(Seg{k, tc, s});
        k += m + 1;
        volatile double tm = tc + (double)m * s;  // exact
        t = tm + c;                               // the crossing: a true addition
    }
    *k_end = k;
    return v;
}

inline double time_at(const std::vector<Seg>& segs, long long k) {
    size_t lo = 0, hi = segs.size();
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (segs[mid].k0 <= k) lo = mid; else hi = mid;
    }
    return segs[lo].t0 + (double)(k - segs[lo].k0) * segs[lo].s;
}

// the input samples outputs [o0, o1) read (o1 <= int(n_in * ratio), o0 < o1): a wing holds at most `taps` taps, the left one
// x[n], x[n-1] ..., the right one x[n+1], x[n+2] ...  *first is rounded down to a multiple of 4.
inline void span_inputs(const Plan& p, const std::vector<Seg>& segs, long long n_in, long long o0, long long o1, long long* first, long long* count) {
    const long long n_lo = (long long)time_at(segs, o0), n_hi = (long long)time_at(segs, o1 - 1);
    long long a = n_lo - p.taps + 1, b = n_hi + p.taps + 1;
    if (a < 0) a = 0;
    a = a / 4 * 4;
    if (b > n_in) b = n_in;
    if (b < a) b = a;
    *first = a;
    *count = b - a;
}

}  // namespace ingest
}  // namespace savad
