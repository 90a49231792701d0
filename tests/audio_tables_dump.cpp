// Prints what voice_activity_detection_amd/csrc/savad_audio_host.h computes, one "key value ..." line each: the SHA-256 of every
// host-built table's raw bytes, the resampler's plans, and the workspace layouts and shapes of the audio entry points.
// tests/test_audio_tables_host.py compares the lines with tests/golden/audio_tables.json and with the library's exports.
// Host C++ only: the one project header, no HIP.
#include "savad_audio_host.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

using namespace savad;

namespace {

struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t block[64];
    uint64_t bytes = 0;

    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void compress() {
        static const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
            0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
            0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
            0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
            0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
            0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64], v[8];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)block[4 * i] << 24 | (uint32_t)block[4 * i + 1] << 16 | (uint32_t)block[4 * i + 2] << 8 | block[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        memcpy(v, h, sizeof(v));
        for (int i = 0; i < 64; ++i) {
            const uint32_t s1 = rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25), ch = (v[4] & v[5]) ^ (~v[4] & v[6]);
            const uint32_t t1 = v[7] + s1 + ch + K[i] + w[i];
            const uint32_t s0 = rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22), maj = (v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]);
            const uint32_t t2 = s0 + maj;
            for (int j = 7; j > 0; --j) v[j] = v[j - 1];
            v[4] += t1;
            v[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i) h[i] += v[i];
    }
    void add(const void* data, size_t n) {
        const uint8_t* p = (const uint8_t*)data;
        for (size_t i = 0; i < n; ++i) {
            block[bytes++ % 64] = p[i];
            if (bytes % 64 == 0) compress();
        }
    }
    std::string hex() {
        const uint64_t bits = bytes * 8;
        const uint8_t one = 0x80, zero = 0;
        add(&one, 1);
        while (bytes % 64 != 56) add(&zero, 1);
        uint8_t len[8];
        for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        add(len, 8);
        char out[65];
        for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
        return out;
    }
};

template <class T>
void print_hash(const std::string& key, const std::vector<T>& v) {
    Sha256 s;
    if (!v.empty()) s.add(v.data(), v.size() * sizeof(T));
    printf("%s %s %zu\n", key.c_str(), s.hex().c_str(), v.size() * sizeof(T));
}

struct Config {   // the fields of savad_frontend_config (include/savad.h)
    int transform, n_fft, hop, win, n_mels, n_mfcc, deltas;
};
struct Named {
    const char* name;
    Config c;
};

}  // namespace

int main() {
    // log-mel of the shipped geometry: the factored kernel's operands, then the DFT-as-GEMM kernel's
    std::vector<float> t1, t3, tm;
    if (!mel::fft_tables(t1, t3, tm)) {
        printf("logmel.fft_tables uncovered\n");
        return 1;
    }
    print_hash("logmel.t1", t1);
    print_hash("logmel.t3", t3);
    print_hash("logmel.tm", tm);
    print_hash("logmel.dft_frag", mel::dft_fragments());
    print_hash("logmel.mel_frag", mel::mel_fragments());
    // the one filterbank under its two roundings, and how many weights tell them apart
    const std::vector<float> fa = mel_filterbank(512, 80, ROUND_FACTORS), pr = mel_filterbank(512, 80, ROUND_PRODUCT);
    print_hash("filterbank.512x80.factors", fa);
    print_hash("filterbank.512x80.product", pr);
    size_t differ = 0, nonzero = 0;
    for (size_t i = 0; i < fa.size(); ++i) {
        differ += fa[i] != pr[i];
        nonzero += pr[i] != 0.0f;
    }
    printf("filterbank.512x80.differ %zu %zu\n", differ, nonzero);

    // log-mel workspaces: total and the two pad segments (bytes)
    for (int n : {1, 159, 160, 161, 4000, 57600000}) {
        const mel::Workspace w = mel::workspace_whole(n);
        printf("logmel.ws.whole.%d %zu %zu %zu\n", n, w.total, w.pad_a, w.pad_b);
    }
    for (int frames : {1, 32, 33, 45000}) {
        const mel::Workspace w = mel::workspace_span(frames);
        printf("logmel.ws.span.%d %zu %zu %zu\n", frames, w.total, w.pad_a, w.pad_b);
    }
    for (long n : {1L, 159L, 160L, 161L, 4000L, 57600000L}) {   // the samples the first, the last and all frames read
        const int frames = 1 + (int)(n / mel::HOP);
        long a, b, c, d, e, f;
        mel::span_samples(n, 0, 1, &a, &b);
        mel::span_samples(n, frames - 1, 1, &c, &d);
        mel::span_samples(n, 0, frames, &e, &f);
        printf("logmel.span_samples.%ld %ld %ld %ld %ld %ld %ld\n", n, a, b, c, d, e, f);
    }

    // general front-end: tables 0-3, and per signal length the shape and the workspace
    const Named configs[] = {{"logmel", {fe::LOGMEL, 512, 160, 400, 80, 0, 0}},
                             {"mel", {fe::MEL, 400, 160, 400, 40, 0, 0}},
                             {"mfcc", {fe::MFCC, 256, 80, 200, 40, 13, 1}},
                             {"spectrogram", {fe::SPECTROGRAM, 128, 64, 128, 0, 0, 0}},
                             {"odd", {fe::LOGMEL, 401, 160, 400, 80, 0, 0}}};
    for (const Named& k : configs) {
        const std::string base = std::string("fe.") + k.name;
        for (int which = 0; which < 4; ++which) print_hash(base + ".table" + std::to_string(which), fe::host_table(k.c, which));
        print_hash(base + ".dft_frag", fe::dft_fragments(fe::geometry(k.c), fe::host_table(k.c, 0)));
        for (long n : {(long)k.c.n_fft / 2 + 1, 4000L, 160000L}) {
            const fe::Shape s = fe::shape(k.c, n);
            const fe::Workspace w = fe::workspace(k.c, n, s.frames);
            printf("%s.shape.%ld %ld %ld %d\n", base.c_str(), n, s.need, s.frames, s.feats);
            printf("%s.ws.%ld %zu %zu %zu %zu %zu\n", base.c_str(), n, w.total, w.gmax, w.sig, w.spec, w.db);
        }
    }

    // resampler: the plan, and the time segments as k0[] | t0[] | s[]
    for (int rate : {8000, 11025, 16001, 22050, 44100, 48000, 96000}) {
        const ingest::Plan p = ingest::plan_for(rate);
        long long k_end = 0;
        const std::vector<ingest::Seg> segs = ingest::time_segments(p.inc, &k_end);
        std::vector<long long> k0;
        std::vector<double> t0, s;
        for (const ingest::Seg& g : segs) {
            k0.push_back(g.k0);
            t0.push_back(g.t0);
            s.push_back(g.s);
        }
        Sha256 sha;
        sha.add(k0.data(), k0.size() * sizeof(long long));
        sha.add(t0.data(), t0.size() * sizeof(double));
        sha.add(s.data(), s.size() * sizeof(double));
        printf("rs.%d.segments %s %zu %lld\n", rate, sha.hex().c_str(), segs.size(), k_end);
        printf("rs.%d.plan %a %a %a %d %d %d %zu %zu\n", rate, p.ratio, p.scale, p.inc, p.step, p.taps, p.span, ingest::lds_bytes(p, true),
               ingest::lds_bytes(p, false));
        long long first, count;
        ingest::span_inputs(p, segs, 3001, 0, (long long)(3001 * p.ratio), &first, &count);
        printf("rs.%d.span_inputs %lld %lld %a\n", rate, first, count, ingest::time_at(segs, 1000));
    }
    return 0;
}
