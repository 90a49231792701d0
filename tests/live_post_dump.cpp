// The streaming rules of voice_activity_detection_amd/csrc/savad_live_post.h held to the offline arithmetic of savad_post_device.h,
// exhaustively, for tests/test_live_post_host.py.  Host code only: no HIP call is made.
//   live_post_dump exhaustive <max_len>
// Every 0/1 row string of length 1 .. max_len (W = 1 probs 0.25 / 0.75, threshold 0.5), (v, h, b, o) in {0, 1, 3}^4, cut into ticks
// as: one row per tick then an empty finish; everything in the finish tick; every two-cut split (empty ticks included).  For every
// run: the events so far are a prefix of the offline segments after every tick and all of them after the finish; every tick meets
// the promptness rule (an event at sample s is out once 160 (R - v - h - b) > s + 1); no entry emits more than event_cap events.
// Prints "OK <runs> <events>" or the first failure.
#include "savad_live_post.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace savad;
namespace lp = savad::livepost;

struct Ev {
    int kind;
    long sample;
};

// the offline path: trim over the whole string, the class of EVERY sample, convert_samples_to_segments
static std::vector<Ev> offline(const std::vector<uint8_t>& raw, const lp::Params& p) {
    const int n = (int)raw.size();
    std::vector<uint8_t> s(raw);
    std::vector<int> last(n), next(n);
    postdev::trim_host(s.data(), n, p.v, p.h, p.b, p.o, last.data(), next.data());
    const postdev::Geometry g = postdev::make_geometry(n, 16000, 10.0, 25.0);
    std::vector<Ev> out;
    bool voice = false;
    for (long i = 0; i < g.num; ++i) {
        const uint8_t c = postdev::sample_class(s.data(), g, i);
        if (c == postdev::ONE && !voice) out.push_back(Ev{lp::START, i}), voice = true;
        else if (c == postdev::ZERO && voice) out.push_back(Ev{lp::END, i - 1}), voice = false;
    }
    if (voice) out.push_back(Ev{lp::END, g.num - 1});
    return out;
}

static long g_runs = 0, g_events = 0;

static bool fail(const char* what, const std::vector<uint8_t>& raw, const lp::Params& p, const std::vector<int>& cuts) {
    printf("FAIL %s: rows ", what);
    for (uint8_t r : raw) printf("%d", r);
    printf(" params %d %d %d %d cuts", p.v, p.h, p.b, p.o);
    for (int c : cuts) printf(" %d", c);
    printf("\n");
    return false;
}

// cuts: row counts of the ticks; the last one is the finish tick
static bool run(const std::vector<uint8_t>& raw, const std::vector<float>& probs, const lp::Params& p, const std::vector<Ev>& want,
                const std::vector<int>& cuts) {
    lp::State st;
    memset(&st, 0xAB, sizeof st);   // the state needs no initialisation
    std::vector<Ev> got;
    std::vector<lp::Event> buf(64);
    long fed = 0;
    for (size_t t = 0; t < cuts.size(); ++t) {
        const bool fin = t + 1 == cuts.size();
        const int cap = lp::event_cap(cuts[t], p);
        if ((int)buf.size() < cap) buf.resize(cap);
        const int n = lp::run_host(&st, p, 5, fed, cuts[t], fin, probs.data() + fed, buf.data(), cap);
        if (n < 0) return fail("refused", raw, p, cuts);
        if (n > cap) return fail("more events than event_cap", raw, p, cuts);
        for (int k = 0; k < n; ++k) {
            if (buf[k].slot != 5) return fail("slot", raw, p, cuts);
            got.push_back(Ev{buf[k].kind, (long)buf[k].sample});
        }
        fed += cuts[t];
        if (got.size() > want.size()) return fail("more events than offline", raw, p, cuts);
        for (size_t k = 0; k < got.size(); ++k)
            if (got[k].kind != want[k].kind || got[k].sample != want[k].sample) return fail("event differs", raw, p, cuts);
        if (!fin) {
            const long bound = 160L * (fed - p.v - p.h - p.b);
            size_t due = 0;
            while (due < want.size() && bound > want[due].sample + 1) ++due;
            if (got.size() < due) return fail("late", raw, p, cuts);
        }
    }
    if (got.size() != want.size()) return fail("events missing after the finish", raw, p, cuts);
    if (st.next_row != -1) return fail("state not closed", raw, p, cuts);
    // a closed state refuses a continuation and stays as it is
    lp::State before = st;
    if (lp::run_host(&st, p, 5, fed, 0, 0, probs.data(), buf.data(), 0) != -1 || memcmp(&before, &st, sizeof st)) return fail("skip", raw, p, cuts);
    ++g_runs, g_events += (long)got.size();
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3 || std::string(argv[1]) != "exhaustive") return 2;
    const int max_len = atoi(argv[2]);
    const int vals[3] = {0, 1, 3};
    for (int len = 1; len <= max_len; ++len)
        for (unsigned bits = 0; bits < (1u << len); ++bits) {
            std::vector<uint8_t> raw(len);
            std::vector<float> probs(len);
            for (int i = 0; i < len; ++i) raw[i] = (bits >> i) & 1, probs[i] = raw[i] ? 0.75f : 0.25f;
            for (int q = 0; q < 81; ++q) {
                const lp::Params p{1, 0.5f, vals[q % 3], vals[q / 3 % 3], vals[q / 9 % 3], vals[q / 27]};
                const std::vector<Ev> want = offline(raw, p);
                std::vector<int> cuts(len, 1);
                cuts.push_back(0);
                if (!run(raw, probs, p, want, cuts)) return 1;
                if (!run(raw, probs, p, want, {len})) return 1;
                for (int a = 0; a <= len; ++a)
                    for (int b = a; b <= len; ++b)
                        if (!run(raw, probs, p, want, {a, b - a, len - b})) return 1;
            }
        }
    printf("OK %ld %ld\n", g_runs, g_events);
    return 0;
}
