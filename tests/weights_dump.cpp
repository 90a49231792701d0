// Prints the weight layout (voice_activity_detection_amd/csrc/savad_weights.h) of a fixed list of configurations: the parameter
// inventory with every raw offset, the packed fp32 buffer and both fragment images.  tests/test_weights_layout_host.py recomputes
// every number from the formulas and compares.  Host C++ only.
//   C <F> <L> <d_model> generic<0|1> FP<n> raw<floats> packed<floats>
//   P <key> <numel> <float offset>                                  (inventory order)
//   R <name> <float offset>                                         (the same offsets by the name savad.hip reads them under)
//   K <name> <float offset>                                         (packed buffer; layer entries carry the layer number)
//   I <image> e<bytes per element> folded<0|1> bytes<total>, then  G <image> <name> <byte offset>
#include "savad_weights.h"

#include <stdio.h>

using namespace savad::weights;

static void image(const char* name, const FragLayout& f) {
    printf("I %s e%d folded%d bytes%zu\n", name, f.elem_bytes, (int)f.folded, f.bytes);
    printf("G %s win %zu\n", name, f.win);
    for (size_t l = 0; l < f.layer.size(); ++l) {
        const LayerFrag& a = f.layer[l];
        printf("G %s %zu.wqkv %zu\nG %s %zu.wo %zu\nG %s %zu.w1 %zu\nG %s %zu.w2 %zu\n", name, l, a.wqkv, name, l, a.wo, name, l, a.w1, name, l, a.w2);
        if (f.folded) printf("G %s %zu.wq_vo %zu\n", name, l, a.wq_vo);
    }
}

static void dump(int F, int L, int d_model) {
    const Layout w = make_layout(F, L, d_model);
    printf("C %d %d %d generic%d FP%d raw%zu packed%zu\n", F, L, d_model, (int)w.generic, w.FP, w.raw_floats, w.packed_floats);
    for (const Param& p : w.params) printf("P %s %zu %zu\n", p.key.c_str(), p.numel, p.off);
    printf("R win %zu\nR bin %zu\n", w.r_win, w.r_bin);
    for (size_t l = 0; l < w.lr.size(); ++l) {
        const LayerRaw& r = w.lr[l];
        const struct { const char* name; size_t off; } f[] = {
            {"wq", r.wq}, {"bq", r.bq}, {"wk", r.wk}, {"bk", r.bk}, {"wv", r.wv}, {"bv", r.bv}, {"wo", r.wo}, {"bo", r.bo},
            {"ln1w", r.ln1w}, {"ln1b", r.ln1b}, {"w1", r.w1}, {"b1", r.b1}, {"w2", r.w2}, {"b2", r.b2}, {"ln2w", r.ln2w}, {"ln2b", r.ln2b}};
        for (const auto& e : f) printf("R %zu.%s %zu\n", l, e.name, e.off);
    }
    printf("R lnf_w %zu\nR lnf_b %zu\nR wc %zu\nR bc %zu\n", w.r_lnf_w, w.r_lnf_b, w.r_wc, w.r_bc);
    if (w.generic) return;
    for (size_t l = 0; l < w.lp.size(); ++l) {
        const LayerPacked& q = w.lp[l];
        const struct { const char* name; size_t off; } f[] = {{"wqkv", q.wqkv}, {"bqkv", q.bqkv}, {"w1", q.w1}, {"b1", q.b1},
                                                               {"wq_vo", q.wq_vo}, {"bq_vo", q.bq_vo}, {"frag", q.frag}};
        for (const auto& e : f) printf("K %zu.%s %zu\n", l, e.name, e.off);
    }
    printf("K bias %zu\nK wc %zu\nK bc %zu\nK win_pad %zu\n", w.p_bias, w.p_wc, w.p_bc, w.p_win_pad);
    image("bf16", w.bf16);
    image("f32s", w.f32s);
}

int main() {
    const int cases[][3] = {{80, 3, 128}, {40, 3, 128}, {13, 1, 128}, {257, 2, 128}, {80, 6, 128}, {80, 8, 128}, {80, 3, 64}, {20, 2, 130}, {80, 1, 2}};
    for (const auto& c : cases) dump(c[0], c[1], c[2]);
    return 0;
}
