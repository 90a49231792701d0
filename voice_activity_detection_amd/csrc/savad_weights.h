// savad_weights.h -- where every weight of a handle lies, decided once: the state_dict inventory with the offset of each tensor in the
// raw buffer, the LayerNorm-folded fp32 buffer of the d_model = 128 kernels, and the fragment images (bf16: 2 bytes per element,
// fp32s: three bf16 pieces, 6 bytes).  make_layout is a pure function of (feature_size, num_layers, d_model); savad.hip allocates
// from its totals and reads the offsets, and tests/weights_dump.cpp prints them (tests/test_weights_layout_host.py).
// Plain C++17: no HIP, no device code.  A further operand format is one more FragLayout, nothing else.
#pragma once

#include <stddef.h>

#include <string>
#include <vector>

#include "savad_dims.h"

namespace savad {
namespace weights {

struct Param {
    std::string key;
    size_t numel;
    size_t off;  // float offset into the raw buffer
};

// float offsets into the raw buffer (the parameters exactly as handed over)
struct LayerRaw {
    size_t wq, bq, wk, bk, wv, bv, wo, bo, ln1w, ln1b, w1, b1, w2, b2, ln2w, ln2b;
};
// float offsets into the packed buffer (LayerNorm affine folded in)
struct LayerPacked {
    size_t wqkv, bqkv, w1, b1;
    size_t wq_vo, bq_vo;  // fp32s, T > 32: Wq~ | Wo Wv' [2 D][D] and bq~ | Wo bv' (fold_qk_kernel, fold_vo_kernel)
    size_t frag;          // the layer's matrices in fragment order (packed_forward_kernel)
};
// byte offsets into a fragment image
struct LayerFrag {
    size_t wqkv, wo, w1, w2;
    size_t wq_vo;  // folded images only: Wq~ | Wo Wv' (the key projection folded into Q, the out-projection into V)
};

struct FragLayout {
    int elem_bytes = 0;   // 2 = bf16, 6 = fp32s
    bool folded = false;  // a second Q / V image per layer (wq_vo)
    size_t win = 0;       // [D][FP]
    std::vector<LayerFrag> layer;
    size_t bytes = 0;
};

inline FragLayout frag_layout(int FP, int L, int elem_bytes, bool folded) {
    FragLayout f;
    f.elem_bytes = elem_bytes;
    f.folded = folded;
    const size_t e = (size_t)elem_bytes;
    auto take = [&f](size_t bytes) {
        const size_t at = f.bytes;
        f.bytes += bytes;
        return at;
    };
    f.win = take((size_t)D * FP * e);
    f.layer.resize(L);
    for (LayerFrag& l : f.layer) {
        l.wqkv = take((size_t)3 * D * D * e);
        l.wo = take((size_t)D * D * e);
        l.w1 = take((size_t)DFF * D * e);
        l.w2 = take((size_t)D * DFF * e);
        l.wq_vo = folded ? take((size_t)2 * D * D * e) : 0;
    }
    return f;
}

struct Layout {
    bool generic = false;  // d_model != 128: the raw parameters alone (savad_generic.h reads them as they are)
    int FP = 0;            // feature size rounded up to a multiple of 16 (kernels' K granularity); generic: the feature size
    // raw buffer: the state_dict inventory in the order of seeded.state_dict_spec, every tensor on a multiple of 4 floats
    std::vector<Param> params;
    size_t raw_floats = 0;
    size_t r_win = 0, r_bin = 0, r_lnf_w = 0, r_lnf_b = 0, r_wc = 0, r_bc = 0;
    std::vector<LayerRaw> lr;
    // packed buffer (not generic)
    size_t packed_floats = 0;
    std::vector<LayerPacked> lp;
    size_t p_bias = 0;     // [L][LBIAS] b1' | b2 | bqkv' | bo (packed_forward_kernel stages them in one sweep)
    size_t p_wc = 0, p_bc = 0;
    size_t p_win_pad = 0;  // [D][FP] zero-padded copy of input_layer.0.weight (read only when FP != feature_size)
    // fragment images (not generic)
    FragLayout bf16, f32s;
};

inline Layout make_layout(int feature_size, int num_layers, int d_model) {
    Layout w;
    w.generic = d_model != D;
    const size_t d = (size_t)d_model, h = 4 * d;  // d_ff = 4 d_model: vad/models/self_attention.py:10
    const int F = feature_size, L = num_layers;
    auto param = [&w](const std::string& key, size_t numel) {
        const size_t off = w.raw_floats;
        w.params.push_back(Param{key, numel, off});
        w.raw_floats += (numel + 3) & ~size_t(3);  // keep every tensor 16-byte aligned
        return off;
    };
    // state_dict inventory: SURVEY.md section 8a / vad/models/self_attention.py:7-21
    static const struct {
        const char* name;
        size_t LayerRaw::*at;
        bool rows_ff, matrix, cols_ff;  // [rows] or [rows][cols], each d_model or d_ff long
    } layer_tensors[] = {
        {"self_attention.query_projection.weight", &LayerRaw::wq, false, true, false},
        {"self_attention.query_projection.bias", &LayerRaw::bq, false, false, false},
        {"self_attention.key_projection.weight", &LayerRaw::wk, false, true, false},
        {"self_attention.key_projection.bias", &LayerRaw::bk, false, false, false},
        {"self_attention.value_projection.weight", &LayerRaw::wv, false, true, false},
        {"self_attention.value_projection.bias", &LayerRaw::bv, false, false, false},
        {"self_attention.final_projection.weight", &LayerRaw::wo, false, true, false},
        {"self_attention.final_projection.bias", &LayerRaw::bo, false, false, false},
        {"self_attention_sublayer.layer_norm.weight", &LayerRaw::ln1w, false, false, false},
        {"self_attention_sublayer.layer_norm.bias", &LayerRaw::ln1b, false, false, false},
        {"feed_forward.feed_forward.0.weight", &LayerRaw::w1, true, true, false},
        {"feed_forward.feed_forward.0.bias", &LayerRaw::b1, true, false, false},
        {"feed_forward.feed_forward.3.weight", &LayerRaw::w2, false, true, true},
        {"feed_forward.feed_forward.3.bias", &LayerRaw::b2, false, false, false},
        {"feed_forward_sublayer.layer_norm.weight", &LayerRaw::ln2w, false, false, false},
        {"feed_forward_sublayer.layer_norm.bias", &LayerRaw::ln2b, false, false, false},
    };
    w.r_win = param("input_layer.0.weight", d * F);
    w.r_bin = param("input_layer.0.bias", d);
    w.lr.resize(L);
    for (int l = 0; l < L; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        for (const auto& t : layer_tensors) w.lr[l].*t.at = param(p + t.name, (t.rows_ff ? h : d) * (t.matrix ? (t.cols_ff ? h : d) : 1));
    }
    w.r_lnf_w = param("encoder.layer_norm.weight", d);
    w.r_lnf_b = param("encoder.layer_norm.bias", d);
    w.r_wc = param("classifier.weight", 2 * d);
    w.r_bc = param("classifier.bias", 2);
    w.FP = w.generic ? F : (F + 15) / 16 * 16;
    if (w.generic) return w;

    auto packed = [&w](size_t floats) {
        const size_t at = w.packed_floats;
        w.packed_floats += floats;
        return at;
    };
    w.lp.resize(L);
    for (LayerPacked& q : w.lp) {
        q.wqkv = packed((size_t)3 * D * D);
        q.bqkv = packed(3 * D);
        q.w1 = packed((size_t)DFF * D);
        q.b1 = packed(DFF);
        q.wq_vo = packed((size_t)2 * D * D);
        q.bq_vo = packed(2 * D);
        q.frag = packed(FRAG_LAYER);
    }
    w.p_bias = packed((size_t)L * LBIAS);
    w.p_wc = packed(2 * D);
    w.p_bc = packed(4);
    w.p_win_pad = packed((size_t)D * w.FP);
    w.bf16 = frag_layout(w.FP, L, 2, false);
    w.f32s = frag_layout(w.FP, L, 6, true);
    return w;
}

}  // namespace weights
}  // namespace savad
