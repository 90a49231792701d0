"""The key projection folded into the query (csrc/savad_kernels_f32s.h: fold_qk_kernel), restated in numpy fp64 exactly as the
kernel's comment states it, the LayerNorm fold (fold_ln_kernel) included:

    Wq' = Wq diag(gamma), bq' = bq + Wq beta   (the same for k),   c = log2(e) / sqrt(D)
    Wq~[n][k] = c sum_o Wk'[o][n] Wq'[o][k],   bq~[n] = c sum_o Wk'[o][n] bq'[o]

With x^ the normalised rows (LayerNorm without its affine), the base-2 softmax over the keys of (Wq~ x^_i + bq~) . x^_j is the
reference's softmax of q_i . k_j / sqrt(D) (vad/modeling/transformer.py:351-363): the term the fold drops is the same for every key
of a row.  Held to 1e-12 for every layer of the seeded and the trained weights, and of seeded weights whose q / k biases are large."""
import numpy as np
import pytest

D = 128
LOG2E = 1.4426950408889634


def layer(state, l):
    p = f"encoder.layers.{l}."
    g = lambda k: state[p + k].astype(np.float64)
    return (g("self_attention.query_projection.weight"), g("self_attention.query_projection.bias"),
            g("self_attention.key_projection.weight"), g("self_attention.key_projection.bias"),
            g("self_attention_sublayer.layer_norm.weight"), g("self_attention_sublayer.layer_norm.bias"))


def folded_query(Wq, bq, Wk, bk, gamma, beta):
    """Wq~, bq~ as fold_qk_kernel builds them from the LayerNorm-folded projections"""
    Wq_, bq_ = Wq * gamma[None, :], bq + Wq @ beta
    Wk_ = Wk * gamma[None, :]
    c = LOG2E / np.sqrt(D)
    Wqt = np.empty((D, D))
    bqt = np.empty(D)
    for n in range(D):
        Wqt[n] = c * (Wk_[:, n][:, None] * Wq_).sum(axis=0)
        bqt[n] = c * (Wk_[:, n] * bq_).sum()
    return Wqt, bqt


def normalised_rows(seed, T):
    h = np.random.default_rng(seed).standard_normal((T, D)) * 3.0 + 0.5
    d = h - h.mean(axis=1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=1, keepdims=True) + 1e-5)


def softmax(s, base2=False):
    s = s - s.max(axis=1, keepdims=True)
    e = np.exp2(s) if base2 else np.exp(s)
    return e / e.sum(axis=1, keepdims=True)


def check(state, tag):
    for l in range(3):
        Wq, bq, Wk, bk, gamma, beta = layer(state, l)
        xh = normalised_rows(10 + l, 70)
        y = xh * gamma + beta                                   # what the reference's projections see
        plain = softmax((y @ Wq.T + bq) @ (y @ Wk.T + bk).T / np.sqrt(D))
        Wqt, bqt = folded_query(Wq, bq, Wk, bk, gamma, beta)
        folded = softmax((xh @ Wqt.T + bqt) @ xh.T, base2=True)    # the key is the normalised row itself
        err = float(np.abs(folded - plain).max())
        print(f"{tag}, layer {l}: max |dP| = {err:.2e}")
        assert err < 1e-12, (tag, l, err)


def test_folded_scores_on_seeded_weights():
    from voice_activity_detection_amd.seeded import seeded_state_dict

    check(seeded_state_dict(1234), "seeded 1234")
    check(seeded_state_dict(77, gain=4.0), "seeded 77, gain 4")


def test_folded_scores_on_trained_weights():
    from tests.golden.data_files import load_trained

    z = load_trained()
    check({k[len("state/"):]: v for k, v in z.items() if k.startswith("state/")}, "trained")


def test_folded_scores_with_large_query_and_key_biases():
    from voice_activity_detection_amd.seeded import seeded_state_dict

    st = seeded_state_dict(4321)
    for k in st:
        if k.endswith("query_projection.bias") or k.endswith("key_projection.bias"):
            st[k] = (st[k] * np.float32(64.0)).astype(np.float32)
    check(st, "q / k biases x 64")
