"""The bf16 arithmetic model (oracle/bf16_model.py) on the CPU: its structure is the fp32 oracle's (rounding off), its
rounding moves it by the bf16 magnitude (rounding on), and each bug planted into it moves it well past the bound at which
tests/test_gpu_bf16_model.py holds the kernels to it -- most of them by less than BF16_TOL, the bound at which the fp32
oracle holds the kernels (tests/test_gpu_parity.py), i.e. bugs that only the model can see."""
import numpy as np
import pytest

from oracle import bf16_model, oracle
from oracle.bf16_model import KERNEL_GAP_BOUND, SHARP_GAP_BOUND

BF16_TOL = 1.2e-2   # tests/test_gpu_parity.py: the fp32-oracle bound of the bf16 path


def seeded(F=80, L=3, seed=1234):
    from voice_activity_detection_amd.seeded import seeded_state_dict

    return seeded_state_dict(seed, feature_size=F, num_layers=L)


def feats(seed, shape):
    from voice_activity_detection_amd.seeded import seeded_features

    return seeded_features(seed, shape)


def qk_x6(st):
    st = {k: v.copy() for k, v in st.items()}
    L = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("encoder.layers."))
    for l in range(L):
        st[f"encoder.layers.{l}.self_attention.query_projection.weight"] *= 6.0
        st[f"encoder.layers.{l}.self_attention.key_projection.weight"] *= 6.0
    return st


def trained():
    from tests.golden.data_files import load_trained
    from voice_activity_detection_amd.seeded import state_dict_spec

    z = load_trained()
    return {k: z["state/" + k] for k, _, _ in state_dict_spec()}


def unrounded_gap(st, x, key_split=False):
    ref = oracle.forward(st, x, threads=16)
    y = bf16_model.forward(st, x, rounding=False, key_split=key_split)
    assert y.shape == ref.shape
    return float(np.abs(y - ref).max())


# ---- a. rounding off: the model's structure (fold, PE, masks, tiles, reference moves, key-split combine) is the oracle's ----
@pytest.mark.parametrize("T", [1, 7, 32, 33, 65, 801])
def test_unrounded_model_is_the_oracle_over_T(T):
    x = feats(10 + T, (2, T, 80))
    assert unrounded_gap(seeded(), x) < 3e-5
    assert unrounded_gap(seeded(), x, key_split=True) < 3e-5


@pytest.mark.parametrize("F", [13, 80, 257])
@pytest.mark.parametrize("L", [1, 3, 6])
def test_unrounded_model_is_the_oracle_over_model_sizes(F, L):
    st = seeded(F, L, seed=50 + F + L)
    for shape in ((5, 7, F), (2, 65, F)):
        assert unrounded_gap(st, feats(F + L + shape[1], shape)) < 3e-5, shape


def test_unrounded_model_is_the_oracle_with_reference_moves():
    st = qk_x6(seeded())
    x = feats(91, (2, 801, 80))
    info = {}
    bf16_model.forward(st, x, rounding=False, info=info)
    assert info["moves"] > 0
    assert unrounded_gap(st, x) < 3e-5
    assert unrounded_gap(st, x, key_split=True) < 3e-5
    assert unrounded_gap(st, feats(92, (9, 7, 80))) < 3e-5


def test_unrounded_model_is_the_oracle_on_trained_weights():
    st = trained()
    assert unrounded_gap(st, feats(93, (40, 7, 80))) < 3e-5
    assert unrounded_gap(st, feats(94, (2, 65, 80))) < 3e-5


# ---- b. rounding on: the bf16 magnitude, and the moves really happen ----------------------------------------------------
def test_rounded_model_differs_by_the_bf16_magnitude():
    st = seeded()
    x = feats(883, (3, 800, 80))
    ref = oracle.forward(st, x, threads=16)
    info = {}
    y = bf16_model.forward(st, x, info=info)
    err = float(np.abs(y - ref).max())
    assert 1e-4 < err < BF16_TOL, err
    assert info["moves"] == 0 and info["saturations"] == 0   # seeded weights: flat softmaxes, small residual stream
    y6 = bf16_model.forward(qk_x6(st), x, info=info)
    assert info["moves"] > 0 and np.isfinite(y6).all()
    # key-split tail frames (the last 32 of 800): with the reference at 0 the same values as the ordinary arithmetic; once the
    # four partial softmaxes move their own references, p is rounded against other references -- a bf16-sized difference
    assert np.abs(bf16_model.forward(st, x, key_split=True) - y).max() < 1e-12
    ks6 = bf16_model.forward(qk_x6(st), x, key_split=True)
    assert 0 < np.abs(ks6 - y6).max() < BF16_TOL


def test_rounded_model_counts_saturations():
    st = seeded()
    st["input_layer.0.weight"] = st["input_layer.0.weight"] * 1.0e4
    info = {}
    y = bf16_model.forward(st, feats(13, (3, 96, 80)), info=info)
    assert np.isfinite(y).all() and info["saturations"] > 0


def test_unknown_plant_is_refused():
    with pytest.raises(ValueError):
        bf16_model.forward(seeded(), feats(1, (1, 7, 80)), plant="nonsense")


# ---- c. the model has to bite ---------------------------------------------------------------------------------------------
def _plant_cases():
    """case -> (state, features, the GPU bound the kernels are held to on that weight set)"""
    st = seeded()
    return {
        "seeded [37,7]": (st, feats(77, (37, 7, 80)), KERNEL_GAP_BOUND),
        "seeded [3,65]": (st, feats(70, (3, 65, 80)), KERNEL_GAP_BOUND),
        "seeded [2,801]": (st, feats(883, (2, 801, 80)), KERNEL_GAP_BOUND),
        "q/k x6 [3,65]": (qk_x6(st), feats(71, (3, 65, 80)), SHARP_GAP_BOUND["q/k x6"]),
        "q/k x6 [2,800]": (qk_x6(st), feats(91, (2, 800, 80)), SHARP_GAP_BOUND["q/k x6"]),
    }


@pytest.fixture(scope="module")
def plant_table():
    """plant -> (largest |plant - model| in units of that case's GPU bound, largest |plant - fp32 oracle|) over the cases"""
    cases = _plant_cases()
    base = {c: bf16_model.forward(s, x) for c, (s, x, _) in cases.items()}
    ref = {c: oracle.forward(s, x, threads=16) for c, (s, x, _) in cases.items()}
    table = {}
    for p in bf16_model.PLANTS:
        ys = {c: bf16_model.forward(s, x, plant=p) for c, (s, x, _) in cases.items()}
        table[p] = (max(float(np.abs(ys[c] - base[c]).max()) / cases[c][2] for c in cases),
                    max(float(np.abs(ys[c] - ref[c]).max()) for c in cases))
    return table


# planted bugs that move the model by more than 3x the GPU bound on some case: the GPU comparison catches them in a kernel
BITES = {"tail_drop_key", "residual_bf16", "pe_shift", "move_no_rescale_l", "move_half_l", "move_half_o"}
# ... and of those, the ones whose distance to the fp32 oracle stays under BF16_TOL on every case: the existing tests miss them
MISSED_BY_BF16_TOL = {"pe_shift", "residual_bf16"}


@pytest.mark.parametrize("plant", sorted(BITES))
def test_planted_bug_moves_the_model_past_three_times_the_gpu_bound(plant_table, plant):
    bite, _ = plant_table[plant]
    assert bite > 3, (plant, bite)


def test_planted_bugs_table(plant_table, capsys):
    with capsys.disabled():
        print(f"\nplanted bug               vs model (x GPU bound)  vs fp32 oracle   (BF16_TOL {BF16_TOL:.1e})")
        for p, (bite, to_ref) in plant_table.items():
            print(f"  {p:24s} {bite:8.2f}               {to_ref:.2e}{'   missed by BF16_TOL' if to_ref < BF16_TOL else ''}")
        bites = {p for p, (b, _) in plant_table.items() if b > 3}
        missed = {p for p in bites if plant_table[p][1] < BF16_TOL}
        print(f"  {len(bites)} of {len(plant_table)} planted bugs move the model past 3x the GPU bound; {len(missed)} of those stay "
              f"under BF16_TOL against the fp32 oracle; {sum(1 for _, r in plant_table.values() if r < BF16_TOL)} of all {len(plant_table)} do")
    assert bites == BITES and len(bites) >= 5
    assert missed == MISSED_BY_BF16_TOL
