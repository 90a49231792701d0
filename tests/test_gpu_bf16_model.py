"""The bf16 kernels against a reference of the SAME arithmetic (oracle/bf16_model.py: operands rounded where the kernels round
them, everything else float64), at one tight bound, KERNEL_GAP_BOUND.  The fp32 oracle can only hold the bf16 path to its own
rounding noise (BF16_TOL = 1.2e-2 in tests/test_gpu_parity.py); against the model what is left is summation order and the
rare rounding flip it causes, so a bug in code every launch schedule shares -- fragment packing, the online softmax, the
residual parking, the LayerNorm fold, the classifier tail -- shows even when it is smaller than bf16's own rounding
(tests/test_bf16_model.py plants such bugs into the model and checks that each one moves the output past this bound).

Measured on an MI355X (scripts/ubench/bf16_model_gap.py), max |dlogp| kernel vs model per case group (mean |dlogp| after it):
    schedules T>32 5.0e-4 (3.8e-5)   packed T<=32 5.3e-4 (3.1e-5)   bf16 inputs 5.0e-4 (4.7e-5)   model sizes 7.1e-4 (1.2e-4, L = 6)
    saturation x1e4 2.2e-5 (1.6e-7)  config2 sample 4.8e-4 (4.1e-5) predictor (probabilities) 2.1e-4 (6.2e-6)
    q/k x6 1.9e-3 (6.0e-5)           trained clip 4.2e-2 (3.1e-4)
KERNEL_GAP_BOUND = 1.5e-3 is 2x the largest seeded-weight group.  The sharp-softmax weight sets get 2x their own (SHARP_GAP_BOUND):
the gap is the rounding-flip floor of this arithmetic, not a missed rounding point -- the model evaluated in fp32 instead of
float64 differs from itself by as much (seeded 4e-4 .. 7e-4, x6 2.3e-3, trained 2.1e-2), and a sharp softmax or a confident
classifier (|log p| up to 9 on the trained clip) amplifies every flip.  Key-split tail frames of the persistent attention kernel
(row_mode 5 and the automatic schedule of large batches) are compared with the model's key_split=True: no separate bound."""
import numpy as np
import pytest

from oracle.bf16_model import KERNEL_GAP_BOUND, SHARP_GAP_BOUND

pytestmark = pytest.mark.gpu

BOUND = KERNEL_GAP_BOUND


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


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


def trained_state():
    from tests.golden.data_files import load_trained
    from voice_activity_detection_amd.seeded import state_dict_spec

    z = load_trained()
    return {k: z["state/" + k] for k, _, _ in state_dict_spec()}


def clip_windows():
    """the 984 seven-frame windows of the reference's test clip (the oracle's log-mel)"""
    from oracle import logmel
    from tests.golden.data_files import data_root
    from voice_activity_detection_amd.features import load_wav_mono16k

    audio = load_wav_mono16k(data_root() / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav")
    feat = logmel.log_mel(audio).astype(np.float32)
    off = np.array([-19, -10, -1, 0, 1, 10, 19])
    return np.ascontiguousarray(feat[np.arange(19, len(feat) - 19)[:, None] + off[None, :]])


_MODELS = {}


def gpu_model(torch, st, key):
    from voice_activity_detection_amd import SelfAttentiveVAD

    if key not in _MODELS:
        F = st["input_layer.0.weight"].shape[1]
        L = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("encoder.layers."))
        m = SelfAttentiveVAD(F, L, 128, 0.5)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        _MODELS[key] = m.to("cuda").eval()
    return _MODELS[key]


def run(torch, m, x, row_mode=0, batch_invariant=False, bf16_input=False):
    m.precision, m.row_mode, m.batch_invariant = "bf16", row_mode, batch_invariant
    try:
        t = torch.from_numpy(x).to("cuda")
        if bf16_input:
            t = t.to(torch.bfloat16)
        with torch.no_grad():
            y = m(features=t)
        torch.cuda.synchronize()
    finally:
        m.precision, m.row_mode, m.batch_invariant = "fp32", 0, False
    return y.cpu().numpy()


def model_out(st, x, key_split=False, info=None):
    from oracle import bf16_model

    return bf16_model.forward(st, x, key_split=key_split, info=info)


def gap(got, want):
    """(max, mean) of |kernel - model| over every log-prob of the case"""
    assert got.shape == want.shape and np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - want)
    return float(d.max()), float(d.mean())


# ---- the cases: each returns [(label, kernel - model gap)], the probe prints them, the tests bound them ------------------------
def pw_splits(T):
    """row_mode 5 without batch_invariant computes a tail group of one or two query blocks as a key-split item"""
    return ((T + 31) // 32) % 8 in (1, 2)


def case_schedules(torch, T):
    """T > 32: every launch schedule, with and without batch_invariant"""
    st = seeded()
    m = gpu_model(torch, st, "seeded")
    B = 1 if T >= 3200 else 2
    x = feats(1000 + T, (B, T, 80))
    want = model_out(st, x)
    want_ks = model_out(st, x, key_split=True) if pw_splits(T) else want
    out = []
    for rm in (0, 1, 2, 3, 5):
        for bi in (False, True):
            w = want_ks if (rm == 5 and not bi) else want
            out.append((f"T{T} rm{rm} bi{int(bi)}", *gap(run(torch, m, x, rm, bi), w)))
    return out


def case_packed(torch, T):
    """T <= 32: the per-layer launches and every variant of the single launch, batches that leave partial packed blocks"""
    st = seeded()
    m = gpu_model(torch, st, "seeded")
    out = []
    for B in (37, 3):
        x = feats(2000 + T + B, (B, T, 80))
        want = model_out(st, x)
        for rm in (0, 1, 4, 5, 6, 7, 8):
            out.append((f"[{B},{T}] rm{rm}", *gap(run(torch, m, x, rm), want)))
    return out


def case_inputs(torch):
    """bf16 input tensors (rounding the features is then the identity), fp32 and bf16 at T <= 32 and T > 32"""
    st = seeded()
    m = gpu_model(torch, st, "seeded")
    out = []
    for shape in ((4, 96, 80), (40, 7, 80), (3, 801, 80)):
        x = feats(3000 + sum(shape), shape)
        xb = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        want = model_out(st, xb)
        for rm in (0, 1):
            out.append((f"{list(shape)} bf16-in rm{rm}", *gap(run(torch, m, x, rm, bf16_input=True), want)))
    return out


def case_model_sizes(torch, F, L):
    st = seeded(F=F, L=L, seed=40 + F + L)
    m = gpu_model(torch, st, f"F{F}L{L}")
    out = []
    for shape in ((9, 7, F), (3, 65, F)):
        x = feats(4000 + F + L + shape[1], shape)
        want = model_out(st, x)
        for rm in (0, 1):
            out.append((f"F{F} L{L} {list(shape)} rm{rm}", *gap(run(torch, m, x, rm), want)))
    return out


def case_qk_x6(torch):
    """q / k weights x6: the reference moves on most rows of most tiles"""
    st = qk_x6(seeded())
    m = gpu_model(torch, st, "x6")
    out = []
    for shape in ((3, 800, 80), (37, 7, 80)):
        x = feats(91 + shape[1], shape)
        info = {}
        want = model_out(st, x, info=info)
        assert info["moves"] > 0
        want_ks = model_out(st, x, key_split=True) if shape[1] > 32 and pw_splits(shape[1]) else want
        for rm in ((1, 3, 5) if shape[1] > 32 else (0, 1)):
            out.append((f"x6 {list(shape)} rm{rm}", *gap(run(torch, m, x, rm), want_ks if rm == 5 else want)))
    return out


def case_trained(torch):
    """the trained weights (peaked softmaxes, confident decisions) on the clip's 984 windows"""
    st = trained_state()
    m = gpu_model(torch, st, "trained")
    x = clip_windows()
    want = model_out(st, x)
    return [(f"trained clip rm{rm}", *gap(run(torch, m, x, rm), want)) for rm in (0, 1, 8)]


def case_saturation(torch):
    """input projection x1e4: the parked residual stream clamps at +-65504 -- the values must be the clamping model's"""
    st = seeded()
    st["input_layer.0.weight"] = st["input_layer.0.weight"] * 1.0e4
    m = gpu_model(torch, st, "x1e4")
    out = []
    for shape in ((3, 96, 80), (40, 7, 80)):
        x = feats(13 + shape[1], shape)
        info = {}
        want = model_out(st, x, info=info)
        assert info["saturations"] > 0
        for rm in (0, 1):
            m.residual_saturations()
            y = run(torch, m, x, rm)
            assert m.residual_saturations() > 0
            out.append((f"x1e4 {list(shape)} rm{rm}", *gap(y, want)))
    return out


def case_config2(torch):
    """[256,800,80] under the automatic schedule (the persistent key-split attention): a sample of the sequences"""
    st = seeded()
    m = gpu_model(torch, st, "seeded")
    x = feats(4242, (256, 800, 80))
    y = run(torch, m, x)
    pick = np.array(sorted({0, 255, 7, 128} | set(np.random.default_rng(5).choice(256, 3, replace=False).tolist())))
    want = model_out(st, x[pick], key_split=True)
    return [(f"[256,800] auto seq {int(b)}", *gap(y[b], want[i])) for i, b in enumerate(pick)]


def case_predictor(torch):
    """predict_windows (windows read in place by the single launch, boosted) against gather -> model -> boost"""
    from oracle import oracle
    from voice_activity_detection_amd import VADFromScratchPredictor

    st = seeded()
    m = gpu_model(torch, st, "seeded")
    out = []
    for n, seed in ((1022, 500), (39, 502)):
        feat = feats(seed, (n, 80))
        m.precision = "bf16"
        try:
            probs = VADFromScratchPredictor(m, "cuda").predict_probabilities(feat)
        finally:
            m.precision = "fp32"
        count = n - 2 * 19
        win, pos = oracle.gather_windows(feat, 19, 9, 0, count)
        want, _ = oracle.boost(model_out(st, win).astype(np.float32), pos, n)
        assert np.array_equal(probs == 0.5, want == 0.5)
        out.append((f"predictor n={n}", *gap(probs, want.astype(np.float64))))
    return out


T_SCHEDULES = [33, 48, 65, 264, 800, 801, 833, 3200]
T_PACKED = [1, 3, 7, 16, 31, 32]
SIZES = [(13, 3), (40, 3), (257, 3), (80, 1), (80, 2), (80, 6)]

GROUPS = {   # case group -> the case calls it is made of (scripts/ubench/bf16_model_gap.py walks these)
    "schedules T>32": [(case_schedules, (T,)) for T in T_SCHEDULES],
    "packed T<=32": [(case_packed, (T,)) for T in T_PACKED],
    "bf16 inputs": [(case_inputs, ())],
    "model sizes": [(case_model_sizes, fl) for fl in SIZES],
    "q/k x6": [(case_qk_x6, ())],
    "trained clip": [(case_trained, ())],
    "saturation x1e4": [(case_saturation, ())],
    "config2 sample": [(case_config2, ())],
    "predictor": [(case_predictor, ())],
}


def check(results, bound=BOUND):
    bad = [(k, mx) for k, mx, _ in results if not mx < bound]
    assert not bad, f"kernel vs bf16 model beyond {bound}: {bad}"


@pytest.mark.parametrize("T", T_SCHEDULES)
def test_schedules_above_32_frames(torch_cuda, T):
    check(case_schedules(torch_cuda, T))


@pytest.mark.parametrize("T", T_PACKED)
def test_packed_single_launch(torch_cuda, T):
    check(case_packed(torch_cuda, T))


def test_bf16_input_tensors(torch_cuda):
    check(case_inputs(torch_cuda))


@pytest.mark.parametrize("F,L", SIZES)
def test_other_model_sizes(torch_cuda, F, L):
    check(case_model_sizes(torch_cuda, F, L))


def test_reference_moves(torch_cuda):
    check(case_qk_x6(torch_cuda), SHARP_GAP_BOUND["q/k x6"])


def test_trained_weights_on_the_clip(torch_cuda):
    check(case_trained(torch_cuda), SHARP_GAP_BOUND["trained clip"])


def test_residual_saturation_values(torch_cuda):
    check(case_saturation(torch_cuda))


def test_config2_automatic_sample(torch_cuda):
    check(case_config2(torch_cuda))


def test_predictor_level(torch_cuda):
    check(case_predictor(torch_cuda))


def test_a_planted_bug_fails_the_bound(torch_cuda):
    """the comparison bites on the GPU too: the kernel against the model with one planted bug is beyond the bound"""
    from oracle import bf16_model

    st = seeded()
    m = gpu_model(torch_cuda, st, "seeded")
    x = feats(1065, (37, 7, 80))
    y = run(torch_cuda, m, x)
    assert gap(y, model_out(st, x))[0] < BOUND
    assert gap(y, bf16_model.forward(st, x, plant="tail_drop_key"))[0] > 3 * BOUND
