"""The forwards in the numeric regimes of tests/numeric_regimes.py: states and inputs in which the LayerNorm epsilon, the two-pass
variance, the sign and the zeros of a LayerNorm weight and the row maximum of the softmax each carry a visible share of the result
(tests/test_numeric_regimes_host.py asserts that on the CPU: a restatement of the reference with that one piece changed moves the
float64 truth by at least 4 x the bound used here).  In the regime of every other parity test none of them moves an output by TIGHT.

fp32 paths -- the three modes `fp32_mode` of tests/test_gpu_parity.py stands for (fp32, fp32s under its automatic schedule, fp32s with
its own kernels pinned) and the other row modes the shape admits, so that every LayerNorm site of csrc/savad_kernels.h,
savad_kernels_f32s.h and savad_device.h is entered; d_model 64 through savad_generic.h -- against the float64 truth
(oracle/torch_port.py on double tensors, pinned to the reference's own float64 outputs) at bound = max(TIGHT, 3 x fp32 floor), the
floor computed here from two plain fp32 evaluations on the CPU, never from a kernel.  One test per path.  In `offset` the paths
named in nr.OFFSET_RESIDUAL_CHAIN_PATHS (every path at (4, 7, 80); the fp32s kernels, the M-split row kernel and the fused
attention + row chain at the longer shapes) are outside that bound for an arithmetic reason -- GEMM accumulators that start at
the residual stream -- and are held to 3 x the floor of that accumulation order instead (nr.chained_port, a CPU restatement;
capped and shown to expose the one-pass variance by the host test): measured 4.8e-5 .. 1.06e-4 against 2.2e-4 .. 3.2e-4.  The
other paths of `offset` keep the plain bound: 4.96e-5 against 5.06e-5 at (3, 33, 80), 5.62e-5 against 5.87e-5 at (2, 70, 80).

bf16 -- `silence`, `affine` and the quiet cases of BF16_VISIBLE against oracle/bf16_model.py at KERNEL_GAP_BOUND, or at twice the
model's own self-difference in that regime (float against double evaluation of the model) where that is above half the bound; `offset`, `sharp` and
`power` to finite outputs; no residual saturation anywhere (the float64 residual stream stays far inside fp16 range).

Measured on an MI355X, max |d log p| against the truth, worst over a regime's shapes and row modes (fp32 / fp32s / fp32s kernels):
    quiet_ln0 .. 5  2.2e-6 / 1.5e-6 / 1.8e-6    quiet_ln6 (classifier x 2)  4.6e-6 / 2.9e-6 / 4.5e-6    d_model 64 (generic) 5.3e-7
    affine 1.0e-5 / 6.2e-6 / 7.1e-6    sharp 1.2e-5 / 1.2e-5 / 6.8e-6    power 1.9e-6 / 1.2e-6 / 1.6e-6    silence 9.2e-7 / 5.0e-7 / 9.7e-7
    offset 1.06e-4 / 5.9e-5 / 8.6e-5 (plain bound 3.1e-5 .. 5.9e-5 on the paths that meet it, 2.2e-4 .. 3.2e-4 on the named ones)
bf16 against the model: quiet_ln6 1.3e-3 (self-difference 1.07e-3, bound 2.1e-3), silence 2.4e-4 (bound 1.5e-3), affine 1.4e-2
(self-difference 1.2e-2, bound 2.5e-2).
DESIGN.md section 4r has the table, the reason for `offset`'s bound and the plants."""
import numpy as np
import pytest

from tests import numeric_regimes as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


_MODELS = {}
_TRUTH = {}


def gpu_model(torch, regime):
    from voice_activity_detection_amd import SelfAttentiveVAD

    if regime not in _MODELS:
        r = nr.BY_NAME[regime]
        st = r.state()
        m = SelfAttentiveVAD(st["input_layer.0.weight"].shape[1], nr.num_layers(st), r.d_model, 0.5)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        _MODELS[regime] = (m.to("cuda").eval(), st)
    return _MODELS[regime]


def reference(case):
    """(truth, bound, chain bound) of a case: computed once, shared, left unchanged"""
    if case not in _TRUTH:
        r = nr.BY_NAME[case[0]]
        st, x = r.state(), r.x(case[1])
        want = nr.truth(st, x)
        want.setflags(write=False)
        _TRUTH[case] = (want,) + nr.kernel_bounds(r, st, x, want)
    return _TRUTH[case]


def run(torch, m, x, precision, row_mode=0, splits=0):
    m.precision, m.row_mode, m.attention_splits = precision, row_mode, splits
    try:
        with torch.no_grad():
            y = m(features=torch.from_numpy(x).to("cuda"))
        torch.cuda.synchronize()
    finally:
        m.precision, m.row_mode, m.attention_splits = "fp32", 0, 0
    return y.cpu().numpy()


# one test per path, so that a LayerNorm site that only one row mode reaches is caught under its own id (savad_device.h: every path;
# savad_kernels.h read_rows_layernorm: the fp32 row modes; savad_kernels_f32s.h merge of partial sums: fp32s rm8)
FP32_PATHS = [(case, path) for case in nr.CASES for path in nr.fp32_runs(nr.BY_NAME[case[0]].d_model, case[1][1])]


@pytest.mark.parametrize("case,path", FP32_PATHS, ids=[f"{nr.case_id(c)}-{p[0].replace(' ', '_')}" for c, p in FP32_PATHS])
def test_fp32_paths_hold_the_truth(torch_cuda, case, path):
    regime, shape = case
    label, precision, row_mode, splits = path
    m, _ = gpu_model(torch_cuda, regime)
    want, bound, chain_bound = reference(case)
    chained = nr.on_residual_chain(nr.BY_NAME[regime], shape[1], label)
    if chained:
        bound = chain_bound
    y = run(torch_cuda, m, nr.BY_NAME[regime].x(shape), precision, row_mode, splits)
    assert y.shape == want.shape and y.dtype == np.float32
    err = float(np.abs(y - want).max()) if np.isfinite(y).all() else float("inf")
    print(f"{nr.case_id(case)} {label}: {err:.2e}, {'residual-chain ' if chained else ''}bound {bound:.2e}")
    assert err < bound, (case, label, err, bound)


# ---- bf16 -----------------------------------------------------------------------------------------------------------------------
def run_bf16(torch, m, x, row_mode):
    m.precision, m.row_mode = "bf16", row_mode
    try:
        with torch.no_grad():
            y = m(features=torch.from_numpy(x).to("cuda"))
        torch.cuda.synchronize()
    finally:
        m.precision, m.row_mode = "fp32", 0
    return y.cpu().numpy()


# automatic, the per-layer launches, the fused launches and the persistent attention (T > 32; at T <= 32 row_mode 5 is a variant of the
# single launch and 3 keeps the per-layer launches)
BF16_ROW_MODES = (0, 1, 3, 5)


BF16_CASES = [c for c in nr.CASES if nr.BY_NAME[c[0]].d_model == 128]


def bf16_is_held(case):
    return case[0] in nr.BF16_HELD or case in nr.BF16_VISIBLE


@pytest.mark.parametrize("case", BF16_CASES, ids=nr.case_id)
def test_bf16_paths(torch_cuda, case):
    regime, shape = case
    m, st = gpu_model(torch_cuda, regime)
    x = nr.BY_NAME[regime].x(shape)
    assert nr.residual_stream_peak(st, x) < 65504.0 / 2   # the reference's residual stream stays inside fp16 range: nothing may clamp
    held = bf16_is_held(case)
    assert held or regime in nr.BF16_FINITE_ONLY or "quiet" in nr.BY_NAME[regime].tags
    if held:
        want = {False: nr.bf16_model_out(st, x)}
        if nr.pw_splits(shape[1]):
            want[True] = nr.bf16_model_out(st, x, key_split=True)
        sd = nr.bf16_regime_self_difference(regime)
        bound = nr.bf16_bound_of(sd)
    m.residual_saturations()
    gaps = {}
    for rm in BF16_ROW_MODES:
        y = run_bf16(torch_cuda, m, x, rm)
        assert y.shape == (shape[0], shape[1], 2) and np.isfinite(y).all(), (case, rm)
        assert m.residual_saturations() == 0, (case, rm)
        if held:
            gaps[rm] = float(np.abs(y - want[rm == 5 and nr.pw_splits(shape[1])]).max())
    if held:
        print(f"{nr.case_id(case)}: bf16 model self-difference {sd:.2e}, bound {bound:.2e}; kernel - model by row_mode "
              + ", ".join(f"{k}: {v:.2e}" for k, v in gaps.items()))
        bad = {k: v for k, v in gaps.items() if not v < bound}
        assert not bad, (case, bound, bad)


# ---- digital silence from the audio on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 160, 1600])
def test_log_mel_of_digital_silence(torch_cuda, n):
    """the power is exactly zero, so only the device logarithm of 1e-6 is left: within 4 ulp (3.8e-6) of float32(log(1e-6))"""
    from voice_activity_detection_amd.features import log_mel

    got = log_mel(np.zeros(n, np.float32)).cpu().numpy()
    assert got.shape == (1 + n // 160, 80) and got.dtype == np.float32
    d = float(np.abs(got.astype(np.float64) - float(nr.SILENCE)).max())
    print(f"n = {n}: |log_mel(0) - float32(log(1e-6))| = {d:.2e}")
    assert d <= 3.8e-6, d


@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
def test_digital_silence_end_to_end(torch_cuda, precision):
    """one second of exact zeros through predict_audio_device (log-mel -> windows -> forward -> boost) against the oracle's chain, at
    the bars of test_end_to_end_from_host_audio (tests/test_gpu_parity.py): 2e-6 on the probabilities, 1e-2 with bf16 operands"""
    from oracle import logmel, oracle
    from voice_activity_detection_amd import VADFromScratchPredictor

    m, st = gpu_model(torch_cuda, "silence")
    audio = np.zeros(16000, np.float32)
    feat = logmel.log_mel(audio)
    assert feat.shape == (101, 80) and (feat == nr.SILENCE).all()
    want, want_mean = oracle.predict_probabilities(st, feat)
    m.precision = precision
    try:
        probs, mean = VADFromScratchPredictor(m, "cuda").predict_audio_device(audio)
        probs, mean = probs.cpu().numpy(), mean.cpu().numpy()
    finally:
        m.precision = "fp32"
    assert probs.shape == want.shape == (101, 7) and np.isfinite(probs).all()
    assert np.array_equal(probs == 0.5, want == 0.5)
    d, dm = float(np.abs(probs - want).max()), float(np.abs(mean - want_mean).max())
    print(f"{precision}: digital silence, max |dp| {d:.2e}, max |d mean| {dm:.2e}")
    bar = 2e-6 if precision != "bf16" else 1e-2
    assert d < bar and dm < bar, (d, dm)


# ---- equal bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["quiet_ln3", "silence"])
def test_two_runs_give_equal_bits_and_a_poisoned_workspace_changes_nothing(torch_cuda, regime):
    torch = torch_cuda
    m, _ = gpu_model(torch, regime)
    r = nr.BY_NAME[regime]
    try:
        for shape in r.shapes:
            xt = torch.from_numpy(r.x(shape)).cuda()
            for precision, row_mode in (("fp32", 0), ("fp32", 1), ("fp32s", 0), ("fp32s", 3), ("bf16", 0), ("bf16", 1)):
                m.precision, m.row_mode = precision, row_mode
                with torch.no_grad():
                    y0 = m(features=xt).clone()
                    y1 = m(features=xt).clone()
                    m._workspace.fill_(255)
                    y2 = m(features=xt)
                assert torch.isfinite(y0).all() and torch.equal(y0, y1) and torch.equal(y0, y2), (regime, shape, precision, row_mode)
    finally:
        m.precision, m.row_mode = "fp32", 0
