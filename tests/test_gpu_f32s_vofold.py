"""fp32s, T > 32: the fused attention + row launches with the out-projection folded into the value projection
(csrc/savad_kernels_f32s.h: V is projected with Wo Wv' and bias Wo bv', the row chain starts at h + bo + O / l and has no Wo
slots).  precision "fp32s" with row_mode 3 pins those launches at every size.  Held to the CPU oracle and to the exact-fp32 kernels
at the suite's own TIGHT, at the smallest shapes where the new chain can go wrong: two key tiles with a ragged last one and a wave
without a block, whole tiles, uneven groups of query blocks, several groups per sequence, a deeper model, padded and chunked input
features; equal bits from run to run and on a poisoned workspace; and a state whose value bias is large enough for Wo bv to be a
visible share of the output, with masked keys in play."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 3e-5   # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


def make_model(torch, state, F=80, L=3):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(F, L, 128, 0.5)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    return make_model(torch_cuda, state1234)


def run(torch, model, x, precision="fp32s"):
    """fp32s: its fused launches (row_mode 3); fp32: the exact-fp32 kernels under their automatic schedule"""
    model.precision, model.row_mode = precision, (3 if precision == "fp32s" else 0)
    try:
        with torch.no_grad():
            y = model(features=torch.from_numpy(x).to("cuda"))
        torch.cuda.synchronize()
    finally:
        model.precision, model.row_mode = "fp32", 0
    return y.cpu().numpy()


def feats(seed, shape):
    from voice_activity_detection_amd.seeded import seeded_features

    return seeded_features(seed, shape)


def check(torch, model, state, x, tag):
    from oracle import oracle

    y = run(torch, model, x)
    e_ref = float(np.abs(y - oracle.forward(state, x, threads=8)).max())
    e_f32 = float(np.abs(y - run(torch, model, x, precision="fp32")).max())
    print(f"{tag}: max |dlogp| against the oracle {e_ref:.2e}, against the exact-fp32 kernels {e_f32:.2e}")
    assert np.isfinite(y).all(), tag
    assert e_ref < TIGHT, (tag, e_ref)
    assert e_f32 < TIGHT, (tag, e_f32)
    return y


@pytest.mark.parametrize("shape", [(3, 33, 80), (2, 64, 80), (5, 129, 80), (3, 801, 80)])
def test_folded_launches_against_oracle_and_fp32(torch_cuda, model, state1234, shape):
    x = feats(300 + shape[1], shape)
    y = check(torch_cuda, model, state1234, x, shape)
    assert np.array_equal(y, run(torch_cuda, model, x)), shape   # two runs: equal bits
    assert np.abs(np.logaddexp(y[..., 0], y[..., 1])).max() < 2e-6


def test_five_layers(torch_cuda):
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(55, num_layers=5)
    check(torch_cuda, make_model(torch_cuda, st, L=5), st, feats(57, (2, 100, 80)), "5 layers")


@pytest.mark.parametrize("F", [13, 257])
def test_odd_feature_sizes(torch_cuda, F):
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(900 + F, feature_size=F)
    check(torch_cuda, make_model(torch_cuda, st, F=F), st, feats(902 + F, (3, 70, F)), f"F={F}")


def test_poisoned_workspace(torch_cuda, model):
    """the workspace filled with 255 between two calls: the over-read rows behind the batch and the blocks of a wave without a query
    block must not reach the result"""
    torch = torch_cuda
    model.precision, model.row_mode = "fp32s", 3
    try:
        for shape in ((3, 33, 80), (5, 129, 80), (3, 801, 80)):
            xt = torch.from_numpy(feats(5, shape)).cuda()
            with torch.no_grad():
                y0 = model(features=xt).clone()
                model._workspace.fill_(255)
                y1 = model(features=xt)
            assert torch.isfinite(y1).all() and torch.equal(y0, y1), shape
    finally:
        model.precision, model.row_mode = "fp32", 0


# The bias path: value_projection.bias of every layer scaled by BV_SCALE, so that Wo bv -- which the folded launches carry as the bias of
# the V projection instead of pushing it through the out-projection -- is a visible share of the output.  The scale was fixed on the
# CPU: at 16 the reference arithmetic itself (stock PyTorch fp32 against the oracle accumulating in fp64) stays within TIGHT / 3, and
# dropping Wo bv would move the log-probabilities by more than 1000 x TIGHT.
BV_SCALE = 16.0


def biased_state():
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(4321)
    for k in st:
        if k.endswith("value_projection.bias"):
            st[k] = (st[k] * np.float32(BV_SCALE)).astype(np.float32)
    return st


@pytest.mark.parametrize("T", [33, 70])
def test_value_bias_path(torch_cuda, T):
    import torch

    from oracle import oracle, torch_port

    st = biased_state()
    x = feats(600 + T, (3, T, 80))
    # pre-condition: the reference arithmetic alone is well inside the bar at this scale
    ref64 = oracle.forward(st, x, acc64=True)
    ref_t = torch_port.forward({k: torch.from_numpy(v) for k, v in st.items()}, torch.from_numpy(x)).numpy()
    spread = float(np.abs(ref_t - ref64).max())
    print(f"T={T}: stock PyTorch fp32 against the fp64-accumulating oracle {spread:.2e}")
    assert spread <= TIGHT / 3, spread
    # ... and the bias matters: without Wo bv the result is somewhere else entirely
    st0 = {k: (np.zeros_like(v) if k.endswith("value_projection.bias") else v) for k, v in st.items()}
    share = float(np.abs(oracle.forward(st0, x) - oracle.forward(st, x)).max())
    print(f"T={T}: dropping the value bias moves the log-probabilities by {share:.2e}")
    assert share > 1000 * TIGHT, share
    check(torch_cuda, make_model(torch_cuda, st), st, x, f"bv x {BV_SCALE:g}, T={T}")
