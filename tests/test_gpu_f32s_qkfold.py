"""fp32s, T > 32: the fused launches with the key projection folded into the query (csrc/savad_kernels_f32s.h: fold_qk_kernel --
the query is projected with Wq~ = c Wk'^T Wq' and bias c Wk'^T bq', the key IS the normalised row, whose operand triples the input
stage and the row chain store as the K image; four Wq~ | Wvo slots instead of six).  precision "fp32s" with row_mode 3 pins those
launches at every size.  Held to the CPU oracle and to the exact-fp32 kernels at the suite's own TIGHT, at the smallest shapes where
the stream can go wrong: two key tiles with a ragged last one and a wave without a block, whole tiles, uneven groups of query
blocks, several groups per sequence, a deeper model, padded and chunked input features; equal bits from run to run and on a
poisoned workspace; peaked softmaxes; and a state whose query and key biases are large, so that the folded bias bq~ carries a
visible share of the scores while the dropped key-bias term is large too."""
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
    x = feats(400 + shape[1], shape)
    y = check(torch_cuda, model, state1234, x, shape)
    assert np.array_equal(y, run(torch_cuda, model, x)), shape   # two runs: equal bits
    assert np.abs(np.logaddexp(y[..., 0], y[..., 1])).max() < 2e-6


def test_five_layers(torch_cuda):
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(56, num_layers=5)
    check(torch_cuda, make_model(torch_cuda, st, L=5), st, feats(58, (2, 100, 80)), "5 layers")


@pytest.mark.parametrize("F", [13, 257])
def test_odd_feature_sizes(torch_cuda, F):
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(910 + F, feature_size=F)
    check(torch_cuda, make_model(torch_cuda, st, F=F), st, feats(912 + F, (3, 70, F)), f"F={F}")


def test_poisoned_workspace(torch_cuda, model):
    """the workspace filled with 255 between two calls: the K blocks no wave stores (a wave without a query block, the over-read rows
    behind the batch) must not reach the result"""
    torch = torch_cuda
    model.precision, model.row_mode = "fp32s", 3
    try:
        for shape in ((3, 33, 80), (5, 129, 80), (3, 801, 80)):
            xt = torch.from_numpy(feats(6, shape)).cuda()
            with torch.no_grad():
                y0 = model(features=xt).clone()
                model._workspace.fill_(255)
                y1 = model(features=xt)
            assert torch.isfinite(y1).all() and torch.equal(y0, y1), shape
    finally:
        model.precision, model.row_mode = "fp32", 0


def test_peaked_softmax(torch_cuda):
    """gain 4: peaked softmaxes, where an error in a score shows.  (The reference arithmetic alone -- stock PyTorch fp32 against fp64 --
    is 5.3e-6 at this state and shape, inside TIGHT / 3.)"""
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(77, gain=4.0)
    check(torch_cuda, make_model(torch_cuda, st), st, feats(79, (3, 70, 80)), "gain 4")


# The bias path: query_projection.bias and key_projection.bias of every layer scaled by QK_BIAS_SCALE.  The folded launches carry the
# query bias as bq~ = c Wk'^T bq' and drop the key bias altogether (its term of a score is the same for every key of a row).  The
# pre-conditions are asserted on the CPU: the reference arithmetic alone stays within TIGHT / 3 at this scale, the query bias is a
# visible share of the result (so a wrong bq~ cannot hide), and the key bias really is invisible to the model in fp64.
QK_BIAS_SCALE = 64.0


def biased_state():
    from voice_activity_detection_amd import seeded_state_dict

    st = seeded_state_dict(4321)
    for k in st:
        if k.endswith("query_projection.bias") or k.endswith("key_projection.bias"):
            st[k] = (st[k] * np.float32(QK_BIAS_SCALE)).astype(np.float32)
    return st


@pytest.mark.parametrize("T", [33, 70])
def test_query_and_key_bias_path(torch_cuda, T):
    import torch

    from oracle import oracle, torch_port

    st = biased_state()
    x = feats(600 + T, (3, T, 80))
    ref64 = oracle.forward(st, x, acc64=True)
    ref_t = torch_port.forward({k: torch.from_numpy(v) for k, v in st.items()}, torch.from_numpy(x)).numpy()
    spread = float(np.abs(ref_t - ref64).max())
    print(f"T={T}: stock PyTorch fp32 against the fp64-accumulating oracle {spread:.2e}")
    assert spread <= TIGHT / 3, spread
    stq = {k: (np.zeros_like(v) if k.endswith("query_projection.bias") else v) for k, v in st.items()}
    share = float(np.abs(oracle.forward(stq, x, acc64=True) - ref64).max())
    print(f"T={T}: zeroing the query biases moves the log-probabilities by {share:.2e}")
    assert share > 100 * TIGHT, share
    # (in fp64 from end to end -- the stock-PyTorch port on double tensors: the oracle's fp64 sums still return fp32 log-probabilities)
    def port64(state):
        return torch_port.forward({k: torch.from_numpy(v).double() for k, v in state.items()}, torch.from_numpy(x).double()).numpy()

    stk = {k: (np.zeros_like(v) if k.endswith("key_projection.bias") else v) for k, v in st.items()}
    keyb = float(np.abs(port64(stk) - port64(st)).max())
    print(f"T={T}: zeroing the key biases moves the fp64 log-probabilities by {keyb:.2e}")
    assert keyb < 1e-12, keyb
    check(torch_cuda, make_model(torch_cuda, st), st, x, f"bq, bk x {QK_BIAS_SCALE:g}, T={T}")
