"""fp32s, T > 32: the waves of the fused launch that have no query block (csrc/savad_kernels_f32s.h: attention_row_kernel_f32s).  A
workgroup is a group of up to four query blocks of one sequence, one wave per block.  A wave without a block computes nothing: it
moves its quarter of every slot of the key / weight stream, meets the working waves at every barrier of the attention and of the row
chain, and is done (it used to run the whole row chain on zeros).  A group of four has no such wave.  precision "fp32s" with
row_mode 3 pins the fused launches at every size.  Shapes = the smallest at which each combination of roles occurs (QB = query
blocks of a sequence):

    T = 40   QB 2   two working waves and two without a block
    T = 96   QB 3   three working waves and one without a block, one workgroup per sequence
    T = 100  QB 4   control: no blockless wave; ragged last key tile
    T = 160  QB 5   groups of 2 and 3
    T = 200  QB 7   a group of 3 and a full group on the same key stream; ragged
    T = 800  QB 25  the headline's grouping (B = 1)

against the CPU oracle at the suite's TIGHT; a sequence's bits do not depend on the batch it arrives in, nor on other forwards in
flight beside it (the roles are decided by the shape alone, never by timing)."""
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


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()}, strict=True)
    return m.to("cuda").eval()


def feats(T, B=3):
    """the features of the B = 3 batch of length T; B = 1 is its sequence 0"""
    from voice_activity_detection_amd.seeded import seeded_features

    return seeded_features(5200 + T, (3, T, 80))[:B].copy()


@pytest.fixture(scope="module")
def fused(torch_cuda, model):
    """x [B,T,80] on the host -> log-probs of the fused launches; one result per (T, B), computed once and shared"""
    torch, done = torch_cuda, {}

    def run(T, B):
        if (T, B) not in done:
            model.precision, model.row_mode = "fp32s", 3
            try:
                with torch.no_grad():
                    y = model(features=torch.from_numpy(feats(T, B)).to("cuda"))
                torch.cuda.synchronize()
            finally:
                model.precision, model.row_mode = "fp32", 0
            done[(T, B)] = y.cpu().numpy()
        return done[(T, B)]

    return run


CASES = [(40, 1), (40, 3), (96, 1), (96, 3), (100, 1), (100, 3), (160, 1), (160, 3), (200, 1), (200, 3), (800, 1)]


@pytest.mark.parametrize("T,B", CASES)
def test_every_role_combination_against_the_oracle(fused, state1234, T, B):
    from oracle import oracle

    y = fused(T, B)
    err = float(np.abs(y - oracle.forward(state1234, feats(T, B), threads=8)).max())
    print(f"[{B},{T},80]: max |dlogp| against the oracle {err:.2e}")
    assert y.shape == (B, T, 2) and np.isfinite(y).all()
    assert err < TIGHT, err
    assert np.abs(np.logaddexp(y[..., 0], y[..., 1])).max() < 2e-6


@pytest.mark.parametrize("T", [96, 200])
def test_a_sequence_has_the_same_bits_in_any_batch(fused, T):
    assert np.array_equal(fused(T, 1)[0], fused(T, 3)[0])


def test_three_forwards_in_flight_have_the_modules_bits(torch_cuda, model, fused):
    """T = 200 (a group of three blocks and a full group per sequence), three of these forwards in flight on three streams"""
    from voice_activity_detection_amd import PipelinedVAD

    torch = torch_cuda
    want = fused(200, 3)
    x = torch.from_numpy(feats(200, 3)).to("cuda")
    model.precision, model.row_mode = "fp32s", 3
    try:
        pipe = PipelinedVAD(model, depth=3)
        outs = pipe.forward_many([x, x, x])
        torch.cuda.synchronize()
    finally:
        model.precision, model.row_mode = "fp32", 0
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), want)
