"""A handle keeps three derived copies of its weights -- the LayerNorm-folded fp32 buffer, the bf16 fragment image and the fp32s image
with its folded Wq~ | Wvo part (csrc/savad.hip: prepare_weights, prepare_frags) -- each rebuilt on demand after the parameters change.
One module runs every precision on weights A, is reloaded with weights B and runs the precisions in the opposite order: every result
after the reload must be bit for bit what a module that only ever saw B gives in that precision and mode.  A stale image of any kind
(A's bf16 fragments, A's folded fp32s image at T = 96, A's packed fp32 buffer under a fresh image) shows as a difference; the
reference is the fresh module, so no tolerance is involved."""
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 80), (2, 96, 80)]                     # the single launch (T <= 32) and the per-layer launches
MODES = [("fp32", 0), ("bf16", 0), ("fp32s", 3)]      # fp32s with row_mode 3: its own kernels and, at T = 96, the folded image


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


def make_model(torch, state):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.to("cuda").eval()


def run(torch, model, mode, xs):
    model.precision, model.row_mode = mode
    try:
        with torch.no_grad():
            ys = [model(features=x).clone() for x in xs]
        torch.cuda.synchronize()
    finally:
        model.precision, model.row_mode = "fp32", 0
    return ys


def test_every_image_follows_a_reload(torch_cuda, state1234):
    from voice_activity_detection_amd.seeded import seeded_features, seeded_state_dict

    torch = torch_cuda
    xs = [torch.from_numpy(seeded_features(70 + i, s)).to("cuda") for i, s in enumerate(SHAPES)]
    state_b = seeded_state_dict(999)
    model = make_model(torch, state1234)
    before = {mode: run(torch, model, mode, xs) for mode in MODES}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state_b.items()}, strict=True)
    for mode in reversed(MODES):
        got = run(torch, model, mode, xs)
        want = run(torch, make_model(torch, state_b), mode, xs)   # a module that only ever saw B, and only this precision
        for shape, y, ref, old in zip(SHAPES, got, want, before[mode]):
            assert torch.isfinite(y).all(), (mode, shape)
            assert torch.equal(y, ref), (mode, shape, float((y - ref).abs().max()))
            assert not torch.equal(y, old), (mode, shape)         # (the two states do differ: the comparison above can fail)
