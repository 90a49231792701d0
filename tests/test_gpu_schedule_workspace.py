"""The workspace a schedule reports is the workspace its launches use (csrc/savad_schedule.h sizes it, savad.hip launches into it).
Every case calls the C ABI directly with a workspace of EXACTLY the reported bytes followed by 4 KiB of a byte pattern: the pattern
must be intact afterwards, and the output bit-equal to the same call through the module, which allocates its own workspace.
Shapes are the smallest that reach each form and variant of the three kernel families: 3 layers, seeded weights."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA5, 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def models(torch_cuda):
    """feature size -> module (80: no padding; 40: features zero-padded to 48 columns)"""
    from voice_activity_detection_amd import SelfAttentiveVAD
    from voice_activity_detection_amd.seeded import seeded_state_dict

    out = {}
    for F in (80, 40):
        m = SelfAttentiveVAD(F, 3, 128, 0.5)
        m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in seeded_state_dict(1234, feature_size=F).items()}, strict=True)
        out[F] = m.to("cuda").eval()
    return out


class Knobs:
    """the module's schedule settings for the length of a case"""

    def __init__(self, model, precision, row_mode, splits=0, batch_invariant=False):
        self.model, self.new = model, (precision, row_mode, splits, batch_invariant)

    def __enter__(self):
        m = self.model
        self.old = (m.precision, m.row_mode, m.attention_splits, m.batch_invariant)
        m.precision, m.row_mode, m.attention_splits, m.batch_invariant = self.new
        return m

    def __exit__(self, *exc):
        m = self.model
        m.precision, m.row_mode, m.attention_splits, m.batch_invariant = self.old


def guarded_call(torch, model, size_fn, call_fn):
    """size_fn(lib, handle, byref(nbytes)) reports the workspace, call_fn(lib, handle, ws_ptr, nbytes, stream) runs on exactly that much"""
    from voice_activity_detection_amd import _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    lib = model._prepare_call(dev)   # weights and knobs pushed to the handle
    nbytes = ctypes.c_size_t()
    _lib.check(size_fn(lib, model._handle, ctypes.byref(nbytes)))
    n = nbytes.value
    assert n > 0
    buf = torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(call_fn(lib, model._handle, ctypes.c_void_p(buf.data_ptr()), n, stream))
    torch.cuda.synchronize()
    guard = buf[n:].cpu().numpy()
    assert (guard == PATTERN).all(), f"{int((guard != PATTERN).sum())} bytes written past the {n} reported workspace bytes"


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def feats(torch, seed, shape):
    from voice_activity_detection_amd.seeded import seeded_features

    return torch.from_numpy(seeded_features(seed, shape)).to("cuda")


def case(precision, shape, row_mode, **kw):
    name = f"{precision}-{'x'.join(map(str, shape))}-m{row_mode}" + "".join(f"-{k}{v}" for k, v in kw.items())
    return pytest.param(precision, shape, row_mode, kw, id=name)


FORWARD_CASES = (
    [case("fp32", (2, 7, 80), mode) for mode in (0, 1, 2, 4)] +
    [case("fp32", (2, 96, 80), mode) for mode in (0, 1, 2, 3)] +
    [case("fp32", (2, 96, 80), 0, splits=2), case("fp32", (3, 20, 40), 0)] +
    [case("bf16", (5, 7, 80), mode) for mode in (0, 1, 5, 6, 7, 8)] +
    [case("bf16", (2, 96, 80), mode) for mode in (0, 1, 2, 3, 5)] +
    [case("bf16", (2, 96, 80), 5, batch_invariant=True), case("bf16", (2, 96, 80), 0, bf16_features=True)] +
    [case("fp32s", (5, 7, 80), mode) for mode in (0, 3, 7, 8)] +
    [case("fp32s", (2, 96, 80), mode) for mode in (0, 3)]   # 0: handed to the exact-fp32 kernels
)


@pytest.mark.parametrize("precision,shape,row_mode,kw", FORWARD_CASES)
def test_forward_stays_inside_reported_workspace(torch_cuda, models, precision, shape, row_mode, kw):
    torch = torch_cuda
    B, T, F = shape
    x = feats(torch, 100 + T + F, shape)
    x_dtype = 0
    if kw.get("bf16_features"):
        x, x_dtype = x.to(torch.bfloat16), 1
    with Knobs(models[F], precision, row_mode, kw.get("splits", 0), kw.get("batch_invariant", False)) as model:
        with torch.no_grad():
            want = model(features=x)
        out = torch.zeros((B, T, 2), dtype=torch.float32, device="cuda")
        guarded_call(torch, model, lambda lib, h, nb: lib.savad_workspace_bytes(h, B, T, nb),
                     lambda lib, h, ws, n, st: lib.savad_forward_ex(h, ptr(x), x_dtype, B, T, ptr(out), ws, n, st))
    assert torch.equal(out, want)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp32s"])
def test_strided_forward_stays_inside_reported_workspace(torch_cuda, models, precision):
    torch = torch_cuda
    T, hop, count, F = 96, 48, 3, 80
    feature = feats(torch, 7, (T + hop * (count - 1), F))
    with Knobs(models[F], precision, 0) as model:
        want = model.forward_windows(feature, T, hop, 0, count)
        out = torch.zeros((count, T, 2), dtype=torch.float32, device="cuda")
        guarded_call(torch, model, lambda lib, h, nb: lib.savad_workspace_bytes(h, count, T, nb),
                     lambda lib, h, ws, n, st: lib.savad_forward_strided(h, ptr(feature), 0, count, T, hop * F, ptr(out), ws, n, st))
    assert torch.equal(out, want)


@pytest.mark.parametrize("row_mode", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp32s"])
def test_predict_stays_inside_reported_workspace(torch_cuda, models, precision, row_mode):
    torch = torch_cuda
    N, half, jump, chunk, F = 60, 19, 9, 16, 80
    feature = feats(torch, 9, (N, F))
    with Knobs(models[F], precision, row_mode) as model:
        want_probs, want_mean = model.predict_windows(feature, half, jump, chunk)
        probs, mean = torch.zeros_like(want_probs), torch.zeros_like(want_mean)
        guarded_call(torch, model, lambda lib, h, nb: lib.savad_predict_workspace_bytes(h, N, half, jump, chunk, nb),
                     lambda lib, h, ws, n, st: lib.savad_predict_probabilities(h, ptr(feature), N, half, jump, chunk, ptr(probs), ptr(mean),
                                                                               ws, n, st))
    assert torch.equal(probs, want_probs) and np.array_equal(mean.cpu().numpy(), want_mean.cpu().numpy())
