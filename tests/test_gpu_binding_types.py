"""The typed pointer arguments of the ctypes binding on the GPU: device tensors become their addresses, what a kernel would have
read wrongly is refused in Python before the call, a typed call and a raw call give the same bits, and the public wrappers still
give the results their own tests hold them to (oracle, numpy, the host post-processing).  Nothing here launches with a bad
pointer."""
import ctypes

import numpy as np
import pytest

from voice_activity_detection_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


def address(param):
    return ctypes.cast(param, ctypes.c_void_p).value


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t * (1 + 0.1 * t)) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    y[: n // 3] *= 0.001
    return y


def test_device_tensors_and_refusals(torch_cuda):
    torch = torch_cuda
    f32 = _lib.dev(_lib.f32)
    t = torch.zeros(64, device="cuda")
    assert address(f32.from_param(t)) == t.data_ptr()
    assert address(f32.from_param(t[8:])) == t.data_ptr() + 32
    assert address(_lib.dev(_lib.i16, _lib.f32).from_param(t)) == t.data_ptr() and address(_lib.dev().from_param(t)) == t.data_ptr()
    with pytest.raises(ValueError, match="contiguous"):
        f32.from_param(t[::2])
    with pytest.raises(ValueError, match="int16"):
        f32.from_param(torch.zeros(64, dtype=torch.int16, device="cuda"))
    for kind in (_lib.host(_lib.f32), _lib.host()):
        with pytest.raises(TypeError, match="host"):
            kind.from_param(t)
    s = torch.cuda.Stream()
    assert address(_lib.stream.from_param(s)) == s.cuda_stream
    assert (address(_lib.stream.from_param(torch.cuda.current_stream())) or 0) == torch.cuda.current_stream().cuda_stream   # (0: the default)
    # the refusal reaches a library call as an exception, before anything is launched
    with pytest.raises(ctypes.ArgumentError):
        _lib.load().savad_pcm16_to_f32(torch.zeros(4, device="cuda"), 4, torch.zeros(4, device="cuda"), torch.cuda.current_stream())


def test_typed_and_raw_calls_give_the_same_bits(torch_cuda):
    torch = torch_cuda
    lib = _lib.load()
    stream = torch.cuda.current_stream()
    raw_stream = ctypes.c_void_p(stream.cuda_stream)
    # savad_pcm16_to_f32, n = 5
    pcm = torch.tensor([-32768, -1, 0, 1, 32767], dtype=torch.int16, device="cuda")
    typed, raw = torch.full((5,), 7.0, device="cuda"), torch.full((5,), 9.0, device="cuda")
    _lib.check(lib.savad_pcm16_to_f32(pcm, 5, typed, stream))
    _lib.check(lib.savad_pcm16_to_f32(pcm.data_ptr(), 5, ctypes.c_void_p(raw.data_ptr()), raw_stream))
    assert torch.equal(typed, raw) and torch.equal(typed, pcm.float() / 32768.0)
    # savad_logmel, n = 513: 4 frames, the last 16-byte piece partial
    n = 513
    audio = torch.from_numpy(_signal(n, 513)).cuda()
    words = lib.savad_logmel_workspace_bytes(n) // 4
    outs = []
    for as_typed in (True, False):
        ws = torch.empty(words, dtype=torch.float32, device="cuda")
        out = torch.full((4, 80), float("nan"), device="cuda")
        if as_typed:
            _lib.check(lib.savad_logmel(audio, n, ws, out, stream))
        else:
            _lib.check(lib.savad_logmel(audio.data_ptr(), n, ws.data_ptr(), out.data_ptr(), raw_stream))
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_public_wrappers_keep_their_results(torch_cuda, state1234):
    """each wrapper against what its own tests compare it with -- never against the code under test"""
    from oracle import logmel, oracle
    from voice_activity_detection_amd import SelfAttentiveVAD
    from voice_activity_detection_amd.features import log_mel, pcm16_to_f32
    from voice_activity_detection_amd.postprocessing import post_frames_device, trim_voice_activity
    from voice_activity_detection_amd.seeded import seeded_features

    torch = torch_cuda
    # pcm16_to_f32: sample / 32768, exactly (tests/test_gpu_caller_buffers.py)
    pcm = np.random.default_rng(5).integers(-32768, 32768, size=1001).astype(np.int16)
    got = pcm16_to_f32(torch.from_numpy(pcm).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.uint32), (pcm.astype(np.float32) / np.float32(32768.0)).view(np.uint32))
    # log_mel: the oracle's float64 restatement, at the bars of tests/test_gpu_parity.py::test_logmel_matches_oracle
    y = _signal(1600, 1600)
    ref = logmel.log_mel(y)
    mel = log_mel(y).cpu().numpy()
    assert mel.shape == ref.shape == (11, 80)
    assert np.abs(mel - ref).max() < 5e-4 and np.median(np.abs(mel - ref)) < 2e-6
    into = torch.empty((11, 80), device="cuda")
    assert log_mel(torch.from_numpy(y).cuda(), "cuda", out=into) is into and np.array_equal(into.cpu().numpy(), mel)
    # post_frames_device at [3, 7]: numpy's float32 row mean, bit for bit, and the host trim (tests/test_gpu_post_device.py)
    probs = np.array([[0.9] * 7, [0.1, 0.2, 0.3, 0.9, 0.8, 0.2, 0.1], [0.6, 0.7, 0.4, 0.5, 0.5, 0.9, 0.3]], dtype=np.float32)
    mean = probs.mean(axis=1)
    for params in ((0, 0, 0, 0), (1, 1, 1, 1)):
        boosted, trimmed = post_frames_device(torch.tensor(probs).cuda(), 0.5, *params)
        assert np.array_equal(boosted.cpu().numpy().view(np.uint32), mean.view(np.uint32))
        assert np.array_equal(trimmed.cpu().numpy(), trim_voice_activity((mean > 0.5).astype(np.uint8), *params))
    # model(features) at [3, 7, 80]: the CPU oracle at the fp32 bar of tests/test_gpu_parity.py (TIGHT)
    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state1234.items()}, strict=True)
    model = model.to("cuda").eval()
    x = seeded_features(21, (3, 7, 80))
    with torch.no_grad():
        logp = model(features=torch.from_numpy(x).cuda())
        again = model(features=torch.from_numpy(x).cuda(), out=torch.empty((3, 7, 2), device="cuda"))
    assert logp.shape == (3, 7, 2) and logp.dtype == torch.float32 and logp.is_contiguous()
    assert np.abs(logp.cpu().numpy() - oracle.forward(state1234, x)).max() < 3e-5
    assert torch.equal(logp, again)
    with pytest.raises(ValueError, match="out must be"):
        model(features=torch.from_numpy(x).cuda(), out=torch.empty((3, 7, 4), device="cuda")[:, :, ::2])


def test_tensor_on_another_device_than_the_current_one(torch_cuda):
    """device 0 current, a tensor on device 1: the argument type refuses it, the public wrapper reaches it through the guard"""
    torch = torch_cuda
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no second device to hold the tensor")
    from voice_activity_detection_amd.features import pcm16_to_f32

    with torch.cuda.device(0):
        pcm = torch.tensor([-32768, -1, 0, 1, 32767], dtype=torch.int16, device="cuda:1")
        with pytest.raises(ValueError, match="cuda:1"):
            _lib.dev(_lib.i16).from_param(pcm)
        assert _lib.on_device(pcm.device) is not _lib.on_device(torch.device("cuda:0"))
        got = pcm16_to_f32(pcm)
        assert got.device == pcm.device and torch.equal(got, pcm.float() / 32768.0)
        assert torch.cuda.current_device() == 0
