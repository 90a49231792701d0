"""The device post-processing (savad_post_frames, savad_post_segments, savad_post_sample_probs; csrc/savad_post_device.h) on the GPU
against the host path that exists: numpy's mean and the postprocessing.py functions (pinned to the reference's goldens by
tests/test_postprocessing.py).  Integers and float bits: every comparison is exact."""
import functools
import json
import math

import numpy as np
import pytest

from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.postprocessing import (convert_frames_to_samples, optimal_split_voice_activity, segment_indices,
                                                         trim_voice_activity)

pytestmark = pytest.mark.gpu

PARAMS = ((0, 0, 0, 0), (20, 20, 10, 10), (3, 5, 0, 7), (1, 1, 1, 1))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    return torch


@pytest.fixture
def block64():
    """the scans at 64 elements per workgroup block: a small input runs three and more levels"""
    lib = _lib.load()
    _lib.check(lib.savad_post_set_block(64))
    yield 64
    _lib.check(lib.savad_post_set_block(0))


def _runs(rng, n, lengths):
    """a 0/1 sequence of n frames made of runs whose lengths are drawn from `lengths`"""
    out = np.empty(n + max(lengths), dtype=np.uint8)
    at, v = 0, int(rng.integers(0, 2))
    while at < n:
        r = int(rng.choice(lengths))
        out[at:at + r] = v
        at, v = at + r, v ^ 1
    return out[:n]


@functools.lru_cache(maxsize=None)
def _probs(N, W):
    """(probs [N, W], numpy's float32 row mean): a planted run-length pattern (short and long runs, so that every trim pass has
    work) plus noise that stays away from the threshold 0.5, and a few rows exactly on it"""
    rng = np.random.default_rng(1000 * W + N)
    pattern = _runs(rng, N, (1, 2, 3, 4, 7, 12, 19, 20, 21, 40, 150))
    probs = np.where(pattern[:, None] != 0, np.float32(0.8), np.float32(0.2)) + (rng.random((N, W), dtype=np.float32) - np.float32(0.5)) * np.float32(0.2)
    probs = probs.astype(np.float32)
    probs[rng.integers(0, N, size=max(N // 50, 1))] = np.float32(0.5)   # mean exactly 0.5: not above the threshold
    probs.setflags(write=False)
    mean = probs.mean(axis=1)
    mean.setflags(write=False)
    return probs, mean


def _check_frames(torch, N, W):
    from voice_activity_detection_amd.postprocessing import post_frames_device

    probs, mean = _probs(N, W)
    assert mean.dtype == np.float32
    dev = torch.tensor(probs).cuda()   # (a copy: the shared reference stays read-only)
    for params in PARAMS:
        boosted, trimmed = post_frames_device(dev, 0.5, *params)
        assert boosted.dtype == torch.float32 and trimmed.dtype == torch.uint8 and boosted.shape == trimmed.shape == (N,)
        assert np.array_equal(boosted.cpu().numpy().view(np.uint32), mean.view(np.uint32)), (N, W)
        want = trim_voice_activity((mean > 0.5).astype(np.uint8), *params)
        got = trimmed.cpu().numpy()
        assert np.array_equal(got, want), (N, W, params, np.flatnonzero(got != want)[:10])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 4097, 70001])
def test_frames_default_block(torch_cuda, N):
    _check_frames(torch_cuda, N, 7)


@pytest.mark.parametrize("W", [8, 39])
def test_frames_other_widths(torch_cuda, W):
    _check_frames(torch_cuda, 4097, W)


@pytest.mark.parametrize("N", [4097, 64 * 64 * 64 + 1])
def test_frames_three_scan_levels(torch_cuda, block64, N):
    _check_frames(torch_cuda, N, 7)


def _patterns():
    rng = np.random.default_rng(5)
    z, o = [0], [1]
    return {
        "zeros": np.zeros(50, np.uint8),
        "ones": np.ones(50, np.uint8),
        "voice at both ends": np.array(o * 5 + z * 20 + o * 5, np.uint8),
        "lone zero": np.array(z * 6 + o * 9 + z + o * 9 + z * 6, np.uint8),       # all MID around it: no segment end
        "lone one": np.array(z * 9 + o + z * 9 + o * 2 + z * 9 + o * 3 + z * 4, np.uint8),   # one or two frames never reach 1.0 at 2.5 hops
        "one frame": np.array(o, np.uint8),
        "two frames": np.array(o + z, np.uint8),
        "runs of 1 2 3": _runs(rng, 3000, (1, 2, 3)),   # every boundary case of a 2.5-hop window
        "mixed runs": _runs(rng, 3001, (1, 2, 3, 5, 8, 30)),
    }


PATTERNS = _patterns()
GEOMETRIES = ((16000, 10, 25), (16000, 10, 10), (16000, 10, 5))


def _check_segments(torch, frames, sr, hop_ms, win_ms):
    from voice_activity_detection_amd.postprocessing import segments_device

    want_s, want_e = segment_indices(convert_frames_to_samples(frames, sr, hop_ms, win_ms))
    got_s, got_e = segments_device(torch.from_numpy(frames).cuda(), None, sr, hop_ms, win_ms)
    assert got_s.dtype == got_e.dtype == np.int64
    assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e), (len(got_s), len(want_s))
    return len(want_s)


@pytest.mark.parametrize("name", list(PATTERNS))
def test_segments_without_split(torch_cuda, name):
    counts = [_check_segments(torch_cuda, PATTERNS[name], *g) for g in GEOMETRIES]
    if name in ("ones", "voice at both ends", "runs of 1 2 3", "mixed runs"):
        assert min(counts) > 0


@pytest.mark.parametrize("name", list(PATTERNS))
def test_segments_without_split_many_blocks(torch_cuda, block64, name):
    for g in GEOMETRIES:
        _check_segments(torch_cuda, PATTERNS[name], *g)


def test_segments_cap_smaller_than_count(torch_cuda):
    import ctypes

    torch = torch_cuda
    frames = PATTERNS["mixed runs"]
    want_s, want_e = segment_indices(convert_frames_to_samples(frames, 16000, 10, 25))
    assert len(want_s) > 8
    lib = _lib.load()
    dev = torch.from_numpy(frames).cuda()
    need = ctypes.c_size_t()
    _lib.check(lib.savad_post_workspace_bytes(len(frames), 1, 16000, 10.0, 25.0, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cap in (0, 3):
        starts, ends = np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int64)
        cnt = lib.savad_post_segments(ctypes.c_void_p(dev.data_ptr()), None, len(frames), 16000, 10.0, 25.0, 0, ctypes.c_void_p(starts.ctypes.data),
                                      ctypes.c_void_p(ends.ctypes.data), cap, ctypes.c_void_p(ws.data_ptr()), need.value, stream)
        assert cnt == len(want_s)   # the count is returned, only `cap` pairs are written
        assert np.array_equal(starts[:cap], want_s[:cap]) and np.array_equal(ends[:cap], want_e[:cap])
        assert (starts[cap:] == -7).all() and (ends[cap:] == -7).all()
    # a workspace that is too small is refused
    assert lib.savad_post_segments(ctypes.c_void_p(dev.data_ptr()), None, len(frames), 16000, 10.0, 25.0, 0, ctypes.c_void_p(starts.ctypes.data),
                                   ctypes.c_void_p(ends.ctypes.data), 3, ctypes.c_void_p(ws.data_ptr()), need.value - 1, stream) == -1


def _split_cases():
    rng = np.random.default_rng(9)
    n = 3000
    ones = np.ones(n, np.uint8)
    noise = (0.6 + 0.39 * rng.random(n)).astype(np.float32)
    lone_zero = ones.copy()
    lone_zero[1500] = 0   # a MID stretch inside one long segment
    dip = noise.copy()
    dip[1499:1502] = np.float32([0.3, 0.01, 0.3])   # ... and the minimum falls into it
    three = np.array([1] * 1200 + [0] * 10 + [1] * 30 + [0] * 10 + [1] * 1750, np.uint8)   # two long segments and a short one
    return {
        "constant": (ones, np.full(n, 0.9, np.float32)),   # all ties: the first index wins
        "decreasing": (ones, np.linspace(0.99, 0.6, n).astype(np.float32)),
        "increasing": (ones, np.linspace(0.6, 0.99, n).astype(np.float32)),
        "noise": (ones, noise),
        "minimum in a MID stretch": (lone_zero, dip),
        "two long one short": (three, noise),
        "mixed runs": (_runs(rng, n, (1, 2, 3, 40, 400)), noise),
    }


SPLIT_CASES = _split_cases()


def _check_split(torch, trimmed, boosted, sr, hop_ms, win_ms, max_samples):
    from voice_activity_detection_amd.postprocessing import segments_device

    seconds = max_samples / sr
    assert int(seconds * sr) == max_samples
    pred = convert_frames_to_samples(trimmed, sr, hop_ms, win_ms)
    split = optimal_split_voice_activity(pred, convert_frames_to_samples(boosted, sr, hop_ms, win_ms), seconds, sr)
    want_s, want_e = segment_indices(split)
    got_s, got_e = segments_device(torch.from_numpy(trimmed).cuda(), torch.from_numpy(boosted).cuda(), sr, hop_ms, win_ms, max_length_seconds=seconds)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e), (len(got_s), len(want_s))
    return len(want_s), len(segment_indices(pred)[0])


@pytest.mark.parametrize("name", list(SPLIT_CASES))
@pytest.mark.parametrize("max_samples", [1000, 4001, 16000])
def test_segments_with_split(torch_cuda, name, max_samples):
    trimmed, boosted = SPLIT_CASES[name]
    after, before = _check_split(torch_cuda, trimmed, boosted, 16000, 10, 25, max_samples)
    assert after > before   # something was split


def test_segments_with_split_many_blocks(torch_cuda, block64):
    for name in ("minimum in a MID stretch", "two long one short"):
        _check_split(torch_cuda, *SPLIT_CASES[name], 16000, 10, 25, 4001)


def test_split_at_exactly_max_samples(torch_cuda):
    """at 100 Hz (hop 1 sample, window 2.5) a run of k frames is a segment of k samples: 50 = max_samples stays, 51 is split"""
    trimmed = np.array([0] * 5 + [1] * 50 + [0] * 5 + [1] * 51 + [0] * 5, np.uint8)
    boosted = (0.6 + 0.3 * np.random.default_rng(2).random(len(trimmed))).astype(np.float32)
    starts, ends = segment_indices(convert_frames_to_samples(trimmed, 100, 10, 25))
    assert (ends + 1 - starts).tolist() == [50, 51]
    after, before = _check_split(torch_cuda, trimmed, boosted, 100, 10, 25, 50)
    assert (before, after) == (2, 3)


@pytest.mark.parametrize("N", [1, 2, 4097])
@pytest.mark.parametrize("sr", [16000, 100])
def test_sample_probs(torch_cuda, sr, N):
    from voice_activity_detection_amd.postprocessing import sample_probs_device

    boosted = _probs(4097, 7)[1][:N]
    want = convert_frames_to_samples(boosted, sr, 10, 25)
    got = sample_probs_device(torch_cuda.from_numpy(np.ascontiguousarray(boosted)).cuda(), sr, 10, 25)
    assert got.dtype == torch_cuda.float64 and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()})
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _features_of(key):
    from oracle import logmel

    return logmel.log_mel(np.frombuffer(key, dtype=np.float32))


def _features(chunk):
    """the CPU log-mel of a chunk, computed once for the host run and the device run"""
    return _features_of(np.ascontiguousarray(chunk, dtype=np.float32).tobytes())


def _chunks(seconds, params):
    return math.ceil(seconds / params.split_max_seconds) if params.split_max_seconds is not None else 1


@pytest.mark.parametrize("case", [0, 1, 2])
def test_predict_device_post_equals_host(torch_cuda, model, case):
    from tests.test_postprocessing import G, _audio
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    c = G["predict"][case]
    audio = _audio(case, c["seconds"])
    params = VADPredictParameters(**c["params"])
    host = VADFromScratchPredictor(model, "cuda")
    device = VADFromScratchPredictor(model, "cuda", device_post=True)
    want = host.predict(audio, params, features_fn=_features).to_json()
    got = device.predict(audio, params, features_fn=_features).to_json()
    assert got == want
    assert want["activities"] == c["json"]["activities"]
    n = _chunks(len(audio) / 16000, params)
    assert device.post_stats == {"device": n, "host": 0} and host.post_stats == {"device": 0, "host": n}


def test_predict_device_post_falls_back_and_runs_under_a_graph(torch_cuda, model):
    import dataclasses

    from tests.test_postprocessing import G, _audio
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    c = G["predict"][0]
    audio = _audio(0, c["seconds"])
    # 30 Hz probabilities: a hop of 0.3 samples stays on the host, silently and correctly
    params = dataclasses.replace(VADPredictParameters(**c["params"]), probs_sample_rate=30)
    device = VADFromScratchPredictor(model, "cuda", device_post=True)
    want = VADFromScratchPredictor(model, "cuda").predict(audio, params, features_fn=_features).to_json()
    assert device.predict(audio, params, features_fn=_features).to_json() == want and len(want["probs"]) > 0
    assert device.post_stats == {"device": 0, "host": 1}
    # a replayed graph owns the probabilities: the device post-processing reads them before the next replay
    c = G["predict"][1]
    audio = _audio(1, c["seconds"])
    params = dataclasses.replace(VADPredictParameters(**c["params"]), return_probs=True, probs_sample_rate=100)
    host = VADFromScratchPredictor(model, "cuda", graph=True)
    device = VADFromScratchPredictor(model, "cuda", graph=True, device_post=True)
    for _ in range(2):
        assert device.predict(audio, params).to_json() == host.predict(audio, params).to_json()
    assert device.graph_stats["replays"] > 0 and device.post_stats["device"] == 2 * _chunks(len(audio) / 16000, params)


def test_cli_device_post(torch_cuda, tmp_path, state1234):
    import wave

    from tests.conftest import write_reference_checkpoint
    from tests.test_postprocessing import _audio
    from voice_activity_detection_amd.__main__ import main

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    pcm = (_audio(0, 6.0) * 20000).astype(np.int16)
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    common = ["predict", str(tmp_path / "a.wav"), str(tmp_path / "m.checkpoint"), "--return-probs", "--probs-sample-rate", "100",
              "--min-vally-ms", "80", "--min-hill-ms", "60", "--hang-before-ms", "30", "--hang-over-ms", "50", "--activity-max-sec", "1"]
    assert main(common + ["--output-path", str(tmp_path / "host.json")]) == 0
    assert main(common + ["--output-path", str(tmp_path / "device.json"), "--device-post"]) == 0
    host, device = json.loads((tmp_path / "host.json").read_text()), json.loads((tmp_path / "device.json").read_text())
    assert device == host and len(host["probs"]) == 602
