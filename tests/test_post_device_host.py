"""The arithmetic of the device post-processing (csrc/savad_post_device.h) on the CPU: the host twins run the inline functions the
kernels run, and are held to the host path that exists -- numpy and the postprocessing.py functions, which tests/test_postprocessing.py
pins to the reference's goldens.  Every comparison is exact."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.postprocessing import convert_frames_to_samples, trim_voice_activity

G = json.loads((Path(__file__).resolve().parent / "golden" / "golden_post.json").read_text())
INVALID, UNSUPPORTED = -1, -2


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def frames_host(probs, threshold=0.5, params=(0, 0, 0, 0)):
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    N, W = probs.shape
    boosted, trimmed = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint8)
    _lib.check(_lib.load().savad_post_frames_host(_p(probs), N, W, threshold, *params, _p(boosted), _p(trimmed)))
    return boosted, trimmed


def trim_host(pred, params):
    """the twin's trim of a 0/1 sequence: one probability per frame, 0.25 or 0.75 around the threshold 0.5"""
    pred = np.asarray(pred, dtype=np.uint8)
    return frames_host(np.where(pred != 0, 0.75, 0.25).astype(np.float32).reshape(-1, 1), 0.5, params)[1]


def class_host(frames, sr, hop_ms, win_ms):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    num = len(convert_frames_to_samples(frames, sr, hop_ms, win_ms))
    cls = np.empty(num, dtype=np.uint8)
    _lib.check(_lib.load().savad_post_sample_class_host(_p(frames), len(frames), sr, float(hop_ms), float(win_ms), 0, num, _p(cls)))
    return cls


@pytest.mark.parametrize("W", [1, 2, 7, 8, 9, 16, 17, 39, 128])
def test_row_mean_has_numpys_bits(W):
    rng = np.random.default_rng(W)
    probs = rng.random((4001, W), dtype=np.float32)
    probs[:50] *= np.float32(1e-3)   # rows of another magnitude
    boosted, trimmed = frames_host(probs, 0.5)
    want = probs.mean(axis=1)
    assert want.dtype == np.float32 and np.array_equal(boosted.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(trimmed, (want > 0.5).astype(np.uint8))


def test_threshold_is_strict_in_float32():
    t = np.float32(0.3)   # 0.3 is no float32: the comparison is against its rounding, as numpy compares a float32 array with a Python float
    rows = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], dtype=np.float32)
    for W in (1, 2, 8, 7):   # (a power of two of equal values has exactly their mean; 7 of them land where they land)
        probs = np.repeat(rows[:, None], W, axis=1)
        boosted, trimmed = frames_host(probs, 0.3)
        assert np.array_equal(boosted, probs.mean(axis=1))
        assert trimmed.tolist() == (probs.mean(axis=1) > 0.3).tolist()
        if W != 7:
            assert np.array_equal(boosted, rows) and trimmed.tolist() == [0, 0, 1]


def _check_trim(pred, params):
    want = trim_voice_activity(np.asarray(pred, dtype=np.uint8), *params)
    got = trim_host(pred, params)
    assert np.array_equal(got, want), (list(pred), params, got.tolist(), want.tolist())


def test_trim_golden_cases():
    assert G["trim"]
    for c in G["trim"]:
        params = (c["min_vally"], c["min_hill"], c["hang_before"], c["hang_over"])
        assert trim_host(c["pred"], params).tolist() == c["out"], c
        _check_trim(c["pred"], params)


def test_trim_random_run_length_sequences():
    rng = np.random.default_rng(11)
    for it in range(4000):
        runs = rng.integers(1, 10, size=rng.integers(1, 14))
        v = int(rng.integers(0, 2))
        pred = []
        for r in runs:
            pred += [v] * int(r)
            v ^= 1
        params = tuple(int(x) for x in rng.integers(0, 9, size=4))
        if it % 5 == 0:
            params = (params[0], params[1], 0, max(params[3], 1))   # the hang pass never runs without hang_before
        _check_trim(pred, params)


def test_trim_edges_and_exact_lengths():
    for n in (0, 1, 2):
        for bits in range(1 << n):
            for params in ((0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 2, 2), (0, 0, 0, 5)):
                _check_trim([(bits >> k) & 1 for k in range(n)], params)
    for m in (1, 2, 4, 7):
        for length in (m - 1, m, m + 1):
            if length < 1:
                continue
            valley = [1, 1, 1] + [0] * length + [1, 1, 1]
            hill = [0, 0, 0] + [1] * length + [0, 0, 0]
            for params in ((m, 0, 0, 0), (0, m, 0, 0), (m, m, 0, 0), (m, m, 2, 3), (0, 0, m, m)):
                _check_trim(valley, params)
                _check_trim(hill, params)
                _check_trim([0] * length + hill + [0] * length, params)
    # runs that touch both ends: zeros and ones at an end are neither a valley nor a hill
    for params in ((5, 5, 0, 0), (5, 5, 3, 3), (2, 2, 8, 8), (0, 0, 1, 0)):
        _check_trim([1, 0, 0, 1, 1, 0, 0, 0, 1], params)
        _check_trim([0, 1, 1, 0, 0, 1, 1, 1, 0], params)
        _check_trim([1] * 6, params)
        _check_trim([0] * 6, params)
        _check_trim([0, 0, 1, 0, 0], params)
        _check_trim([1, 1, 0, 1, 1], params)


GEOMETRIES = [(16000, 10, 25), (16000, 10, 10), (100, 10, 25), (16000, 10, 5), (16000, 12.5, 25)]


@pytest.mark.parametrize("sr,hop_ms,win_ms", GEOMETRIES)
def test_sample_class_matches_frames_to_samples(sr, hop_ms, win_ms):
    lib = _lib.load()
    assert lib.savad_post_supported(7, sr, float(hop_ms), float(win_ms), 100) == 1
    rng = np.random.default_rng(sr + int(win_ms))
    patterns = [rng.integers(0, 2, size=n).astype(np.uint8) for n in (1, 2, 3, 17, 120)]
    patterns += [np.zeros(9, np.uint8), np.ones(9, np.uint8), np.array([1, 1, 0, 1, 1], np.uint8), np.array([0, 0, 1, 0, 0], np.uint8),
                 np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0] * 3, np.uint8)]
    for frames in patterns:
        value = convert_frames_to_samples(frames, sr, hop_ms, win_ms)
        want = np.where(value == 1.0, 1, np.where(value == 0.0, 0, 2)).astype(np.uint8)
        got = class_host(frames, sr, hop_ms, win_ms)
        assert np.array_equal(got, want), (sr, hop_ms, win_ms, frames.tolist())
    # a slice of the samples is the slice of the whole
    frames = patterns[4]
    whole = class_host(frames, sr, hop_ms, win_ms)
    part = np.empty(len(whole) // 2, dtype=np.uint8)
    _lib.check(lib.savad_post_sample_class_host(_p(frames), len(frames), sr, float(hop_ms), float(win_ms), 5, len(part), _p(part)))
    assert np.array_equal(part, whole[5:5 + len(part)])


def test_supported_conditions():
    lib = _lib.load()
    assert lib.savad_post_supported(7, 16000, 10.0, 25.0, 360001) == 1
    assert lib.savad_post_supported(128, 100, 10.0, 25.0, 0) == 1
    assert lib.savad_post_supported(7, 30, 10.0, 25.0, 100) == 0       # hop = 0.3 samples
    assert lib.savad_post_supported(129, 16000, 10.0, 25.0, 100) == 0  # numpy sums a row of more than 128 in another order
    assert lib.savad_post_supported(0, 16000, 10.0, 25.0, 100) == 0
    assert lib.savad_post_supported(7, 16000, 10.0, 25.0, -1) == 0
    assert lib.savad_post_supported(7, 16001, 10.0, 25.0, 100) == 0    # hop = 160.01
    assert lib.savad_post_supported(7, 0, 10.0, 25.0, 100) == 0
    from voice_activity_detection_amd.postprocessing import device_post_supported

    assert device_post_supported(7, 16000, 10, 25, 1001) and not device_post_supported(7, 30, 10, 25, 1001)
    assert not device_post_supported(7, None, 10, 25, 1001)


def test_argument_validation():
    lib = _lib.load()
    probs = np.full((4, 7), 0.5, dtype=np.float32)
    boosted, trimmed = np.empty(4, np.float32), np.empty(4, np.uint8)
    frames, cls = np.ones(4, np.uint8), np.empty(1000, np.uint8)
    longs = np.empty(4, np.int64)
    size = ctypes.c_size_t()
    fh = lib.savad_post_frames_host
    assert fh(None, 4, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID and b"null" in lib.savad_last_error()
    assert fh(_p(probs), 4, 7, 0.5, 0, 0, 0, 0, None, _p(trimmed)) == INVALID
    assert fh(_p(probs), 4, 7, 0.5, 0, 0, 0, 0, _p(boosted), None) == INVALID
    assert fh(_p(probs), -1, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), 4, 0, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), 4, 7, 0.5, -1, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), 4, 7, 0.5, 0, 0, 0, -2, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), 4, 129, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == UNSUPPORTED
    assert fh(None, 0, 7, 0.5, 0, 0, 0, 0, None, None) == 0   # no frames: a no-op
    ch = lib.savad_post_sample_class_host
    assert ch(None, 4, 16000, 10.0, 25.0, 0, 10, _p(cls)) == INVALID
    assert ch(_p(frames), 4, 16000, 10.0, 25.0, 0, 10, None) == INVALID
    assert ch(_p(frames), -1, 16000, 10.0, 25.0, 0, 10, _p(cls)) == INVALID
    assert ch(_p(frames), 4, 16000, 10.0, 25.0, -1, 10, _p(cls)) == INVALID
    assert ch(_p(frames), 4, 16000, 10.0, 25.0, 0, -1, _p(cls)) == INVALID
    assert ch(_p(frames), 4, 16000, 10.0, 25.0, 0, 3 * 160 + 400 + 1, _p(cls)) == INVALID   # one past the last sample
    assert ch(_p(frames), 4, 16000, 10.0, 25.0, 0, 3 * 160 + 400, _p(cls)) == 0
    assert ch(_p(frames), 4, 30, 10.0, 25.0, 0, 1, _p(cls)) == UNSUPPORTED
    # the device entry points refuse bad arguments before they touch the device
    pf = lib.savad_post_frames
    assert pf(None, 4, 7, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == INVALID
    assert pf(None, -1, 7, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == INVALID
    assert pf(None, 4, 7, 0.5, 0, -1, 0, 0, None, None, None, 0, None) == INVALID
    assert pf(None, 4, 129, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == UNSUPPORTED
    assert pf(None, 0, 7, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == 0
    ps = lib.savad_post_segments
    assert ps(None, None, 4, 16000, 10.0, 25.0, 0, _p(longs), _p(longs), 4, None, 0, None) == INVALID     # null frames
    assert ps(None, None, -1, 16000, 10.0, 25.0, 0, _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, 4, 16000, 10.0, 25.0, 0, _p(longs), _p(longs), -1, None, 0, None) == INVALID    # cap < 0
    assert ps(None, None, 4, 16000, 10.0, 25.0, 0, None, None, 4, None, 0, None) == INVALID               # null outputs with room asked for
    assert ps(None, None, 4, 16000, 10.0, 25.0, -5, _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, 4, 16000, 10.0, 25.0, 1, _p(longs), _p(longs), 4, None, 0, None) == INVALID     # (savad_optimal_split refuses it too)
    assert ps(None, None, 4, 30, 10.0, 25.0, 0, _p(longs), _p(longs), 4, None, 0, None) == UNSUPPORTED
    assert ps(None, None, 0, 16000, 10.0, 25.0, 0, None, None, 0, None, 0, None) == 0                    # no frames: no segments
    sp = lib.savad_post_sample_probs
    assert sp(None, 4, 16000, 10.0, 25.0, None, None) == INVALID
    assert sp(None, -1, 16000, 10.0, 25.0, None, None) == INVALID
    assert sp(None, 4, 30, 10.0, 25.0, None, None) == UNSUPPORTED
    wb = lib.savad_post_workspace_bytes
    assert wb(4, 7, 16000, 10.0, 25.0, None) == INVALID
    assert wb(-1, 7, 16000, 10.0, 25.0, ctypes.byref(size)) == INVALID
    assert wb(4, 129, 16000, 10.0, 25.0, ctypes.byref(size)) == UNSUPPORTED
    assert wb(4, 7, 30, 10.0, 25.0, ctypes.byref(size)) == UNSUPPORTED
    assert wb(4, 7, 16000, 10.0, 25.0, ctypes.byref(size)) == 0 and size.value > 0
    small = size.value
    assert wb(360001, 7, 16000, 10.0, 25.0, ctypes.byref(size)) == 0 and small < size.value < 1 << 28   # the hour: two bytes a sample and change
    sb = lib.savad_post_set_block
    for bad in (-64, 1, 32, 63, 96, 4096, 1 << 20):
        assert sb(bad) == INVALID and b"scan block" in lib.savad_last_error()
    for ok in (64, 128, 2048, 0):
        assert sb(ok) == 0
