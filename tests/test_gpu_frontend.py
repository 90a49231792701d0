"""Feature front-end for any transform config on the MI355X (savad_frontend, features.FrontEnd): device features against the
float64 restatement tests/frontend_ref.py, the generic kernels on the shipped geometry against savad_logmel, bit stability
(unaligned audio, repeated calls, graph replay), and a non-shipped checkpoint end to end through the CLI."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import frontend_ref as ref

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]

CONFIGS = [  # (transform, n_fft, hop_ms, window_ms, n_mels, n_mfcc)
    ("log-mel", 400, 10, 25, 40, None),
    ("log-mel", 1024, 20, 50, 64, None),
    ("log-mel", 401, 10, 25, 80, None),
    ("mel", 512, 10, 25, 80, None),
    ("mfcc", 512, 10, 25, 40, 13),
    ("spectrogram", 320, 10, 20, None, None),
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


def _chirp(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t * (1 + 0.1 * np.minimum(t, 10.0)))
         + 0.05 * rng.standard_normal(n)).astype(np.float32)
    y[: n // 3] *= 0.001  # near silence: the log floor, the dB clamp
    return y


def _wav():
    from tests.golden.data_files import data_root
    from voice_activity_detection_amd.features import load_wav_mono16k

    return load_wav_mono16k(data_root() / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav")


def _front(c, deltas=False):
    from voice_activity_detection_amd.features import FrontEnd

    return FrontEnd(*c, deltas)


def _check(name, got, want, base_factor=1.0):
    """the bars of the front-end (include/savad.h); base_factor 2 for the temporal differences"""
    d = np.abs(got.astype(np.float64) - want)
    if name == "log-mel":
        assert d.max() < 5e-4 * base_factor and np.median(d) < 2e-6 * base_factor, (d.max(), np.median(d))
    elif name == "mfcc":
        assert d.max() < 5e-3 * base_factor and np.median(d) < 1e-4 * base_factor, (d.max(), np.median(d))
    else:
        assert d.max() / np.abs(want).max() < 1e-5 * base_factor, d.max() / np.abs(want).max()


def _compare(fe, y, torch):
    got = fe.extract(y, "cuda").cpu().numpy()
    want = ref.features(y, fe.transform, fe.n_fft, fe.hop_ms, fe.window_ms, fe.n_mels, fe.n_mfcc, fe.deltas)
    assert got.shape == want.shape == (fe.frames(len(y)), fe.feature_size)
    F = fe.base_size
    _check(fe.transform, got[:, :F], want[:, :F])
    if fe.deltas:
        _check(fe.transform, got[:, F:2 * F], want[:, F:2 * F], 2.0)
        _check(fe.transform, got[:, 2 * F:], want[:, 2 * F:], 2.0)


@pytest.mark.parametrize("deltas", [False, True])
@pytest.mark.parametrize("c", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_front_end_matches_reference(torch_cuda, c, deltas):
    fe = _front(c, deltas)
    lo = fe.n_fft if fe.transform == "spectrogram" else fe.n_fft // 2 + 1
    n9 = fe.n_fft + 8 * fe.hop if fe.transform == "spectrogram" else max(8 * fe.hop + 1, lo)   # 9 frames
    for n in (3 * 16000 + 77, n9 if deltas else lo):   # a few seconds; 9 frames / exactly the minimum length
        _compare(fe, _chirp(n, n), torch_cuda)
    _compare(fe, _wav(), torch_cuda)


def test_front_end_minimum_lengths_and_nine_frames(torch_cuda):
    fe = _front(("log-mel", 400, 10, 25, 40, None), True)
    n9 = 8 * fe.hop                      # 1 + n // hop = 9
    assert fe.frames(n9) == 9
    _compare(fe, _chirp(n9, 1), torch_cuda)
    sp = _front(("spectrogram", 320, 10, 20, None, None), True)
    assert sp.frames(320 + 8 * 160) == 9
    _compare(sp, _chirp(320 + 8 * 160, 2), torch_cuda)
    from voice_activity_detection_amd import _lib

    for f, n in ((fe, n9 - fe.hop), (sp, 320 + 7 * 160)):   # 8 frames
        with pytest.raises(_lib.SavadError, match="at least 9"):
            f.extract(_chirp(n, 3), "cuda")


def test_front_end_hour_sampled(torch_cuda):
    """one hour through log-mel (400, 10, 25, 40): the first, a middle and the last stretch of frames against frontend_ref"""
    fe = _front(("log-mel", 400, 10, 25, 40, None))
    n = 3600 * 16000
    rng = np.random.default_rng(11)
    t = np.arange(n, dtype=np.float32) / np.float32(16000.0)
    y = (0.3 * np.sin(np.float32(2 * np.pi * 440) * t) + 0.05 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    y[n // 2:n // 2 + 16000 * 5] *= 0.001
    got = fe.extract(y, "cuda").cpu().numpy()
    N = fe.frames(n)
    assert got.shape == (N, 40)
    for a in (0, N // 2 - 64, N // 2 + 100, N - 200):
        fr = np.arange(a, min(a + 200, N))
        _check("log-mel", got[fr], ref.log_mel_frames(y, 400, 160, 400, 40, fr))


def test_generic_path_on_shipped_geometry_matches_savad_logmel(torch_cuda):
    from voice_activity_detection_amd.features import SHIPPED_FRONT_END, log_mel

    for y in (_chirp(16000 * 7 + 33, 4), _wav()):
        a = SHIPPED_FRONT_END.extract(y, "cuda", generic=True).cpu().numpy()
        b = log_mel(y, "cuda").cpu().numpy()
        assert a.shape == b.shape and np.abs(a - b).max() < 5e-4
        assert np.array_equal(SHIPPED_FRONT_END.extract(y, "cuda").cpu().numpy(), b)   # the shipped config keeps log_mel's bits


@pytest.mark.parametrize("c", [CONFIGS[2], CONFIGS[4], CONFIGS[5]], ids=lambda c: c[0])
def test_unaligned_audio_and_repeated_calls_give_the_same_bits(torch_cuda, c):
    torch = torch_cuda
    fe = _front(c, True)
    y = _chirp(16000 * 2 + 5, 6)
    dev = torch.from_numpy(np.concatenate([[0.0], y]).astype(np.float32)).cuda()
    a = fe.extract(dev[1:], "cuda").cpu().numpy()        # 4 bytes past a 16-byte boundary
    b = fe.extract(dev[1:].clone(), "cuda").cpu().numpy()
    c2 = fe.extract(y, "cuda").cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(b, c2)


def _checkpoint(tmp_path, transform, deltas, size):
    import copy

    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd.seeded import seeded_state_dict

    cfg = copy.deepcopy(REFERENCE_CONFIG)
    cfg["feature_extractor"]["transform"] = dict(transform)
    cfg["feature_extractor"]["temporal_differences"] = deltas
    state = seeded_state_dict(21, feature_size=size)
    return write_reference_checkpoint(tmp_path / "fe.checkpoint", state, cfg), state


MFCC = {"name": "mfcc", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": 13}
LOGMEL40 = {"name": "log-mel", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": None}


def test_graph_mode_equals_eager_for_mfcc_with_deltas(torch_cuda, tmp_path):
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor

    path, _ = _checkpoint(tmp_path, MFCC, True, 39)
    eager = VADFromScratchPredictor.from_checkpoint(path, "cuda", extended_front_end=True)
    pg = VADFromScratchPredictor.from_checkpoint(path, "cuda", extended_front_end=True)
    pg.graph = True
    y = _chirp(16000 * 4 + 19, 8)
    pe, me = eager.predict_audio_device(y)
    pe, me = pe.cpu().numpy(), me.cpu().numpy()
    for _ in range(2):
        p, m = pg.predict_audio_device(y)
        assert np.array_equal(p.cpu().numpy(), pe) and np.array_equal(m.cpu().numpy(), me)
    assert pg.graph_stats["captures"] == 1 and pg.graph_stats["replays"] == 2


def test_checkpoint_end_to_end_cli_predict_and_evaluate(torch_cuda, tmp_path):
    """log-mel 40 + deltas (feature_size 120): `predict --extended-front-end` against the same model fed frontend_ref's features,
    fp32 and fp32s; `evaluate --extended-front-end` runs; the host / streaming audio paths refuse the front-end"""
    from tests.golden.data_files import data_root
    from voice_activity_detection_amd.predictor import StreamingPredictor, VADFromScratchPredictor, VADPredictParameters

    path, _ = _checkpoint(tmp_path, LOGMEL40, True, 120)
    wav = data_root() / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav"
    y = _wav()
    env = dict(os.environ, PYTHONPATH=str(REPO))
    pred = VADFromScratchPredictor.from_checkpoint(path, "cuda", extended_front_end=True)
    params = VADPredictParameters(None, 0.5, 0, 0, 0, 0, None, True, 100, True)
    feats = lambda chunk: ref.features(chunk, "log-mel", 512, 10, 25, 40, None, True).astype(np.float32)  # noqa: E731
    for prec in ("fp32", "fp32s"):
        out = tmp_path / f"out_{prec}.json"
        r = subprocess.run([sys.executable, "-m", "voice_activity_detection_amd", "predict", str(wav), str(path), "--extended-front-end",
                            "--return-probs", "--probs-sample-rate", "100", "--precision", prec, "--output-path", str(out)],
                           cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array(json.loads(out.read_text())["probs"])
        pred.model.precision = prec
        want = np.array(pred.predict(y, params, features_fn=feats).probs)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-4, np.abs(got - want).max()
    pred.model.precision = "fp32"
    r = subprocess.run([sys.executable, "-m", "voice_activity_detection_amd", "evaluate", str(data_root() / "eval_list.jsonl"), str(path),
                        "--extended-front-end", "--output-path", str(tmp_path / "eval.jsonl")],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    total = json.loads((tmp_path / "eval.jsonl").read_text().splitlines()[0])
    assert 0.0 <= total["auc"] <= 1.0
    with pytest.raises(NotImplementedError):
        pred.predict_audio_host(y)
    sp = StreamingPredictor(pred.model, "cuda", front_end=pred.front_end)
    for call in (lambda: sp.predict_audio_device(y), lambda: sp.predict_audio_host(y), lambda: sp.audio_span_logp(y, 0, 1)):
        with pytest.raises(NotImplementedError):
            call()
