"""Feature front-end for any transform config (include/savad.h, "Feature front-end"), host side: tests/frontend_ref.py against
independent implementations (scipy, CPU torch), the library's host-built tables and shapes against frontend_ref, and
from_checkpoint(extended_front_end=True) building every config the reference can name.  No GPU needed."""
from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest

from tests import frontend_ref as ref

GEOMETRIES = [  # (transform, n_fft, hop_ms, window_ms, n_mels, n_mfcc)
    ("log-mel", 400, 10, 25, 40, None),
    ("log-mel", 1024, 20, 50, 64, None),
    ("log-mel", 401, 10, 25, 80, None),
    ("mel", 512, 10, 25, 80, None),
    ("mfcc", 512, 10, 25, 40, 13),
    ("spectrogram", 320, 10, 20, None, None),
    ("log-mel", 512, 10, 25, 80, None),
]


def _signal(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t * (1 + 0.1 * t)) + 0.05 * rng.standard_normal(n)
    y[: n // 3] *= 0.001
    return y.astype(np.float32)


def _front(g, deltas=False):
    from voice_activity_detection_amd.features import FrontEnd

    name, n_fft, hop_ms, window_ms, n_mels, n_mfcc = g
    return FrontEnd(name, n_fft, hop_ms, window_ms, n_mels, n_mfcc, deltas)


# ---- frontend_ref against independent implementations -----------------------------------------------------------------

@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [9, 10, 37])
def test_ref_delta_is_savgol_interp(order, n):
    from scipy.signal import savgol_filter

    x = np.random.default_rng(order * 100 + n).standard_normal((n, 5))
    want = savgol_filter(x, 9, polyorder=order, deriv=order, axis=0, mode="interp")
    got = ref.delta(x, order)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max()) + 1e-12
    # the 4 edge frames on each side included
    assert np.allclose(got[:4], want[:4], atol=1e-12) and np.allclose(got[-4:], want[-4:], atol=1e-12)
    with pytest.raises(ValueError):
        ref.delta(x[:8], order)


def test_ref_dct_is_scipy_ortho():
    from scipy.fft import dct

    x = np.random.default_rng(5).standard_normal((11, 40))
    assert np.abs(x @ ref.dct_ortho(40, 13).T - dct(x, type=2, norm="ortho", axis=1)[:, :13]).max() < 1e-12


@pytest.mark.parametrize("n_fft,hop,win", [(512, 160, 400), (1024, 320, 800), (401, 160, 400), (400, 160, 400)])
def test_ref_centred_stft_matches_scipy(n_fft, hop, win):
    """librosa's stft(center=True) centres the window in the n_fft frame: against scipy.signal.stft (window at the start of
    the segment) it differs by a linear phase only, once the signal is reflect-padded by n_fft // 2 - lpad"""
    from scipy.signal import get_window, stft

    y = _signal(16000 + 77).astype(np.float64)
    lpad = (n_fft - win) // 2
    x = np.pad(y, n_fft // 2 - lpad, mode="reflect")
    _, _, Z = stft(x, fs=16000, window="hann", nperseg=win, noverlap=win - hop, nfft=n_fft, boundary=None, padded=False)
    want = np.abs(Z).T * get_window("hann", win).sum()
    got = np.abs(ref.stft(y, n_fft, hop, win, center=True))
    k = min(len(want), len(got))
    assert k >= len(got) - 3
    assert np.abs(got[:k] - want[:k]).max() < 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("n_fft,hop,win", [(320, 160, 320), (512, 160, 400), (401, 160, 400)])
def test_ref_spectrogram_matches_torch_stft(n_fft, hop, win):
    import torch

    y = _signal(16000 + 5)
    want = torch.stft(torch.from_numpy(y), n_fft, hop_length=hop, win_length=win, window=torch.hamming_window(win), center=False,
                      normalized=False, onesided=True, return_complex=True).abs().numpy().T
    got = ref.features(y, "spectrogram", n_fft, hop / 16, win / 16)
    assert got.shape == want.shape == (ref.frame_count("spectrogram", len(y), n_fft, hop), n_fft // 2 + 1)
    assert np.abs(got - want).max() < 2e-5 * np.abs(want).max()


def test_ref_log_mel_is_the_oracle():
    from oracle import logmel

    y = _signal(8000 + 3)
    assert np.abs(ref.features(y, "log-mel", 512, 10, 25, 80) - logmel.log_mel(y)).max() < 1e-3


# ---- the library's host tables and shapes against frontend_ref --------------------------------------------------------

def _tables(fe):
    from voice_activity_detection_amd import _lib

    lib = _lib.load()
    cfg = fe.config()
    out = []
    for which in range(4):
        n = lib.savad_frontend_table_floats(ctypes.byref(cfg), which)
        assert n >= 0, lib.savad_last_error()
        buf = np.zeros(max(n, 1), dtype=np.float32)
        _lib.check(lib.savad_frontend_tables_host(ctypes.byref(cfg), which, buf.ctypes.data_as(ctypes.c_void_p)))
        out.append(buf[:n])
    return out


def _dft_ref(name, n_fft, win):
    """the DFT table as include/savad.h describes it, from frontend_ref's windows"""
    lpad = (n_fft - win) // 2
    k0 = lpad & ~3
    kr = (lpad + win - k0 + 7) // 8 * 8
    rows = 2 * ((n_fft + 1) // 2)
    R = (rows + 127) // 128 * 128
    w = np.zeros(n_fft + 16)
    w[lpad:lpad + win] = ref.hamming_periodic(win) if name == "spectrogram" else ref.hann_periodic(win)
    kp = k0 + np.arange(kr)
    wk = w[kp]
    T = np.zeros((R, kr))
    T[0] = wk
    if n_fft % 2 == 0:
        T[1] = wk * np.cos(2 * np.pi * (n_fft // 2) * kp / n_fft)
    for b in range(1, (n_fft + 1) // 2):
        T[2 * b] = wk * np.cos(2 * np.pi * b * kp / n_fft)
        T[2 * b + 1] = -wk * np.sin(2 * np.pi * b * kp / n_fft)
    return T


@pytest.mark.parametrize("g", GEOMETRIES, ids=lambda g: "-".join(str(v) for v in g))
def test_library_tables_match_reference(g):
    fe = _front(g)
    dft, mel, dct, sg = _tables(fe)
    want = _dft_ref(fe.transform, fe.n_fft, fe.win)
    assert dft.shape == (want.size,)
    assert np.abs(dft.reshape(want.shape) - want).max() < 2e-7
    if fe.transform == "spectrogram":
        assert mel.size == 0 and dct.size == 0
    else:
        mb = ref.mel_basis(fe.n_fft, fe.n_mels)
        assert np.abs(mel.reshape(mb.shape) - mb).max() < 1e-7 * max(1.0, np.abs(mb).max()) + 1e-9
    if fe.transform == "mfcc":
        assert np.abs(dct.reshape(fe.n_mfcc, fe.n_mels) - ref.dct_ortho(fe.n_mels, fe.n_mfcc)).max() < 1e-7
    else:
        assert dct.size == 0
    sgw = np.stack([ref.savgol_rows(1), ref.savgol_rows(2)])
    assert np.abs(sg.reshape(2, 9, 9) - sgw).max() < 1e-7


@pytest.mark.parametrize("g", GEOMETRIES, ids=lambda g: "-".join(str(v) for v in g))
def test_library_shapes_and_workspace(g):
    from voice_activity_detection_amd import _lib

    lib = _lib.load()
    for deltas in (False, True):
        fe = _front(g, deltas)
        cfg = fe.config()
        lo = fe.n_fft if fe.transform == "spectrogram" else fe.n_fft // 2 + 1
        for n in (lo, lo + 1, 16000, 16000 * 3 + 7):
            N_ref = ref.frame_count(fe.transform, n, fe.n_fft, fe.hop)
            if n <= 16000:   # the count of frames the restated STFT itself produces
                assert N_ref == len(ref.stft(np.zeros(n), fe.n_fft, fe.hop, fe.win, fe.transform != "spectrogram"))
            N, F, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            rc = lib.savad_frontend_shape(ctypes.byref(cfg), n, ctypes.byref(N), ctypes.byref(F))
            if deltas and N_ref < 9:
                assert rc != 0 and b"at least 9" in lib.savad_last_error()
                continue
            _lib.check(rc)
            assert (N.value, F.value) == (N_ref, fe.feature_size) == (fe.frames(n), fe.feature_size)
            _lib.check(lib.savad_frontend_workspace_bytes(ctypes.byref(cfg), n, ctypes.byref(ws)))
            spec = N_ref * ((fe.n_fft // 2 + 1 + 3) // 4 * 4) if fe.transform != "spectrogram" else 0
            assert ws.value >= 4 * (n + fe.n_fft + spec + (N_ref * fe.n_mels if fe.transform == "mfcc" else 0))
            assert ws.value % 256 == 0
        # below the minimum length
        rc = lib.savad_frontend_shape(ctypes.byref(cfg), lo - 1, ctypes.byref(N), ctypes.byref(F))
        assert rc != 0 and b"n_samples >=" in lib.savad_last_error()


def test_library_refuses_out_of_limit_geometry():
    from voice_activity_detection_amd import _lib

    lib = _lib.load()
    N, F = ctypes.c_int(), ctypes.c_int()
    for cfg, word in ((_lib.savad_frontend_config(2, 4096, 160, 400, 80, 0, 0), b"2048"),
                      (_lib.savad_frontend_config(2, 256, 160, 400, 80, 0, 0), b"n_fft"),
                      (_lib.savad_frontend_config(1, 512, 160, 400, 300, 0, 0), b"n_mels"),
                      (_lib.savad_frontend_config(3, 512, 160, 400, 40, 41, 0), b"n_mfcc"),
                      (_lib.savad_frontend_config(3, 512, 160, 400, 40, 0, 0), b"n_mfcc"),
                      (_lib.savad_frontend_config(7, 512, 160, 400, 40, 0, 0), b"unsupported")):
        assert lib.savad_frontend_shape(ctypes.byref(cfg), 16000, ctypes.byref(N), ctypes.byref(F)) != 0
        assert word in lib.savad_last_error(), lib.savad_last_error()


# ---- the product surface ----------------------------------------------------------------------------------------------

def _cfg(transform, deltas=False, stack=False, silence=None):
    from tests.conftest import REFERENCE_CONFIG

    cfg = copy.deepcopy(REFERENCE_CONFIG)
    cfg["feature_extractor"]["transform"] = dict(transform)
    cfg["feature_extractor"]["temporal_differences"] = deltas
    cfg["feature_extractor"]["stack_differences"] = stack
    if silence is not None:
        cfg["feature_extractor"]["silence_remover"] = silence
    return cfg


EXTENDED = [  # (transform node, deltas, model.feature_size)
    ({"name": "log-mel", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": None}, False, 40),
    ({"name": "log-mel", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": None}, True, 120),
    ({"name": "mfcc", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": 13}, False, 13),
    ({"name": "mfcc", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 40, "n_mfcc": 13}, True, 39),
    ({"name": "spectrogram", "n_fft": 320, "hop_ms": 10, "window_ms": 20, "n_mels": None, "n_mfcc": None}, False, 161),
    ({"name": "mel", "n_fft": 1024, "hop_ms": 20, "window_ms": 50, "n_mels": 64, "n_mfcc": None}, False, 64),
    ({"name": "log-mel", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 80, "n_mfcc": None}, False, 80),
]


@pytest.mark.parametrize("transform,deltas,size", EXTENDED, ids=lambda v: str(v))
def test_from_checkpoint_extended_front_end_builds_each_config(tmp_path, transform, deltas, size):
    from tests.conftest import write_reference_checkpoint
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor
    from voice_activity_detection_amd.seeded import seeded_state_dict

    path = write_reference_checkpoint(tmp_path / "x.checkpoint", seeded_state_dict(3, feature_size=size), _cfg(transform, deltas))
    p = VADFromScratchPredictor.from_checkpoint(path, "cpu", extended_front_end=True)
    assert p.model.feature_size == size == p.front_end.feature_size
    assert (p.hop_ms, p.window_ms) == (transform["hop_ms"], transform["window_ms"])
    assert p.front_end.is_shipped == (transform["n_mels"] == 80 and not deltas)
    if not (transform["n_mels"] == 80 and not deltas):
        with pytest.raises(NotImplementedError, match="unsupported"):   # the default still refuses it
            VADFromScratchPredictor.from_checkpoint(path, "cpu")


@pytest.mark.parametrize("cfg_args,match", [
    (dict(deltas=True, stack=True), "unsupported"),
    (dict(silence={"silence_threshold": 0.1}), "unsupported"),
    (dict(transform_patch={"name": "mfcc", "n_mfcc": None}), "unsupported"),
    (dict(transform_patch={"name": "mel", "n_mels": None}), "unsupported"),
    (dict(transform_patch={"name": "log-mel", "n_mels": None}), "unsupported"),
    (dict(transform_patch={"name": "cqt"}), "unsupported"),
    (dict(transform_patch={"n_fft": 4096}), "2048"),
    (dict(transform_patch={"n_fft": 256}), "n_fft"),
    (dict(transform_patch={"n_mels": 300}), "n_mels"),
    (dict(transform_patch={"name": "mfcc", "n_mels": 20, "n_mfcc": 30}), "n_mfcc"),
], ids=str)
def test_from_checkpoint_extended_front_end_refusals(tmp_path, state1234, cfg_args, match):
    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor

    tr = dict(REFERENCE_CONFIG["feature_extractor"]["transform"])
    tr.update(cfg_args.pop("transform_patch", {}))
    path = write_reference_checkpoint(tmp_path / "bad.checkpoint", state1234, _cfg(tr, **cfg_args))
    with pytest.raises((NotImplementedError, ValueError), match=match):
        VADFromScratchPredictor.from_checkpoint(path, "cpu", extended_front_end=True)


def test_front_end_is_hashable_and_shipped_default():
    from voice_activity_detection_amd.features import SHIPPED_FRONT_END, FrontEnd

    assert SHIPPED_FRONT_END.is_shipped and SHIPPED_FRONT_END.feature_size == 80
    assert not FrontEnd(deltas=True).is_shipped and FrontEnd(deltas=True).feature_size == 240
    assert len({FrontEnd(), FrontEnd(), FrontEnd("mel")}) == 2
