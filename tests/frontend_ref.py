"""float64 numpy restatement of the feature front-end (include/savad.h, "Feature front-end") -- TEST INFRASTRUCTURE ONLY.

Restates librosa 0.8.0 (absent from this image, like for oracle/logmel.py) and torch 1.8.1's stft for the reference's four
transforms (vad/acoustics/transforms/*.py) and its temporal differences (vad/acoustics/feature_extractor.py:135-145).
numpy only, so that the GPU tests can use it; tests/test_frontend_host.py pins it against scipy and CPU torch.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.logmel import hann_periodic, mel_filterbank

SR = 16000
TRANSFORMS = {"spectrogram": 0, "mel": 1, "log-mel": 2, "mfcc": 3}


def samples(ms) -> int:
    """int(ms / 1000 * sample_rate), as the reference's transforms compute hop and window"""
    return int(ms / 1000 * SR)


def hamming_periodic(n: int) -> np.ndarray:
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / n)  # torch.hamming_window(n) (periodic)


def frame_count(name: str, n: int, n_fft: int, hop: int) -> int:
    """util.frame over the signal, reflect-padded by n_fft // 2 per side when centred: 1 + n // hop for an even n_fft"""
    return 1 + (n + (0 if name == "spectrogram" else 2 * (n_fft // 2)) - n_fft) // hop


def stft(y, n_fft: int, hop: int, win: int, center: bool) -> np.ndarray:
    """complex [N, n_fft // 2 + 1]: librosa.stft(center=True, reflect, hann) or torch.stft(center=False, hamming)"""
    y = np.asarray(y, dtype=np.float64)
    w = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = hann_periodic(win) if center else hamming_periodic(win)
    if center:
        y = np.pad(y, n_fft // 2, mode="reflect")
    n = 1 + (len(y) - n_fft) // hop
    idx = hop * np.arange(n)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(y[idx] * w[None, :], axis=1)


def mel_basis(n_fft: int, n_mels: int) -> np.ndarray:
    return mel_filterbank(SR, n_fft, n_mels).astype(np.float64)


def dct_ortho(n_mels: int, n_mfcc: int) -> np.ndarray:
    """[n_mfcc, n_mels]: scipy.fftpack.dct(type=2, norm="ortho") as a matrix"""
    k = np.arange(n_mfcc)[:, None]
    n = np.arange(n_mels)[None, :]
    d = np.cos(np.pi * k * (2 * n + 1) / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    d[0] *= np.sqrt(0.5)
    return d


def savgol_rows(order: int, width: int = 9) -> np.ndarray:
    """[width, width]: row u = weights of the order-th derivative at position u of the degree-`order` polynomial fitted
    to `width` points (u = width // 2: the interior filter; the others: mode="interp" at the edges)"""
    pos = np.arange(width, dtype=np.float64)
    V = pos[:, None] ** np.arange(order + 1)[None, :]
    pinv = np.linalg.pinv(V)                                  # coefficients = pinv @ x
    D = np.zeros((width, order + 1))                          # d^order / du^order of u^k at each position
    for k in range(order, order + 1):
        D[:, k] = math.factorial(k) / math.factorial(k - order) * pos ** (k - order)
    return D @ pinv


def delta(x: np.ndarray, order: int, width: int = 9) -> np.ndarray:
    """librosa.feature.delta(x.T, width, order, axis=-1, mode="interp").T for x [N, F]"""
    N = x.shape[0]
    if N < width:
        raise ValueError(f"delta needs at least {width} frames, got {N}")
    rows = savgol_rows(order, width)
    out = np.empty_like(x, dtype=np.float64)
    h = width // 2
    for t in range(N):
        s = min(max(t - h, 0), N - width)
        out[t] = rows[t - s] @ x[s:s + width]
    return out


def features(y, name: str, n_fft: int, hop_ms, window_ms, n_mels=None, n_mfcc=None, deltas: bool = False) -> np.ndarray:
    """[N, F] float64"""
    hop, win = samples(hop_ms), samples(window_ms)
    if name == "spectrogram":
        x = np.abs(stft(y, n_fft, hop, win, center=False))
    else:
        S = np.abs(stft(y, n_fft, hop, win, center=True)) ** 2
        mel = S @ mel_basis(n_fft, n_mels).T
        if name == "mel":
            x = mel
        elif name == "log-mel":
            x = np.log(mel + 1e-6)
        elif name == "mfcc":
            db = 10.0 * np.log10(np.maximum(1e-10, mel))
            db = np.maximum(db, db.max() - 80.0)
            x = db @ dct_ortho(n_mels, n_mfcc).T
        else:
            raise ValueError(name)
    if deltas:
        x = np.concatenate([x, delta(x, 1), delta(x, 2)], axis=1)
    return x


def log_mel_frames(y, n_fft: int, hop: int, win: int, n_mels: int, frames) -> np.ndarray:
    """rows `frames` of features(y, "log-mel", ...) without padding or framing the whole signal (long inputs)"""
    y = np.asarray(y)
    n = len(y)
    frames = np.asarray(frames)
    i = hop * frames[:, None] + np.arange(n_fft)[None, :] - n_fft // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    w = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = hann_periodic(win)
    S = np.abs(np.fft.rfft(y[i].astype(np.float64) * w[None, :], axis=1)) ** 2
    return np.log(S @ mel_basis(n_fft, n_mels).T + 1e-6)
