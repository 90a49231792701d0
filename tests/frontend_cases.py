"""The front-end geometries, signals and error model the generic feature front-end (savad_frontend, features.FrontEnd) is
held to: tests/test_frontend_cases_host.py on the CPU, tests/test_gpu_frontend_cases.py on the GPU -- TEST INFRASTRUCTURE ONLY, numpy.

A case states hop and window IN SAMPLES (hop_ms = hop / 16, window_ms = win / 16; the host test holds FrontEnd to the round trip).

group      what no earlier test entered                                            the wrong result it exists to expose (DEVIATIONS)
scalar     hop % 4 != 0: stft_kernel<false>, scalar loads from an unaligned source  hop_cut: frames cut at hop & ~3
offgrid    lpad % 4 != 0: k0 < lpad, zero weights in front of the window; k0 + kr   window_k0: the window placed at k0
           past n_fft (the spectrogram's choice between the audio and a copy)
sizes      n_fft 2048 / 640 / 16 / odd: row-block groups per wave                   (held by the truth alone)
widths     n_mels 1 / 64 / 65 / 256, empty filters, n_mfcc == n_mels, 64 and 65     (held by the truth alone)
frames     N = 1, 31 .. 129: the last workgroup's idle lanes, the GEMM's row tiles  last_copy: the last frame a copy of the one before
deltas     N = 9 .. 18: the two clamped edge regions overlap up to N = 16           delta_centred: edge frames filtered around themselves

signal      what it is for                                                          deviation
stepped     the same broadband content at 1, 1e-3, 1e-6, then exact zeros           quiet_zero: the 1e-6 stretch replaced by zeros
dc_nyquist  0.4 + 0.3 (-1)^n + noise: bins 0 and n_fft / 2 carry every frame        drop_nyq (bin n_fft / 2 zero), swap_dc_nyq (even n_fft)
quiet       amplitude 1e-4: every dB value of the MFCC is negative                  clamp_pos: the clamp taken from max(0, maximum)
zeros       all zero: the amin floor everywhere
chirp       tests/test_gpu_frontend.py's signal (its first third at 1e-3)

ERROR MODEL (`errors`): every frame in its own scale.
  mel, spectrogram  rel  = max over frames of max_c |got - want| / max_c |want|; a frame whose truth is exactly zero must equal it
  log-mel, mfcc     abs  = max |got - want|, med = median |got - want|; log-mel also mel_rel = the figure above for exp(got) - 1e-6
                    against the mel truth, over the cells with mel > 1e-4 (the log cannot hide a frame)
  differences       d_abs (log-mel, mfcc) / d_rel (mel, spectrogram: the scale of frame t is the largest |truth| of the 9 frames its
                    filter reads, since a difference of a steady frame has no scale of its own)
bound = 3 x floor per figure (`bounds`); floor = the same figure for `restate_fp32`, a plain fp32 restatement (tables rounded to fp32,
frames in fp32, every sum one fp32 multiply and one fp32 add at a time in index order, fp32 epilogues) against frontend_ref's float64.
The factor 3 is DESIGN §4r's: room for another accumulation order.  Nothing here is taken from a kernel.
The exception is `med`: it keeps today's bar (2e-6 log-mel, 1e-4 mfcc) as it is.  Where most cells of a matrix are the constant
log(1e-6) (silence, empty filters) the median IS the error of one value of logf, and numpy's fp32 log is correctly rounded while a device
logf (log2 in hardware, times ln 2) is specified to 1 - 2 ulp (ulp(13.8) = 9.5e-7): 3 x the restatement's median says nothing about it."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import frontend_ref as ref

Case = namedtuple("Case", "id group transform n_fft hop win n_mels n_mfcc")
Run = namedtuple("Run", "case signal n")      # one call: a case on `signal` of n samples
FACTOR = 3.0
OLD_BARS = {"log-mel": (5e-4, 2e-6), "mfcc": (5e-3, 1e-4), "mel": (1e-5, None), "spectrogram": (1e-5, None)}   # tests/test_gpu_frontend._check
f32 = np.float32


def _c(group, transform, n_fft, hop, win, n_mels=None, n_mfcc=None):
    tail = "" if n_mels is None else f"-{n_mels}" + ("" if n_mfcc is None else f"-{n_mfcc}")
    return Case(f"{transform}-{n_fft}-{hop}-{win}{tail}", group, transform, n_fft, hop, win, n_mels, n_mfcc)


SP402 = _c("offgrid", "spectrogram", 402, 160, 401)          # k0 + kr = 408 > n_fft: run at four placements by its own test
FRAMES_CENTRED = _c("frames", "log-mel", 64, 40, 64, 10)     # N = 1 needs hop > n_fft / 2 + 1 under reflect padding
FRAMES_SPEC = _c("frames", "spectrogram", 64, 41, 64)        # the scalar-load kernel at the tile edges
FRAME_COUNTS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129]
DELTA_COUNTS = [9, 10, 12, 13, 16, 17, 18]

# (case, signals)
_TABLE = [
    # ---- scalar-load STFT ----
    (_c("scalar", "log-mel", 512, 161, 400, 80), ("chirp", "stepped")),
    (_c("scalar", "mel", 512, 161, 400, 80), ("chirp", "stepped")),
    (_c("scalar", "mfcc", 512, 101, 400, 40, 13), ("chirp", "stepped", "quiet", "zeros")),
    (_c("scalar", "spectrogram", 320, 161, 320), ("chirp", "stepped", "dc_nyquist")),
    (_c("scalar", "spectrogram", 320, 162, 320), ("chirp",)),
    (_c("scalar", "spectrogram", 320, 163, 320), ("chirp",)),
    (_c("scalar", "spectrogram", 64, 1, 64), ("chirp",)),
    (_c("scalar", "log-mel", 512, 602, 400, 80), ("chirp",)),
    # ---- off-grid window ----
    (_c("offgrid", "log-mel", 500, 160, 400, 80), ("chirp", "stepped")),
    (_c("offgrid", "log-mel", 512, 160, 401, 80), ("chirp",)),
    (_c("offgrid", "log-mel", 500, 160, 401, 80), ("chirp",)),
    (_c("offgrid", "spectrogram", 512, 160, 401), ("chirp", "dc_nyquist")),
    (SP402, ("chirp",)),
    (_c("offgrid", "log-mel", 500, 101, 401, 40), ("chirp", "stepped")),     # with the scalar-load STFT
    # ---- sizes ----
    (_c("sizes", "mel", 2048, 160, 2048, 128), ("stepped",)),
    (_c("sizes", "log-mel", 2048, 200, 1600, 128), ("chirp",)),
    (_c("sizes", "spectrogram", 2048, 160, 2000), ("chirp",)),
    (_c("sizes", "mel", 640, 160, 400, 40), ("chirp", "dc_nyquist")),
    (_c("sizes", "mel", 16, 8, 16, 4), ("chirp",)),
    (_c("sizes", "spectrogram", 16, 8, 16), ("chirp", "dc_nyquist")),
    (_c("sizes", "spectrogram", 401, 160, 400), ("chirp", "dc_nyquist")),     # odd n_fft: no row 1
    # ---- widths ----
    (_c("widths", "mel", 512, 160, 400, 1), ("chirp",)),
    (_c("widths", "log-mel", 512, 160, 400, 64), ("chirp",)),
    (_c("widths", "mel", 512, 160, 400, 65), ("chirp",)),
    (_c("widths", "log-mel", 512, 160, 400, 256), ("chirp",)),
    (_c("widths", "log-mel", 400, 160, 400, 256), ("chirp",)),               # 45 empty filters: exactly log(1e-6)
    (_c("widths", "mfcc", 512, 160, 400, 40, 40), ("chirp", "quiet")),
    (_c("widths", "mfcc", 512, 160, 400, 80, 65), ("chirp",)),
    (_c("widths", "mfcc", 512, 160, 400, 64, 64), ("chirp", "zeros")),
]
CASES = [c for c, _ in _TABLE] + [FRAMES_CENTRED, FRAMES_SPEC]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def centred(case) -> bool:
    return case.transform != "spectrogram"


def hop_ms(case) -> float:
    return case.hop / 16.0


def window_ms(case) -> float:
    return case.win / 16.0


def front_end_args(case, deltas=False):
    """the arguments of features.FrontEnd"""
    return (case.transform, case.n_fft, hop_ms(case), window_ms(case), case.n_mels, case.n_mfcc, deltas)


def base_size(case) -> int:
    return {"spectrogram": case.n_fft // 2 + 1, "mfcc": case.n_mfcc}.get(case.transform, case.n_mels)


def geometry(case):
    """(lpad, k0, kr) as csrc/savad_audio_host.h's fe::geometry"""
    lpad = (case.n_fft - case.win) // 2
    k0 = lpad & ~3
    return lpad, k0, (lpad + case.win - k0 + 7) // 8 * 8


def frames_of(case, n: int) -> int:
    return ref.frame_count(case.transform, n, case.n_fft, case.hop)


def length_for(case, frames: int, extra: int = 0) -> int:
    """the shortest signal of `frames` frames, plus `extra` samples (extra < hop keeps the count)"""
    n = case.hop * (frames - 1) + (case.n_fft if not centred(case) else case.n_fft - 2 * (case.n_fft // 2)) + extra
    lo = case.n_fft if not centred(case) else case.n_fft // 2 + 1
    assert n >= lo and frames_of(case, n) == frames, (case.id, frames, n)
    return n


def default_length(case) -> int:
    """about a third of a second (37 frames at hop 160), 0.6 s at n_fft 2048; never fewer than 9 frames; the end ragged"""
    if case.n_fft == 2048:
        frames = 8000 // case.hop
    elif case.hop == 1:
        frames = 200
    else:
        frames = min(max(9, 5800 // case.hop), 130)
    return length_for(case, frames, min(case.hop - 1, 77))


def _runs():
    out = [Run(c, s, default_length(c)) for c, sigs in _TABLE for s in sigs]
    for N in FRAME_COUNTS:
        out.append(Run(FRAMES_CENTRED, "chirp", length_for(FRAMES_CENTRED, N, 33 if N == 1 else 7)))   # N = 1: n = 33 .. 39
        out.append(Run(FRAMES_SPEC, "chirp", length_for(FRAMES_SPEC, N, 7)))
    for N in DELTA_COUNTS:
        out.append(Run(FRAMES_CENTRED, "stepped", length_for(FRAMES_CENTRED, N, 7)))
    return out


RUNS = _runs()


def run_id(r) -> str:
    return f"{r.case.id}-{r.signal}-N{frames_of(r.case, r.n)}"


assert len({run_id(r) for r in RUNS}) == len(RUNS)


# ---- signals ------------------------------------------------------------------------------------------------------------------------

def chirp(n, seed=0):
    from tests.test_gpu_frontend import _chirp

    return _chirp(n, seed)


def _broadband(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.1 * np.sin(2 * np.pi * 6500 * t) + 0.05 * rng.standard_normal(n)


def stepped_edges(n):
    """first samples of the 1e-3, 1e-6 and zero stretches: odd, so that they fall on no frame boundary of an even hop"""
    return [int(n * f) | 1 for f in (0.28, 0.52, 0.78)]


def stepped(n, seed=1, quiet_zero=False):
    a, b, c = stepped_edges(n)
    y = _broadband(n, seed)
    y[a:b] *= 1e-3
    y[b:c] *= 0.0 if quiet_zero else 1e-6
    y[c:] = 0.0
    return y.astype(f32)


def dc_nyquist(n, seed=2):
    return (0.4 + 0.3 * (1 - 2 * (np.arange(n) & 1)) + 0.01 * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def quiet(n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (1e-4 * (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 1e-3 * rng.standard_normal(n))).astype(f32)


def zeros(n, seed=0):
    return np.zeros(n, dtype=f32)


SIGNALS = {"chirp": chirp, "stepped": stepped, "dc_nyquist": dc_nyquist, "quiet": quiet, "zeros": zeros}


@functools.lru_cache(maxsize=None)
def signal(r):
    y = SIGNALS[r.signal](r.n)
    y.setflags(write=False)
    return y


# ---- the float64 truth, with the deviations ---------------------------------------------------------------------------------------

def _window(case, at=None):
    lpad = (case.n_fft - case.win) // 2
    at = lpad if at is None else at
    w = np.zeros(case.n_fft)
    w[at:at + case.win] = ref.hann_periodic(case.win) if centred(case) else ref.hamming_periodic(case.win)
    return w


def _delta(x, order, centred_edges=False):
    if not centred_edges:
        return ref.delta(x, order)
    rows = ref.savgol_rows(order)
    N = x.shape[0]
    idx = np.clip(np.arange(N)[:, None] - 4 + np.arange(9)[None, :], 0, N - 1)     # frames outside the recording repeat its edge
    return np.einsum("j,tjc->tc", rows[4], x[idx])


def truth(case, y, deltas=False, deviation=None, parts=False):
    """[N, F] float64: frontend_ref.features(...), or the wrong result `deviation` names.  parts: (features, mel or None)"""
    dev = deviation
    if dev is None:
        x = ref.features(y, *front_end_args(case)[:6], deltas)
        if not parts:
            return x
        mel = None if not centred(case) else np.abs(ref.stft(y, case.n_fft, case.hop, case.win, True)) ** 2 @ ref.mel_basis(case.n_fft, case.n_mels).T
        return x, mel
    y = np.asarray(y, dtype=np.float64)
    if dev == "quiet_zero":
        a, b, c = stepped_edges(len(y))
        y = y.copy()
        y[b:c] = 0.0
    N = frames_of(case, len(y))
    hop = case.hop & ~3 if dev == "hop_cut" else case.hop
    w = _window(case, geometry(case)[1] if dev == "window_k0" else None)
    yp = np.pad(y, case.n_fft // 2, mode="reflect") if centred(case) else y
    idx = hop * np.arange(N)[:, None] + np.arange(case.n_fft)[None, :]
    mag = np.abs(np.fft.rfft(yp[idx] * w[None, :], axis=1))
    h = case.n_fft // 2
    if dev == "drop_nyq":
        mag[:, h] = 0.0
    if dev == "swap_dc_nyq":
        mag[:, [0, h]] = mag[:, [h, 0]]
    if not centred(case):
        x = mag
    else:
        mel = mag ** 2 @ ref.mel_basis(case.n_fft, case.n_mels).T
        if case.transform == "mel":
            x = mel
        elif case.transform == "log-mel":
            x = np.log(mel + 1e-6)
        else:
            db = 10.0 * np.log10(np.maximum(1e-10, mel))
            db = np.maximum(db, (max(0.0, db.max()) if dev == "clamp_pos" else db.max()) - 80.0)
            x = db @ ref.dct_ortho(case.n_mels, case.n_mfcc).T
    if dev == "last_copy":
        x[-1] = x[-2]
    if deltas:
        x = np.concatenate([x, _delta(x, 1, dev == "delta_centred"), _delta(x, 2, dev == "delta_centred")], axis=1)
    return x


def deviations(r, deltas=False):
    """the wrong results this run must tell from the truth"""
    c, N = r.case, frames_of(r.case, r.n)
    out = []
    if r.signal == "zeros":     # (no geometry shows on silence)
        return out
    if c.hop % 4 and N >= 2:
        out.append("hop_cut")
    if geometry(c)[0] != geometry(c)[1]:
        out.append("window_k0")
    if r.signal == "dc_nyquist" and not centred(c):      # (the mel filters weigh bins 0 and n_fft / 2 with zero: a mel cannot see them)
        out.append("drop_nyq")
        if c.n_fft % 2 == 0:
            out.append("swap_dc_nyq")
    if r.signal == "stepped" and c.group != "frames":
        out.append("quiet_zero")
    if r.signal == "quiet" and c.transform == "mfcc":
        out.append("clamp_pos")
    if c.group == "frames" and r.signal == "chirp" and N >= 2:
        out.append("last_copy")
    if deltas and c.group == "frames" and r.signal == "stepped":
        out.append("delta_centred")
    return out


# ---- the plain fp32 restatement (the floor) -----------------------------------------------------------------------------------------

def dft_tables_f32(case):
    """(cos [nb, n_fft], -sin [nb, n_fft]) window-folded, computed in float64 and rounded to fp32 (as test_frontend_host._dft_ref)"""
    w = _window(case)
    k = np.arange(case.n_fft)
    b = np.arange(case.n_fft // 2 + 1)[:, None]
    ph = 2.0 * np.pi * ((b * k[None, :]) % case.n_fft) / case.n_fft
    return (w * np.cos(ph)).astype(f32), (-w * np.sin(ph)).astype(f32)


def _seq_matmul(a, w):
    """a [M, K] @ w [N, K].T in fp32: acc = fl(acc + fl(a_k * w_k)) for k in index order (columns of zero weights skipped: they add +0)"""
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=f32)
    for k in np.flatnonzero(np.any(w != 0, axis=0)):
        acc += a[:, k, None] * w[None, :, k]
    return acc


def restate_fp32(case, y, deltas=False, base=None):
    """[N, F] float32 (base: the result without differences, if the caller has it)"""
    if base is not None:
        return restate_deltas_fp32(base) if deltas else base
    y = np.asarray(y, dtype=f32)
    N = frames_of(case, len(y))
    yp = np.pad(y, case.n_fft // 2, mode="reflect") if centred(case) else y
    fr = yp[case.hop * np.arange(N)[:, None] + np.arange(case.n_fft)[None, :]]
    co, si = dft_tables_f32(case)
    re, im = _seq_matmul(fr, co), _seq_matmul(fr, si)
    pw = re * re + im * im
    if not centred(case):
        x = np.sqrt(pw)
    else:
        mel = _seq_matmul(pw, ref.mel_basis(case.n_fft, case.n_mels).astype(f32))
        if case.transform == "mel":
            x = mel
        elif case.transform == "log-mel":
            x = np.log(mel + f32(1e-6))
        else:
            db = f32(10.0) * np.log10(np.maximum(f32(1e-10), mel))
            db = np.maximum(db, db.max() - f32(80.0))
            x = _seq_matmul(db, ref.dct_ortho(case.n_mels, case.n_mfcc).astype(f32))
    assert x.dtype == f32
    return restate_deltas_fp32(x) if deltas else x


def restate_deltas_fp32(x):
    """[N, F] float32 -> [N, 3F]: the Savitzky-Golay sums of delta_kernel, one fp32 multiply and add at a time"""
    N = x.shape[0]
    cols = [x]
    for order in (1, 2):
        rows = ref.savgol_rows(order).astype(f32)
        d = np.zeros_like(x)
        for t in range(N):
            s = min(max(t - 4, 0), N - 9)
            for j in range(9):
                d[t] += rows[t - s, j] * x[s + j]
        cols.append(d)
    x = np.concatenate(cols, axis=1)
    assert x.dtype == f32
    return x


# ---- the error model ----------------------------------------------------------------------------------------------------------------

def _frame_rel(got, want, scale=None):
    """(max over the frames with a non-zero scale of max_c |got - want| / scale, whether the other frames equal the truth)"""
    d = np.abs(got - want).max(axis=1)
    s = np.abs(want).max(axis=1) if scale is None else scale
    nz = s > 0
    return (float((d[nz] / s[nz]).max()) if nz.any() else 0.0), bool(np.array_equal(got[~nz], want[~nz]))


def errors(case, got, want, mel=None):
    """figure name -> value, in the norms of the module docstring.  got / want: [N, F] or [N, 3F]; mel: the float64 mel truth (log-mel).
    `exact` = every frame whose truth is exactly zero equals it (mel / spectrogram)."""
    got = np.asarray(got, dtype=np.float64)
    F = base_size(case)
    g, w = got[:, :F], want[:, :F]
    out = {}
    if case.transform in ("mel", "spectrogram"):
        out["rel"], out["exact"] = _frame_rel(g, w)
    else:
        d = np.abs(g - w)
        out["abs"], out["med"] = float(d.max()), float(np.median(d))
        if case.transform == "log-mel":
            m = mel > 1e-4
            rows = m.any(axis=1)
            if rows.any():
                out["mel_rel"] = _frame_rel(np.where(m, np.exp(g) - 1e-6, 0.0)[rows], np.where(m, mel, 0.0)[rows])[0]
    if got.shape[1] == 3 * F:
        N = got.shape[0]
        for o in (1, 2):
            gd, wd = got[:, o * F:(o + 1) * F], want[:, o * F:(o + 1) * F]
            if case.transform in ("mel", "spectrogram"):
                fmax = np.abs(w).max(axis=1)
                scale = np.array([fmax[min(max(t - 4, 0), N - 9):][:9].max() for t in range(N)])
                rel, exact = _frame_rel(gd, wd, scale)
                out["d_rel"] = max(out.get("d_rel", 0.0), rel)
                out["exact"] = out["exact"] and exact
            else:
                out["d_abs"] = max(out.get("d_abs", 0.0), float(np.abs(gd - wd).max()))
    return out


@functools.lru_cache(maxsize=None)
def _truth_cached(r, deltas):
    x, mel = truth(r.case, signal(r), deltas, parts=True)
    x.setflags(write=False)
    return x, mel


def run_truth(r, deltas=False):
    """(float64 features, float64 mel or None) of a run: computed once, read-only"""
    return _truth_cached(r, deltas)


@functools.lru_cache(maxsize=None)
def _restated_base(r):
    return restate_fp32(r.case, signal(r))


@functools.lru_cache(maxsize=None)
def floors(r, deltas=False):
    """the figures of the fp32 restatement for a run"""
    want, mel = run_truth(r, deltas)
    e = errors(r.case, restate_fp32(r.case, None, deltas, base=_restated_base(r)), want, mel)
    assert e.pop("exact", True), "the fp32 restatement of a silent frame is not silent"
    return e


def bounds(r, deltas=False):
    return {k: OLD_BARS[r.case.transform][1] if k == "med" else FACTOR * v for k, v in floors(r, deltas).items()}


def old_bars(case, deltas=False):
    """today's bar per figure (tests/test_gpu_frontend._check; 2 x for the differences): no bound may be looser"""
    mx, med = OLD_BARS[case.transform]
    out = {"rel": mx} if med is None else {"abs": mx, "med": med}
    if case.transform == "log-mel":
        out["mel_rel"] = OLD_BARS["mel"][0]
    if deltas:
        out["d_rel" if med is None else "d_abs"] = 2 * mx
    return out


def check(r, got, deltas=False):
    """the assertion of the GPU tests: every figure of `got` within 3 x its floor; returns (figures, bounds)"""
    want, mel = run_truth(r, deltas)
    assert got.shape == want.shape, (got.shape, want.shape)
    e, b = errors(r.case, got, want, mel), bounds(r, deltas)
    assert e.pop("exact", True), f"{run_id(r)}: a frame whose truth is exactly zero is not zero"
    assert set(e) == set(b)
    bad = {k: (e[k], b[k]) for k in e if not e[k] <= b[k]}
    assert not bad, f"{run_id(r)} deltas={deltas}: (error, bound) {bad}; all figures {e}"
    return e, b
