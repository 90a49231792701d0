"""Post-processing of the predict path -- same function names and semantics as the reference's
``vad/postprocessing/{trim,convert,split}.py``, executed by the native host code in libsavad.so
(``csrc/savad_post.h``).  Pinned by goldens produced with the reference functions themselves
(``tests/golden/make_golden_post.py``)."""
from __future__ import annotations

import ctypes
from datetime import timedelta

import numpy as np
import torch

from . import _lib


def trim_voice_activity(predictions, min_vally=20, min_hill=20, hang_before=10, hang_over=10):
    """vad/postprocessing/trim.py:4-66.  predictions: 0/1 (or bool) per frame; returns the same dtype."""
    p = np.ascontiguousarray(predictions)
    src = (p != 0).astype(np.uint8)
    out = np.empty_like(src)
    _lib.check(_lib.load().savad_trim_voice_activity(src, len(src), int(min_vally), int(min_hill), int(hang_before), int(hang_over), out))
    return out.astype(p.dtype)


def convert_frames_to_samples(frames, sample_rate=16000, hop_ms=10, window_ms=10):
    """vad/postprocessing/convert.py:6-24 (float64 result, like numpy.zeros)."""
    f = np.ascontiguousarray(frames, dtype=np.float64)
    lib = _lib.load()
    n = lib.savad_frames_to_samples(f, len(f), int(sample_rate), float(hop_ms), float(window_ms), None)
    if n < 0:
        _lib.check(int(n))
    out = np.empty(int(n), dtype=np.float64)
    lib.savad_frames_to_samples(f, len(f), int(sample_rate), float(hop_ms), float(window_ms), out)
    return out


def segment_indices(samples):
    """(start, end) SAMPLE indices of convert_samples_to_segments' segments."""
    s = np.ascontiguousarray(samples, dtype=np.float64)
    lib = _lib.load()
    cnt = lib.savad_samples_to_segments(s, len(s), None, None, 0)
    if cnt < 0:
        _lib.check(cnt)
    starts = np.empty(cnt, dtype=np.int64)
    ends = np.empty(cnt, dtype=np.int64)
    if cnt:
        lib.savad_samples_to_segments(s, len(s), starts, ends, cnt)
    return starts, ends


def convert_samples_to_segments(samples, sample_rate=16000):
    """vad/postprocessing/convert.py:27-61: list of (start, end) timedeltas (seconds = index / sample_rate)."""
    starts, ends = segment_indices(samples)
    return [(timedelta(seconds=int(a) / sample_rate), timedelta(seconds=int(b) / sample_rate)) for a, b in zip(starts, ends)]


def optimal_split_voice_activity(sample_predictions, sample_probs, max_length_seconds=300, sample_rate=16000):
    """vad/postprocessing/split.py:26-78."""
    pred = np.ascontiguousarray(sample_predictions, dtype=np.float64)
    probs = np.ascontiguousarray(sample_probs, dtype=np.float64)
    out = np.empty_like(pred)
    _lib.check(_lib.load().savad_optimal_split(pred, probs, len(pred), int(max_length_seconds * sample_rate), out))
    return out


# ---- the same on the device (csrc/savad_post_device.h): probabilities -> segments without host arrays -------------------------

def device_post_supported(W, sample_rate=16000, hop_ms=10, window_ms=25, n_frames=0) -> bool:
    """savad_post_supported: 1 <= W <= 128 and a hop of a whole number of samples (>= 1); host arithmetic only."""
    if sample_rate is None:
        return False
    return bool(_lib.load().savad_post_supported(int(W), int(sample_rate), float(hop_ms), float(window_ms), int(n_frames)))


def _post_workspace(n_frames, W, sample_rate, hop_ms, window_ms, device):
    need = ctypes.c_size_t()
    _lib.check(_lib.load().savad_post_workspace_bytes(int(n_frames), int(W), int(sample_rate), float(hop_ms), float(window_ms), ctypes.byref(need)))
    return torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=device), int(need.value)


def post_frames_device(probs, threshold=0.5, min_vally=0, min_hill=0, hang_before=0, hang_over=0):
    """probs [N, W] float32 on the device -> (boosted [N] float32, trimmed [N] uint8), both on the device: numpy's
    probs.mean(axis=1), and trim_voice_activity(boosted > threshold, ...).  Asynchronous on the current stream."""
    _lib.check_tensor(probs, "probs", torch.float32, 2, contiguous=False)
    probs = probs.contiguous()
    N, W = probs.shape
    with _lib.on_device(probs.device):
        boosted = torch.empty((N,), dtype=torch.float32, device=probs.device)
        trimmed = torch.empty((N,), dtype=torch.uint8, device=probs.device)
        # (the frame stage's share of the workspace does not depend on the geometry: asked for at one sample per frame, the smallest)
        ws, ws_bytes = _post_workspace(N, W, 1000, 1, 1, probs.device)
        _lib.check(_lib.load().savad_post_frames(probs, N, W, float(threshold), int(min_vally), int(min_hill), int(hang_before),
                                                 int(hang_over), boosted, trimmed, ws, ws_bytes, torch.cuda.current_stream(probs.device)))
    return boosted, trimmed


def segments_device(trimmed, boosted=None, sample_rate=16000, hop_ms=10, window_ms=25, max_length_seconds=None, cap=None):
    """trimmed [N] uint8 (0 / 1) on the device -> (starts, ends): numpy int64 SAMPLE indices, what
    segment_indices(convert_frames_to_samples(trimmed, ...)) gives; with max_length_seconds (and boosted [N] float32 on the
    device) after optimal_split_voice_activity against convert_frames_to_samples(boosted, ...).  Synchronises the current
    stream (with a split: once more per range query, on the order of length / max_length per long segment).
    `cap`: room for that many segments on the first call (default: one per frame); a second call fetches a larger count."""
    _lib.check_tensor(trimmed, "trimmed", torch.uint8, 1, contiguous=False)
    trimmed = trimmed.contiguous()
    N = int(trimmed.shape[0])
    max_samples = int(max_length_seconds * sample_rate) if max_length_seconds else 0
    if max_samples:
        _lib.check_tensor(boosted, "boosted (a split needs it)", torch.float32, shape=(N,), device=trimmed.device, contiguous=False)
        boosted = boosted.contiguous()
    lib = _lib.load()
    with _lib.on_device(trimmed.device):
        ws, ws_bytes = _post_workspace(N, 1, sample_rate, hop_ms, window_ms, trimmed.device)
        cap = N + 2 if cap is None else int(cap)
        while True:
            starts, ends = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
            cnt = lib.savad_post_segments(trimmed, boosted if max_samples else None, N, int(sample_rate), float(hop_ms), float(window_ms),
                                          max_samples, starts, ends, cap, ws, ws_bytes, torch.cuda.current_stream(trimmed.device))
            if cnt < 0:
                _lib.check(cnt)
            if cnt <= cap:
                return starts[:cnt], ends[:cnt]
            cap = cnt   # (a split into more pieces than frames)


# ---- every clip of a batch at once (csrc/savad_post_batch.h): launches and synchronisations do not grow with the clips ---------

def device_post_many_supported(table, W, sample_rate=16000, hop_ms=10, window_ms=25) -> bool:
    """savad_post_batch_supported: a clip table whose every clip device_post_supported takes; host arithmetic only."""
    if sample_rate is None:
        return False
    table = np.ascontiguousarray(table, dtype=np.int32)
    return bool(_lib.load().savad_post_batch_supported(table, len(table) - 1, int(W), int(sample_rate), float(hop_ms), float(window_ms)))


def slot_table(table, sample_rate=16000, hop_ms=10, window_ms=25) -> np.ndarray:
    """slot_first [C + 1] int64 of a clip table: a clip with frames owns its samples and one closing slot, a clip without owns nothing"""
    table = np.ascontiguousarray(table, dtype=np.int32)
    out = np.empty(len(table), dtype=np.int64)
    _lib.check(_lib.load().savad_post_batch_slot_table(table, len(table) - 1, int(sample_rate), float(hop_ms), float(window_ms), out))
    return out


def _clip_tables(table, table_dev, rows, device):
    """the host table checked against the matrix it describes, and its device copy (uploaded when the caller has none)"""
    from .clips import check_clip_table

    table = check_clip_table(table)
    if int(table[-1]) != int(rows):
        raise ValueError(f"the clip table ends at row {int(table[-1])}, the matrix has {int(rows)}")
    if table_dev is None:
        table_dev = torch.from_numpy(table).to(device)
    _lib.check_tensor(table_dev, "table_dev", torch.int32, shape=(len(table),), device=device)
    return table, table_dev


def _post_batch_workspace(table, W, sample_rate, hop_ms, window_ms, device):
    need = ctypes.c_size_t()
    _lib.check(_lib.load().savad_post_batch_workspace_bytes(table, len(table) - 1, int(W), int(sample_rate), float(hop_ms), float(window_ms),
                                                            ctypes.byref(need)))
    return torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=device), int(need.value)


def post_frames_device_many(probs, table, table_dev=None, threshold=0.5, min_vally=0, min_hill=0, hang_before=0, hang_over=0):
    """post_frames_device for every clip of a batch in one pass: probs [sum N, W] float32 on the device, `table` its clip table
    (clips.clip_table; `table_dev` its int32 copy on the device, uploaded here when None) -> (boosted [sum N], trimmed [sum N]) on
    the device, each clip's rows holding post_frames_device of that clip alone.  Asynchronous on the current stream."""
    _lib.check_tensor(probs, "probs", torch.float32, 2, contiguous=False)
    probs = probs.contiguous()
    N, W = probs.shape
    table, table_dev = _clip_tables(table, table_dev, N, probs.device)
    with _lib.on_device(probs.device):
        boosted = torch.empty((N,), dtype=torch.float32, device=probs.device)
        trimmed = torch.empty((N,), dtype=torch.uint8, device=probs.device)
        # (the frame stage's share of the workspace does not depend on the geometry: asked for at one sample per frame, the smallest)
        ws, ws_bytes = _post_batch_workspace(table, W, 1000, 1, 1, probs.device)
        _lib.check(_lib.load().savad_post_batch_frames(probs, table, table_dev, len(table) - 1, W, float(threshold), int(min_vally), int(min_hill),
                                                       int(hang_before), int(hang_over), boosted, trimmed, ws, ws_bytes,
                                                       torch.cuda.current_stream(probs.device)))
    return boosted, trimmed


def segments_device_many(trimmed, table, table_dev=None, boosted=None, sample_rate=16000, hop_ms=10, window_ms=25, max_length_seconds=None,
                         cap=None, return_long=False):
    """segments_device for every clip of a batch: trimmed [sum N] uint8 on the device and its clip table -> (seg_first [C + 1],
    starts, ends), numpy int64: clip c's segments are starts / ends [seg_first[c]:seg_first[c + 1]], SAMPLE indices local to the
    clip, what segments_device gives for the clip alone.  With max_length_seconds (and boosted [sum N]) the clips that hold a longer
    segment are found on the device and go through segments_device's split one by one; `return_long` appends their flags [C]
    (uint8) to the result.  Synchronises the current stream twice when no clip is split, whatever the number of clips."""
    _lib.check_tensor(trimmed, "trimmed", torch.uint8, 1, contiguous=False)
    trimmed = trimmed.contiguous()
    N = int(trimmed.shape[0])
    table, table_dev = _clip_tables(table, table_dev, N, trimmed.device)
    C = len(table) - 1
    max_samples = int(max_length_seconds * sample_rate) if max_length_seconds else 0
    if max_samples:
        _lib.check_tensor(boosted, "boosted (a split needs it)", torch.float32, shape=(N,), device=trimmed.device, contiguous=False)
        boosted = boosted.contiguous()
    lib = _lib.load()
    with _lib.on_device(trimmed.device):
        ws, ws_bytes = _post_batch_workspace(table, 1, sample_rate, hop_ms, window_ms, trimmed.device)
        cap = N + 2 * C if cap is None else int(cap)
        seg_first, long_clips = np.zeros(C + 1, dtype=np.int64), np.zeros(C, dtype=np.uint8)
        while True:
            starts, ends = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
            cnt = lib.savad_post_batch_segments(trimmed, boosted if max_samples else None, table, table_dev, C, int(sample_rate), float(hop_ms),
                                                float(window_ms), max_samples, seg_first, long_clips, starts, ends, cap, ws, ws_bytes,
                                                torch.cuda.current_stream(trimmed.device))
            if cnt < 0:
                _lib.check(cnt)
            if cnt <= cap:
                result = (seg_first, starts[:cnt], ends[:cnt])
                return result + (long_clips,) if return_long else result
            cap = cnt   # (splits into more pieces than frames)


def sample_probs_device(boosted, sample_rate=16000, hop_ms=10, window_ms=25):
    """boosted [N] float32 on the device -> convert_frames_to_samples(boosted, ...) as a float64 tensor on the device.  Asynchronous."""
    _lib.check_tensor(boosted, "boosted", torch.float32, 1, contiguous=False)
    boosted = boosted.contiguous()
    N = int(boosted.shape[0])
    # savad_frames_to_samples' count, int((n-1)*hop + window), in the same double arithmetic
    num = max(int((N - 1) * (int(sample_rate) * float(hop_ms) / 1000) + int(sample_rate) * float(window_ms) / 1000), 0)
    with _lib.on_device(boosted.device):
        out = torch.empty((int(num),), dtype=torch.float64, device=boosted.device)
        _lib.check(_lib.load().savad_post_sample_probs(boosted, N, int(sample_rate), float(hop_ms), float(window_ms), out,
                                                       torch.cuda.current_stream(boosted.device)))
    return out
