"""Clip tables: many recordings as slices of one concatenated feature matrix (include/savad.h, "many clips in one call").

``clip_first [C + 1]`` (int32, non-decreasing, ``clip_first[0] = 0``): clip ``c`` owns rows ``[clip_first[c], clip_first[c + 1])``.
Host arithmetic only -- nothing here touches the GPU."""
from __future__ import annotations

import math

import numpy as np

ROW_LIMIT = 2 ** 31 - 1   # an int32 table names no more rows


def clip_table(lengths) -> np.ndarray:
    """row counts of the clips, in order -> clip_first [C + 1] int32 (at least one clip; an empty clip is legal)"""
    n = np.asarray(list(lengths), dtype=np.int64)
    if n.ndim != 1 or n.size < 1:
        raise ValueError("a clip table needs at least one clip")
    if (n < 0).any():
        raise ValueError("a clip cannot have a negative number of rows")
    first = np.zeros(n.size + 1, dtype=np.int64)
    np.cumsum(n, out=first[1:])
    if first[-1] > ROW_LIMIT:
        raise ValueError(f"{int(first[-1])} rows in all: a clip table holds at most {ROW_LIMIT}")
    return first.astype(np.int32)


def check_clip_table(clip_first) -> np.ndarray:
    """anything that lists a table -> the int32 array the library takes, or ValueError for what is not a clip table"""
    t = np.asarray(clip_first)
    if t.ndim != 1 or t.size < 2 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("clip_first must be a 1-D integer array of C + 1 >= 2 entries")
    t = t.astype(np.int64)
    if t[0] != 0 or (np.diff(t) < 0).any() or t[-1] > ROW_LIMIT:
        raise ValueError("clip_first must start at 0, must not decrease and must end at no more than 2^31 - 1")
    return np.ascontiguousarray(t, dtype=np.int32)


def window_items(clip_first, half: int) -> np.ndarray:
    """items_first [C + 1]: the exclusive prefix sum of the clips' window counts max(0, rows - 2 half) (vad/predictor.py:169)"""
    n = np.maximum(np.diff(np.asarray(clip_first, dtype=np.int64)) - 2 * int(half), 0)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def audio_clip_table(lengths, align: int = 4):
    """sample counts of the clips, in order -> (table [C, 2] int64 of (first, count), audio_count): the clips one after the other in
    ONE buffer of audio_count samples, every `first` rounded up to a multiple of `align` samples (savad_logmel_batch reads 16-byte
    chunks straight from a clip: 4 floats; 8 also suits a PCM16 staging buffer converted in 8-byte pieces).  An empty clip is legal."""
    n = np.asarray(list(lengths), dtype=np.int64)
    align = int(align)
    if n.ndim != 1 or n.size < 1:
        raise ValueError("an audio clip table needs at least one clip")
    if (n < 0).any():
        raise ValueError("a clip cannot have a negative number of samples")
    if align < 4 or align % 4:
        raise ValueError("align must be a positive multiple of 4 samples")
    table = np.zeros((n.size, 2), dtype=np.int64)
    table[:, 1] = n
    padded = (n + align - 1) // align * align
    table[1:, 0] = np.cumsum(padded[:-1])
    return table, int(table[-1, 0] + n[-1])


def split_by_clip(rows, clip_first) -> list:
    """rows [sum N, ...] (array or tensor) -> one view per clip, in order: rows[clip_first[c]:clip_first[c + 1]]"""
    t = [int(v) for v in clip_first]
    if len(rows) != t[-1]:
        raise ValueError(f"{len(rows)} rows for a table of {t[-1]}")
    return [rows[a:b] for a, b in zip(t[:-1], t[1:])]


def chunk_bounds(n_samples: int, sample_rate: int, split_max_seconds):
    """(seconds per chunk, [(start sample, end sample)]): the chunks VADFromScratchPredictor.predict cuts a recording into
    (vad/predictor.py:86-93) -- equal lengths of at most split_max_seconds; None: the recording as one chunk."""
    duration_s = n_samples / sample_rate
    num_chunks = math.ceil(duration_s / split_max_seconds) if split_max_seconds is not None else 1
    adjusted = duration_s / num_chunks
    return adjusted, [(int(ci * adjusted * sample_rate), int((ci + 1) * adjusted * sample_rate)) for ci in range(num_chunks)]
