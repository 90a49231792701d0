"""Inputs of the batched device-metrics tests (tests/test_eval_batch_host.py on the CPU, tests/test_gpu_eval_batch.py on the GPU) and
the calls they share -- TEST INFRASTRUCTURE ONLY.  A batch is (clips, threshold); a clip is (probs [N, W] float32, labels [n_labels]
int64) as in tests/eval_cases.py.  The shapes are the smallest at which each mechanism of csrc/savad_eval_batch.h can go wrong."""
import functools

import numpy as np

from tests.eval_cases import L, counts_host, edge_cases, planted
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.metrics import EVAL_COUNTERS

RAGGED_ROWS = (0, 1, 2, 63, 64, 65, 0, 129, 7, 300)


def empty(W):
    return np.zeros((0, W), dtype=np.float32), np.zeros(0, dtype=np.int64)


def ragged(W, rotation, rows=RAGGED_ROWS):
    """labels equal to, 3 shorter than, 3 longer than, or empty against the rows, in rotation"""
    clips = []
    for i, N in enumerate(rows):
        n_labels = (N, max(N - 3, 0), N + 3, 0)[(i + rotation) % 4]
        if N == 0:
            clips.append((empty(W)[0], planted(2, W, n_labels)[1][:n_labels] if n_labels else empty(W)[1]))
        else:
            clips.append(planted(N, W, n_labels))
    return clips


def tie_across_boundaries():
    """the last row of clip c and the first row of clip c + 1 carry the same boosted score bits with opposite labels"""
    clips = []
    for c, N in enumerate((65, 64, 66, 9)):
        probs, labels = (a.copy() for a in planted(N, 7))
        probs[0], probs[-1] = np.float32(0.625), np.float32(0.625)
        labels[0], labels[-1] = c % 2, c % 2   # clip c ends with c % 2, clip c + 1 starts with (c + 1) % 2: the opposite
        labels[1] = 1 - labels[0]              # both classes whatever the pattern drew
        clips.append((probs, labels))
    for (_, a), (_, b) in zip(clips[:-1], clips[1:]):
        assert a[-1] != b[0]
    return clips


def cut(case):
    return case[0], case[1]


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (clips, threshold)"""
    e6, e65, e130 = edge_cases(6), edge_cases(65), edge_cases(130)
    out = {}
    for rotation in range(4):
        out[f"ragged W7 rotation {rotation}"] = (ragged(7, rotation), 0.5)
    for W in (1, 8, 128):
        out[f"ragged W{W}"] = (ragged(W, 1), 0.5)
    out["ragged with a clip of many blocks"] = (ragged(7, 1, RAGGED_ROWS + (1100, 0, 5)), 0.3)
    out["tie across a boundary"] = (tie_across_boundaries(), 0.5)
    out["all scores of all clips equal"] = ([cut(e["all scores equal"]) for e in (e65, e6, e130, e65)], 0.5)
    out["k/16-quantised scores"] = ([cut(e["ties k/16"]) for e in (e65, e130, e6, e65)], 0.5)
    ends, inverted = cut(e65["segments at both ends"]), cut(e65["segments at both ends, inverted"])
    out["segments at the ends"] = ([ends, ends, inverted, inverted, ends, inverted], 0.5)
    big_probs, big_labels = planted(1500, 7)
    many, at = [], 0
    for i in range(300):
        n = 1 + (i * 7 + i // 9) % 9
        many.append((big_probs[at:at + n], big_labels[at:at + n]))
        at += n - 1   # (clips overlap by a frame in the source: unrelated to the batch, which sees them as separate clips)
    out["many clips"] = (many, 0.5)
    out["bad clips among good ones"] = ([planted(65, 7), cut(e65["a NaN score"]), planted(40, 7), cut(e65["a label of 2"]), planted(7, 7)], 0.5)
    zeros = e65["minus zero"]
    wide_zeros = (np.repeat(zeros[0], 7, axis=1), zeros[1])
    out["zeros and mixed clips"] = ([planted(12, 7), wide_zeros, planted(65, 7), (wide_zeros[0], e65["minus zero, threshold below"][1])], 0.5)
    out["zeros, threshold below"] = ([wide_zeros, planted(30, 7)], -0.5)
    out["single-class clips"] = ([planted(30, 7), cut(e65["labels all 0"]), planted(65, 7), cut(e65["labels all 1"]), planted(12, 7)], 0.5)
    out["one clip"] = ([planted(301, 7)], 0.5)
    return out


BAD = {"bad clips among good ones": (1, 3)}   # the clips that report a NaN score / a label above 1


def concatenate(clips):
    """clips -> (probs_all [rows, W] float32, clip_first [C + 1] int32, labels_all uint8, label_first [C + 1] int32)"""
    W = clips[0][0].shape[1]
    probs_all = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, W) for p, _ in clips]))
    labels_all = np.ascontiguousarray(np.concatenate([np.asarray(y).astype(np.uint8) for _, y in clips]))
    clip_first = np.concatenate([[0], np.cumsum([len(p) for p, _ in clips])]).astype(np.int32)
    label_first = np.concatenate([[0], np.cumsum([len(y) for _, y in clips])]).astype(np.int32)
    return probs_all, clip_first, labels_all, label_first


def clip_frames(clip_first, label_first):
    return np.minimum(np.diff(clip_first.astype(np.int64)), np.diff(label_first.astype(np.int64)))


def segment_room(clip_first, label_first):
    return int(((clip_frames(clip_first, label_first) + 1) // 2).sum())


def counts_host_batch(clips, threshold, half_width=L, seg_cap=None):
    """savad_eval_batch_counts_host -> (count, counters [C, 16], seg [room, 8] filled with 0xEE behind the records, seg_first [C + 1])"""
    probs_all, clip_first, labels_all, label_first = concatenate(clips)
    C = len(clips)
    counters = np.full((C, EVAL_COUNTERS), -1, dtype=np.int64)
    seg = np.full((segment_room(clip_first, label_first) if seg_cap is None else seg_cap, 8), 0xEE, dtype=np.uint8)
    seg_first = np.full(C + 1, -1, dtype=np.int64)
    # (an array without elements has no address worth passing: the library wants a pointer it may offset)
    count = _lib.load().savad_eval_batch_counts_host(probs_all if probs_all.size else np.zeros(1, np.float32), clip_first,
                                                     labels_all if labels_all.size else np.zeros(1, np.uint8), label_first, C, probs_all.shape[1],
                                                     float(threshold), half_width, counters, seg if len(seg) else None, len(seg), seg_first)
    return count, counters, seg, seg_first


def per_clip_counts(clips, threshold, half_width=L):
    """what savad_eval_counts_host gives for every clip alone: [(counters, seg)]; a clip without a frame has zero counters and no record"""
    out = []
    for probs, labels in clips:
        if min(len(probs), len(labels)) == 0:
            out.append((np.zeros(EVAL_COUNTERS, dtype=np.int64), np.zeros((0, 8), dtype=np.uint8)))
        else:
            out.append(counts_host(probs, labels, threshold, half_width))
    return out


def assert_batch_equals_clips(name, got, want):
    """(count, counters, seg, seg_first) of a batched call against per_clip_counts"""
    count, counters, seg, seg_first = got
    assert count == sum(len(s) for _, s in want), (name, count)
    assert seg_first.tolist() == np.concatenate([[0], np.cumsum([len(s) for _, s in want])]).tolist(), name
    for c, (want_counters, want_seg) in enumerate(want):
        assert counters[c].tolist() == want_counters.tolist(), (name, c)
        assert np.array_equal(seg[seg_first[c]:seg_first[c + 1]], want_seg), (name, c)
    assert (seg[count:] == 0xEE).all(), name


def first_outcome(fn, clips, threshold):
    """what a loop of fn(labels, probs, threshold) over the clips ends with: ("ok", [metrics]) or the first error"""
    from tests.eval_cases import outcome

    out = []
    for probs, labels in clips:
        one = outcome(fn, labels, probs, threshold)
        if one[0] == "error":
            return one
        out.append(one[1])
    return ("ok", out)
