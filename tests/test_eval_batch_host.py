"""The batched device metrics (csrc/savad_eval_batch.h) on the CPU: the host twin savad_eval_batch_counts_host against
savad_eval_counts_host on every clip's slice (which tests/test_eval_counts_host.py holds to evaluate.file_metrics), metrics_from_counts
on the twin's counters against file_metrics on the slice, the refusals, the workspace arithmetic and the argument errors of
evaluate_vad_from_scratch(batch_files=...).  Every comparison is exact: integers, and float64 values with == and by their bits."""
import ctypes

import numpy as np
import pytest

from tests.eval_batch_cases import BAD, assert_batch_equals_clips, batches, clip_frames, concatenate, counts_host_batch, per_clip_counts
from tests.eval_cases import L, assert_same_metrics, outcome
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.evaluate import file_metrics
from voice_activity_detection_amd.metrics import EVAL_BAD_LABEL, EVAL_COUNTERS, EVAL_N, EVAL_NAN, metrics_from_counts

INVALID, UNSUPPORTED = -1, -2
NAMES = list(batches())


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_the_single_clip_twin_on_every_slice(name):
    clips, threshold = batches()[name]
    got = counts_host_batch(clips, threshold)
    assert_batch_equals_clips(name, got, per_clip_counts(clips, threshold))
    probs_all, clip_first, labels_all, label_first = concatenate(clips)
    assert got[1][:, EVAL_N].tolist() == clip_frames(clip_first, label_first).tolist()


@pytest.mark.parametrize("name", NAMES)
def test_metrics_from_the_twins_counters_equal_file_metrics(name):
    clips, threshold = batches()[name]
    count, counters, seg, seg_first = counts_host_batch(clips, threshold)
    for c, (probs, labels) in enumerate(clips):
        n = min(len(probs), len(labels))
        bad = bool(counters[c, EVAL_NAN] or counters[c, EVAL_BAD_LABEL])
        assert bad == (c in BAD.get(name, ())), (name, c)
        if n == 0 or bad:   # (these go to file_metrics in the Python layer)
            assert n > 0 or (counters[c] == 0).all()
            continue
        got = outcome(metrics_from_counts, counters[c], seg[seg_first[c]:seg_first[c + 1]], n)
        assert_same_metrics(got, outcome(file_metrics, labels, probs, threshold), (name, c))


def test_single_class_clips_raise_what_file_metrics_raises():
    clips, threshold = batches()["single-class clips"]
    count, counters, seg, seg_first = counts_host_batch(clips, threshold)
    for c in (1, 3):
        got = outcome(metrics_from_counts, counters[c], seg[seg_first[c]:seg_first[c + 1]], len(clips[c][1]))
        assert got == ("error", "ValueError", "AUC needs both classes") == outcome(file_metrics, clips[c][1], clips[c][0], threshold)


def test_other_half_widths():
    clips, threshold = batches()["segments at the ends"]
    for half_width in (1, 9, 254):
        assert_batch_equals_clips(half_width, counts_host_batch(clips, threshold, half_width), per_clip_counts(clips, threshold, half_width))


def _call_host(probs_all, clip_first, labels_all, label_first, C, W, half_width=L, counters=True, seg_cap=64):
    out = np.full((max(C, 1), EVAL_COUNTERS), -7, dtype=np.int64)
    seg = np.full((64, 8), 0xEE, dtype=np.uint8)
    seg_first = np.full(max(C, 1) + 1, -7, dtype=np.int64)
    rc = _lib.load().savad_eval_batch_counts_host(probs_all, clip_first, labels_all, label_first, C, W, 0.5, half_width, out if counters else None, seg,
                                                  seg_cap, seg_first)
    return rc, out, seg, seg_first


def test_refusals_write_nothing():
    lib = _lib.load()
    clips, _ = batches()["segments at the ends"]
    probs_all, clip_first, labels_all, label_first = concatenate(clips)
    C, W = len(clips), probs_all.shape[1]
    i32 = lambda *v: np.array(v, dtype=np.int32)
    late = clip_first.copy()
    late[0] = 1
    down = label_first.copy()
    down[2] = down[1] - 1
    refused = {
        "C = 0": dict(C=0), "C = -1": dict(C=-1), "table from 1": dict(clip_first=late), "decreasing": dict(label_first=down),
        "negative": dict(clip_first=i32(0, -5, 0, 0, 0, 0, 0)), "W = 0": dict(W=0), "W = 129": dict(W=129), "L = 0": dict(half_width=0),
        "L = 255": dict(half_width=255), "null table": dict(label_first=None), "null probs": dict(probs_all=None), "null labels": dict(labels_all=None),
        "null counters": dict(counters=False),
    }
    for what, change in refused.items():
        args = dict(probs_all=probs_all, clip_first=clip_first, labels_all=labels_all, label_first=label_first, C=C, W=W)
        args.update(change)
        rc, out, seg, seg_first = _call_host(**args)
        assert rc in ((UNSUPPORTED,) if what == "W = 129" else (INVALID,)), (what, rc)
        assert (out == -7).all() and (seg == 0xEE).all() and (seg_first == -7).all(), what
        if "null" not in what and "L =" not in what:
            tables = (args["clip_first"], args["label_first"], args["C"], args["W"])
            assert lib.savad_eval_batch_supported(*tables) == 0, what
            assert lib.savad_eval_batch_workspace_bytes(*tables, ctypes.byref(ctypes.c_size_t())) < 0, what
    assert lib.savad_eval_batch_supported(clip_first, label_first, C, W) == 1 and lib.savad_eval_batch_supported(clip_first, label_first, C, 128) == 1
    assert lib.savad_eval_batch_workspace_bytes(clip_first, label_first, C, W, None) == INVALID
    # an int32 table names fewer than 2^31 frames: the largest one is still a legal table (host arithmetic only)
    huge = i32(0, 2 ** 31 - 1)
    assert lib.savad_eval_batch_supported(huge, huge, 1, 7) == 1
    # room for fewer records than true segments is an error once the counters are known, not a truncation
    want = per_clip_counts(clips, 0.5)
    total = sum(len(s) for _, s in want)
    rc, out, seg, seg_first = _call_host(probs_all, clip_first, labels_all, label_first, C, W, seg_cap=total - 1)
    assert rc == INVALID and b"room for" in lib.savad_last_error()
    assert [out[c].tolist() for c in range(C)] == [w[0].tolist() for w in want] and (seg[total - 1:] == 0xEE).all()
    rc, out, seg, seg_first = _call_host(probs_all, clip_first, labels_all, label_first, C, W, seg_cap=total)
    assert rc == total


def workspace_bytes(clip_first, label_first, W=7):
    need = ctypes.c_size_t()
    _lib.check(_lib.load().savad_eval_batch_workspace_bytes(clip_first, label_first, len(clip_first) - 1, W, ctypes.byref(need)))
    return need.value


def test_workspace_is_monotone_in_the_table_and_independent_of_the_block():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 400, size=40)
    labels = rows + rng.integers(-3, 4, size=40).clip(-rows)
    first = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    base = workspace_bytes(first(rows), first(labels))
    assert base > 0
    for c in range(0, 40, 3):   # a longer clip never needs less
        more_rows, more_labels = rows.copy(), labels.copy()
        more_rows[c] += 70
        more_labels[c] += 70
        assert workspace_bytes(first(more_rows), first(more_labels)) >= base
    assert workspace_bytes(first(np.append(rows, 1)), first(np.append(labels, 1))) >= base   # nor does one more clip
    assert workspace_bytes(first(rows), first(np.zeros(40, dtype=np.int64))) <= base          # and no label means no frame
    try:   # the knob never outgrows a workspace: the same bytes at every block
        for block in (64, 256, 2048):
            _lib.check(lib.savad_eval_set_block(block))
            assert workspace_bytes(first(rows), first(labels)) == base
    finally:
        _lib.check(lib.savad_eval_set_block(0))
    # the digit table has room for every clip's blocks of 64: 256 entries of 4 bytes per block
    assert workspace_bytes(first([1] * 10), first([1] * 10)) >= 10 * 256 * 4


def test_files_metrics_device_without_a_device_tensor_is_file_metrics():
    from voice_activity_detection_amd.evaluate import files_metrics_device

    clips, threshold = batches()["ragged W7 rotation 1"]
    clips = [clip for clip in clips if min(len(clip[0]), len(clip[1])) > 1]
    probs_all, clip_first, _, _ = concatenate(clips)
    got = files_metrics_device([y for _, y in clips], probs_all, clip_first, threshold)
    assert len(got) == len(clips)
    for c, (probs, labels) in enumerate(clips):
        assert_same_metrics(("ok", got[c]), outcome(file_metrics, labels, probs, threshold), c)
    with pytest.raises(ValueError, match="label vectors"):
        files_metrics_device([y for _, y in clips][1:], probs_all, clip_first, threshold)


def test_batch_files_argument_errors(tmp_path):
    from voice_activity_detection_amd.evaluate import evaluate_vad_from_scratch

    (tmp_path / "list.jsonl").write_text("")
    with pytest.raises(ValueError, match="device_metrics"):
        evaluate_vad_from_scratch(tmp_path / "list.jsonl", tmp_path / "none.checkpoint", batch_files=2)
    with pytest.raises(ValueError, match="probabilities_fn"):
        evaluate_vad_from_scratch(tmp_path / "list.jsonl", device_metrics=True, batch_files=2, probabilities_fn=lambda path: np.zeros((1, 7), np.float32))
    with pytest.raises(ValueError, match="negative"):
        evaluate_vad_from_scratch(tmp_path / "list.jsonl", tmp_path / "none.checkpoint", device_metrics=True, batch_files=-1)


def test_cli_takes_batch_files():
    from voice_activity_detection_amd.__main__ import main

    with pytest.raises(ValueError, match="device_metrics"):   # (the flag reaches evaluate_vad_from_scratch, which refuses it alone)
        main(["evaluate", "list.jsonl", "none.checkpoint", "--batch-files", "2"])
