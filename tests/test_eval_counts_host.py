"""The arithmetic of the device metrics (csrc/savad_eval_device.h) on the CPU: the host twin savad_eval_counts_host runs the inline
functions the kernels run (std::stable_sort in place of the radix passes), and metrics.metrics_from_counts turns its integers into
the 18 values of evaluate.file_metrics -- the numpy path that tests/test_metrics.py pins to the reference's goldens.  Every
comparison is exact: integers, and float64 values with == and by their bits."""
import numpy as np
import pytest

from tests.eval_cases import L, assert_same_metrics, counts_host, edge_cases, grid_cases, outcome
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.evaluate import file_metrics, file_metrics_device
from voice_activity_detection_amd.metrics import (EVAL_BAD_LABEL, EVAL_N, EVAL_NAN, EVAL_POS, EVAL_PRED, EVAL_PRED_STRIDE, EVAL_TRUE, EVAL_U2,
                                                  detect_boundaries, equal_error_rate, metrics_from_counts, roc_auc)

INVALID, UNSUPPORTED = -1, -2
GRID = grid_cases((1, 2, 6, 64, 1000))
EDGES = {f"{name} ({N})": case for N in (6, 64, 1000) for name, case in edge_cases(N).items()}
UNCOUNTABLE = ("a NaN score", "a label of 2")


def from_counts(probs, labels, threshold):
    counters, seg = counts_host(probs, labels, threshold)
    return metrics_from_counts(counters, seg, min(len(probs), len(labels)))


def check(name, probs, labels, threshold):
    want = outcome(file_metrics, labels, probs, threshold)
    assert_same_metrics(outcome(from_counts, probs, labels, threshold), want, name)
    return want


@pytest.mark.parametrize("name", list(GRID))
def test_grid_equals_file_metrics(name):
    want = check(name, *GRID[name])
    assert (want[0] == "ok") == (len(GRID[name][1]) > 1)   # (one frame holds one class: both paths raise the same error)


@pytest.mark.parametrize("name", [k for k in EDGES if not k.startswith(UNCOUNTABLE)])
def test_edge_cases_equal_file_metrics(name):
    probs, labels, threshold = EDGES[name]
    want = check(name, probs, labels, threshold)
    if name.startswith("labels all"):
        assert want == ("error", "ValueError", "AUC needs both classes")
    else:
        assert want[0] == "ok"
    if name.startswith("all scores equal"):
        assert want[1]["auc"] == 0.5
    if name.startswith("predictions all 0"):   # the zero guards: no predicted segment, no predicted positive, a zero in the harmonic mean
        assert want[1]["bp"] == 0 and want[1]["boosted_precision"] == 0.0 and want[1]["vacc"] == 0
    if name.startswith("predictions all 1"):
        assert want[1]["boosted_recall"] == 1.0


def test_counters_are_the_counts_numpy_gives():
    """the counter block against plain numpy, so that a wrong counter cannot hide behind a metric that ignores it"""
    probs, labels, threshold = edge_cases(1000)["ties k/16"]
    counters, seg = counts_host(probs, labels, threshold)
    y = labels.astype(bool)
    boosted = probs.mean(axis=1)
    assert counters[EVAL_N] == len(y) and counters[EVAL_POS] == y.sum() and counters[EVAL_NAN] == 0 and counters[EVAL_BAD_LABEL] == 0
    starts, ends, n_true = detect_boundaries(labels)
    assert counters[EVAL_TRUE] == n_true == len(seg)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    assert counters[EVAL_U2] == round(2 * roc_auc(labels, boosted) * n_pos * n_neg)
    for p, pred in enumerate((probs[:, 3] > threshold, boosted > threshold)):
        got = counters[EVAL_PRED + p * EVAL_PRED_STRIDE:EVAL_PRED + (p + 1) * EVAL_PRED_STRIDE].tolist()
        assert got == [(y & pred).sum(), (~y & pred).sum(), (y & ~pred).sum(), (~y & ~pred).sum(), detect_boundaries(pred)[2]]
        match = pred == y
        for k, (b, e) in enumerate(zip(starts, ends)):
            lo, hi = max(e - L, 0), min(b + L, len(y))
            assert seg[k, 4 * p:4 * p + 4].tolist() == [match[b:hi].sum(), hi - b, match[lo:e + 1].sum(), e - lo + 1]


@pytest.mark.parametrize("name", [k for k in EDGES if k.startswith(UNCOUNTABLE)])
def test_nan_scores_and_labels_outside_01_fall_back(name):
    """the counters say so, metrics_from_counts refuses them, and file_metrics_device answers with file_metrics' values"""
    probs, labels, threshold = EDGES[name]
    counters, seg = counts_host(probs, labels, threshold)
    assert (counters[EVAL_NAN] > 0) == name.startswith("a NaN") and (counters[EVAL_BAD_LABEL] > 0) == name.startswith("a label")
    with pytest.raises(ValueError, match="do not determine"):
        metrics_from_counts(counters, seg)
    assert_same_metrics(outcome(file_metrics_device, labels, probs, threshold), outcome(file_metrics, labels, probs, threshold), name)


def test_file_metrics_device_without_a_device_tensor_is_file_metrics():
    probs, labels, threshold = GRID["N1000-W7-t0.5"]
    assert_same_metrics(outcome(file_metrics_device, labels, probs, threshold), outcome(file_metrics, labels, probs, threshold), "numpy input")


def test_shared_bisection_keeps_equal_error_rate():
    """equal_error_rate now shares its bisection with the counts path: its values on a scored and on a 0/1 input are the ones of the
    goldens' restatement (a root of 1 - x - interp on the curve, to the last bit of 200 halvings)"""
    from voice_activity_detection_amd.metrics import roc_curve_points

    probs, labels, _ = GRID["N1000-W7-t0.5"]
    for scores in (probs.mean(axis=1), probs.mean(axis=1) > 0.5):
        fpr, tpr = roc_curve_points(labels, scores)
        lo, hi = 0.0, 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if 1.0 - mid - np.interp(mid, fpr, tpr) > 0:
                lo = mid
            else:
                hi = mid
        assert equal_error_rate(labels, scores) == 0.5 * (lo + hi)


def test_supported_and_refusals():
    lib = _lib.load()
    assert lib.savad_eval_supported(7, 1000, 1000) == 1 and lib.savad_eval_supported(128, 1, 5) == 1
    assert lib.savad_eval_supported(129, 1000, 1000) == 0 and lib.savad_eval_supported(0, 1000, 1000) == 0
    assert lib.savad_eval_supported(7, 0, 1000) == 0 and lib.savad_eval_supported(7, 1000, 0) == 0
    assert lib.savad_eval_supported(7, 2 ** 31, 2 ** 31 - 1) == 1 and lib.savad_eval_supported(7, 2 ** 31, 2 ** 31) == 0
    probs, labels, threshold = GRID["N64-W7-t0.5"]
    for half_width in (0, 255):
        with pytest.raises(_lib.SavadError, match="L ="):
            counts_host(probs, labels, threshold, half_width)
    with pytest.raises(_lib.SavadError, match="2\\^31"):
        counts_host(np.zeros((4, 129), np.float32), labels, threshold)
    # room for fewer boundary records than true segments is an error, not a truncation
    import ctypes

    probs, labels, threshold = edge_cases(64)["segments at both ends"]
    p32, l8 = np.ascontiguousarray(probs), labels.astype(np.uint8)
    counters, seg = np.zeros(16, np.int64), np.zeros((1, 8), np.uint8)
    assert detect_boundaries(labels)[2] > 1
    assert lib.savad_eval_counts_host(ctypes.c_void_p(p32.ctypes.data), len(p32), 3, ctypes.c_void_p(l8.ctypes.data), len(l8), 0.5, L,
                                      ctypes.c_void_p(counters.ctypes.data), ctypes.c_void_p(seg.ctypes.data), 1) == INVALID
    assert lib.savad_eval_set_block(48) == INVALID and lib.savad_eval_set_block(4096) == INVALID and lib.savad_eval_set_block(32) == INVALID
    assert lib.savad_eval_set_block(64) == 0 and lib.savad_eval_set_block(0) == 0


def test_other_boundary_half_widths():
    """L is an argument of the ABI: 1 and 9 against vad_accuracy's own L"""
    from voice_activity_detection_amd.metrics import vad_accuracy

    probs, labels, threshold = GRID["N1000-W7-t0.5"]
    pred = probs.mean(axis=1) > threshold
    for half_width in (1, 9):
        counters, seg = counts_host(probs, labels, threshold, half_width)
        _, _, sba, eba, _ = vad_accuracy(labels, pred, L=half_width)
        n_true = len(seg)
        total_s = total_e = 0.0
        for rec in seg.tolist():
            total_s += rec[4] / rec[5]
            total_e += rec[6] / rec[7]
        assert total_s / n_true == sba and total_e / n_true == eba
