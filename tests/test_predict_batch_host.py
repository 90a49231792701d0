"""Many clips in one call, the parts that need no GPU: the planner (csrc/savad_schedule.h: plan_predict_batch, through the stand-alone
tests/predict_batch_dump.cpp), the library's refusal of what is not a clip table (before anything is launched), and the Python
clip-table helpers (voice_activity_detection_amd/clips.py)."""
import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "predict_batch_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"

CLIPS = [1022, 39, 0, 38, 5, 2100, 40, 1]   # the GPU tests' clip set: 3049 windows at half = 19


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    exe = tmp_path_factory.mktemp("predict_batch") / "predict_batch_dump"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)

    def run(precision, row_mode, F, chunk, half, jump, *rest):
        out = subprocess.run([str(exe), *map(str, (precision, row_mode, F, chunk, half, jump)), *map(str, rest)], check=True,
                             capture_output=True, text=True, timeout=60)
        assert out.stderr == ""
        return out.stdout.strip()

    return run


def parse(line):
    head, _, tail = line.partition(" :")
    words = head.split()
    plan = {k: int(v) for k, v in zip(words[::2], words[1::2])}
    forwards = [tuple(int(v) for v in w.split(":")) for w in tail.split()]
    return plan, forwards


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("row_mode", [0, 1, 4])
@pytest.mark.parametrize("lengths,F,chunk,half,jump", [
    (CLIPS, 80, 16384, 19, 9), (CLIPS, 80, 1000, 19, 9), (CLIPS, 80, 8, 19, 9), (CLIPS, 80, 999, 19, 9), (CLIPS, 13, 1000, 5, 1),
    ([38, 0, 5], 80, 16384, 19, 9), ([39], 80, 16384, 19, 9), ([0], 80, 7, 19, 9), ([40, 40, 40], 80, 3, 19, 9), ([50000, 7, 50000], 40, 4095, 3, 2)])
def test_plan_covers_every_item_once_and_sizes_its_workspace(dump, precision, row_mode, lengths, F, chunk, half, jump):
    from voice_activity_detection_amd.clips import clip_table, window_items

    plan, forwards = parse(dump(precision, row_mode, F, chunk, half, jump, *lengths))
    W = 2 * ((half + jump - 1) // jump) + 1
    items = int(window_items(clip_table(lengths), half)[-1])
    assert (plan["W"], plan["C"], plan["rows"], plan["items"]) == (W, len(lengths), sum(lengths), items)
    # the chunk rule of plan_predict: even, at most the item count
    even = chunk + chunk % 2
    assert plan["chunk"] == (even if even <= items else max(items, 1))
    # every item exactly once, in order
    covered = 0
    for first, count, _ in forwards:
        assert first == covered and 1 <= count <= plan["chunk"]
        assert first * W * 8 % 16 == 0          # the forward's output pointer: 16-byte aligned inside logp
        covered += count
    assert covered == items and len(forwards) == -(-items // plan["chunk"])
    # consecutive 16-byte aligned buffers, each as large as its use
    assert plan["items_first"] == 0 and plan["logp"] >= 4 * (len(lengths) + 1)
    assert plan["windows"] - plan["logp"] >= items * W * 2 * 4
    assert plan["fwd"] - plan["windows"] >= plan["chunk"] * W * F * 4
    assert plan["total"] - plan["fwd"] >= plan["fwd_bytes"]
    assert all(plan[k] % 16 == 0 for k in ("logp", "windows", "fwd", "total"))
    for _, _, need in forwards:
        assert need <= plan["fwd_bytes"]        # every forward the call makes fits the forward workspace it was given


def test_plan_refuses_what_is_not_a_clip_table(dump):
    assert dump(0, 0, 80, 1000, 19, 9, "-").startswith("err -1 ")                       # no clip
    assert "clip_first[0]" in dump(0, 0, 80, 1000, 19, 9, "table", 1, 5)
    assert "decrease" in dump(0, 0, 80, 1000, 19, 9, "table", 0, 50, 49, 100)
    assert dump(0, 0, 80, 1000, 40, 1, 100).startswith("err -2 ") and "64 frames" in dump(0, 0, 80, 1000, 40, 1, 100)   # W = 81
    assert dump(0, 0, 80, 0, 19, 9, 100).startswith("err -1 ")
    assert dump(0, 0, 80, 1000, 19, 0, 100).startswith("err -1 ")
    # rows up to 2^31 - 1 fit the table; their windows x W do not fit a 32-bit index
    assert "32-bit" in dump(0, 0, 80, 1000, 19, 9, 2 ** 31 - 1) and dump(0, 0, 80, 1000, 19, 9, 2 ** 31 - 1).startswith("err -2 ")
    assert dump(0, 0, 80, 1000, 19, 9, 2 ** 30, 2 ** 30 - 1).startswith("err -2 ")
    plan, _ = parse(dump(0, 0, 80, 1 << 20, 19, 9, (2 ** 31 - 1) // 7 + 38))              # exactly at the limit: planned
    assert plan["items"] * 7 == (2 ** 31 - 1) // 7 * 7


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def test_library_refuses_bad_tables_without_a_launch(lib):
    """savad_gather_windows_batch / savad_boost_batch validate the HOST table first: with every device pointer NULL a refusal can only
    have come from that validation (on a machine without a GPU too)."""
    def table(*v):
        return np.array(v, dtype=np.int32)

    def gather(t, C, half=19, jump=9, F=80, first=0, count=0):
        return lib.savad_gather_windows_batch(None, ctypes.c_void_p(t.ctypes.data), None, C, F, half, jump, first, count, None, None, None,
                                              None)

    def boost(t, C, half=19, jump=9):
        return lib.savad_boost_batch(None, ctypes.c_void_p(t.ctypes.data), None, C, half, jump, None, None, None, None)

    for call in (gather, boost):
        assert call(table(0, 50, 49), 2) == -1 and b"decrease" in lib.savad_last_error()
        assert call(table(3, 50), 1) == -1 and b"clip_first[0]" in lib.savad_last_error()
        assert call(table(0, 50), 0) == -1 and b"at least one clip" in lib.savad_last_error()
        assert call(table(0, 50), -3) == -1
        assert call(table(0, 2 ** 31 - 1), 1) == -2 and b"32-bit" in lib.savad_last_error()
        assert call(table(0, 2000), 1, half=40, jump=1) == -2 and b"64 frames" in lib.savad_last_error()
        assert call(table(0, 2000), 1, jump=0) == -1
        assert call(table(0, 0, 0), 2) == 0     # nothing but empty clips: nothing to do
    assert lib.savad_gather_windows_batch(None, None, None, 1, 80, 19, 9, 0, 0, None, None, None, None) == -1
    assert gather(table(0, 100), 1, first=60, count=3) == -1 and b"outside" in lib.savad_last_error()   # 62 windows
    assert gather(table(0, 100), 1, first=-1, count=1) == -1
    assert gather(table(0, 100), 1, first=0, count=62) == -1 and b"null" in lib.savad_last_error()      # valid items, no buffers
    assert boost(table(0, 100), 1) == -1 and b"null" in lib.savad_last_error()
    size = ctypes.c_size_t()
    t = table(0, 100)
    assert lib.savad_predict_batch_workspace_bytes(None, ctypes.c_void_p(t.ctypes.data), 1, 19, 9, 1000, ctypes.byref(size)) == -1
    assert lib.savad_predict_probabilities_batch(None, None, ctypes.c_void_p(t.ctypes.data), None, 1, 19, 9, 1000, None, None, None, 0, None) == -1


def test_clip_table_helpers():
    from voice_activity_detection_amd.clips import check_clip_table, clip_table, split_by_clip, window_items

    t = clip_table(CLIPS)
    assert t.dtype == np.int32 and t.tolist() == [0, 1022, 1061, 1061, 1099, 1104, 3204, 3244, 3245]
    assert window_items(t, 19).tolist() == [0, 984, 985, 985, 985, 985, 3047, 3049, 3049]
    assert window_items(t, 5).tolist()[-1] == 1012 + 29 + 0 + 28 + 0 + 2090 + 30 + 0
    assert clip_table([0]).tolist() == [0, 0] and clip_table(iter([3, 4])).tolist() == [0, 3, 7]
    for bad in ([], [3, -1], [2 ** 31 - 1, 1]):
        with pytest.raises(ValueError):
            clip_table(bad)
    assert check_clip_table([0, 3, 3, 9]).dtype == np.int32 and check_clip_table(t) is not None
    for bad in ([0], [1, 2], [0, 5, 4], [0.0, 2.0], [[0, 1]], [0, 2 ** 31]):
        with pytest.raises(ValueError):
            check_clip_table(bad)
    rows = np.arange(3245 * 2).reshape(3245, 2)
    parts = split_by_clip(rows, t)
    assert [len(p) for p in parts] == CLIPS and all(np.shares_memory(p, rows) for p in parts if len(p))     # views, not copies
    assert np.array_equal(np.concatenate(parts), rows) and parts[5][0, 0] == 2 * 1104
    with pytest.raises(ValueError):
        split_by_clip(rows[:-1], t)


def test_split_by_clip_takes_tensors():
    import torch

    from voice_activity_detection_amd.clips import clip_table, split_by_clip

    x = torch.arange(12.0).reshape(6, 2)
    parts = split_by_clip(x, clip_table([2, 0, 4]))
    assert [tuple(p.shape) for p in parts] == [(2, 2), (0, 2), (4, 2)] and parts[2].data_ptr() == x[2:].data_ptr()


@pytest.mark.parametrize("n_samples,split", [(160000, None), (160000, 2), (159999, 2), (49120, 2), (49120, 0.7), (16000 * 3600 + 13, 10), (1, 2),
                                             (33333, 1.0)])
def test_chunk_bounds_are_the_reference_chunks(n_samples, split):
    """clips.chunk_bounds (what predict and predict_many both cut a recording by) against vad/predictor.py:86-93 written out"""
    import math

    from voice_activity_detection_amd.clips import chunk_bounds

    duration = n_samples / 16000
    num = math.ceil(duration / split) if split is not None else 1
    adjusted = duration / num
    want = [(int(i * adjusted * 16000), int((i + 1) * adjusted * 16000)) for i in range(num)]
    got_adjusted, got = chunk_bounds(n_samples, 16000, split)
    assert got_adjusted == adjusted and got == want
    assert got[0][0] == 0 and all(a[1] == b[0] for a, b in zip(got, got[1:])) and abs(got[-1][1] - n_samples) <= 1
