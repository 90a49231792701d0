"""The log-mel front-end over a clip table, the parts that need no GPU: the host plan (csrc/savad_logmel_batch_plan.h, through the
stand-alone tests/logmel_batch_dump.cpp built with the address and undefined-behaviour sanitizers), every refusal through the dump
and through the library (which refuses before anything is launched), the Python table helper (clips.audio_clip_table), and the
pad rule the single-clip path and the batch kernels share (mel::pad_rule / mel::pad_source) against numpy's reflect padding, which
is what oracle/logmel.py pads with."""
import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "logmel_batch_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"

EDGE_LENGTHS = [1, 159, 160, 208, 255, 256, 257, 415, 416, 4959, 4960, 5119, 5120, 0, 16000, 52001]   # the GPU test's clips
HEAD_SLOT, TAIL_SLOT = 208, 212   # floats


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    exe = tmp_path_factory.mktemp("logmel_batch") / "logmel_batch_dump"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True, timeout=60)
        assert out.stderr == ""
        return out.stdout.strip()

    return run


def plan_of(dump, table, audio_count):
    line = dump("plan", audio_count, *[f"{int(a)}:{int(b)}" for a, b in table] or ["-"])
    if line.startswith("err"):
        return line
    head, first, tiles = line.split(" :")
    words = head.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}, [int(v) for v in first.split()], [int(v) for v in tiles.split()]


def expected(table):
    """the counts and the layout in a few lines of numpy"""
    counts = np.asarray(table, dtype=np.int64).reshape(-1, 2)[:, 1]
    frames = np.where(counts > 0, 1 + counts // 160, 0)
    tiles = (frames + 31) // 32
    C = len(counts)
    o_head = (4 * (C + 1) + 15) // 16 * 16
    o_tail = o_head + 4 * HEAD_SLOT * C
    return ([0] + np.cumsum(frames).tolist(), [0] + np.cumsum(tiles).tolist(),
            {"tiles_first": 0, "head": o_head, "tail": o_tail, "total": o_tail + 4 * TAIL_SLOT * C})


def check_plan(dump, table, audio_count):
    plan, clip_first, tiles_first = plan_of(dump, table, audio_count)
    want_first, want_tiles, layout = expected(table)
    assert clip_first == want_first and tiles_first == want_tiles
    assert (plan["C"], plan["rows"], plan["tiles"]) == (len(table), want_first[-1], want_tiles[-1])
    assert {k: plan[k] for k in layout} == layout
    assert (plan["head_slot"], plan["tail_slot"]) == (HEAD_SLOT, TAIL_SLOT)
    assert all(plan[k] % 16 == 0 for k in layout) and HEAD_SLOT % 4 == 0 and TAIL_SLOT % 4 == 0   # every piece, every slot: 16 bytes


def test_plan_of_the_edge_lengths(dump):
    from voice_activity_detection_amd.clips import audio_clip_table

    table, audio_count = audio_clip_table(EDGE_LENGTHS)
    check_plan(dump, table, audio_count)
    plan, clip_first, tiles_first = plan_of(dump, table, audio_count)
    # 1 / 159: one frame; 160: two; 4959 / 4960 / 5119 / 5120: 31 / 32 / 32 / 33 frames = 1 / 1 / 1 / 2 tiles; the empty clip: nothing
    assert np.diff(clip_first).tolist() == [1, 1, 2, 2, 2, 2, 2, 3, 3, 31, 32, 32, 33, 0, 101, 326]
    assert np.diff(tiles_first).tolist() == [1] * 12 + [2, 0, 4, 11]


def test_plan_of_random_tables(dump):
    rng = np.random.default_rng(20)
    for _ in range(12):
        C = int(rng.integers(1, 40))
        counts = rng.choice([0, 1, 159, 160, 161, 5119, 5120, 5121, 40000], size=C) + rng.integers(0, 3, size=C) * (rng.random(C) < 0.3)
        audio_count = int(counts.max() + 4 * rng.integers(0, 50) + 64)
        firsts = np.array([4 * rng.integers(0, (audio_count - c) // 4 + 1) for c in counts])   # anywhere, overlapping or not
        check_plan(dump, np.stack([firsts, counts], axis=1), audio_count)


REFUSALS = [   # (table, audio_count, code, word of the message)
    ([], 100, -1, "at least one clip"),
    ([(0, -1)], 100, -1, "count -1"),
    ([(-4, 8)], 100, -1, "first -4"),
    ([(0, 50), (96, 5)], 100, -1, "first 96 + count 5 reaches past"),
    ([(104, 0)], 100, -1, "reaches past"),
    ([(2 ** 63 - 4, 2 ** 63 - 1)], 2 ** 63 - 1, -1, "reaches past"),   # (the refusal adds nothing up: first + count would overflow)
    ([(8, 2 ** 63 - 1)], 100, -1, "reaches past"),
    ([(0, 50)], -1, -1, "audio_count"),
    ([(0, 50), (6, 10)], 100, -1, "multiple of 4"),
    ([(0, 2_000_000_001)], 2_000_000_001, -2, "2000000000"),
    ([(0, 2_000_000_000)] * 172, 2_000_000_000, -2, "2^31 - 1"),   # 172 x 12 500 001 rows
]


@pytest.mark.parametrize("table,audio_count,code,word", REFUSALS)
def test_plan_refuses(dump, table, audio_count, code, word):
    line = plan_of(dump, table, audio_count)
    assert isinstance(line, str) and line.startswith(f"err {code} ") and word in line, line


def test_plan_takes_what_is_legal(dump):
    check_plan(dump, [(0, 100), (0, 100), (48, 52)], 100)         # overlapping and repeated clips: they are only read
    check_plan(dump, [(100, 0), (0, 0)], 100)                     # empty clips, one at the very end
    check_plan(dump, [(0, 0)], 0)                                 # no audio at all
    check_plan(dump, [(0, 2_000_000_000)] * 171, 2_000_000_000)   # 2 137 500 171 rows: below 2^31 - 1


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


@pytest.mark.parametrize("table,audio_count,code,word", REFUSALS)
def test_library_refuses_bad_tables_without_a_launch(lib, table, audio_count, code, word):
    """savad_logmel_batch and its two host queries validate the HOST table first: with every device pointer NULL a refusal can only
    have come from that validation (on a machine without a GPU too)."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 2))
    host = ctypes.c_void_p(t.ctypes.data) if len(t) else None
    rows, tiles, size = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    calls = [lambda: lib.savad_logmel_batch_shape(host, len(t), audio_count, ctypes.byref(rows), ctypes.byref(tiles)),
             lambda: lib.savad_logmel_batch_workspace_bytes(host, len(t), audio_count, ctypes.byref(size)),
             lambda: lib.savad_logmel_batch(None, audio_count, host, None, len(t), None, None, None, None)]
    for call in calls:
        assert call() == code and word.encode() in lib.savad_last_error(), lib.savad_last_error()


def test_library_host_queries_and_the_refusals_behind_the_table(lib):
    from voice_activity_detection_amd.clips import audio_clip_table

    table, audio_count = audio_clip_table(EDGE_LENGTHS)
    want_first, want_tiles, layout = expected(table)
    rows, tiles, size = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    assert lib.savad_logmel_batch_shape(table, len(table), audio_count, ctypes.byref(rows), ctypes.byref(tiles)) == 0
    assert (rows.value, tiles.value) == (want_first[-1], want_tiles[-1])
    assert lib.savad_logmel_batch_shape(table, len(table), audio_count, None, None) == 0
    assert lib.savad_logmel_batch_workspace_bytes(table, len(table), audio_count, ctypes.byref(size)) == 0 and size.value == layout["total"]
    assert lib.savad_logmel_batch_workspace_bytes(table, len(table), audio_count, None) == -1
    assert lib.savad_logmel_batch_shape(table, 0, audio_count, None, None) == -1 and lib.savad_logmel_batch_shape(table, -2, audio_count, None, None) == -1
    # a good table, no buffers: refused for the null pointers, still before any launch
    assert lib.savad_logmel_batch(None, audio_count, table, None, len(table), None, None, None, None) == -1 and b"null" in lib.savad_last_error()
    # the one-GEMM DFT has no batch form
    assert lib.savad_logmel_set_algorithm(1) == 0
    try:
        assert lib.savad_logmel_batch(None, audio_count, table, None, len(table), None, None, None, None) == -2
        assert b"no batch form" in lib.savad_last_error()
    finally:
        assert lib.savad_logmel_set_algorithm(0) == 0


def test_audio_clip_table():
    from voice_activity_detection_amd.clips import audio_clip_table

    table, audio_count = audio_clip_table([5, 0, 8, 3])
    assert table.dtype == np.int64 and table.tolist() == [[0, 5], [8, 0], [8, 8], [16, 3]] and audio_count == 19
    table, audio_count = audio_clip_table(iter([5, 1]), align=8)
    assert table.tolist() == [[0, 5], [8, 1]] and audio_count == 9
    table, audio_count = audio_clip_table(EDGE_LENGTHS)
    assert (table[:, 0] % 4 == 0).all() and table[:, 1].tolist() == EDGE_LENGTHS
    assert (table[1:, 0] >= table[:-1].sum(axis=1)).all() and (table[1:, 0] - table[:-1].sum(axis=1) < 4).all()   # in order, gaps below 4
    assert audio_count == int(table[-1].sum())
    table, audio_count = audio_clip_table([0])
    assert table.tolist() == [[0, 0]] and audio_count == 0
    for bad in ([], [3, -1]):
        with pytest.raises(ValueError):
            audio_clip_table(bad)
    for align in (0, 2, 6, -4):
        with pytest.raises(ValueError):
            audio_clip_table([3], align=align)


def rule_lines(dump, lo, hi):
    for line in dump("rule", lo, hi).splitlines():
        head, a, b = line.split(" :")
        n, a_j0, a_count, a_end, b_j0, b_count, j_first, j_last = (int(v) for v in head.split())
        yield n, a_j0, a_count, a_end, b_j0, b_count, j_first, j_last, [int(v) for v in a.split()], [int(v) for v in b.split()]


def test_pad_rule_geometry(dump):
    """what the rule says about the padded indices, for every n: the frames' chunks are [48, j_last + 4); A is [48, 256), B starts at
    the first 16-byte chunk that holds a padded index past the last sample and ends with the last chunk; everything between is audio"""
    for n, a_j0, a_count, a_end, b_j0, b_count, j_first, j_last, a, b in rule_lines(dump, 1, 700):
        frames = 1 + n // 160
        assert (j_first, j_last) == (48, 160 * (frames - 1) + 460)
        assert (a_j0, a_count, a_end) == (48, 208, 256) and len(a) == 208
        assert b_j0 % 4 == 0 and b_j0 - 256 <= n < b_j0 - 256 + 4 and b_j0 + b_count == j_last + 4 and 0 < b_count <= TAIL_SLOT and len(b) == b_count
        assert a_count <= HEAD_SLOT
        assert all(0 <= i < n for i in a + b)               # a source is always a sample of the signal


def test_pad_rule_against_the_oracles_reflect_indices(dump):
    """mel::pad_rule -- which padded indices the frames read from stretch A, from stretch B and straight from the audio -- against
    numpy.pad(arange(n), 256, mode="reflect"), the padding of oracle/logmel.py, for n = 1 .. 700: every index of [48, j_last + 4) lies in
    exactly one of the three, an index read from the audio is its own sample j - 256 in the oracle's padding too (no reflection there), and
    the two stretches are no longer than they must be: A ends where the reflection ends, B starts with the first 16-byte chunk that holds
    an index past the last sample."""
    from oracle import logmel

    half = logmel.N_FFT // 2
    for n, a_j0, a_count, a_end, b_j0, b_count, j_first, j_last, _, _ in rule_lines(dump, 1, 700):
        want = np.pad(np.arange(n), half, mode="reflect")
        j = np.arange(j_first, j_last + 4)
        in_a, in_b = (j >= a_j0) & (j < a_end), j >= b_j0
        assert a_end == a_j0 + a_count and j_last + 4 == b_j0 + b_count and not (in_a & in_b).any(), n
        direct = j[~in_a & ~in_b]
        assert direct.size == 0 or (direct[0] == a_end and direct[-1] == b_j0 - 1), n
        assert ((direct - half >= 0) & (direct - half < n)).all() and np.array_equal(want[direct], direct - half), n
        assert want[a_end] == 0 and (j[in_a] - half < 0).all(), n            # A: exactly the indices in front of sample 0
        assert (np.arange(b_j0, b_j0 + 4) - half >= n).any(), n              # B: its first chunk already leaves the signal


def clamped(j, n):
    """reflect_pad_segments_kernel's index rule, restated: one reflection at each end, then the clamps"""
    i = j - 256
    i = -i if i < 0 else i
    i = 2 * (n - 1) - i if i >= n else i
    return min(max(i, 0), n - 1)


def test_pad_source_is_the_single_clip_index_rule(dump):
    """mel::pad_source over both stretches, n = 1 .. 700: the rule of reflect_pad_segments_kernel (the batch must give savad_logmel's bits, so
    it keeps that rule, clamps included), and numpy's reflect padding wherever one reflection at each end stays inside the signal -- the
    head reflects up to sample 208 and the tail up to 208 samples back, so from n = 209 on.  (Measured: the two also agree for n = 1,
    105 .. 159 and 185 .. 208; for n = 2 .. 104 and 160 .. 184 the clamps take sample 0 or n - 1 where numpy goes on reflecting, in
    savad_logmel as here.)"""
    for n, a_j0, a_count, _, b_j0, b_count, _, _, a, b in rule_lines(dump, 1, 700):
        assert a == [clamped(a_j0 + k, n) for k in range(a_count)] and b == [clamped(b_j0 + k, n) for k in range(b_count)], n
        if n >= 209:
            want = np.pad(np.arange(n), 256, mode="reflect")
            assert a == want[a_j0:a_j0 + a_count].tolist() and b == want[b_j0:b_j0 + b_count].tolist(), n
