"""Every window geometry a checkpoint can name, the parts that need no GPU (tests/window_geometry_cases.py has the geometries):
the CPU oracle against the reference's own predictor (tests/golden/golden_geometry.npz), a loop-by-loop numpy restatement of the
reference's gather and boost against the oracle, the precondition of the GPU tests (an address that is one frame off is far outside
their tolerance), the window count everywhere it is computed, and the geometries that are refused."""
import copy
import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle
from tests import window_geometry_cases as cases
from tests.window_geometry_cases import DISAGREEING, GEOMETRIES, geometry_id

REPO = Path(__file__).resolve().parents[1]
GOLDEN_TOL = 1e-6        # the float64-accumulating oracle against the reference (measured 3.0e-7 at worst: a 3x margin)
BOOST_TOL = 2e-7         # one float32 softmax against another
TIGHT = 3e-5             # the GPU tests' bound on fp32 / fp32s probabilities (tests/test_gpu_window_geometry.py)
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def goldens():
    with np.load(REPO / "tests" / "golden" / "golden_geometry.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def test_golden_file_holds_the_geometry_table(goldens):
    assert [tuple(g) for g in goldens["geometries"]] == GEOMETRIES
    for (half, jump), row in zip(GEOMETRIES, goldens["half_jump_W_N_seed"]):
        W, N = len(cases.offsets(half, jump)), cases.golden_length(half, jump)
        assert tuple(row) == (half, jump, W, N, 7000 + 100 * half + jump)
        assert W == cases.reference_formula(half, jump)          # the reference can run every one of them
        probs = goldens[cases.golden_key(half, jump)]
        assert probs.shape == (N, W) and probs.dtype == np.float32
    assert [len(cases.offsets(h, j)) for h, j in GEOMETRIES] == [1, 3, 3, 5, 7, 11, 17, 31, 33, 63]
    assert list(cases.offsets(20, 9)) == [-20, -11, -2, 0, 1, 10, 19] and list(cases.offsets(3, 5)) == [-3, 0, 1]
    assert 23 == min(cases.golden_length(h, j) for h, j in GEOMETRIES) and 163 == max(cases.golden_length(h, j) for h, j in GEOMETRIES)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_oracle_against_the_reference(goldens, state1234, geometry):
    half, jump = geometry
    want = goldens[cases.golden_key(half, jump)]
    N = want.shape[0]
    probs, mean = oracle.predict_probabilities(state1234, cases.features(half, jump, N), half, jump, acc64=True)
    err = float(np.abs(probs.astype(np.float64) - want).max())
    print(f"oracle vs reference at {half} / {jump}: max |dp| = {err:.2e}")
    assert probs.shape == want.shape and err <= GOLDEN_TOL
    assert np.array_equal(probs == 0.5, want == 0.5)
    assert float(np.abs(mean - want.mean(axis=1)).max()) <= GOLDEN_TOL


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_numpy_restatement_against_the_oracle(state1234, geometry):
    half, jump = geometry
    assert np.array_equal(oracle.window_offsets(half, jump), cases.offsets(half, jump))
    for N in cases.lengths(half, jump):
        feat = cases.features(half, jump, N)
        windows, positions = cases.gather(feat, half, jump)
        n = max(N - 2 * half, 0)
        assert windows.shape == (n, len(cases.offsets(half, jump)), 80)
        if n == 0:
            probs, _ = oracle.predict_probabilities(state1234, feat, half, jump)
            assert probs.shape == (N, windows.shape[1]) and (probs == 0.5).all()
            continue
        win, pos = oracle.gather_windows(feat, half, jump, 0, n)
        assert np.array_equal(win.view(np.uint32), windows.view(np.uint32)) and np.array_equal(pos, positions)
        logp = oracle.forward(state1234, windows)
        want, want_mean = oracle.boost(logp, positions, N)
        probs, mean = cases.boost(logp, positions, N)
        assert np.array_equal(probs == 0.5, want == 0.5)
        assert float(np.abs(probs - want).max()) <= BOOST_TOL and float(np.abs(mean - want_mean).max()) <= BOOST_TOL


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_an_offset_one_frame_off_is_far_outside_the_gpu_bound(state1234, geometry):
    """What lets a GPU comparison at TIGHT catch a wrong address: for every window slot w, reading the frame next to the right one
    moves some probability of column w by more than 100 x TIGHT."""
    half, jump = geometry
    N = cases.golden_length(half, jump)
    feat = cases.features(half, jump, N)
    windows, positions = cases.gather(feat, half, jump)
    base, _ = oracle.boost(oracle.forward(state1234, windows, acc64=True), positions, N)
    worst = np.inf
    for w in range(windows.shape[1]):
        moved, same_positions = cases.gather(feat, half, jump, moved=(w, 1))
        assert np.array_equal(same_positions, positions) and not np.array_equal(moved[:, w], windows[:, w])
        assert np.array_equal(np.delete(moved, w, axis=1), np.delete(windows, w, axis=1))      # ONE offset moved
        probs, _ = oracle.boost(oracle.forward(state1234, moved, acc64=True), positions, N)
        change = float(np.abs(probs[:, w] - base[:, w]).max())
        worst = min(worst, change)
        assert change > 100 * TIGHT, (half, jump, w, change)
    print(f"{half} / {jump}: the least change of a column whose offset moved by one frame = {worst:.2e}")


# ---- the window count ---------------------------------------------------------------------------------------------------------------

def _live_W(lib, half, jump):
    """W as the live plan reports it for one push (host arithmetic: the addresses are never followed), or the refusal's code"""
    from voice_activity_detection_amd import _lib

    cfg = _lib.savad_live_config(1, 1600, half, jump, 1024)
    nbytes = ctypes.c_size_t()
    rc = lib.savad_live_table_bytes(ctypes.byref(cfg), 1, ctypes.byref(nbytes))
    if rc:
        return rc
    slots = (_lib.savad_live_slot * 1)()
    assert lib.savad_live_open(ctypes.byref(cfg), slots, 0) == 0
    table = ctypes.create_string_buffer(nbytes.value)
    counts = _lib.savad_live_counts()
    push = (_lib.savad_live_push * 1)(_lib.savad_live_push(0, 1600, 1, 0, 1 << 30))
    assert lib.savad_live_plan(ctypes.byref(cfg), slots, push, 1, ctypes.c_void_p(1 << 20), table, len(table), ctypes.byref(counts), None) == 0
    return counts.W


def _dump(tmp_path, name, *args):
    """stdout of tests/<name>.cpp, compiled with the host compiler against the library's headers"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    exe = tmp_path / name
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{REPO / 'voice_activity_detection_amd' / 'csrc'}",
                    str(REPO / "tests" / f"{name}.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe), *args], check=True, capture_output=True, text=True, timeout=60).stdout


def test_the_geometry_header_is_the_rule(tmp_path):
    """csrc/savad_windows.h alone (tests/windows_dump.cpp): the one copy of the offsets rule against numpy for half 0 .. 40 and jump
    1 .. 12, the refusal of a window longer than 64 frames (a caller's int32_t[64] is never overrun), and the item, chunk and
    workspace rules against their one-line definitions."""
    lines = _dump(tmp_path, "windows_dump", "offsets", "40", "12").splitlines()
    assert len(lines) == 41 * 12
    seen_refusal = False
    for line in lines:
        head, _, tail = line.partition(" :")
        _, half, jump, W, message = head.split(" ", 4)
        half, jump, W = int(half), int(jump), int(W)
        want = np.concatenate([np.arange(-half, 0, jump), [0], np.arange(1, half + 1, jump)])
        assert np.array_equal(want, cases.offsets(half, jump))
        assert W == len(want), (half, jump)
        assert message == ("'window longer than 64 frames'" if W > 64 else "''"), (half, jump)
        assert [int(v) for v in tail.split()] == list(want[:64]), (half, jump)
        seen_refusal |= W > 64
    assert seen_refusal and len(cases.offsets(32, 1)) == 65      # the boundary itself is among them
    n = {"i": 0, "c": 0, "l": 0}
    up = lambda b: (b + 255) // 256 * 256
    for line in _dump(tmp_path, "windows_dump", "rules").splitlines():
        kind, *v = line.replace(":", " ").split()
        v = [int(x) for x in v]
        n[kind] += 1
        if kind == "i":
            rows, half, items = v
            assert items == max(0, rows - 2 * half), line
        elif kind == "c":
            chunk, n_items, even, at_most = v
            assert at_most == max(1, min(chunk, n_items)), line
            assert even == max(1, min(chunk + chunk % 2, n_items)), line      # even, at most n_items, at least 1
        else:
            table, logp_items, chunk, W, F, fwd, o_table, o_logp, o_win, o_fwd, total = v
            assert o_table == 0 and o_logp == up(4 * table) and o_win == o_logp + up(4 * logp_items * W * 2), line
            assert o_fwd == o_win + up(4 * chunk * W * F) and total == o_fwd + up(fwd), line
    assert n == {"i": 40, "c": 99, "l": 5}


def test_window_count_is_the_number_of_offsets_everywhere(lib, tmp_path):
    out = _dump(tmp_path, "schedule_dump", "windows", "40", "12")
    planned = {(int(h), int(j)): int(w) for h, j, w in (line.split() for line in out.splitlines())}
    assert len(planned) == 41 * 12
    disagree = []
    for half in range(41):
        for jump in range(1, 13):
            want = cases.offsets(half, jump)
            W = len(want)
            assert lib.savad_window_offsets(half, jump, None) == W == planned[half, jump], (half, jump)
            buf = (ctypes.c_int32 * W)()
            assert lib.savad_window_offsets(half, jump, buf) == W and list(buf) == list(want), (half, jump)
            live = _live_W(lib, half, jump)
            assert live == (W if W <= 64 else E_UNSUPPORTED), (half, jump, live)
            assert (W != cases.reference_formula(half, jump)) == (2 * ((half - 1) % jump) >= jump)
            if W != cases.reference_formula(half, jump):
                disagree.append((half, jump))
    assert set(DISAGREEING) <= set(disagree) and not set(GEOMETRIES) & set(disagree)
    assert lib.savad_window_offsets(-1, 1, None) == E_INVALID and lib.savad_window_offsets(3, 0, None) == E_INVALID


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _model():
    from voice_activity_detection_amd import SelfAttentiveVAD

    return SelfAttentiveVAD(80, 3, 128, 0.5)


def test_a_window_of_65_frames_is_refused_by_the_library(lib):
    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.predictor import ContextResolution, VADFromScratchPredictor, window_offsets

    assert len(cases.offsets(32, 1)) == 65 and len(cases.offsets(31, 1)) == 63
    table = np.array([0, 200], dtype=np.int32)
    for half, code in ((31, 0), (32, E_UNSUPPORTED)):
        # a clip table that is fine, no windows asked for and no buffers: the geometry is checked first, nothing is launched
        assert lib.savad_gather_windows_batch(None, ctypes.c_void_p(table.ctypes.data), None, 1, 80, half, 1, 0, 0, None, None, None, None) == code
        if code:
            assert b"64 frames" in lib.savad_last_error()
        cfg = _lib.savad_live_config(2, 1600, half, 1, 1024)
        nbytes = ctypes.c_size_t()
        assert lib.savad_live_state_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == code
        if code:
            assert b"64 frames" in lib.savad_last_error()
    # the formula and the offsets agree at 32 / 1: the Python layer leaves the refusal to the library
    assert VADFromScratchPredictor(_model(), "cpu", ContextResolution(32, 1)).context_window_frames == 65
    assert list(window_offsets(32, 1)) == list(range(-32, 33))


@pytest.mark.parametrize("geometry", DISAGREEING, ids=geometry_id)
def test_a_geometry_the_reference_cannot_run_is_refused(tmp_path, state1234, geometry):
    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd.predictor import ContextResolution, VADFromScratchPredictor, context_window_frames, window_offsets

    half, jump = geometry
    W, formula = len(cases.offsets(half, jump)), cases.reference_formula(half, jump)
    assert W != formula
    message = f"formula gives {formula} frames, its window offsets are {W}"
    with pytest.raises(ValueError, match=message):
        context_window_frames(half, jump)
    with pytest.raises(ValueError, match=message):
        VADFromScratchPredictor(_model(), "cpu", ContextResolution(half, jump))
    cfg = copy.deepcopy(REFERENCE_CONFIG)
    cfg["context_resolution"].update(context_window_half_frames=half, context_window_jump_frames=jump)
    path = write_reference_checkpoint(tmp_path / "geometry.checkpoint", state1234, cfg)
    for extended in (False, True):
        with pytest.raises(ValueError, match=message):
            VADFromScratchPredictor.from_checkpoint(path, "cpu", extended_front_end=extended)
    assert list(window_offsets(half, jump)) == list(cases.offsets(half, jump))     # the C ABI keeps serving its own arange geometry


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_every_geometry_of_the_table_is_accepted(tmp_path, state1234, geometry):
    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor

    half, jump = geometry
    cfg = copy.deepcopy(REFERENCE_CONFIG)
    cfg["context_resolution"].update(context_window_half_frames=half, context_window_jump_frames=jump)
    p = VADFromScratchPredictor.from_checkpoint(write_reference_checkpoint(tmp_path / "geometry.checkpoint", state1234, cfg), "cpu")
    assert (p.context_window_half_frames, p.context_window_jump_frames) == (half, jump)
    assert p.context_window_frames == len(cases.offsets(half, jump)) == cases.reference_formula(half, jump)
