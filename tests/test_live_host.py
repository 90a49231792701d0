"""The live mode, the parts that need no GPU: the host plan (csrc/savad_live_plan.h through the stand-alone tests/live_dump.cpp, built
with the address and undefined-behaviour sanitizers), the prefix property of the log-mel front-end that the plan's frame counts rest
on, and the library's refusals, which come before anything is launched."""
import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "live_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"
IRREGULAR = [1, 159, 160, 161, 0, 4000, 7, 255, 257]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    exe = tmp_path_factory.mktemp("live") / "live_dump"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True, timeout=120)
        assert out.stderr == ""
        return out.stdout.splitlines()

    return run


def K_brute(n):
    """frames whose 416-sample stretch 160 f - 208 .. 160 f + 207 lies below n, once the offline minimum of 257 samples is there"""
    if n < 257:
        return 0
    f = 0
    while 160 * f + 207 < n:
        f += 1
    return f


def test_counts_against_brute_force(dump):
    half = 19
    lines = dump("counts", half, 8000)
    assert len(lines) == 8001
    for n, line in enumerate(lines):
        got = list(map(int, line.split()))
        K = K_brute(n)
        E = max(0, K - 2 * half)
        N = 1 + n // 160
        keep = max(0, 160 * K - 208)
        assert got == [n, K, E, N, N - E, keep], (n, got)
        assert keep % 4 == 0 and n - keep <= 415


def parse(lines):
    """[geometry, ticks]: a tick = dict(counts, entries, tiles, items) or dict(refused=...)"""
    assert lines[0].startswith("G ")
    names = "W P max_new max_rows feat_cap logp_cap sample_cap stride max_tiles max_items".split()
    geo = dict(zip(names, map(int, lines[0].split()[1:])))
    ticks = []
    enames = ("slot finish n_before n_after base_before base_after keep_off keep_count row_first row_count row_out n_frames frame_first_mod "
              "n_windows win_first_mod win_kept item0 head_write tail_count tail_j0 rows_first rows_ok").split()
    for line in lines[1:]:
        tag, *vals = line.split()
        if tag == "X":
            ticks.append({"refused": line})
        elif tag == "T":
            ticks.append({"counts": list(map(int, vals)), "entries": [], "tiles": [], "items": []})
        elif tag == "E":
            ticks[-1]["entries"].append(dict(zip(enames, map(int, vals))))
        elif tag == "L":
            ticks[-1]["tiles"].append(dict(zip("entry count J0 j_last jA_end jB0 pos".split(), map(int, vals))))
        elif tag == "I":
            ticks[-1]["items"].append(tuple(map(int, vals)))
    return geo, ticks


def chunkings(total, rng):
    yield [total]
    yield [1600] * (total // 1600) + ([total % 1600] if total % 1600 else [])
    seq, left, k = [], total, 0
    while left > 0:
        c = min(IRREGULAR[k % len(IRREGULAR)], left)
        seq.append(c)
        left -= c
        k += 1
    yield seq
    seq, left = [], total
    while left > 0:
        c = min(int(rng.integers(0, 4001)), left)
        seq.append(c)
        left -= c
    yield seq


@pytest.mark.parametrize("half,jump", [(19, 9), (10, 2), (4, 4)])   # W = 7, 11, 3
def test_rows_tiles_items_and_state(dump, half, jump):
    """Every tick of a push sequence: emitted rows contiguous and summing to N; tiles cover the new frames once, read only samples the
    buffer holds (or the mirrored stretches) and write ring rows the tick's windows do not still need; every window sits at slot
    j mod (32 // W); the kept tail is inside what the last tick left."""
    rng = np.random.default_rng(half)
    for total in (300, 6250, 6720, 16001, 37333):
        for seq in chunkings(total, rng):
            ticks_arg = [f"0:{c}" for c in seq] + ["0:0f"]
            geo, ticks = parse(dump("sim", 1, max(4000, *seq), half, jump, *ticks_arg))
            W, P = geo["W"], geo["P"]
            assert W == len(np.arange(-half, 0, jump)) + 1 + len(np.arange(1, half + 1, jump)) and P == 32 // W
            N = 1 + total // 160
            next_row = next_frame = next_window = 0
            held = 0                      # samples the current buffer holds from position 0
            ring = {}                     # ring position -> absolute feature row
            for tick in ticks:
                assert "refused" not in tick, tick
                (e,) = tick["entries"]
                assert e["rows_ok"] == 1 and e["rows_first"] == e["row_first"] == next_row and e["row_out"] == 0
                next_row += e["row_count"]
                assert e["row_count"] <= geo["max_rows"] and e["n_frames"] <= geo["max_new"]
                # the state: the kept tail lies inside what the buffer held, the new content fits
                assert e["keep_off"] >= 0 and e["keep_off"] + e["keep_count"] == held
                held = e["keep_count"] + (e["n_after"] - e["n_before"])
                assert held <= geo["sample_cap"] and e["base_after"] % 4 == 0 and held == e["n_after"] - e["base_after"]
                # tiles
                f = next_frame
                for t in tick["tiles"]:
                    assert 1 <= t["count"] <= 32 and t["J0"] == 160 * f + 48 and t["pos"] == f % geo["feat_cap"]
                    assert t["pos"] + t["count"] <= geo["feat_cap"]
                    lo, hi = t["J0"] - 256, 160 * (f + t["count"] - 1) + 460 + 4 - 256   # samples the tile's frames read
                    assert hi <= t["j_last"] + 4 - 256
                    if lo < 0:
                        assert t["jA_end"] == 256 and (e["head_write"] or e["n_before"] >= 257)
                    else:
                        assert lo >= e["base_after"]
                    if e["finish"] and hi > e["n_after"]:
                        assert t["jB0"] - 256 <= (e["n_after"] + 3) // 4 * 4 and t["jB0"] == e["tail_j0"]
                        assert t["j_last"] + 4 - t["jB0"] == e["tail_count"] <= 212
                    else:
                        assert hi <= e["n_after"], (t, e)
                    for k in range(t["count"]):
                        ring[(f + k) % geo["feat_cap"]] = f + k
                    f += t["count"]
                assert f - next_frame == e["n_frames"] and e["frame_first_mod"] == next_frame % geo["feat_cap"]
                next_frame = f
                if not e["finish"]:
                    assert next_frame == K_brute(e["n_after"])
                # items: window j at slot j mod P, its rows in the ring
                assert len(tick["items"]) % P == 0 and len(tick["items"]) <= geo["max_items"]
                j = next_window
                for idx, entry, centre in tick["items"]:
                    if entry < 0:
                        continue
                    assert idx % P == j % P and centre == (j + half) % geo["feat_cap"]
                    if j == next_window:
                        assert idx == e["item0"]
                    for o in range(-half, half + 1):
                        assert ring[(centre + o) % geo["feat_cap"]] == j + half + o
                    j += 1
                assert j - next_window == e["n_windows"] and e["win_first_mod"] == next_window % geo["logp_cap"]
                assert e["win_kept"] == min(next_window, 2 * half) and e["n_windows"] + e["win_kept"] <= geo["logp_cap"]
                next_window = j
                assert next_window == max(0, next_frame - 2 * half)
                if not e["finish"]:
                    assert next_row == next_window
            assert next_row == N == next_frame, (total, seq)


def test_many_streams_share_a_tick(dump):
    geo, ticks = parse(dump("sim", 4, 1600, 19, 9, "0:1600,2:800", "0:1600,1:1600,2:1600", "0:1600,1:1600,2:0f", "3:1600,2:300", "0:1600,1:5,3:9"))
    rows = 0
    for tick in ticks:
        assert "refused" not in tick
        first = 0
        for e in tick["entries"]:
            assert e["row_out"] == first and e["rows_ok"] == 1
            first += e["row_count"]
        assert first == tick["counts"][3]
        rows += first
        assert len(tick["items"]) % geo["P"] == 0
    # slot 2 was finished in tick 3 and opened again in tick 4: it starts from nothing
    e2 = [e for e in ticks[3]["entries"] if e["slot"] == 2][0]
    assert e2["n_before"] == 0 and e2["base_before"] == 0 and e2["row_first"] == 0


def test_plan_refusals(dump):
    _, ticks = parse(dump("sim", 2, 1600, 19, 9, "0:1601", "0:100f", "5:10", "0:10,0:10", "0:300f"))
    assert "maximum" in ticks[0]["refused"] and "needs" in ticks[1]["refused"] and "slot" in ticks[2]["refused"]
    assert "twice" in ticks[3]["refused"] and "refused" not in ticks[4]
    assert dump("sim", 1, 1600, 200, 1)[0].startswith("X -2")   # W = 401


def test_logmel_prefix_property():
    """frames below K(n) of a prefix are the whole signal's; frame K(n) is not"""
    from oracle import logmel

    audio = (np.random.default_rng(11).standard_normal(32000) * 0.1).astype(np.float32)
    full = logmel.log_mel(audio)
    for n in (257, 415, 416, 1000, 5000, 31999):
        K = K_brute(n)
        part = logmel.log_mel(audio[:n])
        assert K >= 1 and part.shape[0] == 1 + n // 160
        assert np.abs(part[:K] - full[:K]).max() <= 1e-6, n
        # The first frame that is NOT the whole signal's.  K(n) counts the kernel's 416-sample read stretch (160 f - 208 .. 160 f + 207);
        # the window itself covers 160 f - 200 .. 160 f + 199 (the oracle's WIN = 400 centred in N_FFT = 512), so for n mod 160 in
        # [40, 48) -- 1000 and 5000 here -- frame K(n) still has all its samples and the first frame that differs is K(n) + 1.
        first_cut = K if 160 * K + logmel.WIN // 2 - 1 >= n else K + 1
        assert first_cut - K == (n in (1000, 5000))
        if first_cut > K:
            assert np.abs(part[K] - full[K]).max() <= 1e-6, n
        if first_cut < part.shape[0]:
            assert np.abs(part[first_cut] - full[first_cut]).max() > 1e-2, n


# ---- the library's refusals (host code of libsavad.so: nothing is launched, so no GPU is needed) ----------------------------------

@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def test_library_refuses_before_launch(lib):
    from voice_activity_detection_amd import _lib

    E_INVALID, E_UNSUPPORTED = -1, -2
    cfg = _lib.savad_live_config(2, 1600, 19, 9, 1024)
    nbytes = ctypes.c_size_t()
    assert lib.savad_live_state_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == 0 and nbytes.value % 256 == 0
    wide = _lib.savad_live_config(2, 1600, 200, 1, 1024)
    assert lib.savad_live_state_bytes(ctypes.byref(wide), ctypes.byref(nbytes)) == E_UNSUPPORTED
    assert b"64 frames" in lib.savad_last_error()
    assert lib.savad_live_table_bytes(ctypes.byref(cfg), 2, ctypes.byref(nbytes)) == 0
    slots = (_lib.savad_live_slot * 2)()
    table = ctypes.create_string_buffer(nbytes.value)
    counts = _lib.savad_live_counts()
    state = ctypes.c_void_p(1 << 20)   # an address, never read by the plan
    data = ctypes.c_void_p(1 << 30)

    def plan(*pushes):
        arr = (_lib.savad_live_push * len(pushes))(*[_lib.savad_live_push(s, n, 1, f, data) for s, n, f in pushes])
        return lib.savad_live_plan(ctypes.byref(cfg), slots, arr, len(pushes), state, table, len(table), ctypes.byref(counts), None)

    assert plan((0, 100, 0)) == E_INVALID and b"closed" in lib.savad_last_error()
    assert lib.savad_live_open(ctypes.byref(cfg), slots, 0) == 0
    assert lib.savad_live_open(ctypes.byref(cfg), slots, 0) == E_INVALID
    assert plan((0, 1601, 0)) == E_INVALID and b"maximum" in lib.savad_last_error()
    assert plan((0, 256, 1)) == E_INVALID and b"257" in lib.savad_last_error()
    assert lib.savad_live_plan(ctypes.byref(cfg), slots, None, 0, state, None, 0, ctypes.byref(counts), None) == E_INVALID
    assert plan((0, 1600, 0)) == 0 and counts.entries == 1 and counts.rows == 0 and counts.tiles == 1
    # stage entries and the step: null tables, and a table whose stream has been closed since
    for fn in (lib.savad_live_append, lib.savad_live_logmel):
        assert fn(ctypes.byref(cfg), table, None, None) == E_INVALID and b"null table" in lib.savad_last_error()
        assert fn(ctypes.byref(cfg), None, None, None) == E_INVALID
    assert lib.savad_live_gather(ctypes.byref(cfg), table, None, 0, 0, None, None) == E_INVALID
    assert lib.savad_live_boost(ctypes.byref(cfg), table, None, None, None, None, None) == E_INVALID
    assert lib.savad_live_step(None, ctypes.byref(cfg), slots, table, None, None, None, None, 0, None) == E_INVALID
    slots[0].open = 0
    assert lib.savad_live_commit(ctypes.byref(cfg), table, slots) == E_INVALID and b"closed" in lib.savad_last_error()
