"""Live post-processing (csrc/savad_live_post.h), the parts that need no GPU.  The host twin savad_live_post_host runs the inline
functions the kernel runs; what it emits over the ticks of a recording, concatenated, must be the segments of the library's own
offline host functions over the whole recording (savad_post_frames_host, savad_frames_to_samples + savad_samples_to_segments, which
the existing suite pins to the reference's goldens), every tick must meet the promptness rule, and the refusals come before any
launch.  The exhaustive part runs natively (tests/live_post_dump.cpp)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "live_post_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"
INVALID = -1
START, END = 0, 1


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def post_config(W, threshold, params):
    from voice_activity_detection_amd import _lib

    return _lib.savad_live_post_config(W, threshold, *params)


def state_bytes(lib, cfg, streams=1):
    n = ctypes.c_size_t()
    assert lib.savad_live_post_state_bytes(ctypes.byref(cfg), streams, ctypes.byref(n)) == 0
    return n.value


def feed(lib, cfg, state, first, probs, finish, slot=0):
    """one entry through the host twin -> [(kind, sample)], or None for count -1"""
    from voice_activity_detection_amd import _lib

    probs = np.ascontiguousarray(probs, dtype=np.float32)
    cap = (len(probs) + cfg.min_vally + cfg.min_hill + cfg.hang_before) // 2 + 4
    events = (_lib.savad_live_event * cap)()
    count = ctypes.c_int()
    rc = lib.savad_live_post_host(ctypes.byref(cfg), _p(state), slot, first, len(probs), int(finish), _p(probs) if len(probs) else None, events, cap,
                                  ctypes.byref(count))
    assert rc == 0, lib.savad_last_error()
    if count.value < 0:
        return None
    assert count.value <= cap, "more events than the stated bound"
    assert all(events[k].slot == slot for k in range(count.value))
    return [(events[k].kind, events[k].sample) for k in range(count.value)]


def offline(lib, probs, threshold, params):
    """the library's offline host functions over the whole recording -> [(kind, sample)]"""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    N, W = probs.shape
    boosted, trimmed = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint8)
    assert lib.savad_post_frames_host(_p(probs), N, W, threshold, *params, _p(boosted), _p(trimmed)) == 0
    frames = trimmed.astype(np.float64)
    num = lib.savad_frames_to_samples(_p(frames), N, 16000, 10.0, 25.0, None)
    assert num == (N - 1) * 160 + 400
    samples = np.empty(num, dtype=np.float64)
    assert lib.savad_frames_to_samples(_p(frames), N, 16000, 10.0, 25.0, _p(samples)) == num
    cap = N + 2
    starts, ends = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
    n = lib.savad_samples_to_segments(_p(samples), num, _p(starts), _p(ends), cap)
    assert 0 <= n <= cap
    out = []
    for a, b in zip(starts[:n], ends[:n]):
        out += [(START, int(a)), (END, int(b))]
    return out


def run_stream(lib, probs, threshold, params, ticks):
    """feeds `probs` in ticks of the given row counts (the last one finishes) and checks prefix, promptness and completeness"""
    cfg = post_config(probs.shape[1], threshold, params)
    want = offline(lib, probs, threshold, params)
    state = np.full(state_bytes(lib, cfg), 0xCD, dtype=np.uint8)   # the state needs no initialisation
    got, fed = [], 0
    v, h, b, _ = params
    for t, count in enumerate(ticks):
        fin = t + 1 == len(ticks)
        events = feed(lib, cfg, state, fed, probs[fed:fed + count], fin)
        assert events is not None
        got += events
        fed += count
        assert got == want[:len(got)], (params, ticks, t)
        if not fin:
            due = sum(1 for _, s in want if 160 * (fed - v - h - b) > s + 1)
            assert len(got) >= due, (params, ticks, t, "late")
    assert fed == len(probs) and got == want, (params, ticks)
    return want


def planted_probs(rng, n, W, threshold, p_flip=0.12):
    """[n, W] float32 whose thresholded row mean follows a 0/1 string with geometric run lengths; about a third of the rows have a
    mean within 1 ulp of the threshold (either side, and ON it), where the order of numpy's sum decides"""
    t = np.float32(threshold)
    bits = np.empty(n, dtype=np.uint8)
    cur, i = int(rng.integers(0, 2)), 0
    while i < n:
        run = int(rng.geometric(p_flip))
        bits[i:i + run] = cur
        cur ^= 1
        i += run
    probs = np.where(bits[:, None] != 0, t + np.float32(0.2), t - np.float32(0.2)).astype(np.float32) * np.ones((n, W), dtype=np.float32)
    probs += (rng.random((n, W), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)
    near = rng.random(n) < 0.33
    for r in np.flatnonzero(near):
        row = np.full(W, t, dtype=np.float32)
        if W > 1:
            d = (rng.random(W // 2, dtype=np.float32) * np.float32(0.3)).astype(np.float32)
            row[:W // 2] += d
            row[W - W // 2:] -= d            # a mean that would be t exactly in real arithmetic: float32 sums land 0 or 1 ulp off
        row[0] = np.nextafter(row[0], np.float32(rng.integers(0, 2)))
        probs[r] = row
    return np.ascontiguousarray(probs)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the stand-alone checker: host code that includes the kernel header, so it is built with hipcc (nothing is launched)"""
    from voice_activity_detection_amd.build import hipcc

    exe = tmp_path_factory.mktemp("live_post") / "live_post_dump"
    subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()

    return run


def test_exhaustive_strings_parameters_and_cuttings(dump):
    """every 0/1 string of length 1 .. 10 x (v, h, b, o) in {0, 1, 3}^4 x (row by row + empty finish | all in the finish | every
    two-cut split): events == offline segments, every tick prompt (v = h = b = 0: no look-ahead at all), event bound held"""
    (line,) = dump("exhaustive", 10)
    tag, runs, events = line.split()
    assert tag == "OK"
    strings = sum(2 ** n for n in range(1, 11))
    assert int(runs) == 81 * sum(2 ** n * (2 + (n + 1) * (n + 2) // 2) for n in range(1, 11)) and int(runs) > 60 * 81 * strings // 2
    assert int(events) > 0


def test_twin_agrees_with_exhaustive_checker_on_the_abi(lib):
    """the same small cases through the C ABI on both sides (the checker above uses the inline functions directly)"""
    for bits in ("1", "0", "0110", "1101100111", "0001000", "1110111011"):
        probs = np.array([[0.75 if c == "1" else 0.25] for c in bits], dtype=np.float32)
        for params in [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (3, 1, 0, 3), (0, 3, 1, 0), (1, 0, 3, 1)]:
            n = len(bits)
            run_stream(lib, probs, 0.5, params, [1] * n + [0])
            run_stream(lib, probs, 0.5, params, [n])
            run_stream(lib, probs, 0.5, params, [n // 2, 0, n - n // 2])


@pytest.mark.parametrize("params", [(20, 20, 10, 10), (3, 0, 0, 5)])
def test_randomised_long_strings(lib, params):
    """200 seeded strings of 200 .. 400 rows, tick sizes 0 .. 40, W in {1, 7, 8, 9, 128} with means within 1 ulp of the threshold"""
    rng = np.random.default_rng(sum(params))
    events = near = 0
    for case in range(200):
        W = (1, 7, 8, 9, 128)[case % 5]
        threshold = (0.5, 0.3, 0.61)[case % 3]
        n = int(rng.integers(200, 401))
        probs = planted_probs(rng, n, W, threshold)
        mean = probs.mean(axis=1)
        t = np.float32(threshold)
        near += int(np.sum((mean >= np.nextafter(t, np.float32(0))) & (mean <= np.nextafter(t, np.float32(1)))))
        ticks, left = [], n
        while left > 0:
            c = min(int(rng.integers(0, 41)), left)
            ticks.append(c)
            left -= c
        ticks.append(0)
        events += len(run_stream(lib, probs, threshold, params, ticks))
    assert events > 400 and near > 1000   # the cases have segments, and rows where the order of the sum matters


def test_hang_pass_does_not_run_without_hang_before(lib):
    """b = 0, o > 0: the reference's `hang_before > 0 or hang_before > 0` skips the pass, so hang_over changes nothing"""
    bits = "0011100000011000"
    probs = np.array([[0.75 if c == "1" else 0.25] for c in bits], dtype=np.float32)
    with_o = run_stream(lib, probs, 0.5, (0, 0, 0, 4), [3, 5, len(bits) - 8])
    assert with_o == run_stream(lib, probs, 0.5, (0, 0, 0, 0), [len(bits)])
    assert with_o != run_stream(lib, probs, 0.5, (0, 0, 1, 4), [len(bits)])   # with b > 0 it does


def test_state_is_bounded_and_carries_100000_rows(lib):
    sizes = {state_bytes(lib, post_config(7, 0.5, params)) for params in [(0, 0, 0, 0), (20, 20, 10, 10), (3000, 3000, 3000, 3000)]}
    assert len(sizes) == 1 and sizes.pop() <= 256                       # a function of neither the parameters ...
    cfg = post_config(7, 0.5, (20, 20, 10, 10))
    assert state_bytes(lib, cfg, 1024) == 1024 * state_bytes(lib, cfg)
    rng = np.random.default_rng(5)
    probs = planted_probs(rng, 100000, 7, 0.5, p_flip=0.05)
    ticks = [1000] * 100 + [0]
    want = run_stream(lib, probs, 0.5, (20, 20, 10, 10), ticks)          # ... nor of the rows fed: one state, 100 000 rows
    assert len(want) > 100   # (many segments: the long run is no empty comparison)


def test_skipped_entry_counts_minus_one_and_leaves_the_state(lib):
    cfg = post_config(1, 0.5, (3, 3, 3, 3))
    state = np.zeros(state_bytes(lib, cfg), dtype=np.uint8)
    probs = np.array([[0.75]] * 6 + [[0.25]] * 6, dtype=np.float32)
    assert feed(lib, cfg, state, 0, probs[:5], False) is not None
    before = state.copy()
    assert feed(lib, cfg, state, 7, probs[7:9], False) is None and np.array_equal(state, before)    # rows 5, 6 were skipped
    assert feed(lib, cfg, state, -3, probs[:1], False) is None and np.array_equal(state, before)
    assert feed(lib, cfg, state, 5, probs[5:], True) is not None
    closed = state.copy()
    assert feed(lib, cfg, state, 12, probs[:1], False) is None and np.array_equal(state, closed)    # finished: only row 0 restarts
    assert feed(lib, cfg, state, 0, probs, True) == offline(lib, probs, 0.5, (3, 3, 3, 3))


def test_abi_refusals(lib):
    from voice_activity_detection_amd import _lib

    n = ctypes.c_size_t()
    at = ctypes.c_size_t()
    good = post_config(7, 0.5, (1, 1, 1, 1))
    for bad, word in [(post_config(0, 0.5, (0, 0, 0, 0)), b"W = 0"), (post_config(129, 0.5, (0, 0, 0, 0)), b"W = 129"),
                      (post_config(7, 0.5, (-1, 0, 0, 0)), b"negative"), (post_config(7, 0.5, (0, 0, 0, -2)), b"negative")]:
        assert lib.savad_live_post_state_bytes(ctypes.byref(bad), 1, ctypes.byref(n)) == INVALID and word in lib.savad_last_error()
        state = np.zeros(64, dtype=np.uint8)
        count = ctypes.c_int()
        assert lib.savad_live_post_host(ctypes.byref(bad), _p(state), 0, 0, 0, 0, None, None, 0, ctypes.byref(count)) == INVALID
    assert lib.savad_live_post_state_bytes(None, 1, ctypes.byref(n)) == INVALID
    assert lib.savad_live_post_state_bytes(ctypes.byref(good), 0, ctypes.byref(n)) == INVALID
    assert lib.savad_live_post_host(ctypes.byref(good), None, 0, 0, 0, 0, None, None, 0, None) == INVALID
    # a planned tick (addresses that are never dereferenced): sizes, then every refusal of the stage itself -- nothing is launched
    cfg = _lib.savad_live_config(2, 40000, 19, 9, 1024)
    assert lib.savad_live_table_bytes(ctypes.byref(cfg), 2, ctypes.byref(n)) == 0
    slots = (_lib.savad_live_slot * 2)()
    table = ctypes.create_string_buffer(n.value)
    counts = _lib.savad_live_counts()
    assert lib.savad_live_open(ctypes.byref(cfg), slots, 0) == 0
    pushes = (_lib.savad_live_push * 1)(_lib.savad_live_push(0, 16000, 1, 1, ctypes.c_void_p(1 << 30)))
    assert lib.savad_live_plan(ctypes.byref(cfg), slots, pushes, 1, ctypes.c_void_p(1 << 20), table, len(table), ctypes.byref(counts), None) == 0
    assert counts.rows == 101
    assert lib.savad_live_post_event_bytes(ctypes.byref(cfg), ctypes.byref(good), table, ctypes.byref(n), ctypes.byref(at)) == 0
    ev_bytes = n.value
    assert at.value == 16 and ev_bytes == 16 + 16 * ((101 + 3) // 2 + 4)
    assert lib.savad_live_post_workspace_bytes(ctypes.byref(cfg), ctypes.byref(good), table, ctypes.byref(n)) == 0
    ws_bytes = n.value
    assert lib.savad_live_post_event_bytes(ctypes.byref(cfg), ctypes.byref(good), None, ctypes.byref(n), None) == INVALID
    assert lib.savad_live_post_event_bytes(ctypes.byref(cfg), None, table, ctypes.byref(n), None) == INVALID
    A = ctypes.c_void_p(1 << 24)   # aligned addresses that a refusal never touches

    def post(pc=good, th=table, td=A, probs=A, state=A, events=A, eb=ev_bytes, ws=A, wb=ws_bytes):
        return lib.savad_live_post(ctypes.byref(cfg), ctypes.byref(pc) if pc is not None else None, th, td, probs, state, events, eb, ws, wb, None)

    assert post(pc=None) == INVALID and b"null post config" in lib.savad_last_error()
    assert post(pc=post_config(8, 0.5, (1, 1, 1, 1))) == INVALID and b"W = 8" in lib.savad_last_error()
    assert post(pc=post_config(7, 0.5, (1, -1, 1, 1))) == INVALID and b"negative" in lib.savad_last_error()
    assert post(th=None) == INVALID and post(td=None) == INVALID
    for name in ("probs", "state", "events", "ws"):
        assert post(**{name: None}) == INVALID and b"null" in lib.savad_last_error()
    assert post(events=ctypes.c_void_p((1 << 24) + 4)) == INVALID and b"aligned" in lib.savad_last_error()
    assert post(eb=ev_bytes - 1) == INVALID and b"event buffer too small" in lib.savad_last_error()
    assert post(wb=ws_bytes - 1) == INVALID and b"workspace too small" in lib.savad_last_error()


def test_python_refuses_what_has_no_online_form():
    from voice_activity_detection_amd.live import post_frames
    from voice_activity_detection_amd.predictor import VADPredictParameters

    assert post_frames(VADPredictParameters(None, 0.4, 200, 200, 100, 100)) == (20, 20, 10, 10)
    assert post_frames(VADPredictParameters(None, 0.4, 26, 24, 5, 15)) == (round(2.6), round(2.4), round(0.5), round(1.5))
    with pytest.raises(ValueError, match="activity_max_seconds"):
        post_frames(VADPredictParameters(activity_max_seconds=10))
    with pytest.raises(ValueError, match="return_probs"):
        post_frames(VADPredictParameters(return_probs=True, probs_sample_rate=100))
    with pytest.raises(ValueError, match="split_max_seconds"):
        post_frames(VADPredictParameters(split_max_seconds=30.0))
    with pytest.raises(ValueError, match="negative"):
        post_frames(VADPredictParameters(min_hill_ms=-20))


def test_header_declares_the_stage():
    text = (REPO / "include" / "savad.h").read_text()
    for name in ("savad_live_post(", "savad_live_post_host(", "savad_live_post_state_bytes(", "savad_live_post_event_bytes(",
                 "savad_live_post_workspace_bytes(", "savad_live_event", "savad_live_post_config"):
        assert name in text
