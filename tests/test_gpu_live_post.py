"""Live post-processing on the GPU (savad_live_post, LiveVAD(post=...), the `live` command).  1. the stage alone, tick for tick,
against the host twin and against the offline device post-processing of the whole matrix; 2. a skipped tick; 3. end to end under
the pinned kernel variants against offline predict(); 4. the automatic schedule against the offline post-processing of the live
run's own probabilities; 5. one tick between guards; 6. the command line."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.buffer_arena import BufferArena
from tests.test_gpu_live import HALF, JUMP, W, Entry, chunking
from tests.test_gpu_schedule_workspace import Knobs, ptr
from tests.test_live_post_host import END, START, feed, offline, planted_probs, post_config, state_bytes

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CLIP = REPO / "tests" / "golden" / "data" / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav"
STAGE_TOTALS = [300, 6250, 6720, 37333]
PARAMS = [(20, 20, 10, 10), (0, 0, 0, 0), (3, 2, 1, 4)]
PINNED = [("fp32", 4), ("fp32s", 8), ("bf16", 8)]
THRESHOLD = 0.5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def planted():
    """[N, 7] planted probabilities per stream total: seeded runs, a third of the rows within 1 ulp of the threshold; never written"""
    return [planted_probs(np.random.default_rng(70 + k), 1 + n // 160, W, THRESHOLD) for k, n in enumerate(STAGE_TOTALS)]


# ---- 1. the stage, bits --------------------------------------------------------------------------------------------------------------

class StageRun:
    """Three slots, real plans (savad_live_plan with addresses that are never dereferenced), savad_live_post alone on planted probs."""

    def __init__(self, torch, lib, params, max_push):
        from voice_activity_detection_amd import _lib

        self.torch, self.lib, self._lib = torch, lib, _lib
        self.cfg = _lib.savad_live_config(3, max_push, HALF, JUMP, 1024)
        self.post = post_config(W, THRESHOLD, params)
        self.slots = (_lib.savad_live_slot * 3)()
        n = ctypes.c_size_t()
        _lib.check(lib.savad_live_table_bytes(ctypes.byref(self.cfg), 3, ctypes.byref(n)))
        self.table = np.zeros(n.value, dtype=np.uint8)
        self.one = state_bytes(lib, self.post)
        assert state_bytes(lib, self.post, 3) == 3 * self.one
        self.state = torch.full((3 * self.one,), 0xEE, dtype=torch.uint8, device="cuda")   # no initialisation needed
        self.twin = np.full((3, self.one), 0xEE, dtype=np.uint8)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plan(self, pushes):
        """pushes: [(slot, samples, finish)] -> the tick's entries"""
        _lib, lib = self._lib, self.lib
        arr = (_lib.savad_live_push * len(pushes))(*[_lib.savad_live_push(s, n, 1, int(f), ctypes.c_void_p(1 << 30)) for s, n, f in pushes])
        counts = _lib.savad_live_counts()
        self.host = ctypes.c_void_p(self.table.ctypes.data)
        _lib.check(lib.savad_live_plan(ctypes.byref(self.cfg), self.slots, arr, len(pushes), ctypes.c_void_p(1 << 20), self.host, self.table.size,
                                       ctypes.byref(counts), None))
        size = ctypes.sizeof(Entry)
        self.counts = counts
        return [Entry.from_buffer_copy(self.table[64 + i * size:64 + (i + 1) * size].tobytes()) for i in range(len(pushes))]

    def commit(self):
        self._lib.check(self.lib.savad_live_commit(ctypes.byref(self.cfg), self.host, self.slots))

    def post_tick(self, entries, rows_of, twin=True):
        """savad_live_post on the planned tick; rows_of(entry) -> its [row_count, W] probs.  -> per entry [(kind, sample)] or None"""
        torch, lib, _lib = self.torch, self.lib, self._lib
        probs = np.zeros((self.counts.rows, W), dtype=np.float32)
        for e in entries:
            probs[e.row_out:e.row_out + e.row_count] = rows_of(e)
        probs_dev = torch.from_numpy(probs).cuda()
        table_dev = torch.from_numpy(self.table).cuda()
        n, at = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.savad_live_post_event_bytes(ctypes.byref(self.cfg), ctypes.byref(self.post), self.host, ctypes.byref(n), ctypes.byref(at)))
        events = torch.full((n.value,), 0x77, dtype=torch.uint8, device="cuda")
        _lib.check(lib.savad_live_post_workspace_bytes(ctypes.byref(self.cfg), ctypes.byref(self.post), self.host, ctypes.byref(n)))
        ws = torch.full((max(n.value, 16),), 0x55, dtype=torch.uint8, device="cuda")
        _lib.check(lib.savad_live_post(ctypes.byref(self.cfg), ctypes.byref(self.post), self.host, ptr(table_dev), ptr(probs_dev), ptr(self.state),
                                       ptr(events), events.numel(), ptr(ws), ws.numel(), self.stream))
        host = events.cpu().numpy()
        k = len(entries)
        meta = host[:4 * (2 * k + 1)].view(np.int32)
        offsets, cnt = meta[:k + 1], meta[k + 1:]
        rec = host[at.value:at.value + 16 * int(offsets[k])].view(np.dtype([("sample", np.int64), ("slot", np.int32), ("kind", np.int32)]))
        out = []
        for i, e in enumerate(entries):
            if cnt[i] < 0:
                assert offsets[i + 1] == offsets[i]
                out.append(None)
                continue
            assert offsets[i + 1] - offsets[i] == cnt[i]
            mine = rec[offsets[i]:offsets[i + 1]]
            assert (mine["slot"] == e.slot).all()
            out.append([(int(r["kind"]), int(r["sample"])) for r in mine])
            if twin:   # the host twin, tick for tick: the same events, the same state
                want = feed(lib, self.post, self.twin[e.slot], e.row_first, rows_of(e), e.finish, slot=e.slot)
                assert out[-1] == want, (e.slot, e.row_first, e.row_count)
        if twin:
            got = self.state.cpu().numpy().reshape(3, self.one)
            for e in entries:
                assert np.array_equal(got[e.slot], self.twin[e.slot]), ("state", e.slot)
        return out


def offline_device(torch, probs, params):
    """savad_post_frames + savad_post_segments of the whole matrix -> [(kind, sample)]"""
    from voice_activity_detection_amd.postprocessing import post_frames_device, segments_device

    v, h, b, o = params
    boosted, trimmed = post_frames_device(torch.from_numpy(probs).cuda(), THRESHOLD, min_vally=v, min_hill=h, hang_before=b, hang_over=o)
    starts, ends = segments_device(trimmed, boosted, sample_rate=16000, hop_ms=10, window_ms=25, max_length_seconds=None)
    out = []
    for a, b_ in zip(starts, ends):
        out += [(START, int(a)), (END, int(b_))]
    return out


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_stage_equals_the_twin_tick_for_tick_and_the_offline_segments(torch_cuda, lib, planted, name, params):
    """four recordings over three slots: one opens per tick (late opens), the fourth takes the first slot that is free again.  (a): one
    push that also finishes -- 234 rows in one tick for 37 333 samples, four turns of the 64-row loop; (b), (c): pushes, then a
    finish of its own that shares its tick with the others' pushes."""
    run = StageRun(torch_cuda, lib, params, max(STAGE_TOTALS))
    cuts = [chunking(name, n) for n in STAGE_TOTALS]
    waiting, active = list(range(len(STAGE_TOTALS))), {}   # slot -> [recording, next chunk]
    got = [[] for _ in STAGE_TOTALS]
    biggest = 0
    while waiting or active:
        free = [s for s in range(3) if not run.slots[s].open]
        if waiting and free:
            assert lib.savad_live_open(ctypes.byref(run.cfg), run.slots, free[0]) == 0
            active[free[0]] = [waiting.pop(0), 0]
        pushes = []
        for slot, (rec, k) in active.items():
            if k < len(cuts[rec]):
                pushes.append((slot, cuts[rec][k], name == "a"))
                active[slot][1] = k + 1
            else:
                pushes.append((slot, 0, True))
        entries = run.plan(pushes)
        by_slot = {slot: rec for slot, (rec, _) in active.items()}
        events = run.post_tick(entries, lambda e: planted[by_slot[e.slot]][e.row_first:e.row_first + e.row_count])
        for e, evs in zip(entries, events):
            assert evs is not None
            got[by_slot[e.slot]] += evs
            biggest = max(biggest, e.row_count)
            if e.finish:
                assert e.row_first + e.row_count == len(planted[by_slot[e.slot]])
                del active[e.slot]
        run.commit()
    if name == "a":
        assert biggest == 234
    some = 0
    for rec, probs in enumerate(planted):
        want = offline_device(torch_cuda, probs, params)
        assert got[rec] == want == offline(lib, probs, THRESHOLD, params), (rec, name, params)
        some += len(want)
    assert some >= 4


# ---- 2. a skipped tick ---------------------------------------------------------------------------------------------------------------

def test_skipped_tick_counts_minus_one_and_leaves_the_state(torch_cuda, lib, planted):
    run = StageRun(torch_cuda, lib, (3, 2, 1, 4), 4000)
    probs = planted[3]
    assert lib.savad_live_open(ctypes.byref(run.cfg), run.slots, 0) == 0 and lib.savad_live_open(ctypes.byref(run.cfg), run.slots, 2) == 0
    rows_of = lambda e: probs[e.row_first:e.row_first + e.row_count]   # noqa: E731
    for _ in range(3):                                       # rows 0 .. of both streams
        entries = run.plan([(0, 4000, False), (2, 4000, False)])
        assert all(evs is not None for evs in run.post_tick(entries, rows_of))
        run.commit()
    assert entries[0].row_first + entries[0].row_count > 0
    run.plan([(0, 4000, False)])                             # slot 0's post stage is skipped for one tick ...
    run.commit()
    before = run.state.cpu().numpy().copy()
    entries = run.plan([(0, 4000, False), (2, 4000, False)])
    events = run.post_tick(entries, rows_of, twin=False)     # ... so its next entry does not continue the state; slot 2's does
    assert events[0] is None and events[1] is not None
    after = run.state.cpu().numpy()
    assert np.array_equal(after[:run.one], before[:run.one]) and not np.array_equal(after[2 * run.one:], before[2 * run.one:])
    run.commit()
    torch_cuda.cuda.synchronize()                            # nothing faulted


# ---- 3. end to end, pinned variants --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recordings():
    from tests.test_gpu_live import TOTALS
    from voice_activity_detection_amd.features import load_wav_mono16k

    out = [load_wav_mono16k(CLIP)]
    for k, n in list(enumerate(TOTALS))[3:5]:               # signals[3:5] of tests/test_gpu_live.py
        t = np.arange(n, dtype=np.float64) / 16000.0
        chirp = 0.2 * np.sin(2 * np.pi * (200.0 + 900.0 * t) * t)
        out.append((np.random.default_rng(40 + k).standard_normal(n) * 0.05 + chirp).astype(np.float32))
    return out


def live_activities(model, audio, parameters, name, collect_probs=False):
    """one recording through LiveVAD(post=...) under chunking `name` -> (activities, events, probs or None)"""
    from voice_activity_detection_amd import LiveVAD

    cuts = chunking(name, len(audio))
    vad = LiveVAD(model, "cuda", streams=2, max_push_samples=max(cuts), post=parameters)
    vad.open()
    slot = vad.open()                                        # (slot 1: the events carry the slot)
    ticks, at = [], 0

    def made(tick):
        ticks.append(tick)
        if len(ticks) % 3:                                   # every third tick is left unread: its successor fetches it first, in order
            tick.events(slot)

    for c in cuts:
        made(vad.push({slot: audio[at:at + c]}))
        at += c
    made(vad.finish([slot]))
    activities = [a for tick in ticks for a in tick.activities(slot)]
    events = [e for tick in ticks for e in tick.events(slot)]
    assert not vad.in_voice(slot)
    import torch

    return activities, events, (torch.cat([t[slot][1] for t in ticks]) if collect_probs else None)


@pytest.mark.parametrize("name", ["b", "c"])
@pytest.mark.parametrize("precision,row_mode", PINNED)
def test_live_activities_equal_offline_predict(torch_cuda, model, recordings, precision, row_mode, name):
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    with Knobs(model, precision, row_mode):
        host = VADFromScratchPredictor(model, "cuda")
        dev = VADFromScratchPredictor(model, "cuda", device_post=True)
        for audio in recordings:
            # seeded weights may never cross 0.5: the threshold is the median of the offline mean (the parent's offline path)
            threshold = float(np.median(host.predict_audio_device(audio)[1].cpu().numpy()))
            parameters = VADPredictParameters(None, threshold, 30, 30, 30, 30)
            want = host.predict(audio, parameters).activities
            # (no empty comparison: the clip has 18 activities at these parameters and the 37 333-sample signal 4; the 16 001-sample
            # signal is one second long and has 2, so the floor of three holds for the recordings that can reach it)
            assert len(want) >= (3 if len(audio) > 16001 else 1)
            assert dev.predict(audio, parameters).activities == want and dev.post_stats["device"] > 0
            got, events, _ = live_activities(model, audio, parameters, name)
            assert got == want, (precision, name, len(audio))
            assert [k for k, _ in events] == [START, END] * len(want)


# ---- 4. the automatic schedule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
def test_automatic_schedule_against_its_own_probabilities(torch_cuda, model, recordings, precision):
    """row_mode 0: the live forwards see other batches than the offline ones, so the reference is the offline post-processing of the
    live run's OWN concatenated probabilities -- exact, whatever rounding the schedules differ by"""
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    with Knobs(model, precision, 0):
        pred = VADFromScratchPredictor(model, "cuda", device_post=True)
        audio = recordings[0]
        threshold = float(np.median(pred.predict_audio_device(audio)[1].cpu().numpy()))
        parameters = VADPredictParameters(None, threshold, 30, 30, 30, 30)
        got, _, probs = live_activities(model, audio, parameters, "c", collect_probs=True)
        want_host, _ = pred._post_host(probs, parameters)
        want_dev, _ = pred._post_device(probs, parameters)
    assert len(want_host) >= 3 and got == want_host == want_dev


def test_python_refusals_and_sessions_without_post(torch_cuda, model):
    from voice_activity_detection_amd import LiveSession, LiveVAD, VADPredictParameters
    from voice_activity_detection_amd._lib import SavadError

    for bad, word in [(VADPredictParameters(activity_max_seconds=5), "activity_max_seconds"), (VADPredictParameters(return_probs=True), "return_probs"),
                      (VADPredictParameters(split_max_seconds=10.0), "split_max_seconds"), (VADPredictParameters(hang_over_ms=-10), "negative")]:
        with pytest.raises(ValueError, match=word):
            LiveVAD(model, "cuda", 2, 1600, post=bad)
        with pytest.raises(ValueError, match=word):
            LiveSession(model, "cuda", 1600, post=bad)
    plain = LiveVAD(model, "cuda", 1, 1600)
    a = plain.open()
    tick = plain.push({a: np.zeros(1600, np.float32)})
    with pytest.raises(SavadError, match="post"):
        tick.events(a)
    # a tick whose post stage was skipped: the stream's next entry gets count -1, which the fetch reports
    vad = LiveVAD(model, "cuda", 1, 16000, post=VADPredictParameters(threshold=0.25))
    a = vad.open()
    assert vad.push({a: np.zeros(16000, np.float32)}).events(a) == [(START, 0)] and vad.in_voice(a)
    post, vad.post = vad.post, None
    vad.push({a: np.zeros(16000, np.float32)})
    vad.post = post
    with pytest.raises(SavadError, match="skipped"):
        vad.push({a: np.zeros(16000, np.float32)}).events(a)
    session = LiveSession(model, "cuda", 16000, post=VADPredictParameters(threshold=0.25))
    session.push(np.zeros(16000, np.float32))                # silence: every probability is 0.5 > 0.25
    assert session.events() == [(START, 0)] and session.activities() == [] and session.in_voice()
    session.finish()
    assert session.events() == [(END, 100 * 160 + 400 - 1)] and len(session.activities()) == 1 and not session.in_voice()


# ---- 5. caller's buffers -----------------------------------------------------------------------------------------------------------------

def test_post_stays_inside_the_callers_buffers(torch_cuda, lib, planted):
    """one tick (6 720 samples pushed and finished: 43 rows) with post state, event buffer and workspace between guards, each at
    the 16 bytes include/savad.h asks for and no more"""
    from voice_activity_detection_amd import _lib

    torch = torch_cuda
    run = StageRun(torch, lib, (3, 2, 1, 4), 6720)
    assert lib.savad_live_open(ctypes.byref(run.cfg), run.slots, 1) == 0
    (e,) = run.plan([(1, 6720, True)])
    assert (e.row_first, e.row_count) == (0, 43)
    probs = planted[2]
    n, at = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.savad_live_post_event_bytes(ctypes.byref(run.cfg), ctypes.byref(run.post), run.host, ctypes.byref(n), ctypes.byref(at)))
    ev_bytes = n.value
    _lib.check(lib.savad_live_post_workspace_bytes(ctypes.byref(run.cfg), ctypes.byref(run.post), run.host, ctypes.byref(n)))
    ws_bytes = n.value
    arena = BufferArena("cuda", 3 * run.one + ev_bytes + ws_bytes + probs.nbytes + run.table.size + 16 * 4096)
    state = arena.place_output(3 * run.one, 16, name="post state")
    events = arena.place_output(ev_bytes, 16, name="events")
    ws = arena.place_output(ws_bytes, 16, name="workspace")
    probs_dev = arena.place_input(torch.from_numpy(probs), 4, name="probs")
    table_dev = arena.place_input(torch.from_numpy(run.table[:run.counts.table_bytes].copy()), 16, name="table")
    _lib.check(lib.savad_live_post(ctypes.byref(run.cfg), ctypes.byref(run.post), run.host, ptr(table_dev), ptr(probs_dev), ptr(state), ptr(events),
                                   ev_bytes, ptr(ws), ws_bytes, run.stream))
    arena.check()
    host = events.cpu().numpy()
    offsets = host[:8].view(np.int32)
    rec = host[at.value:at.value + 16 * int(offsets[1])].view(np.dtype([("sample", np.int64), ("slot", np.int32), ("kind", np.int32)]))
    want = offline(lib, probs, THRESHOLD, (3, 2, 1, 4))
    assert [(int(r["kind"]), int(r["sample"])) for r in rec] == want and len(want) >= 2 and (rec["slot"] == 1).all()


# ---- 6. the command line -----------------------------------------------------------------------------------------------------------------

def test_live_command_writes_predicts_json(torch_cuda, model, state1234, tmp_path):
    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.features import load_wav_mono16k

    path = write_reference_checkpoint(tmp_path / "model.checkpoint", state1234, REFERENCE_CONFIG)
    # the two commands run other batches (automatic schedule), so their means differ by rounding: the threshold sits in the middle of
    # the widest gap between neighbouring means of the central fifth, far from every mean on that scale
    with Knobs(model, "fp32", 0):
        mean = np.sort(VADFromScratchPredictor(model, "cuda").predict_audio_device(load_wav_mono16k(CLIP))[1].cpu().numpy().astype(np.float64))
    mid = mean[2 * len(mean) // 5:3 * len(mean) // 5]
    k = int(np.argmax(np.diff(mid)))
    threshold = float((mid[k] + mid[k + 1]) / 2)
    assert mid[k + 1] - mid[k] > 1e-5
    flags = ["--threshold", repr(threshold), "--min-vally-ms", "30", "--min-hill-ms", "30", "--hang-before-ms", "30", "--hang-over-ms", "30"]
    base = [sys.executable, "-m", "voice_activity_detection_amd"]
    r = subprocess.run(base + ["predict", str(CLIP), str(path), "--output-path", str(tmp_path / "predict.json")] + flags, cwd=str(REPO),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["live", str(CLIP), str(path), "--push-ms", "100", "--output-path", str(tmp_path / "live.json")] + flags, cwd=str(REPO),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = json.loads((tmp_path / "predict.json").read_text())
    assert json.loads((tmp_path / "live.json").read_text()) == want and len(want["activities"]) >= 3
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [e["event"] for e in lines] == ["start", "end"] * len(want["activities"])
