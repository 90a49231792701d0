"""Live sessions on the GPU (include/savad.h: savad_live_*; voice_activity_detection_amd/live.py): what comes out chunk by chunk is the
offline result of the finished recording, row for row.

Streams: 300 samples (N = 2: placeholders only), 6 250 (N = 40: one window), 6 720 (N = 43: 5 windows, a stream's run of windows crosses
a packed-block boundary), 16 001 and 37 333.  Chunkings: (a) one push then finish, (b) 1 600 samples per tick, (c) the irregular
sequence 1, 159, 160, 161, 0, 4 000, 7, 255, 257 repeating, (d) three slots for the five recordings: streams open late, finish early
(in a tick in which others push) and every slot is used again."""
import ctypes

import numpy as np
import pytest

from tests.buffer_arena import BufferArena, same_bits
from tests.test_gpu_schedule_workspace import Knobs, ptr
from tests.test_live_host import IRREGULAR
from tests.test_live_host import test_library_refuses_before_launch as abi_refusals

pytestmark = pytest.mark.gpu

TOTALS = [300, 6250, 6720, 16001, 37333]
HALF, JUMP, W = 19, 9, 7
# kernel variants that include/savad.h states deterministic and independent of the batch
PINNED = [("fp32", 4), ("fp32s", 8), ("fp32s", 5), ("bf16", 8), ("bf16", 5)]
FP32_BATCH, BF16_BATCH = 2e-6, 1e-2    # tests/test_gpu_parity.py: offline paths whose batches differ
ORACLE_FP32, BF16_PROBS = 1e-4, 6e-3   # test_config1_reference_clip_end_to_end; tests/test_gpu_predict_batch.py


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


def make_signals():
    """seeded noise plus a chirp, one per total; never written (tests/test_gpu_window_geometry.py runs two of them at other geometries)"""
    out = []
    for k, n in enumerate(TOTALS):
        t = np.arange(n, dtype=np.float64) / 16000.0
        chirp = 0.2 * np.sin(2 * np.pi * (200.0 + 900.0 * t) * t)
        out.append((np.random.default_rng(40 + k).standard_normal(n) * 0.05 + chirp).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def signals():
    return make_signals()


def cut(total, sizes):
    seq, left, k = [], total, 0
    while left > 0:
        c = min(sizes[k % len(sizes)], left)
        seq.append(c)
        left -= c
        k += 1
    return seq


def chunking(name, total):
    return {"a": [total], "b": cut(total, [1600]), "c": cut(total, IRREGULAR), "d": cut(total, [1600])}[name]


def run_live(torch, model, signals, name, dtype=np.float32, context=None):
    """every recording through one LiveVAD under chunking `name` -> [(probs, mean)] on the host, in recording order.
    `context` (ContextResolution; None = the shipped 19 / 9): the session's window geometry, whose W the rows must have"""
    from voice_activity_detection_amd import LiveVAD

    cuts = [chunking(name, len(s)) for s in signals]
    slots_n = 3 if name == "d" else len(signals)
    vad = LiveVAD(model, "cuda", streams=slots_n, max_push_samples=max(max(c) for c in cuts), context=context)
    W = vad.W
    assert W == 7 or context is not None
    waiting = list(range(len(signals)))
    active = {}    # slot -> [recording, next chunk index, samples pushed]
    got = [[] for _ in signals]
    rows = [0] * len(signals)
    tick_no = 0
    while waiting or active:
        # (d): at most one stream opens per tick, so the streams are out of step with each other
        while waiting and len(active) < slots_n:
            active[vad.open()] = [waiting.pop(0), 0, 0]
            if name == "d":
                break
        chunks, ending = {}, []
        for slot, st in active.items():
            rec, k, at = st
            c = cuts[rec][k]
            piece = signals[rec][at:at + c]
            if dtype is np.int16:
                piece = np.round(piece * 32768.0).astype(np.int16)
            elif (tick_no + slot) % 3 == 0:
                piece = torch.from_numpy(piece).cuda()        # a device chunk now and then
            chunks[slot] = piece
            st[1], st[2] = k + 1, at + c
            if st[1] == len(cuts[rec]) and name == "d":
                ending.append(slot)                            # (d): the last chunk and the finish share a tick with the others' pushes
        tick = vad.step(chunks, ending)
        for slot in list(active):
            rec = active[slot][0]
            first, probs, mean = tick[slot]
            assert first == rows[rec] and probs.shape == (mean.shape[0], W)
            rows[rec] += probs.shape[0]
            got[rec].append((probs, mean))
            if slot in ending:
                del active[slot]
        done = [slot for slot, st in active.items() if st[1] == len(cuts[st[0]])]
        if done:                                               # (a) - (c): the finish is a tick of its own
            tick = vad.finish(done)
            for slot in done:
                rec = active.pop(slot)[0]
                first, probs, mean = tick[slot]
                assert first == rows[rec]
                rows[rec] += probs.shape[0]
                got[rec].append((probs, mean))
        tick_no += 1
    out = []
    for rec, parts in enumerate(got):
        probs = torch.cat([p for p, _ in parts]).cpu().numpy()
        mean = torch.cat([m for _, m in parts]).cpu().numpy()
        assert probs.shape == (1 + len(signals[rec]) // 160, W)
        out.append((probs, mean))
    return out


# ---- 1. stages, bits ---------------------------------------------------------------------------------------------------------------

class Entry(ctypes.Structure):   # csrc/savad_live_plan.h: Entry
    _fields_ = ([(n, ctypes.c_int32) for n in ("slot", "finish", "dtype", "push")] +
                [(n, ctypes.c_uint64) for n in ("src", "buf_old", "buf_new", "head", "tail", "feat", "logp")] +
                [(n, ctypes.c_int64) for n in ("n_before", "n_after", "base_before", "base_after", "tail_j0")] +
                [(n, ctypes.c_int32) for n in ("keep_off", "keep_count", "head_write", "tail_count", "frame_first_mod", "n_frames", "win_first_mod",
                                               "n_windows", "win_kept", "item0", "row_count", "row_out")] +
                [("row_first", ctypes.c_int64), ("phase_after", ctypes.c_int32), ("pad", ctypes.c_int32)])


def run_stages(torch, lib, model, audio, sizes, sub_ranges=False):
    """One stream in slot 1 of 2, every stage entry called by hand; every stage's output compared with the offline entry's bits.
    sub_ranges: the gather also runs over items [first, first + count) at the edges of its 32-item tiles, and `seen` counts the
    ticks whose first 32 items have the feature ring's wrap between their centres."""
    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.features import log_mel

    ok = _lib.check
    n_total = len(audio)
    N = 1 + n_total // 160
    max_push = max(sizes)
    cfg = _lib.savad_live_config(2, max_push, HALF, JUMP, 1024)
    feat_cap = 2 * HALF + max_push // 160 + 3
    nbytes = ctypes.c_size_t()
    ok(lib.savad_live_state_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)))
    state = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    ok(lib.savad_live_table_bytes(ctypes.byref(cfg), 1, ctypes.byref(nbytes)))
    table = np.zeros(nbytes.value, dtype=np.uint8)
    slots = (_lib.savad_live_slot * 2)()
    ok(lib.savad_live_open(ctypes.byref(cfg), slots, 1))
    full = log_mel(audio, "cuda")                                   # the finished recording's features
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    live_rows, all_logp, seen = [], [], {"one_frame": 0, "tiles": 0, "frames": 0, "windows": 0, "wrapped": 0}
    at = 0
    for size, last in [(s, False) for s in sizes] + [(0, True)]:
        chunk = torch.from_numpy(audio[at:at + size].copy()).cuda() if size else None
        at += size
        push = (_lib.savad_live_push * 1)(_lib.savad_live_push(1, size, 1, int(last), chunk.data_ptr() if size else None))
        counts = _lib.savad_live_counts()
        ok(lib.savad_live_plan(ctypes.byref(cfg), slots, push, 1, ptr(state), ctypes.c_void_p(table.ctypes.data), table.size, ctypes.byref(counts), None))
        table_dev = torch.from_numpy(table).cuda()
        host = ctypes.c_void_p(table.ctypes.data)
        e = Entry.from_buffer_copy(table[64:64 + ctypes.sizeof(Entry)].tobytes())
        ok(lib.savad_live_append(ctypes.byref(cfg), host, ptr(table_dev), stream))
        ok(lib.savad_live_logmel(ctypes.byref(cfg), host, ptr(table_dev), stream))
        # the new rows of the feature ring = rows of log_mel(whole signal)
        ring = state[e.feat - state.data_ptr():][:feat_cap * 320].view(torch.float32).view(feat_cap, 80)
        K0 = seen["frames"]
        if e.n_frames:
            pos = [(K0 + k) % feat_cap for k in range(e.n_frames)]
            assert same_bits(ring[pos], full[K0:K0 + e.n_frames]), (K0, e.n_frames)
        seen["frames"] += e.n_frames
        seen["tiles"] += counts.tiles
        seen["one_frame"] += e.n_frames == 1
        logp = None
        if counts.items:
            win = torch.empty((counts.items, W, 80), dtype=torch.float32, device="cuda")
            ok(lib.savad_live_gather(ctypes.byref(cfg), host, ptr(table_dev), 0, counts.items, ptr(win), stream))
            E0 = seen["windows"]
            want = torch.empty((e.n_windows, W, 80), dtype=torch.float32, device="cuda")
            ok(lib.savad_gather_windows(ptr(full), N, 80, HALF, JUMP, E0, e.n_windows, ptr(want), None, stream))
            assert e.item0 % 4 == E0 % 4 and same_bits(win[e.item0:e.item0 + e.n_windows], want)
            dummies = torch.cat([win[:e.item0], win[e.item0 + e.n_windows:]])
            assert not dummies.any()
            if sub_ranges:
                centre0 = (E0 + HALF) % feat_cap - e.item0        # ring position item 0 would have: item i sits at centre0 + i, modulo the ring
                seen["wrapped"] += counts.items >= 33 and centre0 + e.item0 < feat_cap <= centre0 + 31
                for first in (0, 5):
                    for count in (1, 31, 32, 33):
                        if first + count <= counts.items:
                            part = torch.empty((count, W, 80), dtype=torch.float32, device="cuda")
                            ok(lib.savad_live_gather(ctypes.byref(cfg), host, ptr(table_dev), first, count, ptr(part), stream))
                            assert same_bits(part, win[first:first + count]), (first, count)
            logp = model(features=win)
            all_logp.append(logp[e.item0:e.item0 + e.n_windows])
            seen["windows"] += e.n_windows
        probs = torch.empty((counts.rows, W), dtype=torch.float32, device="cuda")
        mean = torch.empty((counts.rows,), dtype=torch.float32, device="cuda")
        ok(lib.savad_live_boost(ctypes.byref(cfg), host, ptr(table_dev), ptr(logp) if logp is not None else None, ptr(probs), ptr(mean), stream))
        live_rows.append((probs, mean))
        torch.cuda.synchronize()
        ok(lib.savad_live_commit(ctypes.byref(cfg), host, slots))
    assert seen["frames"] == N and seen["windows"] == max(0, N - 2 * HALF) and not slots[1].open
    # the boost: savad_boost_batch of the same log-probs as one clip
    clip = np.array([0, N], dtype=np.int32)
    clip_dev = torch.from_numpy(clip).cuda()
    items_first = torch.empty(2, dtype=torch.int32, device="cuda")
    want_p = torch.empty((N, W), dtype=torch.float32, device="cuda")
    want_m = torch.empty((N,), dtype=torch.float32, device="cuda")
    logp = torch.cat(all_logp) if all_logp else None
    ok(lib.savad_boost_batch(ptr(logp) if logp is not None else None, ctypes.c_void_p(clip.ctypes.data), ptr(clip_dev), 1, HALF, JUMP,
                             ptr(items_first), ptr(want_p), ptr(want_m), stream))
    assert same_bits(torch.cat([p for p, _ in live_rows]), want_p) and same_bits(torch.cat([m for _, m in live_rows]), want_m)
    return seen


@pytest.mark.parametrize("name", ["b", "c"])
def test_stages_have_the_offline_bits(torch_cuda, lib, model, signals, name):
    one_frame = 0
    for audio in signals:
        seen = run_stages(torch_cuda, lib, model, audio, chunking(name, len(audio)))
        one_frame += seen["one_frame"]
    if name == "c":
        assert one_frame > 0   # a tile with one frame (the 160-sample pushes)


def test_stages_many_tiles_in_one_tick(torch_cuda, lib, model, signals):
    """one push of the whole 37 333 samples: interior tiles, tiles cut at the ring's wrap, and the finish tile"""
    seen = run_stages(torch_cuda, lib, model, signals[4], [len(signals[4])])
    assert seen["tiles"] >= 8


def test_gather_tile_edges_with_the_ring_wrap_inside(torch_cuda, lib, model, signals):
    """pushes of 6000 samples: 37 or 38 windows a tick (more than the gather's 32-item tile) in a ring of 78 rows, so the wrap falls
    between the centres of a tick's first tile again and again; savad_live_gather over 1, 31, 32 and 33 items from item 0 and from
    item 5 gives the rows of the whole-tick gather, which run_stages holds to the offline gather's bits"""
    n = len(signals[4])
    seen = run_stages(torch_cuda, lib, model, signals[4], [6000] * (n // 6000) + [n % 6000], sub_ranges=True)
    assert seen["wrapped"] >= 1


# ---- 2. chunking invariance and 3. the offline path, pinned variants: bits ------------------------------------------------------

@pytest.mark.parametrize("precision,row_mode", PINNED)
def test_chunking_invariance_and_offline_bits(torch_cuda, model, signals, precision, row_mode):
    from voice_activity_detection_amd import VADFromScratchPredictor

    with Knobs(model, precision, row_mode):
        runs = {name: run_live(torch_cuda, model, signals, name) for name in "abcd"}
        pred = VADFromScratchPredictor(model, "cuda")
        offline = [tuple(t.cpu().numpy() for t in pred.predict_audio_device(s)) for s in signals]
    for name in "bcd":
        for rec in range(len(signals)):
            assert same_bits(runs[name][rec][0], runs["a"][rec][0]) and same_bits(runs[name][rec][1], runs["a"][rec][1]), (name, rec)
    for rec in range(len(signals)):
        assert same_bits(runs["a"][rec][0], offline[rec][0]) and same_bits(runs["a"][rec][1], offline[rec][1]), rec


# ---- 3. the offline path, automatic schedule on both sides ------------------------------------------------------------------------

@pytest.mark.parametrize("precision,bound", [("fp32", FP32_BATCH), ("fp32s", FP32_BATCH), ("bf16", BF16_BATCH)])
def test_against_the_offline_path(torch_cuda, model, signals, precision, bound):
    from voice_activity_detection_amd import VADFromScratchPredictor

    with Knobs(model, precision, 0):
        live = run_live(torch_cuda, model, signals, "c")
        pred = VADFromScratchPredictor(model, "cuda")
        offline = [tuple(t.cpu().numpy() for t in pred.predict_audio_device(s)) for s in signals]
    for (probs, mean), (want, want_mean) in zip(live, offline):
        assert probs.shape == want.shape and mean.shape == want_mean.shape
        assert np.array_equal(probs == 0.5, want == 0.5)
        err = float(np.abs(probs - want).max()), float(np.abs(mean - want_mean).max())
        print(f"live vs offline ({precision}, N = {len(mean)}): max |dp| = {err[0]:.3e}, max |dmean| = {err[1]:.3e}")
        assert max(err) <= bound
    assert (live[0][0] == 0.5).all()   # N = 2: nothing but placeholders


def test_pcm16_pushes(torch_cuda, model, signals):
    """int16 chunks are converted as savad_pcm16_to_f32 converts them: the offline result of the quantised recording, bit for bit"""
    from voice_activity_detection_amd import VADFromScratchPredictor

    with Knobs(model, "fp32", 4):
        live = run_live(torch_cuda, model, signals[1:4], "c", dtype=np.int16)
        pred = VADFromScratchPredictor(model, "cuda")
        for (probs, mean), s in zip(live, signals[1:4]):
            quantised = (np.round(s * 32768.0).astype(np.int16) / np.float32(32768.0)).astype(np.float32)
            want, want_mean = pred.predict_audio_device(quantised)
            assert same_bits(probs, want) and same_bits(mean, want_mean)


# ---- 4. the oracle ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reference_clip(state1234):
    from pathlib import Path

    from oracle import logmel, oracle
    from voice_activity_detection_amd.features import load_wav_mono16k

    wav = Path(__file__).resolve().parent / "golden" / "data" / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav"
    audio = load_wav_mono16k(wav)
    return audio, oracle.predict_probabilities(state1234, logmel.log_mel(audio))


@pytest.mark.parametrize("precision,bound", [("fp32", ORACLE_FP32), ("fp32s", ORACLE_FP32), ("bf16", BF16_PROBS)])
def test_reference_clip_against_the_oracle(torch_cuda, model, reference_clip, precision, bound):
    audio, (ref_probs, ref_mean) = reference_clip
    with Knobs(model, precision, 0):
        ((probs, mean),) = run_live(torch_cuda, model, [audio], "b")
    err = float(np.abs(probs - ref_probs).max())
    print(f"live vs oracle on the reference clip ({precision}): max |dp| = {err:.3e}")
    assert probs.shape == ref_probs.shape == (1022, 7) and err <= bound
    assert float(np.abs(mean - ref_mean).max()) <= bound


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals(torch_cuda, lib, model):
    from voice_activity_detection_amd import ContextResolution, LiveSession, LiveVAD, VADFromScratchPredictor
    from voice_activity_detection_amd._lib import SavadError
    from voice_activity_detection_amd.features import FrontEnd

    abi_refusals(lib)   # every code of the C ABI, with null device pointers: a launch would fault
    from voice_activity_detection_amd import _lib

    # the step with a real handle: a null device table, then a table whose stream has been closed since it was planned
    cfg = _lib.savad_live_config(2, 1600, HALF, JUMP, 1024)
    slots = (_lib.savad_live_slot * 2)()
    assert lib.savad_live_open(ctypes.byref(cfg), slots, 0) == 0
    table = ctypes.create_string_buffer(1 << 16)
    counts = _lib.savad_live_counts()
    push = (_lib.savad_live_push * 1)(_lib.savad_live_push(0, 1600, 1, 0, 1 << 30))
    assert lib.savad_live_plan(ctypes.byref(cfg), slots, push, 1, ctypes.c_void_p(1 << 20), table, len(table), ctypes.byref(counts), None) == 0
    handle = model._prepare_call(torch_cuda.device("cuda", torch_cuda.cuda.current_device())) and model._handle
    assert lib.savad_live_step(handle, ctypes.byref(cfg), slots, table, None, None, None, None, 0, None) == -1
    assert b"null table" in lib.savad_last_error()
    slots[0].open = 0
    assert lib.savad_live_step(handle, ctypes.byref(cfg), slots, table, ctypes.c_void_p(1 << 20), None, None, None, 0, None) == -1
    assert b"closed" in lib.savad_last_error()
    with pytest.raises(SavadError, match="HIP device"):
        LiveVAD(model, "cpu", 2, 1600)
    with pytest.raises(NotImplementedError, match="16 kHz mono"):
        LiveVAD(model, "cuda", 2, 1600, sample_rate=8000)
    with pytest.raises(NotImplementedError, match="16 kHz mono"):
        LiveVAD(model, "cuda", 2, 1600, channels=2)
    other = VADFromScratchPredictor(model, "cuda", front_end=FrontEnd("log-mel", n_fft=512, hop_ms=10, window_ms=20, n_mels=80))
    with pytest.raises(NotImplementedError, match="shipped"):
        LiveVAD(other, "cuda", 2, 1600)
    with pytest.raises(SavadError, match="64 frames"):
        LiveVAD(model, "cuda", 2, 1600, ContextResolution(200, 1))
    vad = LiveVAD(model, "cuda", 2, 1600)
    a = vad.open()
    with pytest.raises(SavadError, match="1600"):
        vad.push({a: np.zeros(1601, np.float32)})
    with pytest.raises(SavadError, match="maximum"):
        vad.push({a: torch_cuda.zeros(1601, device="cuda")})
    with pytest.raises(SavadError, match="closed"):
        vad.push({1: np.zeros(16, np.float32)})
    with pytest.raises(ValueError):
        vad.push({a: np.zeros((2, 16), np.float32)})
    vad.push({a: np.zeros(100, np.float32)})
    with pytest.raises(SavadError, match="257"):
        vad.finish([a])
    assert vad.samples(a) == 100   # a refused tick changes nothing
    first, probs, mean = vad.finish([a], {a: np.zeros(157, np.int16)})[a]
    assert first == 0 and probs.shape == (2, 7) and bool((probs == 0.5).all()) and vad.open() == a
    session = LiveSession(model, "cuda", 1600)
    assert session.push(np.zeros(1600, np.float32))[1].shape == (0, 7)
    assert session.finish()[1].shape == (11, 7)


# ---- 6. caller's buffers ------------------------------------------------------------------------------------------------------------

def test_tick_stays_inside_the_callers_buffers(torch_cuda, lib, model, signals):
    """One tick (6 720 samples of PCM16 pushed and finished: head and tail mirrors, two tiles, five windows, 43 rows) with state,
    table, samples, workspace and outputs between guards, every buffer at the alignment include/savad.h asks for and no more."""
    from voice_activity_detection_amd import _lib

    torch = torch_cuda
    ok = _lib.check
    audio = np.round(signals[2] * 32768.0).astype(np.int16)
    cfg = _lib.savad_live_config(2, len(audio), HALF, JUMP, 1024)
    dev = torch.device("cuda", torch.cuda.current_device())
    with Knobs(model, "fp32", 4):
        lib = model._prepare_call(dev)
        sizes = {}
        nbytes = ctypes.c_size_t()
        ok(lib.savad_live_state_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)))
        sizes["state"] = nbytes.value
        ok(lib.savad_live_table_bytes(ctypes.byref(cfg), 1, ctypes.byref(nbytes)))
        sizes["table"] = nbytes.value
        ok(lib.savad_live_workspace_bytes(model._handle, ctypes.byref(cfg), 1, ctypes.byref(nbytes)))
        sizes["ws"] = nbytes.value
        arena = BufferArena("cuda", sum(sizes.values()) + 2 * len(audio) + 43 * 8 * 4 + 16 * 4096 + 4096)
        state = arena.place_output(sizes["state"], 16, name="state")
        pcm = arena.place_input(torch.from_numpy(audio), 2, name="samples")
        ws = arena.place_output(sizes["ws"], 16, name="workspace")
        slots = (_lib.savad_live_slot * 2)()
        ok(lib.savad_live_open(ctypes.byref(cfg), slots, 1))
        table = np.zeros(sizes["table"], dtype=np.uint8)
        push = (_lib.savad_live_push * 1)(_lib.savad_live_push(1, len(audio), 0, 1, pcm.data_ptr()))
        counts = _lib.savad_live_counts()
        ok(lib.savad_live_plan(ctypes.byref(cfg), slots, push, 1, ptr(state), ctypes.c_void_p(table.ctypes.data), table.size, ctypes.byref(counts), None))
        assert (counts.rows, counts.tiles, counts.items) == (43, 2, 8)
        table_dev = arena.place_input(torch.from_numpy(table[:counts.table_bytes].copy()), 16, name="table")
        probs = arena.place_output(43 * W * 4, 4, torch.float32, name="probs").view(43, W)
        mean = arena.place_output(43 * 4, 4, torch.float32, name="mean")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ok(lib.savad_live_step(model._handle, ctypes.byref(cfg), slots, ctypes.c_void_p(table.ctypes.data), ptr(table_dev), ptr(probs), ptr(mean),
                               ptr(ws), sizes["ws"], stream))
        arena.check()
        assert not slots[1].open
        ((want, want_mean),) = run_live(torch, model, [signals[2]], "a", dtype=np.int16)
    assert same_bits(probs, want) and same_bits(mean, want_mean)
