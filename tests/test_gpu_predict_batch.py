"""Many clips in one call (include/savad.h: savad_gather_windows_batch, savad_boost_batch, savad_predict_probabilities_batch; the module's
predict_windows_batch, the predictor's predict_probabilities_many / predict_many / batch_chunks) on ONE clip set:

    L = [1022, 39, 0, 38, 5, 2100, 40, 1] frames -- two reference-run goldens (g5, g5b) and the one-window golden (g5c), an empty clip,
    clips too short for a window (38, 5, 1), a clip of two windows: 3049 windows in all at the reference geometry (half 19, jump 9),

run with chunk 16384 (every clip in one forward), 1000 (chunk cuts inside clips, chunks that span clips) and 8 (chunks smaller than
the gaps between clips)."""
import ctypes

import numpy as np
import pytest

from tests.buffer_arena import BufferArena, same_bits
from tests.test_gpu_schedule_workspace import Knobs, guarded_call, ptr

pytestmark = pytest.mark.gpu

L = [1022, 39, 0, 38, 5, 2100, 40, 1]
SEEDS = [500, 502, None, 503, 504, 501, 505, 506]   # clips 0, 1, 5: the features of the goldens g5, g5c, g5b
GOLDEN = {0: "g5", 1: "g5c", 5: "g5b"}
CHUNKS = [16384, 1000, 8]
PRECISIONS = ["fp32", "fp32s", "bf16"]
TIGHT, BF16_PROBS = 3e-5, 6e-3   # the predictor-level tolerances of tests/test_gpu_parity.py
HALF, JUMP, W = 19, 9, 7


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


def clip_features(F=80):
    from voice_activity_detection_amd.seeded import seeded_features

    return [seeded_features(seed, (n, F)) if n else np.zeros((0, F), np.float32) for seed, n in zip(SEEDS, L)]


@pytest.fixture(scope="module")
def clips():
    """the clips' features, their table and the concatenated matrix (host); computed once, never written"""
    from voice_activity_detection_amd.clips import clip_table

    per_clip = clip_features()
    return {"features": per_clip, "table": clip_table(L), "matrix": np.concatenate(per_clip)}


@pytest.fixture(scope="module")
def oracle_per_clip(state1234, clips):
    """oracle.predict_probabilities of every clip ALONE: (probs [N_c, 7], mean [N_c])"""
    from oracle import oracle

    return [oracle.predict_probabilities(state1234, f) if len(f) else (np.zeros((0, W), np.float32), np.zeros((0,), np.float32))
            for f in clips["features"]]


def stream_(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    from voice_activity_detection_amd import _lib

    _lib.check(rc)


def host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def plan_chunk(chunk, items):
    """the chunk rule of the schedule: even, at most the item count"""
    even = chunk + chunk % 2
    return even if even <= items else max(items, 1)


def gather_batch(torch, lib, feature, table, half, jump, first, count, positions=True):
    F = feature.shape[1]
    Wn = lib.savad_window_offsets(half, jump, None)
    table_dev = torch.from_numpy(table).cuda()
    items_first = torch.empty(len(table), dtype=torch.int32, device="cuda")
    win = torch.empty((count, Wn, F), dtype=torch.float32, device="cuda")
    pos = torch.empty((count, Wn), dtype=torch.int64, device="cuda") if positions else None
    ok(lib.savad_gather_windows_batch(ptr(feature), host_ptr(table), ptr(table_dev), len(table) - 1, F, half, jump, first, count,
                                      ptr(items_first), ptr(win), ptr(pos) if positions else None, stream_(torch)))
    return win, pos, items_first


def boost_batch(torch, lib, logp, table, half, jump):
    Wn = lib.savad_window_offsets(half, jump, None)
    rows = int(table[-1])
    table_dev = torch.from_numpy(table).cuda()
    items_first = torch.empty(len(table), dtype=torch.int32, device="cuda")
    probs = torch.empty((rows, Wn), dtype=torch.float32, device="cuda")
    mean = torch.empty((rows,), dtype=torch.float32, device="cuda")
    ok(lib.savad_boost_batch(ptr(logp), host_ptr(table), ptr(table_dev), len(table) - 1, half, jump, ptr(items_first), ptr(probs), ptr(mean),
                             stream_(torch)))
    return probs, mean


# ---- 1. the gather against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half,jump", [(19, 9), (5, 1), (16, 1)])     # W = 7, 11 and 33 (more frames than a tile has items)
@pytest.mark.parametrize("F", [80, 13])
def test_gather_matches_the_oracle_per_clip(torch_cuda, lib, half, jump, F):
    from oracle import oracle
    from voice_activity_detection_amd.clips import clip_table, window_items

    torch = torch_cuda
    per_clip, table = clip_features(F), clip_table(L)
    items_first = window_items(table, half)
    wins, poss = [], []
    for c, f in enumerate(per_clip):
        n_c = int(items_first[c + 1] - items_first[c])
        assert n_c == max(0, len(f) - 2 * half)
        if n_c:
            w, p = oracle.gather_windows(f, half, jump, 0, n_c)
            wins.append(w)
            poss.append(p + int(table[c]))          # the clip's positions plus clip_first[c]: rows of the concatenated matrix
    want_win, want_pos = np.concatenate(wins), np.concatenate(poss)
    total = int(items_first[-1])
    assert len(want_win) == total and (half != 19 or total == 3049)
    feature = torch.from_numpy(np.concatenate(per_clip)).cuda()
    win, pos, got_first = gather_batch(torch, lib, feature, table, half, jump, 0, total)
    torch.cuda.synchronize()
    assert np.array_equal(got_first.cpu().numpy(), items_first)                     # the scan the call left behind
    assert np.array_equal(win.cpu().numpy(), want_win) and np.array_equal(pos.cpu().numpy(), want_pos)
    # a sub-range that starts inside clip 0, crosses the short and empty clips and ends inside clip 5; and one without positions
    first, count = int(items_first[1]) - 77, 77 + int(items_first[5] - items_first[1]) + 333
    for with_positions in (True, False):
        win, pos, _ = gather_batch(torch, lib, feature, table, half, jump, first, count, with_positions)
        torch.cuda.synchronize()
        assert np.array_equal(win.cpu().numpy(), want_win[first:first + count])
        assert not with_positions or np.array_equal(pos.cpu().numpy(), want_pos[first:first + count])
    win, _, _ = gather_batch(torch, lib, feature, table, half, jump, total - 1, 1)   # the last item alone: clip 6's second window
    assert np.array_equal(win.cpu().numpy(), want_win[-1:])
    # one clip runs the same tile kernel (savad_gather_windows): the indexing rule feature[half + first + item + off[w]], positions
    # included, at the edges of a 32-item tile, on a matrix that ends with the last window's last frame
    off = oracle.window_offsets(half, jump)
    rows = np.concatenate(per_clip)
    for first in (0, 5):
        for count in (1, 31, 32, 33):
            N = 2 * half + first + count
            one = torch.from_numpy(rows[:N].copy()).cuda()
            win = torch.empty((count, len(off), F), dtype=torch.float32, device="cuda")
            pos = torch.empty((count, len(off)), dtype=torch.int64, device="cuda")
            ok(lib.savad_gather_windows(ptr(one), N, F, half, jump, first, count, ptr(win), ptr(pos), stream_(torch)))
            want = half + first + np.arange(count)[:, None] + off[None, :]
            assert want.min() == first and want[-1, -1] == N - 1
            assert np.array_equal(pos.cpu().numpy(), want) and np.array_equal(win.cpu().numpy(), rows[want]), (first, count)


# ---- 2. the boost against the existing path --------------------------------------------------------------------------------------

def test_boost_matches_savad_boost_per_clip(torch_cuda, lib):
    from oracle import oracle
    from voice_activity_detection_amd.clips import clip_table, window_items

    torch = torch_cuda
    table = clip_table(L)
    items_first = window_items(table, HALF)
    total = int(items_first[-1])
    logp_np = np.log(np.random.default_rng(7).dirichlet([1, 1], size=(total, W))).astype(np.float32)
    logp = torch.from_numpy(logp_np).cuda()
    probs, mean = boost_batch(torch, lib, logp, table, HALF, JUMP)
    torch.cuda.synchronize()
    dummy = np.zeros((1, 80), np.float32)
    for c, N in enumerate(L):
        a, b, i0, i1 = int(table[c]), int(table[c + 1]), int(items_first[c]), int(items_first[c + 1])
        if N == 0:
            continue
        n_c = i1 - i0
        pos = oracle.gather_windows(np.repeat(dummy, N, axis=0), HALF, JUMP, 0, n_c)[1] if n_c else np.zeros((0, W), np.int64)
        # the existing entry on this clip alone, on the GPU
        want_probs, want_mean = torch.empty((N, W), device="cuda"), torch.empty((N,), device="cuda")
        d_pos = torch.from_numpy(pos).cuda()
        ok(lib.savad_boost(ptr(logp[i0:i1].contiguous()) if n_c else None, ptr(d_pos) if n_c else None, n_c, N, W,
                           ptr(torch.empty((N, W, 2), device="cuda")), ptr(want_probs), ptr(want_mean), stream_(torch)))
        torch.cuda.synchronize()
        assert torch.equal(probs[a:b], want_probs) and torch.equal(mean[a:b], want_mean), c
        ref_probs, ref_mean = oracle.boost(logp_np[i0:i1], pos, N)
        got = probs[a:b].cpu().numpy()
        assert np.abs(got - ref_probs).max() < 2e-7 and np.abs(mean[a:b].cpu().numpy() - ref_mean).max() < 2e-7   # device expf vs libm
        assert np.array_equal(got == 0.5, ref_probs == 0.5), c        # the placeholders sit exactly where the oracle leaves them
        if n_c == 0:
            assert (got == 0.5).all()


# ---- 3. / 4. the one call against the entry points step by step ------------------------------------------------------------------

def stepwise_batch(torch, lib, model, feature, table, chunk):
    """savad_gather_windows_batch + savad_forward per chunk + savad_boost_batch, at the one call's chunking"""
    from voice_activity_detection_amd.clips import window_items

    total = int(window_items(table, HALF)[-1])
    step = plan_chunk(chunk, total)
    logp = torch.empty((total, W, 2), dtype=torch.float32, device="cuda")
    with torch.no_grad():
        for first in range(0, total, step):
            count = min(step, total - first)
            win, _, _ = gather_batch(torch, lib, feature, table, HALF, JUMP, first, count, positions=False)
            model(features=win, out=logp[first:first + count])
    return boost_batch(torch, lib, logp, table, HALF, JUMP)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_call_matches_the_stepwise_batch(torch_cuda, lib, model, clips, precision, chunk):
    torch = torch_cuda
    feature = torch.from_numpy(clips["matrix"]).cuda()
    with Knobs(model, precision, 0):
        p1, m1 = model.predict_windows_batch(feature, clips["table"], HALF, JUMP, chunk)
        p0, m0 = stepwise_batch(torch, lib, model, feature, clips["table"], chunk)
        torch.cuda.synchronize()
    assert p1.shape == (sum(L), W) and m1.shape == (sum(L),)
    assert torch.equal(p1, p0) and torch.equal(m1, m0)


@pytest.mark.parametrize("N", [1022, 39, 38, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_clip_table_is_the_stepwise_predictor(torch_cuda, model, precision, N):
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.seeded import seeded_features

    torch = torch_cuda
    feature = torch.from_numpy(seeded_features(900 + N, (N, 80))).cuda()
    pred = VADFromScratchPredictor(model, "cuda")
    with Knobs(model, precision, 0):
        (p1, m1), = pred.predict_probabilities_many([feature])
        p0, m0 = pred.predict_probabilities_device_stepwise(feature)
        torch.cuda.synchronize()
    assert p1.shape == (N, W) and torch.equal(p1, p0) and torch.equal(m1, m0)


# ---- 5. / 6. goldens of the reference and the oracle, clip by clip ---------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_results(torch_cuda, model, clips):
    """(precision, chunk) -> the one call's (probs, mean) per clip, on the host; each computed once"""
    from voice_activity_detection_amd.clips import split_by_clip

    torch = torch_cuda
    feature = torch.from_numpy(clips["matrix"]).cuda()
    done = {}

    def get(precision, chunk):
        if (precision, chunk) not in done:
            with Knobs(model, precision, 0):
                probs, mean = model.predict_windows_batch(feature, clips["table"], HALF, JUMP, chunk)
                torch.cuda.synchronize()
            done[precision, chunk] = (split_by_clip(probs.cpu().numpy(), clips["table"]), split_by_clip(mean.cpu().numpy(), clips["table"]))
        return done[precision, chunk]

    return get


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_clips_match_the_reference_goldens(batch_results, golden, precision, chunk):
    probs, mean = batch_results(precision, chunk)
    tol = BF16_PROBS if precision == "bf16" else TIGHT
    for c, tag in GOLDEN.items():
        want = golden[f"{tag}_probs"]
        assert probs[c].shape == want.shape and probs[c].dtype == np.float32
        assert np.abs(probs[c] - want).max() < tol, (tag, np.abs(probs[c] - want).max())
        assert np.abs(mean[c] - golden[f"{tag}_mean"]).max() < tol, tag
        assert np.array_equal(probs[c] == 0.5, want == 0.5), tag      # every placeholder where the reference leaves it, and no other


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_clip_matches_the_oracle_alone(batch_results, oracle_per_clip, precision, chunk):
    probs, mean = batch_results(precision, chunk)
    tol = BF16_PROBS if precision == "bf16" else TIGHT
    assert [len(p) for p in probs] == L
    for c, (want_probs, want_mean) in enumerate(oracle_per_clip):
        if L[c] == 0:
            continue
        assert np.abs(probs[c] - want_probs).max() < tol, (c, np.abs(probs[c] - want_probs).max())
        assert np.abs(mean[c] - want_mean).max() < tol, c
        assert np.array_equal(probs[c] == 0.5, want_probs == 0.5), c
        if L[c] <= 2 * HALF:
            assert (probs[c] == 0.5).all() and (mean[c] == 0.5).all()      # no window: nothing but placeholders


def test_library_refuses_a_table_that_is_none(torch_cuda, lib, model, clips):
    """the handle's entries: refused from the host table, before any launch (NULL device pointers would fault otherwise)"""
    torch = torch_cuda
    dev = torch.device("cuda", torch.cuda.current_device())
    model._prepare_call(dev)
    n = ctypes.c_size_t()
    bad = np.array([0, 50, 49], dtype=np.int32)
    assert lib.savad_predict_batch_workspace_bytes(model._handle, host_ptr(bad), 2, HALF, JUMP, 1000, ctypes.byref(n)) == -1
    assert b"decrease" in lib.savad_last_error()
    assert lib.savad_predict_probabilities_batch(model._handle, None, host_ptr(bad), None, 2, HALF, JUMP, 1000, None, None, None, 0, None) == -1
    big = np.array([0, 2 ** 31 - 1], dtype=np.int32)
    assert lib.savad_predict_batch_workspace_bytes(model._handle, host_ptr(big), 1, HALF, JUMP, 1000, ctypes.byref(n)) == -2
    assert lib.savad_predict_batch_workspace_bytes(model._handle, host_ptr(clips["table"]), len(L), 40, 1, 1000, ctypes.byref(n)) == -2   # W = 81
    assert lib.savad_predict_batch_workspace_bytes(model._handle, host_ptr(clips["table"]), 0, HALF, JUMP, 1000, ctypes.byref(n)) == -1
    with pytest.raises(ValueError):
        model.predict_windows_batch(torch.zeros((10, 80), device="cuda"), [0, 4, 9], HALF, JUMP, 1000)   # the table ends off the matrix
    with pytest.raises(ValueError):
        model.predict_windows_batch(torch.zeros((10, 80), device="cuda"), [0, 7, 4, 10], HALF, JUMP, 1000)


# ---- 7. predict_many and predict(batch_chunks=True) on the committed recording ---------------------------------------------------

@pytest.fixture(scope="module")
def recording(state1234):
    """the committed wav, its chunks at split_max_seconds = 2, and a threshold at least 1e-3 away from every boosted probability the
    CPU oracle gives for those chunks: no frame can change sides between two paths that agree to 2e-6"""
    from pathlib import Path

    from oracle import logmel, oracle
    from voice_activity_detection_amd.clips import chunk_bounds
    from voice_activity_detection_amd.features import load_wav_mono16k

    audio = load_wav_mono16k(Path(__file__).resolve().parent / "golden" / "data" / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav")
    _, bounds = chunk_bounds(len(audio), 16000, 2)
    assert len(bounds) == 6
    boosted = np.concatenate([oracle.predict_probabilities(state1234, logmel.log_mel(audio[a:b]))[1] for a, b in bounds]).astype(np.float64)
    values = np.unique(boosted)
    gaps = np.diff(values)
    above = np.array([(boosted > v).sum() for v in values[:-1]])
    wide = np.flatnonzero(gaps >= 2e-3)                       # (a midpoint of such a gap is 1e-3 from both sides)
    assert wide.size, "no gap of 2e-3 between the oracle's boosted probabilities"
    k = wide[np.argmin(np.abs(above[wide] - len(boosted) / 2))]   # ... the one that splits the frames most evenly
    threshold = float(0.5 * (values[k] + values[k + 1]))
    assert np.abs(boosted - threshold).min() >= 1e-3, np.abs(boosted - threshold).min()
    assert 0 < (boosted > threshold).sum() < len(boosted)     # a threshold that separates something
    return audio, bounds, threshold


@pytest.mark.parametrize("device_post", [False, True])
def test_predict_many_and_batch_chunks_on_the_committed_wav(torch_cuda, model, recording, device_post):
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.predictor import VADPredictParameters

    torch = torch_cuda
    audio, bounds, threshold = recording
    params = VADPredictParameters(split_max_seconds=2, threshold=threshold, min_vally_ms=10, min_hill_ms=10, hang_before_ms=10, hang_over_ms=10)
    looped = VADFromScratchPredictor(model, "cuda", device_post=device_post)
    batched = VADFromScratchPredictor(model, "cuda", device_post=device_post, batch_chunks=True)
    # the probabilities of the six chunks: one call against the loop
    feats = [looped.features(audio[a:b]) for a, b in bounds]
    many = batched.predict_probabilities_many(feats)
    assert len(many) == 6
    for f, (p1, m1) in zip(feats, many):
        p0, m0 = looped.predict_probabilities_device(f)
        assert p1.shape == p0.shape and float((p1 - p0).abs().max()) <= 2e-6 and float((m1 - m0).abs().max()) <= 2e-6
        assert torch.equal(p1 == 0.5, p0 == 0.5)
    want = looped.predict(audio, params)
    assert len(want.activities) >= 1
    assert batched.predict(audio, params) == want                                  # the flag: the chunks of one recording
    assert looped.predict_many([audio], params) == [want]                          # the method itself needs no flag
    pieces = [audio[a:b] for a, b in bounds]
    single = VADPredictParameters(None, threshold, 10, 10, 10, 10)
    assert looped.predict_many(pieces + [audio], single) == [looped.predict(p, single) for p in pieces] + [looped.predict(audio, single)]
    stats = batched.post_stats
    assert stats["device" if device_post else "host"] == 6 and stats["host" if device_post else "device"] == 0
    assert looped.predict_many([], params) == []


# ---- 8. caller buffers -----------------------------------------------------------------------------------------------------------

def out_f32(arena, shape, align, name):
    import torch

    return arena.place_output(4 * int(np.prod(shape)), align, torch.float32, name).view(shape)


@pytest.mark.parametrize("F", [80, 13])
def test_gather_batch_stays_inside_its_buffers(torch_cuda, lib, F):
    from voice_activity_detection_amd.clips import clip_table, window_items

    torch = torch_cuda
    table = clip_table(L)
    items_first = window_items(table, HALF)
    feature = torch.from_numpy(np.concatenate(clip_features(F))).cuda()
    fal = 16 if F % 4 == 0 else 4
    # the whole set at F = 13; at F = 80 the items around the short clips (the end of clip 0 up to the start of clip 5) and the tail
    ranges = [(0, 3049)] if F == 13 else [(900, 300), (3049 - 45, 45)]
    for first, count in ranges:
        want, want_pos, want_first = gather_batch(torch, lib, feature, table, HALF, JUMP, first, count)
        arena = BufferArena("cuda", 4 << 20)
        fa = arena.place_input(feature, fal, "feature")
        ta = arena.place_input(torch.from_numpy(table), 4, "clip_first")
        first_out = arena.place_output(4 * len(table), 4, torch.int32, "items_first")
        win = out_f32(arena, (count, W, F), fal, "windows")
        pos = arena.place_output(8 * count * W, 8, torch.int64, "positions").view(count, W)
        ok(lib.savad_gather_windows_batch(ptr(fa), host_ptr(table), ptr(ta), len(L), F, HALF, JUMP, first, count, ptr(first_out), ptr(win),
                                          ptr(pos), stream_(torch)))
        arena.check()
        assert same_bits(win, want) and same_bits(pos, want_pos) and same_bits(first_out, want_first)
        assert np.array_equal(first_out.cpu().numpy(), items_first)


def test_boost_batch_stays_inside_its_buffers(torch_cuda, lib):
    from voice_activity_detection_amd.clips import clip_table

    torch = torch_cuda
    table = clip_table(L)
    logp = torch.from_numpy(np.log(np.random.default_rng(8).dirichlet([1, 1], size=(3049, W))).astype(np.float32)).cuda()
    want_probs, want_mean = boost_batch(torch, lib, logp, table, HALF, JUMP)
    arena = BufferArena("cuda", 1 << 20)
    la = arena.place_input(logp, 8, "logp")
    ta = arena.place_input(torch.from_numpy(table), 4, "clip_first")
    first_out = arena.place_output(4 * len(table), 4, torch.int32, "items_first")
    probs, mean = out_f32(arena, (sum(L), W), 4, "probs"), out_f32(arena, (sum(L),), 4, "mean")
    ok(lib.savad_boost_batch(ptr(la), host_ptr(table), ptr(ta), len(L), HALF, JUMP, ptr(first_out), ptr(probs), ptr(mean), stream_(torch)))
    arena.check()
    assert same_bits(probs, want_probs) and same_bits(mean, want_mean)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict_batch_stays_inside_its_buffers_and_its_workspace(torch_cuda, model, clips, precision, chunk):
    """feature, table, probs and mean between guards, the workspace exactly as large as savad_predict_batch_workspace_bytes reports"""
    torch = torch_cuda
    table = clips["table"]
    feature = torch.from_numpy(clips["matrix"]).cuda()
    with Knobs(model, precision, 0):
        want_probs, want_mean = model.predict_windows_batch(feature, table, HALF, JUMP, chunk)
        arena = BufferArena("cuda", 2 << 20)
        fa = arena.place_input(feature, 16, "feature")
        ta = arena.place_input(torch.from_numpy(table), 4, "clip_first")
        probs, mean = out_f32(arena, (sum(L), W), 4, "probs"), out_f32(arena, (sum(L),), 4, "mean")
        guarded_call(torch, model,
                     lambda lib, h, nb: lib.savad_predict_batch_workspace_bytes(h, host_ptr(table), len(L), HALF, JUMP, chunk, nb),
                     lambda lib, h, ws, n, st: lib.savad_predict_probabilities_batch(h, ptr(fa), host_ptr(table), ptr(ta), len(L), HALF, JUMP, chunk,
                                                                                     ptr(probs), ptr(mean), ws, n, st))
    arena.check()
    assert same_bits(probs, want_probs) and same_bits(mean, want_mean)
