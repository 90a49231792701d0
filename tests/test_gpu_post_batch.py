"""The batched device post-processing (savad_post_batch_frames, savad_post_batch_segments; csrc/savad_post_batch.h; the predictor's
`batch_post`) on the GPU: every clip of a batch against post_frames_device + segments_device on that clip ALONE and against the host
functions, integer for integer and bit for bit.  The batches and the planted seams are those of tests/test_post_batch_host.py, which
shows on the CPU that each seam discriminates (a batch path that ignored the clip table would fail here)."""
import ctypes
import dataclasses
import functools
import json

import numpy as np
import pytest

from tests.buffer_arena import BufferArena, same_bits
from tests.test_post_batch_host import GEOMETRY, TRIM, WIDTHS, batches, probs_of, reference_frames, reference_segments
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.clips import clip_table, split_by_clip
from voice_activity_detection_amd.postprocessing import convert_frames_to_samples, optimal_split_voice_activity, segment_indices

pytestmark = pytest.mark.gpu

INVALID = -1
TRIM_KW = dict(zip(("min_vally", "min_hill", "hang_before", "hang_over"), TRIM))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(params=[0, 64], ids=["default block", "block 64"])
def post_block(request):
    """the scans at the default block and at 64 elements per workgroup block (a small batch runs three and more levels)"""
    lib = _lib.load()
    _lib.check(lib.savad_post_set_block(request.param))
    try:
        yield request.param
    finally:
        _lib.check(lib.savad_post_set_block(0))


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()}, strict=True)
    return m.to("cuda").eval()


def stream_(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def alone_on_the_device(name, W):
    """[(boosted, trimmed, starts, ends)] (numpy) of every clip of a batch through the single-clip device calls; computed once per
    batch, never written"""
    import torch

    from voice_activity_detection_amd.postprocessing import post_frames_device, segments_device

    probs, table = batches(W)[name]
    out = []
    for rows in split_by_clip(torch.from_numpy(probs).cuda(), table):
        boosted, trimmed = post_frames_device(rows, 0.5, **TRIM_KW)
        starts, ends = segments_device(trimmed, None, *GEOMETRY)
        out.append((boosted.cpu().numpy(), trimmed.cpu().numpy(), starts, ends))
    return out


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("name", ["lengths", "seams", "one clip", "one empty clip"])
def test_every_clip_is_the_clip_alone(torch_cuda, post_block, name, W):
    from voice_activity_detection_amd.postprocessing import post_frames_device_many, segments_device_many

    torch = torch_cuda
    probs, table = batches(W)[name]
    dev = torch.from_numpy(probs).cuda()
    table_dev = torch.from_numpy(table).cuda()
    boosted, trimmed = post_frames_device_many(dev, table, table_dev, 0.5, **TRIM_KW)
    seg_first, starts, ends = segments_device_many(trimmed, table, table_dev, None, *GEOMETRY)
    assert boosted.shape == trimmed.shape == (len(probs),) and seg_first.shape == (len(table),) and seg_first[0] == 0
    assert seg_first[-1] == len(starts) == len(ends)
    alone, host = alone_on_the_device(name, W), reference_frames(probs, table)
    b_clips, t_clips = split_by_clip(boosted.cpu().numpy(), table), split_by_clip(trimmed.cpu().numpy(), table)
    for c in range(len(table) - 1):
        a, b = int(seg_first[c]), int(seg_first[c + 1])
        for want_b, want_t, want_s, want_e in (alone[c], host[c] + reference_segments(host[c][1])):
            assert np.array_equal(b_clips[c].view(np.uint32), want_b.view(np.uint32)), (name, c)
            assert np.array_equal(t_clips[c], want_t), (name, c)
            assert np.array_equal(starts[a:b], want_s) and np.array_equal(ends[a:b], want_e), (name, c, starts[a:b], want_s, ends[a:b], want_e)
    if name in ("lengths", "seams"):
        assert len(starts) >= 3
    # the table uploaded by the wrapper gives the same
    again = post_frames_device_many(dev, table.tolist(), None, 0.5, **TRIM_KW)
    assert same_bits(again[0], boosted) and same_bits(again[1], trimmed)


def test_other_geometries(torch_cuda, post_block):
    """a window shorter than the hop (samples no frame covers), a hop of one sample with a window of two and a half (a clip's last
    samples), a window below one sample (a clip that is its closing slot alone)"""
    from voice_activity_detection_amd.postprocessing import post_frames_device_many, segments_device_many

    torch = torch_cuda
    probs, table = batches(7)["lengths"]
    boosted, trimmed = post_frames_device_many(torch.from_numpy(probs).cuda(), table, None, 0.5, 2, 2, 1, 1)
    want = reference_frames(probs, table, trim=(2, 2, 1, 1))
    for geometry in [(16000, 10.0, 5.0), (100, 10.0, 25.0), (100, 10.0, 5.0), (8000, 10.0, 25.0)]:
        seg_first, starts, ends = segments_device_many(trimmed, table, None, None, *geometry)
        for c, (_, t) in enumerate(want):
            a, b = int(seg_first[c]), int(seg_first[c + 1])
            s, e = reference_segments(t, geometry)
            assert np.array_equal(starts[a:b], s) and np.array_equal(ends[a:b], e), (geometry, c)


# ---- over-long segments ----------------------------------------------------------------------------------------------------------

SPLIT_SECONDS = 0.125   # 2000 samples: a run of 12 frames and more is over-long
SPLIT_PREDS = [[0] * 5 + [1] * 60 + [0] * 5, [0] * 9 + [1] * 8 + [0] * 9, [], [0] * 30, [1] * 40 + [0] * 3 + [1] * 5 + [0] * 2 + [1] * 30,
               [1], [0] * 3 + [1] * 11 + [0] * 70, [1] * 13]


def split_batch():
    probs = np.concatenate([probs_of(p, 7, 40 + c) for c, p in enumerate(SPLIT_PREDS)])
    return probs, clip_table(len(p) for p in SPLIT_PREDS)


def host_split_reference(probs, table):
    """[(starts, ends, over-long?)] of each clip alone through the host functions, no trim"""
    out = []
    max_samples = int(SPLIT_SECONDS * GEOMETRY[0])
    for boosted, trimmed in reference_frames(probs, table, trim=(0, 0, 0, 0)):
        if len(trimmed) == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64), False))
            continue
        samples = convert_frames_to_samples(trimmed, *GEOMETRY)
        s, e = segment_indices(samples)
        split = optimal_split_voice_activity(samples, convert_frames_to_samples(boosted, *GEOMETRY), SPLIT_SECONDS, GEOMETRY[0])
        out.append(segment_indices(split) + (bool((e + 1 - s > max_samples).any()),))
    return out


def test_over_long_segments_go_through_the_split(torch_cuda, post_block, model):
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters
    from voice_activity_detection_amd.postprocessing import post_frames_device, post_frames_device_many, segments_device, segments_device_many

    torch = torch_cuda
    probs, table = split_batch()
    host = host_split_reference(probs, table)
    flagged = [c for c, (_, _, over) in enumerate(host) if over]
    # the CPU reference: the inputs hold flagged clips and unflagged clips with voice (runs of 60, 40, 30 and 13 frames against 8, 5, 1 and 11)
    assert flagged == [0, 4, 7] and len(flagged) < sum(1 for p in SPLIT_PREDS if 1 in p)
    dev = torch.from_numpy(probs).cuda()
    boosted, trimmed = post_frames_device_many(dev, table, None, 0.5)
    seg_first, starts, ends, flags = segments_device_many(trimmed, table, None, boosted, *GEOMETRY, max_length_seconds=SPLIT_SECONDS, return_long=True)
    assert np.flatnonzero(flags).tolist() == flagged
    for c, rows in enumerate(split_by_clip(dev, table)):
        a, b = int(seg_first[c]), int(seg_first[c + 1])
        b1, t1 = post_frames_device(rows, 0.5)
        s1, e1 = segments_device(t1, b1, *GEOMETRY, max_length_seconds=SPLIT_SECONDS)
        assert np.array_equal(starts[a:b], s1) and np.array_equal(ends[a:b], e1), c
        assert np.array_equal(starts[a:b], host[c][0]) and np.array_equal(ends[a:b], host[c][1]), c
    assert seg_first[-1] == len(starts) > len(segments_device_many(trimmed, table, None, None, *GEOMETRY)[1])   # something was split
    # without a maximum nothing is flagged
    assert not segments_device_many(trimmed, table, None, boosted, *GEOMETRY, return_long=True)[3].any()

    # the predictor: the same chunks through _post_device one by one, and the counters
    params = VADPredictParameters(threshold=0.5, activity_max_seconds=SPLIT_SECONDS)
    pred = VADFromScratchPredictor(model, "cuda", device_post=True, batch_post=True)
    got = pred._post_device_many(dev, table, None, params)
    assert got == [pred._post_device(rows, params) for rows in split_by_clip(dev, table)]
    assert got == [pred._post_host(rows, params) for rows in split_by_clip(dev, table)]
    assert pred.post_batch_stats == {"calls": 1, "clips": len(SPLIT_PREDS), "split": len(flagged), "last_split": flagged}


# ---- the C ABI: cap, refusals, caller buffers ------------------------------------------------------------------------------------

def small_batch():
    lengths = [0, 3, 0, 5, 2, 9]
    preds = [[1] * 3, [0, 1, 1, 0, 1], [1, 0], [0, 1, 1, 1, 0, 0, 1, 1, 0]]
    it = iter(preds)
    probs = np.concatenate([probs_of(next(it), 7, 60 + c) for c, n in enumerate(lengths) if n])
    return probs, clip_table(lengths)


def workspace_bytes(table, W):
    nb = ctypes.c_size_t()
    _lib.check(_lib.load().savad_post_batch_workspace_bytes(table, len(table) - 1, W, *GEOMETRY, ctypes.byref(nb)))
    return nb.value


def test_cap_refusals_and_caller_buffers(torch_cuda, post_block):
    """savad_post_batch_frames / _segments inside guarded buffers of exactly the stated sizes (probs, the device table, boosted:
    4 x 19 bytes, trimmed: 19 bytes, the workspace of the size query); a cap below the count; refusals that write nothing"""
    torch = torch_cuda
    lib, st = _lib.load(), stream_(torch)
    probs, table = small_batch()
    N, W, C = len(probs), probs.shape[1], len(table) - 1
    want = reference_frames(probs, table, trim=(0, 0, 0, 0))
    want_segments = [reference_segments(t) for _, t in want]
    count = sum(len(s) for s, _ in want_segments)
    assert count == 5   # (1 + 1 + 1 + 2: the single 0 frame of [0, 1, 1, 0, 1] has no sample of its own under a 25 ms window)
    nb = workspace_bytes(table, W)

    arena = BufferArena("cuda", 1 << 22)
    pa = arena.place_input(torch.from_numpy(probs).cuda(), 4, "probs")
    ta = arena.place_input(torch.from_numpy(table).cuda(), 4, "clip_first")
    boosted = arena.place_output(4 * N, 4, torch.float32, "boosted")
    trimmed = arena.place_output(N, 1, torch.uint8, "trimmed")
    ws = arena.place_output(nb, 16, torch.uint8, "workspace")
    # refused: a workspace one byte short, a table that is none, a null pointer, a negative parameter -- nothing is written
    pf = lib.savad_post_batch_frames
    assert pf(pa, table, ta, C, W, 0.5, 0, 0, 0, 0, boosted, trimmed, ws, 0, st) == INVALID and b"workspace" in lib.savad_last_error()
    assert pf(pa, np.array([0, 5, 4, N], np.int32), ta, 3, W, 0.5, 0, 0, 0, 0, boosted, trimmed, ws, nb, st) == INVALID
    assert pf(pa, table, None, C, W, 0.5, 0, 0, 0, 0, boosted, trimmed, ws, nb, st) == INVALID
    assert pf(pa, table, ta, C, W, 0.5, 0, -1, 0, 0, boosted, trimmed, ws, nb, st) == INVALID
    arena.check()
    assert (boosted.view(torch.uint8) == 0xA5).all() and (trimmed == 0xA5).all() and (ws == 0xA5).all()
    _lib.check(pf(pa, table, ta, C, W, 0.5, 0, 0, 0, 0, boosted, trimmed, ws, nb, st))
    arena.check()
    assert same_bits(boosted, np.concatenate([b for b, _ in want])) and same_bits(trimmed, np.concatenate([t for _, t in want]))

    for cap in (count + 2, 2, 0):
        arena = BufferArena("cuda", 1 << 22)
        tr = arena.place_input(torch.from_numpy(np.concatenate([t for _, t in want])).cuda(), 1, "trimmed")
        bo = arena.place_input(torch.from_numpy(np.concatenate([b for b, _ in want])).cuda(), 4, "boosted")
        ta = arena.place_input(torch.from_numpy(table).cuda(), 4, "clip_first")
        ws = arena.place_output(nb, 16, torch.uint8, "workspace")
        seg_first, flags = np.full(C + 1, -7, np.int64), np.full(C, 9, np.uint8)
        starts, ends = np.full(count + 2, -7, np.int64), np.full(count + 2, -7, np.int64)
        ps = lib.savad_post_batch_segments
        assert ps(tr, bo, table, ta, C, *GEOMETRY, 0, seg_first, flags, starts, ends, cap, ws, nb - 1, st) == INVALID
        assert ps(tr, bo, table, None, C, *GEOMETRY, 0, seg_first, flags, starts, ends, cap, ws, nb, st) == INVALID
        assert ps(tr, None, table, ta, C, *GEOMETRY, 4000, seg_first, flags, starts, ends, cap, ws, nb, st) == INVALID   # a split needs boosted
        assert (seg_first == -7).all() and (flags == 9).all() and (starts == -7).all() and (ws == 0xA5).all()
        got = ps(tr, bo, table, ta, C, *GEOMETRY, 4000, seg_first, flags, starts, ends, cap, ws, nb, st)
        arena.check()
        assert got == count                                           # the count, whatever the room
        wrote = min(cap, count)
        assert np.array_equal(starts[:wrote], np.concatenate([s for s, _ in want_segments])[:wrote])
        assert np.array_equal(ends[:wrote], np.concatenate([e for _, e in want_segments])[:wrote])
        assert (starts[wrote:] == -7).all() and (ends[wrote:] == -7).all()
        assert seg_first.tolist() == [0] + np.cumsum([len(s) for s, _ in want_segments]).tolist() and not flags.any()


# ---- the predictor ---------------------------------------------------------------------------------------------------------------

def test_probabilities_of_one_batched_prediction(torch_cuda, model):
    """predict_probabilities_many computed ONCE, then post-processed chunk by chunk (_post, host and device) and in one batched call"""
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters
    from voice_activity_detection_amd.seeded import seeded_features

    lengths = [45, 0, 300, 39, 1, 120]
    pred = VADFromScratchPredictor(model, "cuda", device_post=True, batch_post=True)
    result, table = pred._probabilities_matrix([seeded_features(700 + c, (n, 80)) if n else np.zeros((0, 80), np.float32)
                                                for c, n in enumerate(lengths)])
    probs = result[0]
    mean = probs.cpu().numpy().mean(axis=1)
    threshold = float(np.median(mean))
    assert 0 < (mean > threshold).sum() < len(mean)
    params = VADPredictParameters(threshold=threshold, min_vally_ms=30, min_hill_ms=30, hang_before_ms=20, hang_over_ms=20)
    chunks = split_by_clip(probs, table)
    got = pred._post_device_many(probs, table, None, params)
    assert pred.post_stats == {"device": len(lengths), "host": 0}
    assert got == [pred._post(rows, params) for rows in chunks]                         # the device loop
    host = VADFromScratchPredictor(model, "cuda")
    assert got == [host._post(rows, params) for rows in chunks]                         # the host loop
    assert sum(len(a) for a, _ in got) >= 2


@pytest.fixture(scope="module")
def recording(state1234):
    """the committed wav, its chunks at split_max_seconds = 2, and a threshold at least 1e-3 away from every boosted probability the
    CPU oracle gives for those chunks: no frame can change sides between two paths that agree to 2e-6 (the margin
    tests/test_gpu_predict_batch.py establishes, restated)"""
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
    assert 0 < (boosted > threshold).sum() < len(boosted)
    return audio, bounds, threshold


def test_batch_post_on_the_committed_wav(torch_cuda, model, recording):
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    audio, bounds, threshold = recording
    params = VADPredictParameters(split_max_seconds=2, threshold=threshold, min_vally_ms=10, min_hill_ms=10, hang_before_ms=10, hang_over_ms=10)
    looped = VADFromScratchPredictor(model, "cuda", device_post=True)
    want = looped.predict(audio, params)
    assert len(want.activities) >= 1
    many = VADFromScratchPredictor(model, "cuda", device_post=True, batch_post=True)
    assert many.predict_many([audio], params) == looped.predict_many([audio], params) == [want]
    assert many.post_stats == {"device": 6, "host": 0} and many.post_batch_stats == {"calls": 1, "clips": 6, "split": 0, "last_split": []}
    chunked = VADFromScratchPredictor(model, "cuda", device_post=True, batch_chunks=True, batch_post=True)
    assert chunked.predict(audio, params) == want
    assert chunked.post_stats == {"device": 6, "host": 0} and chunked.post_batch_stats["calls"] == 1
    # several recordings in one call: one batched post-processing for the chunks of all of them
    pieces = [audio[a:b] for a, b in bounds]
    single = VADPredictParameters(None, threshold, 10, 10, 10, 10)
    assert many.predict_many(pieces + [audio], single) == looped.predict_many(pieces + [audio], single)
    assert many.post_batch_stats["calls"] == 2 and many.post_batch_stats["clips"] == 6 + 7
    # the flag alone (no device_post) changes nothing and batches nothing
    plain = VADFromScratchPredictor(model, "cuda", batch_post=True)
    assert plain.predict_many([audio], params) == [want]
    assert plain.post_stats == {"device": 0, "host": 6} and plain.post_batch_stats["calls"] == 0


def test_return_probs_and_the_fallback(torch_cuda, model, recording):
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters

    audio, bounds, threshold = recording
    params = VADPredictParameters(split_max_seconds=2, threshold=threshold, min_vally_ms=10, min_hill_ms=10, hang_before_ms=10, hang_over_ms=10,
                                  return_probs=True, probs_sample_rate=100)
    looped = VADFromScratchPredictor(model, "cuda", device_post=True, batch_chunks=True)
    batched = VADFromScratchPredictor(model, "cuda", device_post=True, batch_chunks=True, batch_post=True)
    want = looped.predict(audio, params).to_json()
    assert batched.predict(audio, params).to_json() == want and len(want["probs"]) > 0
    assert batched.post_stats == {"device": 6, "host": 0} and batched.post_batch_stats["calls"] == 1
    # 30 Hz probabilities: a hop of 0.3 samples -- every chunk takes the host code, as without the flag
    params = dataclasses.replace(params, probs_sample_rate=30)
    want = looped.predict(audio, params).to_json()
    assert batched.predict(audio, params).to_json() == want and len(want["probs"]) > 0
    assert batched.post_stats == {"device": 6, "host": 6} and batched.post_batch_stats["calls"] == 1


def test_cli_batch_post(torch_cuda, tmp_path, state1234):
    import wave

    from tests.conftest import write_reference_checkpoint
    from tests.test_postprocessing import _audio
    from voice_activity_detection_amd.__main__ import main

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    pcm = (_audio(0, 6.0) * 20000).astype(np.int16)
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    common = ["predict", str(tmp_path / "a.wav"), str(tmp_path / "m.checkpoint"), "--split-max-seconds", "2", "--min-vally-ms", "80",
              "--min-hill-ms", "60", "--hang-before-ms", "30", "--hang-over-ms", "50", "--device-post", "--batch-chunks"]
    assert main(common + ["--output-path", str(tmp_path / "looped.json")]) == 0
    assert main(common + ["--output-path", str(tmp_path / "batched.json"), "--batch-post"]) == 0
    assert json.loads((tmp_path / "batched.json").read_text()) == json.loads((tmp_path / "looped.json").read_text())
