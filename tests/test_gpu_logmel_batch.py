"""The log-mel front-end over a clip table on the GPU (savad_logmel_batch, features.log_mel_many, VADFromScratchPredictor(batch_front_end=True)).

Every feature comparison is BIT FOR BIT (torch.equal) against savad_logmel of the clip copied alone into a fresh aligned tensor: a frame is
a column of every MFMA B operand of the tile loop, so its bits depend on nothing but its own 400 samples, and the batch kernel runs that
loop (mel::logmel_fft_tiles) unchanged -- no tolerance is involved.  The references are computed once per module and never written."""
import ctypes

import numpy as np
import pytest

from tests.buffer_arena import BufferArena, same_bits
from tests.test_gpu_schedule_workspace import Knobs

pytestmark = pytest.mark.gpu

# shorter than the mirror (1 .. 255), head and tail stretches overlapping (up to 415), one frame (1, 159), 31 / 32 / 32 / 33 frames = the tile
# boundary (4959 .. 5120), an empty clip in the middle, multi-tile clips
EDGE_LENGTHS = [1, 159, 160, 208, 255, 256, 257, 415, 416, 4959, 4960, 5119, 5120, 0, 16000, 52001]


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


def frames_of(n):
    return 1 + n // 160 if n > 0 else 0


def row_table(counts):
    return np.concatenate([[0], np.cumsum([frames_of(int(n)) for n in counts])]).astype(np.int32)


def alone(torch, lib, clip):
    """savad_logmel of the clip copied alone into a fresh (allocator-aligned) tensor"""
    from voice_activity_detection_amd import _lib

    y = clip.clone()
    n = y.numel()
    out = torch.empty((frames_of(n), 80), dtype=torch.float32, device="cuda")
    if n:
        assert y.data_ptr() % 16 == 0
        ws = torch.empty(lib.savad_logmel_workspace_bytes(n) // 4, dtype=torch.float32, device="cuda")
        _lib.check(lib.savad_logmel(y, n, ws, out, torch.cuda.current_stream()))
    return out


def batch(torch, lib, audio, table, audio_count=None):
    """savad_logmel_batch on fresh buffers of exactly the reported sizes -> (features, clip_first)"""
    from voice_activity_detection_amd import _lib

    table = np.ascontiguousarray(table, dtype=np.int64)
    audio_count = audio.numel() if audio_count is None else audio_count
    nbytes, rows = ctypes.c_size_t(), ctypes.c_int64()
    _lib.check(lib.savad_logmel_batch_workspace_bytes(table, len(table), audio_count, ctypes.byref(nbytes)))
    _lib.check(lib.savad_logmel_batch_shape(table, len(table), audio_count, ctypes.byref(rows), None))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    features = torch.full((rows.value, 80), float("nan"), dtype=torch.float32, device="cuda")
    clip_first = torch.full((len(table) + 1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.savad_logmel_batch(audio, audio_count, table, torch.from_numpy(table).cuda(), len(table), ws, features, clip_first,
                                      torch.cuda.current_stream()))
    return features, clip_first


def check_clips(torch, features, clip_first, table, audio, want):
    """clip_first is the host plan's, every clip's rows are `want` of that clip (a list, or a function of (first, count)), nothing is NaN"""
    first = row_table(table[:, 1])
    assert np.array_equal(clip_first.cpu().numpy(), first)
    assert features.shape == (int(first[-1]), 80) and not bool(torch.isnan(features).any())
    for c, (a, n) in enumerate(table):
        ref = want[c] if isinstance(want, list) else want(int(a), int(n))
        assert torch.equal(features[first[c]:first[c + 1]], ref), f"clip {c} ({int(n)} samples at {int(a)})"


@pytest.fixture(scope="module")
def edge(torch_cuda, lib):
    """the edge lengths in one buffer: a gap of 4 .. 63 floats of NaN in front of every clip (and behind the last), every first a multiple
    of 4; each clip's stand-alone features"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    firsts, end = [], 0
    for n in EDGE_LENGTHS:
        firsts.append((end + 3) // 4 * 4 + 4 * int(rng.integers(1, 16)))
        end = firsts[-1] + n
    table = np.stack([np.array(firsts), np.array(EDGE_LENGTHS)], axis=1).astype(np.int64)
    host = np.full(end + 36, np.nan, dtype=np.float32)
    for a, n in table:
        host[a:a + n] = (rng.random(n, dtype=np.float32) - 0.5) * 0.4
    gaps = table[:, 0] - np.concatenate([[0], table[:-1].sum(axis=1)])
    assert (table[:, 0] % 4 == 0).all() and (gaps >= 4).all() and (gaps <= 64).all()
    audio = torch.from_numpy(host).cuda()
    want = [alone(torch, lib, audio[a:a + n]) for a, n in table]
    assert all(not bool(torch.isnan(w).any()) for w in want)
    torch.cuda.synchronize()
    return {"audio": audio, "table": table, "want": want}


# ---- 1. the edge lengths, one call -------------------------------------------------------------------------------------------

def test_edge_lengths_in_one_call(torch_cuda, lib, edge):
    features, clip_first = batch(torch_cuda, lib, edge["audio"], edge["table"])
    assert np.diff(clip_first.cpu().numpy()).tolist() == [1, 1, 2, 2, 2, 2, 2, 3, 3, 31, 32, 32, 33, 0, 101, 326]
    check_clips(torch_cuda, features, clip_first, edge["table"], edge["audio"], edge["want"])   # (a NaN of a gap that was read would show)


# ---- 2. order and overlap ------------------------------------------------------------------------------------------------------

def test_reversed_order_and_clips_that_share_storage(torch_cuda, lib, edge):
    torch = torch_cuda
    table, want = edge["table"][::-1].copy(), edge["want"][::-1]
    features, clip_first = batch(torch, lib, edge["audio"], table)
    check_clips(torch, features, clip_first, table, edge["audio"], want)
    # two clips inside the 52001-sample clip that overlap, one of them twice, between two of the others
    a52 = int(edge["table"][-1, 0])
    shared = np.array([edge["table"][9], (a52 + 400, 9000), (a52 + 4400, 9001), (a52 + 400, 9000), edge["table"][2]], dtype=np.int64)
    features, clip_first = batch(torch, lib, edge["audio"], shared)
    refs = {}

    def want_of(a, n):
        if (a, n) not in refs:
            refs[a, n] = alone(torch, lib, edge["audio"][a:a + n])
        return refs[a, n]

    check_clips(torch, features, clip_first, shared, edge["audio"], want_of)


# ---- 3. a one-clip table ---------------------------------------------------------------------------------------------------------

def test_one_clip_table_is_savad_logmel(torch_cuda, lib):
    torch = torch_cuda
    audio = (torch.rand(160000, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda") - 0.5) * 0.3
    features, clip_first = batch(torch, lib, audio, np.array([[0, 160000]]))
    assert clip_first.tolist() == [0, 1001] and torch.equal(features, alone(torch, lib, audio))


# ---- 4. many small clips: more than one tile of the scan, many one-row tiles ----------------------------------------------------------

def test_300_clips_of_one_to_three_frames(torch_cuda, lib):
    from voice_activity_detection_amd.clips import audio_clip_table

    torch = torch_cuda
    rng = np.random.default_rng(300)
    counts = rng.integers(1, 480, size=300)
    counts[[0, 255, 256, 299]] = [1, 479, 160, 319]
    table, audio_count = audio_clip_table(counts)
    assert set(np.unique(1 + counts // 160)) == {1, 2, 3}
    audio = (torch.rand(audio_count, generator=torch.Generator(device="cuda").manual_seed(6), device="cuda") - 0.5) * 0.3
    features, clip_first = batch(torch, lib, audio, table)
    tiles = ctypes.c_int64()
    assert lib.savad_logmel_batch_shape(table, 300, audio_count, None, ctypes.byref(tiles)) == 0 and tiles.value == 300
    check_clips(torch, features, clip_first, table, audio, lambda a, n: alone(torch, lib, audio[a:a + n]))


# ---- 5. caller buffers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["edge", "small", "empty"])
def test_batch_stays_inside_its_buffers_and_its_workspace(torch_cuda, lib, edge, which):
    """audio and the device table between poisoned guards; the workspace exactly as large as savad_logmel_batch_workspace_bytes reports,
    features exactly rows x 80 floats and clip_first exactly C + 1 ints, each between guards"""
    from voice_activity_detection_amd import _lib

    torch = torch_cuda
    if which == "edge":
        audio, table = edge["audio"], edge["table"]
    elif which == "small":   # one- and two-frame clips only: every tile reads both of its clip's slots
        audio, table = edge["audio"], edge["table"][:6]
    else:                    # nothing but empty clips: the row table is still written
        audio, table = edge["audio"], np.array([[0, 0], [8, 0]], dtype=np.int64)
    table = np.ascontiguousarray(table)
    want, want_first = batch(torch, lib, audio, table)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.savad_logmel_batch_workspace_bytes(table, len(table), audio.numel(), ctypes.byref(nbytes)))
    arena = BufferArena("cuda", 2 << 20)
    aa = arena.place_input(audio, 16, "audio")
    ta = arena.place_input(torch.from_numpy(table), 8, "clips")
    ws = arena.place_output(nbytes.value, 16, torch.uint8, "workspace")
    features = arena.place_output(4 * want.numel(), 16, torch.float32, "features").view(want.shape)
    clip_first = arena.place_output(4 * (len(table) + 1), 16, torch.int32, "clip_first")
    _lib.check(lib.savad_logmel_batch(aa, aa.numel(), table, ta, len(table), ws, features, clip_first, torch.cuda.current_stream()))
    arena.check()
    assert same_bits(features, want) and same_bits(clip_first, want_first)


def test_misaligned_buffers_are_refused(torch_cuda, lib, edge):
    torch = torch_cuda
    table = np.ascontiguousarray(edge["table"][:3])
    audio = edge["audio"]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    features = torch.empty(4 * 80 + 4, dtype=torch.float32, device="cuda")
    first = torch.empty(8, dtype=torch.int32, device="cuda")
    td = torch.from_numpy(table).cuda()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731
    st = torch.cuda.current_stream()
    for args in ((p(audio, 4), p(ws), p(features), p(first)), (p(audio), p(ws, 8), p(features), p(first)),
                 (p(audio), p(ws), p(features, 4), p(first)), (p(audio), p(ws), p(features), p(first, 4))):
        assert lib.savad_logmel_batch(args[0], audio.numel() - 1, table, td, 3, args[1], args[2], args[3], st) == -1
        assert b"16-byte aligned" in lib.savad_last_error()


# ---- 6. features.log_mel_many ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many(torch_cuda):
    """clips on the host as float32 and as PCM16, and the per-clip log_mel of both"""
    from voice_activity_detection_amd.features import log_mel

    rng = np.random.default_rng(12)
    lengths = [16000, 1, 4960, 0, 5121, 333, 48000]
    f32 = [((rng.random(n, dtype=np.float32) - 0.5) * 0.5) for n in lengths]
    pcm = [rng.integers(-3000, 3000, size=n).astype(np.int16) for n in lengths]
    empty = torch_cuda.empty((0, 80), dtype=torch_cuda.float32, device="cuda")
    return {"lengths": lengths, "f32": f32, "pcm": pcm, "want_f32": [log_mel(a, "cuda") if len(a) else empty for a in f32],
            "want_pcm": [log_mel(a, "cuda") if len(a) else empty for a in pcm]}


def check_many(torch, result, lengths, want):
    feature, first, first_dev = result
    assert first.dtype == np.int32 and np.array_equal(first, row_table(lengths)) and np.array_equal(first_dev.cpu().numpy(), first)
    assert first_dev.dtype == torch.int32 and first_dev.is_cuda and feature.shape == (int(first[-1]), 80)
    for c, w in enumerate(want):
        assert torch.equal(feature[first[c]:first[c + 1]], w), f"clip {c}"


@pytest.mark.parametrize("source", ["f32", "pcm"])
def test_log_mel_many_from_the_host(torch_cuda, many, source):
    from voice_activity_detection_amd.features import log_mel_many

    for _ in range(2):   # (the second call reuses the staging buffer)
        check_many(torch_cuda, log_mel_many(many[source], "cuda"), many["lengths"], many["want_" + source])
    check_many(torch_cuda, log_mel_many([torch_cuda.from_numpy(a) for a in many["f32"]], "cuda"), many["lengths"], many["want_f32"])


def test_log_mel_many_from_a_host_list_that_mixes_pcm16_and_float(torch_cuda, many):
    """int16 is PCM16 wherever it stands: a host list that is not all int16 is staged as float32, its int16 clips scaled by 1 / 32768 as
    log_mel scales them on the device -- also as a CPU tensor, and beside float64"""
    from voice_activity_detection_amd.features import log_mel_many

    kinds = ["f32", "pcm", "pcm", "f32", "f32", "pcm", "f32"]
    mixed = [many[k][c] for c, k in enumerate(kinds)]
    want = [many["want_" + k][c] for c, k in enumerate(kinds)]
    check_many(torch_cuda, log_mel_many(mixed, "cuda"), many["lengths"], want)
    mixed[1], mixed[0] = torch_cuda.from_numpy(mixed[1]), mixed[0].astype(np.float64)
    check_many(torch_cuda, log_mel_many(mixed, "cuda"), many["lengths"], want)
    check_many(torch_cuda, log_mel_many([many["f32"][0], many["pcm"][1]], "cuda"), many["lengths"][:2], [many["want_f32"][0], many["want_pcm"][1]])


def test_staging_buffers_are_capped_and_released(torch_cuda, many, monkeypatch):
    from voice_activity_detection_amd import features

    features.release_staging()
    assert features._staging == {}
    check_many(torch_cuda, features.log_mel_many(many["pcm"], "cuda"), many["lengths"], many["want_pcm"])
    assert len(features._staging) == 1                                   # kept for the next call
    monkeypatch.setattr(features, "STAGING_KEEP_BYTES", 1000)
    check_many(torch_cuda, features.log_mel_many(many["f32"], "cuda"), many["lengths"], many["want_f32"])
    assert len(features._staging) == 1                                   # above the cap: lives for its call only
    features.release_staging()
    assert features._staging == {}


def test_log_mel_many_from_device_views_in_place(torch_cuda, many):
    from voice_activity_detection_amd import features

    torch = torch_cuda
    rows = (torch.rand((5, 16000), generator=torch.Generator(device="cuda").manual_seed(9), device="cuda") - 0.5) * 0.3
    views = [rows[i] for i in (3, 0, 4)] + [rows[1][400:12400], rows[2][:0]]
    base, table, audio_count = features._in_place_clips(views)          # read where they are: nothing is copied
    assert base == rows.data_ptr() and table.tolist() == [[48000, 16000], [0, 16000], [64000, 16000], [16400, 12000], [0, 0]]
    want = [features.log_mel(v, "cuda") if v.numel() else torch.empty((0, 80), device="cuda") for v in views]
    check_many(torch, features.log_mel_many(views, "cuda"), [v.numel() for v in views], want)
    # views at other offsets, separate tensors, a host array among them: gathered into one buffer first
    assert features._in_place_clips([rows[0][2:9000], rows[1]]) is None and features._in_place_clips([rows[0], rows[1].clone()]) is None
    mixed = [rows[0][2:9000], rows[1].clone(), many["f32"][2], rows[3][1:1], many["pcm"][5]]
    want = [features.log_mel(v, "cuda") if len(v) else torch.empty((0, 80), device="cuda") for v in mixed]
    check_many(torch, features.log_mel_many(mixed, "cuda"), [len(v) for v in mixed], want)
    with pytest.raises(ValueError):
        features.log_mel_many([], "cuda")
    with pytest.raises(ValueError):
        features.log_mel_many([rows], "cuda")


# ---- 7. end to end on the committed recording --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(torch_cuda):
    from voice_activity_detection_amd import SelfAttentiveVAD
    from voice_activity_detection_amd.seeded import seeded_state_dict

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in seeded_state_dict(1234).items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def recording():
    from pathlib import Path

    from voice_activity_detection_amd.features import load_wav_mono16k

    return load_wav_mono16k(Path(__file__).resolve().parent / "golden" / "data" / "WhenTheWeatherIsFine" / "When_the_Weather_Is_Fine_12_4.wav")


def spied(predictor):
    """the (probs, mean) of every batched prediction the predictor makes"""
    seen, inner = [], predictor._predict_matrix

    def wrapped(*args):
        seen.append(inner(*args))
        return seen[-1]

    predictor._predict_matrix = wrapped
    return seen


@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
def test_predictor_with_one_front_end_call_gives_the_bits_of_the_loop(torch_cuda, lib, model, recording, precision):
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.predictor import VADPredictParameters

    torch = torch_cuda
    params = VADPredictParameters(split_max_seconds=2, threshold=0.5, min_vally_ms=10, min_hill_ms=10, hang_before_ms=10, hang_over_ms=10)
    on_device = torch.from_numpy(recording).cuda()
    with Knobs(model, precision, 0):
        old = VADFromScratchPredictor(model, "cuda", batch_chunks=True, batch_front_end=False)
        new = VADFromScratchPredictor(model, "cuda", batch_chunks=True, batch_front_end=True)
        seen_old, seen_new = spied(old), spied(new)
        # (the chunks of on_device[:128000] start at multiples of 4 samples: read in place; the other device chunks are gathered first)
        audios = [recording, on_device, recording[:30001], on_device[1000:40000], on_device[:128000]]
        assert new.predict_many(audios, params) == old.predict_many(audios, params)        # the activities
        assert new.predict(recording, params) == old.predict(recording, params)            # the batch_chunks path of predict
        assert new.predict(on_device, params) == old.predict(on_device, params)
        assert len(seen_new) == len(seen_old) == 3
        for (p1, m1), (p0, m0) in zip(seen_new, seen_old):
            assert torch.equal(p1, p0) and torch.equal(m1, m0)                             # the probabilities, bit for bit
        for predictor in (old, new):                                                       # an empty recording: refused as before
            with pytest.raises(ValueError, match="non-empty"):
                predictor.predict_many([recording, recording[:0]], VADPredictParameters(None, 0.5, 10, 10, 10, 10))
        # the work goes to the current stream: once more under a stream that is not the default one
        side, calls, inner = torch.cuda.Stream(), [], lib.savad_logmel_batch
        lib.savad_logmel_batch = lambda *args: calls.append(args[-1].cuda_stream) or inner(*args)
        try:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                assert new.predict(recording, params) == old.predict(recording, params)
        finally:
            lib.savad_logmel_batch = inner
        torch.cuda.current_stream().wait_stream(side)
        assert calls == [side.cuda_stream] and side.cuda_stream != torch.cuda.default_stream().cuda_stream
        assert torch.equal(seen_new[-1][0], seen_old[1][0])   # ... and gives what the default stream gave
