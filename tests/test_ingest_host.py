"""Host side of the device audio ingest (include/savad.h: savad_resample_*, savad_ingest_downmix; features.read_audio): the test-side
lane-wise restatement against the oracle, the library's filter table, time-register segments, span arithmetic and lengths, the
property of numpy's channel mean the downmix kernel mirrors, and the decode half of the loader.  No GPU."""
import ctypes
import struct
import wave

import numpy as np
import pytest

from oracle import resample as orc
from tests import ingest_ref

PAIRS = ((8000, 1500), (44100, 4000), (48000, 3001), (22050, 2000), (16001, 700), (44100, 1), (8000, 2), (96000, 5000), (11025, 1500))
RATES = (8000, 11025, 12345, 16001, 22050, 32000, 44100, 48000, 96000)
NWIN = 8193


def _signal(rate, n, seed=0):
    t = np.arange(n) / rate
    return (0.4 * np.sin(2 * np.pi * (300 + 4000 * t) * t) + 0.1 * np.random.default_rng(rate + n + seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import features

    return features._resample_lib()


def _segments(lib, rate):
    k0, t0, s, covered = (ctypes.c_long * 256)(), (ctypes.c_double * 256)(), (ctypes.c_double * 256)(), ctypes.c_long()
    n = lib.savad_resample_segments_host(rate, 256, k0, t0, s, ctypes.byref(covered))
    assert 0 < n <= 256, lib.savad_last_error()
    return np.array(k0[:n], dtype=np.int64), np.array(t0[:n]), np.array(s[:n]), covered.value


def _expand(segs, k_lo, k_hi):
    """time registers of outputs [k_lo, k_hi) from the library's segments: t_0 + (k - k_0) * s, as a device lane forms them"""
    k0, t0, s, _ = segs
    k = np.arange(k_lo, k_hi, dtype=np.int64)
    i = np.searchsorted(k0, k, side="right") - 1
    return t0[i] + (k - k0[i]).astype(np.float64) * s[i]


@pytest.mark.parametrize("rate,n", PAIRS)
def test_lane_restatement_equals_the_oracle(rate, n):
    """tests/ingest_ref.py (lanes, taps in order, float32 accumulator) has the bits of oracle.resample.resample"""
    x = _signal(rate, n)
    want, got = orc.resample(x, rate), ingest_ref.resample(x, rate)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    # and a block deep inside, from its time registers alone
    n_out = int(n * 16000.0 / rate)
    if n_out > 10:
        times = ingest_ref.all_time_registers(rate, n_out)
        assert np.array_equal(ingest_ref.resample_block(x, rate, times[n_out // 3:n_out // 3 + 7]), want[n_out // 3:n_out // 3 + 7])


def test_library_table_is_the_oracles(lib):
    """savad_resample_table_host: for an upsampling rate the oracle's half window bit for bit, for a downsampling rate that table
    times the ratio (one float64 product per entry), the differences np.diff's with a final zero"""
    base = orc.kaiser_fast_window()[0]
    assert base.shape == (NWIN,)
    win, delta = np.empty(NWIN), np.empty(NWIN)
    for rate in (8000, 11025, 44100, 48000, 96000):
        assert lib.savad_resample_table_host(rate, win.ctypes.data, delta.ctypes.data) == 0, lib.savad_last_error()
        want = ingest_ref.tables(rate)
        if rate < 16000:
            assert np.array_equal(win, base)
        else:
            assert np.array_equal(win, base * (16000.0 / rate))
        assert np.array_equal(win, want[0]) and np.array_equal(delta, want[1]) and delta[-1] == 0.0
    # the window is an input that cannot silently change under tables already built
    other = base.copy()
    other[5] += 1e-9
    assert lib.savad_resample_set_window(other.ctypes.data) != 0
    assert lib.savad_resample_set_window(base.ctypes.data) == 0


@pytest.mark.parametrize("rate", RATES)
def test_time_segments_equal_repeated_addition(lib, rate):
    """the library's (first output, time, step) segments, expanded as a device lane expands them, equal np.cumsum's repeated float64
    addition EXACTLY over 20 M outputs (44.1 kHz: an hour of output, 57.6 M); k * increment would not (also asserted, 44.1 kHz)"""
    total = 57_600_000 if rate == 44100 else 20_000_000
    segs = _segments(lib, rate)
    assert segs[3] >= total and len(segs[0]) <= 64 and segs[0][0] == 0 and segs[1][0] == 0.0 and np.all(np.diff(segs[0]) > 0)
    for k0, t in ingest_ref.time_registers(rate, total, chunk=1 << 22):
        got = _expand(segs, k0, k0 + t.shape[0])
        assert np.array_equal(got, t), (rate, k0)
    if rate == 44100:
        k = np.arange(1 << 22, dtype=np.float64)
        assert not np.array_equal(k * (1.0 / (16000.0 / rate)), ingest_ref.all_time_registers(rate, 1 << 22))


def test_output_length(lib):
    for rate in RATES + (16000,):
        for n in (0, 1, 2, 3, 159, 160, 4000, 44101, 172_800_000):
            assert lib.savad_resample_length(n, rate) == int(np.ceil(n * (16000.0 / rate))), (rate, n)
    assert lib.savad_resample_length(100, 999) < 0 and lib.savad_resample_length(100, 100001) < 0 and lib.savad_resample_length(-1, 8000) < 0


def _touched(rate, n_in, times):
    """[lowest, highest] input index the oracle's two loops touch for outputs with these time registers (brute force from its tap
    limits: oracle/resample.py:55-72)"""
    win, _, scale, step, num_table = ingest_ref.tables(rate)
    lo, hi = None, None
    for t in times:
        n = int(t)
        frac = scale * (t - n)
        offset = int(frac * num_table)
        i_max = min(n + 1, (NWIN - offset) // step)
        offset = int((scale - frac) * num_table)
        k_max = min(n_in - n - 1, (NWIN - offset) // step)
        idx = [n - i for i in range(i_max)] + [n + k + 1 for k in range(k_max)]
        if idx:
            lo = min(idx) if lo is None else min(lo, min(idx))
            hi = max(idx) if hi is None else max(hi, max(idx))
    return lo, hi


def test_span_samples_cover_what_the_oracle_touches(lib):
    """savad_resample_span_samples: the named input range contains every index the oracle's loops touch for random output spans, and
    is tight to what the header states: first a multiple of 4 within 1 + 3 of the lowest index read, the end within 1 of the
    highest, except where the range is clipped to the signal"""
    rng = np.random.default_rng(11)
    for rate in RATES:
        n_in = int(rng.integers(30_000, 60_000))
        n_fix, n_out = int(np.ceil(n_in * (16000.0 / rate))), int(n_in * (16000.0 / rate))
        times = ingest_ref.all_time_registers(rate, n_out)
        spans = [(0, n_fix), (0, 1), (n_out - 1, 1), (n_fix - 1, 1)] + [(int(a), int(rng.integers(1, 300))) for a in rng.integers(0, n_out - 300, 12)]
        for o0, cnt in spans:
            first, count = ctypes.c_long(), ctypes.c_long()
            assert lib.savad_resample_span_samples(n_in, rate, o0, cnt, ctypes.byref(first), ctypes.byref(count)) == 0, lib.savad_last_error()
            first, count = first.value, count.value
            lo, hi = _touched(rate, n_in, times[o0:min(o0 + cnt, n_out)])
            if lo is None:   # nothing but fix_length's zeros
                assert count == 0
                continue
            assert first % 4 == 0 and 0 <= first <= lo and hi < first + count <= n_in, (rate, o0, cnt)
            assert lo - first <= 4 or first == 0, (rate, o0, cnt, lo, first)
            assert first + count - 1 - hi <= 1 or first + count == n_in, (rate, o0, cnt, hi, first + count)
        bad = ctypes.c_long()
        assert lib.savad_resample_span_samples(n_in, rate, n_fix, 1, ctypes.byref(bad), ctypes.byref(bad)) != 0
    first, count = ctypes.c_long(), ctypes.c_long()
    assert lib.savad_resample_span_samples(1000, 16000, 10, 20, ctypes.byref(first), ctypes.byref(count)) == 0
    assert (first.value, count.value) == (8, 22)


def test_device_entry_points_refuse_bad_arguments_without_a_device(lib):
    """argument errors are reported before anything touches a device"""
    assert lib.savad_ingest_downmix(None, 1, 8, 10, None, None) == -2 and b"float32" in lib.savad_last_error()   # SAVAD_E_UNSUPPORTED
    assert lib.savad_ingest_downmix(None, 0, 257, 10, None, None) == -2
    assert lib.savad_ingest_downmix(None, 2, 2, 10, None, None) == -1
    assert lib.savad_ingest_downmix(None, 0, 2, 0, None, None) == 0
    assert lib.savad_resample(None, 100, 500, None, None) == -2 and b"rate" in lib.savad_last_error()
    assert lib.savad_resample(None, 0, 44100, None, None) == 0


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7])
def test_numpy_channel_mean_is_the_ordered_sum(C):
    """what savad_ingest_downmix mirrors: numpy's float32 .reshape(-1, C).mean(axis=1) is the left-to-right float32 sum divided by
    float32(C) for C <= 7 (random float data: int16-valued data would not show the order, its sums are exact)"""
    x = np.random.default_rng(C).standard_normal((200_000, C)).astype(np.float32)
    s = x[:, 0].copy()
    for c in range(1, C):
        s = (s + x[:, c]).astype(np.float32)
    assert np.array_equal(x.reshape(-1).reshape(-1, C).mean(axis=1), s / np.float32(C))


def test_int16_channel_sums_are_exact():
    """int16 sources: every partial sum of up to 256 values k / 32768 is a multiple of 2^-15 below 2^8: exact in float32, so any
    summation order gives the mean's bits (C = 8 and 16, where numpy sums pairwise)"""
    rng = np.random.default_rng(3)
    for C in (8, 16, 256):
        v = rng.integers(-32768, 32768, (5000, C)).astype(np.int16)
        f = v.astype(np.float32) / 32768.0
        s = f[:, 0].copy()
        for c in range(1, C):
            s = (s + f[:, c]).astype(np.float32)
        assert np.array_equal(f.mean(axis=1), s / np.float32(C))
        assert np.array_equal(s.astype(np.float64) * 32768.0, v.astype(np.int64).sum(axis=1).astype(np.float64))


def _write_wav(path, data, width, ch, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(data)


def _write_float_wav(path, data, ch, rate):
    raw = np.asarray(data, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_read_audio_is_the_decode_half_of_the_loader(tmp_path):
    """read_audio + the host conversion, channel mean and resample_to_16k == load_wav_mono16k, for WAV of 8 / 16 / 24 / 32 bits and
    float, mono and stereo; 16-bit files come back as the stored int16, everything else as float32"""
    from voice_activity_detection_amd.features import load_wav_mono16k, read_audio, resample_to_16k

    rng = np.random.default_rng(8)
    for ch in (1, 2):
        for rate in (16000, 44100):
            n = 3000
            tone = 0.6 * rng.uniform(-1, 1, n * ch)
            v24 = np.round(tone * 8388607).astype(np.int32)
            files = {
                "u8": (np.round(tone * 127 + 128).astype(np.uint8).tobytes(), 1),
                "s16": (np.round(tone * 32767).astype("<i2").tobytes(), 2),
                "s24": (np.stack([v24 & 255, (v24 >> 8) & 255, (v24 >> 16) & 255], axis=1).astype(np.uint8).tobytes(), 3),
                "s32": (np.round(tone * 2147483647).astype("<i4").tobytes(), 4),
            }
            for name, (data, width) in files.items():
                _write_wav(tmp_path / f"{name}.wav", data, width, ch, rate)
            _write_float_wav(tmp_path / "f32.wav", tone, ch, rate)
            for name in list(files) + ["f32"]:
                path = tmp_path / f"{name}.wav"
                raw, r, c = read_audio(path)
                assert (r, c) == (rate, ch) and raw.ndim == 1 and raw.shape[0] == n * ch
                assert raw.dtype == (np.int16 if name == "s16" else np.float32)
                if name == "s16":
                    assert np.array_equal(raw, np.frombuffer(files["s16"][0], dtype="<i2"))
                pcm = raw.astype(np.float32) / 32768.0 if raw.dtype == np.int16 else raw
                if ch > 1:
                    pcm = pcm.reshape(-1, ch).mean(axis=1).astype(np.float32)
                assert np.array_equal(resample_to_16k(pcm, rate), load_wav_mono16k(path)), (name, ch, rate)
    pcm16 = np.round(0.5 * rng.uniform(-1, 1, 500) * 32767).astype("<i2")
    pcm16.tofile(tmp_path / "a.pcm")
    raw, r, c = read_audio(tmp_path / "a.pcm")
    assert (r, c) == (16000, 1) and raw.dtype == np.int16 and np.array_equal(raw, pcm16)
    assert np.array_equal(load_wav_mono16k(tmp_path / "a.pcm"), pcm16.astype(np.float32) / 32768.0)


def test_predictor_takes_the_ingest_switch():
    """device_ingest is an opt-in of the constructor, from_checkpoint, evaluate and both CLI commands; predict_audio_host takes the
    recording's rate and channel count"""
    import inspect

    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.evaluate import evaluate_vad_from_scratch

    for fn in (VADFromScratchPredictor.__init__, VADFromScratchPredictor.from_checkpoint, evaluate_vad_from_scratch):
        assert inspect.signature(fn).parameters["device_ingest"].default is False
    sig = inspect.signature(VADFromScratchPredictor.predict_audio_host).parameters
    assert sig["sample_rate"].default == 16000 and sig["channels"].default == 1
