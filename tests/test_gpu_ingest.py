"""Device audio ingest on the GPU: the resampler (savad_resample, savad_resample_span) bit for bit against oracle/resample.py and its
lane-wise restatement tests/ingest_ref.py (pinned to the oracle by tests/test_ingest_host.py), the channel average
(savad_ingest_downmix) against the host loader, and the predictor paths that use them.  Bit-equality throughout: no tolerance."""
import json
import struct
import wave

import numpy as np
import pytest

from oracle import resample as orc
from tests import ingest_ref

pytestmark = pytest.mark.gpu

PAIRS = ((8000, 1500), (44100, 4000), (48000, 3001), (22050, 2000), (16001, 700), (44100, 1), (8000, 2), (96000, 5000), (11025, 1500))
BLOCK = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()})
    return m.cuda().eval()


def _signal(rate, n, seed=0):
    t = np.arange(n) / rate
    return (0.4 * np.sin(2 * np.pi * (300 + 4000 * t) * t) + 0.1 * np.random.default_rng(rate + n + seed).standard_normal(n)).astype(np.float32)


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    out = np.empty(n, dtype=np.float32)
    for a in range(0, n, 1 << 24):
        out[a:a + (1 << 24)] = rng.standard_normal(min(1 << 24, n - a), dtype=np.float32) * 0.25
    return out


def _device_resample(torch, x, rate):
    from voice_activity_detection_amd.features import resample_to_16k_device

    return resample_to_16k_device(torch.from_numpy(x).cuda(), rate)


@pytest.mark.parametrize("rate,n", PAIRS)
def test_resampler_has_the_oracles_bits(torch_cuda, rate, n):
    """resample_to_16k_device == oracle.resample.resample, bit for bit, on the nine (rate, length) pairs (two of them with
    int(n * ratio) == 0: nothing but fix_length's zero), on an all-zero signal and on a full-scale +-1 square wave; twice the same"""
    torch = torch_cuda
    square = np.where((np.arange(n) // 7) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for x in (_signal(rate, n), np.zeros(n, dtype=np.float32), square):
        want = torch.from_numpy(orc.resample(x, rate))
        got = _device_resample(torch, x, rate)
        assert got.dtype == torch.float32 and got.shape == want.shape == (int(np.ceil(n * 16000 / rate)),)
        assert torch.equal(got.cpu(), want), (rate, n, float((got.cpu() - want).abs().max()))
        assert torch.equal(_device_resample(torch, x, rate), got)


def test_16k_source_is_returned_unchanged(torch_cuda):
    from voice_activity_detection_amd.features import resample_span_device, resample_to_16k_device

    torch = torch_cuda
    x = torch.from_numpy(_signal(16000, 5000)).cuda()
    assert resample_to_16k_device(x, 16000) is x
    assert torch.equal(resample_span_device(x[96:], 96, 5000, 16000, 100, 900), x[100:1000])


@pytest.mark.parametrize("rate", [44100, 48000])
def test_ten_minutes_equal_the_lane_restatement(torch_cuda, rate):
    """10 minutes at 44.1 kHz and at 48 kHz: every output sample has the bits of tests/ingest_ref.py"""
    torch = torch_cuda
    x = _noise(600 * rate, rate)
    got = _device_resample(torch, x, rate).cpu().numpy()
    want = ingest_ref.resample(x, rate)
    assert got.shape == want.shape == (9_600_000,)
    assert np.array_equal(got, want), int((got != want).sum())


def test_one_hour_at_44100_on_sampled_blocks(torch_cuda):
    """one hour at 44.1 kHz (158.76 M samples in, 57.6 M out): blocks of 4096 outputs -- the first, the last, the block around every
    binade crossing of the time register, 64 seeded random positions -- each compared in full with tests/ingest_ref.py"""
    torch = torch_cuda
    rate, n_in = 44100, 3600 * 44100
    x = _noise(n_in, 44)
    got = _device_resample(torch, x, rate).cpu().numpy()
    n_out = int(n_in * (16000.0 / rate))
    assert got.shape == (57_600_000,) and n_out == 57_600_000
    starts = {0, n_out - BLOCK} | {int(s) for s in np.random.default_rng(64).integers(0, n_out - BLOCK, 64)}
    crossings = []
    prev_exp = None
    blocks = {}
    # one walk of the repeated addition: finds the binade crossings ...
    for k0, t in ingest_ref.time_registers(rate, n_out):
        e = np.frexp(t)[1]
        if prev_exp is None:
            idx = np.nonzero(np.diff(e))[0] + k0 + 1                               # output idx is the first of a new binade
        else:
            idx = np.nonzero(np.diff(np.concatenate([[prev_exp], e])))[0] + k0
        crossings += [int(i) for i in idx]
        prev_exp = e[-1]
    assert len(crossings) >= 27 and crossings[-1] > n_out // 2      # (0 -> 2.76 -> 5.5 -> 8.3 ... up to 2^27 = 134 M input samples)
    starts |= {min(max(c - BLOCK // 2, 0), n_out - BLOCK) for c in crossings}
    # ... and a second one collects the time registers of the sampled blocks
    for k0, t in ingest_ref.time_registers(rate, n_out):
        for s in starts:
            a, b = max(s, k0), min(s + BLOCK, k0 + t.shape[0])
            if a < b:
                blocks.setdefault(s, []).append(t[a - k0:b - k0])
    tab = ingest_ref.tables(rate)
    assert len(blocks) == len(starts)
    for s in sorted(starts):
        times = np.concatenate(blocks[s])
        assert times.shape == (BLOCK,)
        want = ingest_ref.resample_block(x, rate, times, tab)
        assert np.array_equal(got[s:s + BLOCK], want), (s, int((got[s:s + BLOCK] != want).sum()))


def test_span_form_has_the_bits_of_the_whole_call(torch_cuda):
    """savad_resample_span: outputs [o0, o1) from the slice savad_resample_span_samples names == the rows of the whole-signal call, for
    seeded random spans (the signal's ends and fix_length's zero included); a slice that misses a sample is refused"""
    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.features import resample_length, resample_span_device, resample_span_samples

    torch = torch_cuda
    rng = np.random.default_rng(21)
    for rate in (8000, 11025, 44100, 48000, 96000):
        n_in = int(rng.integers(200_000, 300_000)) | 1
        x = torch.from_numpy(_signal(rate, n_in)).cuda()
        whole = _device_resample(torch, x.cpu().numpy(), rate)
        n_fix = resample_length(n_in, rate)
        spans = [(0, n_fix), (0, 1), (n_fix - 1, 1), (n_fix - 3000, 3000)]
        longest = min(40_000, n_fix // 2)
        spans += [(int(a), int(rng.integers(1, longest))) for a in rng.integers(0, n_fix - longest, 10)]
        for o0, cnt in spans:
            first, count = resample_span_samples(n_in, rate, o0, cnt)
            got = resample_span_device(x[first:first + count], first, n_in, rate, o0, cnt)
            assert torch.equal(got, whole[o0:o0 + cnt]), (rate, o0, cnt)
        mid = n_fix // 2
        first, count = resample_span_samples(n_in, rate, mid, 1000)
        with pytest.raises(_lib.SavadError):
            resample_span_device(x[first:first + count - 2], first, n_in, rate, mid, 1000)
        with pytest.raises(_lib.SavadError):
            resample_span_device(x[first + 8:first + count], first + 8, n_in, rate, mid, 1000)


def test_rate_limits(torch_cuda):
    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.features import resample_to_16k_device

    x = torch_cuda.zeros(1000, device="cuda")
    for rate in (999, 100_001):
        with pytest.raises(_lib.SavadError, match="rate"):
            resample_to_16k_device(x, rate)
    assert resample_to_16k_device(x, 1000).shape == (16000,) and resample_to_16k_device(x[:600], 100_000).shape == (int(np.ceil(600 * (16000.0 / 100_000))),)


@pytest.mark.parametrize("C", [1, 2, 3, 6, 8])
def test_downmix_int16_has_the_host_loaders_bits(torch_cuda, C):
    from voice_activity_detection_amd.features import downmix_device

    torch = torch_cuda
    raw = np.random.default_rng(C).integers(-32768, 32768, 100_003 * C).astype(np.int16)
    raw[:4 * C] = [32767] * C + [-32768] * C + [32767, -32768] * (C // 2) + [1] * (C % 2) + [-1] * C
    f = raw.astype(np.float32) / 32768.0
    want = f if C == 1 else f.reshape(-1, C).mean(axis=1).astype(np.float32)
    got = downmix_device(torch.from_numpy(raw).cuda(), C)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want))
    # a slice that starts off the 8- and 16-byte grid
    got = downmix_device(torch.from_numpy(raw).cuda()[3 * C:], C)
    assert torch.equal(got.cpu(), torch.from_numpy(want[3:]))


@pytest.mark.parametrize("C", [1, 2, 3, 6, 7])
def test_downmix_float32_has_the_host_loaders_bits(torch_cuda, C):
    from voice_activity_detection_amd.features import downmix_device

    torch = torch_cuda
    raw = np.random.default_rng(10 + C).standard_normal(100_003 * C).astype(np.float32)
    want = raw if C == 1 else raw.reshape(-1, C).mean(axis=1).astype(np.float32)
    got = downmix_device(torch.from_numpy(raw).cuda(), C)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_downmix_float32_of_eight_channels_is_refused(torch_cuda):
    """numpy sums a row of 8 or more float32 values pairwise: the kernel's ordered sum would not have its bits, so the call is refused"""
    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.features import downmix_device

    with pytest.raises(_lib.SavadError, match="limit is 7"):
        downmix_device(torch_cuda.zeros(80, device="cuda"), 8)


def _raw_case(rate, channels, dtype, seconds=12.0):
    n = int(seconds * rate)
    t = np.arange(n) / rate
    env = (np.sin(2 * np.pi * 0.7 * t) > 0).astype(np.float32)
    rng = np.random.default_rng(rate + channels)
    chans = [env * 0.3 * np.sin(2 * np.pi * (200 + 60 * c) * t) + 0.02 * rng.standard_normal(n) for c in range(channels)]
    inter = np.stack(chans, axis=1).reshape(-1).astype(np.float32)
    return (inter * 20000).astype(np.int16) if dtype == np.int16 else inter


@pytest.mark.parametrize("rate,channels,dtype", [(44100, 2, np.int16), (48000, 1, np.float32)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_predict_audio_host_from_raw_samples(torch_cuda, model, rate, channels, dtype, precision):
    """predict_audio_host(raw, sample_rate, channels) == predict_audio_device(resample_to_16k_device(downmix_device(raw))): probs and
    mean, bit for bit, for several chunk sizes, under fp32 and under bf16 with batch_invariant"""
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.features import downmix_device, resample_to_16k_device

    torch = torch_cuda
    raw = _raw_case(rate, channels, dtype)
    pred = VADFromScratchPredictor(model, "cuda")
    model.precision, model.batch_invariant = precision, precision == "bf16"
    try:
        audio16 = resample_to_16k_device(downmix_device(torch.from_numpy(raw).cuda(), channels), rate)
        want, want_mean = pred.predict_audio_device(audio16)
        assert want.shape == (1 + audio16.numel() // 160, 7)
        for per in (100, 333, 65536):
            src = torch.from_numpy(raw).pin_memory() if per == 333 else raw
            got, got_mean = pred.predict_audio_host(src, frames_per_chunk=per, sample_rate=rate, channels=channels)
            assert torch.equal(got, want) and torch.equal(got_mean, want_mean), (per, float((got - want).abs().max()))
    finally:
        model.precision, model.batch_invariant = "fp32", False


def test_predict_audio_host_other_combinations(torch_cuda, model):
    """16 kHz stereo (no resampling) and 8 kHz mono int16 (no averaging) go through the same chunked path"""
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.features import downmix_device, resample_to_16k_device

    torch = torch_cuda
    pred = VADFromScratchPredictor(model, "cuda")
    for rate, channels, dtype in ((16000, 2, np.int16), (8000, 1, np.int16), (16000, 3, np.float32)):
        raw = _raw_case(rate, channels, dtype, seconds=6.0)
        want, want_mean = pred.predict_audio_device(resample_to_16k_device(downmix_device(torch.from_numpy(raw).cuda(), channels), rate))
        got, got_mean = pred.predict_audio_host(raw, frames_per_chunk=200, sample_rate=rate, channels=channels)
        assert torch.equal(got, want) and torch.equal(got_mean, want_mean), (rate, channels)


def test_predict_audio_host_defaults_are_unchanged(torch_cuda, model):
    """with the defaults (16 kHz mono) predict_audio_host gives predict_audio_device's bits, as before"""
    from voice_activity_detection_amd import VADFromScratchPredictor

    torch = torch_cuda
    pred = VADFromScratchPredictor(model, "cuda")
    pcm = _raw_case(16000, 1, np.int16, seconds=10.0)
    want, want_mean = pred.predict_audio_device(pcm.astype(np.float32) / 32768.0)
    for per in (500, 65536):
        got, got_mean = pred.predict_audio_host(pcm, frames_per_chunk=per)
        assert torch.equal(got, want) and torch.equal(got_mean, want_mean)
    got, _ = pred.predict_audio_host(pcm, frames_per_chunk=500, sample_rate=16000, channels=1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("pinned", [False, True])
def test_predict_audio_host_16k_mono_exactly(torch_cuda, model, dtype, pinned):
    """16 kHz mono, int16 (converted by the one-channel average) and float32 (the upload buffer is the signal), pageable and pinned, in
    several chunks and in one: predict_audio_device's probs and mean bit for bit under fp32 (every launch is the same single-launch
    kernel)"""
    from voice_activity_detection_amd import VADFromScratchPredictor

    torch = torch_cuda
    n = 16000 * 3 + 77
    raw = _raw_case(16000, 1, dtype, seconds=n / 16000)
    assert raw.shape == (n,) and raw.dtype == dtype
    pred = VADFromScratchPredictor(model, "cuda")
    want, want_mean = pred.predict_audio_device(raw.astype(np.float32) / 32768.0 if dtype == np.int16 else raw)
    assert want.shape == (301, 7)
    src = torch.from_numpy(raw).pin_memory() if pinned else raw
    for per in (100, 65536):
        got, got_mean = pred.predict_audio_host(src, frames_per_chunk=per)
        assert torch.equal(got, want) and torch.equal(got_mean, want_mean), (per, float((got - want).abs().max()))


def _write_wav(path, pcm, channels, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def test_predict_from_path_with_device_ingest(torch_cuda, model, tmp_path):
    """predict_from_path(device_ingest=True) on a 2 s 44.1 kHz stereo WAV == predict(the oracle's resampling of the host loader's
    mono signal): exactly the same VoiceActivity; predict also takes the 16 kHz device tensor itself; load_audio_device of float and
    24-bit files has the oracle's bits too"""
    from voice_activity_detection_amd import VADFromScratchPredictor, VADPredictParameters
    from voice_activity_detection_amd.features import load_audio_device

    torch = torch_cuda
    raw = _raw_case(44100, 2, np.int16, seconds=2.0)
    _write_wav(tmp_path / "clip.wav", raw, 2, 44100)
    mono = (raw.astype(np.float32) / 32768.0).reshape(-1, 2).mean(axis=1).astype(np.float32)
    want16 = orc.resample(mono, 44100)
    dev16 = load_audio_device(tmp_path / "clip.wav", "cuda")
    assert dev16.is_cuda and torch.equal(dev16.cpu(), torch.from_numpy(want16))
    params = VADPredictParameters(None, 0.5, 20, 20, 10, 10, None, True, 100)
    ingest = VADFromScratchPredictor(model, "cuda", device_ingest=True)
    host = VADFromScratchPredictor(model, "cuda")
    assert ingest.device_ingest and not host.device_ingest
    want = host.predict(want16, params).to_json()
    assert ingest.predict_from_path(tmp_path / "clip.wav", params).to_json() == want
    assert host.predict(dev16, params).to_json() == want
    split = VADPredictParameters(0.7, 0.5, 20, 20, 10, 10, None, False, None)
    assert host.predict(dev16, split).to_json() == host.predict(want16, split).to_json()
    # a float32 file with three channels
    f = _raw_case(22050, 3, np.float32, seconds=0.5)
    data = f.astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 3, 22050, 22050 * 12, 12, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    (tmp_path / "f.wav").write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    want = orc.resample(f.reshape(-1, 3).mean(axis=1).astype(np.float32), 22050)
    assert torch.equal(load_audio_device(tmp_path / "f.wav", "cuda").cpu(), torch.from_numpy(want))


def test_cli_with_device_ingest(torch_cuda, state1234, tmp_path):
    """`predict --device-ingest` and `evaluate --device-ingest` end to end on a 44.1 kHz stereo file; from_checkpoint passes the
    switch on; the ingest composes with --extended-front-end"""
    from datetime import timedelta

    from tests.conftest import write_reference_checkpoint
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.__main__ import main
    from voice_activity_detection_amd.data_models import Activity, VoiceActivity

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    assert VADFromScratchPredictor.from_checkpoint(tmp_path / "m.checkpoint", "cuda", device_ingest=True).device_ingest
    assert not VADFromScratchPredictor.from_checkpoint(tmp_path / "m.checkpoint", "cuda").device_ingest
    _write_wav(tmp_path / "clip.wav", _raw_case(44100, 2, np.int16, seconds=3.0), 2, 44100)
    out = tmp_path / "out" / "va.json"
    assert main(["predict", str(tmp_path / "clip.wav"), str(tmp_path / "m.checkpoint"), "--output-path", str(out), "--device-ingest",
                 "--return-probs", "--probs-sample-rate", "100"]) == 0
    data = json.loads(out.read_text())
    assert data["version"] == "v0.3" and data["duration"] == "00:00:03.000" and len(data["probs"]) == 302
    out2 = tmp_path / "out" / "va2.json"
    assert main(["predict", str(tmp_path / "clip.wav"), str(tmp_path / "m.checkpoint"), "--output-path", str(out2), "--device-ingest",
                 "--extended-front-end", "--return-probs", "--probs-sample-rate", "100"]) == 0
    assert json.loads(out2.read_text()) == data
    VoiceActivity(timedelta(seconds=3), [Activity(timedelta(seconds=0.0), timedelta(seconds=0.7)),
                                         Activity(timedelta(seconds=1.4), timedelta(seconds=2.1))], None, None).save(tmp_path / "va.json")
    (tmp_path / "list.jsonl").write_text(json.dumps({"audio_path": "clip.wav", "voice_activity_path": "va.json"}) + "\n")
    assert main(["evaluate", str(tmp_path / "list.jsonl"), str(tmp_path / "m.checkpoint"), "--output-path", str(tmp_path / "eval.jsonl"),
                 "--device-ingest"]) == 0
    lines = [json.loads(line) for line in (tmp_path / "eval.jsonl").read_text().splitlines()]
    assert len(lines) == 2 and all(np.isfinite(v) for k, v in lines[1].items() if not k.endswith("_path"))
    # the host path gives the same metrics up to the 2e-6 between the host resampler and the oracle
    assert main(["evaluate", str(tmp_path / "list.jsonl"), str(tmp_path / "m.checkpoint"), "--output-path", str(tmp_path / "eval_host.jsonl")]) == 0
    host = json.loads((tmp_path / "eval_host.jsonl").read_text().splitlines()[0])
    assert abs(host["auc"] - lines[0]["auc"]) < 1e-3
