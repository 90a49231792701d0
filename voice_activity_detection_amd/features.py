"""Feature front-end on the GPU: mirror of the reference's ``FeatureExtractor.extract_with_postprocessing``
(``vad/acoustics/feature_extractor.py:71-80``): ``log_mel`` for its shipped transform (log-mel, n_fft 512, hop 10 ms, window
25 ms, 80 mels @16 kHz: ``vad/acoustics/transforms/log_mel_spectrogram.py:19-32``), ``FrontEnd`` for every other transform
configuration a checkpoint can name."""
from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib

SAMPLE_RATE = 16000  # vad/data_models/audio_data.py:9


_RS_ZEROS, _RS_BITS, _RS_ROLLOFF, _RS_BETA = 16, 9, 0.85, 8.555504641634386   # resampy's "kaiser_fast" table
_rs_table = None


def _kaiser_fast_table():
    """right wing of rolloff * sinc(rolloff * t), t in [0, 16], 512 samples per zero crossing, under the right half of a Kaiser
    window (beta above) + its first differences (for the linear interpolation between entries)"""
    global _rs_table
    if _rs_table is None:
        n = (1 << _RS_BITS) * _RS_ZEROS
        win = np.kaiser(2 * n + 1, _RS_BETA)[n:] * _RS_ROLLOFF * np.sinc(_RS_ROLLOFF * np.linspace(0, _RS_ZEROS, num=n + 1, endpoint=True))
        _rs_table = win
    return _rs_table


def resample_to_16k(audio: np.ndarray, sample_rate: int) -> np.ndarray:
    """Band-limited (windowed-sinc) interpolation to 16 kHz: the algorithm of the reference's
    ``librosa.resample(audio, sr, 16000, res_type="kaiser_fast")`` (vad/data_models/audio_data.py:27-30) = resampy's
    "kaiser_fast" filter -- 16 zero crossings, 512 table entries per crossing linearly interpolated, roll-off 0.85, Kaiser
    beta 8.5555; table scaled by the ratio and strided when downsampling -- then zero-padded to ceil(n * 16000 / rate) samples
    (librosa's fix_length).  numpy only, vectorised over blocks of output samples.  librosa / resampy are absent from this
    image, so parity with THEM is unpinned; this function is held to a loop-by-loop restatement of resampy's published code
    (the test-side CPU restatement, resample.py) on 8 kHz / 44.1 kHz / 48 kHz fixtures (tests/test_postprocessing.py)."""
    x = np.asarray(audio, dtype=np.float32)
    rate = int(sample_rate)
    if rate == SAMPLE_RATE or x.shape[0] == 0:
        return x
    ratio = float(SAMPLE_RATE) / rate
    n_in = x.shape[0]
    n_out = int(n_in * ratio)
    n_fix = int(np.ceil(n_in * ratio))
    win = _kaiser_fast_table()
    num_table = 1 << _RS_BITS
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    nwin = win.shape[0]
    taps = nwin // step + 1                                    # upper bound of a wing's length
    xp = x.astype(np.float64)
    y = np.zeros(n_fix, dtype=np.float32)
    # the time register is accumulated as resampy does it (repeated addition, not t * increment)
    times = np.concatenate([[0.0], np.cumsum(np.full(max(n_out - 1, 0), 1.0 / ratio))]) if n_out else np.zeros(0)
    j = np.arange(taps)
    for t0 in range(0, n_out, 32768):
        tr = times[t0:t0 + 32768]
        n = tr.astype(np.int64)
        frac = scale * (tr - n)
        acc = np.zeros(tr.shape[0], dtype=np.float64)
        for wing in (0, 1):
            f = frac if wing == 0 else scale - frac
            idx_f = f * num_table
            off = idx_f.astype(np.int64)
            eta = idx_f - off
            widx = off[:, None] + j[None, :] * step            # table index of tap j
            src = (n[:, None] - j[None, :]) if wing == 0 else (n[:, None] + j[None, :] + 1)
            limit = np.minimum(n + 1, (nwin - off) // step) if wing == 0 else np.minimum(n_in - n - 1, (nwin - off) // step)
            ok = j[None, :] < limit[:, None]
            widx = np.where(ok, widx, 0)
            src = np.where(ok, src, 0)
            w = win[widx] + eta[:, None] * delta[widx]
            acc += np.where(ok, w * xp[src], 0.0).sum(axis=1)
        y[t0:t0 + tr.shape[0]] = acc.astype(np.float32)
    return y


def _riff_wave(path):
    """(rate, channels, width, is_float, raw little-endian sample bytes) of a RIFF/WAVE file: PCM (format 1), IEEE float (3) and
    WAVE_FORMAT_EXTENSIBLE (0xFFFE) wrapping either -- the stdlib `wave` module refuses the last two, soundfile (the reference's reader,
    vad/data_models/audio_data.py:32) reads them"""
    import struct

    data = Path(path).read_bytes()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, raw = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = body
        elif tag == b"data":
            raw = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or raw is None or len(fmt) < 16:
        raise ValueError(f"{path}: no fmt / data chunk")
    code, ch, rate, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if code == 0xFFFE and len(fmt) >= 26:   # extensible: the sub-format GUID starts with the plain format code
        code = struct.unpack("<H", fmt[24:26])[0]
    if code not in (1, 3):
        raise ValueError(f"{path}: unsupported WAVE format code {code} (PCM and IEEE float are read)")
    return rate, ch, bits // 8, code == 3, raw


def _pcm_to_float(raw: bytes, width: int, big_endian: bool = False, unsigned8: bool = True) -> np.ndarray:
    """interleaved integer PCM bytes -> float32 in [-1, 1) (divide by 2^(bits - 1), as soundfile does)"""
    e = ">" if big_endian else "<"
    if width == 2:
        return np.frombuffer(raw, dtype=e + "i2").astype(np.float32) / 32768.0
    if width == 1:
        if unsigned8:   # WAV
            return (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        return np.frombuffer(raw, dtype=np.int8).astype(np.float32) / 128.0   # AIFF / AU
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        if big_endian:
            b = b[:, ::-1]
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    if width == 4:
        return (np.frombuffer(raw, dtype=e + "i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    raise ValueError(f"unsupported PCM sample width {width}")


def read_audio(path):
    """Audio file -> (samples, rate, channels): the decode half of load_wav_mono16k.  `samples` is the file's interleaved
    sample stream, 1-D: int16 as stored for a 16-bit source (what the device ingest uploads: 2 bytes per sample), float32 in
    [-1, 1) for every other format (converted as soundfile does).  A trailing partial frame is dropped.  Formats: see
    load_wav_mono16k."""
    path = Path(path)
    suffix = path.suffix.lower()
    if suffix == ".pcm":
        return np.fromfile(path, dtype=np.int16), SAMPLE_RATE, 1
    if suffix in (".aiff", ".aif", ".aifc", ".au", ".snd"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)   # (both readers leave the stdlib in Python 3.13)
            mod = __import__("aifc" if suffix.startswith(".aif") else "sunau")
        with mod.open(str(path), "rb") as r:
            if r.getcomptype() not in (b"NONE", "NONE"):
                raise ValueError(f"{path}: compressed {suffix} audio ({r.getcomptype()!r}) is not read")
            rate, width, ch = r.getframerate(), r.getsampwidth(), r.getnchannels()
            raw = r.readframes(r.getnframes())
            pcm = np.frombuffer(raw, dtype=">i2").astype(np.int16) if width == 2 else _pcm_to_float(raw, width, big_endian=True, unsigned8=False)
    else:
        rate, ch, width, is_float, raw = _riff_wave(path)
        raw = raw[:len(raw) // width * width]
        if is_float:
            if width not in (4, 8):
                raise ValueError(f"{path}: IEEE float samples of {8 * width} bits")
            pcm = np.frombuffer(raw, dtype="<f4" if width == 4 else "<f8").astype(np.float32)
        elif width == 2:
            pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16)
        else:
            pcm = _pcm_to_float(raw, width)
    if ch > 1:
        pcm = pcm[:pcm.size // ch * ch]
    return pcm, int(rate), int(ch)


def load_wav_mono16k(path) -> np.ndarray:
    """Audio file -> float32 mono @16 kHz in [-1, 1): the reference's AudioData.load (vad/data_models/audio_data.py:
    18-34) with the stdlib instead of soundfile: ``.pcm`` = headerless 16-bit mono @16 kHz (:21-24); WAV with integer PCM of
    8 / 16 / 24 / 32 bits or IEEE float 32 / 64 (plain or WAVE_FORMAT_EXTENSIBLE); AIFF / AIFF-C (uncompressed) and Sun AU (linear PCM)
    through the stdlib readers; any channel count (averaged, :26) and any rate (resampled, :27-30).  Compressed containers (FLAC,
    OGG, MP3 ...) need a decoder this image does not have: convert them first."""
    pcm, rate, ch = read_audio(path)
    if pcm.dtype == np.int16:
        pcm = pcm.astype(np.float32) / 32768.0
    if Path(path).suffix.lower() == ".pcm":
        return pcm.astype(np.float32)
    if ch > 1:
        pcm = pcm.reshape(-1, ch).mean(axis=1).astype(np.float32)
    return resample_to_16k(pcm, rate)


_HOP = 160  # savad_audio_host.h: mel::HOP (frames = 1 + n // hop)
_PCM16 = (torch.int16, np.dtype("int16"))


def pcm16_to_f32(pcm: torch.Tensor) -> torch.Tensor:
    """int16 PCM samples on a HIP device -> float32 in [-1, 1) (sample / 32768, savad_pcm16_to_f32): the conversion soundfile does for
    the reference (vad/data_models/audio_data.py:21-24,32), on the device -- so that an upload moves 2 bytes per sample"""
    _lib.check_tensor(pcm, "pcm", torch.int16, 1)
    with _lib.on_device(pcm.device):
        out = torch.empty(pcm.numel(), dtype=torch.float32, device=pcm.device)
        _lib.check(_lib.load().savad_pcm16_to_f32(pcm, pcm.numel(), out, torch.cuda.current_stream(pcm.device)))
    return out


_RS_WINDOW = 8193   # include/savad.h: SAVAD_RESAMPLE_WINDOW
_rs_window_set = False


def kaiser_fast_window() -> np.ndarray:
    """resampy's "kaiser_fast" half window as resampy.filters.sinc_window groups it: taper * (rolloff * sinc).  (`_kaiser_fast_table`
    above multiplies in another order and differs in the last bit of some entries; resample_to_16k keeps that one and its bits.)"""
    n = (1 << _RS_BITS) * _RS_ZEROS
    sinc_win = _RS_ROLLOFF * np.sinc(_RS_ROLLOFF * np.linspace(0, _RS_ZEROS, num=n + 1, endpoint=True))
    return np.ascontiguousarray(np.kaiser(2 * n + 1, _RS_BETA)[n:] * sinc_win, dtype=np.float64)


def _resample_lib():
    """the library with the resampler's filter handed over (savad_resample_set_window: the table is numpy's, see include/savad.h)"""
    global _rs_window_set
    lib = _lib.load()
    if not _rs_window_set:
        win = kaiser_fast_window()
        assert win.shape == (_RS_WINDOW,)
        _lib.check(lib.savad_resample_set_window(win))
        _rs_window_set = True
    return lib


def resample_length(n_samples: int, rate: int) -> int:
    """samples of the 16 kHz signal: ceil(n_samples * 16000 / rate) (librosa's fix_length target)"""
    n = _lib.load().savad_resample_length(int(n_samples), int(rate))
    if n < 0:
        _lib.check(n)
    return n


def resample_span_samples(n_samples: int, rate: int, out_first: int, out_count: int):
    """(first, count): the input samples outputs [out_first, +out_count) of an n_samples-long recording read (first % 4 == 0)"""
    first, count = ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.load().savad_resample_span_samples(int(n_samples), int(rate), int(out_first), int(out_count),
                                                       ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


def resample_prepare(rate: int, device) -> None:
    """build and upload a source rate's tables on `device` (synchronises; the compute calls do it on first use otherwise)"""
    with _lib.on_device(torch.device(device)):
        _lib.check(_resample_lib().savad_resample_prepare(int(rate)))


def resample_to_16k_device(audio_dev: torch.Tensor, rate: int) -> torch.Tensor:
    """float32 mono samples at `rate` Hz on a HIP device -> the 16 kHz signal, ceil(n * 16000 / rate) samples, on the device: the
    reference's librosa.resample(audio, sr, 16000, res_type="kaiser_fast") (vad/data_models/audio_data.py:27-30) with the bits of
    resampy's loop (savad_resample; include/savad.h).  A 16 kHz source is returned as it is."""
    _lib.check_tensor(audio_dev, "audio", torch.float32, 1)
    rate = int(rate)
    if rate == SAMPLE_RATE:
        return audio_dev
    lib = _resample_lib()
    n = audio_dev.numel()
    with _lib.on_device(audio_dev.device):
        out = torch.empty(resample_length(n, rate), dtype=torch.float32, device=audio_dev.device)
        _lib.check(lib.savad_resample(audio_dev, n, rate, out, torch.cuda.current_stream(audio_dev.device)))
    return out


def resample_span_device(audio_dev: torch.Tensor, audio_first: int, n_samples: int, rate: int, out_first: int, out_count: int,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Samples [out_first, out_first + out_count) of the 16 kHz signal of an n_samples-long recording, from a device slice that starts
    at input sample `audio_first` (savad_resample_span; `resample_span_samples` names the slice a span needs): the same bits as
    resample_to_16k_device(whole recording)[out_first:out_first + out_count].  `out`: where to write them."""
    _lib.check_tensor(audio_dev, "audio", torch.float32, 1)
    lib = _resample_lib()
    with _lib.on_device(audio_dev.device):
        if out is None:
            out = torch.empty(int(out_count), dtype=torch.float32, device=audio_dev.device)
        _lib.check_tensor(out, "out", torch.float32, shape=(int(out_count),))
        _lib.check(lib.savad_resample_span(audio_dev, int(audio_first), audio_dev.numel(), int(n_samples), int(rate), int(out_first),
                                           int(out_count), out, torch.cuda.current_stream(audio_dev.device)))
    return out


def downmix_device(raw_dev: torch.Tensor, channels: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """interleaved int16 or float32 samples [frames * channels] on a HIP device -> float32 mono [frames] in [-1, 1) with the bits of the
    host loader (sample / 32768 for int16, then the float32 channel mean: vad/data_models/audio_data.py:26; savad_ingest_downmix).
    Limits: int16 up to 256 channels, float32 up to 7 (beyond that numpy's mean sums in another order: refused)."""
    channels = int(channels)
    _lib.check_tensor(raw_dev, "raw", (torch.int16, torch.float32), 1)
    if channels < 1 or raw_dev.numel() % channels:
        raise ValueError(f"{raw_dev.numel()} samples are not whole frames of {channels} channels")
    if channels == 1 and raw_dev.dtype == torch.float32 and out is None:
        return raw_dev
    frames = raw_dev.numel() // channels
    with _lib.on_device(raw_dev.device):
        if out is None:
            out = torch.empty(frames, dtype=torch.float32, device=raw_dev.device)
        _lib.check_tensor(out, "out", torch.float32, shape=(frames,))
        _lib.check(_lib.load().savad_ingest_downmix(raw_dev, 0 if raw_dev.dtype == torch.int16 else 1, channels, frames, out,
                                                    torch.cuda.current_stream(raw_dev.device)))
    return out


def load_audio_device(path, device="cuda") -> torch.Tensor:
    """Audio file -> float32 mono @16 kHz on `device`: load_wav_mono16k with the channel average and the resampling on the GPU.  The
    file's samples go up as they are stored (16-bit PCM: 2 bytes per sample), then downmix_device and resample_to_16k_device."""
    raw, rate, channels = read_audio(path)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.SavadError("the device ingest runs only on a HIP device (no CPU fallback)")
    if raw.size == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    return resample_to_16k_device(downmix_device(torch.from_numpy(raw).to(dev), channels), rate)


def _device_audio(audio, device, what: str) -> torch.Tensor:
    """the audio argument of the front-ends -> a non-empty contiguous 1-D float32 tensor on `device`: int16 PCM goes up as it is
    and is converted there, anything else becomes float32 on the device"""
    dev = device if isinstance(device, torch.device) else torch.device(device)
    if getattr(audio, "dtype", None) in _PCM16:
        audio = pcm16_to_f32(torch.as_tensor(audio).to(dev).contiguous())
    y = audio if (isinstance(audio, torch.Tensor) and audio.dtype == torch.float32 and audio.device == dev and audio.is_contiguous()) \
        else torch.as_tensor(audio, dtype=torch.float32).to(dev).contiguous()
    if y.dim() != 1 or y.numel() < 1:
        raise ValueError("audio must be a non-empty 1-D array")
    if y.device.type != "cuda":
        raise _lib.SavadError(f"the {what} front-end runs only on a HIP device (no CPU fallback)")
    return y


def log_mel(audio, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio: 1-D float32 samples @16 kHz (numpy or tensor; int16 PCM is uploaded as it is and converted on the device) -> device
    tensor [N, 80] float32, N = 1 + len // 160.  `out`: a contiguous float32 [N, 80] tensor on the device to write into (a clip's
    slice of a concatenated matrix: predict_many) instead of a new one.
    (Host side kept thin on purpose: for a 10 s clip the two kernels take ~25 us, the Python around them used to
    take longer.)"""
    lib = _lib.load()
    y = _device_audio(audio, device, "log-mel")
    n = y.numel()
    frames = 1 + n // _HOP
    with _lib.on_device(y.device):
        buf = torch.empty(lib.savad_logmel_workspace_bytes(n) // 4, dtype=torch.float32, device=y.device)
        if out is None:
            out = torch.empty((frames, 80), dtype=torch.float32, device=y.device)
        else:
            _lib.check_tensor(out, "out", torch.float32, shape=(frames, 80), device=y.device)
        # (raw addresses, as in the model's forward: made or checked above, and a typed argument costs ~1 us each, a fifth of this call)
        _lib.check(lib.savad_logmel(y.data_ptr(), n, buf.data_ptr(), out.data_ptr(), torch.cuda.current_stream(y.device)))
    return out


_staging = {}   # (dtype, device) -> [pinned host buffer, event of the last upload from it]; guarded by _staging_lock
_staging_lock = threading.Lock()
STAGING_KEEP_BYTES = 128 << 20   # a staging buffer above this is not kept between calls (one hour of PCM16 is 115 MB)


def release_staging() -> None:
    """give back the pinned staging buffers log_mel_many keeps between calls (after their last upload has finished)"""
    with _staging_lock:
        for _, busy in _staging.values():
            if busy is not None:
                busy.synchronize()
        _staging.clear()


def _upload_staged(arrays, table, audio_count: int, dtype, dev: torch.device) -> torch.Tensor:
    """host arrays -> their table positions of ONE pinned staging buffer -> the device, in one copy.  The buffer is kept between calls
    and grows, up to STAGING_KEEP_BYTES (a larger one lives for its call only); release_staging() gives the kept ones back.  One lock
    covers the whole step -- waiting for the previous upload from the buffer, filling it, queueing the copy, recording its event --
    so calls from several threads take turns."""
    with _staging_lock:
        slot = _staging.get((dtype, dev))
        if slot is None or slot[0].numel() < audio_count:
            slot = [torch.empty(max(audio_count, 1), dtype=dtype, pin_memory=True), None]
            if slot[0].numel() * slot[0].element_size() <= STAGING_KEEP_BYTES:
                _staging[dtype, dev] = slot
            else:
                _staging.pop((dtype, dev), None)
        stage, busy = slot
        if busy is not None:
            busy.synchronize()
        view = stage.numpy()
        for a, (first, count) in zip(arrays, table):
            view[first:first + count] = a
        up = stage[:audio_count].to(dev, non_blocking=True)   # (torch's pinned allocator keeps an unkept buffer's memory until the copy is done)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(dev))
    return up


def _in_place_clips(tensors):
    """1-D float32 views of ONE storage whose byte offsets from a 16-byte-aligned base are multiples of 16 -> (base address, table,
    audio_count): the clips are read where they are.  None for any other list."""
    full = [t for t in tensors if t.numel()]   # (an empty view has no address: it is clip (0, 0))
    if not full:
        return None
    store = full[0].untyped_storage().data_ptr()
    base = min(t.data_ptr() for t in full)
    if base % 16 or any(t.untyped_storage().data_ptr() != store or (t.data_ptr() - base) % 16 for t in full):
        return None
    table = np.array([((t.data_ptr() - base) // 4, t.numel()) if t.numel() else (0, 0) for t in tensors], dtype=np.int64)
    return base, table, int((table[:, 0] + table[:, 1]).max())


def log_mel_many(audios, device="cuda"):
    """The log-mel features of MANY clips through one library call (savad_logmel_batch: three launches whatever the number of
    clips) -> (feature [rows, 80] float32 on the device, clip_first [C + 1] int32 on the host, the same table on the device): clip
    c's rows are feature[clip_first[c]:clip_first[c + 1]], with the bits of log_mel(clip).  An empty clip is legal and has no rows.
    audios: 1-D clips @16 kHz; int16 is PCM16 (sample / 32768), anything else is taken as float32.  Host arrays are copied to their
    places in one pinned staging buffer and go up in ONE copy (a list of int16 arrays only as PCM16, converted on the device by one
    savad_pcm16_to_f32; int16 clips among others are converted while staging).  float32 device tensors that are views of one
    storage at 16-byte steps (the rows of a matrix, the chunks of a recording cut at multiples of 4 samples) are read in place;
    any other list is gathered into one device buffer first."""
    from .clips import audio_clip_table

    lib = _lib.load()
    dev = device if isinstance(device, torch.device) else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SavadError("the log-mel front-end runs only on a HIP device (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    audios = list(audios)
    if not audios:
        raise ValueError("log_mel_many needs at least one clip")
    for a in audios:
        if getattr(a, "ndim", None) != 1:
            raise ValueError("every clip must be a 1-D array")
    with _lib.on_device(dev):
        keep = None   # what owns the device audio until the launches are queued
        if all(isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float32 and a.is_contiguous() for a in audios):
            placed = _in_place_clips(audios)
            if placed is not None:
                audio, table, audio_count = placed
                keep = audios
        elif not any(isinstance(a, torch.Tensor) and a.is_cuda for a in audios):
            host = [a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in audios]
            pcm = all(a.dtype == np.int16 for a in host)
            if not pcm:   # float32 staging: an int16 clip among the others is scaled as the device conversion scales it (exact)
                host = [a.astype(np.float32) * np.float32(1.0 / 32768.0) if a.dtype == np.int16 else np.asarray(a, dtype=np.float32) for a in host]
            table, audio_count = audio_clip_table([a.size for a in host])
            keep = _upload_staged(host, table, audio_count, torch.int16 if pcm else torch.float32, dev)
            if pcm and audio_count:
                keep = pcm16_to_f32(keep)
            audio = keep.data_ptr()
        if keep is None:   # anything else: every clip as float32 on the device, gathered at the table's positions by one cat
            clips = [_device_audio(a, dev, "log-mel") if len(a) else torch.empty(0, dtype=torch.float32, device=dev) for a in audios]
            table, audio_count = audio_clip_table([c.numel() for c in clips])
            gap = torch.zeros(3, dtype=torch.float32, device=dev)
            parts = []
            for c, (first, count), nxt in zip(clips, table, list(table[1:, 0]) + [audio_count]):
                parts += [c, gap[:int(nxt - first - count)]]
            keep = torch.cat(parts)
            audio = keep.data_ptr()
        counts = table[:, 1]
        nbytes = ctypes.c_size_t()
        _lib.check(lib.savad_logmel_batch_workspace_bytes(table, len(table), audio_count, ctypes.byref(nbytes)))   # (validates the table)
        clip_first = np.concatenate([[0], np.cumsum(np.where(counts > 0, 1 + counts // _HOP, 0))]).astype(np.int32)
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        table_dev = torch.from_numpy(table).to(dev)
        feature = torch.empty((int(clip_first[-1]), 80), dtype=torch.float32, device=dev)
        clip_first_dev = torch.empty(len(table) + 1, dtype=torch.int32, device=dev)
        _lib.check(lib.savad_logmel_batch(audio, audio_count, table, table_dev, len(table), ws, feature, clip_first_dev,
                                          torch.cuda.current_stream(dev)))
    return feature, clip_first, clip_first_dev


def log_mel_span(audio, audio_first: int, n_samples: int, frame_first: int, frame_count: int) -> torch.Tensor:
    """Frames [frame_first, frame_first + frame_count) of the log-mel matrix of an n_samples-long signal, from a device
    slice `audio` that starts at sample `audio_first` (savad_logmel_span; `span_samples` names the slice a frame span
    needs).  What one rank of a sharded run computes: the same bits as the rows of log_mel(whole signal)."""
    lib = _lib.load()
    _lib.check_tensor(audio, "audio", torch.float32, 1)
    with _lib.on_device(audio.device):
        buf = torch.empty(lib.savad_logmel_span_workspace_bytes(int(frame_count)) // 4, dtype=torch.float32, device=audio.device)
        out = torch.empty((int(frame_count), 80), dtype=torch.float32, device=audio.device)
        _lib.check(lib.savad_logmel_span(audio, int(audio_first), audio.numel(), int(n_samples), int(frame_first), int(frame_count),
                                         buf, out, torch.cuda.current_stream(audio.device)))
    return out


def span_samples(n_samples: int, frame_first: int, frame_count: int):
    """(first, count): the samples frames [frame_first, +frame_count) of an n_samples-long signal read (first % 4 == 0)."""
    lib = _lib.load()
    first, count = ctypes.c_long(), ctypes.c_long()
    _lib.check(lib.savad_logmel_span_samples(int(n_samples), int(frame_first), int(frame_count), ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


_FE_TRANSFORMS = {"spectrogram": 0, "mel": 1, "log-mel": 2, "mfcc": 3}   # include/savad.h: SAVAD_FE_*


@dataclass(frozen=True)
class FrontEnd:
    """A checkpoint's ``feature_extractor`` (vad/acoustics/transforms/transform_factory.py:13-59,
    vad/acoustics/feature_extractor.py:122-147): one of the four transforms at any geometry, optionally followed by the temporal
    differences [x, delta, delta-delta] along the features.  ``extract`` runs savad_frontend (include/savad.h: semantics and
    limits); the shipped configuration (log-mel, n_fft 512, hop 10 ms, window 25 ms, 80 mels, no differences) runs ``log_mel``,
    so its features keep their bits."""
    transform: str = "log-mel"
    n_fft: int = 512
    hop_ms: float = 10
    window_ms: float = 25
    n_mels: Optional[int] = 80
    n_mfcc: Optional[int] = None
    deltas: bool = False

    def __post_init__(self):
        if self.transform not in _FE_TRANSFORMS:
            raise NotImplementedError(f"unsupported transform {self.transform!r} (known: {', '.join(_FE_TRANSFORMS)})")
        if self.transform != "spectrogram" and self.n_mels is None:
            raise NotImplementedError(f"unsupported transform {self.transform!r} without n_mels")
        if self.transform == "mfcc" and self.n_mfcc is None:
            raise NotImplementedError("unsupported transform 'mfcc' without n_mfcc")
        hop, win = self.hop, self.win
        if hop < 1 or win < 1 or not (win <= self.n_fft <= 2048):
            raise ValueError(f"front-end geometry outside the limits: hop {hop} >= 1, window {win} <= n_fft {self.n_fft} <= 2048")
        if self.transform != "spectrogram" and not 1 <= self.n_mels <= 256:
            raise ValueError(f"n_mels {self.n_mels} outside the limit 1 <= n_mels <= 256")
        if self.transform == "mfcc" and not 1 <= self.n_mfcc <= self.n_mels:
            raise ValueError(f"n_mfcc {self.n_mfcc} outside the limit 1 <= n_mfcc <= n_mels ({self.n_mels})")

    @classmethod
    def from_config(cls, fe) -> "FrontEnd":
        """A checkpoint config's ``feature_extractor`` node (dict or attribute object).  Refuses, with "unsupported" in the
        message, what the device path does not build: stacked differences (a [T, F, 3] tensor the self-attention model's
        nn.Linear(feature_size, d_model) cannot take: vad/models/model_factory.py:42-48) and a silence remover."""
        def get(c, name, default=None):
            if isinstance(c, dict):
                return c.get(name, default)
            return getattr(c, name, default)

        tr = get(fe, "transform")
        if tr is None:
            raise NotImplementedError("unsupported feature_extractor: no transform")
        if get(fe, "silence_remover"):
            raise NotImplementedError("unsupported feature_extractor: silence_remover (vad/acoustics/feature_extractor.py:115-116) is not built")
        deltas = bool(get(fe, "temporal_differences", False))
        if deltas and get(fe, "stack_differences", False):
            raise NotImplementedError("unsupported feature_extractor: stack_differences yields [T, F, 3], which the self-attention "
                                      "model cannot consume (vad/models/model_factory.py:42-48)")
        name = get(tr, "name")
        n_mels = get(tr, "n_mels")
        n_mfcc = get(tr, "n_mfcc")
        return cls(str(name), int(get(tr, "n_fft")), get(tr, "hop_ms"), get(tr, "window_ms"),
                   None if n_mels is None else int(n_mels), None if n_mfcc is None else int(n_mfcc), deltas)

    @property
    def hop(self) -> int:
        return int(self.hop_ms / 1000 * SAMPLE_RATE)

    @property
    def win(self) -> int:
        return int(self.window_ms / 1000 * SAMPLE_RATE)

    @property
    def is_shipped(self) -> bool:
        """the reference's shipped configuration: the tuned savad_logmel path"""
        return (self.transform, self.n_fft, self.hop, self.win, self.n_mels, self.deltas) == ("log-mel", 512, _HOP, 400, 80, False)

    @property
    def base_size(self) -> int:
        return {"spectrogram": self.n_fft // 2 + 1, "mfcc": self.n_mfcc}.get(self.transform, self.n_mels)

    @property
    def feature_size(self) -> int:
        return 3 * self.base_size if self.deltas else self.base_size

    def config(self):
        return _lib.savad_frontend_config(_FE_TRANSFORMS[self.transform], self.n_fft, self.hop, self.win, self.n_mels or 0,
                                          self.n_mfcc or 0, int(self.deltas))

    def frames(self, n_samples: int) -> int:
        """rows of extract() for n_samples samples (raises outside the limits)"""
        N, F = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().savad_frontend_shape(self.config(), int(n_samples), ctypes.byref(N), ctypes.byref(F)))
        return N.value

    def prepare(self, device) -> None:
        """build and upload this config's tables on `device` (synchronises: the step before a graph capture)"""
        with _lib.on_device(torch.device(device)):
            _lib.check(_lib.load().savad_frontend_prepare(self.config()))

    def extract(self, audio, device="cuda", generic: bool = False) -> torch.Tensor:
        """audio: 1-D float32 samples @16 kHz (numpy or tensor; int16 PCM is uploaded as it is and converted on the device) ->
        device tensor [frames(n), feature_size] float32.  `generic=True` runs the shipped configuration through savad_frontend as
        well (the cross-check against savad_logmel)."""
        if self.is_shipped and not generic:
            return log_mel(audio, device)
        lib = _lib.load()
        y = _device_audio(audio, device, "feature")
        with _lib.on_device(y.device):
            cfg = self.config()
            n = y.numel()
            N, F, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            _lib.check(lib.savad_frontend_shape(cfg, n, ctypes.byref(N), ctypes.byref(F)))
            _lib.check(lib.savad_frontend_workspace_bytes(cfg, n, ctypes.byref(ws)))
            buf = torch.empty(ws.value // 4, dtype=torch.float32, device=y.device)
            out = torch.empty((N.value, F.value), dtype=torch.float32, device=y.device)
            _lib.check(lib.savad_frontend(cfg, y, n, buf, out, torch.cuda.current_stream(y.device)))
        return out


SHIPPED_FRONT_END = FrontEnd()
