"""Device audio ingest, measured: python scripts/ubench/ingest_bench.py [--hours 1.0] [--out FILE.json]

HIP events around the calls, warm-up first, then BLOCKS blocks of REPS back-to-back repetitions; a figure is the median over the blocks
of a block's mean (its spread is printed next to it).  One JSON object on stdout:
  * resample: one hour at 48 kHz and at 44.1 kHz, table in LDS (the default) and read through the cache (the A/B)
  * downmix: one hour of 48 kHz stereo int16
  * host: features.resample_to_16k on a 60 s clip, SCALED to the hour (the baseline the device path replaces)
  * end to end: predict_audio_host for the hour of 48 kHz stereo int16 (pinned), bf16 and fp32s, next to the same call on the 16 kHz
    mono hour (the path that existed before), the H2D time of the raw bytes alone and the device-resident work
    (downmix + resample + predict_audio_device); ratio = end to end / max(H2D, device work)
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from voice_activity_detection_amd import SelfAttentiveVAD, VADFromScratchPredictor, _lib, seeded_state_dict  # noqa: E402
from voice_activity_detection_amd.features import (downmix_device, resample_prepare, resample_to_16k, resample_to_16k_device)  # noqa: E402

BLOCKS, REPS, WARMUP = 5, 4, 3


def timed(fn):
    """median over BLOCKS of the mean of REPS calls, in ms, and the (min, max) of the block means"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) / REPS)
    return {"ms": round(statistics.median(means), 4), "min": round(min(means), 4), "max": round(max(means), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lib = _lib.load()
    res = {"hours": args.hours, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "reps": REPS}
    rng = np.random.default_rng(0)

    for rate in (48000, 44100):
        n = int(args.hours * 3600 * rate)
        x = (torch.randn(n, device=dev) * 0.25).contiguous()
        resample_prepare(rate, dev)
        for mode, name in ((0, "lds"), (1, "cache")):
            _lib.check(lib.savad_resample_set_table_mode(mode))
            res[f"resample_{rate}_{name}"] = timed(lambda: resample_to_16k_device(x, rate))
        _lib.check(lib.savad_resample_set_table_mode(0))
        del x

    n48 = int(args.hours * 3600 * 48000)
    raw = torch.from_numpy(rng.integers(-8000, 8000, 2 * n48, dtype=np.int16)).pin_memory()
    raw_dev = raw.to(dev)
    res["downmix_48000_stereo_int16"] = timed(lambda: downmix_device(raw_dev, 2))
    res["h2d_raw_bytes"] = raw.numel() * 2
    res["h2d_raw"] = timed(lambda: raw_dev.copy_(raw, non_blocking=True))
    mono16 = torch.from_numpy(rng.integers(-8000, 8000, int(args.hours * 3600 * 16000), dtype=np.int16)).pin_memory()
    mono16_dev = mono16.to(dev)
    res["h2d_16k_mono"] = timed(lambda: mono16_dev.copy_(mono16, non_blocking=True))

    clip = (rng.standard_normal(60 * 48000) * 0.25).astype(np.float32)
    for rate in (48000, 44100):
        c = clip[:60 * rate]
        t0 = time.perf_counter()
        resample_to_16k(c, rate)
        sec = time.perf_counter() - t0
        res[f"host_resample_{rate}"] = {"clip_s": 60, "clip_ms": round(sec * 1e3, 1), "scaled_to_hours_ms": round(sec * 1e3 * 60 * args.hours, 0)}

    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1234).items()})
    model = model.to(dev).eval()
    pred = VADFromScratchPredictor(model, dev)
    for prec in ("bf16", "fp32s"):
        model.precision = prec
        try:
            def device_work():
                return pred.predict_audio_device(resample_to_16k_device(downmix_device(raw_dev, 2), 48000))

            e2e = timed(lambda: pred.predict_audio_host(raw, sample_rate=48000, channels=2))
            work = timed(device_work)
            base = timed(lambda: pred.predict_audio_host(mono16))
            base_work = timed(lambda: pred.predict_audio_device(mono16_dev))
            res[f"predict_audio_host_{prec}"] = {
                "raw_48k_stereo_int16": e2e, "device_work": work,
                "ratio_to_max_h2d_work": round(e2e["ms"] / max(res["h2d_raw"]["ms"], work["ms"]), 3),
                "mono_16k_int16": base, "mono_16k_device_work": base_work,
                "mono_ratio_to_max_h2d_work": round(base["ms"] / max(res["h2d_16k_mono"]["ms"], base_work["ms"]), 3)}
        finally:
            model.precision = "fp32"
    text = json.dumps(res)
    print(text)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()
