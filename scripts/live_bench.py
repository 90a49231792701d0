#!/usr/bin/env python3
"""Milliseconds per tick of the live mode (voice_activity_detection_amd/live.py) against the only alternative the offline entry
points offer for audio that is still arriving: per stream, predict_audio_device over the last 2 * (2 * half * 160 + 208) samples plus
the push, in a loop.  Writes profiles/live_bench.json; not part of bench.py.

    python scripts/live_bench.py [--streams 1 64 1024] [--ticks 40] [--repeats 5] [--out profiles/live_bench.json]

S streams push 100 ms (1 600 samples) or 20 ms (320 samples) of 16-bit PCM from host memory per tick; precisions bf16 and fp32s,
automatic schedule.  Every case: warm-up ticks until every stream is past its 393 ms of latency (so a tick does its steady-state
work), then `repeats` windows of `ticks` ticks, each window timed with a host clock around work that ends in a device synchronise;
reported: the mean of the windows' ms per tick, their standard deviation, minimum and maximum.  The loop is timed the same way, its
audio already on the device (the favourable case for it); it returns every frame of its slice, the live tick only the rows that
became final, so the loop's figure is what a caller pays today to learn the same rows.  Needs a GPU: there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

HALF, JUMP = 19, 9
HALO = 2 * (2 * HALF * 160 + 208)


def stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"mean_ms": float(a.mean()), "std_ms": float(a.std()), "min_ms": float(a.min()), "max_ms": float(a.max()), "windows": len(ms)}


def time_windows(torch, fn, ticks, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / ticks)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-ticks", type=int, default=3, help="ticks per window of the per-stream loop (S calls each)")
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "live_bench.json")
    args = ap.parse_args()

    import torch

    from voice_activity_detection_amd import LiveVAD, SelfAttentiveVAD, VADFromScratchPredictor, seeded_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("live_bench.py needs a HIP device")
    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1234).items()})
    model = model.to("cuda").eval()
    rng = np.random.default_rng(7)
    cases = []
    for precision in ("bf16", "fp32s"):
        model.precision, model.row_mode = precision, 0
        predictor = VADFromScratchPredictor(model, "cuda")
        for push in (1600, 320):
            for S in args.streams:
                pcm = (rng.standard_normal((S, push)) * 3000).astype(np.int16)
                vad = LiveVAD(model, "cuda", streams=S, max_push_samples=push)
                slots = [vad.open() for _ in range(S)]
                chunks = {s: pcm[i] for i, s in enumerate(slots)}
                warm = (2 * HALF * 160 + 208) // push + 12
                rows = 0
                for _ in range(warm):
                    rows = vad.push(chunks).probs.shape[0]
                live = time_windows(torch, lambda: vad.push(chunks), args.ticks, args.repeats)
                assert vad.push(chunks).probs.shape[0] == rows == S * (push // 160)
                slices = [torch.from_numpy((rng.standard_normal(HALO + push) * 0.1).astype(np.float32)).cuda() for _ in range(min(S, 64))]

                def loop_tick():
                    for i in range(S):
                        predictor.predict_audio_device(slices[i % len(slices)])

                loop_tick()
                loop = time_windows(torch, loop_tick, args.loop_ticks if S > 1 else args.ticks, args.repeats)
                case = {"precision": precision, "push_samples": push, "push_ms": push / 16.0, "streams": S, "rows_per_tick": rows,
                        "live_tick": stats(live), "offline_loop": stats(loop), "loop_slice_samples": HALO + push}
                print(json.dumps(case), flush=True)
                cases.append(case)
                del vad
    model.precision = "fp32"
    result = {"what": "ms per tick: LiveVAD.push of S streams (host PCM16 chunks) vs a loop of predict_audio_device over each stream's last "
                      f"{HALO} samples plus the push (audio on the device)",
              "device": torch.cuda.get_device_name(0), "half": HALF, "jump": JUMP, "ticks_per_window": args.ticks, "cases": cases}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
