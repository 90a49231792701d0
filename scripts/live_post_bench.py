#!/usr/bin/env python3
"""Milliseconds per tick of the live mode with and without its post-processing stage (LiveVAD(post=...), csrc/savad_live_post.h), and
the bytes a tick brings down.  Writes profiles/live_post_bench.json; not part of bench.py.

    python scripts/live_post_bench.py [--streams 1 64 1024] [--ticks 40] [--repeats 5] [--out profiles/live_post_bench.json]

S streams push 100 ms (1 600 samples) or 20 ms (320 samples) of 16-bit PCM from host memory per tick; precisions bf16 and fp32s,
automatic schedule; trim at the command line's usual 200 / 200 / 100 / 100 ms, the threshold at the median of the warm-up ticks'
means so that events do occur.  Three sessions per case, warmed up until every stream is past its latency, then timed in ALTERNATING
windows (off, on, fetch, off, on, fetch ...) of `ticks` ticks, each with a host clock around work that ends in a device synchronise:
  off    post=None: the tick as it was before the stage existed
  on     post set, nobody reads the events: two more launches, no read-back
  fetch  post set, tick.events() of one slot read every tick: one device -> host copy per tick for all slots
Reported: mean, standard deviation, minimum and maximum of the windows' ms per tick; the bytes the fetch copies per tick against the
rows x 4 bytes of downloading `mean` to run a state machine on the host.  Needs a GPU: there is no CPU fallback."""
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


def stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"mean_ms": float(a.mean()), "std_ms": float(a.std()), "min_ms": float(a.min()), "max_ms": float(a.max()), "windows": len(ms)}


def window(torch, fn, ticks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ticks


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "live_post_bench.json")
    args = ap.parse_args()

    import torch

    from voice_activity_detection_amd import LiveVAD, SelfAttentiveVAD, VADPredictParameters, seeded_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("live_post_bench.py needs a HIP device")
    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1234).items()})
    model = model.to("cuda").eval()
    rng = np.random.default_rng(7)
    cases = []
    for precision in ("bf16", "fp32s"):
        model.precision, model.row_mode = precision, 0
        for push in (1600, 320):
            for S in args.streams:
                # a few different chunks per stream, so that the means move around the threshold from tick to tick
                pcm = (rng.standard_normal((4, S, push)) * 3000 * rng.random((4, S, 1))).astype(np.int16)
                warm = (2 * HALF * 160 + 208) // push + 12 + 50 * 160 // push
                turn = [0]

                def session(post):
                    vad = LiveVAD(model, "cuda", streams=S, max_push_samples=push, post=post)
                    slots = [vad.open() for _ in range(S)]
                    return vad, slots

                def pusher(vad, slots, fetch):
                    def tick():
                        turn[0] += 1
                        t = vad.push({s: pcm[turn[0] % 4, i] for i, s in enumerate(slots)})
                        if fetch:
                            tick.events += len(t.events(slots[0]))
                            tick.bytes.append(t.fetched_bytes)
                        return t
                    tick.events, tick.bytes = 0, []
                    return tick

                off = pusher(*session(None), False)
                means = []
                for _ in range(warm):
                    means.append(off().mean)
                threshold = float(torch.cat(means).median())
                post = VADPredictParameters(None, threshold, 200, 200, 100, 100)
                on, fetch = pusher(*session(post), False), pusher(*session(post), True)
                for _ in range(warm):
                    on(), fetch()
                rows = off().probs.shape[0]
                assert rows == S * (push // 160)
                fetch.bytes.clear()
                times = {"off": [], "on": [], "fetch": []}
                for _ in range(args.repeats):
                    times["off"].append(window(torch, off, args.ticks))
                    times["on"].append(window(torch, on, args.ticks))
                    times["fetch"].append(window(torch, fetch, args.ticks))
                case = {"precision": precision, "push_samples": push, "push_ms": push / 16.0, "streams": S, "rows_per_tick": rows,
                        "threshold": threshold, "post_off": stats(times["off"]), "post_on_no_fetch": stats(times["on"]),
                        "post_on_fetch_every_tick": stats(times["fetch"]), "fetch_bytes_per_tick": float(np.mean(fetch.bytes)),
                        "mean_download_bytes_per_tick": rows * 4, "events_of_slot0_seen": fetch.events}
                print(json.dumps(case), flush=True)
                cases.append(case)
    model.precision = "fp32"
    result = {"what": "ms per tick of LiveVAD.push of S streams (host PCM16 chunks): post off / post on, events never read / post on, events "
                      "read every tick; alternating windows; trim 20 / 20 / 10 / 10 frames",
              "device": torch.cuda.get_device_name(0), "half": HALF, "jump": JUMP, "ticks_per_window": args.ticks, "cases": cases}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
