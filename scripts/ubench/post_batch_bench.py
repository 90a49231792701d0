"""Post-processing of a batched prediction, looped against batched, measured:
    python scripts/ubench/post_batch_bench.py [--out profiles/post_batch_bench.json]

What is timed is  probs [sum N, 7] of all chunks on the device -> list of VoiceActivity  (VADFromScratchPredictor._voice_activities,
the tail of predict_many) in one process, three ways:
  * host:    every chunk through _post_host (device -> host copy of its matrix, the host functions)
  * device:  every chunk through _post_device (savad_post_frames + savad_post_segments per chunk: `device_post`)
  * batched: all chunks through ONE savad_post_batch_frames + savad_post_batch_segments (`device_post` and `batch_post`)
for 64 clips of 10 s (64 recordings), 512 clips of 1 s (512 recordings) and the 360 chunks of one hour at split_max_seconds = 10
(one recording), with the probabilities of the bf16 and of the fp32s forward of seeded weights on seeded features, thresholded at their
median, post parameters (20, 20, 10, 10) frames.  Warm-up first, then PAIRS alternating (host, device, batched) rounds, the device
synchronised before every stamp.  The three results must be equal.  One JSON object on stdout (and in --out)."""
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

from voice_activity_detection_amd import (SelfAttentiveVAD, VADFromScratchPredictor, VADPredictParameters, seeded_features,  # noqa: E402
                                          seeded_state_dict)

PAIRS = 5
WORKLOADS = {   # name -> (chunks, frames per chunk, recordings)
    "64_clips_of_10s": (64, 1001, 64),
    "512_clips_of_1s": (512, 101, 512),
    "hour_in_360_chunks_of_10s": (360, 1001, 1),
}


def stamp() -> float:
    torch.cuda.synchronize()
    return time.perf_counter()


def measure(model, precision: str, chunks: int, frames: int, recordings: int) -> dict:
    dev = torch.device("cuda")
    model.precision = precision
    legs = {"host": VADFromScratchPredictor(model, dev), "device": VADFromScratchPredictor(model, dev, device_post=True),
            "batched": VADFromScratchPredictor(model, dev, device_post=True, batch_post=True)}
    feats = [seeded_features(3000 + c, (frames, 80)) for c in range(chunks)]
    (probs, mean), table = legs["host"]._probabilities_matrix(feats)
    table_dev = torch.from_numpy(table).to(dev)
    per = chunks // recordings
    seconds = (frames - 1) / 100
    plan = [(seconds, range(r * per, (r + 1) * per)) for r in range(recordings)]
    params = VADPredictParameters(threshold=float(mean.median()), min_vally_ms=200, min_hill_ms=200, hang_before_ms=100, hang_over_ms=100)

    def run(name):
        return legs[name]._voice_activities(probs, table, table_dev, plan, params)

    first = {name: run(name) for name in legs}
    for name in legs:   # warm-up: allocator, code objects
        run(name)
    assert first["host"] == first["device"] == first["batched"], "the three paths disagree"
    assert legs["batched"].post_batch_stats["calls"] == 2 and legs["device"].post_stats["device"] == 2 * chunks
    pairs = []
    for _ in range(PAIRS):
        pair = {}
        for name in legs:
            t0 = stamp()
            run(name)
            pair[name + "_ms"] = round((stamp() - t0) * 1e3, 3)
        pairs.append(pair)
    med = {name: statistics.median(p[name + "_ms"] for p in pairs) for name in legs}
    return {"chunks": chunks, "frames_per_chunk": frames, "recordings": recordings,
            "segments": sum(len(v.activities) for v in first["batched"]), "pairs": pairs,
            "host_ms_median": med["host"], "device_ms_median": med["device"], "batched_ms_median": med["batched"],
            "batched_us_per_chunk": round(med["batched"] * 1e3 / chunks, 2),
            "batched_below_both_in_every_pair": all(p["batched_ms"] < min(p["host_ms"], p["device_ms"]) for p in pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1234).items()})
    model = model.to("cuda").eval()
    res = {"device": torch.cuda.get_device_name(0), "pairs_per_input": PAIRS, "post_parameters_frames": [20, 20, 10, 10]}
    for name, (chunks, frames, recordings) in WORKLOADS.items():
        for precision in ("bf16", "fp32s"):
            res[f"{name}_{precision}"] = measure(model, precision, chunks, frames, recordings)
            print(name, precision, {k: v for k, v in res[f"{name}_{precision}"].items() if k != "pairs"}, file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
