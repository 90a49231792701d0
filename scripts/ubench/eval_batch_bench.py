"""The metrics step of evaluate for MANY files, batch against per-file loops, measured:
python scripts/ubench/eval_batch_bench.py [--out profiles/eval_batch_bench.json]

What is timed is  probs [rows, 7] of all clips on the device + the label vectors on the host -> the list of 18-value dicts  in one
process:
  * batch:        evaluate.files_metrics_device: one label upload -> savad_eval_batch_counts -> metrics_from_counts per clip
  * batch_counts_only: the batch leg with metrics_from_counts stubbed out (this script only): upload, workspace and the library
                  call, so that batch - batch_counts_only is the per-clip Python behind the counters
  * loop_device:  a loop of evaluate.file_metrics_device over the clips' slices (per clip: upload, workspace, savad_eval_counts)
  * loop_host:    a loop of evaluate.file_metrics over the clips' downloaded slices (numpy and Python)
on 64 clips of 10 s (1 000 frames each), 512 clips of 1 s (100 frames) and 8 clips of 10 min (60 000 frames) of the synthetic
speech-like data of eval_bench.py.  Warm-up first, then ROUNDS alternating (batch, batch_counts_only, loop_device, loop_host) rounds, the device
synchronised before every stamp.  One JSON object on stdout (and in --out): every round, the median and the range of every leg.
Recorded, not judged: no ratio is asserted.  The three full legs must return equal lists."""
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

from voice_activity_detection_amd import evaluate  # noqa: E402
from voice_activity_detection_amd.clips import clip_table, split_by_clip  # noqa: E402

ROUNDS = 7
W = 7
WORKLOADS = {"clips_64x10s": (64, 1000), "clips_512x1s": (512, 100), "clips_8x10min": (8, 60000)}


def planted(n_frames: int, seed: int):
    """eval_bench.py's data with runs short enough for a 1 s clip to hold both classes: voice runs of 10 .. 39 frames, pauses of
    10 .. 59, scores at 0.8 / 0.2 +-0.1 around a pattern that differs from the labels in 0.5 % of the frames"""
    rng = np.random.default_rng(seed)
    labels = np.zeros(n_frames, dtype=np.int64)
    at, voice = 0, False
    while at < n_frames:
        r = int(rng.integers(10, 40 if voice else 60))
        labels[at:at + r] = voice
        at, voice = at + r, not voice
    pattern = labels.astype(bool)
    pattern[rng.integers(0, n_frames, size=max(n_frames // 200, 1))] ^= True
    probs = np.where(pattern[:, None], np.float32(0.8), np.float32(0.2)) + (rng.random((n_frames, W), dtype=np.float32) - np.float32(0.5)) * np.float32(0.2)
    return probs.astype(np.float32), labels


def stamp() -> float:
    torch.cuda.synchronize()
    return time.perf_counter()


def batch(labels, probs_dev, table):
    return evaluate.files_metrics_device(labels, probs_dev, table, 0.5)


def batch_counts_only(labels, probs_dev, table):
    """the batch leg without metrics_from_counts (this script only): label upload, workspace, the library call -- what is left of
    `batch` is the per-clip Python that turns the counters into the 18 values"""
    keep = evaluate.metrics_from_counts
    evaluate.metrics_from_counts = lambda counters, seg, n: None
    try:
        return evaluate.files_metrics_device(labels, probs_dev, table, 0.5)
    finally:
        evaluate.metrics_from_counts = keep


def loop_device(labels, probs_dev, table):
    return [evaluate.file_metrics_device(y, rows, 0.5) for y, rows in zip(labels, split_by_clip(probs_dev, table))]


def loop_host(labels, probs_dev, table):
    return [evaluate.file_metrics(y, rows.cpu().numpy(), 0.5) for y, rows in zip(labels, split_by_clip(probs_dev, table))]


def measure(clips: int, n_frames: int) -> dict:
    data = [planted(n_frames, 100 + c) for c in range(clips)]
    labels = [y for _, y in data]
    table = clip_table(len(p) for p, _ in data)
    probs_dev = torch.from_numpy(np.concatenate([p for p, _ in data])).cuda()
    legs = {"batch": batch, "batch_counts_only": batch_counts_only, "loop_device": loop_device, "loop_host": loop_host}
    first = {}
    for name, fn in legs.items():   # warm-up: allocator, code objects, page faults of the host arrays
        for _ in range(2):
            first[name] = fn(labels, probs_dev, table)
    assert first["batch"] == first["loop_device"] == first["loop_host"], "the paths disagree"
    rounds = []
    for _ in range(ROUNDS):
        one = {}
        for name, fn in legs.items():
            t0 = stamp()
            fn(labels, probs_dev, table)
            one[name + "_ms"] = round((stamp() - t0) * 1e3, 3)
        rounds.append(one)
    res = {"clips": clips, "frames_per_clip": n_frames, "W": int(probs_dev.shape[1]), "rounds": rounds}
    for name in legs:
        times = [r[name + "_ms"] for r in rounds]
        res[name + "_ms_median"] = statistics.median(times)
        res[name + "_ms_range"] = [min(times), max(times)]
    res["batch_below_loop_device_in_every_round"] = all(r["batch_ms"] < r["loop_device_ms"] for r in rounds)
    res["batch_below_loop_host_in_every_round"] = all(r["batch_ms"] < r["loop_host_ms"] for r in rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_workload": ROUNDS}
    for name, (clips, n_frames) in WORKLOADS.items():
        res[name] = measure(clips, n_frames)
    text = json.dumps(res, indent=1)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
