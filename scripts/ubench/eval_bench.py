"""The metrics step of evaluate, host against device, measured: python scripts/ubench/eval_bench.py [--out profiles/eval_bench.json]

What is timed is  probs [N, 7] on the device + the label vector on the host -> the 18 metric values  in one process:
  * host:            the step evaluate has always run: probs_dev.cpu().numpy() -> evaluate.file_metrics (numpy and Python)
  * device:          evaluate.file_metrics_device: label upload -> savad_eval_counts -> metrics.metrics_from_counts
  * host_vectorised: for honesty, the host step with a vectorised numpy mid-rank in place of metrics.roc_auc's Python loop over the
                     tie groups (this script only; the product's host path is unchanged).  Same AUC bits.
  * sort_ms:         savad_eval_sort alone (the four radix passes over N keys), between HIP events.
for one hour (360 001 frames) and for a 10 s clip (1 000 frames; recorded, not judged: it is launch-bound) of synthetic speech-like
data: voice runs of about 40 % of the frames, scores at 0.8 / 0.2 +-0.1 around a pattern that differs from the labels in 0.5 % of the
frames.  Warm-up first, then ROUNDS alternating (host, device, host_vectorised) rounds, the device synchronised before every stamp.
One JSON object on stdout (and in --out): every round, the medians, and whether the device step was below the host step in every
round.  The three legs must return equal dicts."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from voice_activity_detection_amd import _lib, evaluate  # noqa: E402
from voice_activity_detection_amd.metrics import roc_auc  # noqa: E402

ROUNDS = 7
W = 7


def planted(n_frames: int, seed: int):
    rng = np.random.default_rng(seed)
    labels = np.zeros(n_frames, dtype=np.int64)
    at, voice = 0, False
    while at < n_frames:
        r = int(rng.integers(50, 300 if voice else 450))
        labels[at:at + r] = voice
        at, voice = at + r, not voice
    pattern = labels.astype(bool)
    pattern[rng.integers(0, n_frames, size=max(n_frames // 200, 1))] ^= True
    probs = np.where(pattern[:, None], np.float32(0.8), np.float32(0.2)) + (rng.random((n_frames, W), dtype=np.float32) - np.float32(0.5)) * np.float32(0.2)
    return probs.astype(np.float32), labels


def roc_auc_vectorised(labels, scores) -> float:
    """metrics.roc_auc with the mid-ranks of the tie groups by np.repeat instead of a Python loop"""
    labels = np.asarray(labels).astype(bool).ravel()
    scores = np.asarray(scores, dtype=np.float64).ravel()
    n_pos = int(labels.sum())
    n_neg = labels.size - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("AUC needs both classes")
    order = np.argsort(scores, kind="mergesort")
    s = scores[order]
    boundaries = np.flatnonzero(np.r_[True, s[1:] != s[:-1], True])
    lo, hi = boundaries[:-1], boundaries[1:]
    ranks = np.empty(labels.size, dtype=np.float64)
    ranks[order] = np.repeat(0.5 * (lo + hi - 1) + 1.0, hi - lo)
    return float((ranks[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def stamp() -> float:
    torch.cuda.synchronize()
    return time.perf_counter()


def host(labels, probs_dev):
    return evaluate.file_metrics(labels, probs_dev.cpu().numpy(), 0.5)


def device(labels, probs_dev):
    return evaluate.file_metrics_device(labels, probs_dev, 0.5)


def host_vectorised(labels, probs_dev):
    evaluate.roc_auc = roc_auc_vectorised
    try:
        return evaluate.file_metrics(labels, probs_dev.cpu().numpy(), 0.5)
    finally:
        evaluate.roc_auc = roc_auc


def sort_alone(probs_dev, labels) -> float:
    lib = _lib.load()
    n = int(probs_dev.shape[0])
    keys = probs_dev.mean(dim=1).contiguous()
    payload = torch.from_numpy(labels.astype(np.uint8)).to(probs_dev.device)
    out_keys, out_payload = torch.empty_like(keys), torch.empty_like(payload)
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_workspace_bytes(n, 1, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=probs_dev.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.savad_eval_sort(ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(payload.data_ptr()), n, ctypes.c_void_p(out_keys.data_ptr()),
                                       ctypes.c_void_p(out_payload.data_ptr()), ctypes.c_void_p(ws.data_ptr()), need.value, stream))

    for _ in range(3):
        run()
    times = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    assert torch.equal(out_keys, torch.sort(keys, stable=True).values)
    return round(statistics.median(times), 4)


def measure(n_frames: int, seed: int) -> dict:
    probs, labels = planted(n_frames, seed)
    probs_dev = torch.from_numpy(probs).cuda()
    legs = {"host": host, "device": device, "host_vectorised": host_vectorised}
    first = {}
    for name, fn in legs.items():   # warm-up: allocator, code objects, page faults of the host arrays
        for _ in range(2):
            first[name] = fn(labels, probs_dev)
    assert first["host"] == first["device"] == first["host_vectorised"], "the paths disagree"
    rounds = []
    for _ in range(ROUNDS):
        one = {}
        for name, fn in legs.items():
            t0 = stamp()
            fn(labels, probs_dev)
            one[name + "_ms"] = round((stamp() - t0) * 1e3, 3)
        rounds.append(one)
    res = {"n_frames": n_frames, "W": W, "auc": first["host"]["auc"], "rounds": rounds}
    for name in legs:
        res[name + "_ms_median"] = statistics.median(r[name + "_ms"] for r in rounds)
    res["device_below_host_in_every_round"] = all(r["device_ms"] < r["host_ms"] for r in rounds)
    res["sort_ms_median"] = sort_alone(probs_dev, labels)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_input": ROUNDS, "hour": measure(360001, 1), "clip_10s": measure(1000, 2)}
    text = json.dumps(res, indent=1)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
