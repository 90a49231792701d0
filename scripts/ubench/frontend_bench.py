"""Feature front-end cost on the GPU: ms per hour of audio for each transform, with and without the temporal differences
(features.FrontEnd.extract = savad_frontend; "shipped" = savad_logmel, the tuned kernel of the shipped geometry, for scale).

    python scripts/ubench/frontend_bench.py [--seconds 3600] [--reps 10] [--timeout 120]

One JSON line per config.  Each config runs in a child process of its own under a time limit; the first child that fails
or runs out of time ends the run (nothing more is started on the GPU).  --one NAME runs a single config in this process
(what the children do; also the form to run under rocprofv3 --kernel-trace --stats)."""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))

CONFIGS = {  # name -> (transform, n_fft, hop_ms, window_ms, n_mels, n_mfcc, deltas, generic)
    "shipped": ("log-mel", 512, 10, 25, 80, None, False, False),
    "logmel-512-80-generic": ("log-mel", 512, 10, 25, 80, None, False, True),
    "logmel-400-40": ("log-mel", 400, 10, 25, 40, None, False, False),
    "logmel-400-40+d": ("log-mel", 400, 10, 25, 40, None, True, False),
    "logmel-1024-64": ("log-mel", 1024, 20, 50, 64, None, False, False),
    "mel-512-80": ("mel", 512, 10, 25, 80, None, False, False),
    "mfcc-512-40-13": ("mfcc", 512, 10, 25, 40, 13, False, False),
    "mfcc-512-40-13+d": ("mfcc", 512, 10, 25, 40, 13, True, False),
    "spectrogram-320": ("spectrogram", 320, 10, 20, None, None, False, False),
    "spectrogram-320+d": ("spectrogram", 320, 10, 20, None, None, True, False),
}


def run_one(name: str, seconds: float, reps: int) -> dict:
    import numpy as np
    import torch

    from voice_activity_detection_amd.features import FrontEnd

    *cfg, generic = CONFIGS[name]
    fe = FrontEnd(*cfg)
    n = int(seconds * 16000)
    rng = np.random.default_rng(0)
    audio = torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).cuda()
    for _ in range(2):
        out = fe.extract(audio, "cuda", generic=generic)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        fe.extract(audio, "cuda", generic=generic)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    return {"config": name, "frames": int(out.shape[0]), "features": int(out.shape[1]), "ms": round(ms, 4),
            "ms_per_hour": round(ms * 3600.0 / seconds, 4), "min_ms": round(float(min(times)), 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--one", default=None)
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run_one(args.one, args.seconds, args.reps)), flush=True)
        return 0
    for name in CONFIGS:
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--one", name, "--seconds", str(args.seconds),
                            "--reps", str(args.reps)], capture_output=True, text=True)
        if r.returncode != 0:
            print(json.dumps({"config": name, "rc": r.returncode, "wall_s": round(time.time() - t0, 1), "tail": (r.stdout + r.stderr)[-1500:]}),
                  flush=True)
            return 1
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
