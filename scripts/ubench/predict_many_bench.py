"""Many clips: one batched prediction against a loop of single-clip calls, measured:
python scripts/ubench/predict_many_bench.py [--out profiles/predict_many_bench.json]

Workloads (seeded noise at 16 kHz on the device; every clip of a workload has the same length, so graph=True replays ONE graph):
  * clips_64x10s   64 clips of 10 s (1001 frames each)
  * clips_512x1s   512 clips of 1 s (101 frames each)
  * hour_split10   one hour cut by split_max_seconds = 10: 360 chunks of 1001 frames
Precisions bf16 and fp32s.  Legs, in ONE process, ROUNDS rounds with the legs alternating inside a round, the device synchronised
before every stamp (wall clock: the host's share is what a loop of small calls pays):
  from the audio (what predict() runs per chunk, without the post-processing)
    * loop_eager   predict_audio_device per clip, graph=False         (the parent commit's behaviour)
    * loop_graph   predict_audio_device per clip, graph=True          (the parent commit's behaviour with its replayed graph)
    * batch        each clip's log-mel into its rows of one matrix (per-clip launches) + ONE predict_windows_batch
  from the features
    * features_loop   predict_probabilities_device per clip           (the parent commit's behaviour)
    * features_batch  ONE predict_windows_batch on the concatenated matrix (the concatenation is not timed: predict_many's
                      front-end writes the matrix in place)
and, between HIP events on the stream, the batch library call alone and the clip-aware gather of all its chunks alone
(savad_gather_windows_batch, which also re-runs the one-workgroup scan per chunk): gather_share = gather / batch call.
One JSON object on stdout (and in --out): every round, the medians, time per clip of each leg, and -- stated, not judged -- whether
the batch is slower than the graph loop.

python scripts/ubench/predict_many_bench.py --front-end [--out profiles/logmel_batch_bench.json]
measures the front-end of the batch alone, the same workloads, precisions, rounds and stamps: audio -> features -> probabilities with
    * per_clip   a log_mel call per clip into its rows of one matrix + ONE predict_windows_batch      (the `batch` leg above)
    * one        ONE log_mel_many on the clip table + ONE predict_windows_batch with its device row table
from host PCM16 (int16 arrays: per_clip uploads and converts each clip, one stages all of them and uploads once) and from float32
audio on the device (the rows of one tensor: read in place).  Twelve cells (3 workloads x 2 precisions x 2 sources); a cell counts
as won when the slowest round of `one` is below the fastest round of `per_clip` (the medians differ by more than the rounds'
spread).  `--trace-calls K --leg LEG --source SRC` makes exactly K calls of one leg on clips_64x10s and nothing else: run under a
kernel trace of its own, the front-end kernels' call counts divided by K are the launches per call."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from voice_activity_detection_amd import SelfAttentiveVAD, VADFromScratchPredictor, _lib, seeded_state_dict  # noqa: E402
from voice_activity_detection_amd.clips import clip_table, split_by_clip, window_items  # noqa: E402
from voice_activity_detection_amd.features import log_mel, log_mel_many  # noqa: E402

ROUNDS = 5
WORKLOADS = {"clips_64x10s": (64, 160000), "clips_512x1s": (512, 16000), "hour_split10": (360, 160000)}


def stamp() -> float:
    torch.cuda.synchronize()
    return time.perf_counter()


def event_ms(fn, repeats=5) -> float:
    """median GPU time of fn() between two events on the current stream"""
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def measure(model, dev, n_clips: int, n_samples: int, seed: int) -> dict:
    eager = VADFromScratchPredictor(model, dev)
    graph = VADFromScratchPredictor(model, dev, graph=True)
    half, jump, chunk = eager.context_window_half_frames, eager.context_window_jump_frames, eager.chunk_size
    gen = torch.Generator(device=dev).manual_seed(seed)
    audio = (torch.rand((n_clips, n_samples), generator=gen, device=dev) - 0.5) * 0.2
    clips = [audio[i] for i in range(n_clips)]
    frames = 1 + n_samples // 160
    table = clip_table([frames] * n_clips)
    features = [log_mel(c, dev) for c in clips]
    matrix = torch.cat(features)

    def batch_from_audio():
        m = torch.empty((int(table[-1]), 80), dtype=torch.float32, device=dev)
        for c, rows in zip(clips, split_by_clip(m, table)):
            log_mel(c, dev, out=rows)
        return model.predict_windows_batch(m, table, half, jump, chunk)

    legs = {
        "loop_eager": lambda: [eager.predict_audio_device(c) for c in clips][-1],
        "loop_graph": lambda: [graph.predict_audio_device(c) for c in clips][-1],
        "batch": batch_from_audio,
        "features_loop": lambda: [eager.predict_probabilities_device(f) for f in features][-1],
        "features_batch": lambda: model.predict_windows_batch(matrix, table, half, jump, chunk),
    }
    for fn in legs.values():   # warm-up: graph capture, workspace growth, allocator
        for _ in range(2):
            fn()
    # the same probabilities either way (to fp32 rounding / bf16's batch dependence): the last clip of the loop against its rows of the batch
    last = legs["loop_eager"]()[0]
    agree = float((legs["batch"]()[0][-frames:] - last).abs().max())
    rounds = []
    for _ in range(ROUNDS):
        r = {}
        for name, fn in legs.items():
            t0 = stamp()
            fn()
            r[name + "_ms"] = round((stamp() - t0) * 1e3, 4)
        rounds.append(r)
    med = {name: statistics.median(r[name + "_ms"] for r in rounds) for name in legs}

    # the batch call's GPU time and the gather's part of it
    lib = _lib.load()
    items = int(window_items(table, half)[-1])
    even = chunk + chunk % 2
    step = even if even <= items else max(items, 1)
    table_dev = torch.from_numpy(table).to(dev)
    items_first = torch.empty(len(table), dtype=torch.int32, device=dev)
    win = torch.empty((step, eager.context_window_frames, 80), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def gather_all():
        for first in range(0, items, step):
            _lib.check(lib.savad_gather_windows_batch(ctypes.c_void_p(matrix.data_ptr()), ctypes.c_void_p(table.ctypes.data),
                                                      ctypes.c_void_p(table_dev.data_ptr()), n_clips, 80, half, jump, first, min(step, items - first),
                                                      ctypes.c_void_p(items_first.data_ptr()), ctypes.c_void_p(win.data_ptr()), None, stream))

    call_ms, gather_ms = event_ms(legs["features_batch"]), event_ms(gather_all)
    return {"clips": n_clips, "frames_per_clip": frames, "windows": items, "forwards_per_batch_call": -(-items // step),
            "max_abs_difference_batch_vs_loop": agree, "rounds": rounds,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "per_clip_us": {k: round(v * 1e3 / n_clips, 3) for k, v in med.items()},
            "batch_call_gpu_ms": round(call_ms, 4), "gather_gpu_ms": round(gather_ms, 4), "gather_share": round(gather_ms / call_ms, 4),
            "batch_over_loop_graph": round(med["batch"] / med["loop_graph"], 4), "batch_over_loop_eager": round(med["batch"] / med["loop_eager"], 4),
            "features_batch_over_features_loop": round(med["features_batch"] / med["features_loop"], 4),
            "batch_slower_than_graph_loop": bool(med["batch"] > med["loop_graph"])}


def front_end_legs(model, dev, n_clips: int, n_samples: int, seed: int) -> dict:
    """(source, leg) -> a call: audio -> features -> probabilities of every clip"""
    pred = VADFromScratchPredictor(model, dev)
    half, jump, chunk = pred.context_window_half_frames, pred.context_window_jump_frames, pred.chunk_size
    gen = torch.Generator(device=dev).manual_seed(seed)
    audio = (torch.rand((n_clips, n_samples), generator=gen, device=dev) - 0.5) * 0.2
    pcm = (audio * 32768.0).to(torch.int16).cpu().numpy()
    sources = {"host_pcm16": [pcm[i] for i in range(n_clips)], "device_f32": [audio[i] for i in range(n_clips)]}
    table = clip_table([1 + n_samples // 160] * n_clips)

    def per_clip(clips):
        m = torch.empty((int(table[-1]), 80), dtype=torch.float32, device=dev)
        for c, rows in zip(clips, split_by_clip(m, table)):
            log_mel(c, dev, out=rows)
        return model.predict_windows_batch(m, table, half, jump, chunk)

    def one(clips):
        m, first, first_dev = log_mel_many(clips, dev)
        return model.predict_windows_batch(m, first, half, jump, chunk, first_dev)

    return {(src, leg): (lambda fn=fn, clips=clips: fn(clips)) for src, clips in sources.items() for leg, fn in (("per_clip", per_clip), ("one", one))}


def measure_front_end(model, dev, n_clips: int, n_samples: int, seed: int) -> dict:
    legs = front_end_legs(model, dev, n_clips, n_samples, seed)
    for fn in legs.values():   # warm-up: table upload, workspace growth, staging buffer, allocator
        for _ in range(2):
            fn()
    out = {"clips": n_clips, "frames_per_clip": 1 + n_samples // 160}
    for src in ("host_pcm16", "device_f32"):
        same = all(torch.equal(a, b) for a, b in zip(legs[src, "per_clip"](), legs[src, "one"]()))
        rounds = []
        for _ in range(ROUNDS):
            r = {}
            for leg in ("per_clip", "one"):
                t0 = stamp()
                legs[src, leg]()
                r[leg + "_ms"] = round((stamp() - t0) * 1e3, 4)
            rounds.append(r)
        med = {leg: statistics.median(r[leg + "_ms"] for r in rounds) for leg in ("per_clip", "one")}
        spread = {leg: [min(r[leg + "_ms"] for r in rounds), max(r[leg + "_ms"] for r in rounds)] for leg in ("per_clip", "one")}
        out[src] = {"same_bits": bool(same), "rounds": rounds, "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": spread,
                    "per_clip_us": {k: round(v * 1e3 / n_clips, 3) for k, v in med.items()},
                    "one_over_per_clip": round(med["one"] / med["per_clip"], 4),
                    "one_below_per_clip_beyond_spread": bool(spread["one"][1] < spread["per_clip"][0])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--front-end", action="store_true", help="the front-end legs (per-clip log_mel calls against one log_mel_many)")
    ap.add_argument("--trace-calls", type=int, default=0, help="make exactly this many calls of --leg from --source and nothing else")
    ap.add_argument("--leg", choices=("per_clip", "one"), default="one")
    ap.add_argument("--source", choices=("host_pcm16", "device_f32"), default="device_f32")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    model = SelfAttentiveVAD(80, 3, 128, 0.5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1234).items()})
    model = model.to(dev).eval()
    if args.trace_calls:
        model.precision = "bf16"
        call = front_end_legs(model, dev, *WORKLOADS["clips_64x10s"], 11)[args.source, args.leg]
        for _ in range(args.trace_calls):
            call()
        torch.cuda.synchronize()
        print(json.dumps({"leg": args.leg, "source": args.source, "calls": args.trace_calls, "clips": WORKLOADS["clips_64x10s"][0]}))
        return
    res = {"device": torch.cuda.get_device_name(0), "rounds_per_workload": ROUNDS, "chunk_size": 16384}
    for precision in ("bf16", "fp32s"):
        model.precision = precision
        run = measure_front_end if args.front_end else measure
        res[precision] = {name: run(model, dev, n, samples, 11 + i) for i, (name, (n, samples)) in enumerate(WORKLOADS.items())}
    if args.front_end:
        cells = [res[p][w][s]["one_below_per_clip_beyond_spread"] for p in ("bf16", "fp32s") for w in WORKLOADS for s in ("host_pcm16", "device_f32")]
        res["cells_won"], res["cells"] = sum(cells), len(cells)
    text = json.dumps(res, indent=1)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
