"""``python -m voice_activity_detection_amd predict AUDIO CHECKPOINT [options]`` and
``... evaluate EVAL_LIST CHECKPOINT [options]`` -- the reference's ``python main.py predict`` / ``evaluate``
(``main.py:8-10``, ``vad/predict.py:10-50``, ``vad/evaluate.py:20-29``) on the MI355X path: same positional
arguments, same options, JSON v0.3 (predict) / metric lines (evaluate) to ``--output-path`` or stdout.
``... live AUDIO CHECKPOINT --push-ms 100`` feeds the file through a live session (live.py): one JSON line per speech start / end as
soon as it is final, then the JSON ``predict`` writes for that file and those parameters.
``train`` is out of scope."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="voice_activity_detection_amd")
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("predict", help="voice activity of one 16 kHz WAV file (vad/predict.py:10-25)")
    p.add_argument("audio_path", type=Path)
    p.add_argument("checkpoint_path", type=Path)
    p.add_argument("--output-path", type=Path, default=None, help="Path to store output. Default to stdout.")
    p.add_argument("--split-max-seconds", type=float, default=None, help="Chunk size to split audio in seconds.")
    p.add_argument("--activity-max-sec", type=int, default=None, help="Maximum length of voice activity in seconds")
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--min-vally-ms", type=int, default=0)
    p.add_argument("--min-hill-ms", type=int, default=0)
    p.add_argument("--hang-before-ms", type=int, default=0)
    p.add_argument("--hang-over-ms", type=int, default=0)
    p.add_argument("--return-probs", action="store_true")
    p.add_argument("--probs-sample-rate", type=int, default=None)
    p.add_argument("--device", default="cuda")
    p.add_argument("--precision", choices=("fp32", "fp32s", "bf16"), default="fp32",
                   help="not in the reference: fp32 = exact-fp32 matrix cores; fp32s = the same results to fp32 rounding on the bf16 matrix "
                        "pipe (split operands, ~1.8x faster on long sequences); bf16 = bf16 operands (AUC parity, log-probs to ~1e-2). "
                        "bf16 results depend on how windows are batched (<= 3e-3 in log-probs) unless --batch-invariant is given.")
    p.add_argument("--batch-invariant", action="store_true",
                   help="bf16 only: the same window gives the same bits in every batching (+4 %% on large forwards); off by default.")
    p.add_argument("--graph", action="store_true",
                   help="replay clip-sized chunks (<= 120 s) as a captured HIP graph: pays when many chunks have the same length "
                        "(--split-max-seconds), same results.")
    p.add_argument("--extended-front-end", action="store_true",
                   help="build any feature_extractor config of the checkpoint (spectrogram, mel, log-mel, mfcc at any geometry within "
                        "the limits, temporal differences); without it only the shipped log-mel is accepted")
    p.add_argument("--device-ingest", action="store_true",
                   help="average the channels and resample to 16 kHz on the GPU (the file's samples are uploaded as stored) instead "
                        "of on the host: pays for every recording that is not 16 kHz mono")
    p.add_argument("--device-post", action="store_true",
                   help="threshold, trim, frame -> sample conversion, split and segment extraction on the GPU (same results; only "
                        "the segments return to the host): pays for long recordings, a short clip is launch-bound")
    p.add_argument("--batch-chunks", action="store_true",
                   help="run the --split-max-seconds chunks of the recording through one batched prediction (one feature matrix, one "
                        "library call for the windows of all chunks) instead of one call per chunk: same results to fp32 rounding")
    p.add_argument("--batch-post", action="store_true",
                   help="with --device-post and --batch-chunks: post-process all chunks in one batched pass on the GPU (a fixed number "
                        "of launches and two synchronisations whatever the number of chunks) instead of one round per chunk: same results")
    e = sub.add_parser("evaluate", help="frame metrics over a labelled data list (vad/evaluate.py:20-29)")
    e.add_argument("eval_path", type=Path)
    e.add_argument("checkpoint_path", type=Path)
    e.add_argument("--output-path", type=Path, default=None, help="Path to store output. Default to stdout.")
    e.add_argument("--data-dir", type=Path, default=None)
    e.add_argument("--threshold", type=float, default=0.5)
    e.add_argument("--shuffle", action="store_true")
    e.add_argument("--limit", type=int, default=None)
    e.add_argument("--random-seed", type=int, default=0)
    e.add_argument("--device", default="cuda")
    e.add_argument("--extended-front-end", action="store_true",
                   help="build any feature_extractor config of the checkpoint (spectrogram, mel, log-mel, mfcc at any geometry within "
                        "the limits, temporal differences); without it only the shipped log-mel is accepted")
    e.add_argument("--device-ingest", action="store_true",
                   help="average the channels and resample to 16 kHz on the GPU (the file's samples are uploaded as stored) instead "
                        "of on the host: pays for every recording that is not 16 kHz mono")
    e.add_argument("--device-metrics", action="store_true",
                   help="compute a file's metrics on the GPU (same values; the labels go up and a few hundred bytes come back instead "
                        "of the probability matrix going down): pays for long recordings, a short clip is launch-bound")
    e.add_argument("--batch-files", type=int, default=0, metavar="K",
                   help="with --device-metrics: groups of K files of the list go through one front-end call, one batched prediction and "
                        "one metrics call (same values; the launches of a group do not grow with K)")
    e.add_argument("--precision", choices=("fp32", "fp32s", "bf16"), default="fp32", help="as for predict")
    lv = sub.add_parser("live", help="one 16 kHz WAV file fed through a live session: an event line as soon as it is final, then "
                                     "predict's JSON")
    lv.add_argument("audio_path", type=Path)
    lv.add_argument("checkpoint_path", type=Path)
    lv.add_argument("--push-ms", type=int, default=100, help="audio per push in milliseconds")
    lv.add_argument("--output-path", type=Path, default=None, help="Path to store the final output. Default to stdout.")
    lv.add_argument("--threshold", type=float, default=0.5)
    lv.add_argument("--min-vally-ms", type=int, default=0)
    lv.add_argument("--min-hill-ms", type=int, default=0)
    lv.add_argument("--hang-before-ms", type=int, default=0)
    lv.add_argument("--hang-over-ms", type=int, default=0)
    lv.add_argument("--device", default="cuda")
    lv.add_argument("--precision", choices=("fp32", "fp32s", "bf16"), default="fp32", help="as for predict")
    args = ap.parse_args(argv)

    if args.command == "evaluate":
        from .evaluate import evaluate_vad_from_scratch

        evaluate_vad_from_scratch(args.eval_path, args.checkpoint_path, args.output_path, args.data_dir, args.threshold,
                                  args.shuffle, args.limit, args.random_seed, args.device, extended_front_end=args.extended_front_end,
                                  device_ingest=args.device_ingest, device_metrics=args.device_metrics, precision=args.precision,
                                  batch_files=args.batch_files)
        return 0

    if args.command == "live":
        return live(args)

    from .predictor import VADFromScratchPredictor, VADPredictParameters

    predictor = VADFromScratchPredictor.from_checkpoint(args.checkpoint_path, args.device, extended_front_end=args.extended_front_end,
                                                        device_ingest=args.device_ingest, device_post=args.device_post,
                                                        batch_chunks=args.batch_chunks, batch_post=args.batch_post)
    predictor.model.precision, predictor.model.batch_invariant, predictor.graph = args.precision, args.batch_invariant, args.graph
    voice_activity = predictor.predict_from_path(
        args.audio_path,
        VADPredictParameters(args.split_max_seconds, args.threshold, args.min_vally_ms, args.min_hill_ms, args.hang_before_ms,
                             args.hang_over_ms, args.activity_max_sec, args.return_probs, args.probs_sample_rate, True))
    if args.output_path:
        args.output_path.parent.mkdir(parents=True, exist_ok=True)
        voice_activity.save(args.output_path)
    else:
        print(json.dumps(voice_activity.to_json(), ensure_ascii=False, indent=4))
    return 0


def live(args) -> int:
    """The file through a LiveSession in pushes of --push-ms: one JSON line per event as it becomes final (sample index and seconds),
    then the VoiceActivity JSON predict writes for the same file and parameters."""
    from datetime import timedelta

    from .clips import chunk_bounds
    from .data_models import VoiceActivity, merge_voice_activities
    from .features import SAMPLE_RATE, load_wav_mono16k
    from .live import START, LiveSession
    from .predictor import VADFromScratchPredictor, VADPredictParameters

    if args.push_ms < 1:
        raise SystemExit("--push-ms must be at least 1")
    predictor = VADFromScratchPredictor.from_checkpoint(args.checkpoint_path, args.device)
    predictor.model.precision = args.precision
    parameters = VADPredictParameters(None, args.threshold, args.min_vally_ms, args.min_hill_ms, args.hang_before_ms, args.hang_over_ms)
    audio = load_wav_mono16k(args.audio_path)
    push = SAMPLE_RATE * args.push_ms // 1000
    session = LiveSession(predictor, predictor.device, max(push, 1), post=parameters)
    activities = []

    def report():
        for kind, sample in session.events():
            print(json.dumps({"event": "start" if kind == START else "end", "sample": sample, "seconds": sample / SAMPLE_RATE}), flush=True)
        activities.extend(session.activities())

    for at in range(0, len(audio), max(push, 1)):
        session.push(audio[at:at + push])
        report()
    session.finish()
    report()
    adjusted, _ = chunk_bounds(len(audio), SAMPLE_RATE, None)
    voice_activity = merge_voice_activities([VoiceActivity(duration=timedelta(seconds=adjusted), activities=activities, probs_sample_rate=None,
                                                           probs=None)])
    if args.output_path:
        args.output_path.parent.mkdir(parents=True, exist_ok=True)
        voice_activity.save(args.output_path)
    else:
        print(json.dumps(voice_activity.to_json(), ensure_ascii=False, indent=4))
    return 0


if __name__ == "__main__":
    sys.exit(main())
