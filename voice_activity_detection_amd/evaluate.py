"""``evaluate`` command: the reference's ``python main.py evaluate`` (``vad/evaluate.py:20-190``) on the MI355X
path.  Same inputs (a JSON-lines data list of ``{"audio_path", "voice_activity_path"}`` pairs, paths relative to
``data_dir``), same per-file and total metrics under the same keys, same output file layout (first line = totals,
then one line per file).  Metrics are numpy-only restatements (``metrics.py``); sklearn is not required.

Reference quirk kept: the un-prefixed ``auc / accuracy / precision / recall`` are computed from the BOOSTED
probabilities exactly like their ``boosted_*`` twins (``vad/evaluate.py:65-68`` vs ``:72-75``); only
``vacc / sba / eba / bp / eer`` use the single-frame (middle window slot) predictions.
"""
from __future__ import annotations

import json
import random
from collections import OrderedDict
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np

from .data_models import VoiceActivity
from .metrics import EVAL_BAD_LABEL, EVAL_COUNTERS, EVAL_NAN, equal_error_rate, metrics_from_counts, precision_recall, roc_auc, vad_accuracy

METRIC_KEYS = ("auc", "accuracy", "precision", "recall", "vacc", "sba", "eba", "bp", "eer")


def load_data_list(path: Path) -> List[dict]:
    """vad/data_models/vad_data.py:38-46: one JSON object per line."""
    pairs = []
    with Path(path).open() as fh:
        for line in fh:
            if line.strip():
                d = json.loads(line)
                pairs.append({"audio_path": Path(d["audio_path"]), "voice_activity_path": Path(d["voice_activity_path"])})
    return pairs


def file_metrics(true_labels, all_frame_probabilities, threshold: float) -> "OrderedDict[str, float]":
    """vad/evaluate.py:56-80 for one file: [N, W] probabilities + label vector -> the 18 metric values."""
    p = np.asarray(all_frame_probabilities)
    y = np.asarray(true_labels)
    single = p[:, int(p.shape[1] / 2)][: len(y)]
    single_pred = single > threshold
    boosted = p.mean(axis=1)[: len(y)]
    boosted_pred = boosted > threshold
    y = y[: len(boosted)]  # (the reference would raise in sklearn on a length mismatch; labels are trimmed instead)
    auc = roc_auc(y, boosted)
    accuracy = float((y.astype(bool) == boosted_pred).mean())
    precision, recall = precision_recall(y, boosted_pred)
    vacc, _, sba, eba, bp = vad_accuracy(y, single_pred)
    eer = equal_error_rate(y, single_pred)
    bvacc, _, bsba, beba, bbp = vad_accuracy(y, boosted_pred)
    beer = equal_error_rate(y, boosted_pred)
    out = OrderedDict(auc=auc, accuracy=accuracy, precision=precision, recall=recall, vacc=vacc, sba=sba, eba=eba, bp=bp, eer=eer)
    out.update(boosted_auc=auc, boosted_accuracy=accuracy, boosted_precision=precision, boosted_recall=recall,
               boosted_vacc=bvacc, boosted_sba=bsba, boosted_eba=beba, boosted_bp=bbp, boosted_eer=beer)
    return out


BOUNDARY_HALF_WIDTH = 5   # vad_accuracy's L


def _to_host(probs):
    return probs.detach().cpu().numpy() if hasattr(probs, "detach") else np.asarray(probs)


def file_metrics_device(true_labels, probs_dev, threshold: float) -> "OrderedDict[str, float]":
    """file_metrics for probabilities that live on the GPU: [N, W] float32 tensor + label vector -> the same 18 values, bit for bit,
    without the matrix leaving the device (savad_eval_counts: the labels go up, a block of integer counters and 8 bytes per true
    segment come back; metrics.metrics_from_counts).  Falls back to file_metrics on the downloaded matrix, silently, when the
    device path does not apply: no float32 [N, W] tensor on a HIP device, savad_eval_supported says no, labels that are no
    0 .. 255 integers, or counters that report a NaN score or a label above 1."""
    import ctypes

    import torch

    from . import _lib

    y = np.asarray(true_labels)
    p = probs_dev
    if not (isinstance(p, torch.Tensor) and p.device.type == "cuda" and p.dtype == torch.float32 and p.dim() == 2):
        return file_metrics(true_labels, _to_host(p), threshold)
    N, W = int(p.shape[0]), int(p.shape[1])
    lib = _lib.load()
    labels = y.astype(np.uint8, copy=True) if y.ndim == 1 and y.dtype.kind in "biu" else None
    if labels is None or not np.array_equal(labels, y) or not lib.savad_eval_supported(W, N, len(labels)):
        return file_metrics(true_labels, _to_host(p), threshold)
    p = p.contiguous()
    n = min(N, len(labels))
    counters = np.zeros(EVAL_COUNTERS, dtype=np.int64)
    seg = np.empty(((n + 1) // 2, 8), dtype=np.uint8)
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_workspace_bytes(N, W, ctypes.byref(need)))
    with _lib.on_device(p.device):
        labels_dev = torch.from_numpy(labels).to(p.device)
        ws = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=p.device)
        count = lib.savad_eval_counts(p, N, W, labels_dev, len(labels), float(threshold), BOUNDARY_HALF_WIDTH, counters, seg, len(seg),
                                      ws, int(need.value), torch.cuda.current_stream(p.device))
    if count < 0:
        _lib.check(int(count))
    if counters[EVAL_NAN] or counters[EVAL_BAD_LABEL]:
        return file_metrics(true_labels, _to_host(p), threshold)
    return metrics_from_counts(counters, seg[:count], n)


def _report(title: str, m: dict) -> str:
    names = [("AUC", "auc"), ("Accuracy", "accuracy"), ("Precision", "precision"), ("Recall", "recall"), ("VACC", "vacc"),
             ("SBA", "sba"), ("EBA", "eba"), ("BP", "bp"), ("EER", "eer")]
    lines = ["", title]
    lines += [f"{label}: {m[key]:0.2%}" for label, key in names]
    lines += [f"Boosted {label}: {m['boosted_' + key]:0.2%}" for label, key in names]
    return "\n".join(lines) + "\n"


def evaluate_vad_from_scratch(eval_path: Path, checkpoint_path: Optional[Path] = None, output_path: Optional[Path] = None,
                              data_dir: Optional[Path] = None, threshold: float = 0.5, shuffle: bool = False,
                              limit: Optional[int] = None, random_seed: int = 0, device: str = "cuda",
                              probabilities_fn: Optional[Callable[[Path], np.ndarray]] = None, echo=print,
                              extended_front_end: bool = False, device_ingest: bool = False, device_metrics: bool = False,
                              precision: str = "fp32") -> dict:
    """Arguments as vad/evaluate.py:20-29.  `probabilities_fn(audio_path) -> [N, W]` replaces checkpoint + GPU
    predictor (host-logic tests); otherwise the audio goes WAV -> the checkpoint's front-end -> predict_probabilities on
    `device` (`extended_front_end`: VADFromScratchPredictor.from_checkpoint).  `device_ingest`: a file's samples are uploaded as
    stored, averaged over the channels and resampled to 16 kHz on the GPU (features.load_audio_device) instead of on the host.
    `device_metrics`: the probabilities stay on the GPU and a file's metrics come from file_metrics_device (same values; a
    `probabilities_fn` that returns numpy keeps the host path).  `precision`: the model's ("fp32", "fp32s", "bf16")."""
    eval_path = Path(eval_path)
    if probabilities_fn is None:
        from .features import load_audio_device, load_wav_mono16k
        from .predictor import VADFromScratchPredictor

        predictor = VADFromScratchPredictor.from_checkpoint(checkpoint_path, device, extended_front_end=extended_front_end)
        predictor.model.precision = precision

        def probabilities_fn(path):
            audio = load_audio_device(path, predictor.device) if device_ingest else load_wav_mono16k(path)
            if device_metrics:
                return predictor.predict_probabilities_device(predictor.features(audio))[0]
            return predictor.predict_probabilities(predictor.features(audio))

    data_dir = eval_path.parent if data_dir is None else Path(data_dir)
    pairs = load_data_list(eval_path)
    if shuffle:
        random.seed(random_seed)
        random.shuffle(pairs)
    if limit:
        pairs = pairs[:limit]

    results = []
    for pair in pairs:
        audio_path = data_dir.joinpath(pair["audio_path"])
        voice_activity_path = data_dir.joinpath(pair["voice_activity_path"])
        true_labels = VoiceActivity.load(voice_activity_path).to_labels(100)
        metrics = (file_metrics_device if device_metrics else file_metrics)(true_labels, probabilities_fn(audio_path), threshold)
        echo(_report(str(pair["audio_path"]), metrics))
        result = OrderedDict(audio_path=str(audio_path), voice_activity_path=str(voice_activity_path))
        result.update(metrics)
        results.append(result)

    total = {key: float(np.mean([r[key] for r in results])) for key in list(METRIC_KEYS) + ["boosted_" + k for k in METRIC_KEYS]}
    echo(_report("Total:", total))
    if output_path is not None:
        output_path = Path(output_path)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        with output_path.open("w") as fh:
            fh.write(json.dumps(total, ensure_ascii=False) + "\n")
            for r in results:
                fh.write(json.dumps(r, ensure_ascii=False) + "\n")
    return {"total": total, "files": results}
