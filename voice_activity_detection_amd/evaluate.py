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


def files_metrics_device(labels_list, probs_all, table, threshold: float, table_dev=None) -> "list[OrderedDict[str, float]]":
    """file_metrics_device for EVERY CLIP OF A BATCH through one library call (savad_eval_batch_counts): the label vectors of the
    clips, the probabilities [rows, W] of all of them on the GPU and their clip table `table` [C + 1] (`table_dev`: its device copy,
    if there is one) -> the 18-value dicts, one per clip, with the bits of file_metrics on each clip's slice.  One label upload,
    one workspace, one call; metrics_from_counts per clip.  A clip goes to file_metrics on its own downloaded slice when it
    reports a NaN score or a label above 1, has no frame in common with its labels, or has labels that are no 0 .. 255 integers;
    the other clips keep the device result.  An exception is the one the per-file loop would have raised first, in list order."""
    import ctypes

    import torch

    from . import _lib
    from .clips import check_clip_table, split_by_clip

    labels_list = list(labels_list)
    table = check_clip_table(table)
    C = len(table) - 1
    if len(labels_list) != C:
        raise ValueError(f"{len(labels_list)} label vectors for a table of {C} clips")
    p = probs_all
    slices = split_by_clip(p, table)
    if not (isinstance(p, torch.Tensor) and p.device.type == "cuda" and p.dtype == torch.float32 and p.dim() == 2):
        return [file_metrics(y, _to_host(rows), threshold) for y, rows in zip(labels_list, slices)]
    W = int(p.shape[1])
    lib = _lib.load()
    labels8 = []   # per clip: its labels as bytes, or None for what the device does not take (that clip then has no label here)
    for y in labels_list:
        y = np.asarray(y)
        as_bytes = y.astype(np.uint8, copy=True) if y.ndim == 1 and y.dtype.kind in "biu" else None
        labels8.append(as_bytes if as_bytes is not None and np.array_equal(as_bytes, y) else None)
    label_first = np.zeros(C + 1, dtype=np.int64)
    np.cumsum([0 if l is None else len(l) for l in labels8], out=label_first[1:])
    frames = np.minimum(np.diff(table.astype(np.int64)), np.diff(label_first))
    if label_first[-1] >= 2 ** 31 or frames.sum() == 0 or not lib.savad_eval_batch_supported(table, label_first.astype(np.int32), C, W):
        return [file_metrics_device(y, rows, threshold) for y, rows in zip(labels_list, slices)]
    label_first = label_first.astype(np.int32)
    labels_all = np.concatenate([l for l in labels8 if l is not None])
    p = p.contiguous()
    counters = np.zeros((C, EVAL_COUNTERS), dtype=np.int64)
    seg = np.empty((int(((frames + 1) // 2).sum()), 8), dtype=np.uint8)
    seg_first = np.zeros(C + 1, dtype=np.int64)
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_batch_workspace_bytes(table, label_first, C, W, ctypes.byref(need)))
    with _lib.on_device(p.device):
        labels_dev = torch.from_numpy(labels_all).to(p.device)
        tables_dev = torch.from_numpy(np.stack([table, label_first])).to(p.device) if table_dev is None else None
        clip_first_dev = tables_dev[0] if table_dev is None else table_dev
        label_first_dev = tables_dev[1] if table_dev is None else torch.from_numpy(label_first).to(p.device)
        ws = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=p.device)
        count = lib.savad_eval_batch_counts(p, table, clip_first_dev, labels_dev, label_first, label_first_dev, C, W, float(threshold),
                                            BOUNDARY_HALF_WIDTH, counters, seg, len(seg), seg_first, ws, int(need.value),
                                            torch.cuda.current_stream(p.device))
    if count < 0:
        _lib.check(int(count))
    out = []
    for c, (y, rows) in enumerate(zip(labels_list, slices)):
        if labels8[c] is None or frames[c] == 0 or counters[c, EVAL_NAN] or counters[c, EVAL_BAD_LABEL]:
            out.append(file_metrics(y, _to_host(rows), threshold))
        else:
            out.append(metrics_from_counts(counters[c], seg[seg_first[c]:seg_first[c + 1]], int(frames[c])))
    return out


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
                              precision: str = "fp32", batch_files: int = 0) -> dict:
    """Arguments as vad/evaluate.py:20-29.  `probabilities_fn(audio_path) -> [N, W]` replaces checkpoint + GPU
    predictor (host-logic tests); otherwise the audio goes WAV -> the checkpoint's front-end -> predict_probabilities on
    `device` (`extended_front_end`: VADFromScratchPredictor.from_checkpoint).  `device_ingest`: a file's samples are uploaded as
    stored, averaged over the channels and resampled to 16 kHz on the GPU (features.load_audio_device) instead of on the host.
    `device_metrics`: the probabilities stay on the GPU and a file's metrics come from file_metrics_device (same values; a
    `probabilities_fn` that returns numpy keeps the host path).  `precision`: the model's ("fp32", "fp32s", "bf16").
    `batch_files` = K > 1 (with `device_metrics`): consecutive groups of K files of the list go through one front-end call (where
    predict_many would make one), one batched prediction and one metrics call (files_metrics_device); same values, same echo
    order, same output file."""
    eval_path = Path(eval_path)
    batch_files = int(batch_files)
    if batch_files < 0:
        raise ValueError("batch_files must not be negative")
    if batch_files and not device_metrics:
        raise ValueError("batch_files needs device_metrics=True: only the device metrics have a batch form")
    if batch_files and probabilities_fn is not None:
        raise ValueError("batch_files runs the checkpoint's batched prediction: it cannot be combined with probabilities_fn")
    predictor = None
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

    def group_metrics(group):
        """the metrics of a group of files through one batched front-end, prediction and metrics call"""
        from .features import log_mel_many

        audios = [(load_audio_device(data_dir.joinpath(pair["audio_path"]), predictor.device) if device_ingest
                   else load_wav_mono16k(data_dir.joinpath(pair["audio_path"]))) for pair in group]
        labels = [VoiceActivity.load(data_dir.joinpath(pair["voice_activity_path"])).to_labels(100) for pair in group]
        if predictor.front_end.is_shipped and predictor.batch_front_end:
            for audio in audios:
                if len(audio) < 1:
                    raise ValueError("audio must be a non-empty 1-D array")
            feature, table, table_dev = log_mel_many(audios, predictor.device)
            probs_all = predictor._predict_matrix(feature, table, table_dev)[0]
        else:
            (probs_all, _), table = predictor._probabilities_matrix([predictor.features(audio) for audio in audios])
            table_dev = None
        return files_metrics_device(labels, probs_all, table, threshold, table_dev)

    results = []
    step = batch_files if batch_files > 1 else 1
    for at in range(0, len(pairs), step):
        group = pairs[at:at + step]
        if batch_files > 1:
            group_results = group_metrics(group)
        for k, pair in enumerate(group):
            audio_path = data_dir.joinpath(pair["audio_path"])
            voice_activity_path = data_dir.joinpath(pair["voice_activity_path"])
            if batch_files > 1:
                metrics = group_results[k]
            else:
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
