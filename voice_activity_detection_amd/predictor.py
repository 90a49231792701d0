"""Device-side mirror of the hot half of ``VADFromScratchPredictor.predict_probabilities``
(reference ``vad/predictor.py:159-262``): sliding-window gather (:180-220), model forward
(:221-224) and the boosted-prediction scatter / softmax / mean (:238-258, :95).

The feature matrix ``[N, F]`` (log-mel frames; the librosa front-end that produces it is
outside this path) is uploaded ONCE; windows are gathered, evaluated and boosted on the GPU;
only ``probs [N, W]`` (and the per-frame mean) come back.  The reference instead builds every
window in a Python loop, pushes ``[B, 7, 80]`` (7x read amplification) per chunk and scatters
with numpy on the host.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from dataclasses import dataclass
from datetime import timedelta
from typing import Optional

import numpy as np
import torch

from . import _lib
from .data_models import Activity, VoiceActivity, merge_voice_activities
from .host_feed import HostFeed, host_source
from .model import SelfAttentiveVAD
from .postprocessing import (convert_frames_to_samples, convert_samples_to_segments, optimal_split_voice_activity,
                             trim_voice_activity)


def window_offsets(half: int, jump: int) -> np.ndarray:
    """arange(-half, 0, jump) ++ [0] ++ arange(1, half+1, jump)  (vad/predictor.py:186-212)."""
    lib = _lib.load()
    w = lib.savad_window_offsets(half, jump, None)
    if w < 0:
        _lib.check(w)
    buf = (ctypes.c_int32 * w)()
    lib.savad_window_offsets(half, jump, buf)
    return np.array(buf[:w], dtype=np.int64)


def context_window_frames(half: int, jump: int) -> int:
    """W of a window geometry: the number of offsets (savad_window_offsets), which is what every kernel, gather and boost uses.
    The reference sizes its result by 2 * (half - 1) // jump + 3 (vad/predictor.py:57-59) and fills it from the offsets (:186-212);
    the two numbers differ whenever 2 * ((half - 1) % jump) >= jump (4 / 2, 9 / 3, 0 / 2 ...), where the reference itself fails with an
    IndexError: such a geometry has no reference result and is refused here."""
    half, jump = int(half), int(jump)
    W = _lib.load().savad_window_offsets(half, jump, None)
    if W < 0:
        _lib.check(W)
    formula = 2 * (half - 1) // jump + 3
    if W != formula:
        raise ValueError(f"window geometry {half} / {jump}: the reference's context_window_frames formula gives {formula} frames, its "
                         f"window offsets are {W}; the reference cannot run this geometry, so there is nothing to reproduce")
    return W


def split_by_clip_pairs(result, table) -> list:
    """(probs [sum N, W], mean [sum N]) -> [(probs of clip c, mean of clip c)]: views"""
    from .clips import split_by_clip

    return list(zip(split_by_clip(result[0], table), split_by_clip(result[1], table)))


def _require_hip(device: torch.device):
    if device.type != "cuda":
        raise _lib.SavadError("the MI355X predictor needs a HIP device (no CPU fallback)")


def _indexed(device: torch.device) -> torch.device:
    """`device` with its index spelled out ("cuda" = the current one)"""
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _require_shipped_front_end(self, what: str):
    """(a method of both predictors; `_not_shipped` is the class's message)"""
    if not self.front_end.is_shipped:
        raise NotImplementedError(self._not_shipped.format(what=what, front_end=self.front_end))


# VADFromScratchPredictor(batch_front_end=...): on, because the one-call front-end was below the per-clip one by more than the rounds'
# spread in all twelve cells of the measured table (profiles/logmel_batch_bench.json)
BATCH_FRONT_END_DEFAULT = True


@dataclass
class ContextResolution:
    """config.context_resolution of the reference (vad/configs/dataset_config.py:7-10)."""
    context_window_half_frames: int = 19
    context_window_jump_frames: int = 9


@dataclass
class VADPredictParameters:
    """vad/predictor.py:27-38 (same field order as the reference's positional construction in vad/predict.py:32-43)."""
    split_max_seconds: Optional[float] = None
    threshold: float = 0.5
    min_vally_ms: int = 0
    min_hill_ms: int = 0
    hang_before_ms: int = 0
    hang_over_ms: int = 0
    activity_max_seconds: Optional[int] = None
    return_probs: bool = False
    probs_sample_rate: Optional[int] = None
    show_progress_bar: bool = False


class VADFromScratchPredictor:
    """The reference class of the same name (vad/predictor.py:41-262) for the self-attention model:
    predict_probabilities on the GPU (log-mel, window gather, forward, boost), predict() with the
    reference's chunking and post-processing (native host code)."""

    hop_ms, window_ms = 10, 25  # the reference's only transform config (tests/configs/vad/train_config.yaml:21-22)

    def __init__(self, model: SelfAttentiveVAD, device: torch.device, context: ContextResolution = ContextResolution(),
                 chunk_size: int = 16384, graph: bool = False, graph_max_seconds: float = 120.0, graph_cache: int = 8,
                 front_end=None, device_ingest: bool = False, device_post: bool = False, batch_chunks: bool = False,
                 batch_front_end: bool = BATCH_FRONT_END_DEFAULT, batch_post: bool = False):
        """`graph=True` (not in the reference's signature): clip-sized inputs -- up to `graph_max_seconds` of audio -- run as a
        replayed HIP graph of the whole chain log-mel -> window gather -> forward -> boost, captured on first use per (length, model
        knobs) and re-captured when the weights change; at most `graph_cache` graphs are kept (least recently used goes).  For a 10 s
        clip the four launches take less time than the Python and the library calls around them: the replay halves the time per clip,
        same bits (predict_audio_device).
        `front_end` (features.FrontEnd; None = the shipped log-mel): the transform predict / predict_audio_device / evaluate run
        on the audio.  Only the shipped one has the host-upload path (predict_audio_host).
        `device_ingest=True`: predict_from_path uploads a file's samples as they are stored and averages the channels and resamples
        to 16 kHz on the GPU (features.load_audio_device) instead of on the host (features.load_wav_mono16k): the resampler has the
        bits of resampy's loop, which the host function approaches within 2e-6.
        `device_post=True`: predict() post-processes a chunk's probabilities on the GPU (postprocessing.post_frames_device /
        segments_device / sample_probs_device: row mean, threshold, trim, frame -> sample classes, optimal split, segments) and
        fetches only the segments -- the host functions' results, bit for bit -- where the geometry allows it (a hop of a whole
        number of samples, at most 128 probabilities per frame); any other chunk takes the host code.  `post_stats` counts the
        chunks either way.  Pays for long recordings (the host builds float64 arrays of one element per sample); a short clip
        is launch-bound.
        `batch_chunks=True`: predict() sends the `split_max_seconds` chunks of a recording through ONE batched prediction
        (predict_many: every chunk's features into one matrix, one library call for the windows of all chunks) instead of one
        call per chunk; the probabilities agree with the looped path to fp32 rounding (the forwards see other batches).  Off by
        default.
        `batch_front_end`: predict_many (and with it the `batch_chunks` path of predict) computes the features of all chunks in ONE
        front-end call on the clip table (features.log_mel_many: three launches and one upload whatever the number of chunks) and
        hands its device row table on to the batched prediction, instead of one log_mel call per chunk; the same bits either way.
        A custom features_fn and the extended front-ends keep the per-chunk calls.  On by default (measured: DESIGN.md section 4o).
        `batch_post=True` (with `device_post`): predict_many (and the `batch_chunks` path of predict) post-processes ALL chunks through
        one batched call (postprocessing.post_frames_device_many / segments_device_many: a fixed number of launches and two stream
        synchronisations whatever the number of chunks) instead of one `device_post` round per chunk; the same activities, integer
        for integer.  Chunks with a segment above `activity_max_seconds` go through the per-chunk split; `return_probs` stays per
        chunk.  Where the device post-processing would refuse any chunk, the per-chunk loop runs as without the flag.
        `post_batch_stats` counts the batched calls, their chunks and the chunks that were split.  Off by default."""
        from .features import SHIPPED_FRONT_END

        self.front_end = SHIPPED_FRONT_END if front_end is None else front_end
        self.device_ingest = bool(device_ingest)
        self.device_post = bool(device_post)
        self.batch_chunks = bool(batch_chunks)
        self.batch_front_end = bool(batch_front_end)
        self.batch_post = bool(batch_post)
        # batched post-processing: calls, the chunks they took, the chunks that went through the split (and which of the last call)
        self.post_batch_stats = {"calls": 0, "clips": 0, "split": 0, "last_split": []}
        self.post_stats = {"device": 0, "host": 0}   # chunks post-processed on the GPU / on the host
        self.graph, self.graph_max_seconds, self.graph_cache = bool(graph), float(graph_max_seconds), int(graph_cache)
        self._graphs: "OrderedDict[tuple, dict]" = OrderedDict()
        self.graph_stats = {"captures": 0, "replays": 0, "eager": 0}
        self.model = model
        self.device = torch.device(device)
        self.context_window_half_frames = context.context_window_half_frames
        self.context_window_jump_frames = context.context_window_jump_frames
        # vad/predictor.py:57-59, as the count of the window offsets (a geometry where the two differ is refused)
        self.context_window_frames = context_window_frames(self.context_window_half_frames, self.context_window_jump_frames)
        # windows per forward.  The reference uses 1000 (vad/predictor.py:180); windows are independent, so any value gives
        # the same probabilities up to fp32 summation order (<= 1e-6: a larger batch may pick another launch schedule), and
        # 10 min of audio take 9.4 ms with 1000 against 5.1 ms with 16384
        self.chunk_size = int(chunk_size)

    @staticmethod
    def _load_checkpoint(checkpoint_path, trust: bool):
        """torch.load restricted to tensors, containers and the numpy scalar / dtype reconstructors a reference
        checkpoint's `metrics` dict holds (weights_only=True inside safe_globals); arbitrary pickles (e.g. a checkpoint
        whose `config` is a pickled OmegaConf object) load only on explicit opt-in: trust=True or SAVAD_TRUST_CHECKPOINT=1."""
        import numpy as np
        safe = [np.dtype, np.ndarray, type(np.dtype("float64")), type(np.dtype("float32")), type(np.dtype("int64")),
                type(np.dtype("int32")), type(np.dtype("bool"))]
        for mod in ("numpy._core.multiarray", "numpy.core.multiarray"):
            try:
                m = __import__(mod, fromlist=["scalar", "_reconstruct"])
                safe += [m.scalar, m._reconstruct]
                break
            except (ImportError, AttributeError):
                continue
        import pickle

        by_env = not trust and os.environ.get("SAVAD_TRUST_CHECKPOINT") == "1"
        trusted = trust or by_env

        def full_unpickle():
            if by_env:   # a process-wide switch is easy to forget: say which file it just applied to
                import warnings
                warnings.warn(f"SAVAD_TRUST_CHECKPOINT=1: unpickling {checkpoint_path} in full (code embedded in the file can run); "
                              "prefer trust_checkpoint=True on the calls that need it", RuntimeWarning, stacklevel=3)
            try:
                return torch.load(checkpoint_path, map_location="cpu", weights_only=False)
            except TypeError:   # torch < 1.13: no weights_only keyword
                return torch.load(checkpoint_path, map_location="cpu")

        if not hasattr(torch.serialization, "safe_globals"):
            if trusted:   # an older torch: the explicit opt-in still loads (what the reference's plain torch.load does)
                return full_unpickle()
            raise RuntimeError("this torch build has no torch.serialization.safe_globals: checkpoints cannot be loaded with weights_only=True "
                               "(pass trust_checkpoint=True / set SAVAD_TRUST_CHECKPOINT=1 if you trust the file)")
        try:
            with torch.serialization.safe_globals(safe):
                return torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as exc:  # an unlisted global: only this falls through; I/O and format errors propagate as they are
            if not trusted:
                raise RuntimeError(
                    f"{checkpoint_path}: not loadable with weights_only=True ({str(exc).splitlines()[0]}). If you trust the "
                    "file, pass trust_checkpoint=True / set SAVAD_TRUST_CHECKPOINT=1 to unpickle it in full "
                    "(this can execute code embedded in the file).") from exc
        return full_unpickle()

    @classmethod
    def from_checkpoint(cls, checkpoint_path, device, trust_checkpoint: bool = False, extended_front_end: bool = False,
                        device_ingest: bool = False, device_post: bool = False, batch_chunks: bool = False,
                        batch_front_end: bool = BATCH_FRONT_END_DEFAULT, batch_post: bool = False):
        """vad/predictor.py:264-280: a training checkpoint holds {"config": ..., "state_dict": ...} plus what
        ModelCheckpointer adds (epoch, global_step, monitor_metric, a `metrics` dict of numpy scalars, optimizer /
        scheduler / grad-scaler state: vad/training/checkpointers/model_checkpointer.py:97-110); the model size, the
        feature transform and the window geometry come from the config, the weights load strictly.  Unlike the
        reference's plain torch.load, the file is first read with weights_only=True (see _load_checkpoint).
        `extended_front_end=True` builds every feature_extractor config features.FrontEnd takes (the four transforms at any
        geometry within its limits, temporal differences); the default refuses all but the shipped one.  The shipped
        features are pinned by goldens and trained-weights AUC, the others by a restatement of librosa 0.8.0: opting in
        acknowledges that.  `device_ingest`, `device_post`, `batch_chunks`, `batch_front_end`, `batch_post`: as in the constructor."""
        ckpt = cls._load_checkpoint(checkpoint_path, trust_checkpoint)
        cfg = ckpt["config"]

        def get(c, *names, default=None):
            for n in names:
                if isinstance(c, dict):
                    if n not in c:
                        return default
                    c = c[n]
                elif hasattr(c, n):
                    c = getattr(c, n)
                else:
                    return default
            return c

        if get(cfg, "model", "name") != "self-attention":
            raise NotImplementedError("only the self-attention model is built for MI355X")
        sa = get(cfg, "model", "self_attention")
        # The device front-end (savad_logmel) implements the reference's one shipped transform configuration
        # (tests/configs/vad/train_config.yaml:18-28).  Anything else would load cleanly and then produce wrong features
        # or timings, so it is refused here rather than failing late with a shape error.
        fe = get(cfg, "feature_extractor")
        if extended_front_end:
            from .features import FrontEnd

            front = FrontEnd.from_config(fe)
            feature_size, hop_ms, window_ms = front.feature_size, front.hop_ms, front.window_ms
        else:
            front = None   # the shipped one
            tr = get(fe, "transform")
            want = {"name": "log-mel", "n_fft": 512, "hop_ms": 10, "window_ms": 25, "n_mels": 80}
            got = {k: get(tr, k) for k in want}
            if got != want:
                raise NotImplementedError(f"unsupported transform {got}: the MI355X front-end implements {want} "
                                          "(vad/acoustics/transforms/transform_factory.py:30-59 has further transforms)")
            if get(fe, "temporal_differences", default=False) or get(fe, "stack_differences", default=False):
                raise NotImplementedError("unsupported feature_extractor: temporal_differences / stack_differences "
                                          "(vad/acoustics/feature_extractor.py:135-147) are not built")
            if get(fe, "silence_remover", default=None):
                raise NotImplementedError("unsupported feature_extractor: silence_remover (vad/acoustics/feature_extractor.py:115-116) is not built")
            feature_size, hop_ms, window_ms = got["n_mels"], got["hop_ms"], got["window_ms"]
        model = SelfAttentiveVAD(feature_size, get(sa, "num_layers"), get(sa, "d_model"), get(sa, "dropout"))
        model.load_state_dict(ckpt["state_dict"])
        ctx = ContextResolution(get(cfg, "context_resolution", "context_window_half_frames"),
                                get(cfg, "context_resolution", "context_window_jump_frames"))
        predictor = cls(model.to(device).eval(), device, ctx, front_end=front, device_ingest=device_ingest, device_post=device_post,
                        batch_chunks=batch_chunks, batch_front_end=batch_front_end, batch_post=batch_post)
        predictor.hop_ms, predictor.window_ms = hop_ms, window_ms  # vad/predictor.py:103-104
        return predictor

    def predict_from_path(self, audio_path, parameters: VADPredictParameters) -> VoiceActivity:
        """vad/predictor.py:71-75: AudioData.load (any channel count, any rate: averaged and resampled to 16 kHz mono) -> predict.
        The loading runs on the host (features.load_wav_mono16k), or with `device_ingest` on the GPU (features.load_audio_device:
        the raw samples are uploaded, the 16 kHz signal never visits the host)."""
        from .features import load_audio_device, load_wav_mono16k

        if self.device_ingest:
            return self.predict(load_audio_device(audio_path, self.device), parameters)
        return self.predict(load_wav_mono16k(audio_path), parameters)

    def predict(self, audio: np.ndarray, parameters: VADPredictParameters, features_fn=None) -> VoiceActivity:
        """vad/predictor.py:77-157.  audio: float32 mono @16 kHz, a numpy array or a 1-D float32 tensor on the predictor's device
        (sliced and fed to the front-end where it is: no host round trip).  features_fn(chunk_audio) -> [N, F] overrides
        the GPU front-end (used by the parity tests to feed the reference's feature matrix)."""
        from .clips import chunk_bounds
        from .features import SAMPLE_RATE

        if self.batch_chunks:
            return self.predict_many([audio], parameters, features_fn)[0]
        if not (isinstance(audio, torch.Tensor) and audio.device.type == "cuda" and audio.dtype == torch.float32 and audio.dim() == 1):
            audio = np.asarray(audio, dtype=np.float32)
        adjusted, bounds = chunk_bounds(len(audio), SAMPLE_RATE, parameters.split_max_seconds)
        def chunk_probs():
            for start_sample, end_sample in bounds:
                chunk = audio[start_sample:end_sample]
                if features_fn is not None:
                    yield self.predict_probabilities_device(features_fn(chunk))[0]
                else:
                    yield self.predict_audio_device(chunk)[0]   # (a replayed HIP graph for clip-sized chunks when graph=True)

        return self._voice_activity(adjusted, (self._post(probs_dev, parameters) for probs_dev in chunk_probs()), parameters)

    def _voice_activity(self, adjusted, posted, parameters: VADPredictParameters) -> VoiceActivity:
        """a recording's VoiceActivity from the post-processed (activities, probs) of its chunks, taken as they arrive (vad/predictor.py:120-157)"""
        chunks = []
        for activities, probs in posted:
            chunks.append(VoiceActivity(duration=timedelta(seconds=adjusted), activities=activities,
                                        probs_sample_rate=parameters.probs_sample_rate if parameters.return_probs else None,
                                        probs=probs))
        return merge_voice_activities(chunks)

    def _post(self, probs_dev, parameters: VADPredictParameters):
        """a chunk's probabilities -> (activities, probs): on the GPU where `device_post` asks for it and the geometry allows it"""
        if self.device_post and self._device_post_applies(probs_dev, parameters):
            self.post_stats["device"] += 1
            return self._post_device(probs_dev, parameters)
        self.post_stats["host"] += 1
        return self._post_host(probs_dev, parameters)

    def predict_many(self, audios, parameters: VADPredictParameters, features_fn=None) -> "list[VoiceActivity]":
        """predict() for a LIST of recordings (each as predict takes it) -> their VoiceActivity, in order, through one batched
        prediction: every recording is cut into its `split_max_seconds` chunks (clips.chunk_bounds: predict's own), every chunk's
        front-end writes its rows of ONE feature matrix (one call for all chunks with `batch_front_end`, else per-chunk launches), the
        windows of all chunks of all recordings run in one library call (predict_probabilities_many), and each chunk's slice is
        post-processed as predict does it -- chunk by chunk, or with `batch_post` (and `device_post`) all chunks in one batched call."""
        from .clips import chunk_bounds, clip_table, split_by_clip
        from .features import SAMPLE_RATE, log_mel, log_mel_many

        _require_hip(self.device)
        dev = _indexed(self.device)
        pieces, plan = [], []   # every chunk of every recording; per recording: (seconds per chunk, its chunks' indices)
        for audio in audios:
            if not (isinstance(audio, torch.Tensor) and audio.device.type == "cuda" and audio.dtype == torch.float32 and audio.dim() == 1):
                audio = np.asarray(audio, dtype=np.float32)
            adjusted, bounds = chunk_bounds(len(audio), SAMPLE_RATE, parameters.split_max_seconds)
            plan.append((adjusted, range(len(pieces), len(pieces) + len(bounds))))
            pieces += [audio[a:b] for a, b in bounds]
        if not pieces:
            return []
        if features_fn is None and self.front_end.is_shipped:
            for piece in pieces:
                if len(piece) < 1:
                    raise ValueError("audio must be a non-empty 1-D array")
            if self.batch_front_end:
                feature, table, table_dev = log_mel_many(pieces, dev)
            else:
                table, table_dev = clip_table(1 + len(piece) // 160 for piece in pieces), None
                feature = torch.empty((int(table[-1]), self.front_end.feature_size), dtype=torch.float32, device=dev)
                for piece, rows in zip(pieces, split_by_clip(feature, table)):
                    log_mel(piece, dev, out=rows)
            probs_all = self._predict_matrix(feature, table, table_dev)[0]
        else:
            (probs_all, _), table = self._probabilities_matrix([features_fn(piece) if features_fn is not None else self.features(piece)
                                                                for piece in pieces])
            table_dev = None
        return self._voice_activities(probs_all, table, table_dev, plan, parameters)

    def _voice_activities(self, probs_all, table, table_dev, plan, parameters: VADPredictParameters) -> "list[VoiceActivity]":
        """the probabilities [sum N, W] of all chunks -> one VoiceActivity per recording of `plan` [(seconds per chunk, its chunks'
        indices)]: every chunk post-processed on its own, or (`batch_post` with `device_post`, where the device takes every chunk)
        all of them in one batched call"""
        from .clips import split_by_clip

        chunk_probs = split_by_clip(probs_all, table)
        if self.batch_post and self.device_post and all(self._device_post_applies(p, parameters) for p in chunk_probs):
            posted = self._post_device_many(probs_all, table, table_dev, parameters)
            return [self._voice_activity(adjusted, (posted[i] for i in indices), parameters) for adjusted, indices in plan]
        return [self._voice_activity(adjusted, (self._post(chunk_probs[i], parameters) for i in indices), parameters) for adjusted, indices in plan]

    @torch.no_grad()
    def _predict_matrix(self, feature, table, table_dev=None):
        """(probs [sum N, W], mean [sum N]) of a concatenated device matrix and its clip table (and the table's device copy, if there is one)"""
        self.model.eval()
        return self.model.predict_windows_batch(feature, table, self.context_window_half_frames, self.context_window_jump_frames,
                                                self.chunk_size, table_dev)

    @torch.no_grad()
    def predict_probabilities_many(self, features) -> "list[tuple]":
        """predict_probabilities_device for a LIST of [N_c, F] feature matrices (numpy or tensor; an empty one is legal) in one
        library call -> [(probs [N_c, W], mean [N_c])] on the device: views of one result, clip by clip."""
        feats = list(features)
        if not feats:
            return []
        result, table = self._probabilities_matrix(feats)
        return split_by_clip_pairs(result, table)

    @torch.no_grad()
    def _probabilities_matrix(self, features):
        """((probs [sum N, W], mean [sum N]), clip table) of a non-empty list of [N_c, F] feature matrices: one library call"""
        from .clips import clip_table

        _require_hip(self.device)
        dev = _indexed(self.device)
        feats = [torch.as_tensor(f, dtype=torch.float32).to(dev) for f in features]
        for f in feats:
            if f.dim() != 2 or f.shape[1] != self.model.feature_size:
                raise ValueError(f"every feature matrix must be [N, {self.model.feature_size}], got {tuple(f.shape)}")
        table = clip_table(f.shape[0] for f in feats)
        feature = feats[0].contiguous() if len(feats) == 1 else torch.cat(feats, dim=0)
        return self._predict_matrix(feature, table), table

    def _post_host(self, probs_dev, parameters: VADPredictParameters):
        """probs [N, W] on the device -> (activities, probs list or None) on the host: vad/predictor.py:95-141"""
        # float64 mean of the float32 [N, 7] matrix, like numpy's probs.mean(axis=1) on the host (:95)
        boosted = probs_dev.cpu().numpy().mean(axis=1)
        predictions = boosted > parameters.threshold
        hop_ms, window_ms = self.hop_ms, self.window_ms
        trimmed = trim_voice_activity(predictions, min_vally=round(parameters.min_vally_ms / hop_ms),
                                      min_hill=round(parameters.min_hill_ms / hop_ms),
                                      hang_before=round(parameters.hang_before_ms / hop_ms),
                                      hang_over=round(parameters.hang_over_ms / hop_ms))
        sample_predictions = convert_frames_to_samples(trimmed, sample_rate=16000, hop_ms=hop_ms, window_ms=window_ms)
        if parameters.activity_max_seconds is not None and parameters.activity_max_seconds > 0:
            sample_full_probs = convert_frames_to_samples(boosted, sample_rate=16000, hop_ms=hop_ms, window_ms=window_ms)
            sample_predictions = optimal_split_voice_activity(sample_predictions, sample_full_probs,
                                                              max_length_seconds=parameters.activity_max_seconds,
                                                              sample_rate=16000)
        activities = [Activity(start=a, end=b) for a, b in convert_samples_to_segments(sample_predictions, 16000)]
        probs = None
        if parameters.return_probs:
            probs = convert_frames_to_samples(boosted, sample_rate=parameters.probs_sample_rate, hop_ms=hop_ms,
                                              window_ms=window_ms).tolist()
        return activities, probs

    def _device_post_applies(self, probs_dev, parameters: VADPredictParameters) -> bool:
        """the conditions of the device post-processing for this chunk (host arithmetic): both geometries in use -- 16 kHz, and
        probs_sample_rate when the probabilities are returned -- have a whole hop, the split length is one the host accepts"""
        from .postprocessing import device_post_supported

        N, W = int(probs_dev.shape[0]), int(probs_dev.shape[1])
        hop_ms, window_ms = self.hop_ms, self.window_ms
        if probs_dev.device.type != "cuda" or not device_post_supported(W, 16000, hop_ms, window_ms, N):
            return False
        if parameters.return_probs and not device_post_supported(W, parameters.probs_sample_rate, hop_ms, window_ms, N):
            return False
        if min(parameters.min_vally_ms, parameters.min_hill_ms, parameters.hang_before_ms, parameters.hang_over_ms) < 0:
            return False
        amax = parameters.activity_max_seconds
        return not (amax is not None and amax > 0 and int(amax * 16000) < 2)

    def _post_device(self, probs_dev, parameters: VADPredictParameters):
        """_post_host's results from the GPU: only the segment indices (and the probability samples, when asked for) come back"""
        from .postprocessing import post_frames_device, segments_device

        hop_ms, window_ms = self.hop_ms, self.window_ms
        boosted, trimmed = post_frames_device(probs_dev, parameters.threshold, **self._trim_frames(parameters))
        amax = parameters.activity_max_seconds
        starts, ends = segments_device(trimmed, boosted, sample_rate=16000, hop_ms=hop_ms, window_ms=window_ms,
                                       max_length_seconds=amax if amax is not None and amax > 0 else None)
        return self._device_result(starts, ends, boosted, parameters)

    def _trim_frames(self, parameters: VADPredictParameters) -> dict:
        """the trim parameters in frames (vad/predictor.py:99-104)"""
        hop_ms = self.hop_ms
        return dict(min_vally=round(parameters.min_vally_ms / hop_ms), min_hill=round(parameters.min_hill_ms / hop_ms),
                    hang_before=round(parameters.hang_before_ms / hop_ms), hang_over=round(parameters.hang_over_ms / hop_ms))

    def _post_device_many(self, probs_all, table, table_dev, parameters: VADPredictParameters) -> list:
        """_post_device for every chunk of a batch through ONE batched call: [(activities, probs)] in chunk order"""
        from .clips import split_by_clip
        from .postprocessing import post_frames_device_many, segments_device_many

        hop_ms, window_ms = self.hop_ms, self.window_ms
        boosted, trimmed = post_frames_device_many(probs_all, table, table_dev, parameters.threshold, **self._trim_frames(parameters))
        amax = parameters.activity_max_seconds
        seg_first, starts, ends, split = segments_device_many(trimmed, table, table_dev, boosted, sample_rate=16000, hop_ms=hop_ms, window_ms=window_ms,
                                                              max_length_seconds=amax if amax is not None and amax > 0 else None, return_long=True)
        chunks = len(table) - 1
        self.post_stats["device"] += chunks
        stats = self.post_batch_stats
        stats["calls"] += 1
        stats["clips"] += chunks
        stats["last_split"] = [int(c) for c in np.flatnonzero(split)]
        stats["split"] += len(stats["last_split"])
        return [self._device_result(starts[a:b], ends[a:b], rows, parameters)
                for a, b, rows in zip(seg_first[:-1], seg_first[1:], split_by_clip(boosted, table))]

    def _device_result(self, starts, ends, boosted, parameters: VADPredictParameters):
        """(activities, probs) of a chunk from its segments' sample indices and its boosted probabilities on the device"""
        from .postprocessing import sample_probs_device

        hop_ms, window_ms = self.hop_ms, self.window_ms
        # (times as convert_samples_to_segments builds them)
        activities = [Activity(start=timedelta(seconds=int(a) / 16000), end=timedelta(seconds=int(b) / 16000)) for a, b in zip(starts, ends)]
        probs = None
        if parameters.return_probs:
            probs = sample_probs_device(boosted, sample_rate=parameters.probs_sample_rate, hop_ms=hop_ms, window_ms=window_ms).cpu().numpy().tolist()
        return activities, probs

    def predict_probabilities(self, feature) -> np.ndarray:
        """feature [N, F] (numpy or tensor) -> positive-class probabilities [N, W] (float32 numpy),
        exactly the array the reference returns from predict_probabilities (:257-260)."""
        probs, _ = self.predict_probabilities_device(feature)
        return probs.cpu().numpy()

    def predict_boosted(self, feature) -> np.ndarray:
        """Per-frame boosted probability = probs.mean(axis=1) (vad/predictor.py:95)."""
        _, mean = self.predict_probabilities_device(feature)
        return mean.cpu().numpy()

    @torch.no_grad()
    def predict_probabilities_device(self, feature):
        """feature [N, F] -> (probs [N, W], mean [N]) on the device: window gather (a13), forward, boosted prediction (a14)
        in one library call (savad_predict_probabilities)."""
        _require_hip(self.device)
        feat = torch.as_tensor(feature, dtype=torch.float32).to(self.device)
        if feat.dim() != 2:
            raise ValueError("feature must be [N, F]")
        self.model.eval()
        return self.model.predict_windows(feat, self.context_window_half_frames, self.context_window_jump_frames, self.chunk_size)

    def features(self, audio) -> torch.Tensor:
        """audio -> the [N, F] feature matrix of self.front_end on the predictor's device"""
        from .features import log_mel

        if self.front_end.is_shipped:
            return log_mel(audio, self.device)
        return self.front_end.extract(audio, self.device)

    _require_shipped_front_end = _require_shipped_front_end
    _not_shipped = ("{what} runs the shipped log-mel front-end only (its spans follow the 160-sample hop, and MFCC's clamp and the "
                    "temporal differences are not local): {front_end} is not; use predict_audio_device")

    @torch.no_grad()
    def predict_audio_device(self, audio):
        """audio: 1-D float32 mono @16 kHz (numpy or tensor) -> (probs [N, W], mean [N]) on the device, N = 1 + len // 160: the GPU
        log-mel front-end (vad/acoustics/transforms/log_mel_spectrogram.py:19-32) followed by predict_probabilities_device
        (vad/predictor.py:159-262) -- what `predict` runs per chunk.  With `graph=True` a clip-sized input replays a captured HIP
        graph (same kernels, same bits); the returned tensors then belong to the graph and are overwritten by the next call with
        the same length and knobs: copy them if they must outlive it."""
        from .features import SAMPLE_RATE

        _require_hip(self.device)
        n = int(audio.shape[0]) if hasattr(audio, "shape") and len(audio.shape) == 1 else -1
        if not self.graph or n < 1 or n > self.graph_max_seconds * SAMPLE_RATE or self.model.training:
            self.graph_stats["eager"] += 1
            return self.predict_probabilities_device(self.features(audio))
        model = self.model
        dev = _indexed(self.device)
        with _lib.on_device(dev):
            model._prepare_call(dev)   # weights pushed, knobs set: the walk over the parameters' versions costs ~8 us
            key = (n, dev.index, model._pushed_knobs, self.context_window_half_frames, self.context_window_jump_frames, self.chunk_size,
                   self.front_end)
            entry = self._graphs.get(key)
            if entry is not None and entry["weights"] is not model._synced_versions:
                # the weights were pushed again since the capture: the library re-folds / re-packs them inside its NEXT call, which a
                # replay never makes -- every graph of this predictor is stale
                self._graphs.clear()
                entry = None
            if entry is None:
                entry = self._capture(key, n, dev)
            else:
                self._graphs.move_to_end(key)
            src = audio if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
            entry["audio"].copy_(src, non_blocking=True)
            entry["graph"].replay()
            self.graph_stats["replays"] += 1
        return entry["probs"], entry["mean"]

    @staticmethod
    def host_chunk_plan(N: int, half: int, W: int, frames_per_chunk: int):
        """[(f0, f1, g0, g1)]: output frames [f0, f1) of an N-frame recording are computed from feature frames [g0, g1).  A frame's W
        probabilities come from the windows centred within `half` of it (vad/predictor.py:238-258), a window reads the frames within
        `half` of its centre (:186-212): 2 x half frames of halo per side, clipped to the recording -- where the slice is clipped, the
        windows that are missing are exactly the ones the whole recording lacks there (the 0.5 placeholders).  g0 is a multiple of
        32 // W, so that every window keeps its slot in a packed 32-row block (the single-launch kernels sum a slot's keys in slot order);
        a tail shorter than half a chunk rides with the chunk before it (a tiny last chunk would run another kernel variant).
        Host-side arithmetic only."""
        G = max(32 // W, 1)
        per = max(int(frames_per_chunk), 4 * half)
        starts = list(range(0, N, per))
        if len(starts) > 1 and N - starts[-1] < per // 2:
            starts.pop()
        plan = []
        for k, f0 in enumerate(starts):
            f1 = starts[k + 1] if k + 1 < len(starts) else N
            plan.append((f0, f1, max(0, f0 - 2 * half) // G * G, min(N, f1 + 2 * half)))
        return plan

    @staticmethod
    def host_upload_plan(n_in: int, rate: int, half: int, W: int, frames_per_chunk: int):
        """(n, [(f0, f1, g0, g1, first, count, have)]) for a recording of n_in frames at `rate` Hz, n samples at 16 kHz: host_chunk_plan
        of its N = 1 + n // 160 frames, the 16 kHz samples [first, first + count) a chunk's feature frames read (span_samples), and the
        raw frames [0, have) the 16 kHz signal up to the chunk's last sample is interpolated from (resample_span_samples; at 16 kHz
        that signal itself).  Host-side arithmetic only."""
        from .features import SAMPLE_RATE, resample_length, resample_span_samples, span_samples

        n = resample_length(n_in, rate)
        if n < 1:
            raise ValueError("audio must be a non-empty array")
        plan = []
        for f0, f1, g0, g1 in VADFromScratchPredictor.host_chunk_plan(1 + n // 160, half, W, frames_per_chunk):
            first, count = span_samples(n, g0, g1 - g0)
            have = first + count if rate == SAMPLE_RATE else sum(resample_span_samples(n_in, rate, 0, first + count))
            plan.append((f0, f1, g0, g1, first, count, have))
        return n, plan

    @torch.no_grad()
    def predict_audio_host(self, audio, frames_per_chunk: int = 65536, sample_rate: int = 16000, channels: int = 1):
        """The reference's mode END TO END from host memory: `audio` = the whole recording on the host, 16-bit PCM
        (uploaded as it is, converted on the device) or float32, numpy array or CPU tensor (pinned: asynchronous uploads) ->
        (probs [N, W], mean [N]) on the device.  Output frames are produced in chunks of `frames_per_chunk`; chunk c needs the feature
        frames within 2 x half of its own (every window that reaches one of its frames, vad/predictor.py:186-258), whose samples are
        uploaded on a copy stream while chunk c - 1 runs (host_feed.HostFeed).  A chunk's first window keeps its place modulo the
        packed block (a multiple of 32 // W windows), so the results are predict_audio_device's bits.
        `sample_rate`, `channels`: the recording as a file holds it -- `audio` is then the interleaved 1-D sample stream at that rate
        (features.read_audio), and a chunk uploads the raw frames its 16 kHz samples are interpolated from; on the device they are
        averaged over the channels (downmix_device) and resampled (resample_span_device) into a 16 kHz signal that grows chunk by
        chunk: the bits of predict_audio_device(resample_to_16k_device(downmix_device(audio))).  A stage the recording does not need
        is skipped: the average for float32 mono (16-bit mono is converted by it: the average of one channel), the resampling at
        16 kHz."""
        from .features import SAMPLE_RATE, downmix_device, log_mel_span, resample_prepare, resample_span_device, resample_span_samples

        _require_hip(self.device)
        self._require_shipped_front_end("predict_audio_host")
        src = host_source(audio)
        rate, channels = int(sample_rate), int(channels)
        if channels < 1 or src.numel() % channels:
            raise ValueError(f"{src.numel()} samples are not whole frames of {channels} channels")
        n_in = src.numel() // channels
        half, jump, Wn = self.context_window_half_frames, self.context_window_jump_frames, self.context_window_frames
        n, plan = self.host_upload_plan(n_in, rate, half, Wn, frames_per_chunk)
        N = 1 + n // 160
        self.model.eval()
        dev = _indexed(self.device)
        with _lib.on_device(dev):
            if rate != SAMPLE_RATE:
                resample_prepare(rate, dev)        # (the table upload synchronises: before the first copy is in flight)
            feed = HostFeed(src, dev, unit=channels, stream_owner=self)
            plain = channels == 1 and src.dtype == torch.float32          # the raw buffer already is the mono signal
            mono = feed.buffer if plain else torch.empty(n_in, dtype=torch.float32, device=dev)
            audio16 = mono if rate == SAMPLE_RATE else torch.empty(n, dtype=torch.float32, device=dev)
            probs = torch.empty((N, Wn), dtype=torch.float32, device=dev)
            mean = torch.empty((N,), dtype=torch.float32, device=dev)
            mixed = done16 = 0                     # frames averaged; 16 kHz samples produced
            for c in feed.chunks([(0, p[6]) for p in plan]):   # (both stages are cumulative: a chunk needs the recording up to `have`)
                f0, f1, g0, g1, first, count, have = plan[c]
                if not plain and have > mixed:
                    downmix_device(feed.buffer[mixed * channels:have * channels], channels, out=mono[mixed:have])
                    mixed = have
                end16 = first + count
                if rate != SAMPLE_RATE and end16 > done16:
                    need_first, _ = resample_span_samples(n_in, rate, done16, end16 - done16)
                    resample_span_device(mono[need_first:have], need_first, n_in, rate, done16, end16 - done16, out=audio16[done16:end16])
                    done16 = end16
                feat = log_mel_span(audio16[first:end16], first, n, g0, g1 - g0)
                p, mu = self.model.predict_windows(feat, half, jump, self.chunk_size)
                probs[f0:f1].copy_(p[f0 - g0:f1 - g0])
                mean[f0:f1].copy_(mu[f0 - g0:f1 - g0])
        return probs, mean

    def _capture(self, key, n: int, dev: torch.device) -> dict:
        from .features import log_mel

        static_audio = torch.zeros(n, dtype=torch.float32, device=dev)
        front = self.front_end
        if not front.is_shipped:
            front.prepare(dev)   # its tables reach the device before the capture (the capture may only launch kernels)

        def chain():
            feat = log_mel(static_audio, dev) if front.is_shipped else front.extract(static_audio, dev)
            return self.model.predict_windows(feat, self.context_window_half_frames, self.context_window_jump_frames, self.chunk_size)

        # eager runs first, on a side stream like the capture itself: positional-encoding table, packed weights and the cached
        # workspace reach their final sizes, so that the captured call launches nothing but its own kernels
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                chain()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            probs, mean = chain()
        entry = {"graph": g, "audio": static_audio, "probs": probs, "mean": mean, "weights": self.model._synced_versions,
                 "workspace": self.model._workspace}   # (the graph holds the workspace's address: keep the block alive)
        self._graphs[key] = entry
        while len(self._graphs) > max(self.graph_cache, 1):
            self._graphs.popitem(last=False)
        self.graph_stats["captures"] += 1
        return entry

    @torch.no_grad()
    def predict_probabilities_device_stepwise(self, feature):
        """The same through the three separate entry points (savad_gather_windows, savad_forward, savad_boost): what
        savad_predict_probabilities must reproduce bit for bit (tests)."""
        lib = _lib.load()
        feat = torch.as_tensor(feature, dtype=torch.float32).to(self.device).contiguous()
        N, F = feat.shape
        half, jump, W = self.context_window_half_frames, self.context_window_jump_frames, self.context_window_frames
        data_length = N - 2 * half  # vad/predictor.py:169
        self.model.eval()
        with _lib.on_device(self.device):
            stream = torch.cuda.current_stream(self.device)
            n_items = max(data_length, 0)
            logp = torch.empty((n_items, W, 2), dtype=torch.float32, device=self.device)
            pos = torch.empty((n_items, W), dtype=torch.int64, device=self.device)
            for first in range(0, n_items, self.chunk_size):
                count = min(self.chunk_size, n_items - first)
                win = torch.empty((count, W, F), dtype=torch.float32, device=self.device)
                _lib.check(lib.savad_gather_windows(feat, N, F, half, jump, first, count, win, pos[first:first + count], stream))
                self.model(features=win, out=logp[first:first + count])  # straight into the boost's input
            probs = torch.empty((N, W), dtype=torch.float32, device=self.device)
            mean = torch.empty((N,), dtype=torch.float32, device=self.device)
            if N > 0:
                boosted = torch.empty((N, W, 2), dtype=torch.float32, device=self.device)
                _lib.check(lib.savad_boost(logp, pos, n_items, N, W, boosted, probs, mean, stream))
        return probs, mean


class StreamingPredictor:
    """Long-form mode of BASELINE.json configs[4]: sliding windows of T frames every `hop` frames over
    a long feature matrix [N, F]; each window is one sequence of the self-attentive model; per-frame
    speech probability = mean over the (<= T/hop) windows covering the frame.  Not a mode of the
    reference (its predictor only cuts 7-frame windows); semantics defined in include/savad.h.
    With torch.distributed initialised, windows are sharded contiguously over the ranks and the
    log-probs are exchanged with ONE all_gather (voice_activity_detection_amd.distributed)."""

    def __init__(self, model: SelfAttentiveVAD, device, T: int = 800, hop: int = 400, max_batch: int = 256, in_flight: int = 2,
                 front_end=None):
        # front_end (features.FrontEnd): the audio paths (audio_span_logp, predict_audio_device, predict_audio_host) cut the signal
        # at the shipped log-mel's 160-sample hop and compute features per span: they refuse any other front-end; predict_device
        # takes features of any front-end
        from .features import SHIPPED_FRONT_END

        self.front_end = SHIPPED_FRONT_END if front_end is None else front_end
        self.model, self.device, self.T, self.hop, self.max_batch = model, torch.device(device), int(T), int(hop), int(max_batch)
        # the window batches are independent: `in_flight` of them run concurrently (PipelinedVAD: own stream / handle / workspace
        # each, same bits); 1 = one after the other on the caller's stream.
        # bf16 operands: a full batch of max_batch windows and a smaller remainder (or a rank's smaller shard) may run different attention
        # kernels, whose results differ in the bf16 rounding of a few rows' context (<= 3e-3 in the log-probs); set
        # model.batch_invariant = True where the same window must give the same bits in every batching (+4 % of a large forward)
        self.in_flight = int(in_flight)
        self._pipe = None

    @torch.no_grad()
    def predict_device(self, feature):
        from .distributed import sharded_rows

        feat = torch.as_tensor(feature, dtype=torch.float32).to(self.device).contiguous()
        N, F = feat.shape
        W = self._window_count(N, self.T, self.hop)
        self.model.eval()
        with _lib.on_device(self.device):
            self._ensure_pipe()

            def windows_logp(lo, hi):  # this rank's contiguous span of windows -> [hi - lo, T, 2] log-probs
                return self._windows_logp(feat, 0, N, lo, hi)

            logp = sharded_rows(W, windows_logp, (self.T, 2), torch.float32, self.device).contiguous()
            return self._merge(logp, W, N)

    @staticmethod
    def _window_count(N: int, T: int, hop: int) -> int:
        W = _lib.load().savad_stream_window_count(N, T, hop)
        if W < 0:
            _lib.check(W)
        return W

    def _ensure_pipe(self):
        if self._pipe is None or self._pipe.model is not self.model or self._pipe.depth != max(self.in_flight, 1):
            from .pipeline import PipelinedVAD
            self._pipe = PipelinedVAD(self.model, depth=max(self.in_flight, 1))

    def _merge(self, logp, W: int, N: int):
        """the windows' log-probs [W, T, 2] -> per-frame probabilities [N] (savad_overlap_merge on the current stream)"""
        probs = torch.empty((N,), dtype=torch.float32, device=logp.device)
        _lib.check(_lib.load().savad_overlap_merge(logp, W, N, self.T, self.hop, probs, torch.cuda.current_stream(logp.device)))
        return probs

    def _windows_logp(self, feat, frame0, n_total, lo, hi, out=None, join=True):
        """log-probs [hi - lo, T, 2] of windows [lo, hi) of an n_total-frame recording, from `feat` = its frames [frame0,
        frame0 + len(feat)): windows that lie inside the recording are read IN PLACE (model.forward_windows, sequences hop * F
        elements apart: no copies); the last window of a recording that does not end on a window boundary is zero-padded
        through savad_gather_strided (one window's copy)."""
        lib = _lib.load()
        T, hop, F = self.T, self.hop, feat.shape[1]
        n_local = feat.shape[0]
        local = out if out is not None else torch.empty((hi - lo, T, 2), dtype=torch.float32, device=self.device)
        full_end = min(hi, (n_total - T) // hop + 1 if n_total >= T else 0)   # windows [lo, full_end) end inside the recording
        for first in range(lo, full_end, self.max_batch):
            count = min(self.max_batch, full_end - first)
            self._pipe.submit_windows(feat, T, hop, first - frame0 // hop, count, out=local[first - lo:first - lo + count])
        for w in range(max(lo, full_end), hi):   # at most one: the padded tail
            if F % 4:   # (savad_gather_strided moves 16-byte pieces)
                win = torch.zeros((1, T, F), dtype=torch.float32, device=self.device)
                f_lo = hop * (w - frame0 // hop)
                win[0, :max(min(T, n_local - f_lo), 0)] = feat[f_lo:f_lo + T]
            else:
                win = torch.empty((1, T, F), dtype=torch.float32, device=self.device)
                _lib.check(lib.savad_gather_strided(feat, n_local, F, T, hop, w - frame0 // hop, 1, win, torch.cuda.current_stream(self.device)))
            self._pipe.submit(win, out=local[w - lo:w - lo + 1])
        if join:
            self._pipe.join()
        return local

    @staticmethod
    def audio_shard_plan(n_samples: int, T: int, hop: int, rank: int, world: int):
        """What rank `rank` of `world` needs of an n_samples-long recording: (W, lo, hi, f0, f1, first, count) -- its windows [lo, hi)
        of the W in all (contiguous split, voice_activity_detection_amd.distributed.shard_bounds), the feature frames [f0, f1)
        they cover, and the samples [first, first + count) those frames read (savad_logmel_span_samples: 208 samples of halo
        per side, the mirrored stretch at an end of the recording; first % 4 == 0).  Host-side arithmetic only."""
        from .distributed import shard_bounds
        from .features import span_samples

        lib = _lib.load()
        N = 1 + n_samples // 160
        W = lib.savad_stream_window_count(N, T, hop)
        if W < 0:
            _lib.check(W)
        lo, hi = shard_bounds(W, rank, world)
        if hi <= lo:
            return W, lo, hi, 0, 0, 0, 0
        f0, f1 = hop * lo, min(N, hop * (hi - 1) + T)
        first, count = span_samples(n_samples, f0, f1 - f0)
        return W, lo, hi, f0, f1, first, count

    @torch.no_grad()
    def audio_span_logp(self, audio, rank: int, world: int):
        """rank-local half of predict_audio_device: log-probs [hi - lo, T, 2] of this rank's windows, from the audio -- only its
        slice of the samples is uploaded (when `audio` is a host array), only its frames' log-mel is computed"""
        from .features import log_mel_span

        self._require_shipped_front_end("audio_span_logp")
        n = int(audio.shape[0])
        W, lo, hi, f0, f1, first, count = self.audio_shard_plan(n, self.T, self.hop, rank, world)
        if hi <= lo:
            return torch.zeros((0, self.T, 2), dtype=torch.float32, device=self.device)
        self.model.eval()
        with _lib.on_device(self.device):
            self._ensure_pipe()
            sl = audio[first:first + count]
            if not isinstance(sl, torch.Tensor):
                sl = torch.from_numpy(np.ascontiguousarray(sl) if sl.dtype == np.int16 else np.ascontiguousarray(sl, dtype=np.float32))
            if sl.dtype == torch.int16:   # 16-bit PCM goes up as it is (half the bytes) and is converted on the device
                from .features import pcm16_to_f32
                sl = pcm16_to_f32(sl.to(self.device).contiguous())
            else:
                sl = sl.to(self.device, torch.float32).contiguous()
            feat = log_mel_span(sl, first, n, f0, f1 - f0)
            return self._windows_logp(feat, f0, 1 + n // 160, lo, hi)

    @torch.no_grad()
    def predict_audio_device(self, audio):
        """configs[4] from the AUDIO: `audio` = the whole recording, mono 16 kHz, float32 or 16-bit PCM (uploaded as it is, converted on the
        device), on the HOST (numpy) or the device.  With
        torch.distributed initialised every rank computes the log-mel features of ITS window span only (audio_shard_plan), runs
        its windows in place on them, and ONE all_gather of the log-probs + the overlap merge give every rank the per-frame
        probabilities.  Same bits as predict_device(log_mel(audio)) on one GPU (tests/test_gpu_parity.py)."""
        import torch.distributed as dist

        from .distributed import all_gather_rows

        self._require_shipped_front_end("predict_audio_device")
        N = 1 + int(audio.shape[0]) // 160
        world, rank = (dist.get_world_size(), dist.get_rank()) if dist.is_initialized() else (1, 0)
        local = self.audio_span_logp(audio, rank, world)
        W = self._window_count(N, self.T, self.hop)
        with _lib.on_device(self.device):
            return self._merge((all_gather_rows(local, W) if world > 1 else local).contiguous(), W, N)

    _host_source = staticmethod(host_source)   # (the name scripts and callers knew it by)

    @staticmethod
    def host_span_plan(n_samples: int, T: int, hop: int, per: int, ramp: bool):
        """[(lo, hi, f0, f1, first, count)], in the order predict_audio_host takes them: windows [lo, hi) of an n_samples-long
        recording, `per` to a span, the feature frames [f0, f1) they cover and the samples [first, first + count) those read
        (span_samples).  Without `ramp` a short last span goes first (the upload nothing can hide is the smallest one); with it
        the spans start at 32, 64, 128 ... windows, up to `per`.  Host-side arithmetic only."""
        from .features import span_samples

        N = 1 + n_samples // 160
        W = StreamingPredictor._window_count(N, T, hop)
        bounds, lo, step = [], 0, 32
        while ramp and lo < W and step < per:
            bounds.append((lo, min(W, lo + step)))
            lo, step = lo + step, 2 * step
        bounds += [(b, min(W, b + per)) for b in range(lo, W, per)]
        if not ramp and len(bounds) > 1 and bounds[-1][1] - bounds[-1][0] < per:
            bounds.insert(0, bounds.pop())
        plan = []
        for lo, hi in bounds:
            f0, f1 = hop * lo, min(N, hop * (hi - 1) + T)
            plan.append((lo, hi, f0, f1) + tuple(span_samples(n_samples, f0, f1 - f0)))
        return plan

    @torch.no_grad()
    def predict_audio_host(self, audio, windows_per_chunk: Optional[int] = None, ramp: bool = False):
        """configs[4] END TO END from host memory on one GPU: `audio` = the whole recording on the host, mono 16 kHz, as 16-bit PCM
        (AudioData's source format, vad/data_models/audio_data.py:21-24: uploaded as it is -- half the bytes of the float signal --
        and converted on the device) or float32; a numpy array or a CPU tensor (pinned memory makes the uploads asynchronous).
        The recording is cut into spans of `windows_per_chunk` windows (default max_batch: the batches predict_device runs, so the
        results are ITS bits); the next span is uploaded on a copy stream while a span's log-mel frames and forwards run.  The SHORT
        span (the recording's last W mod windows_per_chunk windows) goes first: the upload nothing can hide is the smallest one.
        `ramp=True` starts with spans of 32, 64, 128 ... windows instead: the exposed upload shrinks to an eighth (1 h fp32s: 10.20 ->
        9.96 ms against 9.75 device-resident; bf16: no gain, its small batches run the slower kernels -- scripts/ubench/
        host_pipeline_parts.py), but the batches are no longer predict_device's: the same bits only where a window's result does
        not depend on its batch (fp32 / fp32s: measured equal; bf16 needs model.batch_invariant).  Returns the per-frame
        probabilities [N] on the device."""
        from .features import log_mel_span, pcm16_to_f32

        self._require_shipped_front_end("predict_audio_host")
        src = host_source(audio)
        n = int(src.shape[0])
        N = 1 + n // 160
        W = self._window_count(N, self.T, self.hop)
        plan = self.host_span_plan(n, self.T, self.hop, int(windows_per_chunk or self.max_batch), ramp)
        self.model.eval()
        dev = _indexed(self.device)
        with _lib.on_device(dev):
            self._ensure_pipe()
            feed = HostFeed(src, dev, stream_owner=self)
            logp = torch.empty((W, self.T, 2), dtype=torch.float32, device=dev)
            for c in feed.chunks([(first, first + count) for *_, first, count in plan]):
                lo, hi, f0, f1, first, count = plan[c]
                sl = feed.buffer[first:first + count]
                if sl.dtype == torch.int16:
                    sl = pcm16_to_f32(sl)
                feat = log_mel_span(sl, first, n, f0, f1 - f0)
                self._windows_logp(feat, f0, N, lo, hi, out=logp[lo:hi], join=False)   # (spans overlap on the pipeline's streams)
            self._pipe.join()
            return self._merge(logp, W, N)

    _require_shipped_front_end = _require_shipped_front_end
    _not_shipped = ("StreamingPredictor.{what} runs the shipped log-mel front-end only (spans at its 160-sample hop, features per span): "
                    "{front_end} is not; extract the features whole and call predict_device")

    def predict(self, feature) -> np.ndarray:
        return self.predict_device(feature).cpu().numpy()
