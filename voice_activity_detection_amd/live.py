"""Live sessions: audio fed as it arrives, many streams per tick (C ABI: the savad_live_* entries of include/savad.h).

What a stream's ticks and its finish return, concatenated, is ``predict_audio_device`` of the finished recording, row for row,
however the recording was cut into pushes: after n samples (n - 208) // 160 + 1 frames are ready (none below 257 samples), and a row
is final once the window centred `half` frames after it exists.  The latency of a row is therefore 2 * half frames + 208 samples:
393 ms at the shipped geometry (half = 19).

One tick of S streams is a fixed number of launches (append, log-mel, window gather and forward per `chunk_size` windows, boost),
one upload (the tick's tables and every host chunk, from one pinned buffer) and no read-back: every count comes from host arithmetic.

With `post=VADPredictParameters(...)` a tick has one more stage on the device (two launches, csrc/savad_live_post.h): "speech started
at sample s" / "speech ended at sample e" as soon as no continuation of the recording can change them.  A stream's events,
concatenated, are the activities offline `predict()` gives for the finished recording with the same parameters, index for index.
`trim` needs look-ahead of its own: with v, h, b = min_vally, min_hill, hang_before in frames, an event at sample s is in the tick
after which 160 (R - v - h - b) > s + 1 for the stream's R final rows, so the worst-case latency behind the audio is the rows'
393 ms plus (v + h + b) frames: 893 ms at 200 / 200 / 100 ms.  Nothing is ever retracted; a tick whose events nobody reads costs no
read-back.

Not built: `activity_max_seconds` online (the optimal split takes the argmin over a whole segment, which needs the segment's end),
`return_probs` and `split_max_seconds` online (both are about the whole recording), other sample rates and channel counts, the
extended front-ends, HIP-graph capture of a tick, more than one GPU.
"""
from __future__ import annotations

import ctypes
import weakref
from datetime import timedelta
from typing import Iterable, Mapping, Optional

import numpy as np
import torch

from . import _lib
from .data_models import Activity
from .predictor import (ContextResolution, VADFromScratchPredictor, VADPredictParameters, _indexed, _require_hip,
                        context_window_frames)

_PCM_INT16, _PCM_FLOAT32 = 0, 1   # SAVAD_PCM_*
START, END = 0, 1                 # SAVAD_LIVE_EVENT_*: the kinds of LiveTick.events


def post_frames(post: VADPredictParameters) -> "tuple[int, int, int, int]":
    """(min_vally, min_hill, hang_before, hang_over) in frames, as predict() derives them; refuses what has no online form"""
    if post.activity_max_seconds is not None and post.activity_max_seconds > 0:
        raise ValueError("activity_max_seconds has no online form: the optimal split takes the argmin over a whole segment, which "
                         "needs the segment's end")
    if post.return_probs:
        raise ValueError("return_probs has no online form: a live tick carries its rows' probabilities (tick[slot])")
    if post.split_max_seconds is not None:
        raise ValueError("split_max_seconds has no online form: a live stream is one recording")
    hop_ms = VADFromScratchPredictor.hop_ms
    frames = tuple(round(ms / hop_ms) for ms in (post.min_vally_ms, post.min_hill_ms, post.hang_before_ms, post.hang_over_ms))
    if min(frames) < 0:
        raise ValueError(f"negative trim parameter: {frames} frames")
    return frames


class LiveTick:
    """The rows one tick made final.  probs [rows, W] and mean [rows] are device tensors holding the slots' rows one after the other;
    `rows` maps slot -> (first row index in its recording, offset into probs / mean, count); tick[slot] -> (first, probs, mean).
    In a session with `post`: events(slot) -> [(kind, sample)] (START / END) and activities(slot) -> the Activity objects this tick
    finished.  The first of these calls on a tick copies the tick's event buffer once, for all slots; ticks are fetched in the
    order they were made (an earlier tick that is still alive is fetched first), which is what pairs an END with its START."""

    def __init__(self, probs: torch.Tensor, mean: torch.Tensor, rows: "dict[int, tuple[int, int, int]]"):
        self.probs, self.mean, self.rows = probs, mean, rows
        self._vad = self._events_dev = self._events = self._activities = None

    def _fetched(self):
        if self._vad is None:
            raise _lib.SavadError("this session has no post-processing: construct it with post=VADPredictParameters(...)")
        if self._events is None:
            self._vad._fetch_through(self)
        return self

    def events(self, slot: int) -> "list[tuple[int, int]]":
        return self._fetched()._events[slot]

    def activities(self, slot: int) -> "list[Activity]":
        return self._fetched()._activities[slot]

    def __getitem__(self, slot: int):
        first, at, count = self.rows[slot]
        return first, self.probs[at:at + count], self.mean[at:at + count]

    def __contains__(self, slot: int) -> bool:
        return slot in self.rows

    def __len__(self) -> int:
        return len(self.rows)


class LiveVAD:
    """`streams` slots of live voice-activity detection on one GPU.

        vad = LiveVAD(model, "cuda:0", streams=64, max_push_samples=1600)
        a, b = vad.open(), vad.open()
        tick = vad.push({a: chunk_a, b: chunk_b})        # chunks: int16 or float32, numpy / CPU tensor, or float32 device tensor
        first, probs, mean = tick[a]                      # rows first .. first + len(probs) - 1 of a's recording
        last = vad.finish([a])                            # the remaining rows; the slot is free again

    `model_or_predictor`: a SelfAttentiveVAD on `device`, or a VADFromScratchPredictor (its model, window geometry and chunk size
    are used; its front-end must be the shipped one).  The model's `precision`, `row_mode` and the chunk size are honoured as in the
    offline paths.  16 kHz mono only.

    `post`: the parameters of predict()'s post-processing (threshold, min_vally_ms, min_hill_ms, hang_before_ms, hang_over_ms); the
    ticks then carry events (module docstring).  Worst-case latency behind the audio: 393 ms + (v + h + b) frames.
    `activity_max_seconds`, `return_probs` and `split_max_seconds` have no online form and are refused."""

    def __init__(self, model_or_predictor, device, streams: int, max_push_samples: int, context: Optional[ContextResolution] = None,
                 chunk_size: Optional[int] = None, sample_rate: int = 16000, channels: int = 1, post: Optional[VADPredictParameters] = None):
        self.post = post
        frames = post_frames(post) if post is not None else None
        if int(sample_rate) != 16000 or int(channels) != 1:
            raise NotImplementedError(f"live sessions take 16 kHz mono audio ({sample_rate} Hz, {channels} channel(s) asked for): "
                                      "resample and downmix before pushing (features.resample_to_16k_device)")
        self.device = torch.device(device)
        _require_hip(self.device)
        self.device = _indexed(self.device)
        model = model_or_predictor
        if hasattr(model_or_predictor, "front_end") and hasattr(model_or_predictor, "model"):
            predictor = model_or_predictor
            predictor._require_shipped_front_end("LiveVAD")
            model = predictor.model
            if context is None:
                context = ContextResolution(predictor.context_window_half_frames, predictor.context_window_jump_frames)
            if chunk_size is None:
                chunk_size = predictor.chunk_size
        context = ContextResolution() if context is None else context
        self.model = model
        self.streams, self.max_push_samples = int(streams), int(max_push_samples)
        self.half, self.jump = int(context.context_window_half_frames), int(context.context_window_jump_frames)
        self.chunk_size = 16384 if chunk_size is None else int(chunk_size)
        lib = self._lib = _lib.load()
        self._cfg = _lib.savad_live_config(self.streams, self.max_push_samples, self.half, self.jump, self.chunk_size)
        nbytes = ctypes.c_size_t()
        _lib.check(lib.savad_live_state_bytes(self._cfg, ctypes.byref(nbytes)))
        self.W = context_window_frames(self.half, self.jump)   # (refuses a geometry the reference cannot run)
        self._slots = (_lib.savad_live_slot * self.streams)()
        with _lib.on_device(self.device):
            self._state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)   # (the allocator aligns it far beyond 16 bytes)
            _lib.check(lib.savad_live_table_bytes(self._cfg, self.streams, ctypes.byref(nbytes)))
            # staging: [the tick's tables | every host chunk, 16-byte aligned]; two pinned buffers, so that filling one never waits for
            # the upload of the other
            self._stage_bytes = nbytes.value + self.streams * ((4 * self.max_push_samples + 15) & ~15)
            self._pinned = [torch.empty(self._stage_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self._uploaded = [None, None]
            self._stage_dev = torch.empty(self._stage_bytes, dtype=torch.uint8, device=self.device)
            if post is not None:
                self._post_cfg = _lib.savad_live_post_config(self.W, float(post.threshold), *frames)
                _lib.check(lib.savad_live_post_state_bytes(self._post_cfg, self.streams, ctypes.byref(nbytes)))
                self._post_state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
                self._post_ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._turn = 0
        self._ws_bytes = {}
        self._open_start = {}    # slot -> sample of its START that has no END yet (after the last fetched tick)
        self._unfetched = []     # weak references to the ticks whose events nobody has read yet, oldest first

    # ---- slots ----------------------------------------------------------------------------------
    def open(self) -> int:
        """a free slot, opened"""
        for slot in range(self.streams):
            if not self._slots[slot].open:
                _lib.check(self._lib.savad_live_open(self._cfg, self._slots, slot))
                return slot
        raise _lib.SavadError(f"all {self.streams} slots are open")

    def samples(self, slot: int) -> int:
        """samples pushed into an open slot so far"""
        return int(self._slots[slot].n_samples)

    def in_voice(self, slot: int) -> bool:
        """is the slot inside a speech segment, as of the last tick whose events were fetched"""
        return slot in self._open_start

    # ---- events ---------------------------------------------------------------------------------
    def _fetch_through(self, tick: LiveTick):
        """fetches every unfetched tick up to `tick`, oldest first (a tick the caller dropped is gone, and with it its events)"""
        while self._unfetched:
            t = self._unfetched.pop(0)()
            if t is None or t._events is not None:
                continue
            self._fetch(t)
            if t is tick:
                break
        if tick._events is None:
            self._fetch(tick)

    def _fetch(self, tick: LiveTick):
        """One device -> host copy for all slots of the tick: the offsets, the counts and as many events as ticks usually hold (a
        tick with more takes a second copy).  Pairs every END with the slot's open START."""
        order, events_at, finished = tick._events_layout
        n = len(order)
        buf = tick._events_dev
        head = min(buf.numel(), events_at + 16 * (n // 2 + 16))
        host = buf[:head].cpu().numpy()
        tick.fetched_bytes = head
        meta = host[:4 * (2 * n + 1)].view(np.int32)
        offsets, counts = meta[:n + 1], meta[n + 1:]
        total = int(offsets[n])
        if events_at + 16 * total > head:
            host = np.concatenate([host, buf[head:events_at + 16 * total].cpu().numpy()])
            tick.fetched_bytes = events_at + 16 * total
        records = host[events_at:events_at + 16 * total].view(np.dtype([("sample", np.int64), ("slot", np.int32), ("kind", np.int32)]))
        if (counts < 0).any():
            slot = order[int(np.flatnonzero(counts < 0)[0])]
            raise _lib.SavadError(f"slot {slot}: the post-processing stage was skipped for an earlier tick of this stream (count -1)")
        events, activities = {slot: [] for slot in order}, {slot: [] for slot in order}
        for i in np.flatnonzero(counts):          # (most entries of most ticks have no event)
            slot = order[i]
            evs, acts = events[slot], activities[slot]
            for r in records[offsets[i]:offsets[i + 1]]:
                kind, sample = int(r["kind"]), int(r["sample"])
                evs.append((kind, sample))
                if kind == START:
                    self._open_start[slot] = sample
                else:
                    if slot not in self._open_start:
                        raise _lib.SavadError(f"slot {slot}: an END at sample {sample} without its START: an earlier tick's events were "
                                              "never fetched")
                    # (times as convert_samples_to_segments builds them)
                    acts.append(Activity(start=timedelta(seconds=self._open_start.pop(slot) / 16000), end=timedelta(seconds=sample / 16000)))
        for slot in finished:
            self._open_start.pop(slot, None)
        tick._events, tick._activities = events, activities
        tick._events_dev = None

    # ---- ticks ----------------------------------------------------------------------------------
    def push(self, chunks: Mapping[int, object]) -> LiveTick:
        return self.step(chunks, ())

    def finish(self, slots: Iterable[int], chunks: Optional[Mapping[int, object]] = None) -> LiveTick:
        """ends the streams in `slots` (after their last chunk in `chunks`, if any): their remaining rows; other slots in `chunks`
        just push -- one tick underneath"""
        return self.step(chunks or {}, slots)

    @torch.no_grad()
    def step(self, chunks: Mapping[int, object], finish: Iterable[int] = ()) -> LiveTick:
        """One tick: every slot in `chunks` pushes its chunk, every slot in `finish` ends after it."""
        lib, cfg = self._lib, self._cfg
        finish = list(dict.fromkeys(int(s) for s in finish))
        order = list(dict.fromkeys([int(s) for s in chunks] + finish))
        n = len(order)
        dev = self.device
        if n == 0:
            tick = LiveTick(torch.empty((0, self.W), dtype=torch.float32, device=dev), torch.empty((0,), dtype=torch.float32, device=dev), {})
            if self.post is not None:
                tick._vad, tick._events, tick._activities = self, {}, {}
            return tick
        if n > self.streams:
            raise _lib.SavadError(f"{n} slots in one tick, the state has {self.streams}")
        nbytes = ctypes.c_size_t()
        _lib.check(lib.savad_live_table_bytes(cfg, n, ctypes.byref(nbytes)))
        table_bytes = nbytes.value
        turn = self._turn
        if self._uploaded[turn] is not None:
            self._uploaded[turn].synchronize()   # (the upload of the tick before last: long done)
        pinned = self._pinned[turn]
        pinned_np = pinned.numpy()
        dev_base = self._stage_dev.data_ptr()
        pushes = (_lib.savad_live_push * n)()
        at = table_bytes
        keep = []   # device chunks stay referenced until the tick is enqueued
        for i, slot in enumerate(order):
            chunk = chunks.get(slot) if slot in chunks else None
            dtype, count, ptr = _PCM_FLOAT32, 0, None
            if chunk is not None:
                if isinstance(chunk, torch.Tensor) and chunk.device.type == "cuda":
                    if chunk.dtype != torch.float32 or chunk.dim() != 1:
                        raise ValueError("a device chunk must be a 1-D float32 tensor")
                    if chunk.device != dev:
                        raise _lib.SavadError(f"chunk on {chunk.device}, the session on {dev}")
                    chunk = chunk.contiguous()
                    keep.append(chunk)
                    count, ptr = chunk.numel(), chunk.data_ptr()
                else:
                    arr = chunk.numpy() if isinstance(chunk, torch.Tensor) else np.asarray(chunk)
                    if arr.ndim != 1:
                        raise ValueError(f"a chunk must be 1-D mono audio, got shape {arr.shape}")
                    if arr.dtype == np.int16:
                        dtype = _PCM_INT16
                    elif arr.dtype != np.float32:
                        raise ValueError(f"a chunk must be int16 or float32, got {arr.dtype}")
                    count = arr.shape[0]
                    if count > self.max_push_samples:
                        raise _lib.SavadError(f"a push of {count} samples; max_push_samples is {self.max_push_samples}")
                    size = count * arr.itemsize
                    pinned_np[at:at + size].view(arr.dtype)[:] = arr
                    ptr = dev_base + at
                    at += (size + 15) & ~15
            pushes[i] = _lib.savad_live_push(slot, count, dtype, int(slot in finish), ptr if count else None)
        counts, rows = _lib.savad_live_counts(), np.zeros((n, 2), dtype=np.int64)
        with _lib.on_device(dev):
            _lib.check(lib.savad_live_plan(cfg, self._slots, pushes, n, self._state, pinned, table_bytes, ctypes.byref(counts), rows))
            model = self.model
            model.eval()
            model._prepare_call(dev)
            key = (n, model._pushed_knobs)
            ws_bytes = self._ws_bytes.get(key)
            if ws_bytes is None:
                _lib.check(lib.savad_live_workspace_bytes(model._handle, cfg, n, ctypes.byref(nbytes)))
                ws_bytes = self._ws_bytes[key] = nbytes.value
            ws = model._workspace_for(ws_bytes, dev)
            self._stage_dev[:at].copy_(pinned[:at], non_blocking=True)   # the one upload of the tick
            event = self._uploaded[turn]
            if event is None:
                event = self._uploaded[turn] = torch.cuda.Event()
            event.record()
            self._turn = turn ^ 1
            probs = torch.empty((counts.rows, self.W), dtype=torch.float32, device=dev)
            mean = torch.empty((counts.rows,), dtype=torch.float32, device=dev)
            stream, stage = torch.cuda.current_stream(dev), self._stage_dev
            _lib.check(lib.savad_live_step(model._handle, cfg, self._slots, pinned, stage, probs, mean, ws, ws.numel(), stream))
            if self.post is not None:
                post, at = self._post_cfg, ctypes.c_size_t()
                _lib.check(lib.savad_live_post_event_bytes(cfg, post, pinned, ctypes.byref(nbytes), ctypes.byref(at)))
                events = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
                _lib.check(lib.savad_live_post_workspace_bytes(cfg, post, pinned, ctypes.byref(nbytes)))
                if self._post_ws.numel() < nbytes.value:
                    self._post_ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
                _lib.check(lib.savad_live_post(cfg, post, pinned, stage, probs, self._post_state, events, events.numel(),
                                               self._post_ws, self._post_ws.numel(), stream))
        del keep
        out, first_out = {}, 0
        for i, slot in enumerate(order):
            out[slot] = (int(rows[i, 0]), first_out, int(rows[i, 1]))
            first_out += int(rows[i, 1])
        tick = LiveTick(probs, mean, out)
        if self.post is not None:
            tick._vad, tick._events_dev, tick._events_layout = self, events, (order, at.value, set(finish))
            self._unfetched = [r for r in self._unfetched if r() is not None]
            self._unfetched.append(weakref.ref(tick))
        return tick


class LiveSession:
    """One live stream: LiveVAD with a single slot.  push(chunk) -> (first, probs, mean): the rows first .. that became final;
    finish() -> the remaining rows.  With `post` (LiveVAD): events() / activities() of the last push or finish."""

    def __init__(self, model_or_predictor, device, max_push_samples: int, context: Optional[ContextResolution] = None,
                 post: Optional[VADPredictParameters] = None, **kwargs):
        self.vad = LiveVAD(model_or_predictor, device, 1, max_push_samples, context, post=post, **kwargs)
        self.slot = self.vad.open()
        self.tick = None   # the last LiveTick

    def push(self, chunk):
        self.tick = self.vad.push({self.slot: chunk})
        return self.tick[self.slot]

    def finish(self, chunk=None):
        """ends the recording (after `chunk`, if given); the session can take a new recording afterwards"""
        self.tick = self.vad.finish([self.slot], {self.slot: chunk} if chunk is not None else None)
        result = self.tick[self.slot]
        self.slot = self.vad.open()
        return result

    def events(self) -> "list[tuple[int, int]]":
        """[(kind, sample)] of the last push or finish"""
        return self.tick.events(next(iter(self.tick.rows)))

    def activities(self) -> "list[Activity]":
        """the Activity objects the last push or finish completed"""
        return self.tick.activities(next(iter(self.tick.rows)))

    def in_voice(self) -> bool:
        return self.vad.in_voice(self.slot)
