"""Host audio -> device, piece by piece, under the compute: the one upload pipeline of the from-host prediction paths
(VADFromScratchPredictor.predict_audio_host, StreamingPredictor.predict_audio_host).  A path names what each of its chunks reads
(`needs`); the feed copies what is not on the device yet on a copy stream, one chunk ahead of the compute."""
from __future__ import annotations

import numpy as np
import torch


def host_source(audio):
    """host audio (numpy array or CPU tensor, int16 PCM or float32) as a CPU tensor without a copy"""
    src = audio if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(audio))
    if src.device.type != "cpu" or src.dim() != 1 or src.numel() < 1 or src.dtype not in (torch.int16, torch.float32) or not src.is_contiguous():
        raise ValueError("audio must be a non-empty contiguous 1-D int16 or float32 array on the host")
    return src


class Uploaded:
    """What is on the device: sorted disjoint half-open ranges (no torch, no device)."""

    def __init__(self):
        self.ranges = []

    def missing(self, a: int, b: int):
        """the pieces of [a, b) that are not present yet, in order; they are present afterwards"""
        if b <= a:
            return []
        gaps, at, lo_all, hi_all, apart = [], a, a, b, []
        for lo, hi in self.ranges:
            if hi < a or lo > b:   # neither overlaps nor touches [a, b)
                apart.append((lo, hi))
                continue
            if lo > at:
                gaps.append((at, lo))
            at = max(at, hi)
            lo_all, hi_all = min(lo_all, lo), max(hi_all, hi)
        if b > at:
            gaps.append((at, b))
        self.ranges = sorted(apart + [(lo_all, hi_all)])
        return gaps


class HostFeed:
    """The device copy of `src` (a host_source; `unit` interleaved samples per position: the channels) and the stream that fills it.
    Create it with `device` current.  The copy stream is cached on `stream_owner` (`_copy_stream`: one per predictor and device)."""

    def __init__(self, src: torch.Tensor, device: torch.device, unit: int = 1, stream_owner=None):
        owner = self if stream_owner is None else stream_owner
        if getattr(owner, "_copy_stream", None) is None or owner._copy_stream.device != device:
            owner._copy_stream = torch.cuda.Stream(device)
        self.src, self.unit, self.stream, self.current = src, int(unit), owner._copy_stream, torch.cuda.current_stream(device)
        self.buffer = torch.empty(src.numel(), dtype=src.dtype, device=device)
        self.buffer.record_stream(self.stream)
        self.stream.wait_stream(self.current)
        self.uploaded = Uploaded()

    def request(self, a: int, b: int) -> "torch.cuda.Event":
        """queue the copy of what positions [a, b) lack on the device; the event fires when they are all there"""
        u, ev = self.unit, torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            for lo, hi in self.uploaded.missing(a, b):
                self.buffer[lo * u:hi * u].copy_(self.src[lo * u:hi * u], non_blocking=True)   # (pageable memory: stages synchronously)
            ev.record(self.stream)
        return ev

    def chunks(self, needs):
        """for c in feed.chunks(needs): needs[c] = (a, b) is on the device for the work the current stream is given in the body, and
        needs[c + 1] has been requested -- its upload runs under chunk c's compute"""
        ev = self.request(*needs[0])
        for c in range(len(needs)):
            nxt = self.request(*needs[c + 1]) if c + 1 < len(needs) else None
            self.current.wait_event(ev)
            yield c
            ev = nxt
