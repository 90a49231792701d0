"""Caller buffers with guards on both sides -- TEST INFRASTRUCTURE for tests/test_gpu_caller_buffers.py.

A torch allocation is rounded up to 512 bytes and lives in a 2 MiB segment, so a kernel that writes 8 bytes past an odd-sized output,
or reads the 16-byte chunk behind the last sample, lands in allocator slack and no test notices.  ``BufferArena`` is ONE uint8 tensor
(on a HIP device, or on the CPU for tests/test_buffer_arena_host.py) inside which the buffers a caller hands to an entry point are
placed at exactly the alignment include/savad.h asks for, between guards:

    place_output(nbytes, align, dtype)   extent and both guards (GUARD bytes each) filled with OUT_FILL (0xA5); returns a typed view
                                         of exactly the extent.  An element the call never wrote still holds the pattern, so the
                                         caller's bit comparison with the clean result fails on it.
    place_input(tensor, align)           the data copied in between two guards of IN_FILL (0xFF) bytes: a NaN as fp32 / fp16 / bf16,
                                         -1 as int16, the invalid label 255 as uint8 -- a read outside the extent that reaches a result
                                         changes it.
    check()                              every guard intact and every input's data unchanged (no entry point writes its input); the
                                         message names the buffer, the side and the number of bytes that changed.

``align`` is 16 or the natural 8 / 4 / 2 / 1: the extent starts at the lowest address behind the front guard that is a multiple of
``align`` and of nothing larger (an odd multiple), so a kernel that assumes more than the header promises is caught, and the case's
shape makes the end ragged.  Everything a test can detect lies inside the one allocation."""
from __future__ import annotations

import numpy as np
import torch

GUARD = 4096
OUT_FILL = 0xA5
IN_FILL = 0xFF


class BufferArena:
    def __init__(self, device="cpu", capacity: int = 1 << 20):
        self.buf = torch.empty(int(capacity), dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.placed = []   # (name, kind, region start, extent start, extent end, fill, expected extent bytes or None)

    def _place(self, nbytes: int, align: int, fill: int, name: str):
        if align not in (1, 2, 4, 8, 16):
            raise ValueError(f"align {align}: 16 or the natural 8 / 4 / 2 / 1")
        nbytes = int(nbytes)
        start = self.cursor + GUARD
        while (self.base + start) % (2 * align) != align:   # an odd multiple of align: that alignment and no more
            start += 1
        end = start + nbytes
        if end + GUARD > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is too small for {name} ({nbytes} bytes)")
        self.buf[self.cursor:end + GUARD] = fill
        region = self.cursor
        self.cursor = end + GUARD
        return region, start, end

    def place_output(self, nbytes: int, align: int, dtype=torch.uint8, name: str = None):
        """a view of exactly `nbytes` bytes as `dtype`, pattern-filled, guarded on both sides"""
        name = name or f"output {len(self.placed)}"
        region, start, end = self._place(nbytes, align, OUT_FILL, name)
        self.placed.append((name, "output", region, start, end, OUT_FILL, None))
        return self.buf[start:end].view(dtype)

    def place_input(self, tensor, align: int, name: str = None):
        """a copy of `tensor` (same dtype and shape) between two poisoned guards"""
        name = name or f"input {len(self.placed)}"
        src = tensor.detach().contiguous()
        raw = src.reshape(-1).view(torch.uint8)
        region, start, end = self._place(raw.numel(), align, IN_FILL, name)
        self.buf[start:end] = raw.to(self.buf.device)
        self.placed.append((name, "input", region, start, end, IN_FILL, raw.cpu().numpy().copy()))
        return self.buf[start:end].view(src.dtype).view(src.shape)

    def violations(self):
        """one line per damaged guard or modified input"""
        if self.buf.device.type == "cuda":
            torch.cuda.synchronize(self.buf.device)
        host = self.buf[:self.cursor].cpu().numpy()
        found = []
        for name, kind, region, start, end, fill, data in self.placed:
            for side, lo, hi in (("front", region, start), ("back", end, end + GUARD)):
                bad = np.flatnonzero(host[lo:hi] != fill)
                if bad.size:
                    where = (start - (lo + int(bad[-1]))) if side == "front" else int(bad[0]) + 1
                    found.append(f"{name}: {bad.size} bytes of the {side} guard changed ({kind} of {end - start} bytes; nearest one "
                                 f"{where} bytes {'in front of' if side == 'front' else 'past'} the extent)")
            if data is not None:
                bad = np.flatnonzero(host[start:end] != data)
                if bad.size:
                    found.append(f"{name}: {bad.size} bytes of the input itself changed (first at byte {int(bad[0])} of {end - start})")
        return found

    def check(self):
        found = self.violations()
        assert not found, "caller buffers violated:\n  " + "\n  ".join(found)


def same_bits(a, b) -> bool:
    """two tensors / arrays of the same dtype and shape, compared byte for byte (NaNs and signed zeros included)"""
    a = a.detach().cpu().contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    b = b.detach().cpu().contiguous() if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
