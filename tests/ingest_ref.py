"""Vectorised numpy restatement of the band-limited resampler -- TEST INFRASTRUCTURE for the device ingest.

The same algorithm as oracle/resample.py (resampy's ``kaiser_fast``), arranged the way the device kernel is: one LANE per output
sample, the taps walked in order (left wing, then right wing), weight and product in float64, the accumulator rounded to float32 after
every tap.  tests/test_ingest_host.py pins it ``np.array_equal`` to ``oracle.resample.resample``; it exists because the oracle's Python
loops take about a minute per 20 s of 48 kHz audio and cannot be asked for a block of outputs deep inside an hour, which this can:
``resample_block`` takes the time registers of any set of outputs, ``time_registers`` walks resampy's repeated addition in chunks.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle.resample import kaiser_fast_window

TARGET = 16000


def tables(rate: int):
    """(win, delta, scale, step, num_table): the filter as oracle.resample.resample prepares it for this source rate"""
    ratio = float(TARGET) / rate
    win, num_table = kaiser_fast_window()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    return win, delta, scale, int(scale * num_table), num_table


def time_registers(rate: int, n_out: int, chunk: int = 1 << 20):
    """yields (k0, times[k0:k0 + len]) for k0 = 0, chunk, ...: the values ``time_register += time_increment`` takes, by sequential
    float64 addition (np.cumsum adds in order; a chunk starts from the value the previous one ended on, so the chain is unbroken)"""
    inc = 1.0 / (float(TARGET) / rate)
    carry = 0.0
    for k0 in range(0, n_out, chunk):
        m = min(chunk, n_out - k0)
        steps = np.full(m + 1, inc)
        steps[0] = carry
        t = np.cumsum(steps)
        carry = float(t[m])          # the register after m more additions
        yield k0, t[:m]


def all_time_registers(rate: int, n_out: int) -> np.ndarray:
    out = np.empty(n_out, dtype=np.float64)
    for k0, t in time_registers(rate, n_out):
        out[k0:k0 + t.shape[0]] = t
    return out


def resample_block(x: np.ndarray, rate: int, times: np.ndarray, tab=None) -> np.ndarray:
    """the output samples whose time registers are `times` (float64), of the float32 signal x at `rate` Hz"""
    win, delta, scale, step, num_table = tab if tab is not None else tables(rate)
    nwin, n_in = win.shape[0], x.shape[0]
    t = np.asarray(times, dtype=np.float64)
    n = t.astype(np.int64)
    frac = scale * (t - n)
    acc = np.zeros(t.shape[0], dtype=np.float32)
    for wing in (0, 1):
        f = frac if wing == 0 else scale - frac
        index_frac = f * num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        reach = (nwin - offset) // step
        limit = np.minimum(n + 1, reach) if wing == 0 else np.minimum(n_in - n - 1, reach)
        for j in range(int(limit.max()) if limit.size else 0):
            on = j < limit
            idx = np.where(on, offset + j * step, 0)
            src = np.where(on, n - j if wing == 0 else n + j + 1, 0)
            weight = win[idx] + eta * delta[idx]
            acc = np.where(on, (acc.astype(np.float64) + weight * x[src].astype(np.float64)).astype(np.float32), acc)
    return acc


def resample(x: np.ndarray, rate: int, block: int = 1 << 16, workers: int = 8) -> np.ndarray:
    """float32 mono signal -> oracle.resample.resample(x, rate) (int(n * ratio) samples, zero-padded to ceil(n * ratio))"""
    x = np.asarray(x, dtype=np.float32)
    if rate == TARGET:
        return x
    ratio = float(TARGET) / rate
    n_out, n_fix = int(x.shape[0] * ratio), int(np.ceil(x.shape[0] * ratio))
    y = np.zeros(n_fix, dtype=np.float32)
    tab = tables(rate)
    times = all_time_registers(rate, n_out)

    def run(k0):
        y[k0:k0 + block][:min(block, n_out - k0)] = resample_block(x, rate, times[k0:k0 + block], tab)

    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(run, range(0, n_out, block)))
    return y
