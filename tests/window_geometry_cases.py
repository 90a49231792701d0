"""The window geometries the predictor is held to (tests/test_window_geometry_host.py on the CPU, tests/test_gpu_window_geometry.py on
the GPU), their inputs, and a plain numpy restatement of the reference's window gather and boosted scatter (vad/predictor.py:180-258)
written as Python loops -- TEST INFRASTRUCTURE ONLY.

half / jump   W   per   why
   0 / 1      1   32    every frame is a window, no placeholders
   1 / 1      3   10    2 idle rows of a packed 32-row block
   3 / 5      3   10    jump > half: offsets [-3, 0, 1]
   6 / 4      5    6    asymmetric offsets, 2 idle rows
  20 / 9      7    4    the shipped W with other, asymmetric offsets [-20, -11, -2, 0, 1, 10, 19]
   5 / 1     11    2    10 idle rows
   8 / 1     17    1    one window per block
  15 / 1     31    1    one idle row
  16 / 1     33    -    the first W without a windowed launch: gather + a T > 32 forward, two query blocks, the second ragged
  31 / 1     63    -    the longest window (32 / 1, W = 65, is refused)
per = windows per packed 32-row block of the single-launch forwards = max(32 // W, 1)."""
import functools

import numpy as np

from voice_activity_detection_amd.seeded import seeded_features

GEOMETRIES = [(0, 1), (1, 1), (3, 5), (6, 4), (20, 9), (5, 1), (8, 1), (15, 1), (16, 1), (31, 1)]
# fp32's windowed launch takes at most 1024 * per windows: these run past it, in chunked forwards with a ragged last chunk
LONG_CASES = [(8, 1, 1043, 1000), (5, 1, 2063, 1000)]   # (half, jump, N, chunk_size)
# geometries where the reference's context_window_frames formula and its offsets disagree (the reference fails on them)
DISAGREEING = [(4, 2), (9, 3), (0, 2)]
FEATURE_SIZE = 80


def geometry_id(g):
    return f"{g[0]}-{g[1]}"


def offsets(half, jump):
    """arange(-half, 0, jump) ++ [0] ++ arange(1, half + 1, jump)  (vad/predictor.py:204-215)"""
    return np.concatenate([np.arange(-half, 0, jump), np.array([0]), np.arange(1, half + 1, jump)]).astype(np.int64)


def reference_formula(half, jump):
    """vad/predictor.py:57-59"""
    return 2 * (half - 1) // jump + 3


def per_block(W):
    return max(32 // W, 1)


def golden_length(half, jump):
    W = len(offsets(half, jump))
    return 2 * half + 5 * per_block(W) + 3


def lengths(half, jump):
    """no window; one window; one window into a second packed block; the golden length (five blocks and a ragged sixth)"""
    W = len(offsets(half, jump))
    return [max(1, 2 * half), 2 * half + 1, 2 * half + per_block(W) + 1, golden_length(half, jump)]


@functools.lru_cache(maxsize=None)
def features(half, jump, N):
    feat = seeded_features(7000 + 100 * half + jump, (N, FEATURE_SIZE))
    feat.setflags(write=False)
    return feat


def golden_key(half, jump):
    return f"h{half}_j{jump}_probs"


# ---- the reference's gather and boost, restated ------------------------------------------------------------------------------------

def gather(feature, half, jump, moved=None):
    """vad/predictor.py:182-218 for every item: (windows [n, W, F] float32, positions [n, W] int64), n = max(N - 2 half, 0).
    moved = (w, d): slot w READS the frame d further on than it should (clamped to the recording); its position stays."""
    N, F = feature.shape
    off = offsets(half, jump)
    W = len(off)
    n = max(N - 2 * half, 0)
    windows = np.zeros((n, W, F), dtype=np.float32)
    positions = np.zeros((n, W), dtype=np.int64)
    for item in range(n):
        centre = half + item
        for w in range(W):
            frame = centre + int(off[w])
            positions[item, w] = frame
            if moved is not None and moved[0] == w:
                frame = min(max(frame + moved[1], 0), N - 1)
            windows[item, w, :] = feature[frame, :]
    return windows, positions


def boost(logp, positions, N):
    """vad/predictor.py:239-258 and :95: scatter the log-probs to (frame, slot), softmax over the two classes (an unfilled slot: the
    softmax of two zeros, exactly 0.5), mean over the slots -> (probs [N, W] float32, mean [N] float64)"""
    n, W, _ = logp.shape
    boosted = np.zeros((N, W, 2), dtype=np.float32)
    for item in range(n):
        for w in range(W):
            boosted[positions[item, w], w, :] = logp[item, w, :]
    probs = np.zeros((N, W), dtype=np.float32)
    for frame in range(N):
        for w in range(W):
            a, b = np.float32(boosted[frame, w, 0]), np.float32(boosted[frame, w, 1])
            m = max(a, b)
            ea, eb = np.exp(a - m), np.exp(b - m)       # float32 throughout, as scipy's softmax of a float32 array
            probs[frame, w] = eb / (ea + eb)
    return probs, probs.mean(axis=1)
