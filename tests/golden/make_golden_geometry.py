#!/usr/bin/env python3
"""Golden vectors of the predictor at every window geometry of tests/window_geometry_cases.py: the REFERENCE's own
VADFromScratchPredictor.predict_probabilities (vad/predictor.py:159-262, unmodified, behind the import shims of make_golden.py)
on the seeded weights and features, at each geometry's golden length.  Run on the build machine, from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geometry.py

Writes tests/golden/golden_geometry.npz (golden.npz is not touched): per geometry `h{half}_j{jump}_probs` = probs [N, W] float32
as the reference returns it, plus the list of geometries, lengths and feature seeds.  Only seeds and outputs are stored."""
from __future__ import annotations

import os
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as base  # noqa: E402  (puts the repo and the reference on sys.path)

sys.path.insert(0, str(HERE.parent))   # (the reference has a `tests` package of its own: the module is imported by its plain name)
import window_geometry_cases as cases  # noqa: E402
from voice_activity_detection_amd.seeded import seeded_state_dict  # noqa: E402


def main():
    model = base.ref_model(seeded_state_dict(1234))
    g = {"geometries": np.array(cases.GEOMETRIES, dtype=np.int64)}
    rows = []
    for half, jump in cases.GEOMETRIES:
        N = cases.golden_length(half, jump)
        pred = base.reference_predictor(model, half, jump)
        feat = cases.features(half, jump, N)
        probs = np.asarray(pred.predict_probabilities(types.SimpleNamespace(feat=feat, sample_rate=16000)))
        W = len(cases.offsets(half, jump))
        assert probs.shape == (N, W) == (N, pred.context_window_frames), (half, jump, probs.shape)
        g[cases.golden_key(half, jump)] = probs.astype(np.float32)
        rows.append((half, jump, W, N, 7000 + 100 * half + jump))
        print(f"{half:>2} / {jump}: W = {W:>2}, N = {N:>3}, {int((probs == 0.5).sum())} placeholders")
    g["half_jump_W_N_seed"] = np.array(rows, dtype=np.int64)
    out = HERE / "golden_geometry.npz"
    np.savez_compressed(out, **g)
    print(f"wrote {out}: {len(g)} arrays, {out.stat().st_size / 1e3:.1f} kB on disk")


if __name__ == "__main__":
    os.chdir(base.REPO)
    main()
