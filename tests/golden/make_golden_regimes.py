#!/usr/bin/env python3
"""Golden vectors of the numeric regimes of tests/numeric_regimes.py: the REFERENCE's own SelfAttentiveVAD (behind make_golden.py's
loader), each regime's state loaded into it, converted with .double() and run on the regime's input as a double tensor -- its float64
log-probabilities per regime and shape.  Run on the build machine, from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_regimes.py

Writes tests/golden/golden_regimes.npz (the other golden files are not touched): `{regime}_B{B}T{T}` = log-probs [B, T, 2] float64.
Only the reference's outputs are stored; states and inputs regenerate from tests/numeric_regimes.py."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as base  # noqa: E402  (puts the repo and the reference on sys.path)

sys.path.insert(0, str(HERE.parent))   # (the reference has a `tests` package of its own: the module is imported by its plain name)
import numeric_regimes as nr  # noqa: E402


def main():
    g = {}
    for r in nr.REGIMES:
        st = r.state()
        m = base.ref_model(st, st["input_layer.0.weight"].shape[1], nr.num_layers(st), r.d_model).double()
        for shape in r.shapes:
            with torch.no_grad():
                y = m(features=torch.from_numpy(r.x(shape)).double()).numpy()
            assert y.dtype == np.float64 and y.shape == (shape[0], shape[1], 2) and np.isfinite(y).all(), (r.name, shape)
            g[r.key(shape)] = y
            print(f"{r.key(shape):28s} log-probs in [{y.min():.3f}, {y.max():.3f}]")
    out = HERE / "golden_regimes.npz"
    np.savez_compressed(out, **g)
    print(f"wrote {out}: {len(g)} arrays, {out.stat().st_size / 1e3:.1f} kB on disk")


if __name__ == "__main__":
    os.chdir(base.REPO)
    main()
