#!/usr/bin/env python3
"""Golden vectors of the routing probes of tests/routing_probes.py: the REFERENCE's own SelfAttentiveVAD (behind make_golden.py's
loader), each regime's state loaded into it, converted with .double() and run on the probe's input as a double tensor -- its float64
log-probabilities per regime and length, at the lengths of GOLDEN_T (the longer ones are not pinned: the fixture stays small).
Run on the build machine, from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_routing.py

Writes tests/golden/golden_routing.npz (the other golden files are not touched): `{regime}_T{T}` = log-probs [B, T, 2] float64.
Only the reference's outputs are stored; states, targets and inputs regenerate from tests/routing_probes.py."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests import routing_probes as rp  # noqa: E402  (before the reference's own `tests` package comes onto the path)

sys.path.insert(0, str(HERE))

import make_golden as base  # noqa: E402  (puts the reference on sys.path)


def main():
    g = {}
    for regime in rp.REGIMES:
        for T in rp.GOLDEN_T:
            st, x, tg = rp.case(regime, T)
            m = base.ref_model(st, rp.FEATURES, rp.num_layers(st), 128).double()
            with torch.no_grad():
                y = m(features=torch.from_numpy(np.array(x)).double()).numpy()
            assert y.dtype == np.float64 and y.shape == (tg.shape[0], T, 2) and np.isfinite(y).all(), (regime, T)
            g[rp.golden_key(regime, T)] = y
            print(f"{rp.golden_key(regime, T):16s} {y.shape} log-probs in [{y.min():.3f}, {y.max():.3f}]")
    out = HERE / "golden_routing.npz"
    np.savez_compressed(out, **g)
    print(f"wrote {out}: {len(g)} arrays, {out.stat().st_size / 1e3:.1f} kB on disk")


if __name__ == "__main__":
    os.chdir(base.REPO)
    main()
