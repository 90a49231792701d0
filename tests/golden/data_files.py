"""Fixtures stored in pieces, because no committed file may exceed 1 MiB, and the functions that put them back together.

* tests/golden/data: a recording stored as <name>.part0, <name>.part1, ... (consecutive byte ranges of the file) is whole again
  under data_root(), a copy of the data directory assembled once per content in the temporary directory.
* tests/golden/trained*.npz: the trained state_dict and the reference's outputs, one archive per encoder layer
  (trained_layer<i>.npz) and one for everything else (trained.npz); load_trained() merges them and save_trained() writes them.
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import tempfile
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent
DATA = GOLDEN / "data"
PART = re.compile(r"^(?P<name>.+)\.part(?P<i>\d+)$")
PIECE_BYTES = 768 << 10

_root = None


def data_root() -> Path:
    """tests/golden/data with every <name>.part<N> set joined into <name> (byte for byte)"""
    global _root
    if _root is not None:
        return _root
    files = sorted(p for p in DATA.rglob("*") if p.is_file())
    if not any(PART.match(p.name) for p in files):
        _root = DATA
        return _root
    h = hashlib.sha256()
    for p in files:
        h.update(str(p.relative_to(DATA)).encode())
        h.update(p.read_bytes())
    root = Path(tempfile.gettempdir()) / f"savad-golden-data-{os.getuid()}-{h.hexdigest()[:16]}"   # (mkdtemp: readable by its owner only)
    if not (root / ".complete").exists():
        tmp = Path(tempfile.mkdtemp(prefix="savad-golden-data-"))
        pieces = {}
        for p in files:
            rel = p.relative_to(DATA)
            m = PART.match(p.name)
            if m:
                pieces.setdefault(rel.parent / m["name"], []).append((int(m["i"]), p))
            else:
                (tmp / rel).parent.mkdir(parents=True, exist_ok=True)
                shutil.copyfile(p, tmp / rel)
        for rel, parts in pieces.items():
            (tmp / rel).parent.mkdir(parents=True, exist_ok=True)
            with open(tmp / rel, "wb") as f:
                for _, p in sorted(parts):
                    f.write(p.read_bytes())
        (tmp / ".complete").touch()
        try:
            os.replace(tmp, root)
        except OSError:   # another process put the same content there first
            shutil.rmtree(tmp, ignore_errors=True)
    _root = root
    return _root


def split_file(path, piece_bytes=PIECE_BYTES):
    """store `path` as path.part0, path.part1, ... of at most piece_bytes each and remove it"""
    path = Path(path)
    data = path.read_bytes()
    for i in range(0, max(1, (len(data) + piece_bytes - 1) // piece_bytes)):
        path.with_name(f"{path.name}.part{i}").write_bytes(data[i * piece_bytes:(i + 1) * piece_bytes])
    path.unlink()


def _layer(key):
    m = re.match(r"^state/encoder\.layers\.(\d+)\.", key)
    return None if m is None else int(m.group(1))


def save_trained(arrays, golden=GOLDEN):
    """{"state/<param>": array, "clip_logp": ..., ...} -> trained.npz + trained_layer<i>.npz (one per encoder layer); trained.npz also
    holds the keys in their order (`keys`): the oracle takes a state_dict's arrays in state_dict order"""
    groups = {"trained.npz": {"keys": np.array(list(arrays))}}
    for k, v in arrays.items():
        layer = _layer(k)
        groups.setdefault("trained.npz" if layer is None else f"trained_layer{layer}.npz", {})[k] = v
    for name, group in groups.items():
        np.savez_compressed(Path(golden) / name, **group)
    return [Path(golden) / name for name in sorted(groups)]


def load_trained(golden=GOLDEN):
    """the arrays save_trained() wrote, merged into one dict in their original order"""
    out = {}
    for f in sorted(Path(golden).glob("trained*.npz")):
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    keys = [str(k) for k in out.pop("keys")]
    assert sorted(keys) == sorted(out), "tests/golden/trained*.npz: the pieces do not match the stored key list"
    return {k: out[k] for k in keys}
