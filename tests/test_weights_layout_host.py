"""The weight layout (csrc/savad_weights.h: make_layout) against its contract: the inventory is seeded.state_dict_spec with every
tensor on a multiple of 4 floats, and the packed fp32 buffer and both fragment images lie where the formulas below put them (they are
the offsets savad.hip computed in place before the layout moved into that header).  tests/weights_dump.cpp is a stand-alone host
program: compiled here with the host C++ compiler and run as a child process, once plain and once under AddressSanitizer + UBSan.
No GPU, nothing loaded into Python."""
import math
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from voice_activity_detection_amd.seeded import state_dict_spec

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "weights_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"

CONFIGS = [(80, 3, 128), (40, 3, 128), (13, 1, 128), (257, 2, 128), (80, 6, 128), (80, 8, 128), (80, 3, 64), (20, 2, 130), (80, 1, 2)]
D, DFF = 128, 512
LBIAS = DFF + 5 * D          # b1 | b2 | bqkv | bo
FRAG_LAYER = 48 * 4096       # floats: a layer's matrices in fragment order


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    return cxx


def _dump(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Wextra", *extra, f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120)
    assert run.stderr == ""
    return run.stdout.splitlines()


def _parse(lines):
    """[(F, L, d_model, header fields, params [(key, numel, off)], raw {name: off}, packed {name: off}, images {image: (e, folded, bytes, {name: off})})]"""
    out = []
    for ln in lines:
        t = ln.split()
        if t[0] == "C":
            head = {"generic": int(t[4][7:]), "FP": int(t[5][2:]), "raw": int(t[6][3:]), "packed": int(t[7][6:])}
            out.append((int(t[1]), int(t[2]), int(t[3]), head, [], {}, {}, {}))
        elif t[0] == "P":
            out[-1][4].append((t[1], int(t[2]), int(t[3])))
        elif t[0] == "R":
            assert t[1] not in out[-1][5]
            out[-1][5][t[1]] = int(t[2])
        elif t[0] == "K":
            assert t[1] not in out[-1][6]
            out[-1][6][t[1]] = int(t[2])
        elif t[0] == "I":
            out[-1][7][t[1]] = (int(t[2][1:]), int(t[3][6:]), int(t[4][5:]), {})
        elif t[0] == "G":
            assert t[2] not in out[-1][7][t[1]][3]
            out[-1][7][t[1]][3][t[2]] = int(t[3])
        else:
            raise AssertionError(ln)
    return out


def _regions(sizes):
    """[(name, size)] laid end to end -> ({name: offset}, total)"""
    at, off = {}, 0
    for name, size in sizes:
        at[name] = off
        off += size
    return at, off


def _disjoint(at, sizes, total):
    spans = sorted((at[name], at[name] + size) for name, size in sizes.items())
    assert spans[0][0] >= 0 and spans[-1][1] <= total
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start


RAW_NAMES = ["wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1w", "ln1b", "w1", "b1", "w2", "b2", "ln2w", "ln2b"]


def _check(lines):
    cases = _parse(lines)
    assert [c[:3] for c in cases] == CONFIGS
    for F, L, dm, head, params, raw, packed, images in cases:
        generic = dm != D
        assert head["generic"] == int(generic)
        FP = F if generic else (F + 15) // 16 * 16
        assert head["FP"] == FP

        # ---- inventory: keys, element counts and order of state_dict_spec; every tensor on a multiple of 4 floats (16 bytes)
        spec = state_dict_spec(F, L, dm)
        assert [(k, n) for k, n, _ in params] == [(k, math.prod(shape)) for k, shape, _ in spec]
        off = 0
        for key, numel, at in params:
            assert at == off and at * 4 % 16 == 0, key
            off += (numel + 3) // 4 * 4
        assert head["raw"] == off
        _disjoint({k: at for k, _, at in params}, {k: n for k, n, _ in params}, head["raw"])
        # the named offsets savad.hip reads are the inventory's, in its order
        names = ["win", "bin"] + [f"{l}.{n}" for l in range(L) for n in RAW_NAMES] + ["lnf_w", "lnf_b", "wc", "bc"]
        assert list(raw) == names
        assert [raw[n] for n in names] == [at for _, _, at in params]

        if generic:   # the raw parameters are all there is
            assert head["packed"] == 0 and not packed and not images
            continue

        # ---- packed fp32 buffer
        sizes = []
        for l in range(L):
            sizes += [(f"{l}.wqkv", 3 * D * D), (f"{l}.bqkv", 3 * D), (f"{l}.w1", DFF * D), (f"{l}.b1", DFF), (f"{l}.wq_vo", 2 * D * D),
                      (f"{l}.bq_vo", 2 * D), (f"{l}.frag", FRAG_LAYER)]
        sizes += [("bias", L * LBIAS), ("wc", 2 * D), ("bc", 4), ("win_pad", D * FP)]
        want, total = _regions(sizes)
        assert packed == want
        assert head["packed"] == total
        _disjoint(packed, dict(sizes), head["packed"])

        # ---- fragment images
        assert sorted(images) == ["bf16", "f32s"]
        for name, e, folded in (("bf16", 2, 0), ("f32s", 6, 1)):
            got_e, got_folded, got_bytes, at = images[name]
            assert (got_e, got_folded) == (e, folded)
            sizes = [("win", D * FP * e)]
            for l in range(L):
                sizes += [(f"{l}.wqkv", 3 * D * D * e), (f"{l}.wo", D * D * e), (f"{l}.w1", DFF * D * e), (f"{l}.w2", D * DFF * e)]
                if folded:
                    sizes.append((f"{l}.wq_vo", 2 * D * D * e))
            want, total = _regions(sizes)
            assert at == want
            assert at["win"] == 0 and got_bytes == total
            _disjoint(at, dict(sizes), got_bytes)


def test_layout_matches_the_formulas(tmp_path):
    _check(_dump(tmp_path, "weights_dump", []))


def test_layout_clean_under_sanitizers(tmp_path):
    _check(_dump(tmp_path, "weights_dump_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
