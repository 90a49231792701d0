"""The audio side's host code (csrc/savad_audio_host.h), without a GPU: every table, resampling plan, workspace layout and shape it
computes, through the stand-alone tests/audio_tables_dump.cpp (host compiler, ASan + UBSan, its own process), against
tests/golden/audio_tables.json -- recorded from the library as it was BEFORE the tables moved into that header -- and against what
the freshly built library's exports return, so that the library is known to use the header."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "audio_tables_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"
GOLDEN = json.loads((REPO / "tests" / "golden" / "audio_tables.json").read_text())

WHOLE_N = (1, 159, 160, 161, 4000, 57_600_000)
SPAN_FRAMES = (1, 32, 33, 45_000)
RATES = (8000, 11025, 16001, 22050, 44100, 48000, 96000)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++, or CXX)")
    exe = tmp_path_factory.mktemp("audio_tables") / "audio_tables_dump"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(SRC), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60)
    assert out.stderr == ""
    lines = [line.split() for line in out.stdout.splitlines()]
    assert len({w[0] for w in lines}) == len(lines)
    return {w[0]: w[1:] for w in lines}


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def _sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def _config(name):
    from voice_activity_detection_amd import _lib

    return _lib.savad_frontend_config(*GOLDEN["frontend"][name]["config"])


def test_every_table_has_the_bits_it_had(dump):
    assert len(GOLDEN["hashes"]) == 5 + 2 + 4 * len(GOLDEN["frontend"])
    for key, want in GOLDEN["hashes"].items():
        assert dump[key][0] == want, key
    for rate in RATES:
        g = GOLDEN["resample"][str(rate)]
        assert dump[f"rs.{rate}.segments"] == [g["segments"], str(g["n_segments"]), str(g["k_end"])], rate
        ratio, scale, inc, step, taps, span, lds_table, lds_plain = dump[f"rs.{rate}.plan"]
        assert [float.fromhex(v).hex() for v in (ratio, scale, inc)] == [g["ratio"], g["scale"], g["inc"]], rate
        assert [int(step), int(taps), int(span)] == [g["step"], g["taps"], g["span"]], rate
        assert int(lds_plain) == 4 * g["span"] and int(lds_table) == 8193 * 16 + 4 * g["span"] <= 160 * 1024
        assert [int(v) for v in dump[f"rs.{rate}.span_inputs"][:2]] == g["span_inputs_3001"], rate


def test_the_two_filterbank_roundings_stay_apart(dump):
    """One filterbank, two roundings of weight x norm, each pinned by its own path's bit-exact tests: merging them would move one."""
    h = GOLDEN["hashes"]
    assert dump["filterbank.512x80.factors"][0] == h["filterbank.512x80.factors"]
    assert dump["filterbank.512x80.product"][0] == h["filterbank.512x80.product"] == h["fe.logmel.table1"]
    assert h["filterbank.512x80.factors"] != h["filterbank.512x80.product"]
    differ, nonzero = map(int, dump["filterbank.512x80.differ"])
    assert (differ, nonzero) == (182, 500)


def test_the_library_hands_out_the_same_tables(lib, dump):
    sizes = [lib.savad_logmel_table_floats(i) for i in range(3)]
    tables = [np.zeros(k, np.float32) for k in sizes]
    assert lib.savad_logmel_tables_host(*[ctypes.c_void_p(t.ctypes.data) for t in tables]) == 0
    for key, t in zip(("logmel.t1", "logmel.t3", "logmel.tm"), tables):
        assert [_sha(t), str(t.nbytes)] == dump[key] and _sha(t) == GOLDEN["hashes"][key]
    for name in GOLDEN["frontend"]:
        cfg = _config(name)
        for which in range(4):
            k = lib.savad_frontend_table_floats(ctypes.byref(cfg), which)
            assert k >= 0
            t = np.zeros(max(k, 1), np.float32)
            assert lib.savad_frontend_tables_host(ctypes.byref(cfg), which, ctypes.c_void_p(t.ctypes.data)) == 0
            key = f"fe.{name}.table{which}"
            assert [_sha(t[:k]), str(4 * k)] == dump[key] and _sha(t[:k]) == GOLDEN["hashes"][key], key
    for rate in RATES:
        k0, t0, s = np.zeros(256, np.int64), np.zeros(256), np.zeros(256)
        covered = ctypes.c_long()
        n = lib.savad_resample_segments_host(rate, 256, *[ctypes.c_void_p(a.ctypes.data) for a in (k0, t0, s)], ctypes.byref(covered))
        assert [_sha(k0[:n], t0[:n], s[:n]), str(n), str(covered.value)] == dump[f"rs.{rate}.segments"], rate
        first, count = ctypes.c_long(), ctypes.c_long()
        ratio = float.fromhex(dump[f"rs.{rate}.plan"][0])
        assert lib.savad_resample_span_samples(3001, rate, 0, int(3001 * ratio), ctypes.byref(first), ctypes.byref(count)) == 0
        assert [str(first.value), str(count.value)] == dump[f"rs.{rate}.span_inputs"][:2]


def test_logmel_workspaces_and_spans(lib, dump):
    ws = GOLDEN["logmel_workspace"]
    for kind, sizes, export in (("whole", WHOLE_N, lib.savad_logmel_workspace_bytes), ("span", SPAN_FRAMES, lib.savad_logmel_span_workspace_bytes)):
        for v in sizes:
            total, pad_a, pad_b = map(int, dump[f"logmel.ws.{kind}.{v}"])
            assert total == ws[kind][str(v)] == export(v), (kind, v)
            assert (pad_a, pad_b) == (ws["pad_a"], ws["pad_b"])
            assert pad_b - pad_a >= 4 * 208 and total - pad_b >= 4 * 212        # the two edge stretches: apart, and inside
    for n in WHOLE_N:
        frames = 1 + n // 160
        got = []
        for first, count in ((0, 1), (frames - 1, 1), (0, frames)):
            a, b = ctypes.c_long(), ctypes.c_long()
            assert lib.savad_logmel_span_samples(n, first, count, ctypes.byref(a), ctypes.byref(b)) == 0
            got += [a.value, b.value]
        assert got == [int(v) for v in dump[f"logmel.span_samples.{n}"]] == GOLDEN["logmel_span_samples"][str(n)], n


def test_frontend_shapes_and_workspaces(lib, dump):
    seen_refusal = False
    for name, g in GOLDEN["frontend"].items():
        cfg = _config(name)
        transform, n_fft, deltas = g["config"][0], g["config"][1], g["config"][6]
        assert set(g["n_samples"]) == {str(n_fft // 2 + 1), "4000", "160000"}
        for n, want in g["n_samples"].items():
            need, frames, feats = map(int, dump[f"fe.{name}.shape.{n}"])
            total, gmax, sig, spec, db = map(int, dump[f"fe.{name}.ws.{n}"])
            fr, ft, by = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            rc = lib.savad_frontend_shape(ctypes.byref(cfg), int(n), ctypes.byref(fr), ctypes.byref(ft))
            assert need == (n_fft if transform == 0 else n_fft // 2 + 1)
            if want is None:     # the library refuses what the header's arithmetic marks: too few samples, or too few frames for deltas
                assert rc == -1 and (int(n) < need or (deltas and frames < 9)), (name, n)
                seen_refusal = True
                continue
            assert rc == 0 and lib.savad_frontend_workspace_bytes(ctypes.byref(cfg), int(n), ctypes.byref(by)) == 0
            assert (frames, feats) == (fr.value, ft.value) == (want["frames"], want["features"]), (name, n)
            assert total == by.value == want["total"], (name, n)
            assert (gmax, sig, spec, db) == (want["gmax"], want["sig"], want["spec"], want["db"]), (name, n)
    assert seen_refusal
