"""The launch schedule (csrc/savad_schedule.h: plan_forward / plan_predict) against the decision table recorded before the decisions
moved into that header (tests/golden/schedule_table.txt; one line per case, every field of the plan; a field at zero is left out).
tests/schedule_dump.cpp is a stand-alone host program: compiled here with the host C++ compiler and run as a child process, once
plain and once under AddressSanitizer + UBSan.  No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "schedule_dump.cpp"
INCLUDE = REPO / "voice_activity_detection_amd" / "csrc"
TABLE = REPO / "tests" / "golden" / "schedule_table.txt"


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


def _compare(lines):
    want = TABLE.read_text().splitlines()
    for i, (a, b) in enumerate(zip(lines, want)):
        assert a == b, f"case {i + 1}: the schedule changed\n  now:      {a}\n  recorded: {b}"
    assert len(lines) == len(want)


def test_schedule_matches_recorded_table(tmp_path):
    _compare(_dump(tmp_path, "schedule_dump", []))


def test_schedule_clean_under_sanitizers(tmp_path):
    _compare(_dump(tmp_path, "schedule_dump_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_table_covers_every_selector_value():
    """every value of every selector appears at least once, and the table stays small"""
    text = TABLE.read_text()
    assert len(text) < 300 * 1024
    for token in ["fam0", "fam1", "fam2", "fam3", "form0", "form1", "form2", "attn1", "attn2", "attn3", "attn4", "var4", "var5", "var6", "var7",
                  "var8", " pad1", "msplit1", "fused1", "wide1", "inp1", "ksc5", "fv1", "win1", "f32s1", "err-2", " S2", " S8", " cb1 ", " x1 "]:
        assert token in text, token
    lines = text.splitlines()
    assert any(" inp1 " in ln and " ksc5" not in ln for ln in lines)          # the persistent input stage with a run-time K-step count
    variants = [re.search(r" var(\d+) last(\d+)", ln) for ln in lines if ln.startswith("P")]
    assert any(v and v.group(1) != v.group(2) for v in variants)              # a predict whose shorter last launch takes another variant
