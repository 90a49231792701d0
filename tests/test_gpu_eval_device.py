"""The device metrics of evaluate (savad_eval_sort, savad_eval_counts; csrc/savad_eval_device.h) on the GPU: the sort against numpy's
stable argsort, the counters and boundary records against the host twin (which tests/test_eval_counts_host.py holds to
evaluate.file_metrics), file_metrics_device against file_metrics, and the evaluate command with and without device_metrics.
Integers and float64 bits: every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from tests.eval_cases import L, assert_same_metrics, counts_host, edge_cases, grid_cases, outcome, planted
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.metrics import EVAL_COUNTERS

pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA5, 4096
SIZES = (1, 65, 4097)
CASES = dict(grid_cases(SIZES))
CASES.update({f"{name} ({N})": case for N in SIZES for name, case in edge_cases(N).items()})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    return torch


@pytest.fixture
def block(request):
    """the sort and its scans at 64 elements per workgroup block (the digit table's scan then runs three and more levels from
    4097 elements on), or at the default (0)"""
    lib = _lib.load()
    _lib.check(lib.savad_eval_set_block(request.param))
    yield request.param
    _lib.check(lib.savad_eval_set_block(0))


BLOCKS = pytest.mark.parametrize("block", [64, 0], ids=["block64", "default"], indirect=True)
# every case at the default; at 64 the ones of more than one default block, which then run many blocks and scan levels
CASE_BLOCKS = [pytest.param(0, name, id=f"default-{name}") for name in CASES] + [pytest.param(64, name, id=f"block64-{name}") for name in CASES if "4097" in name]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def guarded_workspace(torch, n_frames, W):
    """a workspace of EXACTLY the reported bytes with a byte pattern behind it"""
    need = ctypes.c_size_t()
    _lib.check(_lib.load().savad_eval_workspace_bytes(n_frames, W, ctypes.byref(need)))
    assert need.value > 0
    buf = torch.full((need.value + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, need.value


def assert_guard_intact(torch, buf, n):
    torch.cuda.synchronize()
    guard = buf[n:].cpu().numpy()
    assert (guard == PATTERN).all(), f"{int((guard != PATTERN).sum())} bytes written past the {n} reported workspace bytes"


@functools.lru_cache(maxsize=None)
def key_sets(n):
    rng = np.random.default_rng(n)
    distinct = rng.permutation(n).astype(np.float32) - np.float32(n // 2)           # negative, zero and positive, no two equal
    distinct *= np.float32(0.37)
    few = rng.choice(np.array([-2.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 0.5, 1.0, 3e38, -3e38, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0], np.float32), size=n)
    equal = np.full(n, 0.625, np.float32)
    labels = rng.integers(0, 2, size=n).astype(np.uint8)
    return {"all distinct": distinct, "16 distinct values": few, "all equal": equal}, labels


@BLOCKS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097, 20001])
def test_sort_is_numpys_stable_argsort(torch_cuda, block, n):
    torch = torch_cuda
    lib = _lib.load()
    sets, labels = key_sets(n)
    buf, need = guarded_workspace(torch, n, 1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, keys in sets.items():
        assert (len(np.unique(keys)) == n) if name == "all distinct" else (len(np.unique(keys)) <= 16)
        order = np.argsort(keys, kind="stable")   # (-0.0 and +0.0 compare equal: they keep their order)
        d_keys, d_labels = torch.from_numpy(keys).cuda(), torch.from_numpy(labels).cuda()
        out_keys, out_labels = torch.full((n,), -7.0, dtype=torch.float32, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        _lib.check(lib.savad_eval_sort(ptr(d_keys), ptr(d_labels), n, ptr(out_keys), ptr(out_labels), ptr(buf), need, stream))
        assert_guard_intact(torch, buf, need)
        want = keys[order] + np.float32(0.0)   # a -0.0 comes back as +0.0; every other value keeps its bits
        assert np.array_equal(out_keys.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, name)
        assert np.array_equal(out_labels.cpu().numpy(), labels[order]), (n, name)
        assert torch.equal(d_keys.cpu(), torch.from_numpy(keys)) and torch.equal(d_labels.cpu(), torch.from_numpy(labels))   # inputs only read


def counts_device(torch, probs, labels, threshold, seg_cap=None):
    """savad_eval_counts on a guarded workspace -> (counters, seg)"""
    lib = _lib.load()
    N, W = probs.shape
    labels8 = labels.astype(np.uint8)
    d_probs, d_labels = torch.tensor(probs).cuda(), torch.from_numpy(labels8).cuda()
    buf, need = guarded_workspace(torch, N, W)
    counters = np.full(EVAL_COUNTERS, -1, dtype=np.int64)
    seg = np.full(((min(N, len(labels8)) + 1) // 2 if seg_cap is None else seg_cap, 8), 0xEE, dtype=np.uint8)
    count = lib.savad_eval_counts(ptr(d_probs), N, W, ptr(d_labels), len(labels8), float(threshold), L, ctypes.c_void_p(counters.ctypes.data),
                                  ctypes.c_void_p(seg.ctypes.data), len(seg), ptr(buf), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert_guard_intact(torch, buf, need)
    return count, counters, seg


def check_case(torch, name, probs, labels, threshold):
    from voice_activity_detection_amd.evaluate import file_metrics, file_metrics_device

    want_counters, want_seg = counts_host(probs, labels, threshold)
    count, counters, seg = counts_device(torch, probs, labels, threshold)
    assert count == len(want_seg), (name, count)
    assert counters.tolist() == want_counters.tolist(), name
    assert np.array_equal(seg[:count], want_seg), (name, np.flatnonzero((seg[:count] != want_seg).any(axis=1))[:10])
    assert (seg[count:] == 0xEE).all()
    got = outcome(file_metrics_device, labels, torch.tensor(probs).cuda(), threshold)
    assert_same_metrics(got, outcome(file_metrics, labels, probs, threshold), name)


@pytest.mark.parametrize("block,name", CASE_BLOCKS, indirect=["block"])
def test_counts_equal_the_host_twin_and_file_metrics(torch_cuda, block, name):
    check_case(torch_cuda, name, *CASES[name])


def test_one_hour(torch_cuda):
    check_case(torch_cuda, "one hour", *planted(360001, 7), 0.5)


def test_refusals_and_small_segment_room(torch_cuda):
    torch = torch_cuda
    lib = _lib.load()
    probs, labels, threshold = edge_cases(65)["segments at both ends"]
    count, counters, seg = counts_device(torch, probs, labels, threshold, seg_cap=1)
    assert count == -1 and b"room for 1" in lib.savad_last_error() and (seg == 0xEE).all()
    # a workspace one byte short is refused before anything is launched
    d_probs, d_labels = torch.tensor(probs).cuda(), torch.from_numpy(labels.astype(np.uint8)).cuda()
    buf, need = guarded_workspace(torch, len(probs), probs.shape[1])
    counters, seg = np.zeros(EVAL_COUNTERS, np.int64), np.zeros((8, 8), np.uint8)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.savad_eval_counts(ptr(d_probs), len(probs), probs.shape[1], ptr(d_labels), len(labels), 0.5, L, ctypes.c_void_p(counters.ctypes.data),
                                 ctypes.c_void_p(seg.ctypes.data), 8, ptr(buf), need - 1, stream) == -1
    out_k, out_l = torch.empty(12, dtype=torch.float32, device="cuda"), torch.empty(12, dtype=torch.uint8, device="cuda")
    assert lib.savad_eval_sort(ptr(d_probs), ptr(d_labels), 12, ptr(out_k), ptr(out_l), ptr(buf), 16, stream) == -1
    assert_guard_intact(torch, buf, need)


def test_evaluate_command_with_device_metrics(torch_cuda, tmp_path):
    """evaluate_vad_from_scratch on the labelled JamakeSpeechSample recordings with the trained checkpoint: device_metrics=True gives
    the dict, the echo and the output file of device_metrics=False"""
    import json

    from tests.conftest import write_reference_checkpoint
    from tests.golden.data_files import data_root, load_trained
    from tests.test_trained_weights import FILES
    from voice_activity_detection_amd.evaluate import evaluate_vad_from_scratch

    state = {k[len("state/"):]: v for k, v in load_trained().items() if k.startswith("state/")}
    write_reference_checkpoint(tmp_path / "trained.checkpoint", state)
    (tmp_path / "list.jsonl").write_text("".join(json.dumps({"audio_path": a, "voice_activity_path": v}) + "\n" for a, v in FILES[:2]))
    results, echoes = {}, {}
    for flag in (False, True):
        echoes[flag] = []
        results[flag] = evaluate_vad_from_scratch(tmp_path / "list.jsonl", tmp_path / "trained.checkpoint", tmp_path / f"out{flag}.jsonl",
                                                  data_dir=data_root(), device_metrics=flag, echo=echoes[flag].append)
    assert results[True] == results[False] and len(results[True]["files"]) == 2
    assert results[True]["files"][0]["auc"] > 0.99   # a trained model on its own recordings: the metrics mean something
    assert echoes[True] == echoes[False]
    assert (tmp_path / "outTrue.jsonl").read_text() == (tmp_path / "outFalse.jsonl").read_text()
    for a, b in zip(results[True]["files"], results[False]["files"]):
        assert_same_metrics(("ok", {k: v for k, v in a.items() if "path" not in k}), ("ok", {k: v for k, v in b.items() if "path" not in k}), a["audio_path"])


def test_cli_evaluate_device_metrics_and_precision(torch_cuda, tmp_path, state1234):
    import json

    from tests.conftest import write_reference_checkpoint
    from tests.golden.data_files import data_root
    from voice_activity_detection_amd.__main__ import main

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    common = ["evaluate", str(data_root() / "eval_list.jsonl"), str(tmp_path / "m.checkpoint"), "--precision", "fp32s"]
    assert main(common + ["--output-path", str(tmp_path / "host.jsonl")]) == 0
    assert main(common + ["--output-path", str(tmp_path / "device.jsonl"), "--device-metrics"]) == 0
    assert (tmp_path / "device.jsonl").read_text() == (tmp_path / "host.jsonl").read_text()
    assert len(json.loads((tmp_path / "host.jsonl").read_text().splitlines()[0])) == 18
