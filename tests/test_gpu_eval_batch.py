"""The batched device metrics (savad_eval_batch_counts; csrc/savad_eval_batch.h) on the GPU: every clip's counters and boundary
records against the host twin and against savad_eval_counts_host on the clip alone, files_metrics_device against file_metrics per
clip, and the evaluate command with batch_files.  Every case runs at savad_eval_set_block 64 and at the default.  Integers and
float64 bits: every comparison is exact."""
import ctypes
import json

import numpy as np
import pytest

from tests.eval_batch_cases import (BAD, assert_batch_equals_clips, batches, concatenate, counts_host_batch, first_outcome, per_clip_counts,
                                    segment_room)
from tests.eval_cases import L, assert_same_metrics, outcome
from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.metrics import EVAL_BAD_LABEL, EVAL_COUNTERS, EVAL_NAN

pytestmark = pytest.mark.gpu

PATTERN, GUARD, HOST_GUARD = 0xA5, 4096, 64
NAMES = list(batches())


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    return torch


@pytest.fixture
def block(request):
    """the sort blocks and the scans at 64 elements per workgroup block, or at the default (0)"""
    lib = _lib.load()
    _lib.check(lib.savad_eval_set_block(request.param))
    yield request.param
    _lib.check(lib.savad_eval_set_block(0))


BLOCKS = pytest.mark.parametrize("block", [64, 0], ids=["block64", "default"], indirect=True)


def counts_device(torch, clips, threshold, seg_cap=None, ws_short=0):
    """savad_eval_batch_counts with the workspace, the counters, the records and seg_first inside guard bands -> (count, counters, seg,
    seg_first); asserts that nothing outside them was written"""
    lib = _lib.load()
    probs_all, clip_first, labels_all, label_first = concatenate(clips)
    C, W = len(clips), probs_all.shape[1]
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_batch_workspace_bytes(clip_first, label_first, C, W, ctypes.byref(need)))
    buf = torch.full((need.value + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert need.value > 0 and buf.data_ptr() % 16 == 0
    d_probs = torch.from_numpy(probs_all).cuda() if probs_all.size else torch.zeros((1, W), dtype=torch.float32, device="cuda")
    d_labels = torch.from_numpy(labels_all).cuda() if labels_all.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_clip_first, d_label_first = torch.from_numpy(clip_first).cuda(), torch.from_numpy(label_first).cuda()
    room = segment_room(clip_first, label_first) if seg_cap is None else seg_cap
    counters = np.full(C * EVAL_COUNTERS + 2 * HOST_GUARD, -7, dtype=np.int64)
    seg = np.full((room + 2 * HOST_GUARD, 8), 0xEE, dtype=np.uint8)
    seg_first = np.full(C + 1 + 2 * HOST_GUARD, -7, dtype=np.int64)
    inside = lambda a: ctypes.c_void_p(a.ctypes.data + HOST_GUARD * a.strides[0])
    count = lib.savad_eval_batch_counts(d_probs, clip_first, d_clip_first, d_labels, label_first, d_label_first, C, W, float(threshold), L,
                                        inside(counters), inside(seg), room, inside(seg_first), buf, need.value - ws_short,
                                        torch.cuda.current_stream())
    torch.cuda.synchronize()
    guard = buf[need.value:].cpu().numpy()
    assert (guard == PATTERN).all(), f"{int((guard != PATTERN).sum())} bytes written past the {need.value} reported workspace bytes"
    for a, fill in ((counters, -7), (seg, 0xEE), (seg_first, -7)):
        assert (a[:HOST_GUARD] == fill).all() and (a[len(a) - HOST_GUARD:] == fill).all()
    return (count, counters[HOST_GUARD:-HOST_GUARD].reshape(C, EVAL_COUNTERS), seg[HOST_GUARD:len(seg) - HOST_GUARD],
            seg_first[HOST_GUARD:-HOST_GUARD])


@BLOCKS
@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_the_host_twin_and_every_clip_alone(torch_cuda, block, name):
    clips, threshold = batches()[name]
    got = counts_device(torch_cuda, clips, threshold)
    twin = counts_host_batch(clips, threshold)
    assert got[0] == twin[0] and got[1].tolist() == twin[1].tolist() and got[3].tolist() == twin[3].tolist(), name
    assert np.array_equal(got[2], twin[2]), name
    assert_batch_equals_clips(name, got, per_clip_counts(clips, threshold))
    flagged = [c for c in range(len(clips)) if got[1][c, EVAL_NAN] or got[1][c, EVAL_BAD_LABEL]]
    assert flagged == list(BAD.get(name, ())), name


@BLOCKS
@pytest.mark.parametrize("name", NAMES)
def test_files_metrics_device_equals_file_metrics_per_clip(torch_cuda, block, name):
    from voice_activity_detection_amd.evaluate import file_metrics, files_metrics_device

    torch = torch_cuda
    clips, threshold = batches()[name]
    probs_all, clip_first, _, _ = concatenate(clips)
    labels_list = [y for _, y in clips]
    want = first_outcome(file_metrics, clips, threshold)
    for table_dev in (None, torch.from_numpy(clip_first).cuda()):
        got = outcome(files_metrics_device, labels_list, torch.from_numpy(probs_all).cuda(), clip_first, threshold, table_dev)
        assert got[0] == want[0], (name, got, want)
        if want[0] == "error":
            assert got == want, name
        else:
            assert len(got[1]) == len(clips)
            for c in range(len(clips)):
                assert_same_metrics(("ok", got[1][c]), ("ok", want[1][c]), (name, c))
    if want[0] == "error":   # the clips that have metrics, as a batch of their own: every value
        each = [outcome(file_metrics, labels, probs, threshold) for probs, labels in clips]
        kept = [clip for clip, one in zip(clips, each) if one[0] == "ok"]
        assert kept, name
        probs_all, clip_first, _, _ = concatenate(kept)
        got = files_metrics_device([y for _, y in kept], torch.from_numpy(probs_all).cuda(), clip_first, threshold)
        for c, want_c in enumerate(one for one in each if one[0] == "ok"):
            assert_same_metrics(("ok", got[c]), want_c, (name, "kept", c))


def test_good_clips_keep_the_device_result_next_to_bad_ones(torch_cuda, monkeypatch):
    """only the clip with a NaN score and the clip with a label of 2 go to file_metrics"""
    from voice_activity_detection_amd import evaluate

    clips, threshold = batches()["bad clips among good ones"]
    probs_all, clip_first, _, _ = concatenate(clips)
    seen = []
    host = evaluate.file_metrics
    monkeypatch.setattr(evaluate, "file_metrics", lambda y, p, t: seen.append(len(p)) or host(y, p, t))
    got = evaluate.files_metrics_device([y for _, y in clips], torch_cuda.from_numpy(probs_all).cuda(), clip_first, threshold)
    assert seen == [len(clips[c][0]) for c in BAD["bad clips among good ones"]]
    for c, (probs, labels) in enumerate(clips):
        assert_same_metrics(("ok", got[c]), outcome(host, labels, probs, threshold), c)


@BLOCKS
def test_one_clip_equals_savad_eval_counts(torch_cuda, block):
    torch = torch_cuda
    lib = _lib.load()
    clips, threshold = batches()["one clip"]
    probs, labels = clips[0]
    labels8 = labels.astype(np.uint8)
    N, W = probs.shape
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_workspace_bytes(N, W, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    counters, seg = np.full(EVAL_COUNTERS, -1, dtype=np.int64), np.full(((N + 1) // 2, 8), 0xEE, dtype=np.uint8)
    count = lib.savad_eval_counts(torch.tensor(probs).cuda(), N, W, torch.from_numpy(labels8).cuda(), len(labels8), threshold, L, counters, seg, len(seg),
                                  ws, need.value, torch.cuda.current_stream())
    got = counts_device(torch, clips, threshold)
    assert count == got[0] > 1 and counters.tolist() == got[1][0].tolist() and np.array_equal(seg, got[2]) and got[3].tolist() == [0, count]


def test_refusals_and_small_segment_room(torch_cuda):
    torch = torch_cuda
    lib = _lib.load()
    clips, threshold = batches()["segments at the ends"]
    want = per_clip_counts(clips, threshold)
    total = sum(len(s) for _, s in want)
    # room for one record fewer than there are: refused with the counters returned, no record written
    count, counters, seg, seg_first = counts_device(torch, clips, threshold, seg_cap=total - 1)
    assert count == -1 and b"room for" in lib.savad_last_error() and (seg == 0xEE).all()
    assert [counters[c].tolist() for c in range(len(clips))] == [w[0].tolist() for w in want]
    # a workspace one byte short is refused before anything is launched or written
    count, counters, seg, seg_first = counts_device(torch, clips, threshold, ws_short=1)
    assert count == -1 and b"workspace" in lib.savad_last_error()
    assert (counters == -7).all() and (seg == 0xEE).all() and (seg_first == -7).all()
    # a misaligned workspace and a null device pointer as well
    probs_all, clip_first, labels_all, label_first = concatenate(clips)
    C, W = len(clips), probs_all.shape[1]
    need = ctypes.c_size_t()
    _lib.check(lib.savad_eval_batch_workspace_bytes(clip_first, label_first, C, W, ctypes.byref(need)))
    buf = torch.full((need.value + 8,), PATTERN, dtype=torch.uint8, device="cuda")
    d_probs, d_labels = torch.from_numpy(probs_all).cuda(), torch.from_numpy(labels_all).cuda()
    d_clip_first, d_label_first = torch.from_numpy(clip_first).cuda(), torch.from_numpy(label_first).cuda()
    counters, seg, seg_first = np.full((C, EVAL_COUNTERS), -7, dtype=np.int64), np.full((total, 8), 0xEE, dtype=np.uint8), np.full(C + 1, -7, dtype=np.int64)
    stream = torch.cuda.current_stream()
    call = lambda probs, table_dev, ws: lib.savad_eval_batch_counts(probs, clip_first, table_dev, d_labels, label_first, d_label_first, C, W, threshold, L,
                                                                    counters, seg, total, seg_first, ws, need.value, stream)
    assert call(d_probs, d_clip_first, ctypes.c_void_p(buf.data_ptr() + 4)) == -1 and b"aligned" in lib.savad_last_error()
    assert call(None, d_clip_first, buf) == -1 and call(d_probs, None, buf) == -1 and call(d_probs, d_clip_first, None) == -1
    torch.cuda.synchronize()
    assert (counters == -7).all() and (seg == 0xEE).all() and (seg_first == -7).all() and (buf.cpu().numpy() == PATTERN).all()
    assert call(d_probs, d_clip_first, buf) == total


# ---- the evaluate command ----------------------------------------------------------------------------------------------------

def reference_results(predictor, pairs, data_dir, K, threshold=0.5):
    """file_metrics on the downloaded slices of predict_probabilities_many over the same groups of K files"""
    from voice_activity_detection_amd.data_models import VoiceActivity
    from voice_activity_detection_amd.evaluate import file_metrics
    from voice_activity_detection_amd.features import load_wav_mono16k

    out = []
    for at in range(0, len(pairs), K):
        group = pairs[at:at + K]
        feats = [predictor.features(load_wav_mono16k(data_dir / pair["audio_path"])) for pair in group]
        for pair, (probs, _) in zip(group, predictor.predict_probabilities_many(feats)):
            labels = VoiceActivity.load(data_dir / pair["voice_activity_path"]).to_labels(100)
            out.append(file_metrics(labels, probs.cpu().numpy(), threshold))
    return out


def strip(result):
    return {k: v for k, v in result.items() if "path" not in k}


def test_evaluate_command_with_batch_files(torch_cuda, tmp_path, state1234):
    """the shipped eval_list.jsonl names one recording, so the list here names it and the two other labelled recordings of the golden
    data: K = 2 makes groups of 2 + 1, K = 8 one group of 3"""
    from tests.conftest import write_reference_checkpoint
    from tests.golden.data_files import data_root
    from tests.test_trained_weights import FILES
    from voice_activity_detection_amd.evaluate import METRIC_KEYS, evaluate_vad_from_scratch, load_data_list
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    shipped = load_data_list(data_root() / "eval_list.jsonl")
    assert [str(pair["audio_path"]) for pair in shipped] == [FILES[2][0]]
    eval_list = tmp_path / "list.jsonl"
    eval_list.write_text("".join(json.dumps({"audio_path": a, "voice_activity_path": v}) + "\n" for a, v in (FILES[2], FILES[0], FILES[1])))
    pairs = load_data_list(eval_list)
    predictor = VADFromScratchPredictor.from_checkpoint(tmp_path / "m.checkpoint", "cuda")
    echoes, runs = {}, {}
    for K in (0, 2, 8):
        echoes[K] = []
        runs[K] = evaluate_vad_from_scratch(eval_list, tmp_path / "m.checkpoint", tmp_path / f"out{K}.jsonl", data_dir=data_root(), device_metrics=True,
                                            batch_files=K, echo=echoes[K].append)
    keys = list(METRIC_KEYS) + ["boosted_" + k for k in METRIC_KEYS]
    for K in (2, 8):
        want = reference_results(predictor, pairs, data_root(), K)
        got = runs[K]
        assert [r["audio_path"] for r in got["files"]] == [r["audio_path"] for r in runs[0]["files"]] and len(got["files"]) == 3
        assert [list(r) for r in got["files"]] == [list(r) for r in runs[0]["files"]] and list(got["total"]) == list(runs[0]["total"]) == keys
        for r, w in zip(got["files"], want):
            assert_same_metrics(("ok", strip(r)), ("ok", w), (K, r["audio_path"]))
        assert_same_metrics(("ok", got["total"]), ("ok", {k: float(np.mean([w[k] for w in want])) for k in keys}), (K, "total"))
        assert len(echoes[K]) == len(echoes[0]) == len(pairs) + 1
        assert [e.splitlines()[1] for e in echoes[K]] == [e.splitlines()[1] for e in echoes[0]]   # the titles, in the list's order
        lines = (tmp_path / f"out{K}.jsonl").read_text().splitlines()
        assert json.loads(lines[0]) == got["total"] and [json.loads(l) for l in lines[1:]] == [dict(r) for r in got["files"]]


def test_cli_evaluate_batch_files(torch_cuda, tmp_path, state1234):
    from tests.conftest import write_reference_checkpoint
    from tests.golden.data_files import data_root
    from voice_activity_detection_amd.__main__ import main
    from voice_activity_detection_amd.evaluate import evaluate_vad_from_scratch

    write_reference_checkpoint(tmp_path / "m.checkpoint", state1234)
    eval_list = data_root() / "eval_list.jsonl"
    assert main(["evaluate", str(eval_list), str(tmp_path / "m.checkpoint"), "--output-path", str(tmp_path / "cli.jsonl"), "--device-metrics",
                 "--batch-files", "2"]) == 0
    evaluate_vad_from_scratch(eval_list, tmp_path / "m.checkpoint", tmp_path / "call.jsonl", device_metrics=True, batch_files=2, echo=lambda s: None)
    assert (tmp_path / "cli.jsonl").read_text() == (tmp_path / "call.jsonl").read_text()
    assert len(json.loads((tmp_path / "cli.jsonl").read_text().splitlines()[0])) == 18
