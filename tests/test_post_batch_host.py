"""The clip rules of the batched device post-processing (csrc/savad_post_batch.h) on the CPU: the host twins run the inline functions
the kernels run and are held, clip by clip, to the host path that exists -- numpy's float32 row mean, trim_voice_activity and
convert_frames_to_samples on each clip ALONE.  Every comparison is exact.  The batches, the planted seams and the per-clip reference
of this file are what tests/test_gpu_post_batch.py runs on the GPU.

Planted seams (trim parameters 20 / 20 / 10 / 10 frames; the run at each seam is shorter than the parameter in question):
    valley       ...1 0x12 | 0x7 1...    19 zeros across the seam: filled if the seam is ignored
    hill         ...0 1 1  | 1 1 0...    4 ones across the seam: removed if the seam is ignored
    hang_over    ...1      | 0...        the hang-over would reach into the next clip
    hang_before  ...0      | 1...        the hang-before would reach back into the previous clip
    voice        ...1      | 1...        one segment if the seam is ignored; two, the first ending at its clip's last sample, the second at 0"""
import ctypes

import numpy as np
import pytest

from voice_activity_detection_amd import _lib
from voice_activity_detection_amd.clips import clip_table, split_by_clip
from voice_activity_detection_amd.postprocessing import convert_frames_to_samples, segment_indices, slot_table, trim_voice_activity

INVALID, UNSUPPORTED = -1, -2
TRIM = (20, 20, 10, 10)             # min_vally, min_hill, hang_before, hang_over in frames
GEOMETRY = (16000, 10.0, 25.0)      # sample rate, hop and window in ms
# empty clips first, doubled in the middle and last; one- and two-frame clips; boundaries before, on and after a 64-element block edge
LENGTHS = [0, 1, 2, 0, 0, 63, 64, 65, 1, 130, 0]
WIDTHS = [7, 8, 39]

_ONES, _ZEROS = (lambda n: [1] * n), (lambda n: [0] * n)
SEAMS = {
    "valley": (_ONES(30) + _ZEROS(12), _ZEROS(7) + _ONES(30)),
    "hill": (_ZEROS(40) + _ONES(2), _ONES(2) + _ZEROS(40)),
    "hang_over": (_ZEROS(30) + _ONES(30), _ZEROS(40)),
    "hang_before": (_ONES(30) + _ZEROS(40), _ONES(30) + _ZEROS(30)),
    "voice": (_ZEROS(30) + _ONES(30), _ONES(30) + _ZEROS(30)),
}


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def probs_of(pred, W, seed):
    """probabilities [N, W] whose float32 row mean is above 0.5 exactly where pred is 1: (0.6, 0.9) for a 1, (0.1, 0.4) for a 0"""
    pred = np.asarray(pred, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.4, size=(len(pred), W)).astype(np.float32)
    p[pred != 0] += np.float32(0.5)
    return p


def random_pred(n, seed):
    """n frames in runs of 1 to 25: valleys, hills and hangs shorter and longer than every parameter of TRIM"""
    rng = np.random.default_rng(seed)
    out, v = [], int(rng.integers(0, 2))
    while len(out) < n:
        out += [v] * int(rng.integers(1, 26))
        v ^= 1
    return out[:n]


def lengths_batch(W, lengths=LENGTHS):
    """(probs [sum N, W], table) of clips of `lengths` frames"""
    preds = [random_pred(n, 100 + c) for c, n in enumerate(lengths)]
    return np.concatenate([probs_of(p, W, 7 * W + c) for c, p in enumerate(preds)]), clip_table(lengths)


def seams_batch(W):
    """every seam's two clips, one after the other"""
    preds = [half for pair in SEAMS.values() for half in pair]
    return np.concatenate([probs_of(p, W, 900 + c) for c, p in enumerate(preds)]), clip_table(len(p) for p in preds)


def batches(W):
    return {"lengths": lengths_batch(W), "seams": seams_batch(W), "one clip": lengths_batch(W, [130]), "one empty clip": lengths_batch(W, [0])}


def reference_frames(probs, table, threshold=0.5, trim=TRIM):
    """[(boosted, trimmed)] of each clip ALONE: numpy's float32 mean and the host trim"""
    out = []
    for rows in split_by_clip(probs, table):
        boosted = rows.mean(axis=1) if len(rows) else np.zeros(0, np.float32)
        out.append((boosted, trim_voice_activity((boosted > threshold).astype(np.uint8), *trim)))
    return out


def reference_segments(trimmed, geometry=GEOMETRY):
    """(starts, ends) of one clip's trimmed frames through the host functions"""
    if len(trimmed) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return segment_indices(convert_frames_to_samples(trimmed, *geometry))


def frames_host_many(probs, table, threshold=0.5, trim=TRIM):
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    N, W = probs.shape
    boosted, trimmed = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint8)
    _lib.check(_lib.load().savad_post_batch_frames_host(_p(probs), _p(table), len(table) - 1, W, threshold, *trim, _p(boosted), _p(trimmed)))
    return boosted, trimmed


def classes_host_many(trimmed, table, geometry=GEOMETRY):
    cls = np.empty(int(slot_table(table, *geometry)[-1]), dtype=np.uint8)
    _lib.check(_lib.load().savad_post_batch_slot_class_host(_p(np.ascontiguousarray(trimmed)), _p(table), len(table) - 1, *geometry, _p(cls)))
    return cls


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("name", ["lengths", "seams", "one clip", "one empty clip"])
def test_frames_of_every_clip_are_the_clip_alone(name, W):
    probs, table = batches(W)[name]
    boosted, trimmed = frames_host_many(probs, table)
    want = reference_frames(probs, table)
    for c, (b, t, (wb, wt)) in enumerate(zip(split_by_clip(boosted, table), split_by_clip(trimmed, table), want)):
        assert wb.dtype == np.float32 and np.array_equal(b.view(np.uint32), wb.view(np.uint32)), (name, c)
        assert np.array_equal(t, wt), (name, c, t.tolist(), wt.tolist())
    if name in ("lengths", "seams"):
        plain = np.concatenate([(b > 0.5).astype(np.uint8) for b, _ in want])
        assert not np.array_equal(trimmed, plain)          # the trim changes something
        assert 0 < int(trimmed.sum()) < len(trimmed)


@pytest.mark.parametrize("trim", [(0, 0, 0, 0), (3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 2, 5), (30, 30, 30, 30), (1, 1, 1, 1)])
def test_every_trim_pass_alone_and_long_parameters(trim):
    probs, table = lengths_batch(7)
    _, trimmed = frames_host_many(probs, table, trim=trim)
    for c, (t, (_, wt)) in enumerate(zip(split_by_clip(trimmed, table), reference_frames(probs, table, trim=trim))):
        assert np.array_equal(t, wt), (trim, c)


def test_random_tables():
    rng = np.random.default_rng(5)
    for it in range(200):
        lengths = [int(n) for n in rng.choice([0, 0, 1, 2, 3, 9, 21, 40], size=rng.integers(1, 9))]
        preds = [random_pred(n, 1000 * it + c) for c, n in enumerate(lengths)]
        table = clip_table(lengths)
        probs = np.concatenate([probs_of(p, 1, it) for p in preds])
        trim = tuple(int(x) for x in rng.integers(0, 12, size=4))
        _, trimmed = frames_host_many(probs, table, trim=trim)
        want = [trim_voice_activity(np.asarray(p, np.uint8), *trim) for p in preds]
        assert np.array_equal(trimmed, np.concatenate(want)), (lengths, trim)


def test_each_seam_discriminates():
    """the host functions on the CONCATENATION of a seam's two clips give something else than on the clips alone: a batch path that
    ignored the table fails the comparisons of this file and of the GPU file"""
    for name, (a, b) in SEAMS.items():
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        alone = [trim_voice_activity(x, *TRIM) for x in (a, b)]
        joined = trim_voice_activity(np.concatenate([a, b]), *TRIM)
        segments_alone = [reference_segments(t) for t in alone]
        segments_joined = reference_segments(joined)
        if name == "voice":
            assert np.array_equal(joined, np.concatenate(alone))            # the frames agree: the seam shows in the segments only
            assert len(segments_joined[0]) == 1 and [len(s[0]) for s in segments_alone] == [1, 1]
            assert segments_alone[0][1][0] == len(convert_frames_to_samples(a, *GEOMETRY)) - 1   # ends at its clip's last sample
            assert segments_alone[1][0][0] == 0                                                  # starts at sample 0
        else:
            assert not np.array_equal(joined, np.concatenate(alone)), name
    # the rule each seam is there for, on the clips alone
    alone = {name: [trim_voice_activity(np.asarray(x, np.uint8), *TRIM) for x in pair] for name, pair in SEAMS.items()}
    assert alone["valley"][0][-2:].tolist() == [0, 0]                    # behind the hang-over: not filled
    assert alone["hill"][0][-2:].tolist() == [1, 1] and alone["hill"][1][:2].tolist() == [1, 1]
    assert not alone["hang_over"][1].any()
    assert alone["hang_before"][0][-10:].tolist() == [0] * 10


def test_slot_table_arithmetic():
    lib = _lib.load()
    for sr, hop_ms, win_ms in [GEOMETRY, (16000, 10.0, 10.0), (100, 10.0, 25.0), (16000, 10.0, 5.0), (8000, 10.0, 25.0), (16000, 12.5, 25.0)]:
        table = clip_table(LENGTHS)
        got = slot_table(table, sr, hop_ms, win_ms)
        slots = [len(convert_frames_to_samples(np.zeros(n), sr, hop_ms, win_ms)) + 1 if n else 0 for n in LENGTHS]
        assert got.dtype == np.int64 and got.tolist() == [0] + np.cumsum(slots).tolist(), (sr, hop_ms, win_ms)
    assert slot_table(clip_table([3]), *GEOMETRY).tolist() == [0, 2 * 160 + 400 + 1]
    assert slot_table(clip_table([0, 0]), *GEOMETRY).tolist() == [0, 0, 0]
    assert slot_table(clip_table([1]), 100, 10.0, 5.0).tolist() == [0, 1]          # a window of half a sample: the closing slot alone
    out = np.full(4, -7, dtype=np.int64)
    bad = np.array([0, 5, 4], dtype=np.int32)
    assert lib.savad_post_batch_slot_table(_p(bad), 2, 16000, 10.0, 25.0, _p(out)) == INVALID and b"decrease" in lib.savad_last_error()
    assert lib.savad_post_batch_slot_table(_p(clip_table([4])), 1, 30, 10.0, 25.0, _p(out)) == UNSUPPORTED
    assert (out == -7).all()


@pytest.mark.parametrize("geometry", [GEOMETRY, (16000, 10.0, 10.0), (100, 10.0, 25.0), (16000, 10.0, 5.0), (16000, 12.5, 25.0), (1000, 1.0, 1.0)])
def test_slot_classes_are_each_clips_own_and_close_every_clip(geometry):
    """a slot's class is savad_post_sample_class_host's for its clip alone, the slot behind a clip's samples is a closing slot (3),
    and a clip's first sample is never in between (2): it is covered by frame 0 alone under every supported geometry"""
    from tests.test_post_device_host import class_host

    probs, table = lengths_batch(1)
    _, trimmed = frames_host_many(probs, table, trim=(2, 2, 1, 1))
    cls = classes_host_many(trimmed, table, geometry)
    slots = slot_table(table, *geometry)
    for c, frames in enumerate(split_by_clip(trimmed, table)):
        own = cls[slots[c]:slots[c + 1]]
        if len(frames) == 0:
            assert len(own) == 0
            continue
        want = class_host(frames, *geometry)
        assert np.array_equal(own[:-1], want) and own[-1] == 3, (geometry, c)
        assert len(want) == 0 or want[0] != 2


def segments_from_classes(cls):
    """the batch segment rule in plain Python: the state restarts behind a closing slot; indices local to the clip"""
    out, voice, first, start = [[]], False, 0, None
    for j, c in enumerate(cls):
        if c == 3:
            if voice:
                out[-1].append((start, j - 1 - first))
            out.append([])
            voice, first = False, j + 1
        elif c == 1 and not voice:
            voice, start = True, j - first
        elif c == 0 and voice:
            voice = False
            out[-1].append((start, j - 1 - first))
    return out[:-1]


def test_segments_restart_at_every_clip():
    for name in ("lengths", "seams"):
        probs, table = batches(7)[name]
        _, trimmed = frames_host_many(probs, table)
        per_clip = iter(segments_from_classes(classes_host_many(trimmed, table)))
        total = 0
        for c, frames in enumerate(split_by_clip(trimmed, table)):
            starts, ends = reference_segments(frames)
            got = next(per_clip) if len(frames) else []
            assert got == list(zip(starts.tolist(), ends.tolist())), (name, c)
            total += len(got)
        assert total >= 3   # (the reference's own count: the inputs hold segments in several clips)


def test_supported_and_refusals():
    lib = _lib.load()
    from voice_activity_detection_amd.postprocessing import device_post_many_supported

    table = clip_table(LENGTHS)
    C = len(table) - 1
    assert lib.savad_post_batch_supported(_p(table), C, 7, 16000, 10.0, 25.0) == 1
    assert lib.savad_post_batch_supported(_p(table), C, 129, 16000, 10.0, 25.0) == 0
    assert lib.savad_post_batch_supported(_p(table), C, 7, 30, 10.0, 25.0) == 0
    assert lib.savad_post_batch_supported(_p(table), 0, 7, 16000, 10.0, 25.0) == 0
    assert lib.savad_post_batch_supported(None, C, 7, 16000, 10.0, 25.0) == 0
    assert lib.savad_post_batch_supported(_p(np.array([0, 5, 4], np.int32)), 2, 7, 16000, 10.0, 25.0) == 0
    assert lib.savad_post_batch_supported(_p(np.array([1, 5], np.int32)), 1, 7, 16000, 10.0, 25.0) == 0
    assert device_post_many_supported(table, 7) and not device_post_many_supported(table, 7, 30) and not device_post_many_supported(table, 7, None)

    probs = np.full((int(table[-1]), 7), 0.75, dtype=np.float32)
    boosted, trimmed = np.full(len(probs), -7, np.float32), np.full(len(probs), 9, np.uint8)
    fh = lib.savad_post_batch_frames_host
    decreasing, off_zero = np.array([0, 5, 4], dtype=np.int32), np.array([1, 5], dtype=np.int32)
    assert fh(_p(probs), None, C, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), _p(table), 0, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), _p(decreasing), 2, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID and b"decrease" in lib.savad_last_error()
    assert fh(_p(probs), _p(off_zero), 1, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), _p(table), C, 0, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID
    assert fh(_p(probs), _p(table), C, 129, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == UNSUPPORTED
    for k in range(4):
        trim = [0, 0, 0, 0]
        trim[k] = -1
        assert fh(_p(probs), _p(table), C, 7, 0.5, *trim, _p(boosted), _p(trimmed)) == INVALID and b"negative" in lib.savad_last_error()
    assert fh(None, _p(table), C, 7, 0.5, 0, 0, 0, 0, _p(boosted), _p(trimmed)) == INVALID and b"null" in lib.savad_last_error()
    assert fh(_p(probs), _p(table), C, 7, 0.5, 0, 0, 0, 0, None, _p(trimmed)) == INVALID
    assert (boosted == -7).all() and (trimmed == 9).all()                 # a refusal writes nothing
    assert fh(None, _p(clip_table([0, 0])), 2, 7, 0.5, 0, 0, 0, 0, None, None) == 0   # no rows: a no-op

    # the device entry points refuse from the host table and the scalars, before they touch the device
    size = ctypes.c_size_t(77)
    wb = lib.savad_post_batch_workspace_bytes
    assert wb(_p(table), C, 7, 16000, 10.0, 25.0, None) == INVALID
    assert wb(_p(decreasing), 2, 7, 16000, 10.0, 25.0, ctypes.byref(size)) == INVALID
    assert wb(_p(table), C, 129, 16000, 10.0, 25.0, ctypes.byref(size)) == UNSUPPORTED
    assert wb(_p(table), C, 7, 30, 10.0, 25.0, ctypes.byref(size)) == UNSUPPORTED and size.value == 77
    assert wb(_p(table), C, 7, 16000, 10.0, 25.0, ctypes.byref(size)) == 0 and size.value > 2 * int(slot_table(table)[-1])
    pf = lib.savad_post_batch_frames
    assert pf(None, _p(decreasing), None, 2, 7, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == INVALID
    assert pf(None, _p(table), None, C, 7, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == INVALID and b"null" in lib.savad_last_error()
    assert pf(None, _p(table), None, C, 7, 0.5, 0, 0, -3, 0, None, None, None, 0, None) == INVALID
    assert pf(None, _p(table), None, C, 200, 0.5, 0, 0, 0, 0, None, None, None, 0, None) == UNSUPPORTED
    seg_first, flags, longs = np.full(C + 1, -7, np.int64), np.full(C, 9, np.uint8), np.full(4, -7, np.int64)
    ps = lib.savad_post_batch_segments
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, 0, _p(seg_first), _p(flags), _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, _p(decreasing), None, 2, 16000, 10.0, 25.0, 0, _p(seg_first), _p(flags), _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, 0, _p(seg_first), _p(flags), _p(longs), _p(longs), -1, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, 1, _p(seg_first), _p(flags), _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, -5, _p(seg_first), _p(flags), _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, 0, None, _p(flags), _p(longs), _p(longs), 4, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 16000, 10.0, 25.0, 0, _p(seg_first), _p(flags), None, None, 4, None, 0, None) == INVALID
    assert ps(None, None, _p(table), None, C, 30, 10.0, 25.0, 0, _p(seg_first), _p(flags), _p(longs), _p(longs), 4, None, 0, None) == UNSUPPORTED
    assert (seg_first == -7).all() and (flags == 9).all() and (longs == -7).all()
    empty = clip_table([0, 0])
    assert ps(None, None, _p(empty), None, 2, 16000, 10.0, 25.0, 0, _p(seg_first), _p(flags), None, None, 0, None, 0, None) == 0   # no rows: no segments
    assert seg_first[:3].tolist() == [0, 0, 0] and flags[:2].tolist() == [0, 0]
