"""Every entry point of include/savad.h stays inside the buffers its caller handed in.

The other GPU tests pass fresh torch allocations, which the caching allocator rounds up to 512 bytes inside 2 MiB segments: a store a
few bytes past an odd-sized output, or a read of the 16-byte chunk behind the last sample that reaches a result, lands in slack and
goes unnoticed.  Here every case runs (1) the clean call -- the module / wrapper call on ordinary tensors, the one the parity tests hold
to oracles and goldens --, (2) the same call through the C ABI with every device buffer the caller owns inside a
tests/buffer_arena.py arena (outputs pre-filled with 0xA5 between 0xA5 guards, inputs between 0xFF guards = NaN / -1 / label 255, each
at exactly the alignment the header asks for), and asserts (3) that every guard and every input is intact and that every element the
header defines of every output has the clean call's bits.  Workspaces stay plain allocations of the reported size (their extents are
held by tests/test_gpu_schedule_workspace.py and tests/test_gpu_eval_device.py).  No tolerance is introduced: the two shapes without
an oracle comparison elsewhere (d_model 64 at [3, 9, 80], bf16 features at F = 13) also compare the clean call with oracle.forward at
tests/test_gpu_parity.py's constants.

The poison sits OUTSIDE the declared extents only (the exception: the probs rows / labels savad_eval_counts declares unused), and no
non-finite value enters a sequence the forward uses (known boundaries).

Guarded arguments (alignment of the placement) and shapes:
    savad_forward_ex             x (16), out (16): every precision x row_mode of the workspace test at [3,7,80] / [1,33,80] / [3,35,80];
                                 F = 13 at [3,7,13], [1,35,13]; bf16 features at [3,7,80], [3,35,80], [3,7,13]; d_model 64 at [3,9,80], [1,33,80]
    savad_forward_strided        feature (16), out (16): (T, hop, count) = (40, 8, 3), (33, 4, 5), first window 0 and 1
    savad_predict_probabilities  feature (16), probs (4), mean (4): (N, half, jump, chunk) = (61, 19, 9, 16), (9, 3, 1, 4), row_mode 0 / 1
    savad_gather_windows         feature, windows (16; 4 at F = 13), positions (8, or NULL); savad_boost: logp (8), positions (8), probs, mean (4)
    savad_gather_strided         feature, windows (16), the last window on the last row and zero-padded; savad_overlap_merge: logp (8), probs (4)
    savad_pcm16_to_f32           pcm (2, once 8), audio (16): n = 1, 3, 5, 1001; savad_ingest_downmix: raw (2 / 4), mono (4)
    savad_resample, _span        audio / slice (4), out (4): 48 kHz, 44.1 kHz, 8 kHz; middle and last span, exact and latest cut
    savad_logmel, _span          audio / slice (16 and 4), features (16): n = 159, 160, 513, 1601 x both algorithms; head / middle / tail span
    savad_frontend               audio (16 and 4), features (16): every config of tests/test_gpu_frontend.py, n = 1601 and the minimum;
                                 four geometries of tests/frontend_cases.py (odd hop, window off the 4-sample grid, K range past n_fft)
                                 at 10 frames, with and without differences ([N, 3F]), the workspace (16) guarded as well
    savad_post_frames            probs (4), boosted (4), trimmed (1): [61, 7], [1, 1]; _segments: trimmed (1), boosted (4); _sample_probs: out (8)
    savad_eval_counts            probs (4), labels (1): (N, n_labels) = (61, 61), (61, 50), (50, 61), block 0 / 64; savad_eval_sort: n = 61, 4097

test_module_accepts_unaligned_views: the Python surface takes contiguous views that start 4 bytes into a larger tensor (the 16-byte
rule is the C ABI's)."""
import ctypes

import numpy as np
import pytest

from tests.buffer_arena import BufferArena, same_bits
from tests.test_gpu_frontend import CONFIGS
from tests.test_gpu_parity import BF16_TOL, TIGHT
from tests.test_gpu_schedule_workspace import FORWARD_CASES, Knobs, feats, guarded_call, ptr

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16", "fp32s"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def states():
    """(feature size, d_model) -> seeded weights, 3 layers"""
    from voice_activity_detection_amd.seeded import seeded_state_dict

    return {(F, D): seeded_state_dict(1234, feature_size=F, num_layers=3, d_model=D) for F, D in ((80, 128), (13, 128), (80, 64))}


@pytest.fixture(scope="module")
def models(torch_cuda, states):
    from voice_activity_detection_amd import SelfAttentiveVAD

    out = {}
    for (F, D), st in states.items():
        m = SelfAttentiveVAD(F, 3, D, 0.5)
        m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in st.items()}, strict=True)
        out[F, D] = m.to("cuda").eval()
    return out


def lib_():
    from voice_activity_detection_amd import _lib

    return _lib.load()


def ok(rc):
    from voice_activity_detection_amd import _lib

    _lib.check(rc)


def stream_(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(torch, nbytes):
    """a plain allocation of the reported size"""
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws


def arena_(capacity=1 << 20):
    return BufferArena("cuda", capacity)


def out_f32(arena, shape, align, name):
    import torch

    return arena.place_output(4 * int(np.prod(shape)), align, torch.float32, name).view(shape)


# ---- forward ---------------------------------------------------------------------------------------------------------------------

def _forward_cases():
    """the precision x row_mode (x splits, batch_invariant) lists of the workspace test, at shapes whose B * T is odd: `out` is an odd
    number of 8-byte rows and ends off a 16-byte boundary"""
    seen, cases = set(), []
    for p in FORWARD_CASES:
        precision, shape, row_mode, kw = p.values
        kw = {k: v for k, v in kw.items() if k != "bf16_features"}   # (bf16 features have their own cases below)
        for new in ([(3, 7, 80)] if shape[1] <= 32 else [(1, 33, 80), (3, 35, 80)]):
            key = (precision, new, row_mode, tuple(sorted(kw.items())))
            if key not in seen:
                seen.add(key)
                cases.append((precision, new, 128, row_mode, kw, False))
    for precision in PRECISIONS:   # F = 13: 273 and 455 floats of x, rows zero-padded to 16 columns inside the workspace
        cases += [(precision, (3, 7, 13), 128, 0, {}, False), (precision, (1, 35, 13), 128, 0, {}, False)]
    cases += [("bf16", shape, 128, 0, {}, True) for shape in ((3, 7, 80), (3, 35, 80), (3, 7, 13))]   # (3, 7, 13): 546 bytes of x
    cases += [("fp32", (3, 9, 80), 64, 0, {}, False), ("fp32", (1, 33, 80), 64, 0, {}, False)]        # the generic kernels
    return [pytest.param(*c, id=f"{c[0]}-{'x'.join(map(str, c[1]))}-d{c[2]}-m{c[3]}" + "".join(f"-{k}{v}" for k, v in c[4].items())
                         + ("-bf16x" if c[5] else "")) for c in cases]


@pytest.mark.parametrize("precision,shape,d_model,row_mode,kw,bf16_features", _forward_cases())
def test_forward(torch_cuda, models, states, precision, shape, d_model, row_mode, kw, bf16_features):
    torch = torch_cuda
    B, T, F = shape
    x = feats(torch, 300 + T + F, shape)
    x_dtype = 0
    if bf16_features:
        x, x_dtype = x.to(torch.bfloat16), 1
    with Knobs(models[F, d_model], precision, row_mode, kw.get("splits", 0), kw.get("batch_invariant", False)) as model:
        with torch.no_grad():
            want = model(features=x)
        arena = arena_()
        xa = arena.place_input(x, 16, "x")
        out = out_f32(arena, (B, T, 2), 16, "out")
        assert xa.data_ptr() % 32 == 16 and out.data_ptr() % 32 == 16
        guarded_call(torch, model, lambda lib, h, nb: lib.savad_workspace_bytes(h, B, T, nb),
                     lambda lib, h, ws, n, st: lib.savad_forward_ex(h, ptr(xa), x_dtype, B, T, ptr(out), ws, n, st))
    arena.check()
    assert same_bits(out, want)
    if (d_model == 64 and shape == (3, 9, 80)) or (bf16_features and F == 13):   # no oracle comparison of these elsewhere
        from oracle import oracle

        ref = oracle.forward(states[F, d_model], x.float().cpu().numpy())
        err = float(np.abs(want.cpu().numpy() - ref).max())
        assert err < (BF16_TOL if precision == "bf16" else TIGHT), err


@pytest.mark.parametrize("T,hop,count", [(40, 8, 3), (33, 4, 5)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_strided_forward(torch_cuda, models, precision, T, hop, count):
    """windows read in place: the matrix has exactly T + hop (count - 1) rows, so the last window ends on its last row; with first > 0
    the rows in front of the first window are live data"""
    torch = torch_cuda
    F = 80
    rows = T + hop * (count - 1)
    feature = feats(torch, 400 + T, (rows, F))
    with Knobs(models[F, 128], precision, 0) as model:
        for first in (0, 1):
            n = count - first
            want = model.forward_windows(feature, T, hop, first, n)
            arena = arena_()
            fa = arena.place_input(feature, 16, "feature")
            out = out_f32(arena, (n, T, 2), 16, "out")
            x = ctypes.c_void_p(fa.data_ptr() + 4 * first * hop * F)
            guarded_call(torch, model, lambda lib, h, nb: lib.savad_workspace_bytes(h, n, T, nb),
                         lambda lib, h, ws, nb, st: lib.savad_forward_strided(h, x, 0, n, T, hop * F, ptr(out), ws, nb, st))
            arena.check()
            assert same_bits(out, want), first


# ---- predict and its pieces ------------------------------------------------------------------------------------------------------

GEOMETRIES = [(61, 19, 9, 16), (9, 3, 1, 4)]   # N, half, jump, chunk


@pytest.mark.parametrize("N,half,jump,chunk", GEOMETRIES)
@pytest.mark.parametrize("row_mode", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict(torch_cuda, models, precision, row_mode, N, half, jump, chunk):
    """the packed single launches read their windows straight out of the matrix, its first and last frames among them"""
    torch = torch_cuda
    F = 80
    feature = feats(torch, 500 + N, (N, F))
    with Knobs(models[F, 128], precision, row_mode) as model:
        want_probs, want_mean = model.predict_windows(feature, half, jump, chunk)
        W = want_probs.shape[1]
        arena = arena_()
        fa = arena.place_input(feature, 16, "feature")
        probs, mean = out_f32(arena, (N, W), 4, "probs"), out_f32(arena, (N,), 4, "mean")
        guarded_call(torch, model, lambda lib, h, nb: lib.savad_predict_workspace_bytes(h, N, half, jump, chunk, nb),
                     lambda lib, h, ws, n, st: lib.savad_predict_probabilities(h, ptr(fa), N, half, jump, chunk, ptr(probs), ptr(mean), ws, n, st))
    arena.check()
    assert same_bits(probs, want_probs) and same_bits(mean, want_mean)


@pytest.mark.parametrize("F", [80, 13])
@pytest.mark.parametrize("N,half,jump,chunk", GEOMETRIES)
def test_gather_windows_and_boost(torch_cuda, N, half, jump, chunk, F):
    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    W = lib.savad_window_offsets(half, jump, None)
    items = N - 2 * half
    feature = feats(torch, 600 + N + F, (N, F))
    fal = 16 if F % 4 == 0 else 4   # (16-byte pieces when the rows are whole ones, one float at a time otherwise)
    for first, count, with_positions in ((0, items, True), (1, items - 1, False)):
        want = torch.zeros((count, W, F), dtype=torch.float32, device="cuda")
        want_pos = torch.zeros((count, W), dtype=torch.int64, device="cuda")
        ok(lib.savad_gather_windows(ptr(feature), N, F, half, jump, first, count, ptr(want), ptr(want_pos), st))
        arena = arena_()
        fa = arena.place_input(feature, fal, "feature")
        win = out_f32(arena, (count, W, F), fal, "windows")
        pos = arena.place_output(8 * count * W, 8, torch.int64, "positions").view(count, W) if with_positions else None
        ok(lib.savad_gather_windows(ptr(fa), N, F, half, jump, first, count, ptr(win), ptr(pos) if with_positions else None, st))
        arena.check()
        assert same_bits(win, want) and same_bits(win, torch.stack([feature[want_pos[i]] for i in range(count)]))
        assert not with_positions or same_bits(pos, want_pos)
    if F != 80:
        return
    # the boosted prediction of all `items` windows: logp and positions in, probs and mean out (boosted_ws is scratch)
    pos_all = torch.zeros((items, W), dtype=torch.int64, device="cuda")
    scratch = torch.zeros((items, W, F), dtype=torch.float32, device="cuda")
    ok(lib.savad_gather_windows(ptr(feature), N, F, half, jump, 0, items, ptr(scratch), ptr(pos_all), st))
    logp = torch.from_numpy(np.log(np.random.default_rng(N).dirichlet([1, 1], size=(items, W))).astype(np.float32)).cuda()
    want_probs, want_mean = torch.zeros((N, W), device="cuda"), torch.zeros((N,), device="cuda")
    ok(lib.savad_boost(ptr(logp), ptr(pos_all), items, N, W, ptr(torch.empty((N, W, 2), device="cuda")), ptr(want_probs), ptr(want_mean), st))
    arena = arena_()
    la, pa = arena.place_input(logp, 8, "logp"), arena.place_input(pos_all, 8, "positions")
    probs, mean = out_f32(arena, (N, W), 4, "probs"), out_f32(arena, (N,), 4, "mean")
    ok(lib.savad_boost(ptr(la), ptr(pa), items, N, W, ptr(torch.empty((N, W, 2), device="cuda")), ptr(probs), ptr(mean), st))
    arena.check()
    assert same_bits(probs, want_probs) and same_bits(mean, want_mean)
    assert int((want_probs == 0.5).sum()) == N * W - items * W   # the slots no window fills


@pytest.mark.parametrize("T,hop,count", [(40, 8, 3), (33, 4, 5)])
def test_gather_strided(torch_cuda, T, hop, count):
    """the last window ends on the matrix's last row; with five rows fewer it is zero-padded instead of read"""
    torch = torch_cuda
    lib, st, F = lib_(), stream_(torch), 80
    rows = T + hop * (count - 1)
    for N in (rows, rows - 5):
        feature = feats(torch, 700 + T, (N, F))
        for first in (0, 1):
            n = count - first
            want = torch.full((n, T, F), 7.0, device="cuda")
            ok(lib.savad_gather_strided(ptr(feature), N, F, T, hop, first, n, ptr(want), st))
            arena = arena_()
            fa = arena.place_input(feature, 16, "feature")
            win = out_f32(arena, (n, T, F), 16, "windows")
            ok(lib.savad_gather_strided(ptr(fa), N, F, T, hop, first, n, ptr(win), st))
            arena.check()
            padded = torch.cat([feature, torch.zeros((rows - N, F), device="cuda")])
            assert same_bits(win, want) and same_bits(win, torch.stack([padded[hop * (first + w):hop * (first + w) + T] for w in range(n)]))


def test_overlap_merge(torch_cuda):
    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    N, T, hop = 101, 40, 8
    W = lib.savad_stream_window_count(N, T, hop)
    assert W == 9
    logp = torch.from_numpy(np.log(np.random.default_rng(5).dirichlet([1, 1], size=(W, T))).astype(np.float32)).cuda()
    want = torch.zeros((N,), device="cuda")
    ok(lib.savad_overlap_merge(ptr(logp), W, N, T, hop, ptr(want), st))
    arena = arena_()
    la = arena.place_input(logp, 8, "logp")
    probs = out_f32(arena, (N,), 4, "probs")
    ok(lib.savad_overlap_merge(ptr(la), W, N, T, hop, ptr(probs), st))
    arena.check()
    assert same_bits(probs, want) and bool(torch.isfinite(want).all())


# ---- audio in --------------------------------------------------------------------------------------------------------------------

def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.4 * np.sin(2 * np.pi * (300 + 900 * t) * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("n,align", [(1, 2), (3, 2), (5, 2), (1001, 2), (1001, 8)])
def test_pcm16_to_f32(torch_cuda, n, align):
    """8-byte pieces when the slice starts on one, a scalar tail; a 2-byte-aligned slice goes one sample at a time"""
    from voice_activity_detection_amd.features import pcm16_to_f32

    torch = torch_cuda
    pcm = torch.from_numpy(np.random.default_rng(n).integers(-32768, 32768, size=n).astype(np.int16)).cuda()
    want = pcm16_to_f32(pcm)
    arena = arena_()
    pa = arena.place_input(pcm, align, "pcm")
    audio = out_f32(arena, (n,), 16, "audio")
    ok(lib_().savad_pcm16_to_f32(ptr(pa), n, ptr(audio), stream_(torch)))
    arena.check()
    assert same_bits(audio, want) and same_bits(audio, pcm.float() / 32768.0)


@pytest.mark.parametrize("dtype,channels,frames", [("int16", 2, 1001), ("float32", 3, 333)])
def test_ingest_downmix(torch_cuda, dtype, channels, frames):
    from voice_activity_detection_amd.features import downmix_device

    torch = torch_cuda
    rng = np.random.default_rng(frames)
    raw = rng.integers(-32768, 32768, size=frames * channels).astype(np.int16) if dtype == "int16" else _signal(frames * channels, 3)
    raw = torch.from_numpy(raw).cuda()
    want = downmix_device(raw, channels)
    arena = arena_()
    ra = arena.place_input(raw, 2 if dtype == "int16" else 4, "raw")
    mono = out_f32(arena, (frames,), 4, "mono")
    ok(lib_().savad_ingest_downmix(ptr(ra), 0 if dtype == "int16" else 1, channels, frames, ptr(mono), stream_(torch)))
    arena.check()
    assert same_bits(mono, want)


# (rate, n_samples): 1001 and 1451 outputs; at 8 kHz the length is 2 n, never odd -- 3002 outputs still end off a 16-byte boundary
RESAMPLE = [(48000, 3001), (44100, 3999), (8000, 1501)]


@pytest.mark.parametrize("rate,n", RESAMPLE)
def test_resample(torch_cuda, rate, n):
    from voice_activity_detection_amd.features import _resample_lib, resample_length, resample_to_16k_device

    torch = torch_cuda
    lib, st = _resample_lib(), stream_(torch)
    x = torch.from_numpy(_signal(n, rate)).cuda()
    want = resample_to_16k_device(x, rate)
    n_out = resample_length(n, rate)
    assert want.shape == (n_out,) and (n_out % 2 == 1 or rate == 8000) and n_out % 4
    arena = arena_()
    xa = arena.place_input(x, 4, "audio")
    out = out_f32(arena, (n_out,), 4, "out")
    ok(lib.savad_resample(ptr(xa), n, rate, ptr(out), st))
    arena.check()
    assert same_bits(out, want)
    # spans from slices cut exactly at savad_resample_span_samples' answer, and as late at the front as the header allows: a middle
    # span and the last one (which includes fix_length's zero when there is one)
    from voice_activity_detection_amd.features import resample_span_samples

    for o0, o1 in ((n_out // 2, n_out // 2 + 97), (n_out - 97, n_out)):
        late = None
        for shift in range(16):   # the first span hereabouts whose lowest tap lies 3 samples behind the (rounded-down) *first
            a, c = resample_span_samples(n, rate, o0 + shift, o1 - o0 - shift)
            assert a % 4 == 0 and c > 0 and a + c <= n
            if shift == 0:
                exact = (a, c, o0, o1 - o0)
            probe = torch.empty(o1 - o0 - shift, device="cuda")
            rc = lib.savad_resample_span(ptr(x[a + 3:a + c].clone()), a + 3, c - 3, n, rate, o0 + shift, o1 - o0 - shift, ptr(probe), st)
            if rc == 0:
                late = (a + 3, c - 3, o0 + shift, o1 - o0 - shift)
                break
            assert rc == -1   # refused on the host, nothing launched: this span's lowest tap is closer to *first
        assert late is not None, "no span whose slice may start 3 samples later"
        for a, c, of, oc in (exact, late):
            arena = arena_()
            xa = arena.place_input(x[a:a + c], 4, "slice")
            out = out_f32(arena, (oc,), 4, "out")
            ok(lib.savad_resample_span(ptr(xa), a, c, n, rate, of, oc, ptr(out), st))
            arena.check()
            assert same_bits(out, want[of:of + oc]), (a, c, of, oc)


# ---- features --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algorithm", [0, 1])
@pytest.mark.parametrize("n", [159, 160, 513, 1601])
def test_logmel(torch_cuda, n, algorithm):
    from voice_activity_detection_amd.features import log_mel

    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    y = torch.from_numpy(_signal(n, n)).cuda()
    frames = lib.savad_logmel_frames(n)
    ok(lib.savad_logmel_set_algorithm(algorithm))
    try:
        want = log_mel(y, "cuda")
        assert want.shape == (frames, 80)
        for align in (16, 4):   # the direct reads / the copy path
            arena = arena_()
            ya = arena.place_input(y, align, "audio")
            out = out_f32(arena, (frames, 80), 16, "features")
            ws = workspace(torch, lib.savad_logmel_workspace_bytes(n))
            ok(lib.savad_logmel(ptr(ya), n, ptr(ws), ptr(out), st))
            arena.check()
            assert same_bits(out, want), align
    finally:
        ok(lib.savad_logmel_set_algorithm(0))


@pytest.mark.parametrize("frame_first,frame_count", [(0, 10), (40, 11), (91, 10)], ids=["head", "middle", "tail"])
def test_logmel_span(torch_cuda, frame_first, frame_count):
    """the slice cut exactly at savad_logmel_span_samples' answer: poison in front of it and behind it"""
    from voice_activity_detection_amd.features import log_mel, span_samples

    torch = torch_cuda
    lib, st, n = lib_(), stream_(torch), 16000
    y = torch.from_numpy(_signal(n, 16)).cuda()
    whole = log_mel(y, "cuda")
    assert whole.shape == (101, 80)
    a, c = span_samples(n, frame_first, frame_count)
    assert a % 4 == 0 and (a == 0) == (frame_first == 0) and (a + c == n) == (frame_first + frame_count == 101)
    for align in (16, 4):
        arena = arena_()
        ya = arena.place_input(y[a:a + c], align, "slice")
        out = out_f32(arena, (frame_count, 80), 16, "features")
        ws = workspace(torch, lib.savad_logmel_span_workspace_bytes(frame_count))
        ok(lib.savad_logmel_span(ptr(ya), a, c, n, frame_first, frame_count, ptr(ws), ptr(out), st))
        arena.check()
        assert same_bits(out, whole[frame_first:frame_first + frame_count]), align


@pytest.mark.parametrize("c", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_frontend(torch_cuda, c):
    """n = 1601 and the smallest signal the config takes; the 13- and 161-column outputs end off a 16-byte boundary"""
    from voice_activity_detection_amd.features import FrontEnd

    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    fe = FrontEnd(*c, False)
    cfg = fe.config()
    for n in (1601, fe.n_fft if fe.transform == "spectrogram" else fe.n_fft // 2 + 1):
        y = torch.from_numpy(_signal(n, n + fe.n_fft)).cuda()
        want = fe.extract(y, "cuda", generic=True)
        N, F, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        ok(lib.savad_frontend_shape(ctypes.byref(cfg), n, ctypes.byref(N), ctypes.byref(F)))
        ok(lib.savad_frontend_workspace_bytes(ctypes.byref(cfg), n, ctypes.byref(nb)))
        assert want.shape == (N.value, F.value) == (fe.frames(n), fe.feature_size)
        for align in (16, 4):
            arena = arena_()
            ya = arena.place_input(y, align, "audio")
            out = out_f32(arena, (N.value, F.value), 16, "features")
            ws = workspace(torch, nb.value)
            ok(lib.savad_frontend(ctypes.byref(cfg), ptr(ya), n, ptr(ws), ptr(out), st))
            arena.check()
            assert same_bits(out, want), (n, align)


# tests/frontend_cases.py: an odd-hop spectrogram, an odd-hop centred case, a window off the 4-sample grid, the K range past n_fft
FRONTEND_CASE_IDS = ["spectrogram-320-163-320", "mfcc-512-101-400-40-13", "log-mel-500-160-401-80", "spectrogram-402-160-401"]


@pytest.mark.parametrize("deltas", [False, True], ids=["base", "deltas"])
@pytest.mark.parametrize("case_id", FRONTEND_CASE_IDS)
def test_frontend_cases(torch_cuda, case_id, deltas):
    """10 frames, ending with the last frame (the spectrogram (402, 160, 401) then reads a copy) and 8 samples later (it reads the audio);
    the workspace too lies between guards, at exactly the reported size; with deltas the [N, 3F] output is the guarded one"""
    from tests import frontend_cases as fc
    from voice_activity_detection_amd.features import FrontEnd

    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    case = fc.BY_ID[case_id]
    fe = FrontEnd(*fc.front_end_args(case, deltas))
    cfg = fe.config()
    for n in (fc.length_for(case, 10), fc.length_for(case, 10, 8)):
        y = torch.from_numpy(_signal(n, n + fe.n_fft)).cuda()
        want = fe.extract(y, "cuda")
        N, F, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        ok(lib.savad_frontend_shape(ctypes.byref(cfg), n, ctypes.byref(N), ctypes.byref(F)))
        ok(lib.savad_frontend_workspace_bytes(ctypes.byref(cfg), n, ctypes.byref(nb)))
        assert want.shape == (N.value, F.value) == (10, (3 if deltas else 1) * fc.base_size(case))
        for align in (16, 4):
            arena = arena_()
            ya = arena.place_input(y, align, "audio")
            out = out_f32(arena, (N.value, F.value), 16, "features")
            ws = arena.place_output(nb.value, 16, torch.uint8, "workspace")
            ok(lib.savad_frontend(ctypes.byref(cfg), ptr(ya), n, ptr(ws), ptr(out), st))
            arena.check()
            assert same_bits(out, want), (n, align)


# ---- post-processing -------------------------------------------------------------------------------------------------------------

TRIM = dict(min_vally=2, min_hill=2, hang_before=1, hang_over=1)
GEOMETRY = (16000, 10.0, 25.0)   # sample rate, hop and window in ms


def _post_probs(N, W):
    """speech for the first three quarters with a dip inside (where a split lands), flickers that the trim removes, silence after"""
    rng = np.random.default_rng(N)
    p = rng.uniform(0.0, 0.35, size=(N, W)).astype(np.float32)
    if N < 4:
        return p + np.float32(0.6)
    p[: 3 * N // 4] += 0.6
    p[N // 3] -= 0.2
    p[N // 2: N // 2 + 1] = 0.1
    p[-3] = 0.9
    return p


def _post_ws(torch, N, W):
    nb = ctypes.c_size_t()
    ok(lib_().savad_post_workspace_bytes(N, W, GEOMETRY[0], GEOMETRY[1], GEOMETRY[2], ctypes.byref(nb)))
    return workspace(torch, nb.value), nb.value


@pytest.fixture
def post_block(request):
    lib = lib_()
    ok(lib.savad_post_set_block(request.param))
    try:
        yield request.param
    finally:
        ok(lib.savad_post_set_block(0))


@pytest.mark.parametrize("post_block,N,W", [(0, 61, 7), (0, 1, 1), (64, 61, 7)], indirect=["post_block"])
def test_post_processing(torch_cuda, post_block, N, W):
    """savad_post_frames (boosted: 4 N bytes, trimmed: N bytes -- 61 is odd), savad_post_segments without and with a split,
    savad_post_sample_probs (float64); at 64 elements per block the scans over the samples run several levels"""
    from voice_activity_detection_amd.postprocessing import post_frames_device, sample_probs_device, segments_device

    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    probs = torch.from_numpy(_post_probs(N, W)).cuda()
    want_boosted, want_trimmed = post_frames_device(probs, 0.5, **TRIM)
    arena = arena_()
    pa = arena.place_input(probs, 4, "probs")
    boosted = out_f32(arena, (N,), 4, "boosted")
    trimmed = arena.place_output(N, 1, torch.uint8, "trimmed")
    ws, nb = _post_ws(torch, N, W)
    ok(lib.savad_post_frames(ptr(pa), N, W, 0.5, TRIM["min_vally"], TRIM["min_hill"], TRIM["hang_before"], TRIM["hang_over"], ptr(boosted),
                             ptr(trimmed), ptr(ws), nb, st))
    arena.check()
    assert same_bits(boosted, want_boosted) and same_bits(trimmed, want_trimmed)
    if N > 1:
        assert 0 < int(want_trimmed.sum()) < N

    for max_seconds in (None, 0.125):   # 0.125 s = 2000 samples: the 45-frame segment is split
        want_starts, want_ends = segments_device(want_trimmed, want_boosted, *GEOMETRY, max_length_seconds=max_seconds)
        arena = arena_()
        ta, ba = arena.place_input(want_trimmed, 1, "trimmed"), arena.place_input(want_boosted, 4, "boosted")
        cap = N + 2
        starts, ends = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64)
        ws, nb = _post_ws(torch, N, 1)
        count = lib.savad_post_segments(ptr(ta), ptr(ba), N, GEOMETRY[0], GEOMETRY[1], GEOMETRY[2], int(max_seconds * GEOMETRY[0]) if max_seconds else 0,
                                        ctypes.c_void_p(starts.ctypes.data), ctypes.c_void_p(ends.ctypes.data), cap, ptr(ws), nb, st)
        arena.check()
        assert count == len(want_starts) and np.array_equal(starts[:count], want_starts) and np.array_equal(ends[:count], want_ends)
        if N > 1:
            assert count >= (3 if max_seconds else 1)

    want = sample_probs_device(want_boosted, *GEOMETRY)
    arena = arena_()
    ba = arena.place_input(want_boosted, 4, "boosted")
    out = arena.place_output(8 * want.numel(), 8, torch.float64, "sample probs")
    ok(lib.savad_post_sample_probs(ptr(ba), N, GEOMETRY[0], GEOMETRY[1], GEOMETRY[2], ptr(out), st))
    arena.check()
    assert want.numel() == (N - 1) * 160 + 400 and same_bits(out, want)


# ---- evaluate --------------------------------------------------------------------------------------------------------------------

EVAL_L = 5


@pytest.fixture
def eval_block(request):
    lib = lib_()
    ok(lib.savad_eval_set_block(request.param))
    try:
        yield request.param
    finally:
        ok(lib.savad_eval_set_block(0))


def _eval_counts(torch, probs, N, W, labels, n_labels):
    from voice_activity_detection_amd.metrics import EVAL_COUNTERS

    lib = lib_()
    nb = ctypes.c_size_t()
    ok(lib.savad_eval_workspace_bytes(N, W, ctypes.byref(nb)))
    ws = workspace(torch, nb.value)
    counters = np.full(EVAL_COUNTERS, -1, dtype=np.int64)
    seg = np.full(((min(N, n_labels) + 1) // 2, 8), 0xEE, dtype=np.uint8)
    count = lib.savad_eval_counts(ptr(probs), N, W, ptr(labels), n_labels, 0.5, EVAL_L, ctypes.c_void_p(counters.ctypes.data),
                                  ctypes.c_void_p(seg.ctypes.data), len(seg), ptr(ws), nb.value, stream_(torch))
    assert count >= 0, lib.savad_last_error()
    return count, counters, seg


@pytest.mark.parametrize("N,n_labels", [(61, 61), (61, 50), (50, 61)])
@pytest.mark.parametrize("eval_block", [0, 64], indirect=True)
def test_eval_counts(torch_cuda, eval_block, N, n_labels):
    """"everything works on n = min(N, n_labels) frames": the probs rows behind n are NaN and the labels behind n are 255 -- inside the
    extents, declared unused -- and outside the extents sits the arena's poison; the NaN and bad-label counters stay 0"""
    from voice_activity_detection_amd.metrics import EVAL_BAD_LABEL, EVAL_NAN

    torch = torch_cuda
    W, n = 7, min(N, n_labels)
    rng = np.random.default_rng(61)
    labels_np = (np.convolve(rng.standard_normal(61), np.ones(5) / 5, mode="same") > 0).astype(np.uint8)
    labels_np[0], labels_np[n - 1] = 1, 1   # a segment at each end of the frames that count
    probs_np = np.clip(labels_np[:, None] * 0.5 + rng.uniform(0.0, 0.7, size=(61, W)), 0, 1).astype(np.float32)
    clean = _eval_counts(torch, torch.from_numpy(probs_np[:n]).cuda(), n, W, torch.from_numpy(labels_np[:n]).cuda(), n)
    probs_np, labels_np = probs_np[:N].copy(), labels_np[:n_labels].copy()
    probs_np[n:] = np.nan
    labels_np[n:] = 255
    arena = arena_()
    pa = arena.place_input(torch.from_numpy(probs_np).cuda(), 4, "probs")
    la = arena.place_input(torch.from_numpy(labels_np).cuda(), 1, "labels")
    count, counters, seg = _eval_counts(torch, pa, N, W, la, n_labels)
    arena.check()
    assert counters[EVAL_NAN] == 0 and counters[EVAL_BAD_LABEL] == 0 and counters[0] == n
    assert count == clean[0] and count >= 2 and counters.tolist() == clean[1].tolist()
    assert np.array_equal(seg[:count], clean[2][:count]) and (seg[count:] == 0xEE).all()


@pytest.mark.parametrize("n", [61, 4097])
def test_eval_sort(torch_cuda, n):
    torch = torch_cuda
    lib, st = lib_(), stream_(torch)
    rng = np.random.default_rng(n)
    keys = torch.from_numpy(rng.choice(np.array([-2.5, -0.0, 0.0, 0.25, 0.5, 1.0, 7.0], np.float32), size=n) + (rng.standard_normal(n) > 1).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, 2, size=n).astype(np.uint8)).cuda()
    nb = ctypes.c_size_t()
    ok(lib.savad_eval_workspace_bytes(n, 1, ctypes.byref(nb)))
    want_keys, want_labels = torch.zeros((n,), device="cuda"), torch.zeros((n,), dtype=torch.uint8, device="cuda")
    ok(lib.savad_eval_sort(ptr(keys), ptr(labels), n, ptr(want_keys), ptr(want_labels), ptr(workspace(torch, nb.value)), nb.value, st))
    arena = arena_()
    ka, la = arena.place_input(keys, 4, "keys"), arena.place_input(labels, 1, "labels")
    out_keys = out_f32(arena, (n,), 4, "sorted keys")
    out_labels = arena.place_output(n, 1, torch.uint8, "sorted labels")
    ok(lib.savad_eval_sort(ptr(ka), ptr(la), n, ptr(out_keys), ptr(out_labels), ptr(workspace(torch, nb.value)), nb.value, st))
    arena.check()
    assert same_bits(out_keys, want_keys) and same_bits(out_labels, want_labels)
    order = np.argsort(keys.cpu().numpy(), kind="stable")
    assert np.array_equal(want_keys.cpu().numpy(), keys.cpu().numpy()[order]) and np.array_equal(want_labels.cpu().numpy(), labels.cpu().numpy()[order])


# ---- the Python surface takes any tensor -----------------------------------------------------------------------------------------

def off4(torch, t):
    """a contiguous view with t's contents that starts 4 bytes into a larger tensor"""
    buf = torch.empty(t.numel() * t.element_size() + 4, dtype=torch.uint8, device=t.device)
    v = buf[4:].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("precision", PRECISIONS)
def test_module_accepts_unaligned_views(torch_cuda, models, precision):
    """model(features=v), model(features=x, out=o), predict_windows and forward_windows on views that start 4 bytes into a larger
    tensor (batch[1:] of [B, 7, 13] MFCC windows is one): the bits of the call on clones; `out` is written in place"""
    torch = torch_cuda
    for F, shape in ((13, (3, 7, 13)), (80, (3, 7, 80)), (80, (2, 35, 80))):
        with Knobs(models[F, 128], precision, 0) as model, torch.no_grad():
            if F == 13:
                batch = feats(torch, 800, (4, 7, 13))
                v = batch[1:]   # 91 floats in: 364 bytes, 12 past a 16-byte boundary
                assert v.is_contiguous() and v.data_ptr() % 16 == 12
            else:
                v = off4(torch, feats(torch, 801 + shape[1], shape))
            want = model(features=v.clone())
            assert same_bits(model(features=v), want)
            if precision == "bf16":
                vb = off4(torch, v.to(torch.bfloat16))
                assert same_bits(model(features=vb), model(features=vb.clone()))
            o = off4(torch, torch.full(shape[:2] + (2,), 7.0, device="cuda"))
            assert model(features=v.clone(), out=o) is o and same_bits(o, want)
            o.fill_(7.0)
            assert model(features=v, out=o) is o and same_bits(o, want)
    with Knobs(models[80, 128], precision, 0) as model:
        fv = off4(torch, feats(torch, 810, (61, 80)))
        got, want = model.predict_windows(fv, 19, 9, 16), model.predict_windows(fv.clone(), 19, 9, 16)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        for T, hop, count in ((40, 8, 3), (7, 3, 5)):   # read in place / gathered first (savad_gather_strided)
            fm = off4(torch, feats(torch, 811, (T + hop * (count - 1), 80)))
            want = model.forward_windows(fm.clone(), T, hop, 1, count - 1)
            assert same_bits(model.forward_windows(fm, T, hop, 1, count - 1), want)
            o = off4(torch, torch.full((count - 1, T, 2), 7.0, device="cuda"))
            assert model.forward_windows(fm, T, hop, 1, count - 1, out=o) is o and same_bits(o, want)


def test_wrappers_accept_unaligned_views(torch_cuda):
    """features.py, postprocessing.py and evaluate.py with one view each that starts 4 bytes (int16: 2 bytes) into a larger tensor"""
    from tests.eval_cases import assert_same_metrics, outcome
    from voice_activity_detection_amd import features as ft
    from voice_activity_detection_amd.evaluate import file_metrics, file_metrics_device
    from voice_activity_detection_amd.features import FrontEnd
    from voice_activity_detection_amd.postprocessing import post_frames_device, sample_probs_device, segments_device

    torch = torch_cuda
    y = torch.from_numpy(_signal(1601, 9)).cuda()
    yv = off4(torch, y)
    assert same_bits(ft.log_mel(yv, "cuda"), ft.log_mel(y, "cuda"))
    a, c = ft.span_samples(1601, 3, 5)
    assert same_bits(ft.log_mel_span(off4(torch, y[a:a + c]), a, 1601, 3, 5), ft.log_mel_span(y[a:a + c].clone(), a, 1601, 3, 5))
    fe = FrontEnd(*CONFIGS[4], False)   # MFCC, 13 columns
    assert same_bits(fe.extract(yv, "cuda"), fe.extract(y, "cuda"))
    assert same_bits(ft.resample_to_16k_device(yv, 44100), ft.resample_to_16k_device(y, 44100))
    raw = torch.from_numpy(np.random.default_rng(2).integers(-32768, 32768, size=2003).astype(np.int16)).cuda()
    pcm = raw[1:]
    assert pcm.data_ptr() % 4 == 2
    assert same_bits(ft.pcm16_to_f32(pcm), ft.pcm16_to_f32(pcm.clone()))
    assert same_bits(ft.downmix_device(pcm, 2), ft.downmix_device(pcm.clone(), 2))
    mono = off4(torch, torch.zeros(1001, device="cuda"))
    assert ft.downmix_device(pcm, 2, out=mono) is mono and same_bits(mono, ft.downmix_device(pcm.clone(), 2))
    probs = torch.from_numpy(_post_probs(61, 7)).cuda()
    pv = off4(torch, probs)
    boosted, trimmed = post_frames_device(probs, 0.5, **TRIM)
    got = post_frames_device(pv, 0.5, **TRIM)
    assert same_bits(got[0], boosted) and same_bits(got[1], trimmed)
    bv, tv = off4(torch, boosted), torch.cat([trimmed[:1], trimmed])[1:]
    assert tv.data_ptr() % 2 == 1
    for a, b in zip(segments_device(tv, bv, *GEOMETRY, max_length_seconds=0.125), segments_device(trimmed, boosted, *GEOMETRY, max_length_seconds=0.125)):
        assert np.array_equal(a, b)
    assert same_bits(sample_probs_device(bv, *GEOMETRY), sample_probs_device(boosted, *GEOMETRY))
    labels = (probs.mean(dim=1) > 0.5).cpu().numpy().astype(np.uint8)
    assert_same_metrics(outcome(file_metrics_device, labels, pv, 0.5), outcome(file_metrics, labels, probs.cpu().numpy(), 0.5), "view")
