"""The generic feature front-end (savad_frontend, features.FrontEnd) on the MI355X at the cases of tests/frontend_cases.py: the
scalar-load STFT (hop % 4 != 0), windows that start off the 4-sample grid, the largest / smallest / odd n_fft, the output widths at the
GEMM's tile edges and the frame counts at the workgroup's, each against the float64 restatement per frame at 3 x the fp32 floor
(tests/test_frontend_cases_host.py holds floors, bounds and deviations on the CPU); bit stability under every audio placement, a dirty
workspace and a workspace a louder call used; the MFCC maximum below zero; graph replay of a scalar-load config."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

from tests import frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


def _front(case, deltas=False):
    from voice_activity_detection_amd.features import FrontEnd

    return FrontEnd(*fc.front_end_args(case, deltas))


def _sizes(fe, n):
    from voice_activity_detection_amd import _lib

    lib, cfg = _lib.load(), fe.config()
    N, F, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _lib.check(lib.savad_frontend_shape(ctypes.byref(cfg), n, ctypes.byref(N), ctypes.byref(F)))
    _lib.check(lib.savad_frontend_workspace_bytes(ctypes.byref(cfg), n, ctypes.byref(nb)))
    return N.value, F.value, nb.value


def _abi(torch, fe, y_dev, ws=None, fill=0):
    """savad_frontend through the C ABI on a workspace of the reported size: the caller's (as the last call left it), or a new one
    filled with the byte `fill`"""
    from voice_activity_detection_amd import _lib

    n = y_dev.numel()
    N, F, nb = _sizes(fe, n)
    if ws is None:
        ws = torch.full((nb,), fill, dtype=torch.uint8, device="cuda")
    assert ws.numel() == nb and ws.data_ptr() % 16 == 0
    out = torch.empty((N, F), dtype=torch.float32, device="cuda")
    cfg = fe.config()
    _lib.check(_lib.load().savad_frontend(ctypes.byref(cfg), ctypes.c_void_p(y_dev.data_ptr()), n, ctypes.c_void_p(ws.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu().numpy(), ws


def _placed(torch, y, floats_off):
    """y on the device, starting 4 * floats_off bytes past a 16-byte boundary"""
    buf = torch.zeros(len(y) + 4, dtype=torch.float32, device="cuda")
    v = buf[floats_off:floats_off + len(y)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(y)))
    assert v.data_ptr() % 16 == 4 * floats_off and v.is_contiguous()
    return v


def _signal(r):
    return fc.signal(r).copy()    # (the shared one is read-only)


def _delta_modes(r):
    return (False, True) if fc.frames_of(r.case, r.n) >= 9 else (False,)


def _report(r, deltas, figures, bounds):
    print("FIGURES " + json.dumps({"run": fc.run_id(r), "deltas": deltas, "error": figures, "bound": bounds}))


# ---- every case x its signals against the truth -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", fc.RUNS, ids=fc.run_id)
def test_case_matches_reference(torch_cuda, r):
    y = _signal(r)
    for deltas in _delta_modes(r):
        fe = _front(r.case, deltas)
        got = fe.extract(y, "cuda").cpu().numpy()
        assert got.shape == (fe.frames(len(y)), fe.feature_size) == (fc.frames_of(r.case, r.n), (3 if deltas else 1) * fc.base_size(r.case))
        _report(r, deltas, *fc.check(r, got, deltas))


def test_empty_filters_give_exactly_the_log_floor(torch_cuda):
    """n_mels 256 at n_fft 400: 45 filters hold no bin, their mel is exactly zero"""
    from tests import frontend_ref as ref

    case = fc.BY_ID["log-mel-400-160-400-256"]
    empty = ref.mel_basis(400, 256).sum(axis=1) == 0
    assert int(empty.sum()) == 45
    got = _front(case).extract(fc.chirp(fc.default_length(case)), "cuda").cpu().numpy()
    floor = got[0, empty][0]
    assert (got[:, empty] == floor).all() and (got[:, ~empty] != floor).any()      # one value, whatever the frame holds
    assert abs(float(floor) - np.log(1e-6)) <= 2 * np.spacing(np.float32(13.8))    # logf(1e-6f) to 2 ulp


@pytest.mark.parametrize("case", [fc.BY_ID["mfcc-512-101-400-40-13"], fc.BY_ID["spectrogram-320-163-320"], fc.BY_ID["log-mel-500-160-401-80"]],
                         ids=lambda c: c.id)
def test_refusals_stay(torch_cuda, case):
    from voice_activity_detection_amd import _lib

    fe = _front(case, True)
    assert fe.frames(fc.length_for(case, 9)) == 9
    with pytest.raises(_lib.SavadError, match="at least 9"):
        fe.extract(fc.chirp(fc.length_for(case, 8, case.hop - 1)), "cuda")       # the longest signal of 8 frames
    lo = case.n_fft if case.transform == "spectrogram" else case.n_fft // 2 + 1
    assert _front(case).extract(fc.chirp(lo), "cuda").shape[0] == fc.frames_of(case, lo)
    with pytest.raises(_lib.SavadError, match="n_samples >="):
        _front(case).extract(fc.chirp(lo - 1), "cuda")


# ---- bit stability ------------------------------------------------------------------------------------------------------------------

STABLE = ["log-mel-512-161-400-80", "spectrogram-320-161-320", "spectrogram-320-162-320", "spectrogram-320-163-320",   # hop % 4 = 1, 1, 2, 3
          "log-mel-500-160-400-80", "spectrogram-512-160-401", "log-mel-500-101-401-40"]                              # lpad 50, 55, 49 (hop % 4 = 1)


@pytest.mark.parametrize("case", [fc.BY_ID[i] for i in STABLE], ids=STABLE)
def test_placement_repeats_and_dirty_workspace_give_the_same_bits(torch_cuda, case):
    torch = torch_cuda
    fe = _front(case, True)
    y = fc.chirp(fc.default_length(case), 5)
    want = fe.extract(y, "cuda").cpu().numpy()                        # a host array
    for off in (1, 2, 3):                                             # 4, 8 and 12 bytes past a 16-byte boundary
        v = _placed(torch, y, off)
        assert np.array_equal(fe.extract(v, "cuda").cpu().numpy(), want), off
        assert np.array_equal(fe.extract(v.clone(), "cuda").cpu().numpy(), want), off
    v = _placed(torch, y, 0)
    assert np.array_equal(fe.extract(v, "cuda").cpu().numpy(), want)
    assert np.array_equal(fe.extract(v, "cuda").cpu().numpy(), want)   # two calls
    for src in (v, _placed(torch, y, 1)):
        zeroed, _ = _abi(torch, fe, src, fill=0)
        dirty, _ = _abi(torch, fe, src, fill=0xFF)                    # NaN wherever a kernel reads what no kernel wrote
        assert np.array_equal(zeroed, want) and np.array_equal(dirty, want)


def test_spectrogram_k_range_past_n_fft_reads_the_audio_or_a_copy(torch_cuda):
    """(402, 160, 401): k0 + kr = 408.  A signal that ends with its last frame is read from an aligned copy, 8 more samples let the
    kernel read the audio in place, audio 4 bytes off a 16-byte boundary is copied either way: the frames have the same bits"""
    torch = torch_cuda
    case, N = fc.SP402, 36
    assert fc.geometry(case) == (0, 0, 408)
    n = fc.length_for(case, N)
    assert n == case.n_fft + case.hop * (N - 1) and case.hop * (N - 1) + 408 > n and case.hop * (N - 1) + 408 <= n + 8
    y = fc.chirp(n + 8, 9)
    for deltas in (False, True):
        fe = _front(case, deltas)
        outs = [fe.extract(_placed(torch, y[:m], off), "cuda").cpu().numpy() for m in (n, n + 8) for off in (0, 1)]
        assert outs[0].shape == (N, (3 if deltas else 1) * 202)
        assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    r = fc.Run(case, "chirp", n)
    got = _front(case, True).extract(_placed(torch, _signal(r), 0), "cuda").cpu().numpy()
    _report(r, True, *fc.check(r, got, True))


# ---- the MFCC maximum -----------------------------------------------------------------------------------------------------------------

MFCC = fc.BY_ID["mfcc-512-101-400-40-13"]


def test_mfcc_of_silence_is_the_dct_of_a_constant_row(torch_cuda):
    """every mel at the amin floor: -100 dB everywhere, maximum -100, no clamp: coefficient 0 = -100 sqrt(n_mels), the others vanish"""
    for case in (MFCC, fc.BY_ID["mfcc-512-160-400-64-64"]):
        r = next(r for r in fc.RUNS if r.case == case and r.signal == "zeros")
        got = _front(case, True).extract(_signal(r), "cuda").cpu().numpy()
        F = case.n_mfcc
        assert (got == got[0]).all()                                              # one row, repeated
        assert abs(got[0, 0] + 100 * np.sqrt(case.n_mels)) < 1e-3 and np.abs(got[0, 1:]).max() < 1e-3   # (the differences vanish too)
        fc.check(r, got, True)


def test_mfcc_maximum_is_reset_per_call(torch_cuda):
    """a quiet call (maximum -67 dB: the negative branch of the float's integer image) on the workspace a loud call (+13 dB) just used"""
    torch = torch_cuda
    fe = _front(MFCC, True)
    rq = next(r for r in fc.RUNS if r.case == MFCC and r.signal == "quiet")
    rl = next(r for r in fc.RUNS if r.case == MFCC and r.signal == "chirp")
    quiet, loud = torch.from_numpy(_signal(rq)).cuda(), torch.from_numpy(_signal(rl)).cuda()
    fresh, _ = _abi(torch, fe, quiet)
    fc.check(rq, fresh, True)
    first, ws = _abi(torch, fe, loud)
    fc.check(rl, first, True)
    after, ws = _abi(torch, fe, quiet, ws)
    assert np.array_equal(after, fresh)
    again, _ = _abi(torch, fe, loud, ws)
    assert np.array_equal(again, first)


# ---- graph replay -------------------------------------------------------------------------------------------------------------------

def test_graph_mode_equals_eager_for_a_scalar_load_config(torch_cuda, tmp_path):
    from tests.test_gpu_frontend import _checkpoint
    from voice_activity_detection_amd.predictor import VADFromScratchPredictor

    transform = {"name": "mfcc", "n_fft": 512, "hop_ms": fc.hop_ms(MFCC), "window_ms": fc.window_ms(MFCC), "n_mels": 40, "n_mfcc": 13}
    path, _ = _checkpoint(tmp_path, transform, True, 39)
    eager = VADFromScratchPredictor.from_checkpoint(path, "cuda", extended_front_end=True)
    pg = VADFromScratchPredictor.from_checkpoint(path, "cuda", extended_front_end=True)
    assert eager.front_end.hop == 101
    pg.graph = True
    y = fc.chirp(16000 + 19, 8)
    pe, me = eager.predict_audio_device(y)
    pe, me = pe.cpu().numpy(), me.cpu().numpy()
    for _ in range(2):
        p, m = pg.predict_audio_device(y)
        assert np.array_equal(p.cpu().numpy(), pe) and np.array_equal(m.cpu().numpy(), me)
    assert pg.graph_stats["captures"] == 1 and pg.graph_stats["replays"] == 2
