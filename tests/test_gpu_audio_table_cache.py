"""The device-table cache of the audio paths (csrc/savad.hip: DeviceTables) with its keys ALTERNATING: every other GPU test takes one
front-end config or one source rate per run and never comes back to it after others were used.  Here three configs, three rates and
both log-mel algorithms take turns twice; the second round must repeat the first bit for bit, and the first round meets the
references of the paths' own tests at those tests' bounds (tests/frontend_ref.py as in test_gpu_frontend.py, oracle.resample and
oracle.logmel as in test_gpu_ingest.py / test_gpu_parity.py)."""
import numpy as np
import pytest

from oracle import logmel
from oracle import resample as orc
from tests import frontend_ref as ref
from tests.test_gpu_frontend import _check, _chirp

pytestmark = pytest.mark.gpu

CONFIGS = [  # (transform, n_fft, hop_ms, window_ms, n_mels, n_mfcc), deltas
    (("log-mel", 512, 10, 25, 80, None), False),     # the shipped geometry through the generic kernels
    (("mel", 400, 10, 25, 40, None), False),
    (("mfcc", 256, 5, 12.5, 40, 13), True),
]
RATES = (48000, 8000, 22050)


def test_alternating_keys_keep_their_tables():
    import torch

    from voice_activity_detection_amd import _lib
    from voice_activity_detection_amd.features import FrontEnd, log_mel, resample_prepare, resample_to_16k_device

    assert torch.cuda.is_available(), "needs a HIP device"
    lib = _lib.load()
    y = _chirp(4000, 21)
    yd = torch.from_numpy(y).cuda()
    fronts = [FrontEnd(*c, deltas) for c, deltas in CONFIGS]
    assert [(f.n_fft, f.hop, f.win) for f in fronts] == [(512, 160, 400), (400, 160, 400), (256, 80, 200)]
    t = np.arange(3001)
    x = {rate: (0.4 * np.sin(2 * np.pi * (300 + 4000 * t / rate) * t / rate)
                + 0.1 * np.random.default_rng(rate).standard_normal(3001)).astype(np.float32) for rate in RATES}
    xd = {rate: torch.from_numpy(v).cuda() for rate, v in x.items()}

    def one_round(algorithms):
        out = []
        for fe, rate, algorithm in zip(fronts, RATES, algorithms):
            out.append(fe.extract(yd, "cuda", generic=True).clone())
            out.append(resample_to_16k_device(xd[rate], rate).clone())
            _lib.check(lib.savad_logmel_set_algorithm(algorithm))
            out.append(log_mel(yd).clone())
        return out

    try:
        first = one_round((0, 1, 0))
        for fe in fronts:            # preparing what is resident builds nothing and moves nothing
            fe.prepare("cuda")
        for rate in RATES:
            resample_prepare(rate, "cuda")
        second = one_round((0, 1, 0))
    finally:
        _lib.check(lib.savad_logmel_set_algorithm(0))
    assert len(first) == len(second) == 9
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i

    want_mel = logmel.log_mel(y)
    for k, (fe, rate) in enumerate(zip(fronts, RATES)):
        got = first[3 * k].cpu().numpy()
        want = ref.features(y, fe.transform, fe.n_fft, fe.hop_ms, fe.window_ms, fe.n_mels, fe.n_mfcc, fe.deltas)
        assert got.shape == want.shape == (fe.frames(len(y)), fe.feature_size)
        F = fe.base_size
        _check(fe.transform, got[:, :F], want[:, :F])
        if fe.deltas:
            _check(fe.transform, got[:, F:2 * F], want[:, F:2 * F], 2.0)
            _check(fe.transform, got[:, 2 * F:], want[:, 2 * F:], 2.0)
        assert torch.equal(first[3 * k + 1].cpu(), torch.from_numpy(orc.resample(x[rate], rate))), rate
        d = np.abs(first[3 * k + 2].cpu().numpy() - want_mel)      # log-mel under algorithm 0, 1, 0: the bounds of test_gpu_parity.py
        assert d.max() < 5e-4 and (k == 1 or np.median(d) < 2e-6), (k, d.max(), np.median(d))
    assert torch.equal(first[2], first[8]) and np.abs((first[2] - first[5]).cpu().numpy()).max() < 5e-4
