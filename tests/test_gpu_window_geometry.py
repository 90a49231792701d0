"""The predict paths at every window geometry a checkpoint can name (tests/window_geometry_cases.py: W = 1 .. 63, symmetric and
asymmetric offsets, every packing of floor(32 / W) windows into a 32-row block, the hand-over at W = 33 from the windowed launches to
gather + a T > 32 forward), against the reference's own predictor (tests/golden/golden_geometry.npz) at each geometry's golden length
and against the CPU oracle -- pinned to those goldens by tests/test_window_geometry_host.py -- at the others.  The host tests also show
that an address one frame off moves a probability by more than 0.1, 3 000 times the bound used here.

Worst |dp| per geometry and precision over every length and pinned variant (MI355X; test_one_call_against_the_reference prints them;
bounds: fp32 / fp32s 3e-5, bf16 6e-3 against the oracle and KERNEL_GAP_BOUND = 1.5e-3 against the bf16 arithmetic model):
    half / jump   W    fp32      fp32s     bf16 vs oracle   bf16 vs its model
       0 / 1      1    3.0e-07   4.8e-07   1.45e-03         6.2e-05
       1 / 1      3    3.9e-07   4.8e-07   1.13e-03         1.1e-04
       3 / 5      3    3.6e-07   4.8e-07   1.30e-03         9.8e-05
       6 / 4      5    4.2e-07   4.8e-07   1.38e-03         8.4e-05
      20 / 9      7    3.9e-07   4.5e-07   1.38e-03         1.6e-04
       5 / 1     11    4.8e-07   6.0e-07   1.08e-03         1.4e-04
       8 / 1     17    4.2e-07   5.4e-07   1.50e-03         1.8e-04
      15 / 1     31    4.2e-07   6.0e-07   1.58e-03         8.5e-05
      16 / 1     33    3.3e-07   5.4e-07   1.42e-03         1.4e-04
      31 / 1     63    4.2e-07   5.4e-07   1.71e-03         1.3e-04
The batch of clips: fp32 / fp32s at most 4.2e-07, bf16 at most 1.6e-03.  No bf16 case came near KERNEL_GAP_BOUND, so the plain forward
was not measured separately.
"""
import functools

import numpy as np
import pytest

from tests import window_geometry_cases as cases
from tests.buffer_arena import same_bits
from tests.test_gpu_schedule_workspace import Knobs
from tests.window_geometry_cases import GEOMETRIES, LONG_CASES, geometry_id

pytestmark = pytest.mark.gpu

TIGHT = 3e-5              # fp32 / fp32s probabilities against the reference
BF16_PROBS = 6e-3         # bf16 probabilities against the fp32 oracle (tests/test_gpu_predict_batch.py, tests/test_gpu_live.py)
FP32S_VARIANTS = 2e-6     # the two fp32s single-launch variants: one fp32 sum in another order (test_one_call_predictor_matches_the_three_entry_points)
# include/savad.h (savad_set_row_mode): the automatic schedule and every variant that can be pinned for windows of at most 32 frames
VARIANTS = {"fp32": (0, 4, 1), "fp32s": (0, 8, 7, 1), "bf16": (0, 8, 5, 1)}
LIVE_PINNED = [("fp32", 4), ("fp32s", 8), ("fp32s", 5), ("bf16", 8), ("bf16", 5)]   # tests/test_gpu_live.py: deterministic, batch-independent


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda, state1234):
    from voice_activity_detection_amd import SelfAttentiveVAD

    m = SelfAttentiveVAD(80, 3, 128, 0.5)
    m.load_state_dict({k: torch_cuda.from_numpy(v) for k, v in state1234.items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def goldens():
    from pathlib import Path

    with np.load(Path(__file__).resolve().parent / "golden" / "golden_geometry.npz") as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _state():
    from voice_activity_detection_amd.seeded import seeded_state_dict

    return seeded_state_dict(1234)


@functools.lru_cache(maxsize=None)
def oracle_of(half, jump, N, seed=None):
    """(probs [N, W], mean [N]) of the float64-accumulating CPU oracle, computed once per input and never written"""
    from oracle import oracle

    feat = cases.features(half, jump, N) if seed is None else clip_features(seed, N)
    probs, mean = oracle.predict_probabilities(_state(), feat, half, jump, acc64=True)
    probs.setflags(write=False)
    mean.setflags(write=False)
    return probs, mean


@functools.lru_cache(maxsize=None)
def bf16_model_of(half, jump, N, key_split):
    """probs [N, W] float64: the boost of the bf16 arithmetic model (oracle/bf16_model.py) over the numpy-gathered windows"""
    from oracle import bf16_model

    windows, positions = cases.gather(cases.features(half, jump, N), half, jump)
    if len(windows) == 0:
        return np.full((N, windows.shape[1]), 0.5)
    logp = bf16_model.forward(_state(), windows, key_split=key_split)
    z = np.zeros((N, windows.shape[1], 2))
    for item in range(len(windows)):
        for w in range(windows.shape[1]):
            z[positions[item, w], w] = logp[item, w]
    return 1.0 / (1.0 + np.exp(z[..., 0] - z[..., 1]))


@functools.lru_cache(maxsize=None)
def clip_features(seed, N):
    from voice_activity_detection_amd.seeded import seeded_features

    feat = seeded_features(seed, (N, cases.FEATURE_SIZE))
    feat.setflags(write=False)
    return feat


def feats(half, jump, N):
    """a writable copy of the shared input (torch warns about tensors over read-only arrays)"""
    return cases.features(half, jump, N).copy()


def predictor(model, half, jump, **kw):
    from voice_activity_detection_amd import ContextResolution, VADFromScratchPredictor

    return VADFromScratchPredictor(model, "cuda", ContextResolution(half, jump), **kw)


def unique_lengths(half, jump):
    return list(dict.fromkeys(cases.lengths(half, jump)))


# ---- 1. one call against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_one_call_against_the_reference(torch_cuda, model, goldens, geometry, precision):
    from oracle.bf16_model import KERNEL_GAP_BOUND

    half, jump = geometry
    W = len(cases.offsets(half, jump))
    golden_N = cases.golden_length(half, jump)
    pred = predictor(model, half, jump)
    assert pred.context_window_frames == W
    worst = worst_mean = worst_model = 0.0
    for N in unique_lengths(half, jump):
        feat = feats(half, jump, N)
        ref, ref_mean = oracle_of(half, jump, N)
        if N == golden_N:
            ref = goldens[cases.golden_key(half, jump)]      # the reference's own result
            ref_mean = ref.mean(axis=1)
        assert ref.shape == (N, W)
        for row_mode in VARIANTS[precision]:
            with Knobs(model, precision, row_mode):
                probs = pred.predict_probabilities(feat)
                boosted = pred.predict_boosted(feat)
            what = (half, jump, N, precision, row_mode)
            assert probs.shape == (N, W) and probs.dtype == np.float32 and boosted.shape == (N,), what
            assert np.array_equal(probs == 0.5, ref == 0.5), what
            err = float(np.abs(probs.astype(np.float64) - ref).max())
            err_mean = float(np.abs(boosted.astype(np.float64) - ref_mean).max())
            worst, worst_mean = max(worst, err), max(worst_mean, err_mean)
            if precision == "bf16":
                # (the persistent attention kernel that 5 pins for T > 32 sums a one- or two-block sequence's keys as four partial softmaxes)
                want = bf16_model_of(half, jump, N, key_split=bool(row_mode == 5 and W > 32))
                gap = float(np.abs(probs - want).max())
                worst_model = max(worst_model, gap)
                print(f"  {half} / {jump} N = {N} bf16 m{row_mode}: vs oracle {err:.2e}, vs bf16 model {gap:.2e}")
                assert err <= BF16_PROBS and err_mean <= BF16_PROBS, what + (err, err_mean)
                assert gap <= KERNEL_GAP_BOUND, what + (gap,)
            else:
                assert err <= TIGHT and err_mean <= TIGHT, what + (err, err_mean)
    print(f"geometry {half:>2} / {jump} W = {W:>2} {precision:>5}: max |dp| = {worst:.2e}, max |dmean| = {worst_mean:.2e}" +
          (f", max |dp| vs the bf16 model = {worst_model:.2e}" if precision == "bf16" else ""))


# ---- 2. one call against the three entry points ----------------------------------------------------------------------------------------

ENTRY_CASES = [(h, j, None, 16384) for h, j in GEOMETRIES] + LONG_CASES


@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
@pytest.mark.parametrize("half,jump,long_N,chunk", ENTRY_CASES, ids=lambda v: str(v))
def test_one_call_against_the_three_entry_points(torch_cuda, model, half, jump, long_N, chunk, precision):
    """savad_predict_probabilities (windows read in place where a single launch applies) against savad_gather_windows + savad_forward
    + savad_boost with the relations of tests/test_gpu_parity.py::test_one_call_predictor_matches_the_three_entry_points: fp32 and
    bf16 the same bits; fp32s, whose one call picks its variant by the clip's window count and the stepwise forwards by the chunk's,
    to fp32 rounding with the same placeholders.  From W = 33 on both sides gather and run a T > 32 forward."""
    torch = torch_cuda
    W = len(cases.offsets(half, jump))
    pred = predictor(model, half, jump, chunk_size=chunk)
    for N in ([long_N] if long_N else unique_lengths(half, jump)):
        feat = torch.from_numpy(feats(half, jump, N)).cuda()
        with Knobs(model, precision, 0):
            p1, m1 = pred.predict_probabilities_device(feat)
            p0, m0 = pred.predict_probabilities_device_stepwise(feat)
            torch.cuda.synchronize()
        what = (half, jump, N, precision)
        assert p1.shape == p0.shape == (N, W) and m1.shape == m0.shape == (N,), what
        if precision == "fp32s":
            assert torch.equal(p1 == 0.5, p0 == 0.5), what
            assert float((p1 - p0).abs().max()) <= FP32S_VARIANTS and float((m1 - m0).abs().max()) <= FP32S_VARIANTS, what
        else:
            assert same_bits(p1, p0) and same_bits(m1, m0), what
        if long_N:
            n_items = N - 2 * half
            assert n_items > 1024 * cases.per_block(W) and n_items % chunk != 0   # past fp32's windowed launch, a ragged last chunk
            assert bool((p1[:half] == 0.5).sum() > 0) and bool(torch.isfinite(p1).all())


# ---- 3. idle rows and rows past the last window never reach a result ------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
@pytest.mark.parametrize("geometry", [(1, 1), (5, 1), (15, 1), (16, 1)], ids=geometry_id)
def test_poisoned_workspace(torch_cuda, model, geometry, precision):
    torch = torch_cuda
    half, jump = geometry
    W = len(cases.offsets(half, jump))
    pred = predictor(model, half, jump)
    for N in (2 * half + cases.per_block(W) + 1, cases.golden_length(half, jump)):
        feat = torch.from_numpy(feats(half, jump, N)).cuda()
        for row_mode in VARIANTS[precision]:
            with Knobs(model, precision, row_mode):
                p1, m1 = pred.predict_probabilities_device(feat)
                torch.cuda.synchronize()
                assert model._workspace is not None and model._workspace.numel() > 0
                model._workspace.fill_(255)            # every float a NaN, every index -1
                p2, m2 = pred.predict_probabilities_device(feat)
                torch.cuda.synchronize()
            what = (half, jump, N, precision, row_mode)
            assert bool(torch.isfinite(p2).all()) and bool(torch.isfinite(m2).all()), what
            assert same_bits(p1, p2) and same_bits(m1, m2), what


# ---- 4. many clips in one call ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp32s", "bf16"])
@pytest.mark.parametrize("geometry", [(1, 1), (6, 4), (8, 1), (16, 1)], ids=geometry_id)
def test_batch_of_clips(torch_cuda, model, geometry, precision):
    """six clips, each with features of its own: every clip's rows are the oracle's of that clip alone (a neighbour's frame in a
    window would move a probability by more than 0.1), its placeholders included"""
    half, jump = geometry
    W = len(cases.offsets(half, jump))
    per, golden_N = cases.per_block(W), cases.golden_length(half, jump)
    clip_lengths = [golden_N, 0, 2 * half, 2 * half + per + 2, 2 * half + 1, 2 * half + 2 * per + 1]
    seeds = [20000 + 1000 * c + 100 * half + jump for c in range(len(clip_lengths))]
    clips = [clip_features(s, n).copy() for s, n in zip(seeds, clip_lengths)]
    pred = predictor(model, half, jump)
    with Knobs(model, precision, 0):
        results = [(p.cpu().numpy(), m.cpu().numpy()) for p, m in pred.predict_probabilities_many(clips)]
    assert len(results) == len(clips)
    bound = BF16_PROBS if precision == "bf16" else TIGHT
    worst = 0.0
    for c, ((probs, mean), n, seed) in enumerate(zip(results, clip_lengths, seeds)):
        assert probs.shape == (n, W) and mean.shape == (n,), (half, jump, c)
        if n == 0:
            continue
        ref, ref_mean = oracle_of(half, jump, n, seed)
        assert np.array_equal(probs == 0.5, ref == 0.5), (half, jump, c)
        err = max(float(np.abs(probs - ref).max()), float(np.abs(mean - ref_mean).max()))
        worst = max(worst, err)
        assert err <= bound, (half, jump, precision, c, n, err)
    print(f"batch at {half} / {jump} ({precision}): max |dp| = {worst:.2e}")


# ---- 5. the host feed: chunk starts aligned to 32 // W --------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,row_mode", LIVE_PINNED)
@pytest.mark.parametrize("geometry", [(5, 1), (8, 1)], ids=geometry_id)
def test_host_feed_has_the_device_bits(torch_cuda, model, geometry, precision, row_mode):
    from voice_activity_detection_amd import VADFromScratchPredictor

    half, jump = geometry
    W = len(cases.offsets(half, jump))
    audio = (np.random.default_rng(900 + half).standard_normal(48000) * 0.1).astype(np.float32)    # 3 s: 301 frames
    pred = predictor(model, half, jump)
    plan = VADFromScratchPredictor.host_chunk_plan(301, half, W, 64)
    assert len(plan) >= 4 and all(g0 % cases.per_block(W) == 0 for _, _, g0, _ in plan) and sum(g0 > 0 for _, _, g0, _ in plan) >= 3
    with Knobs(model, precision, row_mode):
        want, want_mean = pred.predict_audio_device(audio)
        probs, mean = pred.predict_audio_host(audio, frames_per_chunk=64)
        torch_cuda.cuda.synchronize()
    assert probs.shape == want.shape == (301, W)
    assert same_bits(probs, want) and same_bits(mean, want_mean)


# ---- 6. live sessions ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def live_signals():
    from tests.test_gpu_live import TOTALS, make_signals

    signals = make_signals()
    picked = [signals[TOTALS.index(6720)], signals[TOTALS.index(16001)]]
    assert [len(s) for s in picked] == [6720, 16001]
    return picked


@pytest.mark.parametrize("precision,row_mode", LIVE_PINNED)
@pytest.mark.parametrize("geometry", [(0, 1), (6, 4), (8, 1)], ids=geometry_id)
def test_live_rows_are_the_offline_rows(torch_cuda, model, live_signals, geometry, precision, row_mode):
    from tests.test_gpu_live import run_live
    from voice_activity_detection_amd import ContextResolution

    half, jump = geometry
    W = len(cases.offsets(half, jump))
    context = ContextResolution(half, jump)
    with Knobs(model, precision, row_mode):
        runs = {name: run_live(torch_cuda, model, live_signals, name, context=context) for name in "ac"}
        pred = predictor(model, half, jump)
        offline = [tuple(t.cpu().numpy() for t in pred.predict_audio_device(s)) for s in live_signals]
    for name in "ac":
        for rec, s in enumerate(live_signals):
            probs, mean = runs[name][rec]
            assert probs.shape == (1 + len(s) // 160, W) and mean.shape == (1 + len(s) // 160,), (name, rec)
            assert same_bits(probs, offline[rec][0]) and same_bits(mean, offline[rec][1]), (half, jump, name, rec)
    if half == 0:
        assert not (offline[0][0] == 0.5).any()      # every frame is a window: no placeholders


# ---- 7. a checkpoint that names another geometry --------------------------------------------------------------------------------------

def test_checkpoint_geometry(torch_cuda, model, state1234, tmp_path):
    import copy

    from tests.conftest import REFERENCE_CONFIG, write_reference_checkpoint
    from voice_activity_detection_amd import VADFromScratchPredictor

    cfg = copy.deepcopy(REFERENCE_CONFIG)
    cfg["context_resolution"].update(context_window_half_frames=6, context_window_jump_frames=4)
    loaded = VADFromScratchPredictor.from_checkpoint(write_reference_checkpoint(tmp_path / "g64.checkpoint", state1234, cfg), "cuda")
    assert (loaded.context_window_half_frames, loaded.context_window_jump_frames, loaded.context_window_frames) == (6, 4, 5)
    direct = predictor(model, 6, 4)
    for N in unique_lengths(6, 4):
        feat = feats(6, 4, N)
        got, want = loaded.predict_probabilities(feat), direct.predict_probabilities(feat)
        assert got.shape == (N, 5) and same_bits(got, want), N


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(torch_cuda, model):
    from voice_activity_detection_amd import ContextResolution, LiveVAD
    from voice_activity_detection_amd._lib import SavadError

    for half, jump in cases.DISAGREEING:
        W, formula = len(cases.offsets(half, jump)), cases.reference_formula(half, jump)
        with pytest.raises(ValueError, match=f"formula gives {formula} frames, its window offsets are {W}"):
            LiveVAD(model, "cuda", 2, 1600, ContextResolution(half, jump))
        with pytest.raises(ValueError, match=f"formula gives {formula} frames"):
            predictor(model, half, jump)
    wide = predictor(model, 32, 1)        # W = 65: the formula agrees, the library refuses
    feat = torch_cuda.from_numpy(feats(32, 1, 80)).cuda()
    for call in (wide.predict_probabilities_device, wide.predict_probabilities_device_stepwise, lambda f: wide.predict_probabilities_many([f])):
        with pytest.raises(SavadError, match="64 frames"):
            call(feat)
    with pytest.raises(SavadError, match="64 frames"):
        LiveVAD(model, "cuda", 2, 1600, ContextResolution(32, 1))
