"""The forwards on the routing probes of tests/routing_probes.py: inputs under which every query of every sequence attends to ONE key
of its own choosing, so that a kernel which drops, doubles or misplaces a key, a key tile or a row of a query block moves the rows
that target it by 1e-2 and more -- where the dense random inputs of every other parity test spread such a fault over all keys of a
row (at T = 800 below the tolerance; tests/test_routing_probes_host.py asserts both statements on the CPU).

One id per (regime, length, path).  Every row of every sequence is held to the reference:
    fp32, fp32s, d_model 64   against the float64 truth (oracle/torch_port.py on double tensors) at bound = max(TIGHT, 3 x fp32 floor)
    bf16                      against oracle/bf16_model.py at its bound (KERNEL_GAP_BOUND, or twice the model's self-difference), in
                              the key-split form where row_mode 5 takes the key-split tail item; from T = 800 on, on the sequences of
                              rp.bf16_sequences (the model takes seconds per sequence there); no residual saturation
A failure prints the (sequence, query, target) of the worst rows: the triple names the (query block, key tile) at fault.

Measured on an MI355X, max |d log p| over the rows, worst over the lengths and paths of a family (bound 3.0e-5; bf16 1.5e-3 .. 2.5e-3):
    sharp  fp32 2.3e-6, fp32s 1.8e-6, d_model 64 2.9e-7, bf16 3.0e-4 .. 1.4e-3 from the model
    soft   fp32 2.4e-6, fp32s 2.3e-6, d_model 64 3.8e-7, bf16 1.8e-4 .. 1.4e-3 from the model
DESIGN.md section 4u has the table per (regime, length, path family), the construction and what stays uncovered."""
from functools import lru_cache

import numpy as np
import pytest

from tests import routing_probes as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (torch.cuda.is_available() is False)")
    return torch


_MODELS = {}


def gpu_model(torch, regime, T, d_model=128):
    """one model per state: `sharp` shares one over the lengths, `soft` has a c of its own per length"""
    from voice_activity_detection_amd import SelfAttentiveVAD

    key = (rp.regime_c(regime, T, d_model), d_model)
    if key not in _MODELS:
        st = rp.routing_state(*key)
        m = SelfAttentiveVAD(rp.FEATURES, rp.num_layers(st), d_model, 0.5)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        _MODELS[key] = m.to("cuda").eval()
    return _MODELS[key]


@lru_cache(maxsize=None)
def device_input(regime, T, d_model=128):
    import torch

    return torch.from_numpy(np.array(rp.case(regime, T, d_model)[1])).to("cuda")


def run(torch, m, x, precision, row_mode=0, splits=0, batch_invariant=False):
    m.precision, m.row_mode, m.attention_splits, m.batch_invariant = precision, row_mode, splits, batch_invariant
    try:
        with torch.no_grad():
            y = m(features=x)
        torch.cuda.synchronize()
    finally:
        m.precision, m.row_mode, m.attention_splits, m.batch_invariant = "fp32", 0, 0, False
    return y.cpu().numpy()


def fp32_paths(T, d_model=128):
    """(label, precision, row_mode, attention_splits) of every fp32-parity path csrc/savad_schedule.h takes at a length"""
    if d_model != 128:   # csrc/savad_generic.h: attention_splits = n > 1 is n query tiles per sequence
        return [("generic", "fp32", 0, 0)] + [(f"generic {n} query tiles", "fp32", 0, n) for n in ((2, 3) if T > 64 else (2,))]
    paths = [("fp32", "fp32", 0, 0), ("fp32 rm1", "fp32", 1, 0), ("fp32 rm2", "fp32", 2, 0),
             ("fp32s", "fp32s", 0, 0), ("fp32s rm1", "fp32s", 1, 0), ("fp32s rm3", "fp32s", 3, 0)]
    if T <= rp.BLOCK:   # the single launches: fp32 packed_forward_kernel; fp32s the wave-per-block and the latency variant
        paths += [("fp32 rm4", "fp32", 4, 0), ("fp32s rm7", "fp32s", 7, 0), ("fp32s rm8", "fp32s", 8, 0)]
    else:               # fused attention + row chain; key splits and their combine (choose_splits caps the count at the key tiles)
        paths += [("fp32 rm3", "fp32", 3, 1), ("fp32 2 key splits", "fp32", 1, 2)]
        if rp.blocks_of(T) >= 3:
            paths += [("fp32 5 key splits", "fp32", 1, 5)]
    return paths


FP32_CASES = [(regime, T, 128, path) for regime in rp.REGIMES for T in rp.SHAPES for path in fp32_paths(T)] \
    + [(regime, T, 64, path) for regime in rp.REGIMES for T in rp.GENERIC_SHAPES for path in fp32_paths(T, 64)]


@pytest.mark.parametrize("regime,T,d_model,path", FP32_CASES,
                         ids=[f"{rp.case_id(r, T, d)}-{p[0].replace(' ', '_')}" for r, T, d, p in FP32_CASES])
def test_fp32_paths_hold_the_truth_row_by_row(torch_cuda, regime, T, d_model, path):
    label, precision, row_mode, splits = path
    want, _, bound = rp.reference(regime, T, d_model)
    tg = rp.target_sets(T)
    y = run(torch_cuda, gpu_model(torch_cuda, regime, T, d_model), device_input(regime, T, d_model), precision, row_mode, splits)
    assert y.shape == want.shape and y.dtype == np.float32
    err = float(rp.row_moves(y, want).max()) if np.isfinite(y).all() else float("inf")
    print(f"{rp.case_id(regime, T, d_model)} {label}: {err:.2e}, bound {bound:.2e}")
    if not err < bound:
        print("worst rows:\n  " + "\n  ".join(rp.worst_rows(y, want, tg)))
    assert err < bound, (regime, T, d_model, label, err, bound)


# ---- bf16 -----------------------------------------------------------------------------------------------------------------------
# automatic, the per-layer launches, the fused launches and the persistent attention (T <= 32: 0 the single launch, 5 its 8-wave
# variant, 1 and 3 the per-layer launches); batch_invariant runs the persistent kernel without its key-split tail items
BF16_PATHS = [(0, False), (1, False), (3, False), (5, False), (0, True), (5, True)]
BF16_CASES = [(regime, T, path) for regime in rp.REGIMES for T in rp.SHAPES for path in BF16_PATHS]


@pytest.mark.parametrize("regime,T,path", BF16_CASES,
                         ids=[f"{rp.case_id(r, T)}-bf16_rm{p[0]}{'_batch_invariant' if p[1] else ''}" for r, T, p in BF16_CASES])
def test_bf16_paths_hold_the_model_row_by_row(torch_cuda, regime, T, path):
    row_mode, invariant = path
    assert (regime, T) in rp.BF16_VISIBLE   # every case is held; which deviations the bound exposes is the host test's table
    want, sd, bound = rp.bf16_reference(regime, T)
    seqs = rp.bf16_sequences(T)
    tg = rp.target_sets(T)[seqs]
    m = gpu_model(torch_cuda, regime, T)
    m.residual_saturations()
    y = run(torch_cuda, m, device_input(regime, T), "bf16", row_mode, 0, invariant)
    assert y.shape == (rp.target_sets(T).shape[0], T, 2) and np.isfinite(y).all(), (regime, T, path)
    assert m.residual_saturations() == 0, (regime, T, path)
    key_split = row_mode == 5 and not invariant and rp.pw_splits(T)
    gap = float(rp.row_moves(y[seqs], want[key_split]).max())
    print(f"{rp.case_id(regime, T)} bf16 row_mode {row_mode}{' batch-invariant' if invariant else ''}: kernel - model {gap:.2e}, "
          f"bound {bound:.2e} (model self-difference {sd:.2e}, {len(seqs)} sequences)")
    if not gap < bound:
        print("worst rows (sequence = index into rp.bf16_sequences):\n  " + "\n  ".join(rp.worst_rows(y[seqs], want[key_split], tg)))
    assert gap < bound, (regime, T, path, gap, bound)


# ---- equal bits -----------------------------------------------------------------------------------------------------------------
# the schedules include/savad.h states independent of the batch a sequence is evaluated in: (precision, row_mode, attention_splits,
# batch_invariant).  T <= 32: the fp32 single launch, the fp32s latency variant, the bf16 single launch in its 8-wave and latency
# variants; longer: fp32 with the key-split count pinned, the fp32s kernels, bf16 with batch_invariant
def pinned_variants(T):
    if T <= rp.BLOCK:
        return [("fp32", 4, 0, False), ("fp32s", 8, 0, False), ("bf16", 5, 0, False), ("bf16", 8, 0, False)]
    return [("fp32", 1, 1, False), ("fp32s", 3, 0, False), ("bf16", 0, 0, True), ("bf16", 5, 0, True)]


@pytest.mark.parametrize("T", [7, 33, 264])
def test_a_sequence_has_the_same_bits_alone_and_among_other_neighbours(torch_cuda, T):
    """a packed tile of four sequences, a two-block sequence with idle waves, the key-split tail item: the neighbours of a sequence in
    its tile, group or launch leave no trace in it.  Two statements per pinned variant: (1) with every OTHER sequence of the batch
    replaced, a sequence keeps its bits, at every index; (2) run alone it has the bits it has inside its batch -- at T <= 32 for
    fp32 and fp32s only when it sits in slot 0 of its packed tile: the masked columns of the other slots are exact zeros, but they
    shift the sequence's keys within the MFMA's summation groups, and its bits move with the slot by one to five ulp (measured
    2.4e-7 .. 6.0e-7 at slots 1 - 3, in row_mode 1, 3, 4, 7 and 8 alike; bf16 keeps its bits at every slot)."""
    torch = torch_cuda
    m = gpu_model(torch, "sharp", T)
    x = device_input("sharp", T)
    B = x.shape[0]
    per = max(1, rp.BLOCK // T)
    others = x.roll(1, 0)
    for variant in pinned_variants(T):
        whole = run(torch, m, x, *variant)
        assert np.isfinite(whole).all(), (T, variant)
        for b in sorted({0, 1, per, B // 2, B - 1}):
            mixed = others.clone()
            mixed[b] = x[b]
            got = run(torch, m, mixed, *variant)
            assert np.array_equal(got[b], whole[b]), (T, variant, b, "other neighbours", float(np.abs(got[b] - whole[b]).max()))
            assert not np.array_equal(got[(b + 1) % B], whole[(b + 1) % B])   # the neighbours did change
            if variant[0] == "bf16" or b % per == 0:
                alone = run(torch, m, x[b:b + 1].contiguous(), *variant)
                assert np.array_equal(alone[0], whole[b]), (T, variant, b, "alone", float(np.abs(alone[0] - whole[b]).max()))


@pytest.mark.parametrize("T", [33, 264])
def test_two_runs_give_equal_bits_and_a_poisoned_workspace_changes_nothing(torch_cuda, T):
    torch = torch_cuda
    m = gpu_model(torch, "sharp", T)
    x = device_input("sharp", T)
    try:
        for precision, row_mode, splits in (("fp32", 0, 0), ("fp32", 3, 1), ("fp32", 1, 2), ("fp32s", 0, 0), ("fp32s", 3, 0),
                                            ("bf16", 0, 0), ("bf16", 1, 0), ("bf16", 5, 0)):
            m.precision, m.row_mode, m.attention_splits = precision, row_mode, splits
            with torch.no_grad():
                y0 = m(features=x).clone()
                y1 = m(features=x).clone()
                m._workspace.fill_(255)
                y2 = m(features=x)
            assert torch.isfinite(y0).all() and torch.equal(y0, y1) and torch.equal(y0, y2), (T, precision, row_mode, splits)
    finally:
        m.precision, m.row_mode, m.attention_splits = "fp32", 0, 0
