"""Numeric regimes no other parity test enters, shared by tests/test_numeric_regimes_host.py (CPU) and
tests/test_gpu_numeric_regimes.py (GPU), and by tests/golden/make_golden_regimes.py.

Every other forward-pass test draws weights from seeded_state_dict (U(+-1/sqrt(fan_in)), LayerNorm weight 1 +- 0.1, bias +- 0.1)
and features from seeded_features.  There every LayerNorm row has a variance near or above 1, so the epsilon, the way the variance
is summed, the sign of a LayerNorm weight or the subtraction of the row maximum have no effect on any output the suite looks at
("Numeric regimes").  A regime here is a state and an input in which one of those pieces of the reference's arithmetic
carries a visible share of the result, together with the DEVIATIONS it must make visible: restatements of the reference with that
one piece changed.  The host test asserts that each deviation moves the float64 truth by at least VISIBLE x bound; the GPU test
holds the kernels to the truth at `bound`.

    truth   oracle/torch_port.py on double tensors (pinned to the reference's own float64 outputs, golden_regimes.npz, to 1e-9)
    floor   the larger error of two plain fp32 evaluations (torch_port on float tensors, the C oracle) against the truth
    bound   max(TIGHT, 3 x floor); 3 x floor must stay within TOL = 1e-4.  The named paths of `offset` alone
            (OFFSET_RESIDUAL_CHAIN_PATHS) are held to 3 x the floor of the kernels' accumulation order instead, capped at 4 x TOL

Shapes: the smallest at which each launch family of csrc/savad_schedule.h is entered --
    (4, 7, 80)    T <= 32: the single launch (fp32 packed_forward_kernel; fp32s / bf16 the latency variant; row_mode 1 - 3 the per-layer
                  launches with the packed attention)
    (3, 33, 80)   the first T > 32 shape: two query blocks, the second with one row, two waves of the group without a block;
                  fp32 per-layer launches (row_mode 1: 32-row N-split tiles, 2: 128-row M-split tiles, 3: fused attention + row chain),
                  fp32s row_mode 3 its fused launches, bf16 fused / separate / persistent attention (key-split tail)
    (2, 70, 80)   three key tiles, a ragged last one
    (2, 129, 80)  five query blocks: two groups per sequence, the second with one block
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

TOL = 1e-4      # the project's stated bar (tests/test_gpu_parity.py)
TIGHT = 3e-5    # what the fp32 paths are held to (tests/test_gpu_parity.py)
FLOOR_FACTOR = 3   # two independent fp32 evaluations of this model differ by up to 2.4 x in error: a third gets that much room
VISIBLE = 4        # a deviation counts when it moves the truth by at least VISIBLE x bound

STATE_SEED = 1234
GOLDEN = Path(__file__).resolve().parent / "golden" / "golden_regimes.npz"

S7, S33, S70, S129 = (4, 7, 80), (3, 33, 80), (2, 70, 80), (2, 129, 80)


# ---- states ---------------------------------------------------------------------------------------------------------------------
def base_state(d_model=128, seed=STATE_SEED):
    from voice_activity_detection_amd.seeded import seeded_state_dict

    return seeded_state_dict(seed, d_model=d_model)


def num_layers(state) -> int:
    return 1 + max(int(k.split(".")[2]) for k in state if k.startswith("encoder.layers."))


def layer_norm_keys(state):
    """(weight key, bias key) of every LayerNorm in call order: attention sublayer of layer l = 2 l, FFN sublayer = 2 l + 1, encoder = 2 L"""
    out = []
    for l in range(num_layers(state)):
        for sub in ("self_attention_sublayer", "feed_forward_sublayer"):
            out.append((f"encoder.layers.{l}.{sub}.layer_norm.weight", f"encoder.layers.{l}.{sub}.layer_norm.bias"))
    out.append(("encoder.layer_norm.weight", "encoder.layer_norm.bias"))
    return out


def _scaled(state, key, factor):
    state[key] = (state[key] * np.float32(factor)).astype(np.float32)


def quiet_state(state, i):
    """LayerNorm i sees rows whose variance is about that of the positional encoding (PE / sqrt(D): 0.5 / D, 4e-3 at D = 128): the
    input weight x 1e-3, the input bias x 1e-2, and the output projections (attention final projection, FFN-2) of every branch before
    LayerNorm i x 1e-2, weights and biases.  Everything after LayerNorm i keeps its size, so its output is not attenuated."""
    st = {k: v.copy() for k, v in state.items()}
    _scaled(st, "input_layer.0.weight", 1e-3)
    _scaled(st, "input_layer.0.bias", 1e-2)
    for branch in range(i):   # branch 2 l = attention of layer l (ends before LayerNorm 2 l + 1), 2 l + 1 = its FFN
        l, name = branch // 2, ("self_attention.final_projection" if branch % 2 == 0 else "feed_forward.feed_forward.3")
        _scaled(st, f"encoder.layers.{l}.{name}.weight", 1e-2)
        _scaled(st, f"encoder.layers.{l}.{name}.bias", 1e-2)
    return st


QUIET_LN6_CLASSIFIER = 2.0


def quiet_ln6_state(state):
    """quiet_state(state, 6) with the classifier weight x 2, for bf16's sake.  With the classifier as seeded the epsilons move
    oracle/bf16_model.py by 3.7 - 4.8 x KERNEL_GAP_BOUND, astride the 4 x a deviation needs to count; x 2 carries the model's
    self-difference past half that bound, the bf16 bound becomes twice the self-difference and the moves stand at 5.8 - 7.4 x it at
    every shape and epsilon (x 4 gives the same multiples: both scale with the classifier from there on)."""
    st = quiet_state(state, 6)
    _scaled(st, "classifier.weight", QUIET_LN6_CLASSIFIER)
    return st


OFFSET_C = 300.0


def offset_state(state):
    st = {k: v.copy() for k, v in state.items()}
    st["input_layer.0.bias"] = (st["input_layer.0.bias"] + np.float32(OFFSET_C)).astype(np.float32)
    return st


AFFINE_WEIGHTS = (0.0, -2.0, 8.0, 0.01, 1.0, -0.5, 3.0)


def affine_state(state):
    """LayerNorm weights drawn from AFFINE_WEIGHTS (zeros, signs, two and a half decades), biases U(-4, 4): the affine part is folded
    into the next projection (fold_ln_kernel; fp32s: on into the fused Wq~ and Wvo) -- a fold that loses a sign or a zero shows"""
    st = {k: v.copy() for k, v in state.items()}
    rng = np.random.default_rng(20_001)
    for wk, bk in layer_norm_keys(st):
        st[wk] = rng.choice(np.array(AFFINE_WEIGHTS, dtype=np.float32), size=st[wk].shape).astype(np.float32)
        st[bk] = rng.uniform(-4.0, 4.0, size=st[bk].shape).astype(np.float32)
    return st


def abs_layer_norm_weights(state):
    st = {k: v.copy() for k, v in state.items()}
    for wk, _ in layer_norm_keys(st):
        st[wk] = np.abs(st[wk])
    return st


SHARP_QK = 16.0
EXP_OVERFLOW = 88.8   # exp(x) overflows fp32 a little above this


def sharp_state(state):
    """query and key weights x 16: scores x 256 (the fp32 modes are otherwise run at gain 4 = x 16 on scores at the most)"""
    st = {k: v.copy() for k, v in state.items()}
    for l in range(num_layers(st)):
        _scaled(st, f"encoder.layers.{l}.self_attention.query_projection.weight", SHARP_QK)
        _scaled(st, f"encoder.layers.{l}.self_attention.key_projection.weight", SHARP_QK)
    return st


def same_state(state):
    return {k: v.copy() for k, v in state.items()}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
SILENCE = np.float32(math.log(1e-6))   # the log-mel of digital silence: log(0 + 1e-6)


def logmel_input(seed, shape):
    from voice_activity_detection_amd.seeded import seeded_features

    return seeded_features(seed, shape)


def power_input(seed, shape):
    """what the `mel` and `spectrogram` transforms feed the model: exp of the log-mel range, twelve decades, all positive"""
    return np.exp(logmel_input(seed, shape).astype(np.float64)).astype(np.float32)


def silence_input(seed, shape):
    return np.full(shape, SILENCE, dtype=np.float32)


# ---- deviations -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Deviation:
    """one piece of the reference's arithmetic changed: `kind` "eps" (LayerNorm `site` with epsilon `value`), "one_pass" (every
    LayerNorm takes its variance as fp32 E[x^2] - mean^2), "abs_ln_weights" (LayerNorm weights replaced by their absolute values)"""
    kind: str
    site: int = -1
    value: float = 0.0

    @property
    def name(self):
        return f"eps={self.value:g}@ln{self.site}" if self.kind == "eps" else self.kind


EPS_VALUES = (0.0, 1e-6, 2e-5)   # against the reference's 1e-5


def eps_deviations(site):
    return tuple(Deviation("eps", site, e) for e in EPS_VALUES)


@dataclass(frozen=True)
class Regime:
    name: str
    make_state: Callable          # seeded state -> the regime's state
    make_input: Callable          # (seed, shape) -> features [B, T, F] float32
    shapes: tuple
    deviations: tuple = ()
    d_model: int = 128
    tags: frozenset = field(default_factory=frozenset)
    residual_chain: frozenset = frozenset()   # the (T, run label) paths held to the residual-chain bound instead (chained_port below)

    def state(self):
        return self.make_state(base_state(self.d_model))

    def x(self, shape):
        return self.make_input(31_000 + 7 * shape[0] + shape[1], shape)

    def key(self, shape):
        return f"{self.name}_B{shape[0]}T{shape[1]}"


def fp32_runs(d_model, T):
    """(label, precision, row_mode, attention_splits) of every fp32-parity path a shape admits (csrc/savad_schedule.h)"""
    if d_model != 128:
        return [("generic", "fp32", 0, 0), ("generic two query tiles", "fp32", 0, 2)]
    runs = [("fp32", "fp32", 0, 0), ("fp32s", "fp32s", 0, 0), ("fp32s-kernels", "fp32s", 3, 0),
            ("fp32 rm1", "fp32", 1, 0), ("fp32 rm2", "fp32", 2, 0)]
    if T <= 32:   # the fp32s single launch: automatic is the latency variant at these sizes, 7 the wave-per-block one
        runs += [("fp32s rm7", "fp32s", 7, 0), ("fp32s rm8", "fp32s", 8, 0)]
    else:         # fp32: attention + row chain fused per layer; with two key splits, the combine of the row kernel
        runs += [("fp32 rm3", "fp32", 3, 1), ("fp32 two key splits", "fp32", 1, 2)]
    return runs


# `offset`: the (T, run label) paths that are outside max(TIGHT, 3 x floor) on the MI355X for the arithmetic reason given at
# chained_port below, and are held to 3 x the floor of that arithmetic instead: every path at (4, 7, 80) (4.8e-5 .. 8.1e-5 against
# 3.1e-5), and at the longer shapes the fp32s kernels, the M-split row kernel and the fused attention + row chain (7.3e-5 .. 1.06e-4
# against 5.1e-5 and 5.9e-5).  Every other path of `offset` -- the 32-row N-split tiles, which the automatic schedule of both fp32
# and fp32s takes at these sizes, with and without key splits: 4.96e-5 and 5.62e-5 -- is held to the plain bound.
OFFSET_RESIDUAL_CHAIN_PATHS = frozenset(
    [(7, label) for label, *_ in fp32_runs(128, 7)]
    + [(T, label) for T in (33, 70) for label in ("fp32s-kernels", "fp32 rm2", "fp32 rm3")])


def _quiet(i, d_model=128, name=None, shapes=(S7, S33, S70), make_state=None):
    return Regime(name or f"quiet_ln{i}", make_state or (lambda st, i=i: quiet_state(st, i)), logmel_input, shapes, eps_deviations(i),
                  d_model, frozenset({"quiet"}))


REGIMES = tuple(_quiet(i) for i in range(6)) + (
    _quiet(6, make_state=quiet_ln6_state),
    # the generic path (any d_model; savad_generic.h has one LayerNorm kernel with its own epsilon literal): a sublayer site and the
    # encoder's.  (PE / sqrt(64) has twice the variance, so the epsilon weighs half as much: of the sublayer sites, 0, 3 and 4 reach only
    # 3 - 5 x bound at (4, 7, 80) in float64, site 2 reaches 15 x and more.)
    _quiet(2, 64, "quiet_d64_ln2", (S7, S33)),
    _quiet(6, 64, "quiet_d64_ln6", (S7, S33)),
    Regime("offset", offset_state, logmel_input, (S7, S33, S70), (Deviation("one_pass"),), residual_chain=OFFSET_RESIDUAL_CHAIN_PATHS),
    Regime("affine", affine_state, logmel_input, (S7, S33, S70, S129), (Deviation("abs_ln_weights"),)),
    Regime("sharp", sharp_state, logmel_input, (S7, S33, S70, S129)),
    Regime("power", same_state, power_input, (S7, S33, S129)),
    Regime("silence", same_state, silence_input, (S7, S33, S129)),
)
BY_NAME = {r.name: r for r in REGIMES}
CASES = [(r.name, s) for r in REGIMES for s in r.shapes]


def case_id(case):
    return f"{case[0]}-{case[1][0]}x{case[1][1]}"


# ---- CPU evaluations ------------------------------------------------------------------------------------------------------------
class _PatchedF:
    """torch.nn.functional with layer_norm replaced, for oracle/torch_port.py alone"""

    def __init__(self, real, layer_norm):
        self._real, self.layer_norm = real, layer_norm

    def __getattr__(self, name):
        return getattr(self._real, name)


@contextmanager
def perturbed_layer_norm(fn):
    """Inside, the k-th F.layer_norm call of a torch_port.forward is fn(k, x, shape, weight, bias) -- or the real one where fn returns
    None.  The counter restarts with every forward (after 2 L + 1 calls it is back at the first).  Restores torch_port on exit."""
    from oracle import torch_port

    real = torch_port.F
    calls = [0]

    def layer_norm(x, shape, weight, bias, eps=1e-5):
        k = calls[0]
        calls[0] += 1
        out = fn(k, x, shape, weight, bias)
        return real.layer_norm(x, shape, weight, bias, eps) if out is None else out

    def counted_forward(state, x):
        calls[0] = 0
        return forward(state, x)

    forward = torch_port.forward
    torch_port.F = _PatchedF(real, layer_norm)
    try:
        yield counted_forward
    finally:
        torch_port.F = real


def _one_pass_layer_norm(x, weight, bias, eps=1e-5):
    """the statistics as a one-pass fp32 kernel would take them: mean and E[x^2] summed in fp32, variance = E[x^2] - mean^2 (clamped
    at 0, as a kernel that survives it would); the rest in the tensor's own precision"""
    import torch

    x32 = x.to(torch.float32)
    mean = x32.mean(-1, keepdim=True)
    var = ((x32 * x32).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (x - mean.to(x.dtype)) / torch.sqrt(var.to(x.dtype) + eps) * weight + bias


@contextmanager
def _one_thread():
    """these shapes are tiny: a thread pool only costs (60 s against 1 s for the whole table)"""
    import torch

    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(old)


def _tensors(state, x, dtype):
    import torch

    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}, torch.from_numpy(np.asarray(x)).to(dtype)


def port(state, x, dtype="float64", deviation: Deviation | None = None) -> np.ndarray:
    """oracle/torch_port.py on tensors of `dtype`, with one deviation applied"""
    import torch

    from oracle import torch_port

    dt = getattr(torch, dtype)
    if deviation is not None and deviation.kind == "abs_ln_weights":
        state, deviation = abs_layer_norm_weights(state), None
    st, xt = _tensors(state, x, dt)
    with _one_thread():
        return _port(torch, torch_port, st, xt, deviation)


def _port(torch, torch_port, st, xt, deviation):
    if deviation is None:
        return torch_port.forward(st, xt).numpy()
    if deviation.kind == "eps":
        def fn(k, h, shape, w, b):
            return torch.nn.functional.layer_norm(h, shape, w, b, deviation.value) if k == deviation.site else None
    elif deviation.kind == "one_pass":
        def fn(k, h, shape, w, b):
            return _one_pass_layer_norm(h, w, b)
    else:
        raise ValueError(deviation.kind)
    with perturbed_layer_norm(fn) as fwd:
        return fwd(st, xt).numpy()


def truth(state, x) -> np.ndarray:
    return port(state, x, "float64")


def floor(state, x, want=None):
    """the error of the same arithmetic in plain fp32: the larger of the stock-PyTorch port and the C oracle against the truth"""
    from oracle import oracle

    want = truth(state, x) if want is None else want
    e_port = float(np.abs(port(state, x, "float32") - want).max())
    e_c = float(np.abs(oracle.forward(state, x, threads=1) - want).max())
    return max(e_port, e_c)


def bound_of(floor_value):
    return max(TIGHT, FLOOR_FACTOR * floor_value)


# The kernels' GEMMs that end in a residual addition (input stage onto bias + PE, attention out-projection and FFN-2 onto the residual
# stream) START their accumulators at that addend (csrc/savad_kernels.h: "the out-projection accumulator starts at the residual
# stream + bias"; the fp32s and bf16 families do the same): every MFMA step rounds at the magnitude of the residual stream, where the
# reference rounds the finished branch once.  With a residual stream of ordinary size that is invisible (the floor of this arithmetic
# equals the plain one in every other regime); with `offset`, |h| ~ 300 against branches of size ~1, the random walk of K / 2
# roundings at ulp(300) = 3e-5 carries the error to 4 - 7 x the plain fp32 floor.  That is arithmetic, not a fault of one kernel, and
# it is the same in every family -- so the paths of `offset` that are outside the plain bound for it (OFFSET_RESIDUAL_CHAIN_PATHS, no
# other) are held to the floor of THIS arithmetic, restated on the CPU:
RESIDUAL_CHAIN_K = 2   # K per accumulation step: v_mfma_f32_32x32x2_f32 (the fp32s family: 16 per step, six products each)


def _chain(acc, a, W, step):
    """acc <- fp32(acc + a[..., k : k + step] W[:, k : k + step]^T), step by step: the products exact (float64), one fp32 rounding of
    the accumulator per step"""
    a64, W64 = a.double(), W.double()
    for k in range(0, a.shape[-1], step):
        acc = (acc.double() + a64[..., k:k + step] @ W64[:, k:k + step].T).float()
    return acc


def chained_port(state, x, step=RESIDUAL_CHAIN_K) -> np.ndarray:
    """oracle/torch_port.py on float tensors, but the three GEMMs that end in a residual addition accumulate onto their addend"""
    import torch

    from oracle import torch_port

    F = torch.nn.functional
    st, xt = _tensors(state, x, torch.float32)
    B, T, _ = xt.shape
    D = st["input_layer.0.weight"].shape[0]
    with _one_thread(), torch.no_grad():
        pe = torch_port.positional_encoding(T, D).unsqueeze(0) / math.sqrt(D)
        h = _chain((st["input_layer.0.bias"] + pe).expand(B, T, D).contiguous(), xt, st["input_layer.0.weight"], step)
        for l in range(num_layers(state)):
            p = f"encoder.layers.{l}."
            n = F.layer_norm(h, (D,), st[p + "self_attention_sublayer.layer_norm.weight"], st[p + "self_attention_sublayer.layer_norm.bias"])
            q, k, v = (F.linear(n, st[p + f"self_attention.{nm}_projection.weight"], st[p + f"self_attention.{nm}_projection.bias"])
                       for nm in ("query", "key", "value"))
            ctx = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(D), -1) @ v
            h = _chain(h + st[p + "self_attention.final_projection.bias"], ctx, st[p + "self_attention.final_projection.weight"], step)
            n = F.layer_norm(h, (D,), st[p + "feed_forward_sublayer.layer_norm.weight"], st[p + "feed_forward_sublayer.layer_norm.bias"])
            a = torch.relu(F.linear(n, st[p + "feed_forward.feed_forward.0.weight"], st[p + "feed_forward.feed_forward.0.bias"]))
            h = _chain(h + st[p + "feed_forward.feed_forward.3.bias"], a, st[p + "feed_forward.feed_forward.3.weight"], step)
        h = F.layer_norm(h, (D,), st["encoder.layer_norm.weight"], st["encoder.layer_norm.bias"])
        return F.log_softmax(F.linear(h, st["classifier.weight"], st["classifier.bias"]), dim=2).numpy()


def residual_chain_floor(state, x, want=None):
    want = truth(state, x) if want is None else want
    return float(np.abs(chained_port(state, x) - want).max())


# A path held to the residual-chain bound still has to expose the regime's deviation.  A kernel that carries the deviation and
# otherwise errs as the chained restatement does lands at least (move - chained floor) from the truth, which is outside the bound
# 3 x chained floor when the move is at least (1 + 1 / 3) x that bound: the host test asserts that multiple, the one such a path
# achieves, next to the 4 x the plain bound keeps.  The bound itself is capped at 4 x TOL: a residual stream that asks for more is
# a reason to change the accumulation order, not to widen the bound again.
CHAIN_VISIBLE = 1 + 1 / FLOOR_FACTOR
CHAIN_BOUND_CAP = 4 * TOL


def chain_bound_of(floor_value, chained_floor_value):
    return bound_of(max(floor_value, chained_floor_value))


def kernel_bounds(regime: "Regime", state, x, want=None):
    """(bound, chain bound) the fp32 paths are held to on the GPU: max(TIGHT, 3 x floor), and for the paths named in
    regime.residual_chain 3 x the floor of the kernels' own accumulation order where that is larger -- both computed on the CPU,
    never from a kernel's output.  The chain bound is None where the regime names no such path."""
    want = truth(state, x) if want is None else want
    fl = floor(state, x, want)
    return bound_of(fl), (chain_bound_of(fl, residual_chain_floor(state, x, want)) if regime.residual_chain else None)


def on_residual_chain(regime: "Regime", T, label):
    return (T, label) in regime.residual_chain


def moved(state, x, deviation, want=None):
    """how far the deviation moves the float64 truth (max |d log p|)"""
    want = truth(state, x) if want is None else want
    return float(np.abs(port(state, x, "float64", deviation) - want).max())


def layer0_score_spread(state, x) -> float:
    """float64: the largest over rows of (largest score - smallest score) in layer 0 -- beyond EXP_OVERFLOW an exponential taken without
    the row maximum overflows fp32"""
    import torch

    from oracle import torch_port

    st, xt = _tensors(state, x, torch.float64)
    D = st["input_layer.0.weight"].shape[0]
    p = "encoder.layers.0."
    F = torch.nn.functional
    h = F.linear(xt, st["input_layer.0.weight"], st["input_layer.0.bias"]) + torch_port.positional_encoding(xt.shape[1], D).unsqueeze(0).double() / math.sqrt(D)
    n = F.layer_norm(h, (D,), st[p + "self_attention_sublayer.layer_norm.weight"], st[p + "self_attention_sublayer.layer_norm.bias"])
    q = F.linear(n, st[p + "self_attention.query_projection.weight"], st[p + "self_attention.query_projection.bias"])
    k = F.linear(n, st[p + "self_attention.key_projection.weight"], st[p + "self_attention.key_projection.bias"])
    s = q @ k.transpose(1, 2) / math.sqrt(D)
    return float((s.amax(-1) - s.amin(-1)).max())


def residual_stream_peak(state, x) -> float:
    """float64: the largest |h| any LayerNorm reads -- the residual stream after the input stage, after every attention branch and after
    every layer, a superset of the points at which the bf16 kernels park it as fp16"""
    import torch

    peak = [0.0]

    def fn(k, h, shape, w, b):
        peak[0] = max(peak[0], float(h.abs().max()))
        return None

    st, xt = _tensors(state, x, torch.float64)
    with _one_thread(), perturbed_layer_norm(fn) as fwd:
        fwd(st, xt)
    return peak[0]


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- bf16: oracle/bf16_model.py is the restatement ------------------------------------------------------------------------------
@contextmanager
def bf16_layer_norm_eps(value):
    """oracle/bf16_model.py with its LN_EPS patched (every LayerNorm of the model: in quiet_ln{i} only site i weighs)"""
    from oracle import bf16_model

    old = bf16_model.LN_EPS
    bf16_model.LN_EPS = value
    try:
        yield bf16_model
    finally:
        bf16_model.LN_EPS = old


def bf16_model_out(state, x, key_split=False, dtype="float64", info=None):
    from oracle import bf16_model

    return bf16_model.forward(state, x, key_split=key_split, dtype=dtype, info=info, threads=1)


def bf16_self_difference(state, x, key_split=False):
    """the bf16 model evaluated on float tensors against itself on double tensors: the rounding-flip floor of that arithmetic here"""
    return float(np.abs(bf16_model_out(state, x, key_split, "float32") - bf16_model_out(state, x, key_split)).max())


def pw_splits(T):
    """bf16 row_mode 5 computes a tail group of one or two query blocks as a key-split item (tests/test_gpu_bf16_model.py)"""
    return T > 32 and ((T + 31) // 32) % 8 in (1, 2)


_BF16_SD = {}


def bf16_regime_self_difference(name):
    """the largest self-difference over the regime's shapes (key-split form included where row_mode 5 takes it): one figure per regime,
    so that a case's bound does not hang on which rounding flips one shape happens to meet"""
    if name not in _BF16_SD:
        r = BY_NAME[name]
        st = r.state()
        _BF16_SD[name] = max(bf16_self_difference(st, r.x(s), ks) for s in r.shapes for ks in ((False, True) if pw_splits(s[1]) else (False,)))
    return _BF16_SD[name]


def bf16_bound_of(self_difference):
    """KERNEL_GAP_BOUND; where the model's self-difference is itself above half of it, twice the self-difference (the way
    tests/test_gpu_bf16_model.py bounds the sharp weight sets: from the model, never from the kernel's gap)"""
    from oracle.bf16_model import KERNEL_GAP_BOUND

    return KERNEL_GAP_BOUND if self_difference <= KERNEL_GAP_BOUND / 2 else 2.0 * self_difference


def bf16_moved(state, x, eps):
    with bf16_layer_norm_eps(eps):
        y = bf16_model_out(state, x)
    return float(np.abs(y - bf16_model_out(state, x)).max())


# (regime, shape) -> the epsilons whose deviation moves the bf16 model by at least VISIBLE x its bound there (asserted by the host test;
# the GPU test holds these cases to the model).  bf16's own rounding covers the epsilon of LayerNorm 0 - 5: in those regimes the model differs from
# itself by 1.8e-3 .. 3.7e-3 (float against double evaluation), and moves by 3 - 9e-3 whatever is perturbed.
BF16_VISIBLE = {
    ("quiet_ln6", S7): (0.0, 1e-6, 2e-5),
    ("quiet_ln6", S33): (0.0, 1e-6, 2e-5),
    ("quiet_ln6", S70): (0.0, 1e-6, 2e-5),
}
BF16_HELD = ("silence", "affine")          # held to the model at bf16_bound_of(self-difference) besides the cases of BF16_VISIBLE
BF16_FINITE_ONLY = ("offset", "sharp", "power")
