"""CPU restatement of the bf16 forward's ARITHMETIC (precision "bf16").  TEST INFRASTRUCTURE ONLY.

``oracle.forward`` is the fp32 model; the bf16 kernels differ from it by their own rounding (bf16 operands, an fp16-parked
residual stream), about 6e-3 in the log-probs -- a gap in which a kernel bug of the same size hides.  This module rounds
operands exactly where the kernels do (bf16 round-to-nearest-even; fp16 with the kernels' clamp at +-65504) and computes
everything else in float64, so that what separates it from the kernels is summation order and the rare rounding flip that
order causes.  Every rounding point below cites the kernel line it mirrors (csrc/ = voice_activity_detection_amd/csrc/).

Switches: ``rounding=False`` runs the same structure without any rounding (then it is the fp32 oracle up to summation
order); ``key_split=True`` computes the tail groups of one or two query blocks the way the persistent attention kernel's
key-split items do (row_mode 5 and the automatic schedule of large batches, unless batch_invariant); ``plant=`` injects one
of the named bugs of PLANTS; ``info`` (a dict) receives the number of reference moves and of clamped residual elements.

May be imported only by tests/ and scripts/ -- never by the product package.
"""
from __future__ import annotations

import math
from contextlib import contextmanager

import numpy as np
import torch

D = 128
DFF = 4 * D
TILE = 32                        # keys per attention tile (csrc/savad_kernels_bf16.h:729-743: one MFMA tile of keys)
RESCALE_LOG2 = 16.0              # csrc/savad_device.h
NEG_BIG = -1.0e30                # csrc/savad_device.h
LN_EPS = 1e-5                    # csrc/savad_device.h
F16_MAX = 65504.0

# Max-abs log-prob gaps allowed between a bf16 kernel and this model (tests/test_gpu_bf16_model.py): 2x what
# scripts/ubench/bf16_model_gap.py measured on an MI355X (per-group numbers in that test's docstring) on seeded weights, and on
# the two sharp-softmax weight sets, whose rounding-flip floor is higher.
KERNEL_GAP_BOUND = 1.5e-3
SHARP_GAP_BOUND = {"q/k x6": 4e-3, "trained clip": 9e-2}

# Bugs a kernel could plausibly have, each one small enough to hide in the bf16 noise against the fp32 oracle
PLANTS = {
    "tail_drop_key": "the last key of a ragged tail tile is masked as if it did not exist",
    "l_from_bf16_p": "the row sum l is summed from the bf16-rounded probabilities instead of the unrounded ones",
    "residual_bf16": "the residual stream is parked as bf16 instead of fp16",
    "residual_unparked": "the residual stream is not parked at all (kept fp32)",
    "residual_parked_twice": "the residual is parked once more, after the out-projection",
    "pe_shift": "frame t gets the positional-encoding row of frame t + 1",
    "move_no_rescale_l": "a reference move rescales O but not the row sum l",
    "move_half_l": "a reference move rescales only one lane half's share of the row sum l",
    "move_half_o": "a reference move rescales only the first 64 context features of O",
    "ln_reads_parked": "the LayerNorm after a parked residual reads the fp16 copy instead of the fp32 registers",
    "ctx_round_before_norm": "the context is rounded to bf16 before, not after, the division by l",
    "q_round_before_scale": "Q is rounded to bf16 before the log2(e)/sqrt(D) scale as well as after it",
}


@contextmanager
def _threads(n: int):
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(int(n), 16)))
    try:
        yield
    finally:
        torch.set_num_threads(old)


class _Arith:
    """the rounding operators (identities when rounding is off) and the counters"""

    def __init__(self, rounding: bool, plant, dtype=torch.float64):
        self.rounding = rounding
        self.dtype = dtype
        self.plant = plant
        self.moves = 0
        self.saturations = 0

    def bf(self, t: torch.Tensor) -> torch.Tensor:
        # every (__bf16) conversion of the kernels: v_cvt_pk_bf16_f32, round to nearest even, of an fp32 value
        if not self.rounding:
            return t
        return t.to(torch.float32).to(torch.bfloat16).to(self.dtype)

    def park(self, t: torch.Tensor) -> torch.Tensor:
        # store_hblock (csrc/savad_kernels_bf16.h:110-133; park_h, csrc/savad_packed_bf16.h:42): clamp to +-65504 (:120), then
        # convert to fp16 (:122); load_hblock (:96-106) adds the fp16 value onto a zeroed fp32 accumulator
        if not self.rounding or self.plant == "residual_unparked":
            return t
        self.saturations += int((~(t.abs() <= F16_MAX)).sum())
        if self.plant == "residual_bf16":
            return self.bf(t.clamp(-F16_MAX, F16_MAX))
        return t.clamp(-F16_MAX, F16_MAX).to(torch.float32).to(torch.float16).to(self.dtype)


def positional_encoding(T: int) -> np.ndarray:
    """build_pe (csrc/savad.hip:211-224) operation for operation: fp32 frequency and angle, sin / cos in double rounded to
    fp32, divided by sqrt(D) in fp32"""
    cexp = np.float32(-(math.log(10000.0) / D))
    scale = np.float32(math.sqrt(D))
    i2 = np.arange(0, D, 2, dtype=np.float32)
    wv = np.exp((i2 * cexp).astype(np.float64)).astype(np.float32)
    a = np.arange(T, dtype=np.float32)[:, None] * wv[None, :]          # fp32 product (:219)
    pe = np.empty((T, D), dtype=np.float32)
    pe[:, 0::2] = np.sin(a.astype(np.float64)).astype(np.float32) / scale
    pe[:, 1::2] = np.cos(a.astype(np.float64)).astype(np.float32) / scale
    return pe


def _fold(W, b, gamma, beta):
    """fold_ln_kernel (csrc/savad_aux_kernels.h): W' = fp32(W * gamma), b' = fp32(b + sum W beta in double)"""
    Wf = (W.astype(np.float32) * gamma.astype(np.float32)[None, :]).astype(np.float32)
    bf = (b.astype(np.float64) + W.astype(np.float64) @ beta.astype(np.float64)).astype(np.float32)
    return Wf, bf


def _t(a, dtype=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)


def _prepare(state: dict, A: _Arith):
    """the weights as the bf16 kernels hold them: folded (fp32) and packed to bf16 fragments (pack_weight_frags_kernel,
    csrc/savad_kernels_bf16.h:1027: (__bf16)W), biases fp32; the classifier stays fp32 (RowArgsBf16::wc, :798)"""
    s = {k: np.asarray(v, dtype=np.float32) for k, v in state.items()}
    L = 1 + max(int(k.split(".")[2]) for k in s if k.startswith("encoder.layers."))
    P = {"win": A.bf(_t(s["input_layer.0.weight"], A.dtype)), "bin": _t(s["input_layer.0.bias"], A.dtype), "layers": []}
    for l in range(L):
        p = f"encoder.layers.{l}."
        g1, b1n = s[p + "self_attention_sublayer.layer_norm.weight"], s[p + "self_attention_sublayer.layer_norm.bias"]
        g2, b2n = s[p + "feed_forward_sublayer.layer_norm.weight"], s[p + "feed_forward_sublayer.layer_norm.bias"]
        lay = {}
        for nm, key in (("q", "query"), ("k", "key"), ("v", "value")):
            W, b = _fold(s[p + f"self_attention.{key}_projection.weight"], s[p + f"self_attention.{key}_projection.bias"], g1, b1n)
            lay["w" + nm], lay["b" + nm] = A.bf(_t(W, A.dtype)), _t(b, A.dtype)
        lay["wo"], lay["bo"] = A.bf(_t(s[p + "self_attention.final_projection.weight"], A.dtype)), _t(s[p + "self_attention.final_projection.bias"], A.dtype)
        W1, b1 = _fold(s[p + "feed_forward.feed_forward.0.weight"], s[p + "feed_forward.feed_forward.0.bias"], g2, b2n)
        lay["w1"], lay["b1"] = A.bf(_t(W1, A.dtype)), _t(b1, A.dtype)
        lay["w2"], lay["b2"] = A.bf(_t(s[p + "feed_forward.feed_forward.3.weight"], A.dtype)), _t(s[p + "feed_forward.feed_forward.3.bias"], A.dtype)
        P["layers"].append(lay)
    wc, bc = _fold(s["classifier.weight"], s["classifier.bias"], s["encoder.layer_norm.weight"], s["encoder.layer_norm.bias"])
    P["wc"], P["bc"] = _t(wc, A.dtype), _t(bc, A.dtype)
    return P


def _layernorm(h: torch.Tensor) -> torch.Tensor:
    """layernorm_regs (csrc/savad_device.h): fp32 statistics, biased variance, no affine part (folded)"""
    mean = h.mean(-1, keepdim=True)
    d = h - mean
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS)


def _tiles(k: torch.Tensor, v: torch.Tensor, j: int, A: _Arith):
    """keys 32 j .. 32 j + 31 of every sequence, and which of them exist (missing keys: NEG_BIG, csrc/savad_kernels_bf16.h:740)"""
    T = k.shape[1]
    kj, vj = k[:, TILE * j:TILE * (j + 1)], v[:, TILE * j:TILE * (j + 1)]
    ok = torch.ones(kj.shape[1], dtype=torch.bool)
    if A.plant == "tail_drop_key" and T % TILE and TILE * (j + 1) >= T:
        ok[-1] = False
    return kj, vj, ok


def _online(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, blocks, A: _Arith, count):
    """online_softmax_shifted + attn_tile (csrc/savad_kernels_bf16.h:610-669) over the key blocks `blocks`, in order.
    q [B,M,D] (bf16, pre-scaled: scores in the base-2 exponent domain), k / v [B,T,D] (bf16).  count [B,M] bool: rows whose
    moves are counted.  Returns (O, l, reference)."""
    B, M, _ = q.shape
    ref = torch.zeros(B, M, dtype=q.dtype)               # attn_state_init (:615-620): reference 0
    l0 = torch.zeros(B, M, dtype=q.dtype)                # l_run of lane half h = 0 (keys 8 i + 0..3) ...
    l1 = torch.zeros(B, M, dtype=q.dtype)                # ... and h = 1 (keys 8 i + 4..7): they meet in store_ctx (:674)
    O = torch.zeros(B, M, D, dtype=q.dtype)
    for i, j in enumerate(blocks):
        first = i == 0
        kj, vj, ok = _tiles(k, v, j, A)
        s = torch.einsum("bmd,bnd->bmn", q, kj) - ref[..., None]      # negm rides in as the C operand of the S^T MFMA (:657-660)
        s = torch.where(ok, s, torch.full_like(s, NEG_BIG))           # mask (:661, :740)
        if s.shape[-1] < TILE:                                        # keys behind the sequence's end: NEG_BIG as well
            s = torch.cat([s, torch.full((B, M, TILE - s.shape[-1]), NEG_BIG, dtype=s.dtype)], -1)
            vj = torch.cat([vj, torch.zeros(B, TILE - vj.shape[1], D, dtype=vj.dtype)], 1)
        mx = s.amax(-1)                                               # row maximum over both lane halves (:622-625)
        move = (mx > RESCALE_LOG2) | ((mx < -RESCALE_LOG2) if first else torch.zeros_like(mx, dtype=torch.bool))   # (:626)
        A.moves += int((move & count).sum())
        d = torch.where(move, mx, torch.zeros_like(mx))               # new reference = old + d (:628)
        if not first:                                                 # O and l are still zero on the first tile (:629)
            alpha = torch.exp2(-d)                                    # (:630-633)
            if A.plant == "move_half_l":
                l0 = l0 * alpha
            elif A.plant != "move_no_rescale_l":
                l0, l1 = l0 * alpha, l1 * alpha
            if A.plant == "move_half_o":
                O = torch.cat([O[..., :D // 2] * alpha[..., None], O[..., D // 2:]], -1)
            else:
                O = O * alpha[..., None]
        s = s - d[..., None]                                          # (:637-638)
        ref = ref + d
        p = torch.exp2(s)                                             # fp32 exponentials (:644)
        pb = A.bf(p)                                                  # p -> bf16 for the PV MFMA (pack_half, :663)
        ps = pb if A.plant == "l_from_bf16_p" else p                  # the row sum takes the UNROUNDED p (:645)
        half = (torch.arange(TILE) // 4) % 2
        l0 = l0 + ps[..., half == 0].sum(-1)
        l1 = l1 + ps[..., half == 1].sum(-1)
        O = O + torch.einsum("bmn,bnd->bmd", pb, vj)                  # O^T += V^T P^T, fp32 accumulation (:666-667)
    return O, l0 + l1, ref


def _attention(q, k, v, A: _Arith, key_split: bool):
    """the context of every query row: [B,T,D] (bf16)"""
    B, T, _ = q.shape
    QB = (T + TILE - 1) // TILE
    ctx = torch.empty(B, T, D, dtype=q.dtype)
    split_from = T
    if key_split and QB % 8 in (1, 2):
        # persistent attention kernel (csrc/savad_attn_pw_bf16.h:7; row_mode 5): a sequence's tail group of one or two query
        # blocks is a KEY-SPLIT item (scripts/gen_attn_pw.py emit_ks_item :1270): wave w takes key blocks w, w + 4, ... and runs
        # its own online softmax from reference 0 (emit_ks_first :1152: the first tile's move rule); emit_ks_combine (:1163):
        # common reference r = max r_w, f_w = 2^(r_w - r) / sum_u l_u 2^(r_u - r), context = sum_w f_w O_w in fp32, then one
        # bf16 rounding (v_cvt_pk_bf16_f32 of the sum).  No rounding point of its own beyond the per-wave bf16 p.
        split_from = TILE * (QB // 8) * 8
        qs = q[:, split_from:]
        cnt = torch.ones(qs.shape[:2], dtype=torch.bool)
        parts = [_online(qs, k, v, list(range(w, QB, 4)), A, cnt) for w in range(min(4, QB))]
        r = torch.stack([pr[2] for pr in parts]).amax(0)
        lsum = sum(pr[1] * torch.exp2(pr[2] - r) for pr in parts)
        acc = sum(pr[0] * (torch.exp2(pr[2] - r) / lsum)[..., None] for pr in parts)
        ctx[:, split_from:] = A.bf(acc)
    if split_from > 0:
        qo = q[:, :split_from]
        O, l, _ = _online(qo, k, v, list(range(QB)), A, torch.ones(qo.shape[:2], dtype=torch.bool))
        inv = 1.0 / l                                                 # store_ctx (:674): 1 / (both halves' row sums)
        if A.plant == "ctx_round_before_norm":
            ctx[:, :split_from] = A.bf(A.bf(O) * inv[..., None])
        else:
            ctx[:, :split_from] = A.bf(O * inv[..., None])            # normalised context -> bf16 fragments (:678-680)
    return ctx


def _qkv(n: torch.Tensor, lay: dict, A: _Arith):
    """qkv_block_bf16 (csrc/savad_kernels_bf16.h:298-326): the bias is the accumulator's initial value (:305, :310), Q is
    multiplied by qscale = fp32(log2(e) / sqrt(D)) (csrc/savad.hip:1299) in fp32 (:319), then Q, K and V^T -> bf16 (:325)"""
    qscale = float(np.float32(1.4426950408889634 / math.sqrt(D)))
    q = lay["bq"] + n @ lay["wq"].T
    if A.plant == "q_round_before_scale":
        q = A.bf(q)
    q = A.bf(q * qscale)
    k = A.bf(lay["bk"] + n @ lay["wk"].T)
    v = A.bf(lay["bv"] + n @ lay["wv"].T)
    return q, k, v


def forward(state: dict, x: np.ndarray, *, rounding: bool = True, key_split: bool = False, plant: str | None = None,
            info: dict | None = None, threads: int = 16, dtype: str = "float64") -> np.ndarray:
    """state: the state_dict (key -> float32 array) that oracle.forward takes; x [B,T,F] (float32, or values that are already
    bf16: feeding a bf16 tensor to the kernels is the same as rounding these).  Returns float64 log-probabilities [B,T,2].
    dtype="float32" evaluates the SAME model on float tensors: its difference from the float64 evaluation (the model's
    self-difference) is the rounding-flip floor of this arithmetic at a state and input."""
    if plant is not None and plant not in PLANTS:
        raise ValueError(f"unknown plant {plant!r}")
    A = _Arith(rounding, plant, getattr(torch, dtype))
    with _threads(threads), torch.no_grad():
        P = _prepare(state, A)
        x = np.asarray(x, dtype=np.float32)
        B, T, F = x.shape
        assert P["win"].shape == (D, F), "feature size / d_model mismatch"
        pe = positional_encoding(T + 1)
        pe = _t(pe[1:] if plant == "pe_shift" else pe[:T], A.dtype)
        # input stage (input_qkv_kernel_bf16, csrc/savad_kernels_bf16.h:376-392; the persistent form :520-578 and the packed
        # single launch, csrc/savad_packed_bf16.h:144-189, do the same): features -> bf16 (load_x_frag :335-336), the fp32
        # accumulator starts at bias + PE (:380-381) and takes the bf16 products (:390)
        h = P["bin"] + pe[None] + A.bf(_t(x, A.dtype)) @ P["win"].T
        hp = A.park(h)                                                # store_hblock (:392)
        for l, lay in enumerate(P["layers"]):
            last = l == len(P["layers"]) - 1
            # layer 0's LayerNorm reads the fp32 registers (:394), later layers' the fp32 registers of the row chain
            # (csrc/savad_kernels_bf16.h:888); only the residual added after the attention comes from the parked copy (:856)
            n = A.bf(_layernorm(hp if plant == "ln_reads_parked" else h))     # pack_row (:69)
            q, k, v = _qkv(n, lay, A)
            ctx = _attention(q, k, v, A, key_split)
            # row chain (row_stage_bf16, :815-916): h1 = parked h + bo + ctx Wo^T (:856-863)
            h1 = hp + lay["bo"] + ctx @ lay["wo"].T
            if plant == "residual_parked_twice":
                h1 = A.park(h1)
            n = A.bf(_layernorm(h1))                                  # (:865-866)
            a = A.bf(lay["b1"] + n @ lay["w1"].T)                    # FFN1: bias-initialised accumulator (:876-877) -> bf16 (:881)
            a = torch.clamp_min(a, 0.0)                               # ReLU on the packed bf16 (relu_frag :60-63, applied at :881-882)
            h = h1 + lay["b2"] + a @ lay["w2"].T                     # FFN2 accumulates onto h1 + b2 (:868-870, :885)
            if not last:
                hp = A.park(h)                                        # (:887)
        # tail (:888, :897-914): final LayerNorm (fp32, from registers) and the fp32 classifier [2][D] with the folded bias, log-softmax
        z = _layernorm(h) @ P["wc"].T + P["bc"]
        out = torch.log_softmax(z, -1)
    if info is not None:
        info["moves"] = A.moves
        info["saturations"] = A.saturations
    return out.to(torch.float64).numpy()
