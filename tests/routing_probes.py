"""Attention routing probes, shared by tests/test_routing_probes_host.py (CPU), tests/test_gpu_routing_probes.py (GPU) and
tests/golden/make_golden_routing.py.

Every other parity test draws dense random weights, under which the attention softmax is diffuse: at T = 800 a key carries about
1 / 800 of a row's context, and a kernel that drops one key, one key tile or mishandles one row of a query block moves the output by
a fraction of the tolerance ("Routing probes"; test_the_old_inputs_are_blind asserts the figures).  Here the INPUTS decide
which key every query attends to, under one ordinary state_dict:

    state    seeded_state_dict(1234) with the input layer, layer 0's attention LayerNorm and its query / key projections replaced:
             features 0..11 -> hidden 0..11 (x A, the key code), features 12..23 -> hidden 12..23 (x A, the query code), the other
             features -> the content columns (x 1); q[d] = c n[12 + d], k[d] = n[d] for d < 12.  Everything else as seeded.
    inputs   frame t carries code(t) as key code and code(targets[b, t]) as query code, code(p) = 6 (cos, sin) pairs of periods
             3, 5, 7, 11, 13, 17 (lcm 255 255, equal norm); the content is standard normal, mean 0 and deviation 1 per frame.
    targets  every sequence is a permutation of the keys: cyclic shifts by 33 k, the reversal, a random permutation -- together
             every (query block of 32, key tile of 32) pair is the (block, target tile) of some query (asserted, sequences added
             where the rule misses one).  All sequences of a batch have the same key codes and different content.
    regimes  `sharp` c = 100: the target holds >= 0.999 of every row.  `soft` c = SOFT_C[d_model, T]: the median target
             probability is in [0.5, 0.7], so that a key counted twice or a wrong normaliser shows as well.

    truth    oracle/torch_port.py on double tensors (pinned to the reference's own float64 outputs at T <= 129, golden_routing.npz)
    floor    the larger error of two plain fp32 evaluations (the port on float tensors, the C oracle) against the truth
    bound    max(TIGHT, 3 x floor), 3 x floor within TOL

DEVIATIONS restate layer 0's attention with one routing fault each; the host test asserts which of them move the truth past
VISIBLE x bound under the per-block share rule, and the GPU test holds every kernel path to the truth at `bound`, row by row."""
from __future__ import annotations

import math
from contextlib import contextmanager
from functools import lru_cache
from pathlib import Path

import numpy as np

from tests.numeric_regimes import FLOOR_FACTOR, STATE_SEED, TIGHT, TOL, VISIBLE, bf16_bound_of, bound_of, num_layers, pw_splits  # noqa: F401

GOLDEN = Path(__file__).resolve().parent / "golden" / "golden_routing.npz"
GOLDEN_T = (7, 33, 70, 129)     # the lengths pinned to the reference (the longer ones would make the fixture large)

PERIODS = (3, 5, 7, 11, 13, 17)
NCODE = 2 * len(PERIODS)        # 12 columns per code
A = 4.0                         # weight of both codes in the input layer
SHARP_C = 100.0
FEATURES = 80
BLOCK = 32                      # rows of a query block = keys of a key tile, in every attention kernel of the d_model = 128 families

SHAPES = (7, 32, 33, 70, 129, 264, 800, 801)
GENERIC_SHAPES = (33, 129)      # d_model 64, csrc/savad_generic.h
REGIMES = ("sharp", "soft")

# soft: c found by search_soft_c (bisection on the float64 port's layer-0 probabilities, median target probability 0.6, rounded to
# three digits); the host test asserts the median these values give and that the search still lands on them
SOFT_C = {
    (128, 7): 0.656, (128, 32): 1.06, (128, 33): 1.06, (128, 70): 1.31, (128, 129): 1.56, (128, 264): 1.95, (128, 800): 2.69, (128, 801): 2.69,
    (64, 33): 1.42, (64, 129): 2.08,
}

CONTENT_SEED = 68_000          # the content of shape T is drawn from seed CONTENT_SEED + T
SHARE = 0.9                     # per-block rule: the share of touched rows that must move by VISIBLE x bound
PER_KEY_MOVE = 1e-2             # per-key rule: the best row that targets a key moves by at least this


# ---- construction ---------------------------------------------------------------------------------------------------------------
def code(p) -> np.ndarray:
    """[..., 12] float64: (cos, sin) of 2 pi p / P for the six periods"""
    p = np.asarray(p, dtype=np.float64)[..., None]
    a = 2.0 * np.pi * p / np.asarray(PERIODS, dtype=np.float64)
    return np.stack([np.cos(a), np.sin(a)], -1).reshape(p.shape[:-1] + (NCODE,))


def content_columns(d_model):
    """(first feature, first hidden column, count) of the content: d_model 128 has room for all 56 features on hidden 64..119,
    d_model 64 carries features 24..63 on hidden 24..63 (features 64..79 then reach nothing)"""
    return (2 * NCODE, 64, FEATURES - 2 * NCODE) if d_model == 128 else (2 * NCODE, 2 * NCODE, d_model - 2 * NCODE)


def routing_state(c, d_model=128):
    from voice_activity_detection_amd.seeded import seeded_state_dict

    st = {k: v.copy() for k, v in seeded_state_dict(STATE_SEED, d_model=d_model).items()}
    w = np.zeros_like(st["input_layer.0.weight"])
    for i in range(2 * NCODE):
        w[i, i] = A
    f0, h0, n = content_columns(d_model)
    for i in range(n):
        w[h0 + i, f0 + i] = 1.0
    st["input_layer.0.weight"] = w
    st["input_layer.0.bias"] = np.zeros_like(st["input_layer.0.bias"])
    p = "encoder.layers.0."
    st[p + "self_attention_sublayer.layer_norm.weight"] = np.ones(d_model, np.float32)
    st[p + "self_attention_sublayer.layer_norm.bias"] = np.zeros(d_model, np.float32)
    wq, wk = np.zeros((d_model, d_model), np.float32), np.zeros((d_model, d_model), np.float32)
    for d in range(NCODE):
        wq[d, NCODE + d] = c
        wk[d, d] = 1.0
    st[p + "self_attention.query_projection.weight"], st[p + "self_attention.key_projection.weight"] = wq, wk
    st[p + "self_attention.query_projection.bias"] = np.zeros(d_model, np.float32)
    st[p + "self_attention.key_projection.bias"] = np.zeros(d_model, np.float32)
    return st


def blocks_of(T):
    return (T + BLOCK - 1) // BLOCK


def pairs_covered(targets) -> set:
    t = np.arange(targets.shape[1])
    return {(int(a), int(b)) for row in targets for a, b in zip(t // BLOCK, row // BLOCK)}


@lru_cache(maxsize=None)
def _target_sets(T):
    t = np.arange(T)
    nb = blocks_of(T)
    rows = [(t + 33 * k) % T for k in range(nb)] if T > BLOCK else [(t + k) % T for k in range(T)]
    rows += [T - 1 - t, np.random.default_rng(61_000 + T).permutation(T)]
    if T > BLOCK:   # the shift rule can miss a (query block, key tile) pair: one more shift per missed pair
        for qb in range(nb):
            for kt in range(nb):
                if (qb, kt) not in pairs_covered(np.stack(rows)):
                    rows.append((t + BLOCK * (kt - qb)) % T)
    out = np.stack(rows).astype(np.int64)
    out.setflags(write=False)
    return out


def target_sets(T) -> np.ndarray:
    """[B, T]: the key each query of each sequence attends to -- every row a permutation of the keys"""
    return _target_sets(int(T))


def routing_inputs(T, targets, seed, d_model=128) -> np.ndarray:
    B = targets.shape[0]
    x = np.zeros((B, T, FEATURES), np.float64)
    x[:, :, :NCODE] = code(np.arange(T))[None]
    x[:, :, NCODE:2 * NCODE] = code(targets)
    f0, _, n = content_columns(d_model)
    z = np.random.default_rng(seed).standard_normal((B, T, n))
    z -= z.mean(-1, keepdims=True)
    z /= z.std(-1, keepdims=True)
    x[:, :, f0:f0 + n] = z
    return x.astype(np.float32)


def soft_c(T, d_model=128):
    return SOFT_C[(d_model, T)]


def regime_c(regime, T, d_model=128):
    return SHARP_C if regime == "sharp" else soft_c(T, d_model)


@lru_cache(maxsize=None)
def case(regime, T, d_model=128):
    """(state, x, targets) of a case; the arrays are shared and read-only"""
    tg = target_sets(T)
    x = routing_inputs(T, tg, CONTENT_SEED + T, d_model)
    x.setflags(write=False)
    return routing_state(regime_c(regime, T, d_model), d_model), x, tg


def case_id(regime, T, d_model=128):
    return f"{regime}-T{T}" + ("" if d_model == 128 else f"-d{d_model}")


def golden_key(regime, T):
    return f"{regime}_T{T}"


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- deviations -----------------------------------------------------------------------------------------------------------------
# name -> what a kernel would have done.  Each is applied to layer 0's attention of the float64 port (hooked_port below).
DEVIATIONS = {
    "a_target_dropped": "the target key is left out of the row's softmax",
    "b_v_rows_swapped": "V rows 2 k and 2 k + 1 are swapped",
    "c_query_rows_swapped": "query rows 2 k and 2 k + 1 read each other's scores",
    "d_last_key_last_block": "the last key is left out for the last query block only",
    "e_tile_not_separated": "T <= 16: the softmax of a packed tile runs over the keys of every sequence in the tile",
    "f_split_unweighted": "T > 32: the partial results of two key ranges are averaged without their exp(m_k - m) weights",
    "g_target_twice": "the target key is counted twice",
    "h_tile_twice": "the keys of the last 32-key tile are counted twice",
}
SOFT_ONLY = ("g_target_twice", "h_tile_twice")


def applies(dev, regime, T):
    if dev in SOFT_ONLY and regime != "soft":
        return False
    if dev == "h_tile_twice":   # with one tile every key is counted twice, which is no change
        return T > BLOCK
    if dev == "e_tile_not_separated":
        return BLOCK // T >= 2
    if dev == "f_split_unweighted":
        return T > BLOCK
    return True


def deviations_of(regime, T):
    return [d for d in DEVIATIONS if applies(d, regime, T)]


def pair_swap(n):
    """the index permutation 2 k <-> 2 k + 1 (an odd last element stays)"""
    idx = np.arange(n)
    m = n - n % 2
    idx[:m] = idx[:m] ^ 1
    return idx


def split_point(T):
    """the first key of the second key range of deviation f: whole tiles, the larger half first"""
    return BLOCK * ((blocks_of(T) + 1) // 2)


def touched_rows(dev, targets) -> np.ndarray:
    """[B, T] bool: the rows whose result the deviation changes by construction (the rows the share rule counts)"""
    B, T = targets.shape
    m = np.ones((B, T), bool)
    if dev == "b_v_rows_swapped":
        m = pair_swap(T)[targets] != targets
    elif dev == "c_query_rows_swapped":
        m[:, pair_swap(T) == np.arange(T)] = False
    elif dev == "d_last_key_last_block":
        m = (targets == T - 1) & (np.arange(T)[None] >= BLOCK * (blocks_of(T) - 1))
    elif dev == "h_tile_twice":
        m = targets >= BLOCK * (blocks_of(T) - 1)
    return m


def _renorm(P):
    return P / P.sum(-1, keepdim=True)


def deviated_context(dev, q, k, v, targets):
    """layer 0's context [B, T, D] with the deviation; q, k, v [B, T, D] as the port has them"""
    import torch

    B, T, D = q.shape
    s = q @ k.transpose(1, 2) / np.sqrt(D)
    tg = torch.from_numpy(np.array(targets))
    if dev == "e_tile_not_separated":
        per = BLOCK // T
        ctx = torch.empty_like(v)
        for b0 in range(0, B, per):
            kk, vv = k[b0:b0 + per].reshape(1, -1, D), v[b0:b0 + per].reshape(1, -1, D)
            ctx[b0:b0 + per] = torch.softmax(q[b0:b0 + per] @ kk.transpose(1, 2) / np.sqrt(D), -1) @ vv
        return ctx
    if dev == "f_split_unweighted":
        ks = split_point(T)
        return 0.5 * (torch.softmax(s[..., :ks], -1) @ v[:, :ks] + torch.softmax(s[..., ks:], -1) @ v[:, ks:])
    P = torch.softmax(s, -1)
    if dev == "a_target_dropped":
        P = _renorm(P.scatter(2, tg[..., None], 0.0))
    elif dev == "b_v_rows_swapped":
        v = v[:, torch.from_numpy(pair_swap(T))]
    elif dev == "c_query_rows_swapped":
        P = P[:, torch.from_numpy(pair_swap(T))]
    elif dev == "d_last_key_last_block":
        P = P.clone()
        P[:, BLOCK * (blocks_of(T) - 1):, T - 1] = 0.0
        P = _renorm(P)
    elif dev == "g_target_twice":
        P = _renorm(P.scatter(2, tg[..., None], 2.0 * P.gather(2, tg[..., None])))
    elif dev == "h_tile_twice":
        P = P.clone()
        P[:, :, BLOCK * (blocks_of(T) - 1):] *= 2.0
        P = _renorm(P)
    else:
        raise ValueError(dev)
    return P @ v


# ---- CPU evaluations ------------------------------------------------------------------------------------------------------------
@contextmanager
def _threads(n):
    import torch

    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(int(n), 16)))
    try:
        yield
    finally:
        torch.set_num_threads(old)


def threads_for(T):
    """the short shapes are quicker on one thread (tests/numeric_regimes.py); the long ones are GEMM-bound"""
    return 1 if T <= 129 else 16


def _tensors(state, x, dtype):
    import torch

    dt = getattr(torch, dtype)
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in state.items()}, torch.from_numpy(np.array(x)).to(dt)   # (x is read-only: a copy)


def port(state, x, dtype="float64", threads=1) -> np.ndarray:
    from oracle import torch_port

    st, xt = _tensors(state, x, dtype)
    with _threads(threads):
        return torch_port.forward(st, xt).numpy()


def hooked_port(state, x, layer_hook=None, layer=0, dtype="float64", threads=1, upto_probabilities=False):
    """oracle/torch_port.py restated operation for operation, with the attention of `layer` handed to layer_hook(q, k, v) -> context
    (None: the port's own).  upto_probabilities: return that layer's probability matrix [B, T, T] instead of going on."""
    import torch

    from oracle import torch_port

    F = torch.nn.functional
    st, h = _tensors(state, x, dtype)
    B, T, _ = h.shape
    D = st["input_layer.0.weight"].shape[0]
    with _threads(threads), torch.no_grad():
        h = F.linear(h, st["input_layer.0.weight"], st["input_layer.0.bias"])
        h = h + torch_port.positional_encoding(T, D).unsqueeze(0).to(h.dtype) / math.sqrt(D)
        for l in range(num_layers(state)):
            p = f"encoder.layers.{l}."
            n = F.layer_norm(h, (D,), st[p + "self_attention_sublayer.layer_norm.weight"], st[p + "self_attention_sublayer.layer_norm.bias"])
            q, k, v = (F.linear(n, st[p + f"self_attention.{nm}_projection.weight"], st[p + f"self_attention.{nm}_projection.bias"])
                       for nm in ("query", "key", "value"))
            if l == layer and upto_probabilities:
                return torch.softmax(q @ k.transpose(1, 2) / np.sqrt(D), -1).numpy()
            ctx = layer_hook(q, k, v) if l == layer and layer_hook is not None else None
            if ctx is None:
                ctx = torch.softmax(q @ k.transpose(1, 2) / np.sqrt(D), -1) @ v
            h = F.linear(ctx, st[p + "self_attention.final_projection.weight"], st[p + "self_attention.final_projection.bias"]) + h
            n = F.layer_norm(h, (D,), st[p + "feed_forward_sublayer.layer_norm.weight"], st[p + "feed_forward_sublayer.layer_norm.bias"])
            f = F.linear(torch.relu(F.linear(n, st[p + "feed_forward.feed_forward.0.weight"], st[p + "feed_forward.feed_forward.0.bias"])),
                         st[p + "feed_forward.feed_forward.3.weight"], st[p + "feed_forward.feed_forward.3.bias"])
            h = f + h
        h = F.layer_norm(h, (D,), st["encoder.layer_norm.weight"], st["encoder.layer_norm.bias"])
        return F.log_softmax(F.linear(h, st["classifier.weight"], st["classifier.bias"]), dim=2).numpy()


def deviated(state, x, targets, dev, layer=0, threads=1) -> np.ndarray:
    return hooked_port(state, x, lambda q, k, v: deviated_context(dev, q, k, v, targets), layer=layer, threads=threads)


def target_probabilities(state, x, targets, threads=1) -> np.ndarray:
    """[B, T] float64: layer 0's probability of each query's target key"""
    P = hooked_port(state, x, threads=threads, upto_probabilities=True)
    return np.take_along_axis(P, targets[..., None], 2)[..., 0]


def search_soft_c(T, d_model=128, want=0.6):
    """the c at which the median target probability of layer 0 is `want`: bisection on the float64 port (the scores are linear in c,
    so one evaluation at c = 1 serves), rounded to three digits"""
    import torch

    tg = target_sets(T)
    x = routing_inputs(T, tg, CONTENT_SEED + T, d_model)
    st, xt = _tensors(routing_state(1.0, d_model), x, "float64")
    F = torch.nn.functional
    from oracle import torch_port

    with _threads(threads_for(T)), torch.no_grad():
        h = F.linear(xt, st["input_layer.0.weight"], st["input_layer.0.bias"])
        h = h + torch_port.positional_encoding(T, d_model).unsqueeze(0).to(h.dtype) / math.sqrt(d_model)
        n = F.layer_norm(h, (d_model,))
        s = n[..., NCODE:2 * NCODE] @ n[..., :NCODE].transpose(1, 2) / np.sqrt(d_model)
        tgt = torch.from_numpy(np.array(tg))[..., None]

        def median(c):
            return float(torch.softmax(c * s, -1).gather(2, tgt).median())

        lo, hi = 0.0, SHARP_C
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if median(mid) < want else (lo, mid)
    return float(f"{0.5 * (lo + hi):.3g}")


def floor(state, x, want, threads=1):
    """the error of the same arithmetic in plain fp32: the larger of the stock-PyTorch port and the C oracle against the truth"""
    from oracle import oracle

    e_port = float(np.abs(port(state, x, "float32", threads) - want).max())
    e_c = float(np.abs(oracle.forward(state, x, threads=threads) - want).max())
    return max(e_port, e_c)


@lru_cache(maxsize=None)
def reference(regime, T, d_model=128):
    """(truth, floor, bound) of a case, computed once and left unchanged"""
    st, x, _ = case(regime, T, d_model)
    th = threads_for(T)
    want = port(st, x, "float64", th)
    want.setflags(write=False)
    fl = floor(st, x, want, th)
    return want, fl, bound_of(fl)


def row_moves(y, want) -> np.ndarray:
    """[B, T]: how far each row's log-probabilities are from the truth's"""
    return np.abs(np.asarray(y, np.float64) - want).max(-1)


def block_shares(moves, touched, threshold):
    """the per-block rule: for every (sequence, query block of at least 8 rows) with a touched row, the share of its touched rows that
    moved by at least `threshold` -> list of (sequence, block, share, touched rows)"""
    B, T = moves.shape
    out = []
    for b in range(B):
        for qb in range(blocks_of(T)):
            r = slice(BLOCK * qb, min(T, BLOCK * (qb + 1)))
            n = int(touched[b, r].sum())
            if r.stop - r.start >= 8 and n:
                out.append((b, qb, float((moves[b, r][touched[b, r]] >= threshold).sum()) / n, n))
    return out


def per_key_best(moves, touched, targets):
    """over the sequences, the largest move of a touched row that targets each key: one figure per key that a touched row targets"""
    best = np.full(targets.shape[1], -1.0)
    np.maximum.at(best, targets[touched], moves[touched])
    return best[best >= 0]


def worst_rows(y, want, targets, n=5):
    """the (sequence, query, target, error) of the n rows furthest from the truth: the triple names the (query block, key tile) at fault"""
    mv = row_moves(y, want) if np.isfinite(y).all() else np.where(np.isfinite(y).all(-1), 0.0, np.inf)
    order = np.argsort(mv, axis=None)[::-1][:n]
    rows = []
    for i in order:
        b, t = np.unravel_index(i, mv.shape)
        g = int(targets[b, t])
        rows.append(f"(sequence {b}, query {t} [block {t // BLOCK}], target {g} [tile {g // BLOCK}]): {mv[b, t]:.2e}")
    return rows


# (regime, T, d_model) -> deviations that do NOT meet the visibility condition there (asserted by the host test: every other
# applicable deviation is visible, these are not -- never dropped silently).  With CONTENT_SEED as it stands there is none.
NOT_VISIBLE = {
}


# ---- the same faults under the inputs of every other parity test ----------------------------------------------------------------
def _drop(P, rows, key):
    P = P.clone()
    P[:, rows, key] = 0.0
    return _renorm(P)


def blind_context(name, q, k, v):
    """one key mishandled in a layer whose softmax is diffuse (no targets: the key is named by its index)"""
    import torch

    T, D = q.shape[1], q.shape[2]
    P = torch.softmax(q @ k.transpose(1, 2) / np.sqrt(D), -1)
    if name == "last key dropped":
        P = _drop(P, slice(None), T - 1)
    elif name == "key 31 dropped":
        P = _drop(P, slice(None), 31)
    elif name == "last key counted twice":
        P = P.clone()
        P[:, :, T - 1] *= 2.0
        P = _renorm(P)
    elif name == "V rows 31 and 32 swapped":
        idx = torch.arange(T)
        idx[31], idx[32] = 32, 31
        v = v[:, idx]
    elif name == "last key dropped for the last query block":
        P = _drop(P, slice(BLOCK * (blocks_of(T) - 1), None), T - 1)
    else:
        raise ValueError(name)
    return P @ v


BLIND_DEVIATIONS = ("last key dropped", "key 31 dropped", "last key counted twice", "V rows 31 and 32 swapped",
                    "last key dropped for the last query block")


# ---- bf16: oracle/bf16_model.py is the restatement ------------------------------------------------------------------------------
BF16_DEVIATIONS = ("a_target_dropped", "b_v_rows_swapped", "c_query_rows_swapped", "d_last_key_last_block", "f_split_unweighted")
# (regime, T) -> the deviations that meet the visibility condition for bf16 (moves of oracle/bf16_model.py with the deviation planted,
# at VISIBLE x the bf16 bound) with room to spare: no counted block below BF16_SPARE.  The bound follows the model's self-difference,
# which moves by a tenth between hosts (6.9e-4 against 7.7e-4 at `sharp`, T = 32), so a cell that holds with one row to spare on
# one host -- a, c at `sharp` T = 33, c at `sharp` T = 129 and `soft` T = 33: 0.9375 and 0.969 -- is not listed.  Every (regime, T) is
# held to the model on the GPU; what the list says is which faults that comparison is sure to expose in at least 0.9 of a block's
# rows.  Everywhere, for a - d, every key has a row beyond VISIBLE x bound (asserted: the smallest multiple is 7).  f, the key-split
# combine, meets the share rule nowhere.
BF16_VISIBLE = {
    ("sharp", 7): ("a_target_dropped", "b_v_rows_swapped", "c_query_rows_swapped", "d_last_key_last_block"),
    ("sharp", 32): ("d_last_key_last_block",),
    ("sharp", 33): ("d_last_key_last_block",),
    ("sharp", 70): ("d_last_key_last_block",),
    ("sharp", 129): ("d_last_key_last_block",),
    ("sharp", 264): ("d_last_key_last_block",),
    ("sharp", 800): ("d_last_key_last_block",),
    ("sharp", 801): ("d_last_key_last_block",),
    ("soft", 7): ("a_target_dropped", "b_v_rows_swapped", "c_query_rows_swapped", "d_last_key_last_block"),
    ("soft", 32): (),
    ("soft", 33): ("d_last_key_last_block",),
    ("soft", 70): ("d_last_key_last_block",),
    ("soft", 129): ("d_last_key_last_block",),
    ("soft", 264): ("d_last_key_last_block",),
    ("soft", 800): ("d_last_key_last_block",),
    ("soft", 801): ("d_last_key_last_block",),
}
BF16_SPARE = 15 / 16
BF16_LONG = 800   # from this length on the bf16 model is evaluated on bf16_sequences(T) alone (the whole batch takes too long)


def bf16_sequences(T):
    """the sequences bf16 is held on: all of them below BF16_LONG; from there the shifts k = 0, 1, nb // 2, nb - 1, the reversal and
    the permutation (the model treats every sequence on its own, so a subset of the batch is the same arithmetic)"""
    B = target_sets(T).shape[0]
    if T < BF16_LONG:
        return list(range(B))
    nb = blocks_of(T)
    return sorted({0, 1, nb // 2, nb - 1, nb, nb + 1})


def bf16_applies(dev, T, key_split):
    """f is the key-split combine: it exists only in the key-split form of the model, at the lengths where row_mode 5 takes it"""
    return dev in BF16_DEVIATIONS and (dev != "f_split_unweighted" or (key_split and pw_splits(T)))


def bf16_touched_rows(dev, targets):
    m = touched_rows(dev, targets)
    if dev == "f_split_unweighted":   # the tail group of one or two query blocks
        T = targets.shape[1]
        m = m & (np.arange(T)[None] >= BLOCK * (blocks_of(T) // 8) * 8)
    return m


@contextmanager
def bf16_routing_plant(dev, targets, layers=3):
    """oracle/bf16_model.py with the attention of layer 0 carrying one deviation (the model's functions are replaced for the duration
    and restored on exit).  a and d mask keys per query row inside the model's own online softmax; b and c permute what goes in or
    comes out of it; f replaces the key-split combine by the plain mean of the partial contexts."""
    import torch

    from oracle import bf16_model as bm

    real_attention, real_online, real_tiles = bm._attention, bm._online, bm._tiles
    calls = [0]
    live = {}
    T = targets.shape[1]
    tg = torch.from_numpy(np.array(targets))

    def tiles(k, v, j, A):
        kj, vj, ok = real_tiles(k, v, j, A)
        if "mask" in live:
            off, M = live["rows"]
            ok = live["mask"][:, off:off + M, BLOCK * j:BLOCK * j + kj.shape[1]] & ok
        return kj, vj, ok

    def online(q, k, v, blocks, A, count):
        if "mask" in live:   # the key-split items of the tail group come first, then the ordinary rows from row 0
            tail = live["tail_calls"] > 0
            live["tail_calls"] -= 1
            live["rows"] = (live["split_from"] if tail else 0, q.shape[1])
        return real_online(q, k, v, blocks, A, count)

    def attention(q, k, v, A, key_split):
        layer = calls[0] % layers
        calls[0] += 1
        if layer != 0:
            return real_attention(q, k, v, A, key_split)
        QB = blocks_of(T)
        split = key_split and QB % 8 in (1, 2)
        split_from = BLOCK * (QB // 8) * 8 if split else T
        if dev == "b_v_rows_swapped":
            return real_attention(q, k, v[:, torch.from_numpy(pair_swap(T))], A, key_split)
        if dev == "c_query_rows_swapped":
            return real_attention(q, k, v, A, key_split)[:, torch.from_numpy(pair_swap(T))]
        if dev in ("a_target_dropped", "d_last_key_last_block"):
            mask = torch.ones(q.shape[0], T, T, dtype=torch.bool)
            if dev == "a_target_dropped":
                mask.scatter_(2, tg[..., None], False)
            else:
                mask[:, BLOCK * (QB - 1):, T - 1] = False
            live.update(mask=mask, split_from=split_from, tail_calls=min(4, QB) if split else 0)
            try:
                return real_attention(q, k, v, A, key_split)
            finally:
                live.clear()
        if dev == "f_split_unweighted":
            assert split
            ctx = real_attention(q, k, v, A, False)
            qs = q[:, split_from:]
            parts = [real_online(qs, k, v, list(range(w, QB, 4)), A, torch.ones(qs.shape[:2], dtype=torch.bool)) for w in range(min(4, QB))]
            ctx[:, split_from:] = A.bf(sum(O / l[..., None] for O, l, _ in parts) / len(parts))
            return ctx
        raise ValueError(dev)

    bm._attention, bm._online, bm._tiles = attention, online, tiles
    try:
        yield bm
    finally:
        bm._attention, bm._online, bm._tiles = real_attention, real_online, real_tiles


def bf16_model_out(state, x, key_split=False, dtype="float64", threads=1):
    from oracle import bf16_model

    return bf16_model.forward(state, x, key_split=key_split, dtype=dtype, threads=threads)


def bf16_planted(state, x, targets, dev, key_split=False, threads=1):
    with bf16_routing_plant(dev, targets, num_layers(state)) as bm:
        return bm.forward(state, x, key_split=key_split, threads=threads)


def bf16_forms(T):
    """the forms of the model a length is evaluated in: key_split False, and True where row_mode 5 takes the key-split tail item"""
    return (False, True) if pw_splits(T) else (False,)


@lru_cache(maxsize=None)
def bf16_reference(regime, T):
    """({key_split: model output on bf16_sequences(T)}, self-difference, bound): computed once and left unchanged"""
    st, x, _ = case(regime, T)
    xs = np.ascontiguousarray(x[bf16_sequences(T)])
    th = threads_for(T)
    want, sd = {}, 0.0
    for ks in bf16_forms(T):
        want[ks] = bf16_model_out(st, xs, ks, threads=th)
        want[ks].setflags(write=False)
        sd = max(sd, float(np.abs(bf16_model_out(st, xs, ks, "float32", th) - want[ks]).max()))
    return want, sd, bf16_bound_of(sd)


def residual_stream_peak(state, x, threads=1) -> float:
    """float64: the largest |h| of the residual stream after the input stage, after every attention branch and after every layer"""
    import torch

    from tests import numeric_regimes as nr

    peak = [0.0]

    def fn(k, h, shape, w, b):
        peak[0] = max(peak[0], float(h.abs().max()))
        return None

    st, xt = _tensors(state, x, "float64")
    with _threads(threads), nr.perturbed_layer_norm(fn) as fwd:
        fwd(st, xt)
    return peak[0]


def is_visible(moves, touched, targets, bound):
    """the visibility condition: every counted (sequence, block) has at least SHARE of its touched rows beyond VISIBLE x bound; where
    no block counts (T < 8, or a deviation that touches only a last block of fewer than 8 rows), every key that a touched row targets
    has a row beyond VISIBLE x bound instead.  -> (visible, worst share or None, smallest per-key best)"""
    shares = [s[2] for s in block_shares(moves, touched, VISIBLE * bound)]
    keys = per_key_best(moves, touched, targets)
    worst = min(shares) if shares else None
    ok = worst >= SHARE if shares else bool(keys.size and keys.min() >= VISIBLE * bound)
    return ok, worst, float(keys.min()) if keys.size else 0.0
