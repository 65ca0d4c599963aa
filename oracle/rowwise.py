"""ORACLE (test infrastructure only) -- the acoustic model's row-wise steps (csrc/acoustic_kernels.hip)
one op at a time in float64, written from the formulas include/tts_hip.h states for the tts_op_*
entries; for the ops that do at most one fp32 operation and one rounding the expected bits; for the
ops that really compute an error bound per output element taken from the reference alone, and a
NumPy float32 replay of the kernel's arithmetic that carries injected defects.

Operands hold values of the working dtype already (`round_to`), so operand rounding stays out of
every comparison.  Everything is per utterance where the op has utterances.

Exact ops (`*_expected`): embed, regulate (fp32 multiply by the scale, one rounding), pos_bias (one
fp32 add, one rounding), transpose_v and mel_out (copies), durations (integers).

Error model of the bounded ops (u = 2^-24; uT the unit roundoff of the output dtype, + 2^-25 for
f16's subnormal spacing: `out_round`; TINY = 2^-126, below which the hardware exponential flushes):
  fast exp      __expf(x) = exp2(x * log2e): the scaled argument carries two roundings (the constant
                and the product), 2 u |x| log2e absolute, i.e. 2 u |x| relative in the result; the
                hardware exp2 is good to one ulp = 2 u.  EXP_REL(x) = 2 u (1 + |x|), + TINY absolute.
  sigmoid       s = 1 / (1 + E), E = __expf(-x): ds/dE = -s^2, so |ds| <= s (1 - s) EXP_REL(x), + u s for
                the add and 2 u s for the division (a reciprocal good to one ulp), + TINY where E over- or
                underflows (there the true s is within 2^-126 of 0 or 1).
  glu_dwconv    g = x s: |x| ds + u |g|.  acc = bias + sum_j w_j g_j by k fused multiply-adds:
                sum |w_j| dg_j + (k + 1) u (|bias| + sum |w_j g_j|).  SiLU y = acc s(acc) is 1.1-Lipschitz:
                1.1 dacc + |acc| ds(acc).  Then the output rounding.
  rel_softmax   s_j = (ac_j + bd_j) * scale: 2 u |s_j|; a_j = s_j - max: u |a_j| (the max itself is a
                common shift and cancels); e_j = __expf(a_j): relative r_j = 2 u |s_j| + u |a_j| + EXP_REL(a_j);
                the sum of L terms in any order: (L - 1) u, its error from the terms sum_i p_i r_i; one
                reciprocal (2 u) and one product (u): dp_j = p_j (r_j + sum_i p_i r_i + (L + 2) u) + TINY.
                The row sum of the outputs is within sum_j bound_j of 1.
  spk_bias      ss = sum e_i^2 in 256 partial sums of ceil(E / 256) fused multiply-adds and an 8-level
                tree: (ceil(E / 256) + 9) u relative; the root 2 u and halves the rest; the reciprocal 2 u
                (no error at all where the 1e-12 clamp decides); the dot product E u sum |w e|; the
                product and the sum with the bias one u each.
  var_embed_add e we + be (fused or not): u (|e we| + |sum|), rounded to the dtype; the same for the pitch;
                x + ee rounded to the dtype; + pp rounded to the dtype: four roundings, each on the
                magnitude it meets, errors carried forward.
  LayerNorm     oracle/conv.py's `_ln_bound` terms (fp32 mean, variance, rsqrt, scale, shift; propagation
                of an input error through 1 / sigma), LN1 materialised in the dtype before LN2.
None of the constants is fitted to a GPU result and no factor sits on top.
"""
from __future__ import annotations

import numpy as np

from .acoustic import durations_from_log, softmax as _softmax
from .attention import round_to
from .conv import F16_FLOOR, U32, UNIT, _ln32, _ln_bound

TINY = 2.0 ** -126
SILU_LIP = 1.1     # max |d/dx x sigmoid(x)| = 1.0998

GLU_DEFECTS = ("off_centre", "reverse_taps", "swap_halves", "no_bias", "no_silu", "halo_neighbour", "drop_tile_edge_row",
               "drop_last_block")
SOFTMAX_DEFECTS = ("shift_off_by_one", "no_max", "mask_at_sk", "no_scale")
LN_DEFECTS = ("var_cm1", "no_eps", "one_pass")
LNG_DEFECTS = ("neighbour_gain",)
SPK_DEFECTS = ("no_norm", "norm_first_256")
VAR_DEFECTS = ("swap_tables",)
DUR_DEFECTS = ("round_half_up", "no_minus_one", "all_zero_batch_wide", "count_past_len", "map_zero_duration")


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def out_round(v, e, dt):
    """Error after rounding a value known to e (reference v) to dtype dt."""
    return e + UNIT[dt] * (np.abs(v) + e) + (F16_FLOOR if dt == "f16" else 0.0)


def exp_rel(x):
    return 2 * U32 * (1 + np.abs(x))


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def sigmoid_err(x, s):
    return s * (1 - s) * exp_rel(x) + 3 * U32 * s + TINY


def _rnd32(q, dt):
    return round_to(q, dt).astype(np.float32)


# ------------------------------------------------------------------------------------ exact ops
def embed_expected(dt, ids, lens, Tm, table, scale):
    """[B, Tm, D]: every row written, zeros from min(lens, N) on; ids clamped to the table."""
    B, N = ids.shape
    V, D = table.shape
    out = np.zeros((B, Tm, D))
    for b in range(B):
        L = min(int(lens[b]), N, Tm)
        rows = np.asarray(table, np.float32)[np.clip(ids[b, :L], 0, V - 1)] * np.float32(scale)
        out[b, :L] = round_to(rows, dt)
    return out


def regulate_expected(dt, enc, tokmap, frames, Tout, scale, sentinel):
    """[B, Tout, D]: frames rows per utterance (token < 0: zeros), the rest the sentinel."""
    B, N, D = enc.shape
    out = np.full((B, Tout, D), float(sentinel))
    for b in range(B):
        tok = tokmap[b, :frames]
        rows = np.asarray(enc[b], np.float32)[np.clip(tok, 0, N - 1)] * np.float32(scale)
        out[b, :frames] = np.where((tok >= 0)[:, None], round_to(rows, dt), 0.0)
    return out


def pos_bias_expected(dt, qkv, D, u, v):
    q = np.asarray(qkv[:, :D], np.float32)
    return round_to(q + np.asarray(u, np.float32), dt), round_to(q + np.asarray(v, np.float32), dt)


def transpose_v_expected(qkv, lens, D, H, Sk, sentinel=None):
    """[B, H, dk, Sk]: key j < min(len, Tm, Sk) copied, the rest zeros."""
    B, Tm = qkv.shape[:2]
    dk = D // H
    out = np.zeros((B, H, dk, Sk))
    for b in range(B):
        L = min(int(lens[b]), Tm, Sk)
        out[b, :, :, :L] = qkv[b, :L, 2 * D:].reshape(L, H, dk).transpose(1, 2, 0)
    return out


def mel_out_expected(x, mel_lens, Tcap):
    B, Tin, C = x.shape
    out = np.zeros((B, Tcap, C))
    for b in range(B):
        L = min(int(mel_lens[b]), Tcap)
        out[b, :L] = x[b, :L]
    return out


def durations_expected(logd, lens, N, Tcap, override_d=None, speed=1.0, defect=None):
    """-> (dur [B, N], mel_lens [B], tokmap [B, Tcap]) as include/tts_hip.h states them; the predicted
    form through oracle.acoustic.durations_from_log.  defect: one of DUR_DEFECTS (a wrong kernel)."""
    B = len(lens)
    dur = np.zeros((B, N), np.int64)
    for b in range(B):
        L = N if defect == "count_past_len" else max(min(int(lens[b]), N), 0)
        if override_d is not None:
            d = np.maximum(np.asarray(override_d[b, :L], np.int64), 0)
        elif defect is None:   # (speed and the all-zero rule included)
            dur[b, :L] = durations_from_log(np.asarray(logd[b, :L], np.float32), speed)
            continue
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(np.asarray(logd[b, :L], np.float32)) - np.float32(0 if defect == "no_minus_one" else 1)
                e = np.nan_to_num(e, nan=0.0, posinf=0.0)
            d = np.maximum(np.floor(e + np.float32(0.5)) if defect == "round_half_up" else np.round(e), 0).astype(np.int64)
        if speed != 1.0:
            t = d.astype(np.float32) * np.float32(speed)
            d = (np.floor(t + np.float32(0.5)) if defect == "round_half_up" else np.round(t)).astype(np.int64)
        dur[b, :L] = d
    for b in range(B):
        L = max(min(int(lens[b]), N), 0)
        zero = dur.sum() == 0 if defect == "all_zero_batch_wide" else dur[b].sum() == 0
        if zero and L:
            dur[b, :L] = 1
    mel = np.minimum(dur.sum(1), Tcap)
    tokmap = np.full((B, Tcap), -1, np.int64)
    for b in range(B):
        m = np.repeat(np.arange(N), dur[b])[:Tcap]
        if defect == "map_zero_duration":      # an upper-bound search that stops one token early on a tie
            cum = np.cumsum(dur[b])
            m = np.searchsorted(cum, np.arange(mel[b]), side="left").clip(0, N - 1)
        tokmap[b, :len(m)] = m
    return dur, mel, tokmap


def duration_margin(logd, lens, speed=1.0):
    """Smallest distance of exp(x) - 1 (valid tokens, float64) from a half-integer: what decides that
    rint of the fp32 value cannot fall the other way."""
    best = np.inf
    for b, L in enumerate(lens):
        v = np.exp(np.asarray(logd[b, :max(int(L), 0)], np.float64)) - 1.0
        if v.size:
            best = min(best, float(np.abs(v - np.floor(v) - 0.5).min()))
    return best


# ------------------------------------------------------------------------------------ glu_dwconv
def glu_problem(dt, a, lens, w, bias):
    """a [B, Tm, 2 D] float64 holding values of dt (rows past each length: anything), w [D, k], bias [D]."""
    return dict(dt=dt, a=np.asarray(a, np.float64), lens=tuple(int(v) for v in lens), w=f32(w), bias=f32(bias))


def _taps(g, w, L, k):
    """sum_j w[:, j] * g[t + j - pad] over the zero-padded g [L, D] -> [L, D]."""
    pad = (k - 1) // 2
    gp = np.zeros((L + k - 1, g.shape[1]), g.dtype)
    gp[pad:pad + L] = g
    acc = np.zeros_like(g)
    for j in range(k):
        acc = acc + gp[j:j + L] * w[:, j].astype(g.dtype)
    return acc


def glu_reference(P, b):
    L, D = P["lens"][b], P["w"].shape[0]
    k = P["w"].shape[1]
    x, gt = P["a"][b, :L, :D], P["a"][b, :L, D:]
    s = sigmoid(gt)
    g = x * s
    acc = _taps(g, P["w"], L, k) + P["bias"]
    A = _taps(np.abs(g), np.abs(P["w"]), L, k) + np.abs(P["bias"])
    sa = sigmoid(acc)
    return dict(x=x, gt=gt, s=s, g=g, acc=acc, A=A, sa=sa, y=acc * sa)


def glu_bound(P, b, ref=None):
    ref = glu_reference(P, b) if ref is None else ref
    L, k = P["lens"][b], P["w"].shape[1]
    dg = np.abs(ref["x"]) * sigmoid_err(ref["gt"], ref["s"]) + U32 * np.abs(ref["g"])
    dacc = _taps(dg, np.abs(P["w"]), L, k) + (k + 1) * U32 * ref["A"]
    dy = SILU_LIP * dacc + np.abs(ref["acc"]) * sigmoid_err(ref["acc"], ref["sa"]) + U32 * np.abs(ref["y"])
    return out_round(ref["y"], dy, P["dt"])


def glu_replay(P, b, defect=None, sentinel=0.0):
    assert defect is None or defect in GLU_DEFECTS, defect
    L, (D, k), dt = P["lens"][b], P["w"].shape, P["dt"]
    a32 = np.asarray(P["a"], np.float32)
    w = np.asarray(P["w"], np.float32)
    if defect == "reverse_taps":
        w = w[:, ::-1]
    sig = lambda v: (np.float32(1) / (np.float32(1) + np.exp(-v))).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        xs, gs = (a32[..., D:], a32[..., :D]) if defect == "swap_halves" else (a32[..., :D], a32[..., D:])
        g_all = (xs * sig(gs)).astype(np.float32)           # [B, Tm, D]
        pad = (k - 1) // 2 - (1 if defect == "off_centre" else 0)
        Tm = a32.shape[1]
        flat = g_all.reshape(-1, D)
        acc = np.zeros((L, D), np.float32)
        for j in range(k):
            t = np.arange(L) + j - pad
            if defect == "halo_neighbour":
                n = t + b * Tm
                ok = (n >= 0) & (n < flat.shape[0])
                rows = np.where(ok[:, None], flat[np.clip(n, 0, flat.shape[0] - 1)], np.float32(0))
            else:
                ok = (t >= 0) & (t < L)
                rows = np.where(ok[:, None], g_all[b][np.clip(t, 0, Tm - 1)], np.float32(0))
            acc = acc + w[:, j] * rows
        if defect != "no_bias":
            acc = acc + np.asarray(P["bias"], np.float32)
        y = acc if defect == "no_silu" else (acc / (np.float32(1) + np.exp(-acc))).astype(np.float32)
    y = round_to(y, dt).copy()
    if defect == "drop_tile_edge_row":
        y[128::128] = sentinel
    if defect == "drop_last_block" and D % 64:
        y[:, 64 * (D // 64):] = sentinel
    return y


# ----------------------------------------------------------------------------------- rel_softmax
def softmax_problem(dt, ac, bd, lens, Tm, scale):
    """ac [B, H, Tm, Sac], bd [B, H, Tm, Sbd] float64 of dt."""
    return dict(dt=dt, ac=np.asarray(ac, np.float64), bd=np.asarray(bd, np.float64), lens=tuple(int(v) for v in lens), Tm=Tm,
                scale=float(np.float32(scale)))


def _shifted(bd, Tm, L, off=0):
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    return bd[:, i, Tm - 1 + off - i + j]


def softmax_reference(P, b):
    """Valid rows and keys of utterance b: dict(s, p) [H, L, L]."""
    L, Tm = P["lens"][b], P["Tm"]
    s = (P["ac"][b][:, :L, :L] + _shifted(P["bd"][b], Tm, L)) * P["scale"]
    return dict(s=s, p=_softmax(s, -1))


def softmax_bound(P, b, ref=None):
    ref = softmax_reference(P, b) if ref is None else ref
    s, p = ref["s"], ref["p"]
    L = s.shape[-1]
    a = s - s.max(-1, keepdims=True)
    r = 2 * U32 * np.abs(s) + U32 * np.abs(a) + exp_rel(a)
    R = (p * r).sum(-1, keepdims=True)
    return out_round(p, p * (r + R + (L + 2) * U32) + TINY, P["dt"])


def softmax_replay(P, b, defect=None, Sk=None):
    """[H, L, Sk or L] float64: the kernel's arithmetic in float32 on the valid rows."""
    assert defect is None or defect in SOFTMAX_DEFECTS, defect
    L, Tm, dt = P["lens"][b], P["Tm"], P["dt"]
    Sk = L if Sk is None else Sk
    nk = min(Sk, P["ac"].shape[-1], Tm) if defect == "mask_at_sk" else L
    ac = np.asarray(P["ac"][b], np.float32)[:, :L, :nk]
    bd = np.asarray(P["bd"][b], np.float32)
    i = np.arange(L)[:, None]
    j = np.arange(nk)[None, :]
    idx = np.clip(Tm - 1 + (1 if defect == "shift_off_by_one" else 0) - i + j, 0, bd.shape[-1] - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        s = ac + bd[:, i, idx]
        if defect != "no_scale":
            s = s * np.float32(P["scale"])
        mx = np.float32(0) if defect == "no_max" else s.max(-1, keepdims=True)
        e = np.exp(s - mx).astype(np.float32)
        p = e * (np.float32(1) / e.sum(-1, keepdims=True, dtype=np.float32))
    out = np.zeros(p.shape[:2] + (Sk,))
    out[..., :nk] = round_to(p, dt)
    return out


# ------------------------------------------------------------------------------------- LayerNorm
def ln_reference(x, g1, b1, eps, g2=None, b2=None):
    """rows x [R, C] float64 -> dict(ln1, ln, var1, z1[, var2, z2])."""
    def stats(q):
        mu = q.mean(-1, keepdims=True)
        var = ((q - mu) ** 2).mean(-1, keepdims=True)
        return var, (q - mu) / np.sqrt(var + eps)
    out = {}
    out["var1"], out["z1"] = stats(x)
    out["ln1"] = out["ln"] = out["z1"] * g1 + b1
    if g2 is not None:
        out["var2"], out["z2"] = stats(out["ln1"])
        out["ln"] = out["z2"] * g2 + b2
    return out


def ln_bound(x, ref, dt, g1, b1, eps, g2=None, b2=None):
    C = x.shape[-1]
    e1 = out_round(ref["ln1"], _ln_bound(x, np.zeros_like(x), g1, b1, ref["var1"], ref["z1"], eps, C), dt)
    if g2 is None:
        return e1
    return out_round(ref["ln"], _ln_bound(ref["ln1"], e1, g2, b2, ref["var2"], ref["z2"], eps, C), dt)


def _ln32_one_pass(v, g, b, eps):
    v = np.asarray(v, np.float32)
    C = np.float32(v.shape[-1])
    mu = v.sum(-1, keepdims=True, dtype=np.float32) / C
    var = (v * v).sum(-1, keepdims=True, dtype=np.float32) / C - mu * mu
    return ((v - mu) / np.sqrt(np.maximum(var, 0) + np.float32(eps))).astype(np.float32) * np.asarray(g, np.float32) + np.asarray(b, np.float32)


def ln_replay(x, dt, g1, b1, eps, g2=None, b2=None, defect=None):
    assert defect is None or defect in LN_DEFECTS, defect
    e = 0.0 if defect == "no_eps" else eps
    one = (lambda q, g, b: _ln32_one_pass(q, g, b, e)) if defect == "one_pass" else \
        (lambda q, g, b: _ln32(q, g, b, e, 1 if defect == "var_cm1" else 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = _rnd32(one(x, g1, b1), dt)
        if g2 is not None:
            y = _rnd32(one(y, g2, b2), dt)
    return y.astype(np.float64)


def lng_replay(x, dt, C, gains, biases, eps, defect=None):
    """x [R, ld] -> the first len(gains) * C columns normalised group by group."""
    assert defect is None or defect in LNG_DEFECTS, defect
    G = len(gains)
    out = np.array(x, np.float64)
    for i in range(G):
        src = (i + 1) % G if defect == "neighbour_gain" else i
        out[:, i * C:(i + 1) * C] = ln_replay(x[:, i * C:(i + 1) * C], dt, gains[src], biases[i], eps)
    return out


# -------------------------------------------------------------------------------------- spk_bias
def spk_reference(e, We, bias):
    """e [E], We [D, E], bias [D] (fp32 values) -> dict(y, n, acc, A)."""
    n = float(np.sqrt((e ** 2).sum()))
    acc = We @ e
    inv = 1.0 / max(n, float(np.float32(1e-12)))
    return dict(n=n, acc=acc, A=np.abs(We) @ np.abs(e), inv=inv, y=bias + acc * inv)


def spk_bound(e, We, bias, dt, ref=None):
    ref = spk_reference(e, We, bias) if ref is None else ref
    E = e.shape[0]
    clamp = float(np.float32(1e-12))
    rel_n = ((-(-E // 256) + 9) * U32 / 2 + 2 * U32) if ref["n"] > clamp else 0.0
    # (a norm within rel_n of the clamp may fall on either side of it: the two branches then differ by rel_n too)
    t = np.abs(ref["acc"]) * ref["inv"]
    d = ref["inv"] * E * U32 * ref["A"] + t * (rel_n + 2 * U32 + U32) + U32 * np.abs(ref["y"])
    return out_round(ref["y"], d, dt)


def spk_replay(e, We, bias, dt, defect=None):
    assert defect is None or defect in SPK_DEFECTS, defect
    e32, W32 = np.asarray(e, np.float32), np.asarray(We, np.float32)
    part = e32[:256] if defect == "norm_first_256" else e32
    n = np.sqrt((part * part).sum(dtype=np.float32))
    inv = np.float32(1) if defect == "no_norm" else np.float32(1) / max(n, np.float32(1e-12))
    return round_to(np.asarray(bias, np.float32) + (W32 @ e32) * inv, dt)


# --------------------------------------------------------------------------------- var_embed_add
def var_reference(x, e, we, be, p, wp, bp):
    """x [R, D] of the dtype; e / p [R], tables [D] fp32 values."""
    ee = e[:, None] * we + be
    pp = p[:, None] * wp + bp
    return dict(ee=ee, pp=pp, y1=x + ee, y=x + ee + pp, Ae=np.abs(e[:, None] * we) + np.abs(be),
                Ap=np.abs(p[:, None] * wp) + np.abs(bp))


def var_bound(x, ref, dt):
    de = out_round(ref["ee"], U32 * (ref["Ae"] + np.abs(ref["ee"])), dt)
    dp = out_round(ref["pp"], U32 * (ref["Ap"] + np.abs(ref["pp"])), dt)
    d1 = out_round(ref["y1"], de + U32 * (np.abs(ref["y1"]) + de), dt)
    return out_round(ref["y"], d1 + dp + U32 * (np.abs(ref["y"]) + d1 + dp), dt)


def var_replay(x, e, we, be, p, wp, bp, dt, defect=None):
    assert defect is None or defect in VAR_DEFECTS, defect
    if defect == "swap_tables":
        we, be, wp, bp = wp, bp, we, be
    c = lambda a: np.asarray(a, np.float32)
    ee = _rnd32(c(e)[:, None] * c(we) + c(be), dt)
    pp = _rnd32(c(p)[:, None] * c(wp) + c(bp), dt)
    return round_to(_rnd32(c(x) + ee, dt) + pp, dt)
