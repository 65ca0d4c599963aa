"""ORACLE (test infrastructure only) -- the relative-position attention of one utterance in
float64, straight from the formula at the top of csrc/attention.hip:

    S[h][i][j] = (Qu[i][h] . k[j][h] + Qv[i][h] . R[i - j][h]) * scale,  Qu = q + pos_u, Qv = q + pos_v
    O[i][h]    = softmax_j(S[h][i]) . v[:, h]

q / k / v are [L, H, dk] arrays holding values of the working dtype; R is the position table as
the engine lays it out, [2 rmax, H, dk] with row r <-> rel = rmax - 1 - r.  Qu and Qv are formed
as the kernels define them -- one float32 add, one round-to-nearest-even to the working dtype --
so operand rounding stays out of every comparison; everything after that is float64.

Besides the plain form there are: a rounded variant (P = 2^(s - m) and the output rounded to the
dtype; for "f32" the whole formula in NumPy float32), which is the error model the parity bounds
are taken from; `lazy_moves`, the replay of the kernels' lazy online-softmax rule on a score
matrix; and `flash`, the 32-key-step online softmax itself in float64 with optional defects, which
the power tests inject to show the bounds reject them.
"""
from __future__ import annotations

import math

import numpy as np

STEP = 32      # keys per online-softmax step (AT_BK)
LAZY = 8.0     # a row's reference max moves when a step's max exceeds it by more than this (log2 units)
LOG2E = 1.4426950408889634

DEFECTS = ("rel_off_by_one", "no_rescale", "rescale_o_only", "drop_step", "mask_last", "admit_len")


def round_to(x, dtype):
    """x rounded to the working dtype (round to nearest even), returned as float64."""
    x = np.asarray(x)
    if dtype == "f64":
        return x.astype(np.float64)
    if dtype in ("f32", "split"):
        return x.astype(np.float32).astype(np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)
    if dtype == "bf16":
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
        u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
        return u.view(np.float32).astype(np.float64)
    raise ValueError(dtype)


def biased_queries(q, pos_u, pos_v, dtype):
    """(Qu, Qv) [L, H, dk] float64: float32 add, one rounding to the dtype ("f64": no rounding at
    all, the form pinned to oracle.acoustic.rel_mha)."""
    if dtype == "f64":
        q = np.asarray(q, np.float64)
        return q + np.asarray(pos_u, np.float64)[None], q + np.asarray(pos_v, np.float64)[None]
    q32 = np.asarray(q, np.float32)
    return (round_to(q32 + np.asarray(pos_u, np.float32)[None], dtype),
            round_to(q32 + np.asarray(pos_v, np.float32)[None], dtype))


def rel_index(L, rmax, shift=0):
    """Table row of (i, j): rel = i - j (+ shift, the off-by-one defect) -> rmax - 1 - rel."""
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    return np.clip(rmax - 1 - (i - j + shift), 0, 2 * rmax - 1)


def scores(q, k, R, pos_u, pos_v, rmax, dtype, scale=None, shift=0, ftype=np.float64):
    """S [H, L, L] (softmax logits, natural units) in `ftype` arithmetic."""
    L, H, dk = q.shape
    scale = 1.0 / math.sqrt(dk) if scale is None else scale
    qu, qv = biased_queries(q, pos_u, pos_v, dtype)
    qu, qv = qu.astype(ftype).transpose(1, 0, 2), qv.astype(ftype).transpose(1, 0, 2)
    ac = qu @ np.asarray(k, ftype).transpose(1, 2, 0)
    bd_full = qv @ np.asarray(R, ftype).transpose(1, 2, 0)          # [H, L, 2 rmax]
    bd = bd_full[:, np.arange(L)[:, None], rel_index(L, rmax, shift)]
    return (ac + bd) * ftype(scale)


def _softmax_pv(s, v, ftype=np.float64):
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    return (e @ np.asarray(v, ftype).transpose(1, 0, 2)) / e.sum(-1, keepdims=True)   # [H, L, dk]


def rel_attention(q, k, v, R, pos_u, pos_v, rmax, dtype, scale=None):
    """The attention output [L, H, dk] in float64 (operands as given, Qu / Qv rounded to dtype)."""
    s = scores(q, k, R, pos_u, pos_v, rmax, dtype, scale)
    return _softmax_pv(s, v).transpose(1, 0, 2)


def rel_attention_rounded(q, k, v, R, pos_u, pos_v, rmax, dtype, scale=None):
    """The rounding model of a kernel in `dtype`, on the same rounded operands.
    f16 / bf16: float64 scores, P = 2^(s - m) rounded to the dtype (the row sum taken over the
    rounded P, as the kernel normalises), the output rounded to the dtype.
    f32 / split: the same formula in plain NumPy float32."""
    if dtype in ("f32", "split"):
        s = scores(q, k, R, pos_u, pos_v, rmax, dtype, scale, ftype=np.float32)
        return _softmax_pv(s, v, np.float32).transpose(1, 0, 2).astype(np.float64)
    s2 = scores(q, k, R, pos_u, pos_v, rmax, dtype, scale) * LOG2E
    p = round_to(np.exp2(s2 - s2.max(-1, keepdims=True)), dtype)
    o = (p @ np.asarray(v, np.float64).transpose(1, 0, 2)) / p.sum(-1, keepdims=True)
    return round_to(o.transpose(1, 0, 2), dtype)


def lazy_moves(s, lazy=LAZY):
    """Replay of the kernels' `grow` rule on scores s [..., L, L] (natural units): over 32-key
    steps a row's reference max moves to the step's max when that exceeds it by more than `lazy`
    log2 units.  -> int array [..., L]: moves after the row's first key step (which always sets
    the reference)."""
    s2 = np.asarray(s, np.float64) * LOG2E
    m = s2[..., :STEP].max(-1)
    n = np.zeros(m.shape, np.int64)
    for j0 in range(STEP, s2.shape[-1], STEP):
        mloc = s2[..., j0:j0 + STEP].max(-1)
        grow = mloc > m + lazy
        n += grow
        m = np.where(grow, mloc, m)
    return n


def flash(s, v, lazy=LAZY, defect=None):
    """The kernels' online softmax over 32-key steps in float64: s [H, L, Lk] (natural units),
    v [Lk, H, dk] -> O [L, H, dk].  lazy = 0 is the eager form of the fp32 kernel.  Without a
    defect this equals the direct softmax up to float64 rounding.  defect:
      no_rescale      alpha forced to 1 on rows that move (neither O nor l rescaled)
      rescale_o_only  alpha applied to O but not to l
      drop_step       the last 32-key step (whole or partial) is skipped; a one-step row is left whole"""
    s2 = np.asarray(s, np.float64) * LOG2E
    H, L, Lk = s2.shape
    vt = np.asarray(v, np.float64).transpose(1, 0, 2)
    m = np.full((H, L), -np.inf)
    l = np.zeros((H, L))
    o = np.zeros((H, L, vt.shape[-1]))
    nsteps = (Lk + STEP - 1) // STEP
    for st, j0 in enumerate(range(0, Lk, STEP)):
        if defect == "drop_step" and st == nsteps - 1 and st > 0:
            continue
        blk = s2[:, :, j0:j0 + STEP]
        mloc = blk.max(-1)
        grow = mloc > m + lazy
        m_new = np.where(grow, mloc, m)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isinf(m), 0.0, np.exp2(m - m_new))
        moved = grow & ~np.isinf(m)
        a_o = np.where(moved, 1.0, alpha) if defect == "no_rescale" else alpha
        a_l = np.where(moved, 1.0, alpha) if defect in ("no_rescale", "rescale_o_only") else alpha
        p = np.exp2(blk - m_new[..., None])
        l = l * a_l + p.sum(-1)
        o = o * a_o[..., None] + p @ vt[:, j0:j0 + STEP]
        m = m_new
    with np.errstate(invalid="ignore"):   # (a row left without a key by a defect: NaN, as a kernel's 0 / 0)
        return (o / l[..., None]).transpose(1, 0, 2)


def rel_attention_defect(defect, q, k, v, R, pos_u, pos_v, rmax, dtype, scale=None, lazy=LAZY, garbage=1e4):
    """The float64 attention with one defect of DEFECTS injected (what a subtly wrong kernel
    would compute): [L, H, dk]."""
    L = q.shape[0]
    shift = 1 if defect == "rel_off_by_one" else 0
    s = scores(q, k, R, pos_u, pos_v, rmax, dtype, scale, shift=shift)
    if defect == "mask_last":
        s, v = s[:, :, :L - 1], v[:L - 1]
    elif defect == "admit_len":
        # one more key: the row past the utterance, filled with the caller's garbage; its relative
        # position is one further than key L - 1's
        g = np.full((1,) + q.shape[1:], garbage)
        qu, qv = biased_queries(q, pos_u, pos_v, dtype)
        sc = 1.0 / math.sqrt(q.shape[2]) if scale is None else scale
        rows = np.clip(rmax - 1 - (np.arange(L) - L), 0, 2 * rmax - 1)
        extra = (np.einsum("ihd,hd->hi", qu, g[0]) + np.einsum("ihd,ihd->hi", qv, np.asarray(R, np.float64)[rows])) * sc
        s, v = np.concatenate([s, extra[..., None]], -1), np.concatenate([np.asarray(v, np.float64), g], 0)
    return flash(s, v, lazy, defect if defect in ("no_rescale", "rescale_o_only", "drop_step") else None)
