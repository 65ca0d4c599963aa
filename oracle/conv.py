"""ORACLE (test infrastructure only) -- one implicit-GEMM conv launch in float64, its epilogue and
optional LayerNorms exactly as csrc/kernels.h writes them, an error bound per output element taken
from the reference alone, and a replay of the kernels' arithmetic that carries injected defects.

    acc[n][m] = sum_{t, c} w[m][c][t] * act_in(x[n + t*dil - pad][c])       rows outside [0, len): 0
    y         = ((alpha * (acc + bias)) -> act) + r1 + r2, then * out_scale
    ln        = LN2?(LN1(y)),   lin = LN1(y) . lin_w + lin_b

A problem is a dict (`problem()`): operands already rounded to the working dtype (`round_to`), so
operand rounding stays out of every comparison; act_in is formed as the kernels define it (below).
Everything is per utterance: `reference(P, b)`, `bound(P, form, b)`, `replay(P, form, b, defect=)`.

Forms: "f16" / "bf16" (16-bit operands, exact products, fp32 accumulation, one rounding of the
result to the dtype -- two when a residual or an output scale follows the activation: conv_xres
stages the activated value in the dtype and adds the residuals to that), "f32" (fp32 MFMA) and
"split" (fp32 operands as two f16 halves, three f16 MFMAs per product: conv_split.hip).

The error model of `bound` (u = 2^-24, uT the unit roundoff of the output dtype; A = sum |x||w| + |bias|
in float64 over the K = taps * Cin products; S split-K slices):
  accumulation     (P + S + 8) u A, P = K products (3K in the split form): the worst case of any
                   summation order, so nothing is assumed about the MFMA's internal order
  split operands   x = xh + xl + ex with |ex| <= 2^-22 |x| while xl is a normal f16, and likewise w:
                   x w - (xh wh + xh wl + xl wh) = xl wl + ex w + x ew + ..., at most
                   C_SPLIT 2^-22 |x||w| with C_SPLIT = 3 (1 + 2^-10) derived (the NumPy emulation below
                   measures 0.26 2^-22 A at most on the normal pattern: test_conv_op_cpu.py prints it);
                   a product whose activation's low half is a subnormal f16 (|x - xh| < 2^-14) adds the
                   absolute floor 2^-25 |w|, one whose scaled weight's low half is 2^-25 2^-s |x|
  epilogue         one u per fp32 operation on the magnitudes it touches; activations are 1-Lipschitz
  output           uT (|y| + e) at the reference value (+ 2^-25 for f16's subnormal spacing)
  LayerNorm        |dLN_i| <= |g_i| (2 + |z_i|) d / sqrt(var + eps), d = max_i |dy_i| plus the fp32 mean's
                   (C + 4) u max|y|; then (C + 12) u (|g_i z_i| + |b_i|) for the fp32 variance, rsqrt,
                   scale and shift; LN1 is materialised in the dtype before LN2 / the Linear
  the whole model times FACTOR = 2 (the MFMA's undocumented internal order) and no more.
None of the constants is fitted to a GPU result.
"""
from __future__ import annotations

import math

import numpy as np

from .attention import round_to

U32 = 2.0 ** -24
UNIT = {"f32": 2.0 ** -24, "split": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
C_SPLIT = 3.0 * (1 + 2.0 ** -10)   # derived (module docstring); the CPU emulation measures < 1
FACTOR = 2.0
F16_TINY = 2.0 ** -14              # smallest normal f16: a low half below it is a subnormal
F16_FLOOR = 2.0 ** -25             # half the subnormal spacing

DEFECTS = ("drop_tap", "reverse_taps", "drop_last_group", "halo_neighbour", "no_unscale", "drop_lo_hi",
           "splitk_drop_last", "bias_per_slice", "ln_var_cm1", "ln_no_eps", "ln_skip_ln2", "unwritten_tail")


def storage(form):
    return "f32" if form == "split" else form


def act_in(x, slope, form):
    """LeakyReLU on load as each kernel family forms it (x holds values of the dtype): f16 runs
    packed, max(x, x * f16(slope)) rounded to f16; bf16 multiplies by the fp32 slope and rounds to
    bf16; fp32 (and the split form, before it splits) multiplies in fp32."""
    x = np.asarray(x, np.float64)
    if slope == 1.0:
        return x
    dt = storage(form)
    s = float(np.float16(slope)) if dt == "f16" else float(np.float32(slope))
    return np.where(x >= 0, x, round_to(x * s, dt))


def im2col(xv, k, dil, pad):
    """xv [L, Cin] (the utterance's valid rows) -> [L, k * Cin], column t * Cin + c = x[n + t dil - pad][c]."""
    L, ci = xv.shape
    xp = np.zeros((L + (k - 1) * dil, ci), xv.dtype)
    xp[pad:pad + L] = xv
    return np.concatenate([xp[t * dil:t * dil + L] for t in range(k)], 1)


def wmat(w):
    """nn.Conv1d weight [M, Cin, k] -> [k * Cin, M] in im2col's column order."""
    M, ci, k = w.shape
    return np.ascontiguousarray(np.transpose(w, (2, 1, 0)).reshape(k * ci, M))


def layer_norm(y, g, b, eps, ddof=0):
    y = np.asarray(y, np.float64)
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).sum(-1, keepdims=True) / (y.shape[-1] - ddof)
    return (y - mu) / np.sqrt(var + eps) * g + b


def lrelu(v, slope):
    return np.where(v >= 0, v, v * slope)


def problem(form, x, lens, w, bias, dil=1, pad=0, in_slope=1.0, act=False, out_slope=0.0, alpha=1.0, out_scale=1.0,
            r1=None, r2=None, ln=None):
    """x [B, rows, Cin], r1 / r2 [B, rows, M] float64 holding values of the dtype (rows past each
    length: anything), w [M, Cin, k] of the dtype, bias fp32 values; act: LeakyReLU(out_slope) as
    act_out; ln: None or dict(g1, b1, eps, g2=None, b2=None, lin_w=None, lin_b=0.0) of fp32 values."""
    f32 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)
    if ln is not None:
        ln = dict(ln)
        for key in ("g1", "b1", "g2", "b2", "lin_w"):
            ln[key] = f32(ln.get(key))
        ln["lin_b"] = float(np.float32(ln.get("lin_b", 0.0)))
        ln["eps"] = float(np.float32(ln["eps"]))
    return dict(form=form, x=np.asarray(x, np.float64), lens=tuple(int(v) for v in lens), w=np.asarray(w, np.float64),
                bias=f32(bias), dil=dil, pad=pad, in_slope=float(in_slope), act=bool(act),
                out_slope=float(np.float32(out_slope)), alpha=float(np.float32(alpha)),
                out_scale=float(np.float32(out_scale)), r1=r1, r2=r2, ln=ln)


def _cols(P, b):
    L = P["lens"][b]
    k = P["w"].shape[2]
    return im2col(act_in(P["x"][b, :L], P["in_slope"], P["form"]), k, P["dil"], P["pad"])


def sums(P, b, floors=False):
    """The K-long sums of utterance b that every epilogue shares -> dict(acc, Axw = sum |x||w|[, floor_x,
    floor_w: the split form's absolute floors (module docstring)])."""
    cols, W = _cols(P, b), wmat(P["w"])
    out = dict(acc=cols @ W, Axw=np.abs(cols) @ np.abs(W))
    if floors:
        s = split_scale(P["w"])
        sub_x = (np.abs(cols - halves(cols)[0]) < F16_TINY).astype(np.float64)
        Ws = W * 2.0 ** s
        sub_w = (np.abs(Ws - halves(Ws)[0]) < F16_TINY).astype(np.float64)
        out["floor_x"] = F16_FLOOR * (sub_x @ np.abs(W))
        out["floor_w"] = F16_FLOOR * 2.0 ** -s * (np.abs(cols) @ sub_w)
    return out


def reference(P, b, base=None):
    """Utterance b in float64 -> dict(acc, A, t, a, v, y[, ln1, ln, lin, var1, z1, var2, z2], base);
    base: sums(P, b), when the caller shares it between epilogues."""
    L = P["lens"][b]
    base = sums(P, b, floors=P["form"] == "split") if base is None else base
    acc = base["acc"]
    A = base["Axw"] + np.abs(P["bias"])
    t = P["alpha"] * (acc + P["bias"])
    a = lrelu(t, P["out_slope"]) if P["act"] else t
    v = a.copy()
    for r in (P["r1"], P["r2"]):
        if r is not None:
            v = v + r[b, :L]
    y = v * P["out_scale"]
    out = dict(acc=acc, A=A, t=t, a=a, v=v, y=y, base=base)
    ln = P["ln"]
    if ln is not None:
        def stats(q):
            mu = q.mean(-1, keepdims=True)
            var = ((q - mu) ** 2).mean(-1, keepdims=True)
            return var, (q - mu) / np.sqrt(var + ln["eps"])
        out["var1"], out["z1"] = stats(y)
        out["ln1"] = out["ln"] = layer_norm(y, ln["g1"], ln["b1"], ln["eps"])
        if ln["g2"] is not None:
            out["var2"], out["z2"] = stats(out["ln1"])
            out["ln"] = layer_norm(out["ln1"], ln["g2"], ln["b2"], ln["eps"])
        if ln["lin_w"] is not None:
            out["lin"] = out["ln1"] @ ln["lin_w"] + ln["lin_b"]
    return out


def split_scale(w):
    """frag_pack_split's exponent s: 2^s puts max|w| in [2^14, 2^15)."""
    mx = float(np.abs(w).max())
    e = math.frexp(mx)[1] if mx > 0 else 0
    return max(-24, min(60, 15 - e))


def halves(v):
    """v (float64 holding fp32 values) -> (hi, lo) f16 values as float64, as the kernels split:
    hi = f16(v), lo = f16(fp32(v - hi))."""
    with np.errstate(over="ignore"):
        hi = np.asarray(v, np.float32).astype(np.float16)
        lo = (np.asarray(v, np.float32) - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _ln_bound(q, dq, g, bb, var, z, eps, C):
    """Propagated + arithmetic error of one fp32 LayerNorm of rows q known to dq (elementwise)."""
    d = dq.max(-1, keepdims=True) + (C + 4) * U32 * np.abs(q).max(-1, keepdims=True)
    return np.abs(g) * (2 + np.abs(z)) * d / np.sqrt(var + eps) + (C + 12) * U32 * (np.abs(g * z) + np.abs(bb))


def bound(P, form, b, S=1, ref=None):
    """Error bounds of utterance b's outputs from the reference alone -> dict(y[, ln, lin]) with the
    shapes of reference()'s; S: split-K slices of the launch."""
    ref = reference(P, b) if ref is None else ref
    uT = UNIT[form]
    sixteen = form in ("f16", "bf16")
    floorT = F16_FLOOR if form == "f16" else 0.0
    A, K = ref["A"], P["w"].shape[1] * P["w"].shape[2]
    nprod = 3 * K if form == "split" else K
    e = (nprod + S + 8) * U32 * A
    if form == "split":
        base = ref["base"] if "floor_x" in ref["base"] else sums(P, b, floors=True)
        e = e + C_SPLIT * 2.0 ** -22 * A + base["floor_x"] + base["floor_w"]
    e = abs(P["alpha"]) * e + 2 * U32 * np.abs(ref["t"])
    if P["act"]:
        e = e + U32 * np.abs(ref["a"])
    staged = sixteen and (P["r1"] is not None or P["r2"] is not None or P["out_scale"] != 1.0)
    if staged:   # the activated value is rounded to the dtype before the residuals (conv_xres)
        e = e + uT * (np.abs(ref["a"]) + e) + floorT
    L = P["lens"][b]
    rsum = sum(np.abs(r[b, :L]) for r in (P["r1"], P["r2"]) if r is not None)
    e = e + 2 * U32 * (np.abs(ref["a"]) + rsum)
    e = abs(P["out_scale"]) * e + U32 * np.abs(ref["y"])
    e = e + uT * (np.abs(ref["y"]) + e) + floorT
    out = dict(y=FACTOR * e)
    ln = P["ln"]
    if ln is not None:
        C = ref["y"].shape[1]
        e1 = _ln_bound(ref["y"], e, ln["g1"], ln["b1"], ref["var1"], ref["z1"], ln["eps"], C)
        e1 = e1 + uT * (np.abs(ref["ln1"]) + e1) + floorT     # LN1's result in the dtype
        eo = e1
        if ln["g2"] is not None:
            eo = _ln_bound(ref["ln1"], e1, ln["g2"], ln["b2"], ref["var2"], ref["z2"], ln["eps"], C)
            eo = eo + uT * (np.abs(ref["ln"]) + eo) + floorT
        out["ln"] = FACTOR * eo
        if ln["lin_w"] is not None:
            dot = np.abs(ref["ln1"]) @ np.abs(ln["lin_w"])
            out["lin"] = FACTOR * (e1 @ np.abs(ln["lin_w"]) + (C + 4) * U32 * (dot + abs(ln["lin_b"])))
    return out


# ------------------------------------------------------------------------------------ replay
def _ln32(v, g, b, eps, ddof=0):
    """The kernels' two-pass fp32 LayerNorm (ln_rows.h ln_batch) in NumPy float32."""
    v = np.asarray(v, np.float32)
    C = v.shape[-1]
    mu = v.sum(-1, keepdims=True, dtype=np.float32) * np.float32(1.0 / C)
    d = v - mu
    q = (d * d).sum(-1, keepdims=True, dtype=np.float32) * np.float32(1.0 / (C - ddof))
    rstd = (np.float32(1) / np.sqrt(q + np.float32(eps))).astype(np.float32)
    return (d * rstd) * np.asarray(g, np.float32) + np.asarray(b, np.float32)


def replay(P, form, b, defect=None, S=1, group=64, sentinel=0.0, measure=None):
    """Utterance b as a kernel of `form` computes it, in NumPy float32 / float16 (products of 16-bit
    operands are exact in fp32; the split form sums hi*hi + hi*lo + lo*hi), over S split-K slices of
    whole `group`-channel groups, with one defect of DEFECTS injected (None: the correct kernel).
    -> dict(y[, ln, lin]) float64.  sentinel: what an unwritten output holds.  measure: a dict that
    receives "split_err" = max |three-product sum - exact| / (2^-22 A) of this utterance."""
    assert defect is None or defect in DEFECTS, defect
    L, dt = P["lens"][b], storage(form)
    w = P["w"]
    M, ci, k = w.shape
    if defect == "reverse_taps":
        w = w[:, :, ::-1]
    xv = act_in(P["x"][b, :L], P["in_slope"], form)
    cols = im2col(xv, k, P["dil"], P["pad"])
    if defect == "halo_neighbour":   # rows outside the utterance come from the flat buffer: a mask failure
        flat = act_in(P["x"].reshape(-1, ci), P["in_slope"], form)
        rows = P["x"].shape[1]
        n = np.arange(L)[:, None] + np.arange(k)[None, :] * P["dil"] - P["pad"] + b * rows
        ok = (n >= 0) & (n < flat.shape[0])
        cols = np.where(ok[:, :, None], flat[np.clip(n, 0, flat.shape[0] - 1)], 0.0).reshape(L, k * ci)
    W = wmat(w)
    keep = np.ones(k * ci, bool).reshape(k, ci)
    if defect == "drop_tap":
        keep[k // 2] = False
    if defect == "drop_last_group":
        keep[:, max(ci - 64, 0):] = False
    keep = keep.reshape(-1)
    chan = np.tile(np.arange(ci), k)
    gsz = group if ci % group == 0 else ci
    ngroups = ci // gsz
    S = max(1, min(S, ngroups))
    per = -(-ngroups // S)
    acc = np.zeros((L, M), np.float32)
    bias32 = P["bias"].astype(np.float32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    s = split_scale(P["w"]) if form == "split" else 0
    if form == "split":
        xh, xl = halves(cols)
        wh, wl = halves(W * 2.0 ** s)
    nsl = S - 1 if defect == "splitk_drop_last" and S > 1 else S
    for sl in range(nsl):
        sel = keep & (chan // gsz >= sl * per) & (chan // gsz < (sl + 1) * per)
        if form == "split":
            part = f32(xh[:, sel]) @ f32(wh[sel]) + f32(xh[:, sel]) @ f32(wl[sel])
            if defect != "drop_lo_hi":
                part = part + f32(xl[:, sel]) @ f32(wh[sel])
            if defect != "no_unscale":
                part = part * np.float32(2.0 ** -s)
        else:
            part = f32(cols[:, sel]) @ f32(W[sel])
        acc = acc + part
        if defect == "bias_per_slice" and sl > 0:
            acc = acc + bias32
    if measure is not None and form == "split" and defect is None:
        ex = cols @ wmat(P["w"])
        three = (xh @ wh + xh @ wl + xl @ wh) * 2.0 ** -s
        A = np.abs(cols) @ np.abs(W)
        measure["split_err"] = float((np.abs(three - ex) / (2.0 ** -22 * A + 1e-300)).max()) if L else 0.0
    t = (acc + bias32) * np.float32(P["alpha"])
    a = np.where(t >= 0, t, t * np.float32(P["out_slope"])).astype(np.float32) if P["act"] else t
    rnd = lambda q: round_to(q, dt).astype(np.float32)
    sixteen = dt != "f32"
    res = [r for r in (P["r1"], P["r2"]) if r is not None]
    if sixteen and (res or P["out_scale"] != 1.0):
        a = rnd(a)
    v = a
    for r in res:
        v = v + f32(r[b, :L])
    y = rnd(v * np.float32(P["out_scale"]))
    if defect == "unwritten_tail":
        y = y.copy()
        y[:, 128 * (M // 128):] = sentinel
    out = dict(y=y.astype(np.float64))
    ln = P["ln"]
    if ln is not None:
        eps = 0.0 if defect == "ln_no_eps" else ln["eps"]
        ddof = 1 if defect == "ln_var_cm1" else 0
        with np.errstate(divide="ignore", invalid="ignore"):
            l1 = rnd(_ln32(y, ln["g1"], ln["b1"], eps, ddof))
            lo = l1
            if ln["g2"] is not None and defect != "ln_skip_ln2":
                lo = rnd(_ln32(l1, ln["g2"], ln["b2"], eps, ddof))
        out["ln"] = lo.astype(np.float64)
        if ln["lin_w"] is not None:
            out["lin"] = (l1 @ ln["lin_w"].astype(np.float32) + np.float32(ln["lin_b"])).astype(np.float64)
    return out
