"""Shapes, inputs, references and expected kernel forms of the op-level conv GEMM tests
(test_conv_op_cpu.py, test_conv_op_gpu.py): the smallest layers at which each form of
csrc/conv_gemm.hip / conv_split.hip / ln_rows.h can still go wrong.  NumPy only.

Cases (Cin, M, k, dil): the table of the issue that asked for these tests, plus
  j  the widest halo the packed-row split form takes (its staging registers hold 64 + 8 rows;
     cases g and h, at the envelope's 64, run the per-utterance form in fp32), and
  k  a LayerNorm over 8 channels, where a variance over C - 1 shows in every dtype.
Two things the eligibility functions decide otherwise than the table's notes: case a (M = 64) runs
the 64-channel-block kernel, which has no DMA form (that one needs 128-channel blocks: case e runs
the 1-tap DMA form once TTS_XRES_NARROW=0 takes the narrow tiles away), and cases d - f default to
the narrow 64 x 64 tiles because their grids are small; the forced-form tests reach the rest.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import conv as oc
from oracle.attention import round_to

ROWS = 192        # x_rows = y_rows: a multiple of 32 (packed-eligible) and of 64 (tiles end on utterances)
ROWS_PAD = 32     # masked rows promised after every utterance (>= every case's pad and right halo)
BATCHES = {"long": (0, 1, 65, 129, ROWS - ROWS_PAD), "short": (31, 32, 33, 63, 64)}
SENTINEL = -77.0  # pre-fill of every output (exact in bf16)
GARBAGE = 3.0     # finite stand-in for what rows past a length hold (the GPU test puts NaN / 1e30 there)
SIGMA_FLOOR = 0.25
EPS = 1e-5

#         Cin   M    k  dil  in_slope  LayerNorm
CASES = {
    "a": (64, 64, 1, 1, 1.0, None),
    "b": (96, 100, 3, 1, 1.0, None),
    "c": (128, 80, 5, 1, 1.0, None),
    "d": (192, 320, 3, 1, 1.0, "ln1"),
    "e": (384, 512, 1, 1, 1.0, "ln12"),
    "f": (256, 256, 3, 1, 1.0, "lin"),
    "g": (64, 128, 65, 1, 1.0, None),
    "h": (128, 128, 17, 4, 0.1, None),
    "i": (768, 128, 3, 1, 1.0, "ln1"),
    "j": (128, 128, 5, 2, 1.0, None),
    "k": (64, 8, 1, 1, 1.0, "ln1"),
}
# eps per case: 1e-5 as the models use, and one large enough that leaving it out shows in bf16
LN_EPS = {"d": EPS, "e": EPS, "f": EPS, "i": 0.5, "k": EPS}
EPILOGUES = {"plain": dict(), "act": dict(act=True, out_slope=0.2, alpha=0.75), "res": dict(res=True, out_scale=0.625)}
PATTERNS = ("normal", "small", "large", "wide_w")
FORMS = ("f16", "bf16", "f32", "split")          # arithmetic forms of oracle.conv
# runs of one problem on the GPU: (name, arithmetic form, layer split copy, ext fields)
RUNS = {
    "f16": ("f16", False, dict()),
    "bf16": ("bf16", False, dict()),
    "split": ("split", True, dict(rows_pad=ROWS_PAD, ws=True)),      # packed rows where eligible
    "split_utt": ("split", True, dict(rows_pad=0)),                  # per-utterance tiles
    "no_split": ("f32", True, dict(no_split=1)),                     # fp32 MFMA
    "splitk": ("f32", True, dict(no_split=1, f32_splitk=1, ws=True)),
}
PK_CONV_GEMM, PK_CONV_XRES, PK_CONV_SPLIT = 0, 1, 6


def shape(case):
    ci, M, k, dil, slope, ln = CASES[case]
    return dict(Cin=ci, M=M, k=k, dil=dil, pad=(k - 1) * dil // 2, in_slope=slope, ln=ln, K=k * ci)


def _rng(*key):
    return np.random.default_rng(int.from_bytes(repr(key).encode(), "little") % (2 ** 63))


@functools.lru_cache(maxsize=None)
def raw_inputs(case, pattern, batch):
    """fp64 inputs before rounding: x [B, ROWS, Cin], w [M, Cin, k], bias, r1, r2, LayerNorm parameters."""
    s = shape(case)
    ci, M, k = s["Cin"], s["M"], s["k"]
    B = len(BATCHES[batch])
    g = _rng(case, pattern, batch)
    x = g.standard_normal((B, ROWS, ci))
    w = g.standard_normal((M, ci, k)) / np.sqrt(k * ci)
    if pattern == "small":
        # magnitudes in [2, 4) 2^-12 whose f16 low half is a subnormal of 0.46 of the high half's
        # spacing, the sign of a channel's activations fixed; output channel 0's weights carry the
        # same signs, so that channel's sum of low halves is coherent: what a kernel that drops the
        # lo . hi term loses, against the floor of the halves' rounding alone
        sgn = np.where(g.random(ci) < 0.5, -1.0, 1.0)
        x = sgn * ((1024 + g.integers(0, 1024, x.shape)) / 512.0 + 0.46 / 512.0) * 2.0 ** -12
        w[0] = np.abs(w[0]) * sgn[:, None]
    elif pattern == "large":
        x, w = x * 2.0 ** 12, w * 2.0 ** -12
    elif pattern == "wide_w":
        mx = np.abs(w).max()
        w[1] *= mx * 2.0 ** -16 / np.abs(w[1]).max()
        w[2] *= mx * 2.0 ** -20 / np.abs(w[2]).max()
    bias = g.standard_normal(M)   # (of order one: it carries a LayerNorm row's spread on the small pattern)
    if pattern == "small" and not s["ln"]:
        bias *= 2.0 ** -12        # (without a LayerNorm: of the sums' order, so the bound stays at the halves' floor)
    if M < 32:                    # few channels: a spread that no row's sums can cancel
        bias = 1.5 * (-1.0) ** np.arange(M) * (1 + 0.2 * g.random(M))
        w *= 0.25
    r1, r2 = g.standard_normal((B, ROWS, M)), g.standard_normal((B, ROWS, M))
    ln = dict(g1=1 + 0.1 * g.standard_normal(M), b1=0.1 * g.standard_normal(M), g2=1 + 0.1 * g.standard_normal(M),
              b2=0.1 * g.standard_normal(M), lin_w=g.standard_normal(M) / np.sqrt(M), lin_b=0.3)
    return x, w, bias, r1, r2, ln


@functools.lru_cache(maxsize=None)
def problem(case, pattern, epi, form, batch):
    """The oracle problem of a case: operands rounded to the form's dtype, rows past each length GARBAGE."""
    s, e = shape(case), EPILOGUES[epi]
    x, w, bias, r1, r2, lnp = raw_inputs(case, pattern, batch)
    dt = oc.storage(form)
    lens = BATCHES[batch]
    x = round_to(x, dt)
    for b, L in enumerate(lens):
        x[b, L:] = GARBAGE
    ln = None
    if s["ln"]:
        ln = dict(g1=lnp["g1"], b1=lnp["b1"], eps=LN_EPS[case])
        if s["ln"] == "ln12":
            ln.update(g2=lnp["g2"], b2=lnp["b2"])
        if s["ln"] == "lin":
            ln.update(lin_w=lnp["lin_w"], lin_b=lnp["lin_b"])
    res = e.get("res", False)
    return oc.problem(form, x, lens, round_to(w, dt), bias, dil=s["dil"], pad=s["pad"], in_slope=s["in_slope"],
                      act=e.get("act", False), out_slope=e.get("out_slope", 0.0), alpha=e.get("alpha", 1.0),
                      out_scale=e.get("out_scale", 1.0), r1=round_to(r1, dt) if res else None,
                      r2=round_to(r2, dt) if res else None, ln=ln)


@functools.lru_cache(maxsize=None)
def _sums(case, pattern, storage, batch):
    """The K-long float64 sums of every utterance: one computation per dtype, shared by the epilogues
    and by the f32 / split forms (the same fp32 operands)."""
    P = problem(case, pattern, "plain", "split" if storage == "f32" else storage, batch)
    return tuple(oc.sums(P, b, floors=storage == "f32") for b in range(len(P["lens"])))


@functools.lru_cache(maxsize=None)
def reference(case, pattern, epi, form, batch):
    """Per utterance: oracle.conv.reference (computed once, shared, never changed)."""
    P, base = problem(case, pattern, epi, form, batch), _sums(case, pattern, oc.storage(form), batch)
    return tuple(oc.reference(P, b, base=base[b]) for b in range(len(P["lens"])))


@functools.lru_cache(maxsize=None)
def bound(case, pattern, epi, form, batch, S=1):
    P, refs = problem(case, pattern, epi, form, batch), reference(case, pattern, epi, form, batch)
    return tuple(oc.bound(P, form, b, S=S, ref=refs[b]) for b in range(len(P["lens"])))


# ----------------------------------------------------------------- expected kernel forms
# The launchers' eligibility rules (conv_gemm.hip / conv_split.hip) restated on the shapes, under
# the default switches, for B utterances of ROWS rows.
XRES_LDS_MAX = (160 // 3 - 1) * 1024
SPLIT_LDS_MAX = 76 * 1024


def xres_group(s, res=False):
    """Channel group of the X-resident kernel for a 16-bit layer (0: conv_gemm_kernel runs it)."""
    ci, M, halo = s["Cin"], s["M"], (s["k"] - 1) * s["dil"]
    if ci % 64 or M < 64 or M % 8:
        return 0
    if s["k"] in (2, 3) and halo <= 32:
        return 64                                   # (xres_dma_layer)
    R = (128 if M >= 128 else 256) + halo
    for cg in (2048, 1024, 512, 256, 128, 64):
        if cg <= ci and ci % cg == 0 and R * (cg * 2 + 16) <= XRES_LDS_MAX:
            return cg
    return 0


def split_group(s, BN):
    R = BN + (s["k"] - 1) * s["dil"]
    for cg in (512, 256, 128, 64, 32):
        if cg <= s["Cin"] and s["Cin"] % cg == 0 and 2 * R * (cg * 2 + 16) <= SPLIT_LDS_MAX:
            return cg
    return 0


def conv_split_eligible(s):
    return s["Cin"] % 32 == 0 and s["M"] % 4 == 0 and split_group(s, 64) > 0 and split_group(s, 32) > 0


def packed_group(s, nt=2):
    R = 32 * nt + (s["k"] - 1) * s["dil"]
    su = 17 if nt >= 4 else 9
    if s["Cin"] % 128 or (R + 7) // 8 > su or 2 * R * (128 * 2 + 16) > SPLIT_LDS_MAX:
        return 0
    return 128


def packed_ok(s, rows_pad):
    right = (s["k"] - 1) * s["dil"] - s["pad"]
    return rows_pad > 0 and rows_pad >= s["pad"] and rows_pad >= right and ROWS % 32 == 0 and s["M"] % 4 == 0


def split_slices(s, cg, ws):
    groups = s["Cin"] // cg
    S = max(1, min(groups, s["K"] // 1152))
    while S > 1 and groups % S:
        S -= 1
    return S if ws else 1


def f32_kslices(s):
    nch = (s["Cin"] + 15) // 16
    S = min(16, s["Cin"] // 32)
    while S > 1 and nch % S:
        S -= 1
    return max(S, 1)


def expected(case, run, epi="plain", B=5, ln_fuse=False, with_ln=True):
    """-> dict(kind, kernels, family, cg, S, tiles): what tts_op_conv1d_ex reports (kind, kernels) and
    what the launcher picks behind it.  ln_fuse: TTS_LN_FUSE=7 with counters given."""
    s = shape(case)
    form, _, ext = RUNS[run]
    M = s["M"]
    ln = s["ln"] if with_ln else None
    act = EPILOGUES[epi].get("act", False)
    mblk = (M + 127) // 128
    out = dict(S=1, cg=0)
    ln_done = False
    if form in ("f16", "bf16"):
        cg = xres_group(s)
        if cg:
            narrow = M % 64 == 0 and M >= 128 and ((ROWS + 63) // 64) * mblk * B < 256
            # 64-channel x 256-row blocks below M = 128; else 64-row tiles (8 * 192 <= 7 * 256), narrow
            # 64 x 64 ones on a grid under 256 blocks
            bn, bm = (256, 64) if M < 128 else (64, 64 if narrow else 128)
            out.update(kind=PK_CONV_XRES, family="conv_xres", cg=cg, narrow=narrow,
                       tiles=((ROWS + bn - 1) // bn) * ((M + bm - 1) // bm) * B)
            ln_done = bool(ln) and ln_fuse and M <= 512
        else:
            bm = 32 if M <= 32 else 64 if M <= 64 else 128
            out.update(kind=PK_CONV_GEMM, family="conv_gemm", tiles=((ROWS + 127) // 128) * ((M + bm - 1) // bm) * B)
        out["kernels"] = 1
    elif form == "split":
        assert conv_split_eligible(s), case
        out["kind"] = PK_CONV_SPLIT
        cg = packed_group(s) if packed_ok(s, ext.get("rows_pad", 0)) else 0
        if cg:
            S = split_slices(s, cg, ext.get("ws", False))
            F = B * ROWS
            nt = 1 if ((F + 63) // 64) * mblk * S < 128 else 2
            if packed_group(s, 4) and ((F + 127) // 128) * mblk * S >= 320:
                nt = 4
            out.update(family="conv_splitp", cg=cg, S=S, tiles=((F + 32 * nt - 1) // (32 * nt)) * mblk * S)
            out["kernels"] = 2 if S > 1 else 1
            if S > 1:
                ln_done = ln in ("ln1", "ln12") and M <= 512 and not act
            else:
                ln_done = bool(ln) and ln_fuse and M <= 512
        else:
            out.update(family="conv_split", cg=split_group(s, 32), kernels=1, tiles=((ROWS + 31) // 32) * mblk * B)
    else:
        out.update(kind=PK_CONV_SPLIT if not ext.get("no_split") else PK_CONV_GEMM, family="conv_gemm", kernels=1)
        S = f32_kslices(s) if ext.get("f32_splitk") and M > 64 else 1
        out["S"] = S
        if S > 1:
            out["kernels"] = 2
            ln_done = ln in ("ln1", "ln12") and M <= 512 and not act
        bm = 32 if M <= 32 else 64 if M <= 64 else 128
        out["tiles"] = ((ROWS + 127) // 128) * ((M + bm - 1) // bm) * B * S
    if ln and not ln_done:
        out["kernels"] += 1
    out["ln_in_launch"] = ln_done
    return out


def slices_of(case, run):
    return expected(case, run)["S"]
