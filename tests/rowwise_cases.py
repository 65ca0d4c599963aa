"""Shapes, inputs and references of the op-level tests of the acoustic model's row-wise kernels
(test_rowwise_op_cpu.py, test_rowwise_op_gpu.py): the smallest shapes at which each branch of
csrc/acoustic_kernels.hip is reached.  NumPy only.  Every input is rounded to the working dtype
here; rows and columns that an op's contract (include/tts_hip.h) calls masked hold GARBAGE, a
finite stand-in -- the GPU test puts NaN / 1e30 there instead and expects the same bits.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import rowwise as rw
from oracle.attention import round_to

DTYPES = ("f16", "bf16", "f32")
SENTINEL = -77.0   # pre-fill of every output (exact in bf16)
GARBAGE = 3.0
EPS = 1e-5
GRID1_ELEMS = 4096 * 256   # elements one trip of the elementwise kernels' grid-stride loop covers


def _rng(*key):
    return np.random.default_rng(int.from_bytes(repr(key).encode(), "little") % (2 ** 63))


def rup(n, m):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------ glu_dwconv
GLU_TM = 272                                                   # row stride of every utterance
GLU_LENS = (0, 1, 3, 15, 127, 128, 129, 256, 257, 272)         # 15: shorter than the k = 31 / 129 halo
SIXTEEN = ("f16", "bf16")
#            k    D   dtypes   kernel
GLU_CASES = {
    "k7_d64": (7, 64, DTYPES, "k"),
    "k7_d72": (7, 72, DTYPES, "k"),          # partial channel block, D % 8 == 0: 16-byte loads stop mid-block
    "k7_d68": (7, 68, ("f32",), "k"),        # D % 4 == 0 only
    "k7_d70": (7, 70, SIXTEEN, "generic"),   # D % 8 != 0: falls to the generic kernel
    "k31_d192": (31, 192, DTYPES, "k"),
    "k31_d72": (31, 72, DTYPES, "k"),
    "k3_d64": (3, 64, DTYPES, "generic"),
    "k9_d192": (9, 192, DTYPES, "generic"),
    "k129_d72": (129, 72, DTYPES, "generic"),  # GLU_DWCONV_MAX_K: a 64 KiB LDS tile
}
GLU_PATTERNS = ("normal", "saturated", "tiny")
GLU_REFUSED_K = (131, 8, 0)


def glu_kernel(k, D, dt):
    """Which kernel launch_glu_dwconv picks."""
    return "k" if k in (7, 31) and D % (4 if dt == "f32" else 8) == 0 else "generic"


@functools.lru_cache(maxsize=None)
def glu_problem(case, pattern, dt):
    k, D, _, _ = GLU_CASES[case]
    g = _rng("glu", case, pattern)
    B = len(GLU_LENS)
    x = g.standard_normal((B, GLU_TM, D))
    gate = 2.0 * g.standard_normal((B, GLU_TM, D))
    w = g.standard_normal((D, k)) / math.sqrt(k)
    bias = 0.3 * g.standard_normal(D)
    if pattern == "saturated":
        # gates far out on both sides (sigmoid through exp -> inf -> 0 and exp -> 0 -> 1); x large enough
        # that the pre-activation sums reach magnitude 40 - 100 and beyond (SiLU through the same)
        top = 6.0e4 if dt == "f16" else 100.0
        gate = np.where(g.random(gate.shape) < 0.5, -1.0, 1.0) * g.uniform(40.0, top, gate.shape)
        x = x * (8.0e3 if dt == "f16" else 60.0)
    elif pattern == "tiny":
        x, gate, bias = x * 2.0 ** -12, gate * 2.0 ** -12, bias * 2.0 ** -12
    a = round_to(np.concatenate([x, gate], -1), dt)
    for b, L in enumerate(GLU_LENS):
        a[b, L:] = GARBAGE
    return rw.glu_problem(dt, a, GLU_LENS, w, bias)


@functools.lru_cache(maxsize=None)
def glu_reference(case, pattern, dt):
    P = glu_problem(case, pattern, dt)
    refs = tuple(rw.glu_reference(P, b) for b in range(len(GLU_LENS)))
    return refs, tuple(rw.glu_bound(P, b, r) for b, r in enumerate(refs))


# ----------------------------------------------------------------------------------- rel_softmax
SM_H = 2
SM_TM = (1, 5, 64, 65, 130)
SM_PATTERNS = ("normal", "equal", "sharp", "negative")
SM_SCALE = 0.125   # 1 / sqrt(64)


def sm_lens(Tm):
    return (0, 1, max(Tm // 2, 1), Tm)


def sm_extents(Tm):
    """(Sac, Sbd, Sk) as acoustic.cpp sizes them."""
    return rup(Tm, 16), rup(2 * Tm, 16), rup(Tm, 16)


def sm_mask(ac, bd, lens, Tm, fill):
    """Everything the contract says is not read (for a valid row) replaced by `fill`, and every row
    at or past a length."""
    ac, bd = ac.copy(), bd.copy()
    for b, L in enumerate(lens):
        ac[b, :, :, L:] = fill
        ac[b, :, L:] = fill
        bd[b, :, L:] = fill
        for i in range(L):
            bd[b, :, i, :Tm - 1 - i] = fill
            bd[b, :, i, Tm - 1 - i + L:] = fill
    return ac, bd


@functools.lru_cache(maxsize=None)
def sm_problem(Tm, pattern, dt):
    g = _rng("softmax", Tm, pattern)
    lens = sm_lens(Tm)
    Sac, Sbd, _ = sm_extents(Tm)
    B = len(lens)
    ac = 8.0 * g.standard_normal((B, SM_H, Tm, Sac))
    bd = 8.0 * g.standard_normal((B, SM_H, Tm, Sbd))
    if pattern == "equal":
        ac[:], bd[:] = 1.5, 0.25
    elif pattern == "sharp":      # one key per row ahead of the rest by >= 80 after the scale
        hot = g.integers(0, np.maximum(np.array(lens), 1)[:, None, None], (B, SM_H, Tm))
        ac = 20.0 * g.standard_normal(ac.shape)
        np.put_along_axis(ac, hot[..., None], 1200.0, -1)
        bd = g.standard_normal(bd.shape)
    elif pattern == "negative":
        ac = -3.0e4 + 64.0 * g.standard_normal(ac.shape)
    ac, bd = sm_mask(round_to(ac, dt), round_to(bd, dt), lens, Tm, GARBAGE)
    return rw.softmax_problem(dt, ac, bd, lens, Tm, SM_SCALE)


@functools.lru_cache(maxsize=None)
def sm_reference(Tm, pattern, dt):
    P = sm_problem(Tm, pattern, dt)
    refs = tuple(rw.softmax_reference(P, b) if L else None for b, L in enumerate(P["lens"]))
    return refs, tuple(rw.softmax_bound(P, b, r) if r else None for b, r in enumerate(refs))


# ----------------------------------------------------------------------------------- transpose_v
TV_H, TV_TM, TV_SK = 2, 80, 88
TV_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 80)
TV_DK = (64, 128, 48, 192)     # 64 / 128: transpose_v16_kernel in 16-bit; the rest and all of fp32: generic
SPECIALS = {   # -0, the smallest subnormal, +-inf and the largest finite value of each dtype
    "f16": (-0.0, 2.0 ** -24, -2.0 ** -24, np.inf, -np.inf, 65504.0, -65504.0),
    "bf16": (-0.0, 2.0 ** -133, -2.0 ** -133, np.inf, -np.inf, float(np.float32(3.3895314e38)), -float(np.float32(3.3895314e38))),
    "f32": (-0.0, 2.0 ** -149, -2.0 ** -149, np.inf, -np.inf, float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max)),
}


def with_specials(a, dt, g, every=37):
    """A copy of `a` (values of dt) with the dtype's special values at every `every`-th element."""
    flat = a.reshape(-1).copy()
    sp = np.array(SPECIALS[dt])
    idx = np.arange(g.integers(0, every), flat.size, every)
    flat[idx] = sp[np.arange(idx.size) % sp.size]
    return flat.reshape(a.shape)


def same_bits(a, b):
    """Equality of fp32-representable arrays bit for bit (-0 != +0)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def tv_inputs(dk, dt):
    g = _rng("transpose_v", dk)
    D = TV_H * dk
    qkv = with_specials(round_to(g.standard_normal((len(TV_LENS), TV_TM, 3 * D)), dt), dt, g)
    return qkv, rw.transpose_v_expected(qkv, TV_LENS, D, TV_H, TV_SK)


# ------------------------------------------------------- pos_bias, var_embed_add, mel_out (elementwise)
#            rows   D
EW_SHAPES = {"small": (37, 72), "two_trips": (GRID1_ELEMS // 80 + 1, 80)}   # the second: 80 elements past one trip


@functools.lru_cache(maxsize=None)
def pb_inputs(shape, dt):
    rows, D = EW_SHAPES[shape]
    g = _rng("pos_bias", shape)
    qkv = round_to(g.standard_normal((rows, 3 * D)), dt)
    u, v = rw.f32(g.standard_normal(D)), rw.f32(g.standard_normal(D))
    return qkv, u, v, rw.pos_bias_expected(dt, qkv, D, u, v)


@functools.lru_cache(maxsize=None)
def ve_inputs(shape, dt):
    rows, D = EW_SHAPES[shape]
    g = _rng("var_embed", shape)
    x = round_to(g.standard_normal((rows, D)), dt)
    e, p = rw.f32(g.standard_normal(rows)), rw.f32(2.0 * g.standard_normal(rows))
    we, be, wp, bp = (rw.f32(g.standard_normal(D)) for _ in range(4))
    ref = rw.var_reference(x, e, we, be, p, wp, bp)
    return dict(x=x, e=e, we=we, be=be, p=p, wp=wp, bp=bp), ref, rw.var_bound(x, ref, dt)


#             B  Tin    Tcap   C   lens
MEL_SHAPES = {"tin_above": (3, 24, 16, 80, (0, 24, 5)), "tin_below": (3, 16, 24, 80, (0, 16, 7)),
              "two_trips": (1, GRID1_ELEMS // 80 + 1, GRID1_ELEMS // 80 + 1, 80, (13000,))}


@functools.lru_cache(maxsize=None)
def mel_inputs(shape, dt):
    B, Tin, Tcap, C, lens = MEL_SHAPES[shape]
    g = _rng("mel_out", shape)
    x = with_specials(round_to(g.standard_normal((B, Tin, C)), dt), dt, g)
    return x, rw.mel_out_expected(x, lens, Tcap)


# ------------------------------------------------------------------------------- embed, regulate
EMB_V, EMB_N, EMB_TM = 50, 12, 16
EMB_LENS = (0, 1, 12, 20, 7)          # 20 > N: clamped
EMB_D = (72, 384)


@functools.lru_cache(maxsize=None)
def emb_inputs(D, dt):
    g = _rng("embed", D)
    ids = g.integers(0, EMB_V, (len(EMB_LENS), EMB_N))
    ids[2, :4] = (0, EMB_V - 1, -5, EMB_V + 3)      # both ends, and out of range on both sides
    ids[3, -2:] = (-1, 10 ** 6)
    table = round_to(g.standard_normal((EMB_V, D)), dt)
    scale = math.sqrt(D)
    return ids, table, scale, rw.embed_expected(dt, ids, EMB_LENS, EMB_TM, table, scale)


REG_N, REG_TCAP, REG_TOUT, REG_FRAMES, REG_B = 12, 40, 48, 33, 3
REG_FORMS = (("f32", "f16"), ("f32", "bf16"), ("f16", "f16"), ("bf16", "bf16"), ("f32", "f32"))
REG_REFUSED = (("f16", "bf16"), ("bf16", "f16"), ("f16", "f32"))


@functools.lru_cache(maxsize=None)
def reg_inputs(D, dt_in, dt):
    g = _rng("regulate", D)
    enc = round_to(g.standard_normal((REG_B, REG_N, D)), dt_in)
    tokmap = g.integers(0, REG_N, (REG_B, REG_TCAP))
    tokmap[0, 20:] = -1
    tokmap[1, ::5] = -1
    tokmap[2, :] = -1
    tokmap[2, 3] = REG_N - 1
    scale = math.sqrt(D)
    return enc, tokmap, scale, rw.regulate_expected(dt, enc, tokmap, REG_FRAMES, REG_TOUT, scale, SENTINEL)


# -------------------------------------------------------------------------------------- durations
DUR_N = (1, 7, 300)
DUR_SPEEDS = (1.0, 0.5, 1.5)
DUR_MARGIN = 0.15      # distance of exp(x) - 1 from every half-integer; fp32 expf is off by < 1e-5 here


def dur_lens(N):
    return (0, 1, N, N, max(N // 2, 1), N)


@functools.lru_cache(maxsize=None)
def dur_inputs(N):
    """logd [B, N] (fp32 values), override [B, N], lens: utterance 2 has zero-duration tokens at both
    ends and in the middle, utterance 3 is all zero (the others are not), utterance 5 is long enough to
    pass a small Tcap; past each length NaN and 1e30 alternate."""
    g = _rng("durations", N)
    lens = dur_lens(N)
    B = len(lens)
    n = g.integers(0, 7, (B, N)).astype(np.float64)
    n[2, [0, N // 2, N - 1]] = 0
    n[3] = 0
    n[5] = 5 + g.integers(0, 3, N)
    v = n + g.uniform(-0.3, 0.3, (B, N))
    logd = np.log(1.0 + v).astype(np.float32)
    ovr = g.integers(-3, 7, (B, N))
    ovr[2, [0, N // 2, N - 1]] = (0, -2, 0)
    ovr[3] = -g.integers(0, 3, N)
    ovr[5] = n[5]
    for b, L in enumerate(lens):
        logd[b, L:] = np.where(np.arange(N - L) % 2 == 0, np.nan, 1e30)
        ovr[b, L:] = 10 ** 6
    return logd, ovr.astype(np.int32), lens


def dur_tcaps(N):
    """A frame cap above every total at every speed (d <= 7, times 1.5), and one below utterance 5's
    (d >= 5, times 0.5)."""
    return (12 * N + 8, N)


# --------------------------------------------------------------------------------------- spk_bias
SPK_E, SPK_D = (1, 64, 300), (72, 384)
SPK_ROWS = ("unit", "zero", "1e-20", "1e3")


@functools.lru_cache(maxsize=None)
def spk_inputs(E, D):
    g = _rng("spk_bias", E, D)
    e = g.standard_normal((len(SPK_ROWS), E))
    e /= np.sqrt((e ** 2).sum(1, keepdims=True))
    e[1] = 0.0
    e[2] *= 1e-20
    e[3] *= 1e3
    e, We, bias = rw.f32(e), rw.f32(g.standard_normal((D, E)) / math.sqrt(E)), rw.f32(g.standard_normal(D))
    return e, We, bias


# ------------------------------------------------------------------------------------- LayerNorm
LN_C = (8, 100, 256, 300, 512)
LN_STRIDE, LN_LENS = 12, (12, 5, 0)
LNG_C, LNG_G, LNG_GAP = (8, 100, 256), (1, 3, 4), 8
LN_REFUSED_C, LNG_REFUSED = 513, dict(groups=5, C=257)


def ln_kernel(C, dt):
    """Which kernel launch_layernorm picks."""
    if dt != "f32" and C % 8 == 0:
        return "layernorm8"
    return "layernorm<4>" if C <= 256 else "layernorm<8>"


def ln_valid_rows():
    return np.concatenate([b * LN_STRIDE + np.arange(L) for b, L in enumerate(LN_LENS)]).astype(np.int64)


def _ln_rows(g, rows, C, dt):
    x = g.standard_normal((rows, C)) * (1.0 + g.random((rows, 1)) * 3.0) + g.standard_normal((rows, 1))
    x[0] = 100.0 + 0.1 * g.standard_normal(C)      # a one-pass variance loses this row's spread
    x[1] = 2.5                                     # constant: eps decides
    return round_to(x, dt)


@functools.lru_cache(maxsize=None)
def ln_inputs(C, dt):
    g = _rng("layernorm", C)
    x = _ln_rows(g, LN_STRIDE * len(LN_LENS), C, dt)
    par = [rw.f32(v) for v in (1 + 0.2 * g.standard_normal(C), 0.2 * g.standard_normal(C), 1 + 0.2 * g.standard_normal(C),
                               0.2 * g.standard_normal(C))]
    return x, par


@functools.lru_cache(maxsize=None)
def ln_reference(C, dt, two):
    x, (g1, b1, g2, b2) = ln_inputs(C, dt)
    if not two:
        g2 = b2 = None
    xv = x[ln_valid_rows()]
    ref = rw.ln_reference(xv, g1, b1, EPS, g2, b2)
    return ref, rw.ln_bound(xv, ref, dt, g1, b1, EPS, g2, b2)


@functools.lru_cache(maxsize=None)
def lng_inputs(G, C, dt):
    g = _rng("layernorm_groups", G, C)
    rows, ld = LN_STRIDE * len(LN_LENS), G * C + LNG_GAP
    x = np.full((rows, ld), GARBAGE)
    for i in range(G):
        x[:, i * C:(i + 1) * C] = _ln_rows(g, rows, C, dt)
    gains = tuple(rw.f32(1 + 0.5 * g.standard_normal(C)) for _ in range(G))
    biases = tuple(rw.f32(0.2 * g.standard_normal(C)) for _ in range(G))
    return x, gains, biases


@functools.lru_cache(maxsize=None)
def lng_reference(G, C, dt):
    """(ref, bound) [valid rows, G * C]."""
    x, gains, biases = lng_inputs(G, C, dt)
    xv = x[ln_valid_rows()]
    ref, bnd = np.zeros((xv.shape[0], G * C)), np.zeros((xv.shape[0], G * C))
    for i in range(G):
        seg = xv[:, i * C:(i + 1) * C]
        r = rw.ln_reference(seg, gains[i], biases[i], EPS)
        ref[:, i * C:(i + 1) * C] = r["ln"]
        bnd[:, i * C:(i + 1) * C] = rw.ln_bound(seg, r, dt, gains[i], biases[i], EPS)
    return ref, bnd
