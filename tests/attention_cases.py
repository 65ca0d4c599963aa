"""Inputs of the op-level attention tests (test_attention_cpu.py, test_attention_gpu.py): score
patterns that drive the fused relative-position attention (csrc/attention.hip, through
tts_op_rel_attn) into the regimes the whole-model tests never reach, the ragged shapes they run
at, the float64 references and the parity bounds taken from the reference alone.

Every pattern: dk = 192; q, k, v and the position table R drawn N(0, 1) with a fixed seed, scaled
as below and stored in the dtype under test; pos_u / pos_v 0.1 N(0, 1) in float32.  R is a random
table, so every relative offset is distinct and a slipped index shows at full contrast (the
model's R is a smooth sinusoid projection).

A plain helper module (no fixtures).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

from oracle import attention as oa

DK = 192
SCALE = 1.0 / math.sqrt(DK)
GARBAGE = 1e4          # fills qkv rows past each length, and the table's unused last row
SENTINEL = -768.0      # prefill of `out` (exact in f16 and bf16)
RMAX_PAD = 256         # the model's table granule: rmax = rup(Tm, 256)
NREL = 511             # relative offsets -255 .. 255 drawn per pattern and head count

# name -> what it reaches, measured on the reference (test_attention_cpu.py asserts the moves)
PATTERNS = OrderedDict([
    # spread ~1 log2, no row moves: the regime the suite had before, kept as the control
    ("flat", "q, k, R x 0.25"),
    # spread 45-55 log2, about a sixth of the rows of a 200-key utterance move once, P spans its range
    ("sharp", "q, k x 2"),
    # scores climb ~16 log2 per 32-key step: every row past 32 keys moves, up to 5 times at 200 keys
    ("ramp", "q = 0.5 q + 8 d, k = 0.5 k + 0.6 j d, R x 0.5 (d: a unit vector, every third component equal)"),
    # the first step holds the max, later steps underflow to 0 (at_exp2); no moves
    ("descend", "as ramp with the k term's sign flipped"),
    # scores from Qv . R alone: the relative-shift index map at full contrast
    ("pos", "k = 0, pos_u = 0, q x 1.5, R x 1.5"),
])

DTYPES = ("f16", "bf16", "f32", "split")   # "split": fp32 operands, the split-precision kernel

# name -> (lengths, heads, padded row stride?, padded table?).  Together the lengths are 1, 15, 16,
# 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 200 and an empty utterance; B H is 2, 9, 9, 18,
# never a multiple of the 8 XCDs; Tp is Tm or rup(Tm + 7, 8); rmax is Tm (both ends of the table
# and the clamp in reach) or rup(Tm, 256) as in the model.
SHAPES = OrderedDict([
    ("b1", ((200,), 2, False, False)),
    ("b3", ((65, 1, 129), 3, True, True)),
    ("b9", ((15, 16, 17, 31, 32, 33, 63, 64, 96), 1, False, False)),
    ("b9z", ((95, 97, 128, 0, 200, 1, 64, 65, 33), 2, True, True)),
])


def rup(x, m):
    return (x + m - 1) // m * m


def extents(lens, pad_rows, pad_table):
    """-> (Tm, Tp, rmax)"""
    Tm = max(lens)
    return Tm, (rup(Tm + 7, 8) if pad_rows else Tm), (rup(Tm, RMAX_PAD) if pad_table else Tm)


def _seed(pattern, *more):
    return [4000 + list(PATTERNS).index(pattern), *more]


def direction():
    d = np.zeros(DK)
    d[::3] = 1.0
    return d / np.sqrt((d ** 2).sum())


def table_by_rel(pattern, H, dtype):
    """R by relative offset: [NREL, H, dk] float64 holding `dtype` values, row n <-> rel = n - 255."""
    R = np.random.default_rng(_seed(pattern, 1, H)).standard_normal((NREL, H, DK))
    R *= {"flat": 0.25, "ramp": 0.5, "descend": 0.5, "pos": 1.5}.get(pattern, 1.0)
    return oa.round_to(R, dtype)


def table(pattern, H, rmax, dtype):
    """The table as build_ptabs lays it out: [2 rmax, H, dk], row r <-> rel = rmax - 1 - r; the last
    row (rel = -rmax, which no query / key pair has) holds garbage."""
    assert rmax <= 256
    Rr = table_by_rel(pattern, H, dtype)
    t = np.full((2 * rmax, H, DK), GARBAGE)
    t[:2 * rmax - 1] = Rr[255 + (rmax - 1 - np.arange(2 * rmax - 1))]
    return t


def pos_bias(pattern, H):
    rng = np.random.default_rng(_seed(pattern, 2, H))
    u, v = (0.1 * rng.standard_normal((2, H, DK))).astype(np.float32)
    if pattern == "pos":
        u = np.zeros_like(u)
    return u, v


def utterance(pattern, shape, b, dtype):
    """(q, k, v) [L, H, dk] float64 holding `dtype` values: utterance b of a shape, its own draw
    (the same whether it runs alone or inside its batch)."""
    lens, H = SHAPES[shape][:2]
    L = lens[b]
    q, k, v = np.random.default_rng(_seed(pattern, 3, list(SHAPES).index(shape), b)).standard_normal((3, L, H, DK))
    d, j = direction(), np.arange(L)[:, None, None]
    if pattern == "flat":
        q, k = 0.25 * q, 0.25 * k
    elif pattern == "sharp":
        q, k = 2 * q, 2 * k
    elif pattern in ("ramp", "descend"):
        q = 0.5 * q + 8 * d
        k = 0.5 * k + (0.6 if pattern == "ramp" else -0.6) * j * d
    elif pattern == "pos":
        q, k = 1.5 * q, np.zeros_like(k)
    return oa.round_to(q, dtype), oa.round_to(k, dtype), oa.round_to(v, dtype)


_CACHE = {}


def _memo(key, f):
    if key not in _CACHE:
        r = f()
        for a in (r if isinstance(r, (list, tuple)) else [r]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def case_inputs(pattern, shape, dtype):
    """-> dict(lens, H, Tm, Tp, rmax, pos_u, pos_v, table [2 rmax, H, dk], utts [(q, k, v)]);
    computed once and shared (read-only)."""
    def make():
        lens, H, pad_rows, pad_table = SHAPES[shape]
        Tm, Tp, rmax = extents(lens, pad_rows, pad_table)
        u, v = pos_bias(pattern, H)
        utts = [utterance(pattern, shape, b, dtype) for b in range(len(lens))]
        for t in utts:
            for a in t:
                a.setflags(write=False)
        return dict(lens=lens, H=H, Tm=Tm, Tp=Tp, rmax=rmax, pos_u=u, pos_v=v, table=table(pattern, H, rmax, dtype),
                    utts=utts)
    return _memo(("in", pattern, shape, dtype), make)


def _per_utt(pattern, shape, dtype, f):
    c = case_inputs(pattern, shape, dtype)
    return [f(q, k, v, c["table"], c["pos_u"], c["pos_v"], c["rmax"], dtype, SCALE) if len(q) else np.zeros((0, c["H"], DK))
            for q, k, v in c["utts"]]


def reference(pattern, shape, dtype):
    """Float64 outputs [L, H, dk], one per utterance."""
    return _memo(("ref", pattern, shape, dtype), lambda: _per_utt(pattern, shape, dtype, oa.rel_attention))


def rounded(pattern, shape, dtype):
    """The rounding model's outputs (oracle.attention.rel_attention_rounded), one per utterance."""
    return _memo(("rnd", pattern, shape, dtype), lambda: _per_utt(pattern, shape, dtype, oa.rel_attention_rounded))


def case_scores(pattern, shape, dtype):
    """Float64 scores [H, L, L] of every non-empty utterance."""
    c = case_inputs(pattern, shape, dtype)
    return _memo(("s", pattern, shape, dtype),
                 lambda: [oa.scores(q, k, c["table"], c["pos_u"], c["pos_v"], c["rmax"], dtype, SCALE)
                          for q, k, v in c["utts"] if len(q)])


def errors(outs, refs):
    """(rel_rms pooled over the non-empty utterances, max_abs over all) of outs against refs."""
    se = sr = mx = 0.0
    for o, r in zip(outs, refs):
        if r.size:
            e = np.asarray(o, np.float64) - r
            se += float((e ** 2).sum())
            sr += float((r ** 2).sum())
            mx = max(mx, float(np.abs(e).max()))
    return float(np.sqrt(se / sr)), mx


# 16-bit: the convention of vocoder_cases.bound.  fp32 and split: nobody had measured these kernels
# at op level, so the bar is the error of the same formula in plain NumPy float32, times 4 -- the
# kernels sum in another order and the split form carries about 22 bits per product.
BOUND_FACTOR = {"f16": 3.0, "bf16": 3.0, "f32": 4.0, "split": 4.0}


def bound(pattern, shape, dtype):
    """(rel_rms, max_abs) parity bound of a case, held on every non-empty utterance in both
    metrics: BOUND_FACTOR x the rounding model's error against the float64 reference, pooled over
    the case's batch.  Both use the same rounded operands; nothing here comes from a kernel."""
    e, m = errors(rounded(pattern, shape, dtype), reference(pattern, shape, dtype))
    f = BOUND_FACTOR[dtype]
    return f * e, f * m


def within(out, ref, bnd):
    """Does one utterance's output meet the bound?  -> (ok, rel_rms, max_abs)"""
    e = np.asarray(out, np.float64) - ref
    rr = float(np.sqrt((e ** 2).mean()) / (np.sqrt((ref ** 2).mean()) + 1e-30))
    mx = float(np.abs(e).max())
    return bool(np.isfinite(e).all() and rr <= bnd[0] and mx <= bnd[1]), rr, mx


def defective(defect, pattern, shape, dtype):
    """The float64 reference with one defect injected (oracle.attention.DEFECTS), one output per
    utterance; the fp32 kernel's online softmax is eager (lazy = 0), the others' lazy."""
    c = case_inputs(pattern, shape, dtype)
    lazy = 0.0 if dtype == "f32" else oa.LAZY
    return [oa.rel_attention_defect(defect, q, k, v, c["table"], c["pos_u"], c["pos_v"], c["rmax"], dtype, SCALE,
                                    lazy=lazy, garbage=GARBAGE) if len(q) else np.zeros((0, c["H"], DK))
            for q, k, v in c["utts"]]


def rejected(defect, pattern, shape, dtype):
    """True when the parity test of this case would fail on a kernel with the defect: some
    utterance's defective output is outside the case's bound."""
    refs, bnd = reference(pattern, shape, dtype), bound(pattern, shape, dtype)
    return any(r.size and not within(o, r, bnd)[0] for o, r in zip(defective(defect, pattern, shape, dtype), refs))


# ------------------------------------------------------------- whole-model complement (rel_softmax)
# The four-launch attention (rel_softmax: every head size other than 192, and 192 under
# TTS_REL_ATTN=0) has no op entry; it gets sharper scores through a whole fp32 model whose
# linear_q / linear_k weights are scaled.  The factor is the largest at which the oracle's own
# float32-against-float64 mel difference stays under a third of the project's fp32 bar (atol 1e-5,
# rtol 1e-4), so the bar is not spent on the reference (test_attention_cpu.py asserts it).  Measured
# on the oracle, as a fraction of the bar / rows that move: h64 1.3: 0.33 / 0, 1.4: 0.25 / 4,
# 1.5: 0.34 / 13, 3: 1.97 / 605; h192 1.25: 0.24 / 0, 1.3: 0.30 / 0, 1.4: 0.60 / 1, 1.5: 0.41 / 1,
# 3: 2.43 / 327.  A factor of 3 is far outside; h64 has a factor where rows move, h192 has
# none (its moving rows are the op-level tests' business), so it runs at the largest clear factor.
SHARPEN = OrderedDict([("h64", 1.4), ("h192", 1.25)])
SHARPEN_MOVES = {"h64": True, "h192": False}
FP32_ATOL, FP32_RTOL = 1e-5, 1e-4


def sharpened_weights(name):
    import acoustic_cases as acs

    def make():
        w = dict(acs.weights(name))
        for k in w:
            if k.endswith(("self_attn.linear_q.weight", "self_attn.linear_k.weight")):
                w[k] = (w[k] * np.float32(SHARPEN[name])).astype(np.float32)
        return w
    return _memo(("sw", name), make)


def sharpened_oracle(name, dtype=np.float64):
    """acoustic_forward mels of acoustic_cases' ragged batch (durations forced) on the sharpened
    weights, one per utterance."""
    import acoustic_cases as acs
    from oracle.acoustic import acoustic_forward

    def make():
        ids, durs = acs.ragged_inputs(name)
        return [acoustic_forward(x, sharpened_weights(name), acs.CASES[name].cfg, durations=d, dtype=dtype)["mel"]
                for x, d in zip(ids, durs)]
    return _memo(("so", name, np.dtype(dtype).name), make)
