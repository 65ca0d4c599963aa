"""Cases, inputs and the float64 reference of the prosody-control tests (test_prosody_cpu.py,
test_prosody_op_gpu.py, test_prosody_gpu.py).  NumPy only.

The reference composes the existing oracle functions (oracle/acoustic.py: conformer_stack,
variance_predictor, postnet, durations_from_log; oracle/rowwise.py: durations_expected) and restates
acoustic_forward's body with the three control formulas of include/tts_hip.h (tts_prosody) in
float64:
    d      = rint(float32(d) * float32(duration_scale)) after the prediction or the override,
             before the all-zero rule
    p'[t]  = m + pitch_range (p[t] - m) + pitch_shift, m the mean of p over the utterance
    e'[t]  likewise
`defect` names a wrong implementation; the CPU test shows that the bounds the GPU tests apply
reject each of them.
"""
from __future__ import annotations

import functools

import numpy as np

import acoustic_cases as ac
import rowwise_cases as rc
from oracle import rowwise as rw
from oracle.attention import round_to

FIELDS = ("duration_scale", "pitch_shift", "pitch_range", "energy_shift", "energy_range")
NEUTRAL = dict(duration_scale=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0)
DEFECTS = ("mean_over_N", "mean_over_Np", "mean_of_neighbour", "range_on_mean", "shift_dropped", "swapped")
DUR_DEFECTS = ("scale_after_zero_rule", "scale_twice")
U = 2.0 ** -24


def controls(**kw):
    c = dict(NEUTRAL)
    c.update(kw)
    return c


def block(ctls):
    """list of control dicts -> float32 [5, B] in tts_prosody's order"""
    return np.asarray([[c[k] for c in ctls] for k in FIELDS], np.float32)


def is_neutral(c, what):
    return c[what + "_range"] == 1.0 and c[what + "_shift"] == 0.0


def adapt(v, rng, shift, mean=None):
    """m + range (v - m) + shift in float64 over the valid tokens v; range 1, shift 0: v itself"""
    v = np.asarray(v, np.float64)
    if rng == 1.0 and shift == 0.0:
        return v.copy()
    m = v.mean() if mean is None else mean
    return m + float(np.float32(rng)) * (v - m) + float(np.float32(shift))


def adapt_bound(v, L, rng, shift):
    """The worst case of any fp32 summation order of the mean plus the three roundings."""
    mx = float(np.abs(np.asarray(v, np.float64)).max()) if L else 0.0
    return (L + 4) * U * (1 + abs(rng)) * mx + U * abs(shift)


def scaled(d, scale):
    """rint(float32(d) * float32(scale)), ties to even; scale 1 skips the multiply"""
    d = np.asarray(d, np.int64)
    if np.float32(scale) == np.float32(1):
        return d.copy()
    return np.rint(d.astype(np.float32) * np.float32(scale)).astype(np.int64)


# -------------------------------------------------------------------------------------- op level
OP_D = (64, 384)


def op_np(N):
    return rc.rup(N + 2, 32)


def op_controls():
    """One per utterance of rowwise_cases.dur_lens (0, 1, N, N, N / 2, N): every scale of the issue
    (0.5 and 1.5 land on ties), ranges 0 / 0.5 / 1 / 2, shifts 0 / +-1, utterance 1 energy-neutral,
    utterance 4 pitch-neutral, utterance 5 neutral in everything."""
    return [
        controls(duration_scale=2.0, pitch_shift=1.0, pitch_range=2.0, energy_shift=-1.0, energy_range=0.0),
        controls(duration_scale=0.5, pitch_shift=1.0, pitch_range=0.0),
        controls(duration_scale=1.5, pitch_shift=-1.0, pitch_range=2.0, energy_shift=1.0, energy_range=0.5),
        controls(duration_scale=2.0, pitch_range=0.5, energy_shift=-1.0, energy_range=2.0),   # the all-zero utterance
        controls(duration_scale=float(np.float32(1) / np.float32(1.2)), energy_shift=1.0, energy_range=0.0),
        controls(),
    ]


def op_tcaps(N):
    """A frame cap above every total at every scale (d <= 7, times 2), and one that clamps
    utterance 5 (d >= 5 at scale 1)."""
    return (16 * N + 8, N)


@functools.lru_cache(maxsize=None)
def op_inputs(N, D, dt):
    """logd / pitch / energy [B, Np] float32 (NaN and inf alternate past each length), override
    [B, N], x [B, Np, D] of dt (rows past a length hold GARBAGE), the two embeddings' weights."""
    logd0, ovr, lens = rc.dur_inputs(N)
    B, Np = len(lens), op_np(N)
    g = np.random.default_rng(5150 + 7 * N + D)
    logd = np.full((B, Np), np.nan, np.float32)
    logd[:, :N] = logd0
    p = (0.9 * g.standard_normal((B, Np)) + 0.3).astype(np.float32)
    e = (0.8 * g.standard_normal((B, Np)) - 0.2).astype(np.float32)
    for b, L in enumerate(lens):
        for a in (logd, p, e):
            a[b, L:] = np.where(np.arange(Np - L) % 2 == 0, np.nan, np.inf)
    x = round_to(g.standard_normal((B, Np, D)), dt)
    for b, L in enumerate(lens):
        x[b, L:] = rc.GARBAGE
    par = [rw.f32(v) for v in (g.standard_normal(D), 0.2 * g.standard_normal(D), g.standard_normal(D),
                               0.2 * g.standard_normal(D))]
    return dict(logd=logd, ovr=ovr, lens=lens, p=p, e=e, x=x, we=par[0], be=par[1], wp=par[2], bp=par[3])


def op_adapt_expected(v, lens, ctls, what, defect=None, N=None):
    """-> (expected [B, Np] float64 with NaN past each length, bound [B, Np]); `what` pitch / energy.
    N: the token extent (the mean_over_N defect divides by it)."""
    B, Np = v.shape
    want, bnd = np.full((B, Np), np.nan), np.zeros((B, Np))
    for b, L in enumerate(lens):
        c = ctls[b]
        rng, shift = c[what + "_range"], c[what + "_shift"]
        src = v[b, :L]
        mean = None
        if defect == "swapped":
            o = "energy" if what == "pitch" else "pitch"
            rng, shift = c[o + "_range"], c[o + "_shift"]
        if defect == "shift_dropped":
            shift = 0.0 if rng != 1.0 else shift
        if L and not (rng == 1.0 and shift == 0.0):
            with np.errstate(invalid="ignore"):
                if defect in ("mean_over_N", "mean_over_Np"):   # garbage past the length counted as zeros
                    n = Np if defect == "mean_over_Np" else N
                    mean = float(np.asarray(src, np.float64).sum() / n)
                elif defect == "mean_of_neighbour":
                    nb = (b + 1) % B
                    mean = float(np.asarray(v[nb, :max(lens[nb], 1)], np.float64).mean()) if lens[nb] else 0.0
            if defect == "range_on_mean":
                m = float(np.asarray(src, np.float64).mean())
                want[b, :L] = rng * m + rng * (np.asarray(src, np.float64) - m) + shift
            else:
                want[b, :L] = adapt(src, rng, shift, mean)
        else:
            want[b, :L] = src
        c = ctls[b]
        bnd[b, :L] = adapt_bound(src, L, c[what + "_range"], c[what + "_shift"]) if not is_neutral(c, what) else 0.0
    return want, bnd


def op_durations_expected(logd, ovr, lens, N, tcap, ctls, defect=None):
    """durations_expected per utterance with its own scale -> (dur [B, N], mel_lens [B], tokmap [B, tcap])"""
    outs = []
    for b, L in enumerate(lens):
        s = float(np.float32(ctls[b]["duration_scale"]))
        o = None if ovr is None else ovr[b:b + 1]
        if defect is None:
            outs.append(rw.durations_expected(logd[b:b + 1, :N], [L], N, tcap, override_d=o, speed=s))
            continue
        d, _, _ = rw.durations_expected(logd[b:b + 1, :N], [L], N, tcap, override_d=o, speed=1.0 if defect == "scale_after_zero_rule" else s)
        d = scaled(d, s)    # after the all-zero rule, or a second time
        mel = np.minimum(d.sum(1), tcap)
        tok = np.full((1, tcap), -1, np.int64)
        m = np.repeat(np.arange(N), d[0])[:tcap]
        tok[0, :len(m)] = m
        outs.append((d, mel, tok))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


# ----------------------------------------------------------------------------------- model level
MODEL_CASES = ("h64", "h64x4", "h192")
T_CAP = 320      # 195 frames at 3 per token become 260 at scale 1.5 (rint(4.5) = 4)
# one control setting each, as the issue measured them on the oracle (rel-RMS move of the mel)
SETTINGS = {
    "pitch_range=2": controls(pitch_range=2.0),
    "pitch_shift=1": controls(pitch_shift=1.0),
    "energy_range=0": controls(energy_range=0.0),
    "energy_shift=-1": controls(energy_shift=-1.0),
}
MOVE_CASES, MOVE_UTTS = ("h64", "h192"), (2, 4)
LOOSEST_BAR = 2e-2     # parity.TOL ac_bf16 rel-RMS


def model_controls():
    """One per utterance of acoustic_cases.TOKENS: utterances 0 and 7 neutral, every setting of
    SETTINGS alone on one utterance, the scale alone, and two combinations."""
    return [
        controls(),
        controls(duration_scale=1.5),
        SETTINGS["pitch_range=2"],
        SETTINGS["pitch_shift=1"],
        SETTINGS["energy_range=0"],
        controls(duration_scale=1.5, energy_shift=-1.0),
        controls(duration_scale=1.5, pitch_range=2.0, energy_shift=-1.0),
        controls(),
    ]


def controlled_forward(ids, w, cfg, ctl, durations=None, spk=None, dtype=np.float64):
    """oracle.acoustic.acoustic_forward's body for one utterance with the controls `ctl` applied."""
    from oracle.acoustic import conformer_stack, durations_from_log, postnet, variance_predictor
    w = {k: np.asarray(v, dtype) if np.asarray(v).dtype.kind == "f" else v for k, v in w.items()}
    x = w["encoder.embed.weight"][np.asarray(ids, np.int64)]
    x = conformer_stack(x, w, "encoder.", cfg.encoder_layers, cfg.num_attention_heads)
    if spk is not None and "projection.weight" in w:
        e = np.asarray(spk, dtype)
        e = e / max(float(np.sqrt((e.astype(np.float64) ** 2).sum())), 1e-12)
        x = np.concatenate([x, np.broadcast_to(e, (x.shape[0], e.shape[0]))], axis=1) @ w["projection.weight"].T \
            + w["projection.bias"]
    pitch = variance_predictor(x, w, "pitch_predictor.", cfg.pitch_predictor_layers)
    energy = variance_predictor(x, w, "energy_predictor.", cfg.energy_predictor_layers)
    logd = variance_predictor(x, w, "duration_predictor.", cfg.duration_predictor_layers)
    s = float(np.float32(ctl["duration_scale"]))
    if durations is None:
        d = durations_from_log(logd, s)
    else:
        d = scaled(np.maximum(np.asarray(durations, np.int64), 0), s)
        if d.sum() == 0:
            d[:] = 1
    pitch = adapt(pitch, ctl["pitch_range"], ctl["pitch_shift"])
    energy = adapt(energy, ctl["energy_range"], ctl["energy_shift"])
    e_emb = energy[:, None] * w["energy_embed.conv.weight"][:, 0, 0] + w["energy_embed.conv.bias"]
    p_emb = pitch[:, None] * w["pitch_embed.conv.weight"][:, 0, 0] + w["pitch_embed.conv.bias"]
    x = (x + e_emb) + p_emb
    x = np.repeat(x, d, axis=0)
    x = conformer_stack(x, w, "decoder.", cfg.decoder_layers, cfg.num_attention_heads)
    return dict(mel=postnet(x, w, cfg.postnet_layers), durations=d, pitch=pitch, energy=energy, log_durations=logd)


_CACHE = {}


def controlled_oracle64(name):
    """The ragged batch of acoustic_cases with model_controls(), durations given; computed once."""
    if name not in _CACHE:
        ids, durs = ac.ragged_inputs(name)
        spk = ac.speaker_embeddings(name, len(ids))
        _CACHE[name] = [controlled_forward(x, ac.weights(name), ac.CASES[name].cfg, c, durations=d,
                                           spk=None if spk is None else spk[b])
                        for b, (x, d, c) in enumerate(zip(ids, durs, model_controls()))]
    return _CACHE[name]
