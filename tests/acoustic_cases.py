"""Small FastSpeech2-Conformer configurations other than the default, shared by the
acoustic-configuration tests (test_acoustic_configs_cpu.py, test_acoustic_configs_gpu.py,
golden/make_ac_cfg_golden.py).

The engine reads every dimension of the acoustic model from the weight shapes, and its kernels are
compiled for more than the one shape the other acoustic tests load (D = 384, 2 heads of 192, FFN
1536 x 3 taps, depthwise 7 / 31, 256-channel predictors, 256-unit postnet).  Each case here is one
or two layers per stack, so the oracle sits close to the kernel under test and costs milliseconds.
Every case keeps 80 mel bins (HipEngine.acoustic allocates [B, T, 80]) and stays inside the
envelope AcousticModel::finalize enforces (`in_envelope` below restates it).

A plain helper module (no fixtures): cases, their weights, inputs and cached float64 oracle outputs.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from gonova_tts_amd.config import AcousticConfig


@dataclass
class Case:
    cfg: AcousticConfig
    # FFN width of the decoder layers where it differs from cfg.linear_units (the encoder's); the
    # project's configuration has one field, transformers' has one per stack
    decoder_linear_units: Optional[int] = None

    @property
    def dec_units(self):
        return self.decoder_linear_units or self.cfg.linear_units


def _cfg(D, H, ffn, ffn_k, dw, dur, pitch, energy, postnet, enc_layers=1, dec_layers=1, spk=None):
    """dur / pitch / energy: (layers, channels, kernel); postnet: (layers, units, kernel); dw: (encoder, decoder)"""
    return AcousticConfig(
        hidden_size=D, num_attention_heads=H, linear_units=ffn, positionwise_conv_kernel_size=ffn_k,
        encoder_layers=enc_layers, decoder_layers=dec_layers, encoder_kernel_size=dw[0], decoder_kernel_size=dw[1],
        duration_predictor_layers=dur[0], duration_predictor_channels=dur[1], duration_predictor_kernel_size=dur[2],
        pitch_predictor_layers=pitch[0], pitch_predictor_channels=pitch[1], pitch_predictor_kernel_size=pitch[2],
        energy_predictor_layers=energy[0], energy_predictor_channels=energy[1], energy_predictor_kernel_size=energy[2],
        postnet_layers=postnet[0], postnet_units=postnet[1], postnet_kernel=postnet[2], speaker_embed_dim=spk)


# name -> case; what each isolates is in the comment above it
CASES = OrderedDict([
    # heads of 64 (transpose_v16, attention GEMMs at K = 64) at the smallest hidden size; FFN of one
    # tap and 320 channels (a multiple of 64, not of 128); depthwise 5 / 9 (the generic kernel);
    # the pitch predictor wider and deeper than the duration predictor (3 layers of 128 against one
    # of 64: the predictor buffers used to be sized by the duration predictor, and batch_predictors
    # declines); a postnet wider than every predictor (320: its buffers were sized by the duration
    # predictor too); predictor kernel 1
    ("h64", Case(_cfg(128, 2, 320, 1, (5, 9), (1, 64, 1), (3, 128, 3), (1, 64, 3), (2, 320, 3)))),
    # heads of 64 at D = 256 / H = 4; FFN of 5 taps; depthwise 15 / 17; equal predictors of 128
    # channels (batched first conv and grouped LayerNorm below 256 channels); a one-layer postnet;
    # the speaker-embedding projection at D = 256
    ("h64x4", Case(_cfg(256, 4, 512, 5, (15, 17), (2, 128, 3), (2, 128, 3), (2, 128, 3), (1, 256, 5), spk=32))),
    # heads of 48 (the generic V transpose, attention GEMMs at K = 48) at D = 192; the compiled
    # depthwise 7 / 31 at a new D; the default predictor plan (pitch 5 taps against 3: the batched
    # conv's zero-padded taps) with three pitch layers
    ("h48", Case(_cfg(192, 4, 384, 3, (7, 31), (2, 256, 3), (3, 256, 5), (2, 256, 3), (2, 256, 5)))),
    # heads of 96 (K = 96) at D = 384 / H = 4; two encoder layers; decoder FFN narrower than the
    # encoder's (640 / 320: H1 is sized for the wider); equal predictors of 64 channels and one tap;
    # a 512-unit postnet of 3 taps (the widest the envelope takes)
    ("h96", Case(_cfg(384, 4, 640, 3, (9, 5), (2, 64, 1), (2, 64, 1), (2, 64, 1), (2, 512, 3), enc_layers=2),
                 decoder_linear_units=320)),
    # one head of 192 at D = 192: the fused relative-position attention at H = 1; depthwise 11 / 21;
    # a one-layer pitch predictor beside deeper ones of the same width (batch_predictors declines)
    ("h192", Case(_cfg(192, 1, 768, 3, (11, 21), (3, 96, 3), (1, 96, 3), (2, 96, 3), (1, 256, 3)))),
    # heads of 256 at D = 512: LayerNorm rows of 512 channels (layernorm_kernel<T, 8> in fp32), the
    # top of the envelope; transpose_v16 at 256; attention GEMMs at K = 256
    ("h256", Case(_cfg(512, 2, 1024, 3, (7, 31), (2, 256, 3), (2, 256, 3), (2, 256, 3), (2, 256, 5)))),
    # heads of 128 at D = 256; FFN of one tap narrower than the hidden size (192); depthwise 3 / 3;
    # unequal predictor widths at equal depth (64 / 128 / 64: batch_predictors declines on the
    # channel count alone, pitch wider than duration); a 384-unit postnet
    ("h128", Case(_cfg(256, 2, 192, 1, (3, 3), (2, 64, 3), (2, 128, 3), (2, 64, 3), (2, 384, 3)))),
    # two layers in both stacks at D = 128; FFN of 5 taps; three-layer predictors of equal width
    # (batched first conv, then two more layers each); a three-layer postnet
    ("deep", Case(_cfg(128, 2, 256, 5, (9, 5), (3, 128, 3), (3, 128, 3), (3, 128, 3), (3, 128, 5),
                       enc_layers=2, dec_layers=2))),
])

DTYPES16 = ("f16", "bf16")
FUSED_ATTN = ("h192",)      # head size 192: the fused relative-position attention
SPLIT_ENC_CASES = ("h64", "h256")   # also run with the all-fp32-MFMA encoder (TTS_F32_ENC_SPLIT=0)
DUR16_CASES = ("h48", "h64x4")      # 16-bit predicted durations on the exact encoder
FAST_CASE = "h96"                   # encoder_precision="fast"

# ------------------------------------------------------------------------------------------ inputs
# The ragged batch: the token counts sit on both sides of the 32- and 64-row tile edges of the
# encoder; three frames per token (a few tokens zero) put the frame counts on both sides of the
# decoder's 32-row (93 / 96 / 99), 64-row (186 / 195 around 192) and 128-row (99 / 129) edges; an
# eighth utterance of 43 tokens is there for the 129 (one row into a second 128-row tile).
TOKENS = (1, 2, 31, 32, 33, 64, 65, 43)
ZERO_TOKENS = {1: (0,), 5: (10, 63)}   # utterance -> tokens of duration 0 (a first and a last token among them)
FRAMES = (3, 3, 93, 96, 99, 186, 195, 129)
T_CAP = 224   # a multiple of 32: the 16-bit decoder's row stride rup(Td, 32) with no pad row
PRED_TOKENS = (20, 7, 1, 12)    # the smaller batch with predicted durations
MARGIN = 1e-2                   # every token's exp(x) - 1 at least this far from a .5 boundary
GOLDEN_TOKENS = 10


def _seed(name):
    return 2000 + list(CASES).index(name)


def ragged_inputs(name):
    """-> (ids, durations): lists of int64 arrays, one per utterance."""
    rng = np.random.default_rng(_seed(name))
    V = CASES[name].cfg.vocab_size
    ids = [rng.integers(1, V, size=n) for n in TOKENS]
    durs = []
    for b, n in enumerate(TOKENS):
        d = np.full(n, 3, np.int64)
        d[list(ZERO_TOKENS.get(b, ()))] = 0
        durs.append(d)
    return ids, durs


def speaker_embeddings(name, n):
    """[n, E] float32, not unit norm (the normalisation matters), or None for a single-speaker case."""
    E = CASES[name].cfg.speaker_embed_dim
    if not E:
        return None
    return (3.0 * np.random.default_rng(_seed(name) + 700).standard_normal((n, E))).astype(np.float32)


_CACHE = {}


def weights(name):
    from gonova_tts_amd.weights import make_acoustic_weights
    if ("w", name) not in _CACHE:
        c = CASES[name]
        w = make_acoustic_weights(0, c.cfg)
        if c.dec_units != c.cfg.linear_units:
            # every tensor is drawn from its own generator seeded by its name, so the decoder
            # layers of the configuration with the other FFN width are the same draws reshaped
            wd = make_acoustic_weights(0, replace(c.cfg, linear_units=c.dec_units))
            for k in w:
                if k.startswith("decoder."):
                    w[k] = wd[k]
        _CACHE["w", name] = w
    return _CACHE["w", name]


def oracle64(name):
    """Float64 oracle outputs (acoustic_forward's dict) of the ragged batch with its durations
    forced, one per utterance; computed once per session and shared (read-only)."""
    from oracle.acoustic import acoustic_forward
    key = ("ref", name)
    if key not in _CACHE:
        ids, durs = ragged_inputs(name)
        spk = speaker_embeddings(name, len(ids))
        refs = [acoustic_forward(x, weights(name), CASES[name].cfg, durations=d, dtype=np.float64,
                                 speaker_embedding=None if spk is None else spk[b])
                for b, (x, d) in enumerate(zip(ids, durs))]
        for r in refs:
            for v in r.values():
                v.setflags(write=False)
        _CACHE[key] = refs
    return _CACHE[key]


def log_durations(name, ids, dtype, spk=None):
    """The oracle's encoder, speaker projection and duration predictor only (HF:1171-1208)."""
    from oracle.acoustic import conformer_stack, variance_predictor
    cfg = CASES[name].cfg
    w = {k: np.asarray(v, dtype) for k, v in weights(name).items()}
    x = conformer_stack(w["encoder.embed.weight"][np.asarray(ids, np.int64)], w, "encoder.", cfg.encoder_layers,
                        cfg.num_attention_heads)
    if spk is not None:
        e = np.asarray(spk, dtype)
        e = e / max(float(np.sqrt((e.astype(np.float64) ** 2).sum())), 1e-12)
        x = np.concatenate([x, np.broadcast_to(e, (x.shape[0], e.shape[0]))], axis=1) @ w["projection.weight"].T \
            + w["projection.bias"]
    return variance_predictor(x, w, "duration_predictor.", cfg.duration_predictor_layers)


def margin(logd):
    """distance of exp(x) - 1 from the nearest .5 rounding boundary, per token"""
    return np.abs((np.exp(np.asarray(logd, np.float64)) - 1) % 1 - 0.5)


def _safe_ids(name, n, salt, spk=None):
    """n token ids whose oracle durations are all at least 2 MARGIN from a rounding boundary in
    float32 and float64: the first of a fixed sequence of draws that is (the CPU test asserts
    MARGIN on the result)."""
    V = CASES[name].cfg.vocab_size
    for attempt in range(400):
        ids = np.random.default_rng([_seed(name), salt, attempt]).integers(1, V, size=n)
        if all(margin(log_durations(name, ids, dt, spk)).min() > 2 * MARGIN for dt in (np.float32, np.float64)):
            return ids
    raise AssertionError(f"no draw of {n} tokens clear of the rounding boundaries for {name}")


def predicted_inputs(name):
    """-> ids (list of int64 arrays) of the predicted-duration batch."""
    key = ("pred", name)
    if key not in _CACHE:
        spk = speaker_embeddings(name, len(PRED_TOKENS))
        _CACHE[key] = [_safe_ids(name, n, 1 + b, None if spk is None else spk[b]) for b, n in enumerate(PRED_TOKENS)]
    return _CACHE[key]


def predicted_oracle64(name):
    """Float64 oracle outputs of the predicted-duration batch (durations predicted)."""
    from oracle.acoustic import acoustic_forward
    key = ("pref", name)
    if key not in _CACHE:
        ids = predicted_inputs(name)
        spk = speaker_embeddings(name, len(ids))
        _CACHE[key] = [acoustic_forward(x, weights(name), CASES[name].cfg, dtype=np.float64,
                                        speaker_embedding=None if spk is None else spk[b]) for b, x in enumerate(ids)]
    return _CACHE[key]


def golden_ids(name):
    """The short utterance of the transformers golden (tests/golden/make_ac_cfg_golden.py)."""
    key = ("gold", name)
    if key not in _CACHE:
        spk = speaker_embeddings(name, 1)
        _CACHE[key] = _safe_ids(name, GOLDEN_TOKENS, 900, None if spk is None else spk[0])
    return _CACHE[key]


# ---------------------------------------------------------------------------------------- envelope
CONV_HALO_MAX = 64       # (taps - 1) * dilation of the implicit-GEMM kernels
DEPTHWISE_MAX_K = 129    # (128 + k - 1) rows x 64 channels of fp32 within 64 KiB of LDS
FFN_MAX, POSTNET_MAX, PRED_MAX = 2048, 512, 256
MEL_BINS = 80            # every forward writes [B][T][80]


def in_envelope(w):
    """The acoustic envelope of INTEGRATION.md restated over a weight dict: None when the model is
    inside, else the name of the first tensor outside."""
    def conv_ok(n, cin):
        s = w[n].shape
        return len(s) == 3 and s[1] == cin and s[1] % 8 == 0 and s[0] % 4 == 0 and s[2] % 2 == 1 and s[2] - 1 <= CONV_HALO_MAX

    V, D = w["encoder.embed.weight"].shape
    if D % 64 or D > 512:
        return "encoder.embed.weight"
    u0 = "encoder.conformer_layers.0.self_attn.pos_bias_u"
    H, dk = w[u0].shape
    if H * dk != D or dk % 16:
        return u0
    for st in ("encoder.", "decoder."):
        i = 0
        while f"{st}conformer_layers.{i}.self_attn.pos_bias_u" in w:
            p = f"{st}conformer_layers.{i}."
            if w[p + "self_attn.pos_bias_u"].shape != (H, dk):
                return p + "self_attn.pos_bias_u"
            k = w[p + "feed_forward.conv1.weight"].shape[2]
            for ff in ("feed_forward.", "feed_forward_macaron."):
                n1, n2 = p + ff + "conv1.weight", p + ff + "conv2.weight"
                if not conv_ok(n1, D) or w[n1].shape[0] > FFN_MAX or w[n1].shape[2] != k:
                    return n1
                if not conv_ok(n2, w[n1].shape[0]) or w[n2].shape[0] != D or w[n2].shape[2] != k:
                    return n2
            for n, co in ((p + "conv_module.pointwise_conv1.weight", 2 * D), (p + "conv_module.pointwise_conv2.weight", D)):
                if w[n].shape != (co, D, 1):
                    return n
            dw = w[p + "conv_module.depthwise_conv.weight"].shape
            if dw[:2] != (D, 1) or dw[2] % 2 == 0 or dw[2] > DEPTHWISE_MAX_K:
                return p + "conv_module.depthwise_conv.weight"
            i += 1
        if i == 0:
            return st + "conformer_layers.0.self_attn.pos_bias_u"
    for pr in ("pitch_predictor.", "energy_predictor.", "duration_predictor."):
        cin, i = D, 0
        while f"{pr}conv_layers.{i}.conv.weight" in w:
            n = f"{pr}conv_layers.{i}.conv.weight"
            if not conv_ok(n, cin) or w[n].shape[0] > PRED_MAX:
                return n
            cin, i = w[n].shape[0], i + 1
        if i == 0:
            return pr + "conv_layers.0.conv.weight"
    for e in ("pitch_embed.conv.weight", "energy_embed.conv.weight"):
        if w[e].shape != (D, 1, 1):
            return e
    if "projection.weight" in w and (w["projection.weight"].ndim != 2 or w["projection.weight"].shape[0] != D
                                     or w["projection.weight"].shape[1] <= D):
        return "projection.weight"
    fo = "speech_decoder_postnet.feat_out.weight"
    nmel = w[fo].shape[0]
    if w[fo].shape[1] != D or nmel != MEL_BINS:
        return fo
    cin, i = nmel, 0
    while f"speech_decoder_postnet.layers.{i}.conv.weight" in w:
        n = f"speech_decoder_postnet.layers.{i}.conv.weight"
        if not conv_ok(n, cin) or w[n].shape[0] > POSTNET_MAX:
            return n
        cin, i = w[n].shape[0], i + 1
    if i == 0 or cin != nmel:
        return f"speech_decoder_postnet.layers.{max(i - 1, 0)}.conv.weight"
    return None


def _weights(**kw):
    from gonova_tts_amd.weights import make_acoustic_weights
    return make_acoustic_weights(0, replace(CASES["h64"].cfg, **kw))


def edited(**tensors):
    """Case h64's weights with some tensors replaced by zeros of another shape."""
    w = dict(_weights())
    for k, shape in tensors.items():
        w[k.replace("__", ".")] = np.zeros(shape, np.float32)
    return w


def macaron_taps(k):
    """Case h64 with the macaron FFN of encoder layer 0 at another kernel size."""
    w, wk = dict(_weights()), _weights(positionwise_conv_kernel_size=k)
    for n in w:
        if n.startswith("encoder.conformer_layers.0.feed_forward_macaron."):
            w[n] = wk[n]
    return w


def mixed_stacks(enc_kw, dec_kw):
    """Encoder-side tensors of one configuration, decoder layers of another."""
    w, wd = _weights(**enc_kw), _weights(**dec_kw)
    return {k: (wd[k] if k.startswith("decoder.") else v) for k, v in w.items()}


# Configurations outside the envelope, one per limit (variations of case h64):
# name: (weights, the tensor the refusal names, words of the limit in the engine's message)
OUTSIDE = {
    "hidden_not_64": (lambda: _weights(hidden_size=96), "encoder.embed.weight", ["96", "multiple of 64"]),
    "hidden_above_512": (lambda: _weights(hidden_size=576), "encoder.embed.weight", ["576", "512"]),
    "head_not_16": (lambda: _weights(hidden_size=320, num_attention_heads=8),
                    "encoder.conformer_layers.0.self_attn.pos_bias_u", ["40", "multiple of 16"]),
    "decoder_heads": (lambda: mixed_stacks({}, dict(num_attention_heads=4)),
                      "decoder.conformer_layers.0.self_attn.pos_bias_u", ["[4][32]", "[2][64]"]),
    "decoder_hidden": (lambda: mixed_stacks({}, dict(hidden_size=256)),
                       "decoder.conformer_layers.0.self_attn.pos_bias_u", ["[2][128]", "[2][64]"]),
    "ffn_above_2048": (lambda: _weights(linear_units=2304), "encoder.conformer_layers.0.feed_forward.conv1.weight",
                       ["2304", "2048"]),
    "ffn_not_8": (lambda: _weights(linear_units=324), "encoder.conformer_layers.0.feed_forward.conv2.weight",
                  ["324", "multiple of 8"]),
    "ffn_even_taps": (lambda: _weights(positionwise_conv_kernel_size=2), "encoder.conformer_layers.0.feed_forward.conv1.weight",
                      ["kernel size 2", "odd"]),
    "ffn_halo": (lambda: _weights(positionwise_conv_kernel_size=67), "encoder.conformer_layers.0.feed_forward.conv1.weight",
                 ["66", "64"]),
    "depthwise_even": (lambda: _weights(encoder_kernel_size=8), "encoder.conformer_layers.0.conv_module.depthwise_conv.weight",
                       ["kernel size 8", "odd"]),
    "depthwise_lds": (lambda: _weights(decoder_kernel_size=131), "decoder.conformer_layers.0.conv_module.depthwise_conv.weight",
                      ["131", "129"]),
    "predictor_above_256": (lambda: _weights(pitch_predictor_channels=320), "pitch_predictor.conv_layers.0.conv.weight",
                            ["320", "256"]),
    "predictor_no_layer": (lambda: _weights(duration_predictor_layers=0), "duration_predictor.conv_layers.0.conv.weight",
                           ["at least one layer"]),
    "predictor_in_not_8": (lambda: _weights(pitch_predictor_channels=36), "pitch_predictor.conv_layers.1.conv.weight",
                           ["36", "multiple of 8"]),
    "predictor_out_not_4": (lambda: _weights(energy_predictor_channels=30), "energy_predictor.conv_layers.0.conv.weight",
                            ["30", "multiple of 4"]),
    "predictor_even_taps": (lambda: _weights(energy_predictor_kernel_size=4), "energy_predictor.conv_layers.0.conv.weight",
                            ["kernel size 4", "odd"]),
    "mel_bins_not_80": (lambda: _weights(num_mel_bins=88), "speech_decoder_postnet.feat_out.weight", ["88 mel bins", "[80]"]),
    "postnet_not_back_to_mel": (lambda: edited(**{"speech_decoder_postnet.layers.1.conv.weight": (76, 320, 3),
                                                  "speech_decoder_postnet.layers.1.batch_norm.weight": (76,),
                                                  "speech_decoder_postnet.layers.1.batch_norm.bias": (76,),
                                                  "speech_decoder_postnet.layers.1.batch_norm.running_mean": (76,),
                                                  "speech_decoder_postnet.layers.1.batch_norm.running_var": (76,)}),
                                "speech_decoder_postnet.layers.1.conv.weight", ["76 output channels", "80 mel bins"]),
    "heads_do_not_split_hidden": (lambda: edited(**{"encoder.conformer_layers.0.self_attn.pos_bias_u": (2, 48)}),
                                  "encoder.conformer_layers.0.self_attn.pos_bias_u", ["[2][48]", "128"]),
    "ffn_kernels_differ": (lambda: macaron_taps(3), "encoder.conformer_layers.0.feed_forward_macaron.conv1.weight",
                           ["kernel size 3", "has 1"]),
    "pointwise_not_2d": (lambda: edited(**{"decoder.conformer_layers.0.conv_module.pointwise_conv1.weight": (128, 128, 1)}),
                         "decoder.conformer_layers.0.conv_module.pointwise_conv1.weight", ["[256][128][1]"]),
    "projection_shape": (lambda: edited(**{"projection.weight": (128, 128), "projection.bias": (128,)}),
                         "projection.weight", ["[128][128 + E]"]),
    "pitch_embed_taps": (lambda: edited(**{"pitch_embed.conv.weight": (128, 1, 3)}), "pitch_embed.conv.weight",
                         ["[128][1][3]", "kernel size of 1"]),
    "postnet_above_512": (lambda: _weights(postnet_units=576), "speech_decoder_postnet.layers.0.conv.weight", ["576", "512"]),
    "postnet_halo": (lambda: _weights(postnet_kernel=67), "speech_decoder_postnet.layers.0.conv.weight", ["66", "64"]),
    "postnet_no_layer": (lambda: _weights(postnet_layers=0), "speech_decoder_postnet.layers.0.conv.weight",
                         ["at least one layer"]),
}
