"""Small HiFi-GAN configurations other than V1, shared by the vocoder-configuration tests
(test_vocoder_configs_cpu.py, test_vocoder_configs_gpu.py, golden/make_cfg_golden.py).

The engine reads channel counts, kernel sizes and the number of stages from the weight shapes and
the strides / dilations from the configuration, and its kernels are compiled for more than the one
configuration the benchmark runs.  Each case here is one or two stages deep, so the oracle sits one
or two kernels away from the waveform and costs milliseconds.  Every case keeps the envelope the
conv_post kernels have: 80 mel bins, conv_pre / conv_post of 7 taps, a last stage of 32 channels.

A plain helper module (no fixtures): cases, their lengths, and the mel inputs.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from gonova_tts_amd.config import VocoderConfig

V1_K = (3, 7, 11)
V1_D = ((1, 3, 5), (1, 3, 5), (1, 3, 5))


@dataclass
class PlannedVocoderConfig(VocoderConfig):
    """A VocoderConfig whose stage channel counts are listed instead of halved."""
    channel_plan: Tuple[int, ...] = ()

    def stage_channels(self, i: int) -> int:
        return self.channel_plan[i]


def _cfg(c0, rates, kernels, rk=V1_K, rd=V1_D):
    return VocoderConfig(upsample_initial_channel=c0, upsample_rates=rates, upsample_kernel_sizes=kernels,
                         resblock_kernel_sizes=rk, resblock_dilation_sizes=rd)


# name -> configuration; what each isolates is in the comment beside it
CASES = OrderedDict([
    # C = 32 chain k = 3 / 7, pair k = 11 with conv_post fused, streaming upsampler 64 -> 64 right after conv_pre
    ("one", _cfg(64, (2,), (4,))),
    # C = 64 chain and pairs, the stage-final stored activation, the C = 64 upsampler fused into the
    # last pair, streaming upsampler 128 -> 128
    ("two", _cfg(128, (2, 2), (4, 4))),
    # C = 256 / 128 pairs and the channel-split form, polyphase stride 2 at Cin = 512 / 256, the
    # C = 128 upsampler fusion
    ("four", _cfg(512, (2, 2, 2, 2), (4, 4, 4, 4))),
    # k = 5 pairs, two pairs per resblock (no chain), dilations 2, 6, 9, polyphase stride 4
    ("v3ish", _cfg(128, (4, 2), (8, 4), (3, 5, 7), ((1, 2), (2, 6), (3, 9)))),
    # 4 taps and 1 tap per phase, two resblocks per stage (1/2 scaling)
    ("taps41", _cfg(128, (2, 2), (8, 2), (3, 11), ((1, 3, 5), (1, 3, 5)))),
    # 3 taps per phase (then the 2-tap streaming upsampler), two resblocks per stage
    ("taps32", _cfg(128, (2, 2), (6, 4), (3, 11), ((1, 3, 5), (1, 3, 5)))),
    # one resblock per stage: no accumulation, scale 1
    ("nk1", _cfg(64, (2,), (4,), (7,), ((1, 3, 5),))),
    # channel counts no pair / X-resident kernel takes (96 -> 48), then the C = 32 kernels
    ("odd", PlannedVocoderConfig(upsample_initial_channel=96, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4),
                                 resblock_kernel_sizes=V1_K, resblock_dilation_sizes=V1_D, channel_plan=(48, 32))),
    # the streaming upsampler at stride 4 (128 -> 4 x 32 outputs per input row; the only other
    # stride its two compiled shapes can take inside the envelope)
    ("stream4", PlannedVocoderConfig(upsample_initial_channel=128, upsample_rates=(4,), upsample_kernel_sizes=(8,),
                                     resblock_kernel_sizes=V1_K, resblock_dilation_sizes=V1_D, channel_plan=(32,))),
    # the k = 5 pairs and dilations 2, 6, 9 at C = 256 / 128 too (whole and channel-split)
    ("v3four", _cfg(512, (2, 2, 2, 2), (4, 4, 4, 4), (3, 5, 7), ((1, 2), (2, 6), (3, 9)))),
])

DTYPES16 = ("f16", "bf16")

# The tallest tile of any kernel is 512 rows (the C = 32 pairs); it only motivates the lengths.
TILE_ROWS = 512
EDGE_ROWS = 3 * TILE_ROWS   # the ragged batch's long utterances sit on this last-stage row count
SWEEP = {"two": range(120, 160), "v3ish": range(60, 100)}  # 40 consecutive lengths across a tile edge


def ragged_lens(name):
    """0, 1, 2 frames, a length whose last-stage row count is a whole number of the tallest tile
    (1,536 rows: more than two tiles of every kernel), and that length -1 / +1 frame."""
    f = EDGE_ROWS // CASES[name].hop
    assert f * CASES[name].hop == EDGE_ROWS
    return [0, 1, 2, f - 1, f, f + 1]


def _seed(name):
    return 1000 + list(CASES).index(name)


def ragged_mel(name):
    """-> (mel [B, T, 80] float32, lens): every utterance its own draw."""
    lens = ragged_lens(name)
    rng = np.random.default_rng(_seed(name))
    return rng.standard_normal((len(lens), max(lens), 80)).astype(np.float32), lens


def sweep_mel(name):
    """-> (mel [40, T, 80] float32, lens): 40 utterances of consecutive lengths, prefixes of one mel."""
    lens = list(SWEEP[name])
    rng = np.random.default_rng(_seed(name) + 500)
    one = rng.standard_normal((max(lens), 80)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(one, (len(lens),) + one.shape)), lens


_CACHE = {}


def weights(name):
    from gonova_tts_amd.weights import make_vocoder_weights
    if ("w", name) not in _CACHE:
        _CACHE["w", name] = make_vocoder_weights(seed=0, cfg=CASES[name])
    return _CACHE["w", name]


def oracle64(name, kind="ragged"):
    """Float64 oracle waveforms of the case's ragged batch (or sweep), one per utterance; computed
    once per session and shared (read-only)."""
    from oracle.vocoder import vocoder_forward
    key = ("ref", name, kind)
    if key not in _CACHE:
        mel, lens = ragged_mel(name) if kind == "ragged" else sweep_mel(name)
        refs = [vocoder_forward(mel[b, :L], weights(name), CASES[name], np.float64) if L else np.zeros((0,))
                for b, L in enumerate(lens)]
        for r in refs:
            r.setflags(write=False)
        _CACHE[key] = refs
    return _CACHE[key]


BOUND_FACTOR = 3.0


def model_error(name, dtype):
    """(rel_rms, max_abs) of the storage-rounding model (oracle/vocoder_rounded.py) against the
    float64 oracle over the case's ragged batch: relative RMS pooled over its non-empty
    utterances, max-abs over all of them.  From the reference alone."""
    from oracle.vocoder_rounded import vocoder_forward_rounded
    key = ("model", name, dtype)
    if key not in _CACHE:
        mel, lens = ragged_mel(name)
        refs = oracle64(name)
        se = sr = mx = 0.0
        for b, L in enumerate(lens):
            if not L:
                continue
            e = vocoder_forward_rounded(mel[b, :L], weights(name), CASES[name], dtype) - refs[b]
            mx = max(mx, float(np.abs(e).max()))
            se += float((e ** 2).sum())
            sr += float((refs[b] ** 2).sum())
        _CACHE[key] = (float(np.sqrt(se / sr)), mx)
    return _CACHE[key]


def bound(name, dtype):
    """The 16-bit parity bound of a case, held on every non-empty utterance in both relative RMS
    and max-abs: BOUND_FACTOR x the rounding model's own error.  The
    kernels' accumulation order and the points where they keep fp32 differ from the model by a
    factor of order one (V1's recorded errors reach 1.8x the model)."""
    e, m = model_error(name, dtype)
    return BOUND_FACTOR * e, BOUND_FACTOR * m


def golden_mel(name):
    """The short mel of the transformers golden (tests/golden/make_cfg_golden.py)."""
    rng = np.random.default_rng(_seed(name) + 900)
    return rng.standard_normal((11, 80)).astype(np.float32)
