"""Generate golden vectors for the small non-default acoustic configurations from transformers
5.15.0 (run on a CPU box that has transformers; the tests read only the .npz).

For every case of tests/acoustic_cases.py the engine's seeded weights for that configuration are
loaded into transformers' `FastSpeech2ConformerModel` built from the same configuration, and one
short utterance (about 10 tokens, B = 1) goes through it in float32 and in float64.  The project's
configuration has one field for the attention heads of both stacks, and one for the FFN width;
transformers has `encoder_*` and `decoder_*` fields for each: the heads go to both, the FFN width
to `encoder_linear_units`, and a case's `decoder_linear_units` (else the same width) to
`decoder_linear_units`.  A case with a speaker embedding passes one.

The float32 run is transformers as it is.  Two places of its model stay float32 whatever the
module's dtype, so the float64 run replaces them: `length_regulator` allocates its output as
float32 (the float64 model would not run; the replacement repeats the rows in the working dtype),
and the relative-position table is built in float32.  The replacement table is transformers'
formula (`extend_pos_enc`) written out here in torch, with the frequencies and the angles rounded
to float32 as there and the sines and cosines taken in float64.  The frequencies are the correctly
rounded float32 exp (torch's float32 `exp` is one ulp off on a few of them, which the float32
golden's tolerance absorbs and the float64 one, 1e-12, would not).  Nothing of the float64 golden
comes from `oracle/`.

Output: tests/golden/golden_ac_cfg.npz (per case: token ids, durations, float32 and float64 mel).
Usage:  python tests/golden/make_ac_cfg_golden.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import acoustic_cases as ac  # noqa: E402


def hf_module(case):
    from transformers import FastSpeech2ConformerConfig, FastSpeech2ConformerModel
    c = case.cfg
    hc = FastSpeech2ConformerConfig(
        hidden_size=c.hidden_size, vocab_size=c.vocab_size, num_mel_bins=c.num_mel_bins,
        encoder_num_attention_heads=c.num_attention_heads, decoder_num_attention_heads=c.num_attention_heads,
        encoder_layers=c.encoder_layers, decoder_layers=c.decoder_layers,
        encoder_linear_units=c.linear_units, decoder_linear_units=case.dec_units,
        positionwise_conv_kernel_size=c.positionwise_conv_kernel_size,
        encoder_kernel_size=c.encoder_kernel_size, decoder_kernel_size=c.decoder_kernel_size,
        duration_predictor_layers=c.duration_predictor_layers, duration_predictor_channels=c.duration_predictor_channels,
        duration_predictor_kernel_size=c.duration_predictor_kernel_size,
        pitch_predictor_layers=c.pitch_predictor_layers, pitch_predictor_channels=c.pitch_predictor_channels,
        pitch_predictor_kernel_size=c.pitch_predictor_kernel_size,
        energy_predictor_layers=c.energy_predictor_layers, energy_predictor_channels=c.energy_predictor_channels,
        energy_predictor_kernel_size=c.energy_predictor_kernel_size,
        speech_decoder_postnet_layers=c.postnet_layers, speech_decoder_postnet_units=c.postnet_units,
        speech_decoder_postnet_kernel=c.postnet_kernel, speaker_embed_dim=c.speaker_embed_dim)
    return FastSpeech2ConformerModel(hc).eval()


def regulate_keeping_dtype(encoded_embeddings, duration_labels, speaking_speed=1.0):
    """transformers' length_regulator (B = 1, speed 1) without its float32 output buffer"""
    assert speaking_speed == 1.0 and encoded_embeddings.size(0) == 1
    if duration_labels.sum() == 0:
        duration_labels[duration_labels.sum(dim=1).eq(0)] = 1
    return torch.repeat_interleave(encoded_embeddings[0], duration_labels[0], dim=0)[None]


def pos_table64(length, d_model):
    """extend_pos_enc of FastSpeech2ConformerRelPositionalEncoding with float64 sines:
    [1][2 L - 1][D], relative positions L-1 .. -(L-1)."""
    position = torch.arange(0, length, dtype=torch.int64).float().unsqueeze(1)
    arg = torch.arange(0, d_model, 2, dtype=torch.int64).float() * -(math.log(10000.0) / d_model)
    div_term = torch.exp(arg.double()).float()   # the float32 frequencies, correctly rounded
    angle = (position * div_term).double()       # the float32 products
    positive = torch.zeros(length, d_model, dtype=torch.float64)
    negative = torch.zeros(length, d_model, dtype=torch.float64)
    positive[:, 0::2], positive[:, 1::2] = torch.sin(angle), torch.cos(angle)
    negative[:, 0::2], negative[:, 1::2] = torch.sin(-1 * angle), torch.cos(-1 * angle)
    return torch.cat([torch.flip(positive, [0]).unsqueeze(0), negative[1:].unsqueeze(0)], dim=1)


def to_float64(m, max_len=64):
    """The module in float64, with the two float32 places above replaced."""
    from transformers.models.fastspeech2_conformer import modeling_fastspeech2_conformer as mod
    m = m.double()
    mod.length_regulator = regulate_keeping_dtype  # (main puts transformers' own back after the run)
    for stack in (m.encoder, m.decoder):
        stack.pos_enc.pos_enc = pos_table64(max_len, m.config.hidden_size)  # (extend_pos_enc keeps a table that is long enough)
    return m


def main():
    from transformers.models.fastspeech2_conformer import modeling_fastspeech2_conformer as mod
    hf_regulator = mod.length_regulator
    torch.manual_seed(0)
    out = {}
    for name, case in ac.CASES.items():
        m = hf_module(case)
        sd = {k: torch.from_numpy(v) for k, v in ac.weights(name).items()}
        for k, v in m.state_dict().items():  # BatchNorm counters are not weights; keep HF's
            if k.endswith("num_batches_tracked"):
                sd[k] = v
        m.load_state_dict(sd, strict=True)
        ids = ac.golden_ids(name)
        spk = ac.speaker_embeddings(name, 1)
        kw = {} if spk is None else {"speaker_embedding": torch.from_numpy(spk[:1])}
        with torch.no_grad():
            o32 = m(torch.from_numpy(ids)[None], return_dict=True, **kw)
            m = to_float64(m)
            if spk is not None:
                kw = {"speaker_embedding": torch.from_numpy(spk[:1]).double()}
            o64 = m(torch.from_numpy(ids)[None], return_dict=True, **kw)
        mod.length_regulator = hf_regulator
        d32, d64 = o32.duration_outputs.numpy()[0], o64.duration_outputs.numpy()[0]
        assert np.array_equal(d32, d64), (name, d32, d64)
        out[f"{name}_ids"] = ids.astype(np.int64)
        out[f"{name}_dur"] = d32.astype(np.int64)
        out[f"{name}_mel32"] = o32.spectrogram.numpy()[0].astype(np.float32)
        out[f"{name}_mel64"] = o64.spectrogram.numpy()[0].astype(np.float64)
        if spk is not None:
            out[f"{name}_emb"] = spk[0]
    path = os.path.join(HERE, "golden_ac_cfg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
