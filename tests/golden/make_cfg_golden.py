"""Generate golden vectors for the small non-V1 vocoder configurations from transformers 5.15.0
(run on a CPU box that has transformers; the tests read only the .npz).

For every case of tests/vocoder_cases.py the engine's seeded weights for that configuration are
loaded into transformers' `FastSpeech2ConformerHifiGan` built from the same configuration, and one
short mel goes through it in float32 and in float64 (B = 1).  A case whose channel plan is not a
halving (`odd`) gets its later layers rebuilt with the planned channel counts: the module's
forward only walks its layer lists.

Output: tests/golden/golden_cfg.npz (per case: mel, float32 and float64 waveforms).
Usage:  python tests/golden/make_cfg_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from gonova_tts_amd.weights import make_vocoder_weights  # noqa: E402
import vocoder_cases as vc  # noqa: E402


def hf_module(cfg):
    from transformers import FastSpeech2ConformerHifiGan, FastSpeech2ConformerHifiGanConfig
    from transformers.models.fastspeech2_conformer.modeling_fastspeech2_conformer import HifiGanResidualBlock
    hc = FastSpeech2ConformerHifiGanConfig(
        model_in_dim=cfg.model_in_dim, upsample_initial_channel=cfg.upsample_initial_channel,
        upsample_rates=list(cfg.upsample_rates), upsample_kernel_sizes=list(cfg.upsample_kernel_sizes),
        resblock_kernel_sizes=list(cfg.resblock_kernel_sizes),
        resblock_dilation_sizes=[list(d) for d in cfg.resblock_dilation_sizes],
        leaky_relu_slope=cfg.leaky_relu_slope, normalize_before=cfg.normalize_before)
    m = FastSpeech2ConformerHifiGan(hc)
    plan = [cfg.stage_channels(i) for i in range(len(cfg.upsample_rates))]
    if plan != [cfg.upsample_initial_channel // 2 ** (i + 1) for i in range(len(plan))]:
        cin = cfg.upsample_initial_channel
        ups, res = nn.ModuleList(), nn.ModuleList()
        for ch, u, k in zip(plan, cfg.upsample_rates, cfg.upsample_kernel_sizes):
            ups.append(nn.ConvTranspose1d(cin, ch, kernel_size=k, stride=u, padding=(k - u) // 2))
            for ks, dil in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
                res.append(HifiGanResidualBlock(ch, ks, tuple(dil), cfg.leaky_relu_slope))
            cin = ch
        m.upsampler, m.resblocks = ups, res
        m.conv_post = nn.Conv1d(cin, 1, kernel_size=7, stride=1, padding=3)
    return m.eval()


def main():
    torch.manual_seed(0)
    out = {}
    for name, cfg in vc.CASES.items():
        w = make_vocoder_weights(seed=0, cfg=cfg)
        mel = vc.golden_mel(name)
        m = hf_module(cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        with torch.no_grad():
            w32 = m(torch.from_numpy(mel)[None]).numpy()[0]
            w64 = m.double()(torch.from_numpy(mel).double()[None]).numpy()[0]
        assert w32.shape == (mel.shape[0] * cfg.hop,), (name, w32.shape)
        out[f"{name}_mel"] = mel
        out[f"{name}_wav32"] = w32.astype(np.float32)
        out[f"{name}_wav64"] = w64.astype(np.float64)
    path = os.path.join(HERE, "golden_cfg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
