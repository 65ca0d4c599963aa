"""ORACLE (test infrastructure only) -- the float64 vocoder oracle with 16-bit storage rounding.

`vocoder_forward_rounded` is `oracle.vocoder.vocoder_forward` in float64 with tensors rounded to
f16 or bf16 (round to nearest even) at exactly the places the engine stores 16-bit values:

  the (normalised) mel; the weights (biases stay fp32); the activated conv_pre output; each
  upsampler output; t inside a ResBlock pair; each pair's h'; the running MRF sum after each
  resblock; the scaled stage sum.  conv_post and tanh run unrounded.

All sums are exact (float64), so its distance from the float64 oracle is the error 16-bit storage
must cause, derived from the reference alone: the GPU parity tests bound the kernels by a small
multiple of it (tests/test_vocoder_configs_gpu.py) instead of by numbers the kernels produced.

`defect=` injects one wrong step into the model (tests/test_vocoder_configs_cpu.py checks that the
GPU tests' bound would reject each of them); it is never set when the model serves as a bound.
"""
from __future__ import annotations

import numpy as np

from .vocoder import conv1d, conv_transpose1d, leaky_relu


def round_f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def round_bf16(x):
    """float64 -> bfloat16 (8 significand bits), round to nearest even, straight from the float64
    bits (no double rounding through float32); values stay far inside bf16's exponent range."""
    b = np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)
    drop = np.uint64(52 - 7)
    lsb = (b >> drop) & np.uint64(1)
    b = (b + lsb + np.uint64((1 << 44) - 1)) & ~np.uint64((1 << 45) - 1)
    return b.view(np.float64)


ROUND = {"f16": round_f16, "bf16": round_bf16, "f64": lambda x: np.asarray(x, np.float64)}  # f64: no rounding


def _conv1d_drop(x, w, b, dilation, padding, drop_tap):
    """conv1d whose last output row lacks tap `drop_tap` (defect "drop_tap")."""
    y = conv1d(x, w, b, dilation=dilation, padding=padding)
    src = (y.shape[0] - 1) + drop_tap * dilation - padding  # input row that tap reads for the last row
    if 0 <= src < x.shape[0]:
        y[-1] -= x[src] @ w[:, :, drop_tap].T
    return y


def vocoder_forward_rounded(mel, weights, cfg=None, dtype="f16", defect=None):
    """One utterance, mel [T, 80] -> waveform [T * hop] float64.

    defect: None, or a dict with "kind" and the place (stage i, resblock j, pair q):
      {"kind": "zero_row", "stage", "block", "pair", "row"}: that pair's h' row zeroed
      {"kind": "drop_tap", "stage", "block", "pair", "tap"}: conv1 of that pair lacks one tap on the
          utterance's last row
      {"kind": "dilation", "stage", "block", "pair"}: that pair's conv1 runs at dilation d + 1
      {"kind": "up_bias", "stage", "phase", "channel"}: that upsampler's bias omitted for one
          channel in one output phase (rows with (row + padding) % stride == phase)
    """
    from gonova_tts_amd.config import VocoderConfig  # config only
    cfg = cfg or VocoderConfig()
    rnd = ROUND[dtype]
    f8 = np.float64
    d = defect or {}
    W = {k: (v.astype(f8) if k.endswith("bias") or k in ("mean", "scale") else rnd(v)) for k, v in weights.items()}
    x = np.asarray(mel, f8)
    if x.shape[0] == 0:
        return np.zeros((0,), f8)
    if cfg.normalize_before:
        x = (x - W["mean"]) / W["scale"]
    x = rnd(x)
    slope = cfg.leaky_relu_slope
    # conv_pre is stored activated (the first upsampler's LeakyReLU in its epilogue)
    x = rnd(leaky_relu(conv1d(x, W["conv_pre.weight"], W["conv_pre.bias"], padding=3), slope))
    nk = len(cfg.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        if i > 0:
            x = leaky_relu(x, slope)
        pad = (k - u) // 2
        y = conv_transpose1d(x, W[f"upsampler.{i}.weight"], W[f"upsampler.{i}.bias"], stride=u, padding=pad)
        if d.get("kind") == "up_bias" and d["stage"] == i:
            rows = (np.arange(y.shape[0]) + pad) % u == d["phase"]
            y[rows, d["channel"]] -= W[f"upsampler.{i}.bias"][d["channel"]]
        x = rnd(y)
        acc = None
        for j, (ks, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            pre = f"resblocks.{i * nk + j}"
            h = x
            for q, dil in enumerate(dils):
                here = d and d.get("stage") == i and d.get("block") == j and d.get("pair") == q
                w1, b1 = W[f"{pre}.convs1.{q}.weight"], W[f"{pre}.convs1.{q}.bias"]
                w2, b2 = W[f"{pre}.convs2.{q}.weight"], W[f"{pre}.convs2.{q}.bias"]
                d1 = dil + 1 if here and d["kind"] == "dilation" else dil
                g = leaky_relu(h, slope)
                if here and d["kind"] == "drop_tap":
                    t = _conv1d_drop(g, w1, b1, d1, (ks * d1 - d1) // 2, d["tap"])
                else:
                    t = conv1d(g, w1, b1, dilation=d1, padding=(ks * d1 - d1) // 2)
                t = rnd(leaky_relu(t, slope))
                hn = rnd(conv1d(t, w2, b2, dilation=1, padding=(ks - 1) // 2) + h)
                if here and d["kind"] == "zero_row":
                    hn[d["row"]] = 0.0
                h = hn
            acc = h if acc is None else rnd(acc + h)
        x = rnd(acc / nk) if nk > 1 else acc
    x = leaky_relu(x, 0.01)
    x = conv1d(x, W["conv_post.weight"], W["conv_post.bias"], padding=3)
    return np.tanh(x)[:, 0]
