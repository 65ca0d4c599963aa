"""The small non-V1 vocoder configurations (tests/vocoder_cases.py) on the CPU: the oracle
against transformers goldens, the storage-rounding model that bounds the 16-bit GPU tests, and
the sensitivity of that bound to injected defects.  No GPU."""
import os

import numpy as np
import pytest

import vocoder_cases as vc
from oracle.vocoder import vocoder_forward
from oracle.vocoder_rounded import ROUND, round_bf16, round_f16, vocoder_forward_rounded
from parity import max_abs, rel_rms

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_cfg.npz"))
NAMES = list(vc.CASES)


def test_case_lengths_cover_tile_edges():
    for name, cfg in vc.CASES.items():
        lens = vc.ragged_lens(name)
        assert lens[:3] == [0, 1, 2]
        assert lens[4] * cfg.hop % vc.TILE_ROWS == 0 and lens[3] + 1 == lens[4] == lens[5] - 1
        assert max(lens) * cfg.hop >= 1100
        assert cfg.stage_channels(len(cfg.upsample_rates) - 1) == 32 and cfg.model_in_dim == 80
    for name, r in vc.SWEEP.items():
        rows = [f * vc.CASES[name].hop for f in r]
        assert len(rows) == 40 and rows[0] < vc.TILE_ROWS < rows[-1]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_transformers_golden(name):
    """vocoder_forward in float32 and float64 against transformers' module built from the same
    configuration (tests/golden/make_cfg_golden.py)."""
    cfg, w, mel = vc.CASES[name], vc.weights(name), G[f"{name}_mel"]
    np.testing.assert_array_equal(mel, vc.golden_mel(name))
    o32 = vocoder_forward(mel, w, cfg, np.float32)
    o64 = vocoder_forward(mel, w, cfg, np.float64)
    assert o32.shape == G[f"{name}_wav32"].shape == (mel.shape[0] * cfg.hop,)
    np.testing.assert_allclose(o32, G[f"{name}_wav32"], atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(o64, G[f"{name}_wav64"], atol=1e-12, rtol=1e-10)


def test_rounding_functions_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -10), 0.1, 0.0])
    np.testing.assert_array_equal(round_f16(x), [1.0, 1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), float(np.float16(0.1)), 0.0])
    y = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, -3.0, 0.0])
    np.testing.assert_array_equal(round_bf16(y), [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0])
    import torch
    z = np.random.default_rng(0).standard_normal(4096)
    np.testing.assert_array_equal(round_bf16(z), torch.from_numpy(z).to(torch.bfloat16).double().numpy())


@pytest.mark.parametrize("dtype", vc.DTYPES16)
@pytest.mark.parametrize("name", NAMES)
def test_rounding_model_error_is_inside_the_stated_bars(name, dtype):
    """The error 16-bit storage must cause: finite, non-zero, and below the project's stated bars
    (relative RMS 5e-3 in f16, 2.5e-2 in bf16) on every case."""
    e, m = vc.model_error(name, dtype)
    print(f"[model] {name} {dtype}: rel_rms {e:.3e} max_abs {m:.3e}")
    assert np.isfinite(e) and np.isfinite(m) and e > 0 and m > 0
    assert e < (5e-3 if dtype == "f16" else 2.5e-2)


# ---------------------------------------------------------------------------------------------
# Sensitivity of the GPU tests' 16-bit bound (3x the rounding model's error, vc.bound): defects
# injected into the rounding model on case `two`, utterance of 385 frames (1,540 last-stage rows).
DEFECT_CASE = "two"


def _defects():
    w = vc.weights(DEFECT_CASE)
    ch = int(np.abs(w["upsampler.1.bias"]).argmax())
    return {
        # one output row of one pair zeroed where a 512-row tile ends (C = 32, k = 11, d = 3)
        "zero_row": dict(kind="zero_row", stage=1, block=2, pair=1, row=vc.TILE_ROWS),
        # conv1 of one pair lacks its first tap on the utterance's last row (C = 64, k = 3, d = 3)
        "drop_tap": dict(kind="drop_tap", stage=0, block=0, pair=1, tap=0),
        # one pair's conv1 at dilation 4 instead of 3 (C = 64, k = 3)
        "dilation": dict(kind="dilation", stage=0, block=0, pair=1),
        # the second upsampler's bias omitted for one channel (its largest) in output phase 1
        "up_bias": dict(kind="up_bias", stage=1, phase=1, channel=ch),
    }


def _defect_errors(dtype, defect):
    mel, lens = vc.ragged_mel(DEFECT_CASE)
    b = len(lens) - 1
    got = vocoder_forward_rounded(mel[b, :lens[b]], vc.weights(DEFECT_CASE), vc.CASES[DEFECT_CASE], dtype, defect=defect)
    ref = vc.oracle64(DEFECT_CASE)[b]
    return rel_rms(got, ref), max_abs(got, ref)


def _rejected(dtype, defect):
    e, m = _defect_errors(dtype, defect)
    be, bm = vc.bound(DEFECT_CASE, dtype)
    print(f"[defect] {dtype} {defect and defect['kind']}: rel_rms {e:.3e} (bound {be:.3e}) max_abs {m:.3e} (bound {bm:.3e})")
    return e > be or m > bm


@pytest.mark.parametrize("dtype", vc.DTYPES16)
def test_bound_accepts_the_clean_model(dtype):
    assert not _rejected(dtype, None)


@pytest.mark.parametrize("kind", ["zero_row", "drop_tap", "dilation", "up_bias"])
def test_f16_bound_rejects_defect(kind):
    assert _rejected("f16", _defects()[kind])


def test_bf16_bound_catches_only_the_coarse_defects():
    """The bf16 bound is ~8x looser: it still rejects the zeroed row and the wrong dilation (a
    local error of 1e-2, a relative RMS of 5e-2), but neither the omitted bias of one channel in
    one phase nor the dropped tap, which sit under bf16's own storage error.  The f16 run of the
    same case is what catches the omitted bias.  (The fp32 run does not stand in for either: it
    launches none of the 16-bit fused kernels.)"""
    d = _defects()
    assert _rejected("bf16", d["zero_row"]) and _rejected("bf16", d["dilation"])
    assert not _rejected("bf16", d["up_bias"]) and not _rejected("bf16", d["drop_tap"])


def test_single_tap_defect_sensitivity_is_reported():
    """One tap missing on one row is at the sensitivity limit of an end-to-end 16-bit bound: the
    placement chosen above is one the f16 bound rejects, but of the tap positions of the last
    stage's pairs that read a row inside the utterance it rejects only some (the count is printed,
    not asserted: a tighter bound may catch more).  Each of them moves the unrounded waveform by
    far more than the fp32 bar (atol 1e-5, rtol 1e-4), so the same mistake in the fp32 conv
    kernels is caught by the fp32 GPU run.  That run launches no pair, chain or streaming kernel,
    though: a tap dropped on one row inside those 16-bit kernels is covered only where the f16
    bound is sensitive enough, and by the bit-for-bit comparisons between the fused paths."""
    cfg, w = vc.CASES[DEFECT_CASE], vc.weights(DEFECT_CASE)
    mel, lens = vc.ragged_mel(DEFECT_CASE)
    b = len(lens) - 1
    ref = vc.oracle64(DEFECT_CASE)[b]
    be, bm = vc.bound(DEFECT_CASE, "f16")
    caught16 = total = 0
    for blk, k in enumerate(cfg.resblock_kernel_sizes):
        for pr in range(len(cfg.resblock_dilation_sizes[blk])):
            for tap in range(k // 2 + 1):  # later taps read the zero padding past the last row
                d = dict(kind="drop_tap", stage=1, block=blk, pair=pr, tap=tap)
                x = vocoder_forward_rounded(mel[b, :lens[b]], w, cfg, "f64", defect=d)
                assert np.any(np.abs(x - ref) > 1e-5 + 1e-4 * np.abs(ref)), d
                y = vocoder_forward_rounded(mel[b, :lens[b]], w, cfg, "f16", defect=d)
                caught16 += rel_rms(y, ref) > be or max_abs(y, ref) > bm
                total += 1
    print(f"[defect] single-tap placements in stage 1: f16 bound rejects {caught16} of {total}")


def test_unrounded_model_is_the_oracle():
    mel, lens = vc.ragged_mel("v3ish")
    got = vocoder_forward_rounded(mel[1, :lens[1]], vc.weights("v3ish"), vc.CASES["v3ish"], "f64")
    np.testing.assert_allclose(got, vc.oracle64("v3ish")[1], atol=1e-14, rtol=1e-12)
    assert set(ROUND) == {"f16", "bf16", "f64"}
