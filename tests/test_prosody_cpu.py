"""What the prosody tests' bounds accept and reject, and the host side of the controls, without a
GPU: the NumPy restatement (prosody_cases.py) under each wrong implementation misses the bound the
GPU test applies to the kernel; every control setting the model-level GPU tests use moves the
oracle mel at least ten times the loosest parity bar; host validation and the request mapping."""
import numpy as np
import pytest

import acoustic_cases as ac
import prosody_cases as pc
import rowwise_cases as rc
from gonova_tts_amd.engine import PROSODY_FIELDS, PROSODY_NEUTRAL, pack_prosody
from gonova_tts_amd.model import _mel_lens_host, prosody_controls, scale_durations
from parity import TOL, rel_rms


def test_field_order_matches_the_engine():
    assert pc.FIELDS == PROSODY_FIELDS and tuple(pc.NEUTRAL[k] for k in pc.FIELDS) == PROSODY_NEUTRAL
    assert pc.LOOSEST_BAR == max(v[0] for k, v in TOL.items() if k.startswith("ac_"))


# ----------------------------------------------------------------------------- the op-level bound
@pytest.mark.parametrize("N", rc.DUR_N[1:])
def test_fp32_evaluations_sit_inside_the_bound(N):
    """The formula in fp32 with a sequential, a reversed and a pairwise mean: all within the bound."""
    i = pc.op_inputs(N, 64, "f32")
    ctls = pc.op_controls()
    for what, key in (("pitch", "p"), ("energy", "e")):
        ref, bnd = pc.op_adapt_expected(i[key], i["lens"], ctls, what)
        for b, L in enumerate(i["lens"]):
            c = ctls[b]
            if not L or pc.is_neutral(c, what):
                continue
            v = i[key][b, :L]
            r, s = np.float32(c[what + "_range"]), np.float32(c[what + "_shift"])
            for order in (v, v[::-1]):
                m = np.float32(0)
                for x in order:
                    m = np.float32(m + x)
                m = np.float32(m / np.float32(L))
                got = (m + r * (v - m)).astype(np.float32) + s
                assert (np.abs(got.astype(np.float64) - ref[b, :L]) <= bnd[b, :L]).all(), (N, what, b)
            m = np.float32(v.sum(dtype=np.float32) / np.float32(L))    # numpy's pairwise sum
            got = (m + r * (v - m)).astype(np.float32) + s
            assert (np.abs(got.astype(np.float64) - ref[b, :L]) <= bnd[b, :L]).all(), (N, what, b)


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_bound_rejects_each_defect(defect):
    """mean over N / Np instead of len, over a neighbour, the range applied to the mean as well, a
    dropped shift, pitch and energy controls swapped: each leaves the bound on some utterance, for
    every N of the GPU test with more than one token."""
    for N in rc.DUR_N[1:]:
        i = pc.op_inputs(N, 64, "f32")
        ctls = pc.op_controls()
        caught = False
        for what, key in (("pitch", "p"), ("energy", "e")):
            ref, bnd = pc.op_adapt_expected(i[key], i["lens"], ctls, what)
            bad, _ = pc.op_adapt_expected(i[key], i["lens"], ctls, what, defect=defect, N=N)
            for b, L in enumerate(i["lens"]):
                if not L:
                    continue
                if pc.is_neutral(ctls[b], what):    # the GPU test asks for the input's bits here
                    caught |= not np.array_equal(bad[b, :L], i[key][b, :L].astype(np.float64))
                else:
                    caught |= bool((np.abs(bad[b, :L] - ref[b, :L]) > bnd[b, :L]).any())
        assert caught, (defect, N)


@pytest.mark.parametrize("defect", pc.DUR_DEFECTS)
def test_durations_reject_scale_defects(defect):
    """The scale applied after the all-zero rule, or twice: other durations than expected."""
    for N in rc.DUR_N:
        i = pc.op_inputs(N, 64, "f32")
        ctls = pc.op_controls()
        caught = False
        for ovr in (None, i["ovr"]):
            for tcap in pc.op_tcaps(N):
                want = pc.op_durations_expected(i["logd"], ovr, i["lens"], N, tcap, ctls)
                bad = pc.op_durations_expected(i["logd"], ovr, i["lens"], N, tcap, ctls, defect=defect)
                caught |= not np.array_equal(want[0], bad[0])
        assert caught, (defect, N)


def test_scales_land_on_ties():
    """0.5 and 1.5 put odd durations on .5 (ties to even); the op inputs hold such durations."""
    assert list(pc.scaled([1, 3, 5, 7], 0.5)) == [0, 2, 2, 4] and list(pc.scaled([1, 3, 5], 1.5)) == [2, 4, 8]
    assert list(pc.scaled([3, 5], 1.0)) == [3, 5]
    i = pc.op_inputs(300, 64, "f32")
    assert (i["ovr"][2, :300] % 2 == 1).any()


# ---------------------------------------------------------------------------- the model-level bars
@pytest.mark.parametrize("name", pc.MOVE_CASES)
def test_every_setting_moves_the_mel_ten_bars(name):
    """Each control setting of the GPU tests moves the oracle mel by at least 10 x the loosest
    parity bar (2e-2 rel-RMS), so the model-level bars detect a missed or swapped control."""
    ids, durs = ac.ragged_inputs(name)
    base = ac.oracle64(name)
    cfg, w = ac.CASES[name].cfg, ac.weights(name)
    for b in pc.MOVE_UTTS:
        neutral = pc.controlled_forward(ids[b], w, cfg, pc.controls(), durations=durs[b])
        assert np.array_equal(neutral["mel"], base[b]["mel"])      # the restatement is the oracle when neutral
        assert 0.5 < neutral["pitch"].std() < 1.5 and 0.5 < neutral["energy"].std() < 1.5
        for label, c in pc.SETTINGS.items():
            moved = pc.controlled_forward(ids[b], w, cfg, c, durations=durs[b])["mel"]
            r = rel_rms(moved, neutral["mel"])
            print(f"[prosody move] {name} b={b} {label}: rel-RMS {r:.3f}")
            assert r >= 10 * pc.LOOSEST_BAR, (name, b, label, r)
    used = [c for c in pc.model_controls() if c != pc.controls()]
    for c in used:      # every non-neutral pitch / energy value the GPU batch uses is one of SETTINGS'
        for k in pc.FIELDS[1:]:
            if c[k] != pc.NEUTRAL[k]:
                assert any(s[k] == c[k] for s in pc.SETTINGS.values()), (k, c[k])


def test_controlled_oracle_scales_given_durations():
    refs = pc.controlled_oracle64("h64")
    assert [r["mel"].shape[0] for r in refs] == [3, 4, 93, 96, 99, 248, 260, 129]
    assert max(r["mel"].shape[0] for r in refs) <= pc.T_CAP


# -------------------------------------------------------------------------------------- host side
def test_exaggeration_mapping():
    assert prosody_controls() is None and prosody_controls(exaggeration=0.5) is None
    assert prosody_controls(exaggeration=0.25)["pitch_range"] == 0.5 == prosody_controls(exaggeration=0.25)["energy_range"]
    assert prosody_controls(exaggeration=1.0)["pitch_range"] == 2.0
    assert prosody_controls(exaggeration=3.0)["energy_range"] == 4.0          # clipped above
    assert prosody_controls(exaggeration=-1.0)["pitch_range"] == 0.0          # and below
    c = prosody_controls(speed=1.2, pitch=-4, energy=4)
    assert np.float32(c["duration_scale"]) == np.float32(1) / np.float32(1.2)
    assert (c["pitch_shift"], c["energy_shift"], c["pitch_range"]) == (-4.0, 4.0, 1.0)
    assert prosody_controls(speed=0.25)["duration_scale"] == 4.0 and prosody_controls(speed=4)["duration_scale"] == 0.25


@pytest.mark.parametrize("kw", [dict(speed=0.2), dict(speed=4.01), dict(speed=0), dict(speed=float("nan")),
                                dict(pitch=4.5), dict(energy=-4.5), dict(pitch=float("inf")), dict(speed="2"),
                                dict(exaggeration=None), dict(exaggeration=float("nan")), dict(energy=True)])
def test_request_values_are_refused(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        prosody_controls(**kw)


def test_pack_prosody_validates_on_the_host():
    assert pack_prosody(None, 3) is None
    assert pack_prosody([None, None], 2) is None and pack_prosody({"pitch_range": [1, 1]}, 2) is None
    blk = pack_prosody([None, {"duration_scale": 1.5, "energy_shift": -1}], 2)
    assert blk.dtype == np.float32 and blk.tolist() == [[1, 1.5], [0, 0], [1, 1], [0, -1], [1, 1]]
    blk = pack_prosody({"pitch_shift": np.float64(2), "duration_scale": np.array([1, 2, 0.5])}, 3)
    assert blk[0].tolist() == [1, 2, 0.5] and blk[1].tolist() == [2, 2, 2]
    for bad in ({"duration_scale": [1.0, 0.0]}, {"duration_scale": [1.0, -1.0]}, {"duration_scale": [1.0, np.inf]},
                {"pitch_shift": [np.nan, 0]}, {"energy_range": [1.0]}, {"energy_range": [[1.0, 1.0]]}, {"tempo": [1, 1]},
                [None], [None, {"pitch_range": [1, 2]}], [None, 3.0]):
        with pytest.raises(ValueError):
            pack_prosody(bad, 2)


def test_given_durations_scale_on_the_host_like_the_kernel():
    """The model scales given durations on the host and sends a neutral scale: the same float32
    rint as the kernel, so the no-sync streaming path's frame counts (_mel_lens_host) match."""
    logd, ovr, lens = rc.dur_inputs(300)
    ctls = pc.op_controls()
    scale = np.asarray([c["duration_scale"] for c in ctls], np.float32)
    d = scale_durations(ovr, scale)
    assert d.dtype == np.int32 and np.array_equal(d[5], ovr[5])      # scale 1: untouched
    for tcap in pc.op_tcaps(300):
        want = pc.op_durations_expected(logd, ovr, lens, 300, tcap, ctls)
        neutral = pc.op_durations_expected(logd, d, lens, 300, tcap, [pc.controls()] * len(lens))
        for a, b in zip(want, neutral):
            assert np.array_equal(a, b)
        assert np.array_equal(_mel_lens_host(np.asarray(lens), d, tcap), want[1])
