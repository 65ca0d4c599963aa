"""The float64 conv reference, its error bound and the defect replay (oracle/conv.py) on the cases
of conv_cases.py, without a GPU: the reference is pinned to the oracles the whole-model tests use,
the cases are shown to reach every kernel family the launchers pick from, and the bound is shown
to accept the kernels' arithmetic replayed in NumPy float32 / float16 and to reject every injected
defect.  test_conv_op_gpu.py holds the kernels to the same bound."""
import numpy as np
import pytest

import conv_cases as cc
from oracle import conv as oc
from oracle.acoustic import layer_norm as acoustic_layer_norm
from oracle.vocoder import conv1d as vocoder_conv1d


# ------------------------------------------------------------------------------ reference pins
@pytest.mark.parametrize("case", ["b", "h", "j"])
def test_reference_is_the_vocoder_oracles_conv(case):
    """acc + bias equals oracle.vocoder.conv1d on every utterance (zero padding, dilation, length)."""
    P = cc.problem(case, "normal", "plain", "f32", "short")
    for b, L in enumerate(P["lens"]):
        xin = oc.act_in(P["x"][b, :L], P["in_slope"], "f32")
        want = vocoder_conv1d(xin, P["w"], P["bias"], dilation=P["dil"], padding=P["pad"])
        got = cc.reference(case, "normal", "plain", "f32", "short")[b]
        assert want.shape == got["y"].shape == (L, cc.shape(case)["M"])
        np.testing.assert_allclose(got["acc"] + P["bias"], want, rtol=0, atol=1e-12)


def test_reference_epilogue_and_layernorm():
    """((alpha (acc + bias)) -> act) + r1 + r2, times out_scale, written out by hand; LN1, LN2 and the
    Linear equal oracle.acoustic.layer_norm."""
    for case, epi in (("e", "res"), ("f", "act"), ("d", "plain")):
        P = cc.problem(case, "normal", epi, "f32", "short")
        e = cc.EPILOGUES[epi]
        for b, L in enumerate(P["lens"]):
            r = cc.reference(case, "normal", epi, "f32", "short")[b]
            t = np.float64(np.float32(e.get("alpha", 1.0))) * (r["acc"] + P["bias"])
            if e.get("act"):
                t = np.where(t >= 0, t, t * np.float64(np.float32(e["out_slope"])))
            if e.get("res"):
                t = t + P["r1"][b, :L] + P["r2"][b, :L]
            t = t * np.float64(np.float32(e.get("out_scale", 1.0)))
            np.testing.assert_allclose(r["y"], t, rtol=0, atol=1e-12)
            ln = P["ln"]
            l1 = acoustic_layer_norm(r["y"], ln["g1"], ln["b1"], ln["eps"])
            np.testing.assert_allclose(r["ln1"], l1, rtol=0, atol=1e-12)
            if ln["g2"] is not None:
                np.testing.assert_allclose(r["ln"], acoustic_layer_norm(l1, ln["g2"], ln["b2"], ln["eps"]), rtol=0, atol=1e-12)
            if ln["lin_w"] is not None:
                np.testing.assert_allclose(r["lin"], l1 @ ln["lin_w"] + ln["lin_b"], rtol=0, atol=1e-12)


def test_operands_hold_values_of_the_dtype():
    for form in cc.FORMS:
        P = cc.problem("c", "wide_w", "res", form, "long")
        for a in (P["x"], P["w"], P["r1"], P["r2"]):
            assert np.array_equal(a, oc.round_to(a, oc.storage(form)))


# ------------------------------------------------------------------------------------ coverage
# (family, channel group, split-K slices) per case: 16-bit | packed split | per-utterance split | fp32 split-K
WANT = {
    "a": (("conv_xres", 64, 1), ("conv_split", 64, 1), ("conv_split", 64, 1), ("conv_gemm", 0, 1)),
    "b": (("conv_gemm", 0, 1), ("conv_split", 32, 1), ("conv_split", 32, 1), ("conv_gemm", 0, 3)),
    "c": (("conv_xres", 64, 1), ("conv_splitp", 128, 1), ("conv_split", 128, 1), ("conv_gemm", 0, 4)),
    "d": (("conv_xres", 64, 1), ("conv_split", 64, 1), ("conv_split", 64, 1), ("conv_gemm", 0, 6)),
    "e": (("conv_xres", 128, 1), ("conv_splitp", 128, 1), ("conv_split", 128, 1), ("conv_gemm", 0, 12)),
    "f": (("conv_xres", 64, 1), ("conv_splitp", 128, 1), ("conv_split", 256, 1), ("conv_gemm", 0, 8)),
    "g": (("conv_xres", 64, 1), ("conv_split", 64, 1), ("conv_split", 64, 1), ("conv_gemm", 0, 2)),
    "h": (("conv_xres", 128, 1), ("conv_split", 128, 1), ("conv_split", 128, 1), ("conv_gemm", 0, 4)),
    "i": (("conv_xres", 64, 1), ("conv_splitp", 128, 2), ("conv_split", 256, 1), ("conv_gemm", 0, 16)),
    "j": (("conv_xres", 128, 1), ("conv_splitp", 128, 1), ("conv_split", 128, 1), ("conv_gemm", 0, 4)),
    "k": (("conv_gemm", 0, 1), ("conv_split", 64, 1), ("conv_split", 64, 1), ("conv_gemm", 0, 1)),
}


def test_cases_reach_the_forms_they_are_there_for():
    got = {c: tuple((e["family"], e["cg"], e["S"]) for e in (cc.expected(c, r) for r in ("f16", "split", "split_utt", "splitk")))
           for c in cc.CASES}
    assert got == WANT
    fam = {(r, cc.expected(c, r)["family"], cc.expected(c, r)["cg"]) for c in cc.CASES for r in cc.RUNS}
    # conv_split_kernel at 128-, 64- and 32-channel groups (KQ = 4, 2, 1); packed rows; both 16-bit kernels
    assert {("split_utt", "conv_split", g) for g in (128, 64, 32)} <= fam
    assert ("split", "conv_splitp", 128) in fam and ("f16", "conv_gemm", 0) in fam and ("bf16", "conv_xres", 128) in fam
    s = cc.shape("b")
    assert s["Cin"] // 32 % 2 == 1 and s["M"] % 8 == 4 and s["M"] % 32 == 4       # KQ = 1; M % 8; a 4-row last block
    assert (cc.shape("g")["k"] - 1) * cc.shape("g")["dil"] == 64 == (cc.shape("h")["k"] - 1) * cc.shape("h")["dil"]
    assert cc.packed_group(cc.shape("j")) and not cc.packed_group(dict(cc.shape("j"), k=6))  # the packed form's widest halo
    for c in ("d",):
        assert cc.shape(c)["M"] % 128                                        # a partial 128-channel block under LN
    # kernels reported: a reduce after split-K, a LayerNorm launch unless the launch applies it itself
    assert cc.expected("i", "split")["kernels"] == 2 and cc.expected("i", "split")["ln_in_launch"]
    assert cc.expected("i", "split", epi="act")["kernels"] == 3
    assert cc.expected("i", "split_utt")["kernels"] == 2 and cc.expected("i", "splitk")["kernels"] == 2
    assert cc.expected("e", "split")["kernels"] == 2 and cc.expected("e", "split", ln_fuse=True)["kernels"] == 1
    assert cc.expected("d", "f16")["kernels"] == 2 and cc.expected("d", "f16", ln_fuse=True)["kernels"] == 1
    assert cc.expected("f", "splitk")["kernels"] == 3          # LayerNorm + Linear is never applied by a reduce
    assert cc.expected("k", "bf16")["kernels"] == 2 and cc.expected("k", "bf16", ln_fuse=True)["kernels"] == 2


def test_every_layernorm_row_has_spread():
    """sigma >= SIGMA_FLOOR on every row of every LayerNorm (the bias carries it on the small pattern),
    so the propagated bound, which divides by sigma, says something."""
    for case in cc.LN_EPS:
        for pattern in cc.PATTERNS:
            for epi in cc.EPILOGUES:
                for batch in cc.BATCHES:
                    for r in cc.reference(case, pattern, epi, "f32", batch):
                        if r["y"].shape[0]:
                            assert np.sqrt(r["var1"].min()) >= cc.SIGMA_FLOOR, (case, pattern, epi, batch)
                            if "var2" in r:
                                assert np.sqrt(r["var2"].min()) >= cc.SIGMA_FLOOR, (case, pattern, epi, batch)


# --------------------------------------------------------------------------------------- power
RUN_OF = {"f16": "f16", "bf16": "bf16", "f32": "splitk", "split": "split"}
GROUP = {"f16": 64, "bf16": 64, "f32": 16, "split": 128}


def worst(case, pattern, epi, form, batch, defect=None, measure=None):
    """max over utterances, outputs and elements of |replay - reference| / bound."""
    P = cc.problem(case, pattern, epi, form, batch)
    S = cc.slices_of(case, RUN_OF[form])
    refs, bnds = cc.reference(case, pattern, epi, form, batch), cc.bound(case, pattern, epi, form, batch, S=S)
    top = 0.0
    for b, L in enumerate(P["lens"]):
        if not L:
            continue
        got = oc.replay(P, form, b, defect=defect, S=S, group=GROUP[form], sentinel=cc.SENTINEL, measure=measure)
        for key, val in got.items():
            err = np.abs(val - refs[b][key]) / bnds[b][key]
            top = max(top, float(np.nan_to_num(err, nan=np.inf).max()))
    return top


@pytest.mark.parametrize("form", cc.FORMS)
def test_the_bound_accepts_the_kernels_arithmetic(form):
    """Every case, pattern and epilogue replayed without a defect stays under its bound."""
    top, split_err = 0.0, 0.0
    for case in cc.CASES:
        for pattern in cc.PATTERNS:
            for epi in cc.EPILOGUES:
                m = {}
                r = worst(case, pattern, epi, form, "long" if case in "gh" else "short", measure=m)
                assert r <= 1.0, (form, case, pattern, epi, r)
                top = max(top, r)
                if pattern == "normal":
                    split_err = max(split_err, m.get("split_err", 0.0))
    print(f"[conv op] {form}: correct replay at most {top:.3f} of the bound"
          + (f"; three-product sum off by at most {split_err:.3f} x 2^-22 A (C_SPLIT = {oc.C_SPLIT:.3f})" if form == "split" else ""))
    if form == "split":
        assert split_err <= oc.C_SPLIT


# where each defect is looked for first: (case, pattern, epilogue)
SEEK = {
    "drop_tap": [("b", "normal", "plain"), ("c", "normal", "plain")],
    "reverse_taps": [("b", "normal", "plain"), ("c", "normal", "plain")],
    "drop_last_group": [("b", "normal", "plain"), ("c", "normal", "plain")],
    "halo_neighbour": [("c", "normal", "plain"), ("j", "normal", "plain")],
    "no_unscale": [("a", "normal", "plain")],
    "drop_lo_hi": [("a", "small", "plain")],
    "splitk_drop_last": [("i", "normal", "plain")],
    "bias_per_slice": [("i", "normal", "plain")],
    "ln_var_cm1": [("k", "normal", "plain")],
    "ln_no_eps": [("i", "normal", "plain")],
    "ln_skip_ln2": [("e", "normal", "plain")],
    "unwritten_tail": [("c", "normal", "plain"), ("d", "normal", "plain")],
}
APPLIES = {"no_unscale": ("split",), "drop_lo_hi": ("split",), "splitk_drop_last": ("f32", "split"),
           "bias_per_slice": ("f32", "split")}


@pytest.mark.parametrize("defect", oc.DEFECTS)
def test_the_bound_rejects_every_defect(defect):
    """In every form it applies to, the defect exceeds the bound on at least one case."""
    for form in APPLIES.get(defect, cc.FORMS):
        seen = [(c, p, e, worst(c, p, e, form, "long", defect=defect)) for c, p, e in SEEK[defect]]
        print(f"[conv op] {defect} {form}: " + ", ".join(f"{c}/{p}/{e} {r:.3g}x" for c, p, e, r in seen))
        assert max(r for *_, r in seen) > 1.0, (defect, form, seen)


def test_small_separates_the_subnormal_floor_from_a_lost_term():
    """On the small pattern the activations' low halves are f16 subnormals: the three-product sum is
    off by far more than 2^-21 relative (what the split form's header used to promise) yet stays under
    the modelled floor, and a kernel that drops the lo . hi term does not."""
    m = {}
    ok = worst("a", "small", "plain", "split", "long", measure=m)
    bad = worst("a", "small", "plain", "split", "long", defect="drop_lo_hi")
    print(f"[conv op] small: three-product sum off by {m['split_err']:.1f} x 2^-22 A; correct {ok:.3f}x, lo.hi dropped {bad:.3f}x of the bound")
    assert m["split_err"] > 2.0 * 8 and ok <= 1.0 < bad
