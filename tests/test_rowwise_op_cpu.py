"""The float64 references, error bounds, expected bits and defect replays of the acoustic model's
row-wise ops (oracle/rowwise.py) on the cases of rowwise_cases.py, without a GPU: the references are
pinned to the whole-model oracle's helpers, the cases are shown to reach every kernel the launchers
pick from, each bound is shown to accept the kernel's arithmetic replayed in NumPy float32 and to
reject every injected defect, and the exact ops' expectations are shown to tell a wrong kernel
apart.  test_rowwise_op_gpu.py holds the kernels to the same bounds and bits."""
import numpy as np
import pytest

import rowwise_cases as rc
from oracle import rowwise as rw
from oracle.acoustic import durations_from_log, layer_norm as acoustic_layer_norm, sigmoid as acoustic_sigmoid


def ratio(got, ref, bnd):
    with np.errstate(invalid="ignore"):
        return float(np.nan_to_num(np.abs(got - ref) / bnd, nan=np.inf).max()) if ref.size else 0.0


# ------------------------------------------------------------------------------ reference pins
def test_glu_reference_is_the_oracles_conv_module_core():
    """GLU, zero-padded depthwise conv, bias, SiLU as oracle.acoustic.conv_module writes them."""
    P = rc.glu_problem("k9_d192", "normal", "f32")
    D, k = P["w"].shape
    for b in (3, 6):
        L = P["lens"][b]
        a = P["a"][b, :L]
        g = a[:, :D] * acoustic_sigmoid(a[:, D:])
        pad = (k - 1) // 2
        gp = np.zeros((L + 2 * pad, D))
        gp[pad:pad + L] = g
        y = sum(gp[j:j + L] * P["w"][:, j] for j in range(k)) + P["bias"]
        np.testing.assert_allclose(rc.glu_reference("k9_d192", "normal", "f32")[0][b]["y"], y * acoustic_sigmoid(y), rtol=0, atol=1e-12)


def test_softmax_reference_shifts_as_the_oracle_does():
    """bd[i][j] = bd_full[i][Tm - 1 - i + j] (oracle.acoustic.rel_mha), scale, softmax over j < len."""
    P = rc.sm_problem(65, "normal", "f32")
    b, L, Tm = 2, P["lens"][2], 65
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    s = (P["ac"][b][:, :L, :L] + P["bd"][b][:, i, (Tm - 1) - i + j]) * rc.SM_SCALE
    e = np.exp(s - s.max(-1, keepdims=True))
    np.testing.assert_allclose(rc.sm_reference(65, "normal", "f32")[0][b]["p"], e / e.sum(-1, keepdims=True), rtol=0, atol=1e-15)


def test_layernorm_reference_is_the_oracles():
    x, (g1, b1, g2, b2) = rc.ln_inputs(100, "f32")
    xv = x[rc.ln_valid_rows()]
    l1 = acoustic_layer_norm(xv, g1, b1, rc.EPS)
    np.testing.assert_allclose(rc.ln_reference(100, "f32", False)[0]["ln"], l1, rtol=0, atol=1e-11)
    np.testing.assert_allclose(rc.ln_reference(100, "f32", True)[0]["ln"], acoustic_layer_norm(l1, g2, b2, rc.EPS), rtol=0, atol=1e-11)


def test_operands_hold_values_of_the_dtype():
    for dt in rc.DTYPES:
        for a in (rc.glu_problem("k7_d72", "saturated", dt)["a"], rc.sm_problem(5, "negative", dt)["ac"],
                  rc.ln_inputs(300, dt)[0], rc.ve_inputs("small", dt)[0]["x"]):
            assert np.array_equal(a, rw.round_to(a, dt))


# ------------------------------------------------------------------------------------ coverage
def test_cases_reach_the_branches_they_are_there_for():
    for case, (k, D, dts, kernel) in rc.GLU_CASES.items():
        for dt in dts:
            assert rc.glu_kernel(k, D, dt) == kernel, (case, dt)
    ks = {c[0] for c in rc.GLU_CASES.values()}
    assert {7, 31, 3, 9, 129} <= ks and (128 + 129 - 1) * 64 * 4 == 64 * 1024
    assert any(D % 64 and D % 8 == 0 for _, D, _, _ in rc.GLU_CASES.values())
    assert {0, 1, 3, 15, 127, 128, 129, 256, 257, 272} == set(rc.GLU_LENS) and rc.GLU_TM == 272
    assert {rc.ln_kernel(C, "f16") for C in rc.LN_C} == {"layernorm8", "layernorm<4>", "layernorm<8>"}
    assert {rc.ln_kernel(C, "f32") for C in rc.LN_C} == {"layernorm<4>", "layernorm<8>"}
    for shape in ("two_trips",):
        rows, D = rc.EW_SHAPES[shape]
        assert rc.GRID1_ELEMS < rows * D <= rc.GRID1_ELEMS + 256
        B, Tin, Tcap, C, _ = rc.MEL_SHAPES[shape]
        assert rc.GRID1_ELEMS < Tcap * C <= rc.GRID1_ELEMS + 256
    assert max(rc.SPK_E) > 256 and max(rc.DUR_N) > 256


def test_saturated_and_sharp_patterns_are_what_they_claim():
    """Saturated: gates of magnitude >= 40 on both sides and pre-activation sums past 40 and past
    88.7 (exp overflows to inf in fp32); sharp: every row with two keys or more spreads >= 80 after
    the scale, so an un-shifted exp overflows; no reference value is NaN or inf."""
    for dt in rc.DTYPES:
        P = rc.glu_problem("k7_d64", "saturated", dt)
        refs, _ = rc.glu_reference("k7_d64", "saturated", dt)
        gt = refs[9]["gt"]
        assert np.abs(gt).min() >= 39.9 and (gt > 0).any() and (gt < 0).any()
        acc = refs[9]["acc"]
        assert (acc < -88.8).any() and (acc > 88.8).any() and ((np.abs(acc) > 40) & (np.abs(acc) < 100)).any()
        assert all(np.isfinite(r["y"]).all() for r in refs)
        lim = {"f16": 65504.0, "bf16": 3e38, "f32": 3e38}[dt]
        assert max(np.abs(r["y"]).max() for r in refs if r["y"].size) < lim
        for Tm in rc.SM_TM:
            refs, _ = rc.sm_reference(Tm, "sharp", dt)
            for r in refs:
                if r is not None and r["s"].shape[-1] >= 2:
                    spread = r["s"].max(-1) - r["s"].min(-1)
                    assert spread.min() >= 80.0, (dt, Tm, spread.min())
                    assert (r["p"].max(-1) > 0.999999).all()


# --------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("dt", rc.DTYPES)
def test_the_bounds_accept_the_kernels_arithmetic(dt):
    """Every bounded op, case and pattern replayed without a defect stays under its bound."""
    top = {}

    def seen(op, r, where):
        assert r < 1.0, (op, dt, where, r)
        top[op] = max(top.get(op, 0.0), r)

    for case, (_, _, dts, _) in rc.GLU_CASES.items():
        if dt in dts:
            for pattern in rc.GLU_PATTERNS:
                P = rc.glu_problem(case, pattern, dt)
                refs, bnds = rc.glu_reference(case, pattern, dt)
                for b in range(len(rc.GLU_LENS)):
                    seen("glu_dwconv", ratio(rw.glu_replay(P, b), refs[b]["y"], bnds[b]), (case, pattern, b))
    for Tm in rc.SM_TM:
        for pattern in rc.SM_PATTERNS:
            P = rc.sm_problem(Tm, pattern, dt)
            refs, bnds = rc.sm_reference(Tm, pattern, dt)
            for b, r in enumerate(refs):
                if r is not None:
                    got = rw.softmax_replay(P, b)
                    seen("rel_softmax", ratio(got, r["p"], bnds[b]), (Tm, pattern, b))
                    assert (np.abs(got.sum(-1) - 1.0) <= bnds[b].sum(-1)).all(), (Tm, pattern, b, "row sum")
    for C in rc.LN_C:
        x, (g1, b1, g2, b2) = rc.ln_inputs(C, dt)
        xv = x[rc.ln_valid_rows()]
        for two in (False, True):
            ref, bnd = rc.ln_reference(C, dt, two)
            got = rw.ln_replay(xv, dt, g1, b1, rc.EPS, g2 if two else None, b2 if two else None)
            seen("layernorm", ratio(got, ref["ln"], bnd), (C, two))
    for G in rc.LNG_G:
        for C in rc.LNG_C:
            x, gains, biases = rc.lng_inputs(G, C, dt)
            ref, bnd = rc.lng_reference(G, C, dt)
            got = rw.lng_replay(x[rc.ln_valid_rows()], dt, C, gains, biases, rc.EPS)[:, :G * C]
            seen("layernorm_groups", ratio(got, ref, bnd), (G, C))
    for E in rc.SPK_E:
        for D in rc.SPK_D:
            e, We, bias = rc.spk_inputs(E, D)
            for r in range(len(rc.SPK_ROWS)):
                ref = rw.spk_reference(e[r], We, bias)
                seen("spk_bias", ratio(rw.spk_replay(e[r], We, bias, dt), ref["y"], rw.spk_bound(e[r], We, bias, dt, ref)), (E, D, r))
    for shape in rc.EW_SHAPES:
        i, ref, bnd = rc.ve_inputs(shape, dt)
        seen("var_embed_add", ratio(rw.var_replay(dt=dt, **i), ref["y"], bnd), shape)
    print(f"[rowwise op] {dt}: correct replays at most " + ", ".join(f"{op} {r:.3f}" for op, r in top.items()) + " of their bounds")


GLU_SEEK = {"off_centre": ["k7_d64", "k9_d192"], "reverse_taps": ["k7_d64", "k3_d64"], "swap_halves": ["k7_d64"],
            "no_bias": ["k7_d64", "k31_d192"], "no_silu": ["k7_d64"], "halo_neighbour": ["k7_d64", "k129_d72"],
            "drop_tile_edge_row": ["k7_d64", "k31_d72"], "drop_last_block": ["k7_d72", "k129_d72"]}


@pytest.mark.parametrize("defect", rw.GLU_DEFECTS)
def test_glu_dwconv_bound_rejects(defect):
    for dt in rc.DTYPES:
        seen = []
        for case in GLU_SEEK[defect]:
            P = rc.glu_problem(case, "normal", dt)
            refs, bnds = rc.glu_reference(case, "normal", dt)
            seen.append(max(ratio(rw.glu_replay(P, b, defect, sentinel=rc.SENTINEL), refs[b]["y"], bnds[b]) for b in range(len(rc.GLU_LENS))))
        print(f"[rowwise op] glu_dwconv {defect} {dt}: " + ", ".join(f"{c} {r:.3g}x" for c, r in zip(GLU_SEEK[defect], seen)))
        assert max(seen) > 1.0, (defect, dt, seen)


@pytest.mark.parametrize("defect", rw.SOFTMAX_DEFECTS)
def test_rel_softmax_bound_rejects(defect):
    pattern = "sharp" if defect == "no_max" else "normal"
    for dt in rc.DTYPES:
        seen = []
        for Tm in (5, 65):
            P = rc.sm_problem(Tm, pattern, dt)
            refs, bnds = rc.sm_reference(Tm, pattern, dt)
            Sk = rc.sm_extents(Tm)[2]
            for b, r in enumerate(refs):
                if r is not None:
                    L = P["lens"][b]
                    got = rw.softmax_replay(P, b, defect, Sk=Sk)
                    tail = 0.0 if (got[..., L:] == 0).all() else np.inf      # columns >= len must be exactly 0
                    seen.append(max(ratio(got[..., :L], r["p"], bnds[b]), tail))
        print(f"[rowwise op] rel_softmax {defect} {dt}: worst {max(seen):.3g}x")
        assert max(seen) > 1.0, (defect, dt, seen)


@pytest.mark.parametrize("defect", rw.LN_DEFECTS + rw.LNG_DEFECTS)
def test_layernorm_bound_rejects(defect):
    for dt in rc.DTYPES:
        if defect == "neighbour_gain":
            x, gains, biases = rc.lng_inputs(3, 100, dt)
            ref, bnd = rc.lng_reference(3, 100, dt)
            r = ratio(rw.lng_replay(x[rc.ln_valid_rows()], dt, 100, gains, biases, rc.EPS, defect)[:, :300], ref, bnd)
        else:
            if defect == "one_pass" and dt != "f32":
                continue   # (16-bit rounds the mean-100 row's spread away before any variance is taken)
            r = 0.0   # (the mean's worst-case-order term grows with C: the few-channel rows are the sharp ones)
            for C in ((8,) if defect == "var_cm1" else (8, 100) if defect == "one_pass" else (256,)):
                x, (g1, b1, _, _) = rc.ln_inputs(C, dt)
                ref, bnd = rc.ln_reference(C, dt, False)
                r = max(r, ratio(rw.ln_replay(x[rc.ln_valid_rows()], dt, g1, b1, rc.EPS, defect=defect), ref["ln"], bnd))
        print(f"[rowwise op] layernorm {defect} {dt}: {r:.3g}x")
        assert r > 1.0, (defect, dt, r)


@pytest.mark.parametrize("defect", rw.SPK_DEFECTS + rw.VAR_DEFECTS)
def test_spk_bias_and_var_embed_bounds_reject(defect):
    for dt in rc.DTYPES:
        if defect == "swap_tables":
            i, ref, bnd = rc.ve_inputs("small", dt)
            r = ratio(rw.var_replay(dt=dt, defect=defect, **i), ref["y"], bnd)
        else:
            e, We, bias = rc.spk_inputs(300, 72)
            r = max(ratio(rw.spk_replay(e[q], We, bias, dt, defect), rw.spk_reference(e[q], We, bias)["y"], rw.spk_bound(e[q], We, bias, dt))
                    for q in range(len(rc.SPK_ROWS)))
        print(f"[rowwise op] {defect} {dt}: {r:.3g}x")
        assert r > 1.0, (defect, dt, r)


def test_spk_bias_clamp_rows():
    """The zero embedding gives the bias itself; the 1e-20 one is divided by 1e-12, not by its norm."""
    e, We, bias = rc.spk_inputs(64, 72)
    assert np.array_equal(rw.spk_reference(e[1], We, bias)["y"], bias)
    np.testing.assert_allclose(rw.spk_reference(e[2], We, bias)["y"], bias + We @ e[2] / float(np.float32(1e-12)), rtol=1e-12)


# ----------------------------------------------------------------------------------- durations
def test_duration_inputs_keep_clear_of_every_tie_of_the_exponential():
    """exp(x) - 1 stays DUR_MARGIN away from every half-integer (fp32 expf is off by < 1e-5 at
    these magnitudes), so the rounding of the predicted form is decided; the speeds do land on ties."""
    for N in rc.DUR_N:
        logd, ovr, lens = rc.dur_inputs(N)
        assert rw.duration_margin(logd, lens) >= rc.DUR_MARGIN, N
        assert float(np.exp(np.nanmax(np.where(np.arange(N)[None] < np.array(lens)[:, None], logd, -np.inf)))) < 16.0
    logd, ovr, lens = rc.dur_inputs(300)
    d = rw.durations_expected(logd, lens, 300, 10 ** 6)[0]
    for speed in (0.5, 1.5):
        assert ((d * speed) % 1 == 0.5).any(), speed


def test_durations_expected_by_hand():
    """lens (3, 2, 0, 4) as tests/test_capi.py's host rule, plus the map."""
    lens = (3, 2, 0, 4)
    ovr = np.array([[2, 3, 1, 9], [0, 0, 5, 5], [4, 4, 4, 4], [-1, 6, 6, 6]])
    dur, mel, tok = rw.durations_expected(None, lens, 4, 16, override_d=ovr)
    assert dur.tolist() == [[2, 3, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 6, 6, 6]]
    assert mel.tolist() == [6, 2, 0, 16]
    assert tok[0].tolist() == [0, 0, 1, 1, 1, 2] + [-1] * 10 and tok[3].tolist() == [1] * 6 + [2] * 6 + [3] * 4
    x = np.log(np.array([[3.5, 1.0, 2.5 + 1e-3, 1.49]], np.float32))      # exp - 1 = 2.5, 0, 1.501, 0.49
    assert rw.durations_expected(x, (4,), 4, 16)[0].tolist() == [[2, 0, 2, 0]]
    assert np.array_equal(rw.durations_expected(x, (4,), 4, 16, speed=1.5)[0][0], durations_from_log(x[0], 1.5))


@pytest.mark.parametrize("defect", rw.DUR_DEFECTS)
def test_duration_defects_show(defect):
    """Each wrong durations kernel differs from the expectation on the cases the GPU test runs."""
    differs = False
    for N in rc.DUR_N:
        logd, ovr, lens = rc.dur_inputs(N)
        for tcap in rc.dur_tcaps(N):
            for speed in rc.DUR_SPEEDS:
                for o in (None, ovr):
                    want = rw.durations_expected(logd, lens, N, tcap, override_d=o, speed=speed)
                    got = rw.durations_expected(logd, lens, N, tcap, override_d=o, speed=speed, defect=defect)
                    differs |= any(not np.array_equal(a, b) for a, b in zip(want, got))
    assert differs, defect


# ------------------------------------------------------------------------------------ exact ops
def test_exact_expectations_by_hand():
    t = np.arange(12.0).reshape(4, 3)
    out = rw.embed_expected("f32", np.array([[3, -2, 9]]), (2,), 4, t, 2.0)
    assert out[0].tolist() == [[18, 20, 22], [0, 2, 4], [0, 0, 0], [0, 0, 0]]
    out = rw.regulate_expected("f16", t[None], np.array([[1, -1, 3, 0]]), 3, 5, 0.5, rc.SENTINEL)
    assert out[0].tolist() == [[1.5, 2, 2.5], [0, 0, 0], [4.5, 5, 5.5]] + [[rc.SENTINEL] * 3] * 2
    qkv = np.arange(2 * 3 * 12.0).reshape(2, 3, 12)     # D = 4, H = 2, dk = 2
    vt = rw.transpose_v_expected(qkv, (2, 0), 4, 2, 4)
    assert vt[0, 1].tolist() == [[10, 22, 0, 0], [11, 23, 0, 0]] and not vt[1].any()
    assert rw.mel_out_expected(qkv, (5, 1), 2)[1].tolist() == [qkv[1, 0].tolist(), [0.0] * 12]
    # one fp32 operation, one rounding: 1 + 2^-11 in f16 is a tie that goes to even
    qu, _ = rw.pos_bias_expected("f16", np.ones((1, 3)), 1, np.array([2.0 ** -11]), np.zeros(1))
    assert qu[0, 0] == 1.0
    assert not rc.same_bits(np.array([0.0]), np.array([-0.0])) and rc.same_bits(np.array([np.inf]), np.array([np.inf]))
    for dt in rc.DTYPES:      # the specials survive the dtype
        sp = np.array(rc.SPECIALS[dt])
        assert rc.same_bits(rw.round_to(sp, dt), sp) and len(set(sp.tolist())) >= 6
