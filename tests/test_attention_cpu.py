"""CPU side of the op-level attention tests: the float64 reference (oracle/attention.py) is pinned
to the acoustic oracle, and everything the GPU tests (test_attention_gpu.py) rely on is shown from
the reference alone -- that the input patterns reach the regimes they are there for (coverage), and
that the parity bounds reject the defects a subtly wrong kernel would have (power).  No kernel runs
here."""
import numpy as np
import pytest

import attention_cases as ac
from oracle import attention as oa


def test_reference_matches_acoustic_oracle():
    """rel_attention (unrounded, "f64") on one layer of the default weights equals
    oracle.acoustic.rel_mha to 1e-12: the same q / k / v projections and position table, the output
    projection applied here."""
    from gonova_tts_amd.weights import make_acoustic_weights
    from oracle.acoustic import rel_mha, rel_pos_table
    w = {k: np.asarray(v, np.float64) for k, v in make_acoustic_weights(0).items() if np.asarray(v).dtype.kind == "f"}
    p = "decoder.conformer_layers.1.self_attn."
    H, dk = w[p + "pos_bias_u"].shape
    L, D = 77, H * dk
    x = np.random.default_rng(5).standard_normal((L, D))
    pe = rel_pos_table(L, D, np.float64)
    want = rel_mha(x, pe, w, p, H)
    q, k, v = ((x @ w[p + f"linear_{n}.weight"].T + w[p + f"linear_{n}.bias"]).reshape(L, H, dk) for n in "qkv")
    for rmax in (L, 256):
        # rel_pos_table's row r <-> rel = L - 1 - r; the engine's table row r <-> rel = rmax - 1 - r
        R = np.zeros((2 * rmax, H, dk))
        R[rmax - L: rmax + L - 1] = (pe @ w[p + "linear_pos.weight"].T).reshape(2 * L - 1, H, dk)
        o = oa.rel_attention(q, k, v, R, w[p + "pos_bias_u"], w[p + "pos_bias_v"], rmax, "f64")
        got = o.reshape(L, D) @ w[p + "linear_out.weight"].T + w[p + "linear_out.bias"]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_flash_replay_equals_direct_softmax():
    """The 32-key-step online softmax the defects are injected into is the direct softmax when
    nothing is injected, lazy or eager."""
    for pattern in ("ramp", "sharp", "descend"):
        for shape in ("b1", "b3"):
            c = ac.case_inputs(pattern, shape, "f16")
            for (q, k, v), s, ref in zip([u for u in c["utts"] if len(u[0])], ac.case_scores(pattern, shape, "f16"),
                                         [r for r in ac.reference(pattern, shape, "f16") if r.size]):
                for lazy in (0.0, oa.LAZY):
                    assert np.abs(oa.flash(s, v, lazy) - ref).max() < 1e-12


def test_rounding_helpers():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, 65519.0, 1e-30])
    assert oa.round_to(x, "bf16").tolist()[:2] == [1.0, 1.0 + 2.0 ** -7]   # ties to even, both ways
    assert oa.round_to(x, "f16")[2] == 65504.0 and oa.round_to(x, "f16")[3] == 0.0
    u = np.full((1, 192), 2.0 ** -12, np.float32)
    qu, _ = oa.biased_queries(np.ones((1, 1, 192)), u, u, "f16")    # one f32 add, then one rounding
    assert (qu == 1.0).all()


# ---------------------------------------------------------------------------------------- coverage
def _moves(pattern, shape, dtype="f16"):
    """[(length, moves [H, L])] of a case's non-empty utterances"""
    lens = [n for n in ac.SHAPES[shape][0] if n]
    return list(zip(lens, [oa.lazy_moves(s) for s in ac.case_scores(pattern, shape, dtype)]))


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_ramp_moves_every_row(dtype):
    """`ramp` climbs ~0.5 log2 per key, so a row moves once its second 32-key step holds more than
    ~16 keys: every row of every utterance of 63 keys and more moves, and at 200 keys some row moves
    at least 4 times.  (The set's 33-key utterance cannot: its second step is one key, 0.5 log2 up.)"""
    most = 0
    for shape in ac.SHAPES:
        for n, m in _moves("ramp", shape, dtype):
            if n >= 63:
                assert (m >= 1).all(), (shape, n)
            most = max(most, int(m.max()))
    assert most >= 4


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_sharp_moves_a_tenth_of_the_rows(dtype):
    for shape in ("b1", "b9z"):
        for n, m in _moves("sharp", shape, dtype):
            if n == 200:
                assert (m > 0).mean() >= 0.10, (shape, float((m > 0).mean()))


def test_sharp_and_ramp_span_the_range_of_p():
    """Row spreads past 24 log2 (f16's whole subnormal range) on `sharp`, `ramp` and `descend`."""
    for pattern in ("sharp", "ramp", "descend"):
        s = ac.case_scores(pattern, "b1", "f16")[0] * oa.LOG2E
        assert (s.max(-1) - s.min(-1)).max() > 40


def test_flat_moves_no_row():
    for shape in ac.SHAPES:
        for dtype in ("f16", "bf16", "f32"):
            assert all(not m.any() for _, m in _moves("flat", shape, dtype))


def test_descend_holds_its_first_step():
    for shape in ac.SHAPES:
        assert all(not m.any() for _, m in _moves("descend", shape))


def _recorded_scores(f):
    """The score matrices every rel_mha of the acoustic oracle hands to its softmax while f() runs."""
    import oracle.acoustic as oac
    rec, orig = [], oac.softmax

    def spy(x, axis=-1):
        rec.append(np.array(x, np.float64))
        return orig(x, axis)

    oac.softmax = spy
    try:
        out = f()
    finally:
        oac.softmax = orig
    return out, rec


def test_default_weight_model_moves_no_row():
    """The regime the whole-model tests run the fused attention in: with make_acoustic_weights
    weights no row of any layer moves after its first key step, which is why the op-level patterns
    exist."""
    from gonova_tts_amd.weights import make_acoustic_weights
    from oracle.acoustic import acoustic_forward
    ids = np.random.default_rng(0).integers(1, 70, size=33)
    _, rec = _recorded_scores(lambda: acoustic_forward(ids, make_acoustic_weights(0), durations=np.full(33, 5),
                                                       dtype=np.float64))
    assert len(rec) == 8 and rec[-1].shape[-1] == 165
    assert sum(int(oa.lazy_moves(s).sum()) for s in rec) == 0


@pytest.mark.parametrize("name", list(ac.SHARPEN))
def test_sharpened_model_keeps_the_reference_clear_of_the_bar(name):
    """The whole-model complement (attention_cases.SHARPEN): on the sharpened weights the oracle's
    float32 mel stays within a third of the fp32 bar of its float64 mel, and where a factor with
    that property moves rows at all (h64) the oracle's rows do move."""
    r64 = ac.sharpened_oracle(name, np.float64)
    r32 = ac.sharpened_oracle(name, np.float32)
    for a, b in zip(r32, r64):
        assert (np.abs(a - b) <= (ac.FP32_ATOL + ac.FP32_RTOL * np.abs(b)) / 3).all(), name
    import acoustic_cases as acs
    from oracle.acoustic import acoustic_forward
    ids, durs = acs.ragged_inputs(name)
    _, rec = _recorded_scores(lambda: [acoustic_forward(x, ac.sharpened_weights(name), acs.CASES[name].cfg, durations=d,
                                                        dtype=np.float64) for x, d in zip(ids, durs)])
    moved = sum(int((oa.lazy_moves(s) > 0).sum()) for s in rec)
    assert (moved > 0) == ac.SHARPEN_MOVES[name], (name, moved)


# ------------------------------------------------------------------------------------------ bounds
def test_bounds_are_finite_and_ordered():
    """Every case has a positive bound from the reference alone; the 16-bit ones sit where the
    formats put them (bf16 8x f16: three fewer mantissa bits), the fp32 ones orders below."""
    for pattern in ac.PATTERNS:
        for shape in ac.SHAPES:
            b = {dt: ac.bound(pattern, shape, dt) for dt in ac.DTYPES}
            for dt in ac.DTYPES:
                assert all(np.isfinite(x) and x > 0 for x in b[dt]), (pattern, shape, dt)
                assert all(np.isfinite(r).all() for r in ac.reference(pattern, shape, dt))
            assert 1e-4 < b["f16"][0] < 2e-3 and 4 < b["bf16"][0] / b["f16"][0] < 16
            assert b["f32"][0] < 0.1 * b["f16"][0] and b["split"] == b["f32"]


# ------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("dtype", ["f16", "f32", "bf16", "split"])
@pytest.mark.parametrize("pattern", ["ramp", "sharp"])
def test_bounds_reject_every_defect(pattern, dtype):
    """Each defect of oracle.attention.DEFECTS, injected into the float64 reference, puts some
    utterance outside the case's bound on `ramp` and `sharp`, on every shape, in every dtype: a
    kernel with that defect fails the GPU parity test.  bf16's wider bound (8x f16's) misses none
    of them on these two patterns.  What the other patterns miss, by construction: `flat`,
    `descend` and most of `pos` move no row in the lazy forms, so the two rescale defects change
    nothing there; `descend` gives the last key step no weight, so the dropped step passes in f16 /
    bf16, and its 200-key utterance gives the last key none either."""
    for shape in ac.SHAPES:
        for defect in oa.DEFECTS:
            assert ac.rejected(defect, pattern, shape, dtype), (defect, pattern, shape, dtype)


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_pos_rejects_the_index_slip(dtype):
    """`pos` takes its scores from Qv . R alone: a relative index off by one is caught on every
    shape in every dtype, bf16 included."""
    for shape in ac.SHAPES:
        assert ac.rejected("rel_off_by_one", "pos", shape, dtype), (shape, dtype)


def test_clean_reference_is_not_rejected():
    """The rejection test itself: the reference without a defect, and the rounding model the bound
    comes from, are inside every bound."""
    for pattern in ac.PATTERNS:
        for shape in ac.SHAPES:
            for dtype in ac.DTYPES:
                bnd, refs = ac.bound(pattern, shape, dtype), ac.reference(pattern, shape, dtype)
                for o, r in zip(ac.rounded(pattern, shape, dtype), refs):
                    if r.size:
                        e = o - r
                        # the model meets its own max-abs bound on every utterance; its relative RMS
                        # is pooled, so one utterance may sit above the pool's mean, not above 3x it
                        assert np.abs(e).max() <= bnd[1] and ac.within(o, r, bnd)[0], (pattern, shape, dtype)
