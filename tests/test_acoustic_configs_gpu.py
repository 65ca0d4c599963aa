"""The HIP acoustic model on small configurations other than the default (tests/acoustic_cases.py)
against the float64 oracle, all through HipEngine.acoustic.

fp32 runs are held to the project's fp32 bar (FP32_ATOL / FP32_RTOL of test_acoustic_gpu.py): the
structural test, where a wrong tap order, head split, relative-position shift or depthwise centring
is off by orders of magnitude.  The reference is the float64 oracle, so the bar is not spent on the
reference's own rounding.  f16 / bf16 runs go through parity.check with the project's acoustic
bars (parity.TOL ac_f16 / ac_bf16: set for the four-layer default model; no case here is deeper),
durations forced.  Predicted durations are compared exactly: the predicted-duration batch is chosen
on the CPU clear of every rounding boundary (test_acoustic_configs_cpu.py).  The kernel-path
switches are compared on the new shapes bit for bit where test_acoustic_gpu.py asserts bit
identity at the default shape, and the profiler's per-kind launch counts show that each case ran
the kernel family it is there for.

Measured 16-bit errors land in $PARITY_LOG (profiles/acoustic_configs_parity.json is that log from
an MI355X run).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import acoustic_cases as ac  # noqa: E402
from gonova_tts_amd.engine import HipEngine, device_bytes  # noqa: E402
from parity import check, rel_rms  # noqa: E402
from test_acoustic_gpu import FP32_ATOL, FP32_RTOL  # noqa: E402

DEV = "cuda:0"
NAMES = list(ac.CASES)
PRED_CAP = 12 * max(ac.PRED_TOKENS)
_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def new_engine(name, dtype, precision="exact"):
    e = HipEngine(DEV, vocoder_dtype="f32", acoustic_dtype=dtype, encoder_precision=precision)
    e.load_weights(acoustic=ac.weights(name))
    assert e.speaker_dim == (ac.CASES[name].cfg.speaker_embed_dim or 0)
    return e


def engine_for(name, dtype, precision="exact"):
    key = (name, dtype, precision)
    if key not in _ENG:
        _ENG[key] = new_engine(name, dtype, precision)
    return _ENG[key]


def run(eng, ids_list, t_cap, durations=None, spk=None):
    """-> (mel [B, t_cap, 80], mel_lens [B], durations [B, N]) as numpy arrays"""
    B, N = len(ids_list), max(len(x) for x in ids_list)
    tok = np.zeros((B, N), np.int32)
    for b, x in enumerate(ids_list):
        tok[b, :len(x)] = x
    lens = torch.tensor([len(x) for x in ids_list], dtype=torch.int32)
    dd = None
    if durations is not None:
        d = np.zeros((B, N), np.int32)
        for b, x in enumerate(durations):
            d[b, :len(x)] = x
        dd = torch.from_numpy(d).to(DEV)
    try:
        mel, mel_lens, dur = eng.acoustic(torch.from_numpy(tok).to(DEV), lens, t_cap, durations=dd, return_durations=True,
                                          speaker_embedding=None if spk is None else torch.from_numpy(np.ascontiguousarray(spk)))
        torch.cuda.synchronize()
        return mel.cpu().numpy(), mel_lens.cpu().numpy(), dur.cpu().numpy()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error, nothing more is started on the GPU: {e}", returncode=3)
        raise


def run_ragged(eng, name, t_cap=ac.T_CAP):
    ids, durs = ac.ragged_inputs(name)
    return run(eng, ids, t_cap, durs, ac.speaker_embeddings(name, len(ids)))


def run_predicted(eng, name):
    ids = ac.predicted_inputs(name)
    return run(eng, ids, PRED_CAP, None, ac.speaker_embeddings(name, len(ids)))


def with_kinds(eng, f):
    """-> (f(), {kernel family: launches}) of the forwards f makes"""
    eng.profile(True)
    try:
        eng.profile_read_kinds()
        out = f()
        kinds = {k: v[2] for k, v in eng.profile_read_kinds().items()}
    finally:
        eng.profile(False)
    return out, kinds


def check_lengths(name, out, forced=True):
    """Frame counts, durations and the zero tail against the oracle's; -> the references."""
    mel, mel_lens, dur = out
    refs = ac.oracle64(name) if forced else ac.predicted_oracle64(name)
    assert np.isfinite(mel).all()
    for b, r in enumerate(refs):
        n = len(r["durations"])
        np.testing.assert_array_equal(dur[b, :n], r["durations"], err_msg=f"{name} b={b}")
        assert int(mel_lens[b]) == int(r["durations"].sum()) == r["mel"].shape[0], (name, b)
        assert np.all(mel[b, int(mel_lens[b]):] == 0), (name, b)
    return refs


def assert_fp32(name, out, forced=True):
    refs = check_lengths(name, out, forced)
    for b, r in enumerate(refs):
        L = r["mel"].shape[0]
        np.testing.assert_allclose(out[0][b, :L], r["mel"], atol=FP32_ATOL, rtol=FP32_RTOL, err_msg=f"{name} b={b} L={L}")


def check16(tag, name, dtype, out, forced=True):
    refs = check_lengths(name, out, forced)
    for b, r in enumerate(refs):
        L = r["mel"].shape[0]
        check(f"ac cfg {name} {dtype} {tag} b={b} ({L} frames)", out[0][b, :L], r["mel"], kind="ac_" + dtype)


def assert_same(a, b, what):
    for x, y, part in zip(a, b, ("mel", "mel_lens", "durations")):
        assert np.array_equal(x, y), (what, part)


def expect_kinds(name, dtype, k):
    """What the configuration fixes, as zero / non-zero launches."""
    print(f"[kinds] {name} {dtype}: " + ", ".join(f"{n} {c}" for n, c in k.items() if c))
    assert (k["rel_attn_kernel"] > 0) == (name in ac.FUSED_ATTN)   # head size 192 only
    assert k["acoustic_elementwise"] > 0
    # the exact encoder side (fp32 models too): split-precision GEMMs; every hidden size here is a
    # multiple of 64, so its projections are eligible
    assert k["conv_split_kernel"] > 0
    # the four-launch attention's head-batched GEMMs and the 80-channel postnet input
    assert k["conv_gemm_kernel"] > 0
    if dtype == "f32":
        assert k["conv_xres_kernel"] == 0
    else:
        assert k["conv_xres_kernel"] > 0   # the 16-bit decoder's FFN, projections and pointwise convs
    assert k["mrf_pair_kernel"] == k["mrf_chain_kernel"] == k["upsample_stream_kernel"] == 0


# ------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("name", NAMES)
def test_fp32_matches_oracle(name):
    """Every case in fp32 against the float64 oracle: the ragged batch with its durations forced
    (zeros among them) and the smaller batch with predicted durations, which equal the oracle's
    exactly.  h64 and h128 are the shapes whose predictor / postnet buffers used to be too small."""
    eng = engine_for(name, "f32")
    out, kinds = with_kinds(eng, lambda: run_ragged(eng, name))
    assert_fp32(name, out)
    expect_kinds(name, "f32", kinds)
    assert_fp32(name, run_predicted(eng, name), forced=False)


@pytest.mark.parametrize("name", ac.SPLIT_ENC_CASES)
def test_fp32_mfma_encoder_matches_oracle(name, switch):
    """The same with every layer on fp32 MFMA (TTS_F32_ENC_SPLIT=0 at finalize): the default's
    durations, the same bar."""
    switch("TTS_F32_ENC_SPLIT", 0)
    eng = new_engine(name, "f32")
    switch("TTS_F32_ENC_SPLIT", None)
    try:
        assert not eng.range_guard
        out, kinds = with_kinds(eng, lambda: run_ragged(eng, name))
        assert kinds["conv_split_kernel"] == 0 and kinds["conv_gemm_kernel"] > 0
        assert_fp32(name, out)
        pred = run_predicted(eng, name)
        assert_fp32(name, pred, forced=False)
        base = run_predicted(engine_for(name, "f32"), name)
        assert np.array_equal(pred[1], base[1]) and np.array_equal(pred[2], base[2])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ f16 / bf16
@pytest.mark.parametrize("dtype", ac.DTYPES16)
@pytest.mark.parametrize("name", NAMES)
def test_16bit_forced_durations_within_the_project_bars(name, dtype):
    eng = engine_for(name, dtype)
    out, kinds = with_kinds(eng, lambda: run_ragged(eng, name))
    check16("forced", name, dtype, out)
    expect_kinds(name, dtype, kinds)


def test_16bit_fast_encoder_within_the_project_bars():
    """encoder_precision="fast": the encoder side in the 16-bit dtype too (no split kernels).
    The case is the one with the most bf16 layers at the widest rows (two encoder layers and a
    decoder layer at D = 384), all on the four-launch attention, which stores its scores and
    probabilities in bf16 where the fused kernel keeps them in fp32.  Measured on MI355X: relative
    RMS 1.9e-2 on the 3-frame utterance (bar 2e-2) and max-abs 9.6e-2 (bar 0.1); the one-layer
    cases measure 1.1e-2 to 1.2e-2 / 6.2e-2 to 8.2e-2 under "fast" and the two-plus-two-layer case
    1.6e-2 / 8.3e-2, so the error follows the number of bf16 layers, not a shape."""
    name = ac.FAST_CASE
    eng = engine_for(name, "bf16", "fast")
    out, kinds = with_kinds(eng, lambda: run_ragged(eng, name))
    print("[kinds] fast: " + ", ".join(f"{n} {c}" for n, c in kinds.items() if c))
    assert kinds["conv_split_kernel"] == 0 and kinds["conv_xres_kernel"] > 0 and kinds["acoustic_elementwise"] > 0
    check16("fast encoder", name, "bf16", out)


@pytest.mark.parametrize("dtype", ac.DTYPES16)
@pytest.mark.parametrize("name", ac.DUR16_CASES)
def test_16bit_predicted_durations_equal_the_oracle(name, dtype):
    """The exact encoder of a 16-bit model: predicted durations equal to the oracle's on every
    token, so the mel compares frame for frame."""
    check16("predicted", name, dtype, run_predicted(engine_for(name, dtype), name), forced=False)


# every setting test_acoustic_gpu.py compares bit for bit at the default shape
SWITCHES = [
    {"TTS_XRES_NT": 2}, {"TTS_XRES_NT": 3}, {"TTS_XRES_NT": 4},
    {"TTS_XRES_NARROW": 0}, {"TTS_XRES_NARROW": 1},
    {"TTS_XRES_NARROW": 0, "TTS_XRES_NT": 2}, {"TTS_XRES_NARROW": 0, "TTS_XRES_NT": 3}, {"TTS_XRES_NARROW": 0, "TTS_XRES_NT": 4},
    {"TTS_XRES_DMA": 2}, {"TTS_XRES_DMA": 3},
    {"TTS_XRES_NARROW": 0, "TTS_XRES_DMA": 2, "TTS_XRES_NT": 2}, {"TTS_XRES_NARROW": 0, "TTS_XRES_DMA": 3, "TTS_XRES_NT": 4},
    {"TTS_XRES_ORDER": 0}, {"TTS_XRES_ORDER": 1}, {"TTS_XRES_ORDER": 2}, {"TTS_XRES_ORDER": 0, "TTS_XRES_NT": 2},
    {"TTS_LN_FUSE": 0}, {"TTS_LN_FUSE": 7},
    {"TTS_SPLIT_NT1": 0}, {"TTS_SPLIT_NT1": 1}, {"TTS_SPLIT_NT1": 4}, {"TTS_SPLIT_NT1": 1, "TTS_LN_FUSE": 7},
    {"TTS_SPLIT_WHOLE": 0},
    {"TTS_VP_BATCH": 0},
    {"TTS_DEC_TRIM": 0}, {"TTS_DEC_TRIM": 1},
]
SWITCHES_F32 = [s for s in SWITCHES if set(s) <= {"TTS_VP_BATCH", "TTS_DEC_TRIM"}]


@pytest.mark.parametrize("dtype", ac.DTYPES16 + ("f32",))
@pytest.mark.parametrize("name", NAMES)
def test_path_switches_bit_identical(name, dtype, switch):
    """Tile heights, narrow tiles, the LDS-DMA forms, the XCD-ordered grid, the fused post-LNs, the
    split GEMMs' tile heights and whole-slice staging, the batched predictors and the decoder
    extent: mel, frame counts and durations equal the automatic path's bit for bit, on the ragged
    batch (durations forced) and on the predicted-duration batch.  fp32 models: the batched
    predictors and the decoder extent."""
    eng = engine_for(name, dtype)
    base = run_ragged(eng, name), run_predicted(eng, name)
    for setting in (SWITCHES_F32 if dtype == "f32" else SWITCHES):
        for k, v in setting.items():
            switch(k, v)
        got = run_ragged(eng, name), run_predicted(eng, name)
        for k in setting:
            switch(k, None)
        assert_same(got[0], base[0], (setting, "ragged"))
        assert_same(got[1], base[1], (setting, "predicted"))


@pytest.mark.parametrize("dtype", ac.DTYPES16 + ("f32",))
def test_fused_attention_at_one_head_matches_unfused(dtype, switch):
    """D = 192, H = 1: the fused relative-position attention against the four-launch path
    (TTS_REL_ATTN=0), at the tolerance test_fused_rel_attention_matches_unfused_and_oracle uses."""
    name = ac.FUSED_ATTN[0]
    eng = engine_for(name, dtype)
    switch("TTS_REL_ATTN", 1)
    fused, kf = with_kinds(eng, lambda: run_ragged(eng, name))
    switch("TTS_REL_ATTN", 0)
    unfused, ku = with_kinds(eng, lambda: run_ragged(eng, name))
    switch("TTS_REL_ATTN", None)
    assert kf["rel_attn_kernel"] > 0 and ku["rel_attn_kernel"] == 0
    tol = {"bf16": 2.5e-2, "f16": 5e-3, "f32": 1e-5}[dtype]
    for tag, out in (("REL_ATTN=1", fused), ("REL_ATTN=0", unfused)):
        if dtype == "f32":
            assert_fp32(name, out)
        else:
            check16(tag, name, dtype, out)
    for b, L in enumerate(ac.FRAMES):
        e = rel_rms(fused[0][b, :L], unfused[0][b, :L])
        assert e <= tol, (b, e)


# ------------------------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_utterance_alone_equals_its_rows_in_the_batch(name, dtype):
    """Every utterance of the ragged batch run alone, at a frame budget of exactly its own frames
    (96 frames: a decoder row stride with no pad row in 16-bit), equals its rows in the batch bit
    for bit."""
    eng = engine_for(name, dtype)
    ids, durs = ac.ragged_inputs(name)
    spk = ac.speaker_embeddings(name, len(ids))
    mel, mel_lens, _ = run(eng, ids, ac.T_CAP, durs, spk)
    for b, L in enumerate(ac.FRAMES):
        m1, l1, _ = run(eng, [ids[b]], L, [durs[b]], None if spk is None else spk[b:b + 1])
        assert int(l1[0]) == int(mel_lens[b]) == L
        assert np.array_equal(m1[0], mel[b, :L]), (name, dtype, b, float(np.abs(m1[0] - mel[b, :L]).max()))


# ------------------------------------------------------------------------- the supported envelope
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(ac.OUTSIDE))
def test_configuration_outside_the_envelope_is_rejected_at_load(case, dtype):
    """A model some dtype, encoder precision or switch setting could not run is refused when the
    weights are finalized, in every dtype, with a message naming the tensor and the limit; nothing
    is uploaded and no kernel runs."""
    make, tensor, words = ac.OUTSIDE[case]
    eng = HipEngine(DEV, vocoder_dtype="f32", acoustic_dtype=dtype)
    try:
        held = device_bytes(DEV)
        with pytest.raises(RuntimeError) as ei:
            eng.load_weights(acoustic=make())
        msg = str(ei.value)
        print(msg)
        assert "acoustic envelope: " + tensor + ":" in msg
        for w in words:
            assert w in msg, (w, msg)
        assert not eng._finalized and device_bytes(DEV) == held
    finally:
        eng.close()
