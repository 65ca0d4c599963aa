"""The HIP vocoder on small HiFi-GAN configurations other than V1 (tests/vocoder_cases.py) against
the float64 oracle.

fp32 runs are held to the project's fp32 bar (atol 1e-5, rtol 1e-4): the structural test, where a
wrong tap order, stride, phase or dilation is off by orders of magnitude.  f16 / bf16 runs are
bounded per utterance by 3x the error of the storage-rounding model (oracle/vocoder_rounded.py)
for that case and dtype, computed here from the reference alone (vocoder_cases.bound): relative RMS
and max-abs on every non-empty utterance, the 1- and 2-frame ones included.  The kernel-path switches are
compared on the new shapes bit for bit where the V1 tests assert bit identity, and the profiler's
per-kind launch counts show that each case ran the kernel family it is there for.

Measured 16-bit errors go through parity.check, so they land in $PARITY_LOG
(profiles/vocoder_configs_parity.json is that log from an MI355X run).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import vocoder_cases as vc  # noqa: E402
from gonova_tts_amd.engine import HipEngine  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda:0"
NAMES = list(vc.CASES)
_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def engine_for(name, dtype):
    if (name, dtype) not in _ENG:
        e = HipEngine(DEV, vocoder_dtype=dtype)
        e.load_weights(vocoder=vc.weights(name), vocoder_cfg=vc.CASES[name])
        assert e.hop == vc.CASES[name].hop
        _ENG[name, dtype] = e
    return _ENG[name, dtype]


def device_batch(mel, lens):
    return torch.from_numpy(mel).to(DEV), torch.tensor(lens, dtype=torch.int32)


def run(eng, mel_d, ln):
    return eng.vocoder(mel_d, ln).cpu().numpy()


def run_kinds(eng, mel_d, ln):
    """-> (waveforms, {kernel family: launches}) of one pass"""
    eng.profile(True)
    try:
        eng.profile_read_kinds()
        wav = run(eng, mel_d, ln)
        kinds = {k: v[2] for k, v in eng.profile_read_kinds().items()}
    finally:
        eng.profile(False)
    return wav, kinds


def assert_zero_tail(wav, lens, hop):
    for b, L in enumerate(lens):
        assert np.all(wav[b, L * hop:] == 0), (b, L)


def check16(tag, name, dtype, wav, lens, refs):
    """Every utterance against its float64 oracle under the case's 3x-model bound."""
    hop = vc.CASES[name].hop
    be, bm = vc.bound(name, dtype)
    assert np.isfinite(wav).all(), tag
    assert_zero_tail(wav, lens, hop)
    for b, L in enumerate(lens):
        if L:
            check(f"cfg {name} {dtype} {tag} b={b} ({L} frames)", wav[b, :L * hop], refs[b], rel_rms_tol=be, max_abs_tol=bm)


def assert_same(a, b, lens, what):
    for i in range(len(lens)):
        assert np.array_equal(a[i], b[i]), (what, i, lens[i], float(np.abs(a[i] - b[i]).max()))


# ------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("name", NAMES)
def test_fp32_matches_oracle(name):
    """Every case in fp32 (conv_gemm, split-precision and split-K forms at the new shapes) against
    the float64 oracle per utterance; the tail past each length exactly zero."""
    cfg = vc.CASES[name]
    eng = engine_for(name, "f32")
    mel, lens = vc.ragged_mel(name)
    wav, kinds = run_kinds(eng, *device_batch(mel, lens))
    refs = vc.oracle64(name)
    assert np.isfinite(wav).all()
    assert_zero_tail(wav, lens, cfg.hop)
    for b, L in enumerate(lens):
        if L:
            np.testing.assert_allclose(wav[b, :L * cfg.hop], refs[b], atol=1e-5, rtol=1e-4, err_msg=f"{name} b={b} L={L}")
    assert kinds["conv_gemm_kernel"] + kinds["conv_split_kernel"] > 0
    assert kinds["mrf_pair_kernel"] == kinds["mrf_chain_kernel"] == kinds["upsample_stream_kernel"] == 0
    if name == "odd":
        assert kinds["conv_gemm_kernel"] >= 21  # conv_pre, both upsamplers, the 18 convs at C = 48


# ------------------------------------------------------------------------------------ f16 / bf16
# The kernel families each case is there for, as zero / non-zero launches of one default 16-bit
# pass.  How many launches a family takes depends on build knobs (which shapes have a chain
# kernel, a fused upsampler, pair kernels at C = 256), so no count is asserted -- only what the
# configuration itself fixes: a resblock of two pairs has no chain kernel, a 1-, 3- or 4-tap or
# stride-4-to-256 upsampler no streaming kernel, 48 channels no pair or X-resident kernel.
def expect_kinds(name, k):
    pair, chain, up, xres, gemm = (k["mrf_pair_kernel"], k["mrf_chain_kernel"], k["upsample_stream_kernel"],
                                   k["conv_xres_kernel"], k["conv_gemm_kernel"])
    assert gemm > 0           # conv_pre (80 input channels) on the generic kernel
    assert pair + chain > 0   # the fused resblock kernels ran: no silent per-conv fallback
    if name in ("one", "two", "nk1", "stream4"):
        assert up > 0 and xres == 0
    elif name in ("four", "v3four", "v3ish", "taps32"):
        assert up > 0 and xres > 0
    elif name == "taps41":
        assert up == 0 and xres > 0
    elif name == "odd":
        # conv_pre, both upsamplers and the 18 convs at C = 48 have no other kernel
        assert gemm >= 21 and xres == 0 and up == 0
    if name in ("v3ish", "v3four"):
        assert chain == 0 and pair > 0


@pytest.mark.parametrize("dtype", vc.DTYPES16)
@pytest.mark.parametrize("name", NAMES)
def test_16bit_matches_oracle_within_model_bound(name, dtype):
    eng = engine_for(name, dtype)
    mel, lens = vc.ragged_mel(name)
    wav, kinds = run_kinds(eng, *device_batch(mel, lens))
    print(f"[kinds] {name} {dtype}: " + ", ".join(f"{k} {n}" for k, n in kinds.items() if n))
    check16("default", name, dtype, wav, lens, vc.oracle64(name))
    expect_kinds(name, kinds)


@pytest.mark.parametrize("dtype", vc.DTYPES16)
@pytest.mark.parametrize("name", NAMES)
def test_path_switches_agree(name, dtype, switch):
    """The alternative kernel paths on the new shapes.  Bit for bit: chain against pairs, fused
    against separate conv_post, short against full-height tiles, channel-split against whole pairs,
    fused against separate upsampler.  Within the 3x-model bound of each other and of the oracle:
    fused against per-conv resblocks, streaming against polyphase upsamplers."""
    eng = engine_for(name, dtype)
    mel, lens = vc.ragged_mel(name)
    md, ln = device_batch(mel, lens)
    refs = vc.oracle64(name)
    hop = vc.CASES[name].hop
    base, kb = run_kinds(eng, md, ln)

    switch("TTS_MRF_CHAIN", 0)
    pairs, kp = run_kinds(eng, md, ln)
    # (a chain launch is one resblock of three pairs)
    assert kp["mrf_chain_kernel"] == 0 and kp["mrf_pair_kernel"] == kb["mrf_pair_kernel"] + 3 * kb["mrf_chain_kernel"]
    assert_same(pairs, base, lens, "chain vs pairs")

    # (every resblock as pair launches from here on)
    switch("TTS_POST_FUSE", 0)
    assert_same(run(eng, md, ln), pairs, lens, "fused vs separate conv_post")
    switch("TTS_POST_FUSE", None)

    switch("TTS_PAIR_SPLIT", 0)
    switch("TTS_PAIR_DIV", 0)
    short = run(eng, md, ln)
    switch("TTS_PAIR_DIV", 1)
    full = run(eng, md, ln)
    assert_same(short, full, lens, "short vs full-height tiles")
    assert_same(full, pairs, lens, "forced vs automatic tiles")
    switch("TTS_PAIR_SPLIT", 1)
    assert_same(run(eng, md, ln), full, lens, "channel-split vs whole pairs")
    switch("TTS_PAIR_SPLIT", None)

    # full-height tiles: the stage-final pairs may carry the next two-tap upsampler
    switch("TTS_UP_FUSE", 1)
    fused, kf = run_kinds(eng, md, ln)
    switch("TTS_UP_FUSE", 0)
    sep, ks = run_kinds(eng, md, ln)
    assert_same(fused, sep, lens, "fused vs separate upsampler")
    assert_same(fused, full, lens, "upsampler fusion vs the automatic path")
    # how many stage-final pairs carry the next upsampler is a build choice; the configuration
    # only says which cases have a candidate (a k = 11 pair before a two-tap C -> C upsampler)
    n_fused = ks["upsample_stream_kernel"] - kf["upsample_stream_kernel"]
    print(f"[up-fuse] {name} {dtype}: {n_fused} upsampler(s) fused into a pair launch")
    assert 0 <= n_fused <= {"two": 1, "four": 2, "taps32": 1}.get(name, 0), (kf, ks)
    switch("TTS_UP_FUSE", None)
    switch("TTS_PAIR_DIV", None)
    switch("TTS_MRF_CHAIN", None)

    be, bm = vc.bound(name, dtype)
    for sw_name, fam in (("TTS_MRF_FUSED", ("mrf_pair_kernel", "mrf_chain_kernel")),
                         ("TTS_UP_STREAM", ("upsample_stream_kernel",))):
        switch(sw_name, 0)
        alt, ka = run_kinds(eng, md, ln)
        switch(sw_name, None)
        assert all(ka[f] == 0 for f in fam), (sw_name, ka)
        check16(f"{sw_name}=0", name, dtype, alt, lens, refs)
        for b, L in enumerate(lens):
            if L:
                n = L * hop
                check(f"cfg {name} {dtype} {sw_name}=0 vs default b={b}", alt[b, :n], base[b, :n],
                      rel_rms_tol=be, max_abs_tol=bm)


# ---------------------------------------------------------------------------------- length sweep
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", list(vc.SWEEP))
def test_length_sweep(name, dtype, switch):
    """40 utterances of consecutive lengths sharing one mel prefix, across a tile edge of every
    stage: each against the oracle of its own length, and the batch against each utterance run
    alone, bit for bit (f16: on the automatic and on the full-height tiles)."""
    cfg = vc.CASES[name]
    eng = engine_for(name, dtype)
    mel, lens = vc.sweep_mel(name)
    md, ln = device_batch(mel, lens)
    refs = vc.oracle64(name, "sweep")
    for div in ((None,) if dtype == "f32" else (None, 1)):
        switch("TTS_PAIR_DIV", div)
        wav = run(eng, md, ln)
        assert_zero_tail(wav, lens, cfg.hop)
        if dtype == "f32":
            for b, L in enumerate(lens):
                np.testing.assert_allclose(wav[b, :L * cfg.hop], refs[b], atol=1e-5, rtol=1e-4, err_msg=f"{name} L={L}")
        else:
            check16(f"sweep div={div}", name, dtype, wav, lens, refs)
        for b, L in enumerate(lens):
            solo = eng.vocoder(md[b:b + 1, :L].contiguous()).cpu().numpy()[0]
            assert np.array_equal(solo, wav[b, :L * cfg.hop]), (name, dtype, div, L)


# ------------------------------------------------------------------------- the supported envelope
def _v1ish(c0, rates, kernels, rk=(7,), rd=((1, 3, 5),)):
    return vc._cfg(c0, rates, kernels, rk, rd)


OUTSIDE = {
    # name: (configuration, what the message must name)
    "last_stage_64": (_v1ish(128, (2,), (4,)), ["conv_post.weight", "32"]),
    "odd_k_minus_s": (_v1ish(64, (3,), (6,)), ["upsampler.0.weight", "stride"]),
    "receptive_field": (_v1ish(64, (2,), (4,), (7,), ((1, 12),)), ["resblocks.0.convs1.1.weight", "72", "64"]),
    "channels_not_16_bytes": (vc.PlannedVocoderConfig(upsample_initial_channel=96, upsample_rates=(2, 2),
                                                      upsample_kernel_sizes=(4, 4), resblock_kernel_sizes=(7,),
                                                      resblock_dilation_sizes=((1, 3, 5),), channel_plan=(44, 32)),
                              ["upsampler.0.weight", "44", "multiple of 8"]),
}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("case", list(OUTSIDE))
def test_configuration_outside_the_envelope_is_rejected_at_load(case, dtype):
    """A configuration some dtype or switch setting could not run is refused when the weights are
    finalized, in every dtype, with a message naming the tensor and the limit (no kernel runs)."""
    from gonova_tts_amd.weights import make_vocoder_weights
    cfg, words = OUTSIDE[case]
    eng = HipEngine(DEV, vocoder_dtype=dtype)
    try:
        with pytest.raises(RuntimeError) as ei:
            eng.load_weights(vocoder=make_vocoder_weights(0, cfg), vocoder_cfg=cfg)
        msg = str(ei.value)
        print(msg)
        assert "vocoder envelope" in msg
        for w in words:
            assert w in msg, (w, msg)
        assert not eng._finalized
    finally:
        eng.close()


def test_conv_post_other_than_seven_taps_is_rejected():
    """The conv_post kernels read as general in k, but only 7 taps have ever run: anything else is
    outside the envelope until it is tested."""
    w = dict(vc.weights("one"))
    w["conv_post.weight"] = np.zeros((1, 32, 9), np.float32)
    eng = HipEngine(DEV, vocoder_dtype="f16")
    try:
        with pytest.raises(RuntimeError, match="conv_post.weight: kernel size 9"):
            eng.load_weights(vocoder=w, vocoder_cfg=vc.CASES["one"])
    finally:
        eng.close()


def test_four_pairs_without_a_dilation_table_are_rejected():
    """Without __cfg__.resblock_dilation_sizes the dilations default to 1, 3, 5 by pair index;
    a resblock of more pairs has no default."""
    from gonova_tts_amd.weights import make_vocoder_weights
    cfg = _v1ish(64, (2,), (4,), (3,), ((1, 3, 5, 7),))
    eng = HipEngine(DEV, vocoder_dtype="f16")
    try:
        for k, v in make_vocoder_weights(0, cfg).items():
            eng.set_weight(k, v)
        assert eng.lib.tts_engine_finalize(eng.handle) != 0
        msg = eng.lib.tts_last_error().decode()
        assert "resblocks.0.convs1.3.weight" in msg and "__cfg__.resblock_dilation_sizes" in msg
    finally:
        eng.close()
