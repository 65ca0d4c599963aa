"""Chunked streaming on HiFi-GAN configurations other than V1 (tests/vocoder_cases.py).

A window that carries the generator's receptive field on each side of a chunk (or reaches the
utterance's edge) feeds every kept sample the inputs the whole-utterance pass feeds it, and the
kernels sum each output row in an order that does not depend on where the row sits in a tile or a
window -- so the chunks equal the full pass bit for bit, the project's claim for V1.  Here it is
held on every small case, in every dtype, at the op (tts_vocoder_forward_chunk: no context at the
ends, a one-frame chunk, windows longer than an utterance, windows wholly past one, utterances that
end on a chunk edge), on two alternative kernel paths, and through GonovaTTS.stream_tokens /
stream_batch with the chunked resampler behind a hop of 2 and 8.  The context comes from
config.vocoder_context_frames, which the engine's own derivation (tts_vocoder_context) must equal;
with the 16 frames that were a constant before, the same comparison fails (test_context_of_16...).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import vocoder_cases as vc  # noqa: E402
from gonova_tts_amd.config import AcousticConfig, VocoderConfig, vocoder_context_frames  # noqa: E402
from gonova_tts_amd.engine import HipEngine  # noqa: E402
from gonova_tts_amd.model import GonovaTTS  # noqa: E402
from gonova_tts_amd.weights import make_acoustic_weights, make_vocoder_weights  # noqa: E402

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


def context_of(name):
    left, right = vocoder_context_frames(vc.CASES[name])
    assert left == right
    return left


# ------------------------------------------------------------------------ (a) the two derivations
@pytest.mark.parametrize("name", NAMES)
def test_engine_context_equals_the_python_derivation(name):
    """tts_vocoder_context, from the taps / dilations / strides of the packed layers, against
    config.vocoder_context_frames, from the configuration."""
    assert engine_for(name, "f16").vocoder_context() == vocoder_context_frames(vc.CASES[name])


def test_engine_context_v1_and_state():
    """V1 is (13, 13) on both sides; before finalize, and on an engine without a vocoder, the
    entry answers TTS_ERR_STATE (-3: "bad state")."""
    eng = HipEngine(DEV, vocoder_dtype="f16")
    try:
        with pytest.raises(RuntimeError, match="bad state"):
            eng.vocoder_context()
        eng.load_weights(vocoder=make_vocoder_weights(0))
        assert eng.vocoder_context() == vocoder_context_frames(VocoderConfig()) == (13, 13)
    finally:
        eng.close()
    eng = HipEngine(DEV, acoustic_dtype="f32")
    try:
        eng.load_weights(acoustic=make_acoustic_weights(0))
        with pytest.raises(RuntimeError, match="bad state"):
            eng.vocoder_context()
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (b) the op level
def op_batch(name):
    """-> (mel [6, T, 80] float32 random in every frame, lens, T): utterances of 0, 1, 7 and 32
    frames (the last two end exactly on an edge of the 7- and 32-frame chunks), one a little longer
    than a context and one that fills T = 2 c + 40."""
    c = context_of(name)
    T = 2 * c + 40
    lens = [0, 1, 7, 32, c + 33, T]
    rng = np.random.default_rng(3000 + NAMES.index(name))
    return rng.standard_normal((len(lens), T, 80)).astype(np.float32), lens, T


def full_and_chunks(eng, name, n, ctx):
    """The full pass of the case's batch and the same frames in chunks of n with ctx frames of
    context per side -> (full [B, T*hop], [(c0, frames, chunk [B, frames*hop])]), numpy."""
    mel, lens, T = op_batch(name)
    md = torch.from_numpy(mel).to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    full = eng.vocoder(md, ln)
    out = []
    for c0 in range(0, T, n):
        tc = min(n, T - c0)
        w0, w1 = max(0, c0 - ctx), min(T, c0 + tc + ctx)
        win_lens = torch.clamp(ln - w0, min=0, max=w1 - w0)
        out.append((c0, tc, eng.vocoder_chunk(md[:, w0:w1].contiguous(), win_lens, c0 - w0, tc)))
    cat = torch.cat([w for _, _, w in out], dim=1).cpu().numpy()  # one copy for all chunks
    hop = eng.hop
    return full.cpu().numpy(), [(c0, tc, cat[:, c0 * hop:(c0 + tc) * hop]) for c0, tc, _ in out]


def differing_chunks(full, chunks, hop):
    """[(c0, utterance, max |difference|)] of the chunks that are not the full pass's samples"""
    bad = []
    for c0, tc, w in chunks:
        want = full[:, c0 * hop:(c0 + tc) * hop]
        assert w.shape == want.shape
        for b in range(full.shape[0]):
            if not np.array_equal(w[b], want[b]):
                bad.append((c0, b, float(np.abs(w[b] - want[b]).max())))
    return bad


def assert_chunks_equal_full(eng, name, sizes, tag):
    cfg = vc.CASES[name]
    _, lens, T = op_batch(name)
    for n in sizes:
        full, chunks = full_and_chunks(eng, name, n, context_of(name))
        assert np.isfinite(full).all()
        for b, L in enumerate(lens):  # a waveform, then exact zeros
            assert np.all(full[b, L * cfg.hop:] == 0) and (L == 0 or np.abs(full[b, :L * cfg.hop]).max() > 0)
        assert sum(tc for _, tc, _ in chunks) == T
        bad = differing_chunks(full, chunks, cfg.hop)
        assert not bad, (name, tag, f"chunks of {n}", bad[:6])


def chunk_sizes(name):
    return (1, 7, 32) if name in ("one", "v3ish") else (7, 32)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_chunks_equal_full_pass_bit_for_bit(name, dtype):
    """Every chunk == the same frames of the full pass (np.array_equal), the zeros past each
    utterance's end and the chunks that lie wholly past an utterance (win_lens 0) included; the
    first and the last chunk have no context on one side."""
    assert_chunks_equal_full(engine_for(name, dtype), name, chunk_sizes(name), dtype)


# ----------------------------------------------------------------------------------- (c) power
def test_context_of_16_frames_is_not_enough_at_hop_2():
    """`one` (hop 2) needs 35 frames; with the 16 that fit V1 some chunk differs from the full
    pass -- the comparison above can fail, and does against a constant context."""
    assert context_of("one") == 35 > GonovaTTS.STREAM_CONTEXT == 16
    eng = engine_for("one", "f32")
    # (what stream_tokens cuts its windows with: not the constant)
    assert GonovaTTS(eng, AcousticConfig(), vc.CASES["one"]).stream_context == 35
    full, chunks = full_and_chunks(eng, "one", 7, GonovaTTS.STREAM_CONTEXT)
    bad = differing_chunks(full, chunks, eng.hop)
    worst = max((e for _, _, e in bad), default=0.0)
    print(f"[context 16] one f32: {len(bad)} (chunk, utterance) pairs differ, worst {worst:.3g}")
    assert bad


# ---------------------------------------------------------------------------- (d) kernel switches
@pytest.mark.parametrize("sw_name", ["TTS_MRF_FUSED", "TTS_UP_STREAM"])
@pytest.mark.parametrize("name", ["two", "v3ish"])
def test_chunks_equal_full_pass_on_the_alternative_paths(name, sw_name, switch):
    """Per-conv resblocks / polyphase upsamplers: chunks equal that path's own full pass."""
    switch(sw_name, 0)
    assert_chunks_equal_full(engine_for(name, "f16"), name, (32,), f"f16 {sw_name}=0")


# ------------------------------------------------------------------------------ (e) model level
@pytest.fixture(scope="module", params=["one", "v3ish"])
def models(request):
    """(native-rate model, 24 kHz model) on one engine: the seeded default acoustic model in fp32
    and the case's vocoder in f16."""
    name = request.param
    cfg = vc.CASES[name]
    eng = HipEngine(DEV, vocoder_dtype="f16", acoustic_dtype="f32")
    eng.load_weights(vocoder=vc.weights(name), acoustic=make_acoustic_weights(0), vocoder_cfg=cfg)
    yield GonovaTTS(eng, AcousticConfig(), cfg), GonovaTTS(eng, AcousticConfig(), cfg, sample_rate=24000)
    eng.close()


def given_batch():
    """Three utterances of 60, 20 and 32 tokens with given durations of 1-3 frames: the second has
    40 frames (an edge of the 5-frame chunks), the third 64 (an edge of the 32-frame ones)."""
    rng = np.random.default_rng(5)
    lens = np.array([60, 20, 32], np.int32)
    tok = np.zeros((3, 60), np.int32)
    dur = np.zeros((3, 60), np.int32)
    for i, L in enumerate(lens):
        tok[i, :L] = rng.integers(1, 78, size=L)
        dur[i, :L] = rng.integers(1, 4, size=L)
    dur[1, :20] = 2
    dur[2, :32] = 2
    return tok, lens, dur


def stream_pieces(m, tok, lens, chunk_frames, **kw):
    pieces = [[] for _ in range(len(lens))]
    for c0, wav, valid in m.stream_tokens(tok, lens, chunk_frames=chunk_frames, **kw):
        assert wav.shape[1] >= int(valid.max())
        w = wav.cpu().numpy()
        for b in range(len(lens)):
            pieces[b].append(w[b, :valid[b]])
    return [np.concatenate(p) for p in pieces]


def test_stream_tokens_equals_synthesize_tokens(models):
    """Default context (the receptive field: 35 / 20 frames), chunks of 32 and 5 frames."""
    m, _ = models
    tok, lens, dur = given_batch()
    hop = m.vocoder_cfg.hop
    assert m.stream_context == max(vocoder_context_frames(m.vocoder_cfg)) > 16
    full, full_lens = m.synthesize_tokens(tok, lens, durations=dur)
    full = full.cpu().numpy()
    np.testing.assert_array_equal(full_lens, dur.sum(axis=1) * hop)
    assert full_lens[1] == 40 * hop and full_lens[2] == 64 * hop
    for chunk in (32, 5):
        got = stream_pieces(m, tok, lens, chunk, durations=dur)
        for b in range(3):
            assert got[b].shape[0] == full_lens[b] and np.abs(got[b]).max() > 0
            np.testing.assert_array_equal(got[b], full[b, :full_lens[b]], err_msg=f"chunks of {chunk}, utterance {b}")


def test_stream_tokens_at_24khz_equals_synthesize_tokens(models):
    """output_rate=24000 at chunks of 32 frames and of 1: a one-frame chunk is 2 (hop 2) or 8
    (hop 8) samples, fewer than the 20 the chunked resampler carries as history, which is then
    built over many chunks.  Against synthesize_tokens of a model at sample_rate=24000."""
    m, m24 = models
    tok, lens, dur = given_batch()
    hop = m.vocoder_cfg.hop
    assert hop < 20 and m24.sr == 24000
    full, full_lens = m24.synthesize_tokens(tok, lens, durations=dur)
    full = full.cpu().numpy()
    np.testing.assert_array_equal(full_lens, -(-dur.sum(axis=1) * hop * 160 // 147))
    for chunk in (32, 1):
        got = stream_pieces(m, tok, lens, chunk, durations=dur, output_rate=24000)
        for b in range(3):
            assert got[b].shape[0] == full_lens[b]
            np.testing.assert_array_equal(got[b], full[b, :full_lens[b]], err_msg=f"chunks of {chunk}, utterance {b}")


TEXTS = ["Good morning to everyone in the room.", "Yes.", "The quick brown fox jumps over the lazy dog!"]


def test_stream_batch_equals_generate_batch(models):
    """Predicted durations, the first chunk enqueued ahead of the host read, at 24 kHz: each
    sentence's pieces concatenate to generate_batch's audio."""
    _, m24 = models
    direct = m24.generate_batch(TEXTS)
    pieces = [[] for _ in TEXTS]
    finished = [0] * len(TEXTS)
    for out in m24.stream_batch(TEXTS, chunk_frames=32):
        for i, a, fin in out:
            assert not finished[i]
            pieces[i].append(a)
            finished[i] += bool(fin)
    assert finished == [1, 1, 1]
    assert max(len(p) for p in pieces) > 1
    for p, d in zip(pieces, direct):
        assert len(d) > 0
        np.testing.assert_array_equal(np.concatenate(p), d)
