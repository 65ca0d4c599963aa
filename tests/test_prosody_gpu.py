"""Per-utterance prosody controls through the engine (tts_acoustic_forward_ctl), the model and the
service, on the small configurations of acoustic_cases.py and the default model.

The neutral controls pin the fused variance-adaptor launch to the three launches it stands in for
(bit identity); a mixed batch shows that an utterance's bits depend on its own controls only; the
controlled mel is held to the float64 oracle restated with the controls (prosody_cases.py) at the
bars test_acoustic_configs_gpu.py applies to the uncontrolled forward.  Measured errors land in
$PARITY_LOG (profiles/prosody_parity.json is that log from an MI355X run)."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import acoustic_cases as ac  # noqa: E402
import prosody_cases as pc  # noqa: E402
from gonova_tts_amd.config import AcousticConfig, VocoderConfig  # noqa: E402
from gonova_tts_amd.engine import HipEngine  # noqa: E402
from gonova_tts_amd.model import GonovaTTS, prosody_controls  # noqa: E402
from gonova_tts_amd.weights import make_acoustic_weights, make_vocoder_weights  # noqa: E402
from parity import check  # noqa: E402
from test_acoustic_configs_gpu import PRED_CAP, assert_same, with_kinds  # noqa: E402
from test_acoustic_gpu import FP32_ATOL, FP32_RTOL  # noqa: E402

DEV = "cuda:0"
DTYPES = ("f32", "f16", "bf16")
_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def engine_for(name, dtype):
    if (name, dtype) not in _ENG:
        e = HipEngine(DEV, vocoder_dtype="f32", acoustic_dtype=dtype)
        e.load_weights(acoustic=ac.weights(name))
        _ENG[name, dtype] = e
    return _ENG[name, dtype]


def run(eng, ids_list, t_cap, durations=None, spk=None, prosody=None):
    """-> (mel, mel_lens, durations) as numpy arrays; prosody: list of control dicts or None"""
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
    blk = None if prosody is None else torch.from_numpy(pc.block(prosody)).to(DEV)
    try:
        mel, mel_lens, dur = eng.acoustic(torch.from_numpy(tok).to(DEV), lens, t_cap, durations=dd, return_durations=True,
                                          speaker_embedding=None if spk is None else torch.from_numpy(np.ascontiguousarray(spk)),
                                          prosody=blk)
        torch.cuda.synchronize()
        return mel.cpu().numpy(), mel_lens.cpu().numpy(), dur.cpu().numpy()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error, nothing more is started on the GPU: {e}", returncode=3)
        raise


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", pc.MODEL_CASES)
def test_neutral_controls_equal_the_plain_forward(name, dtype):
    """All-neutral control arrays through tts_acoustic_forward_ctl (the fused launch) give the
    plain forward's mel, frame counts and durations bit for bit, given and predicted durations;
    and the controlled forward enqueues no more elementwise launches than the neutral one."""
    eng = engine_for(name, dtype)
    ids, durs = ac.ragged_inputs(name)
    spk = ac.speaker_embeddings(name, len(ids))
    neutral = [pc.controls()] * len(ids)
    plain, k0 = with_kinds(eng, lambda: run(eng, ids, pc.T_CAP, durs, spk))
    fused, k1 = with_kinds(eng, lambda: run(eng, ids, pc.T_CAP, durs, spk, neutral))
    assert_same(fused, plain, (name, dtype, "given"))
    assert k1["acoustic_elementwise"] < k0["acoustic_elementwise"], (k0, k1)
    for k in k0:
        if k != "acoustic_elementwise":
            assert k1[k] == k0[k], (k, k0, k1)
    pids = ac.predicted_inputs(name)
    pspk = ac.speaker_embeddings(name, len(pids))
    assert_same(run(eng, pids, PRED_CAP, None, pspk, [pc.controls()] * len(pids)), run(eng, pids, PRED_CAP, None, pspk),
                (name, dtype, "predicted"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", pc.MODEL_CASES)
def test_mixed_batch_against_the_controlled_oracle(name, dtype):
    """One batch, a different control setting per utterance: durations and frame counts equal the
    oracle's scaled ones, the mel is within the uncontrolled forward's bars of the controlled
    float64 oracle, a neutral utterance has the uncontrolled forward's bits, and a controlled
    utterance alone equals itself inside the batch."""
    eng = engine_for(name, dtype)
    ids, durs = ac.ragged_inputs(name)
    spk = ac.speaker_embeddings(name, len(ids))
    ctls = pc.model_controls()
    mel, mel_lens, dur = run(eng, ids, pc.T_CAP, durs, spk, ctls)
    plain = run(eng, ids, pc.T_CAP, durs, spk)
    refs = pc.controlled_oracle64(name)
    assert int(max(r["mel"].shape[0] for r in refs)) == 260
    for b, r in enumerate(refs):
        n, L = len(r["durations"]), r["mel"].shape[0]
        np.testing.assert_array_equal(dur[b, :n], r["durations"], err_msg=f"{name} b={b}")
        assert int(mel_lens[b]) == L and np.all(mel[b, L:] == 0), (name, b)
        if ctls[b] == pc.controls():
            assert np.array_equal(mel[b], plain[0][b]), (name, dtype, b, "a neutral utterance moved")
        if dtype == "f32":
            np.testing.assert_allclose(mel[b, :L], r["mel"], atol=FP32_ATOL, rtol=FP32_RTOL, err_msg=f"{name} b={b}")
            check(f"prosody {name} f32 b={b} ({L} frames)", mel[b, :L], r["mel"])
        else:
            check(f"prosody {name} {dtype} b={b} ({L} frames)", mel[b, :L], r["mel"], kind="ac_" + dtype)
    for b in (1, 4, 6):
        alone = run(eng, [ids[b]], pc.T_CAP, [durs[b]], None if spk is None else spk[b:b + 1], [ctls[b]])
        L = int(mel_lens[b])
        assert int(alone[1][0]) == L and np.array_equal(alone[0][0, :L], mel[b, :L]), (name, dtype, b, "alone")
        assert np.array_equal(alone[2][0, :len(ids[b])], dur[b, :len(ids[b])])


@pytest.mark.parametrize("name", pc.MODEL_CASES)
def test_predicted_durations_scale(name):
    """Predicted durations under scale s equal rint(float32(d0) * float32(s)), d0 the oracle's."""
    eng = engine_for(name, "f32")
    ids = ac.predicted_inputs(name)
    spk = ac.speaker_embeddings(name, len(ids))
    scales = (1.5, 0.5, float(np.float32(1) / np.float32(1.2)), 2.0)
    ctls = [pc.controls(duration_scale=s) for s in scales]
    _, mel_lens, dur = run(eng, ids, 2 * PRED_CAP, None, spk, ctls)
    for b, r in enumerate(ac.predicted_oracle64(name)):
        want = pc.scaled(r["durations"], scales[b])
        if want.sum() == 0:
            want[:] = 1
        np.testing.assert_array_equal(dur[b, :len(want)], want, err_msg=f"{name} b={b}")
        assert int(mel_lens[b]) == int(want.sum())


# ------------------------------------------------------------------------------- the default model
@pytest.fixture(scope="module")
def model():
    m = GonovaTTS.from_pretrained(DEV, vocoder_dtype="f16", acoustic_dtype="f32")
    yield m
    m.engine.close()


def _tokens(ns, seed=11):
    rng = np.random.default_rng(seed)
    N = max(ns)
    tok = np.zeros((len(ns), N), np.int32)
    for b, n in enumerate(ns):
        tok[b, :n] = rng.integers(1, 78, size=n)
    return tok, np.asarray(ns, np.int32)


def _d0(model, tok, lens):
    _, _, dur = model.engine.acoustic(torch.from_numpy(tok).to(DEV), torch.from_numpy(lens), 12 * tok.shape[1],
                                      return_durations=True)
    return dur.cpu().numpy().astype(np.int64)


def test_budget_retry_scales_once(model):
    """speed 0.25 (scale 4) on sentences whose scaled need exceeds the first-pass budget: the exact
    second pass feeds the scaled durations back and must not scale them again."""
    tok, lens = _tokens((40, 25))
    d0 = _d0(model, tok, lens)
    want = np.asarray([pc.scaled(d0[b, :lens[b]], 4.0).sum() for b in range(2)])
    ctl = prosody_controls(speed=0.25)
    assert ctl["duration_scale"] == 4.0
    old = model.FRAMES_PER_TOKEN_CAP
    model.FRAMES_PER_TOKEN_CAP = 1
    try:
        assert want.max() > model._frame_budget(tok.shape[1], 4.0)   # the retry is taken
        _, wav_lens = model.synthesize_tokens(tok, lens, prosody=[ctl, ctl])
        chunks = list(model.stream_tokens(tok, lens, chunk_frames=64, prosody=[ctl, ctl]))
    finally:
        model.FRAMES_PER_TOKEN_CAP = old
    hop = model.vocoder_cfg.hop
    assert list(wav_lens) == list(hop * want)
    assert [int(sum(v[b] for _, _, v in chunks)) for b in range(2)] == list(hop * want)


@pytest.mark.parametrize("rate", (22050, 24000))
@pytest.mark.parametrize("given", (False, True))
def test_stream_concatenates_to_synthesize(model, rate, given):
    """stream_tokens with controls concatenates to synthesize_tokens with the same controls."""
    m = GonovaTTS(model.engine, model.acoustic_cfg, model.vocoder_cfg, sample_rate=rate)
    tok, lens = _tokens((21, 9, 14), seed=12)
    durs = None
    if given:
        durs = np.where(np.arange(tok.shape[1])[None, :] < lens[:, None], 5, 0).astype(np.int32)
        durs[1, 3] = 0
    ctls = [prosody_controls(speed=1 / 1.5, pitch=1.0), None, prosody_controls(speed=2.0, energy=-1.0, exaggeration=1.0)]
    wav, wav_lens = m.synthesize_tokens(tok, lens, durations=durs, prosody=ctls)
    plain, plain_lens = m.synthesize_tokens(tok, lens, durations=durs)
    wav = wav.cpu().numpy()
    assert wav_lens[0] > plain_lens[0] and wav_lens[1] == plain_lens[1] and wav_lens[2] < plain_lens[2]
    if given:   # rint(5 * 1.5) = 8 (7.5 ties to even), rint(5 * 0.5) = 2 (2.5 ties to even)
        hop = m.vocoder_cfg.hop
        if rate == 22050:
            assert list(wav_lens) == [21 * 8 * hop, 8 * 5 * hop, 14 * 2 * hop]
    assert np.array_equal(wav[1, :wav_lens[1]], plain.cpu().numpy()[1, :plain_lens[1]])
    pieces = [[] for _ in lens]
    for _, w, valid in m.stream_tokens(tok, lens, chunk_frames=32, durations=durs, output_rate=rate, prosody=ctls):
        w = w.cpu().numpy()
        for b in range(len(lens)):
            pieces[b].append(w[b, :int(valid[b])])
    for b in range(len(lens)):
        got = np.concatenate(pieces[b])
        assert got.shape == (int(wav_lens[b]),) and np.array_equal(got, wav[b, :int(wav_lens[b])]), (rate, given, b)


def test_range_guard_rerun_keeps_the_controls():
    """The existing guard test's weight scaling with controls on: the rerun on the fp32 encoder
    keeps them (the frame counts are the controlled forward's on that encoder)."""
    aw = make_acoustic_weights(seed=0)
    k = "encoder.conformer_layers.0.feed_forward_macaron.conv1.weight"
    aw2 = dict(aw)
    aw2[k] = aw[k] * 20000.0
    e = HipEngine(DEV, vocoder_dtype="f16", acoustic_dtype="bf16")
    e.load_weights(acoustic=aw2, vocoder=make_vocoder_weights(seed=0))
    try:
        tok, lens = _tokens((40, 23), seed=5)
        ctls = [prosody_controls(speed=0.5, pitch=1.0), prosody_controls(exaggeration=1.0)]
        m = GonovaTTS(e, AcousticConfig(), VocoderConfig())
        with pytest.warns(RuntimeWarning, match="f16 range"):
            wav, wav_lens = m.synthesize_tokens(tok, lens, prosody=ctls)
        assert m.range_fallbacks == 1 and np.isfinite(wav.cpu().numpy()).all()
        with e.encoder_f32():
            _, mel_lens, dur = e.acoustic(torch.from_numpy(tok).to(DEV), torch.from_numpy(lens), 24 * 40,
                                          return_durations=True, prosody=ctls)
            _, _, d0 = e.acoustic(torch.from_numpy(tok).to(DEV), torch.from_numpy(lens), 24 * 40, return_durations=True)
        assert list(wav_lens) == [int(x) * 256 for x in mel_lens.cpu().numpy()]
        d0 = d0.cpu().numpy()
        assert np.array_equal(dur.cpu().numpy()[0, :40], pc.scaled(d0[0, :40], 2.0))
        assert np.array_equal(dur.cpu().numpy()[1], d0[1])
    finally:
        e.close()


def test_engine_refuses_bad_controls(model):
    tok, lens = _tokens((5, 3))
    for bad in ([{"duration_scale": 0.0}, None], [{"pitch_shift": float("nan")}, None], [{"tempo": 1.0}, None],
                {"duration_scale": [1.0, 1.0, 1.0]}):
        with pytest.raises(ValueError):
            model.engine.acoustic(torch.from_numpy(tok).to(DEV), torch.from_numpy(lens), 64, prosody=bad)
    with pytest.raises(ValueError, match="speed"):
        model.generate("Hello.", speed=8.0)


def test_service_speed():
    """A `synthesize` with speed 2.0 returns exactly the samples a direct generate_batch with the
    same controls gives, and fewer than the neutral request."""
    from fastapi.testclient import TestClient
    from gonova_tts_amd.service.server import create_app
    from test_service_gpu import recv_until_complete
    holder = {}

    def factory():
        holder["m"] = GonovaTTS.from_pretrained(DEV, vocoder_dtype="f32", acoustic_dtype="f32")
        return holder["m"]

    text = "This is a test!"
    with TestClient(create_app(factory, max_wait=0.05, idle_wait=0.05)) as c:
        counts = {}
        for speed in (2.0, None):
            msg = {"type": "synthesize", "text": text, "voice_id": "default"}
            if speed:
                msg["speed"] = speed
            with c.websocket_connect("/v1/stream/tts") as ws:
                ws.send_text(json.dumps(msg))
                frames, final = recv_until_complete(ws)
            assert final["type"] == "synthesis_complete" and len(frames) == 1
            counts[speed] = frames[0]
        direct = holder["m"].generate_batch([text], prosody=[prosody_controls(speed=2.0)])[0]
        assert counts[2.0].shape == direct.shape and np.array_equal(counts[2.0], direct)
        assert 0 < counts[2.0].size < counts[None].size
        with c.websocket_connect("/v1/stream/tts") as ws:
            ws.send_text(json.dumps({"type": "synthesize", "text": text, "speed": 9}))
            assert ws.receive_json()["message"].startswith("Synthesis request refused: speed")
