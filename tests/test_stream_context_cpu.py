"""The streaming context is the generator's receptive field (no GPU).

config.vocoder_context_frames derives, in integer interval arithmetic, how many mel frames on each
side of a chunk the vocoder reads.  Here it is held to a table worked out by hand from the layer
definitions of oracle/vocoder.py, and to the float64 oracle itself: a window with that much context
reproduces the whole-utterance pass, and (where random weights reach the farthest tap) one frame
less on either side does not -- so the bound is tight and these tests can fail.  Then the pieces
that use it: GonovaTTS.stream_context, the refusal of a smaller explicit context, and the service's
floor on `stream_frames`.
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import vocoder_cases as vc
from gonova_tts_amd.config import AcousticConfig, VocoderConfig, vocoder_context_frames
from gonova_tts_amd.model import GonovaTTS
from oracle.vocoder import vocoder_forward

# frames of context per side: the row interval of one frame taken back through conv_post (+-3), each
# stage's MRF (+- max over resblocks of sum over pairs (k-1)/2 * (d+1)), each transposed conv
# ([ceil((a + p - (k-1)) / s), floor((b + p) / s)]) and conv_pre (+-3)
TABLE = {"V1": 13, "one": 35, "two": 50, "four": 61, "v3ish": 20, "taps41": 51, "taps32": 50, "nk1": 23,
         "odd": 50, "stream4": 20, "v3four": 44}
TIGHT = ("one", "nk1", "v3ish", "stream4")  # cases whose farthest taps weigh more than 1e-12 of the output

T_MEL, C0, N_CHUNK = 120, 58, 4  # a 120-frame mel and a 4-frame chunk in its middle
RTOL = 1e-12                     # x max|full pass|: float64 sums in another association order, no more


def cfg_of(name):
    return VocoderConfig() if name == "V1" else vc.CASES[name]


def test_table_covers_every_case():
    assert set(TABLE) == {"V1"} | set(vc.CASES)


@pytest.mark.parametrize("name", list(TABLE))
def test_context_frames_equal_the_table(name):
    left, right = vocoder_context_frames(cfg_of(name))
    assert (left, right) == (TABLE[name], TABLE[name])


_FULL = {}


def full_pass(name):
    """-> (mel [T_MEL, 80], float64 oracle waveform of all of it); once per case, read-only."""
    if name not in _FULL:
        mel = np.random.default_rng(7000 + list(vc.CASES).index(name)).standard_normal((T_MEL, 80)).astype(np.float32)
        wav = vocoder_forward(mel, vc.weights(name), vc.CASES[name], np.float64)
        wav.setflags(write=False)
        _FULL[name] = (mel, wav)
    return _FULL[name]


def window_error(name, left, right):
    """max |oracle on the window [C0 - left, C0 + N_CHUNK + right) - full pass| over the chunk's
    samples, relative to max |full pass|."""
    hop = vc.CASES[name].hop
    mel, full = full_pass(name)
    w0, w1 = max(0, C0 - left), min(T_MEL, C0 + N_CHUNK + right)
    win = vocoder_forward(mel[w0:w1], vc.weights(name), vc.CASES[name], np.float64)
    got = win[(C0 - w0) * hop:(C0 - w0 + N_CHUNK) * hop]
    want = full[C0 * hop:(C0 + N_CHUNK) * hop]
    assert got.shape == want.shape == (N_CHUNK * hop,)
    return float(np.abs(got - want).max() / np.abs(full).max())


@pytest.mark.parametrize("name", list(vc.CASES))
def test_oracle_window_with_the_context_equals_the_full_pass(name):
    left, right = vocoder_context_frames(vc.CASES[name])
    err = window_error(name, left, right)
    print(f"[window] {name}: context {left}/{right}, rel err {err:.3g}")
    assert err <= RTOL


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", TIGHT)
def test_one_frame_less_context_does_not(name, side):
    """The window reaches neither end of the mel here, so the missing frame is a real one."""
    left, right = vocoder_context_frames(vc.CASES[name])
    assert C0 - left > 0 and C0 + N_CHUNK + right < T_MEL
    err = window_error(name, left - (side == "left"), right - (side == "right"))
    print(f"[window] {name}: one frame less on the {side}, rel err {err:.3g}")
    assert err > RTOL


def model_for(name):
    """A GonovaTTS around no engine: any engine call fails (AttributeError)."""
    return GonovaTTS(SimpleNamespace(device_index=0), AcousticConfig(), cfg_of(name))


@pytest.mark.parametrize("name", list(TABLE))
def test_stream_context_is_the_receptive_field_but_16_for_v1(name):
    m = model_for(name)
    assert GonovaTTS.STREAM_CONTEXT == 16
    assert m.stream_context == (16 if name == "V1" else TABLE[name])
    assert m.stream_context >= max(vocoder_context_frames(m.vocoder_cfg))


@pytest.mark.parametrize("name", ["V1", "one", "v3ish"])
def test_explicit_context_below_the_receptive_field_raises(name):
    """Before any GPU work: the model's engine is a stub without a device, a stream or a forward."""
    m = model_for(name)
    need = TABLE[name]
    tokens, lens = np.ones((1, 4), np.int32), np.array([4])
    with pytest.raises(ValueError) as ei:
        next(m.stream_tokens(tokens, lens, context=need - 1))
    assert str(need - 1) in str(ei.value) and str(need) in str(ei.value)
    with pytest.raises(ValueError):
        next(m._stream_tokens(tokens, lens, 32, 0, None, None, None))
    assert m._context(need) == need and m._context(need + 40) == need + 40
    assert m._context(None) == m.stream_context


class _FakeStreamModel:
    """A sentence of n characters is 100 n samples, streamed in pieces of chunk_frames * 10."""
    sr = 22050

    def __init__(self, stream_context=None):
        self.stream_calls = []
        if stream_context is not None:
            self.stream_context = stream_context

    def generate_batch(self, texts):
        return [np.full(100 * len(t), len(t), np.float32) for t in texts]

    def stream_batch(self, texts, chunk_frames, speaker_embeddings=None):
        self.stream_calls.append((list(texts), chunk_frames))
        step = chunk_frames * 10
        full = self.generate_batch(texts)
        for c0 in range(0, max(len(a) for a in full), step):
            yield [(i, a[c0:c0 + step], c0 + step >= len(a)) for i, a in enumerate(full) if c0 < len(a)]


def _final(ws):
    while True:
        m = ws.receive()
        if m.get("text") is not None:
            return json.loads(m["text"])


@pytest.mark.parametrize("ctx, floor", [(None, 32), (16, 32), (35, 70), (61, 122)])
def test_service_floor_follows_the_models_stream_context(ctx, floor):
    """A request's stream_frames and the service's default both round up to twice the model's
    stream_context (a model without the attribute: the 32 of before); larger values pass."""
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from gonova_tts_amd.service.server import create_app
    model = _FakeStreamModel(ctx)
    text = "Hello world."
    with TestClient(create_app(lambda: model, stream_frames=40)) as c:
        assert c.app.state.service.stream_frames == max(40, floor)
        with c.websocket_connect("/v1/stream/tts") as ws:
            for frames in (None, 1, 200):
                msg = {"type": "synthesize", "text": text}
                if frames is not None:
                    msg["stream_frames"] = frames
                ws.send_text(json.dumps(msg))
                assert _final(ws)["type"] == "synthesis_complete"
    assert model.stream_calls == [([text], max(40, floor)), ([text], floor), ([text], 200)]
