"""The service's prosody controls with a fake engine: refusal shapes, the `prosody` keyword only
for non-neutral batches, one list entry per sentence, and requests with different controls sharing
an engine batch."""
import json
import threading

import numpy as np
import pytest

pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from gonova_tts_amd.prosody import prosody_controls  # noqa: E402
from gonova_tts_amd.service.queues import SynthesisRequest  # noqa: E402
from gonova_tts_amd.service.server import create_app  # noqa: E402
from test_service_cpu import FakeModel, recv_until_complete  # noqa: E402


class ProsodyModel(FakeModel):
    """Records every call's keywords; a sentence's audio length follows its duration_scale."""

    def __init__(self, delay=0.0):
        super().__init__(delay=delay)
        self.calls = []

    def generate_batch(self, texts, **kw):
        with self.lock:
            self.calls.append((list(texts), kw))
        out = FakeModel.generate_batch(self, texts)
        pros = kw.get("prosody") or [None] * len(texts)
        return [a[:int(len(a) * (p or {}).get("duration_scale", 1.0))] for a, p in zip(out, pros)]


def test_neutral_requests_pass_no_prosody_keyword():
    """A model whose generate_batch takes no keywords (every fake engine before this feature) keeps
    working, exaggeration 0.5 included; the recording model sees no `prosody` key."""
    for model in (FakeModel(), ProsodyModel()):
        with TestClient(create_app(lambda: model)) as c:
            with c.websocket_connect("/v1/stream/tts") as ws:
                ws.send_text(json.dumps({"type": "synthesize", "text": "Hello world. Again.", "exaggeration": 0.5,
                                         "speed": 1.0, "pitch": 0, "energy": 0.0}))
                frames, final = recv_until_complete(ws)
        assert final == {"type": "synthesis_complete", "chunk_id": 2} and len(frames) == 2
    assert model.calls and all("prosody" not in kw for _, kw in model.calls)


def test_controls_reach_the_model_per_sentence():
    model = ProsodyModel()
    with TestClient(create_app(lambda: model)) as c:
        with c.websocket_connect("/v1/stream/tts") as ws:
            ws.send_text(json.dumps({"type": "synthesize", "text": "Hello world. Again.", "speed": 2.0, "pitch": 1,
                                     "energy": -0.5, "exaggeration": 1.0}))
            frames, final = recv_until_complete(ws)
    assert final["chunk_id"] == 2
    assert [len(f) for f in frames] == [600, 300]     # 100 samples per character, halved
    want = prosody_controls(speed=2.0, pitch=1, energy=-0.5, exaggeration=1.0)
    assert want == dict(duration_scale=0.5, pitch_shift=1.0, pitch_range=2.0, energy_shift=-0.5, energy_range=2.0)
    got = [kw["prosody"] for texts, kw in model.calls if "prosody" in kw]
    assert got and all(len(p) == len(t) for (t, kw), p in zip([c_ for c_ in model.calls if "prosody" in c_[1]], got))
    assert all(entry == want for p in got for entry in p)


def test_requests_with_different_controls_share_a_batch():
    """_take does not group by controls: a neutral request and two controlled ones land in one
    engine batch, whose prosody list has None for the neutral sentences."""
    model = ProsodyModel(delay=0.05)
    msgs = [dict(speed=2.0), dict(pitch=-1.0), dict()]
    results = {}
    with TestClient(create_app(lambda: model, max_wait=0.3, idle_wait=0.3)) as c:
        def client(i):
            with c.websocket_connect("/v1/stream/tts") as ws:
                ws.send_text(json.dumps({"type": "synthesize", "text": f"Sentence number {i} here.", **msgs[i]}))
                results[i] = recv_until_complete(ws)
        ts = [threading.Thread(target=client, args=(i,)) for i in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=30)
    assert len(results) == 3
    mixed = [(texts, kw) for texts, kw in model.calls if len(texts) == 3]
    assert mixed, [t for t, _ in model.calls]
    texts, kw = mixed[0]
    by_text = dict(zip(texts, kw["prosody"]))
    assert by_text["Sentence number 0 here."] == prosody_controls(speed=2.0)
    assert by_text["Sentence number 1 here."] == prosody_controls(pitch=-1.0)
    assert by_text["Sentence number 2 here."] is None
    assert len(results[0][0][0]) * 2 == len(results[2][0][0])


@pytest.mark.parametrize("field,value,word", [
    ("speed", "fast", "speed must be a number"), ("speed", 0.1, "speed 0.1 outside"), ("speed", 5, "speed 5.0 outside"),
    ("speed", None, "speed must be a number"), ("pitch", 4.5, "pitch 4.5 outside"), ("energy", -5, "energy -5.0 outside"),
    ("pitch", True, "pitch must be a number"), ("exaggeration", "lots", "exaggeration must be a number"),
    ("energy", [1], "energy must be a number"),
])
def test_bad_controls_are_refused_before_queueing(field, value, word):
    model = ProsodyModel()
    with TestClient(create_app(lambda: model)) as c:
        n0 = len(model.calls)
        with c.websocket_connect("/v1/stream/tts") as ws:
            ws.send_text(json.dumps({"type": "synthesize", "text": "Hello.", field: value}))
            m = ws.receive_json()
            assert m["type"] == "error" and m["message"].startswith("Synthesis request refused: "), m
            assert word in m["message"], m
            # the connection lives on and a good request still goes through
            ws.send_text(json.dumps({"type": "synthesize", "text": "Hello."}))
            frames, final = recv_until_complete(ws)
            assert len(frames) == 1 and final["type"] == "synthesis_complete"
        assert c.get("/metrics").json()["requests_received"] == 1
        assert len(model.calls) == n0 + 1


def test_non_finite_controls_are_refused():
    """json.loads takes NaN and Infinity; they are refused like any other bad value."""
    with TestClient(create_app(lambda: ProsodyModel())) as c:
        with c.websocket_connect("/v1/stream/tts") as ws:
            for raw in ('{"type":"synthesize","text":"Hi.","pitch":NaN}', '{"type":"synthesize","text":"Hi.","exaggeration":Infinity}'):
                ws.send_text(raw)
                m = ws.receive_json()
                assert m["message"].startswith("Synthesis request refused: ") and "finite" in m["message"], m


def test_request_fields_default_to_neutral():
    r = SynthesisRequest("c", "t", "default", 0.0)
    assert (r.speed, r.pitch, r.energy, r.exaggeration) == (1.0, 0.0, 0.0, 0.5)
    assert prosody_controls(r.speed, r.pitch, r.energy, r.exaggeration) is None
    assert np.float32(prosody_controls(speed=1.2)["duration_scale"]) == np.float32(1) / np.float32(1.2)
