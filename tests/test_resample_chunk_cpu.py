"""Chunked resampler, host side (no GPU): the per-chunk output counts tts_resample_poly_chunk
emits (engine.resample_chunk_counts, the kernel's integer arithmetic on the host), the history /
flush sizes tts_resample_history reports, and the service accepting `stream_frames` from a
resampling model that declares `streams_resampled`."""
import json
import threading
from math import gcd

import numpy as np
import pytest

from gonova_tts_amd.engine import resample_chunk_counts, resample_history
from oracle.resample import design

RATIOS = [(160, 147), (147, 160), (2, 1), (1, 2), (3, 2), (1, 8), (8, 1)]
CHUNKS = [1, 3, 37, 256, 8192]
N_IN = list(range(60)) + [255, 256, 257, 2205, 8191, 8192, 8193]


@pytest.mark.parametrize("up,down", RATIOS)
def test_history_entry_matches_oracle_design(up, down):
    """tts_resample_history == (taps per output - 1, n_pre_remove) of the oracle's filter design,
    for the reduced ratio and for an unreduced one."""
    h, npr = design(up, down)
    nq = -(-len(h) // up)
    assert resample_history(up, down) == (nq - 1, npr)
    assert resample_history(up * 150, down * 150) == (nq - 1, npr)
    if (up, down) == (160, 147):
        assert (nq - 1, npr) == (20, 11)


def test_history_entry_refuses_bad_rates():
    with pytest.raises(RuntimeError, match="must be positive"):
        resample_history(0, 1)
    with pytest.raises(RuntimeError, match="must be positive"):
        resample_history(3, -2)


@pytest.mark.parametrize("up,down", RATIOS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunk_counts_telescope_stay_in_bound_and_need_no_later_input(up, down, chunk):
    """For every utterance length: the chunks' counts add up to ceil(n_in*up/down) (also when the
    stream runs on past a short utterance's end, as in a ragged batch); no chunk emits more than
    ceil(chunk*up/down) + n_flush; and the newest input an emitted output reads,
    x[(m + n_pre_remove) * down // up], lies before the chunk's end unless the utterance has ended
    (its samples are then all there, and inputs at or past n_in are skipped by the sum)."""
    n_hist, npr = resample_history(up, down)
    n_in = np.asarray(N_IN, np.int64)
    n_out = -(-n_in * up // down)
    cap = -(-chunk * up // down) + npr
    total = np.zeros_like(n_in)
    end = int(n_in.max()) + chunk  # one chunk past the longest utterance
    for start in range(0, end, chunk):
        c = resample_chunk_counts(n_in, start, chunk, up, down)
        assert c.dtype == np.int64 and c.shape == n_in.shape
        assert np.all(c >= 0) and np.all(c <= cap)
        total += c
        live = (start + chunk < n_in) & (total > 0)  # not ended: the last emitted output is total - 1
        newest = (total[live] - 1 + npr) * down // up
        assert np.all(newest < start + chunk)
        # ... and the oldest input of the chunk's first output is within the history
        first = c > 0
        oldest = (total[first] - c[first] + npr) * down // up - n_hist
        assert np.all(oldest >= start - n_hist)
    np.testing.assert_array_equal(total, n_out)


def test_chunk_counts_reduce_the_ratio():
    a = resample_chunk_counts([700, 1, 0, 256], 37, 64, 24000, 22050)
    b = resample_chunk_counts([700, 1, 0, 256], 37, 64, 160, 147)
    np.testing.assert_array_equal(a, b)
    assert gcd(24000, 22050) == 150


# ------------------------------------------------------------------ service
class ResampledStreamModel:
    """CPU fake of a model that streams at a resampled rate: a sentence of n characters is 100 n
    samples of value n; stream_batch cuts it into pieces of unequal length (chunk_frames * 10,
    alternately + 3 and - 3 samples, as a resampler's chunks differ)."""
    sr, native_sr = 24000, 22050
    streams_resampled = True

    def __init__(self):
        self.lock = threading.Lock()
        self.stream_calls = []

    def generate_batch(self, texts):
        return [np.full(100 * len(t), len(t), np.float32) for t in texts]

    def stream_batch(self, texts, chunk_frames, speaker_embeddings=None):
        with self.lock:
            self.stream_calls.append((list(texts), chunk_frames))
        full = self.generate_batch(texts)
        pos = [0] * len(full)
        k = 0
        while any(p < len(a) for p, a in zip(pos, full)):
            step = chunk_frames * 10 + (3 if k % 2 == 0 else -3)
            out = []
            for i, a in enumerate(full):
                if pos[i] < len(a):
                    out.append((i, a[pos[i]:pos[i] + step], pos[i] + step >= len(a)))
                    pos[i] += step
            k += 1
            yield out


def recv_until_complete(ws):
    frames = []
    while True:
        m = ws.receive()
        if m.get("bytes") is not None:
            frames.append(np.frombuffer(m["bytes"], np.float32))
        elif m.get("text") is not None:
            return frames, json.loads(m["text"])


def test_service_streams_frames_from_a_model_that_streams_resampled():
    """A model with sr != native_sr that declares streams_resampled: stream_frames is accepted (per
    request and as the service default), the pieces arrive in sentence order and concatenate to the
    per-sentence audio, and audio_seconds is counted at the model's 24,000 Hz."""
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from gonova_tts_amd.service.server import create_app
    model = ResampledStreamModel()
    app = create_app(lambda: model, stream_frames=40)
    text = "Hello world. This is a test! Is it working? yes it is."
    with TestClient(app) as c:
        assert app.state.service.can_stream()
        assert c.get("/health").json()["sample_rate"] == 24000
        before = app.state.service.batcher.stats["audio_seconds"]
        with c.websocket_connect("/v1/stream/tts") as ws:
            ws.send_text(json.dumps({"type": "synthesize", "text": text, "stream_frames": 64}))
            frames, final = recv_until_complete(ws)
        assert final == {"type": "synthesis_complete", "chunk_id": len(frames)}
        # sentence by sentence (12, 15, 25 characters), each in pieces of 643, 637, ... samples
        assert [len(f) for f in frames] == [643, 557] + [643, 637, 220] + [643, 637, 643, 577]
        want = np.concatenate([np.full(100 * n, n, np.float32) for n in (12, 15, 25)])
        np.testing.assert_array_equal(np.concatenate(frames), want)
        stats = app.state.service.batcher.stats
        assert abs(stats["audio_seconds"] - before - len(want) / 24000) < 1e-9
        with c.websocket_connect("/v1/stream/tts") as ws:  # the service default applies too
            ws.send_text(json.dumps({"type": "synthesize", "text": "Hello world."}))
            frames, final = recv_until_complete(ws)
        assert [len(f) for f in frames] == [403, 397, 400] and final["chunk_id"] == 3
    assert model.stream_calls == [(["Hello world.", "This is a test!", "Is it working? yes it is."], 64),
                                  (["Hello world."], 40)]
