"""Chunked resampler on the GPU (tts_resample_poly_chunk): a stream fed in chunks comes out as the
full-utterance pass (tts_resample_poly) bit for bit -- at the op, through
GonovaTTS.stream_tokens(output_rate=24000), through stream_batch and through the service's
`stream_frames` at 24 kHz (the rate the reference's clients assume, synthesizer.py:119)."""
import json

import numpy as np
import pytest
import scipy.signal as ss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gonova_tts_amd.engine import HipEngine, resample_chunk_counts, resample_history  # noqa: E402
from gonova_tts_amd.model import GonovaTTS  # noqa: E402

LENS = [700, 1, 0, 256, 519]


@pytest.fixture(scope="module")
def eng():
    return HipEngine("cuda:0", vocoder_dtype="f16")


@pytest.fixture(scope="module")
def ragged():
    """(x float32 [B, 700] with garbage past each length, the same on the device)"""
    rng = np.random.default_rng(11)
    x = np.zeros((len(LENS), max(LENS)), np.float32)
    for b, L in enumerate(LENS):
        x[b, :L] = 0.5 * rng.standard_normal(L)
        x[b, L:] = 7.0  # garbage past the length must not leak in
    return x, torch.from_numpy(x).cuda()


@pytest.mark.parametrize("in_count", [7, 37, 256])
@pytest.mark.parametrize("up,down", [(160, 147), (147, 160), (1, 2)])
def test_chunks_equal_full_pass_bit_for_bit(eng, ragged, up, down, in_count):
    """Ragged batch in chunks of in_count samples (7 at 1/2: shorter than the 42-sample history,
    which is then built over several chunks): outputs concatenate to eng.resample of the whole
    input bit for bit, out_lens are the host helper's counts, every chunk is zero past its count,
    and the result is within the full pass's 2e-6 of scipy.signal.resample_poly."""
    x, xd = ragged
    B, S = x.shape
    lens_d = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    full, full_lens = eng.resample(xd, lens_d, up, down)
    full, full_lens = full.cpu().numpy(), full_lens.cpu().numpy()
    n_hist, n_flush = resample_history(up, down)
    hist = torch.full((2, B, n_hist), 9.0, device="cuda")  # (chunk 0 must not read it)
    pieces = [[] for _ in range(B)]
    for k, start in enumerate(range(0, S, in_count)):
        cur = xd[:, start:start + in_count].contiguous()
        out, out_lens = eng.resample_chunk(cur, start, lens_d, up, down, hist[k % 2], hist[(k + 1) % 2])
        n = cur.shape[1]
        assert out.shape == (B, -(-n * up // down) + n_flush)
        out, out_lens = out.cpu().numpy(), out_lens.cpu().numpy()
        np.testing.assert_array_equal(out_lens, resample_chunk_counts(LENS, start, n, up, down))
        for b in range(B):
            assert np.all(out[b, out_lens[b]:] == 0)
            pieces[b].append(out[b, :out_lens[b]])
    for b, L in enumerate(LENS):
        got = np.concatenate(pieces[b])
        assert got.shape[0] == full_lens[b] == -(-L * up // down)
        np.testing.assert_array_equal(got, full[b, :full_lens[b]])
        if L:
            ref = ss.resample_poly(x[b, :L].astype(np.float64), up, down)
            err = float(np.abs(got - ref).max())
            print(f"{up}/{down} in_count {in_count} utterance {b}: max|err| vs scipy {err:.2e}")
            assert err <= 2e-6, (b, err)


def test_chunk_entry_refuses_bad_arguments(eng, ragged):
    _, xd = ragged
    B = xd.shape[0]
    lens_d = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    n_hist, n_flush = resample_history(160, 147)
    hist = torch.zeros((2, B, n_hist), device="cuda")
    cur = xd[:, :64].contiguous()
    with pytest.raises(RuntimeError, match="out_cap"):
        eng.resample_chunk(cur, 0, lens_d, 160, 147, hist[0], hist[1],
                           out=torch.empty((B, 70 + n_flush - 1), device="cuda"))  # ceil(64*160/147) = 70
    with pytest.raises(RuntimeError, match="non-negative"):
        eng.resample_chunk(cur, -1, lens_d, 160, 147, hist[0], hist[1])
    with pytest.raises(RuntimeError, match="must not be d_hist_in"):
        eng.resample_chunk(cur, 64, lens_d, 160, 147, hist[0], hist[0])
    with pytest.raises(RuntimeError, match="must be positive"):
        eng.resample_chunk(cur, 0, lens_d, 0, 147, hist[0], hist[1])


# ------------------------------------------------------------------ model
def _stream_pieces(m, tok, lens, chunk_frames, **kw):
    pieces = [[] for _ in range(len(lens))]
    for c0, wav, valid in m.stream_tokens(tok, lens, chunk_frames=chunk_frames, output_rate=24000, **kw):
        w = wav.cpu().numpy()
        assert w.shape[1] >= int(valid.max())
        for b in range(len(lens)):
            pieces[b].append(w[b, :valid[b]])
    return [np.concatenate(p) for p in pieces]


@pytest.fixture(scope="module")
def given():
    """A 24 kHz model on the seeded weights, a batch with given durations (token lengths 9, 1, 5, 8,
    durations 1-3; the last utterance has 8 x 2 = 16 frames, a whole number of 1- and 4-frame
    chunks) and its full-pass output at 24 kHz."""
    m = GonovaTTS.from_pretrained("cuda:0", sample_rate=24000)
    rng = np.random.default_rng(4)
    lens = np.array([9, 1, 5, 8], np.int32)
    tok = np.zeros((4, 9), np.int32)
    dur = np.zeros((4, 9), np.int32)
    for i, L in enumerate(lens):
        tok[i, :L] = rng.integers(1, 78, size=L)
        dur[i, :L] = rng.integers(1, 4, size=L)
    dur[3, :8] = 2
    full, full_lens = m.synthesize_tokens(tok, lens, durations=dur)
    return m, tok, lens, dur, full.cpu().numpy(), np.asarray(full_lens)


@pytest.mark.parametrize("chunk_frames", [1, 4, 32])
def test_stream_tokens_at_24khz_equals_full_pass(given, chunk_frames):
    """stream_tokens(output_rate=24000) pieces == synthesize_tokens' 24 kHz output, bit for bit
    (chunks of 1 and 4 frames: many chunks, one utterance ending exactly at a chunk edge; 32: every
    utterance ends inside the first chunk, which then also carries the flush)."""
    m, tok, lens, dur, full, full_lens = given
    frames = dur.sum(axis=1)
    assert frames[3] == 16 and np.all(full_lens == -(-frames * 256 * 160 // 147))
    got = _stream_pieces(m, tok, lens, chunk_frames, durations=dur)
    for b in range(len(lens)):
        assert got[b].shape[0] == full_lens[b]
        np.testing.assert_array_equal(got[b], full[b, :full_lens[b]])
    # output_rate=None stays native whatever the model's rate is
    c0, wav, valid = next(iter(m.stream_tokens(tok, lens, chunk_frames=chunk_frames, durations=dur)))
    assert wav.shape[1] == min(chunk_frames, int(frames.max())) * 256
    np.testing.assert_array_equal(valid, np.clip(frames, 0, chunk_frames) * 256)


def test_stream_tokens_at_24khz_utterance_ends_at_a_32_frame_edge(given):
    """Chunks of 32 frames with an utterance of exactly 32 frames (8 tokens x 4) next to one of 45
    (9 x 5): the stream goes on past the edge the short one ends at, and its flush comes with the
    first chunk."""
    m, tok, lens, dur, _, _ = given
    dur = dur.copy()
    dur[0, :9], dur[3, :8] = 5, 4
    full, full_lens = m.synthesize_tokens(tok, lens, durations=dur)
    full = full.cpu().numpy()
    got = _stream_pieces(m, tok, lens, 32, durations=dur)
    assert full_lens[3] == -(-32 * 256 * 160 // 147) and full_lens[0] == -(-45 * 256 * 160 // 147)
    for b in range(len(lens)):
        assert got[b].shape[0] == full_lens[b]
        np.testing.assert_array_equal(got[b], full[b, :full_lens[b]])


@pytest.mark.parametrize("lens", [[5, 3, 7], [10, 3, 8]])
def test_stream_tokens_at_24khz_predicted_durations(lens):
    """Predicted durations (6 frames per token): the first chunk and its resample are enqueued
    ahead of the host read of the frame counts.  18-42 frames: the longest utterance does not cover
    that chunk's 48-frame window, so both are discarded and computed again; 18-60 frames: they are
    used, and the second chunk reads the history the early one wrote.  Either way the pieces equal
    the full pass."""
    m = GonovaTTS.from_pretrained("cuda:0", fixed_duration=6, sample_rate=24000)
    rng = np.random.default_rng(3)
    lens = np.array(lens, np.int32)
    tok = np.zeros((3, int(lens.max())), np.int32)
    for i, L in enumerate(lens):
        tok[i, :L] = rng.integers(1, 78, size=L)
    full, full_lens = m.synthesize_tokens(tok, lens)
    full = full.cpu().numpy()
    got = _stream_pieces(m, tok, lens, 32)
    for b in range(3):
        assert got[b].shape[0] == full_lens[b] == -(-6 * 256 * int(lens[b]) * 160 // 147)
        np.testing.assert_array_equal(got[b], full[b, :full_lens[b]])


# ------------------------------------------------------------------ stream_batch and the service
TEXTS = ["Good morning to everyone in the room.", "The quick brown fox jumps over the lazy dog!"]


def _split_at(frames, lengths):
    """Consecutive frames grouped so that group k adds up to lengths[k] exactly."""
    groups, it = [], iter(frames)
    for n in lengths:
        g, got = [], 0
        while got < n:
            g.append(next(it))
            got += len(g[-1])
        assert got == n
        groups.append(g)
    assert next(it, None) is None
    return groups


def test_stream_batch_and_service_at_24khz_equal_generate_batch():
    """Two short texts at 24 kHz: stream_batch's pieces, and the frames of a service with
    stream_frames=32, concatenate per sentence to generate_batch's audio at 24 kHz bit for bit,
    in more than one piece per sentence."""
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from gonova_tts_amd.service.server import create_app
    holder = {}

    def factory():
        holder["m"] = GonovaTTS.from_pretrained("cuda:0", sample_rate=24000)
        return holder["m"]

    app = create_app(factory, stream_frames=32)
    with TestClient(app) as c:
        m = holder["m"]
        assert m.sr == 24000 and m.streams_resampled and app.state.service.can_stream()
        direct = m.generate_batch(TEXTS)
        pieces = [[] for _ in TEXTS]
        finished = [0] * len(TEXTS)
        for out in m.stream_batch(TEXTS, chunk_frames=32):
            for i, a, fin in out:
                assert not finished[i]
                pieces[i].append(a)
                finished[i] += bool(fin)
        assert finished == [1, 1]
        for p, d in zip(pieces, direct):
            assert sum(len(a) > 0 for a in p) > 1
            np.testing.assert_array_equal(np.concatenate(p), d)
        with c.websocket_connect("/v1/stream/tts") as ws:
            ws.send_text(json.dumps({"type": "synthesize", "text": " ".join(TEXTS)}))
            frames = []
            while True:
                msg = ws.receive()
                if msg.get("bytes") is not None:
                    frames.append(np.frombuffer(msg["bytes"], np.float32))
                elif msg.get("text") is not None:
                    final = json.loads(msg["text"])
                    break
        assert final == {"type": "synthesis_complete", "chunk_id": len(frames)}
        for g, d in zip(_split_at(frames, [len(d) for d in direct]), direct):
            assert len(g) > 1
            np.testing.assert_array_equal(np.concatenate(g), d)
        assert c.get("/health").json()["sample_rate"] == 24000
