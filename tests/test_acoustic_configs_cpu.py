"""The small non-default acoustic configurations (tests/acoustic_cases.py) on the CPU: the oracle
against transformers goldens, the lengths the GPU tests rely on, the rounding margins of the
predicted-duration batch, and the supported envelope restated in Python.  No GPU."""
import os

import numpy as np
import pytest

import acoustic_cases as ac
from gonova_tts_amd.weights import make_acoustic_weights
from oracle.acoustic import acoustic_forward

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_ac_cfg.npz"))
NAMES = list(ac.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_transformers_golden(name):
    """acoustic_forward in float32 and float64 against transformers' module built from the same
    configuration (tests/golden/make_ac_cfg_golden.py), at the tolerances the vocoder
    configurations' goldens are held to."""
    cfg, w, ids = ac.CASES[name].cfg, ac.weights(name), G[f"{name}_ids"]
    np.testing.assert_array_equal(ids, ac.golden_ids(name))
    spk = G[f"{name}_emb"] if cfg.speaker_embed_dim else None
    if spk is not None:
        np.testing.assert_array_equal(spk, ac.speaker_embeddings(name, 1)[0])
    o32 = acoustic_forward(ids, w, cfg, dtype=np.float32, speaker_embedding=spk)
    o64 = acoustic_forward(ids, w, cfg, dtype=np.float64, speaker_embedding=spk)
    for o in (o32, o64):
        np.testing.assert_array_equal(o["durations"], G[f"{name}_dur"])
    assert o32["mel"].shape == G[f"{name}_mel32"].shape == (int(G[f"{name}_dur"].sum()), 80)
    np.testing.assert_allclose(o32["mel"], G[f"{name}_mel32"], atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(o64["mel"], G[f"{name}_mel64"], atol=1e-12, rtol=1e-10)


def test_cases_cover_the_axes():
    """What the case comments claim, read back from the configurations."""
    c = {n: k.cfg for n, k in ac.CASES.items()}
    heads = {(v.hidden_size, v.num_attention_heads) for v in c.values()}
    assert (384, 2) not in heads   # the shape every other acoustic test loads
    assert {(128, 2), (256, 4), (192, 1), (512, 2)} <= heads
    assert {v.head_dim for v in c.values()} >= {48, 64, 96, 128, 192, 256}
    assert [n for n, v in c.items() if v.head_dim == 192] == list(ac.FUSED_ATTN)
    dw = {k for v in c.values() for k in (v.encoder_kernel_size, v.decoder_kernel_size)}
    assert {5, 9} <= dw and max(dw - {31}) >= 15 and (c["h48"].encoder_kernel_size, c["h48"].decoder_kernel_size) == (7, 31)
    assert {v.positionwise_conv_kernel_size for v in c.values()} >= {1, 3, 5}
    assert any(v.linear_units % 128 and v.linear_units % 64 == 0 for v in c.values())
    assert ac.CASES["h96"].dec_units != c["h96"].linear_units
    w = ac.weights("h96")
    assert w["encoder.conformer_layers.0.feed_forward.conv1.weight"].shape[0] == 640
    assert w["decoder.conformer_layers.0.feed_forward.conv1.weight"].shape == (320, 384, 3)
    # predictors: unequal widths, pitch wider than duration, equal below 256, one and three layers, kernel 1
    assert (c["h128"].duration_predictor_channels, c["h128"].pitch_predictor_channels, c["h128"].energy_predictor_channels) == (64, 128, 64)
    assert c["h64"].pitch_predictor_channels > c["h64"].duration_predictor_channels
    assert c["h64x4"].duration_predictor_channels == c["h64x4"].pitch_predictor_channels == c["h64x4"].energy_predictor_channels == 128
    layers = {n for v in c.values() for n in (v.duration_predictor_layers, v.pitch_predictor_layers, v.energy_predictor_layers)}
    assert {1, 3} <= layers
    assert any(v.duration_predictor_kernel_size == 1 for v in c.values())
    # postnet: wider than every predictor, one and two layers, kernel 3
    for n in ("h64", "h128", "h96"):
        assert c[n].postnet_units > max(c[n].duration_predictor_channels, c[n].pitch_predictor_channels, c[n].energy_predictor_channels)
    assert {1, 2} <= {v.postnet_layers for v in c.values()} and any(v.postnet_kernel == 3 for v in c.values())
    assert [n for n, v in c.items() if v.speaker_embed_dim] == ["h64x4"]
    for v in c.values():
        assert v.num_mel_bins == 80 and max(v.encoder_layers, v.decoder_layers) <= 2


def test_case_lengths_sit_on_the_tile_edges():
    assert len(ac.TOKENS) <= 8 and set(ac.TOKENS) >= {1, 2, 31, 32, 33, 64, 65}
    for name in NAMES:
        ids, durs = ac.ragged_inputs(name)
        assert [len(x) for x in ids] == list(ac.TOKENS) == [len(d) for d in durs]
        assert tuple(int(d.sum()) for d in durs) == ac.FRAMES
        assert all(set(np.unique(d)) <= {0, 3} for d in durs) and sum(int((d == 0).sum()) for d in durs) >= 3
        assert all(int(d.sum()) > 0 for d in durs)   # (no utterance falls under the all-zero rule)
        assert all(x.min() >= 1 and x.max() < ac.CASES[name].cfg.vocab_size for x in ids)
        assert tuple(r["mel"].shape[0] for r in ac.oracle64(name)) == ac.FRAMES
    f = sorted(ac.FRAMES)
    for edge in (32, 64, 128):   # utterances on both sides of an edge of every tile height
        assert any(x < edge for x in ac.TOKENS + ac.FRAMES) and any(x > edge for x in ac.TOKENS + ac.FRAMES)
    assert {31, 32, 33} <= set(ac.TOKENS) and {64, 65} <= set(ac.TOKENS)           # encoder rows
    assert {93, 96, 99} <= set(f) and 129 in f and max(x for x in f if x < 192) == 186 and 195 in f
    assert f[0] == 3 and f[-1] == 195 and ac.T_CAP % 32 == 0 and ac.T_CAP >= f[-1]
    assert 96 % 32 == 0   # the 32-token utterance run alone (t_cap = its frames): a full row stride, no pad row


@pytest.mark.parametrize("name", NAMES)
def test_predicted_batch_is_clear_of_rounding_boundaries(name):
    """Every token of the predicted-duration batch (and of the golden utterance) has its oracle
    exp(x) - 1 more than MARGIN from a .5 boundary in float32 and in float64, so the GPU tests
    compare durations exactly, with no carve-out."""
    ids = ac.predicted_inputs(name)
    assert [len(x) for x in ids] == list(ac.PRED_TOKENS)
    spk = ac.speaker_embeddings(name, len(ids))
    refs = ac.predicted_oracle64(name)
    for b, x in enumerate(ids + [ac.golden_ids(name)]):
        e = None if spk is None else spk[b if b < len(ids) else 0]
        d = []
        for dt in (np.float32, np.float64):
            logd = ac.log_durations(name, x, dt, e)
            m = float(ac.margin(logd).min())
            print(f"[margin] {name} b={b} {np.dtype(dt).name}: {m:.3e}")
            assert m > ac.MARGIN
            d.append(np.maximum(np.round(np.exp(logd) - 1), 0).astype(np.int64))
        np.testing.assert_array_equal(d[0], d[1])
        if b < len(ids):
            np.testing.assert_array_equal(d[0], refs[b]["durations"])
            assert refs[b]["mel"].shape[0] == int(d[0].sum()) <= 12 * max(ac.PRED_TOKENS)


# ---------------------------------------------------------------------------------------- envelope
def test_every_case_is_inside_the_envelope():
    for name in NAMES:
        assert ac.in_envelope(ac.weights(name)) is None, name
    assert ac.in_envelope(make_acoustic_weights(0)) is None   # the default configuration


@pytest.mark.parametrize("case", list(ac.OUTSIDE))
def test_outside_configurations_fail_the_python_predicate_on_the_named_tensor(case):
    make, tensor, _ = ac.OUTSIDE[case]
    assert ac.in_envelope(make()) == tensor
