"""The stage 2-3 upsamplers fused into the preceding stage's last pair launch (TTS_UP_FUSE,
mrf_pair_kernel's UP form) against the two-launch path: the same arithmetic in the same order,
so the waveforms are compared bit for bit.  The profiler's per-kind launch counts show which
path a run took, so a comparison cannot pass without running the fused kernel.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gonova_tts_amd.engine import HipEngine  # noqa: E402
from gonova_tts_amd.weights import make_vocoder_weights  # noqa: E402

DEV = "cuda:0"
HOP = 256

# Fused tile heights (mrf_pair.hip: the full-height k = 11 tiles less the upsampler's extra row):
# 127 rows at stage 1 (64 rows per frame), 277 rows at stage 2 (128 rows per frame).  The smallest
# frame counts whose row count is a whole number of fused tiles are 127 and 277 (64 and 127, 128
# and 277 are coprime): there the upsampler's last input row u = len is the first row of a tile
# that holds no other row of the utterance.
TILE_LENS = [126, 127, 128, 276, 277, 278]

CASES = {
    # 6 x 36 = 216 full-height blocks at stages 1 and 2 (short tiles start under 128)
    "ragged": (71, [71, 1, 2, 0, 33, 64]),
    "tile_multiples": (278, TILE_LENS),
    # len == T == a whole number of stage-1 tiles: the tile of row u = len exists only because the
    # fused grid covers rows 0 .. T (2 x 64 = 128 full-height blocks)
    "full_length": (127, [127, 126]),
}


@pytest.fixture(scope="module")
def vw():
    return make_vocoder_weights(seed=0)


_ENG = {}


def engine_for(dtype, vw):
    if dtype not in _ENG:
        e = HipEngine(DEV, vocoder_dtype=dtype)
        e.load_weights(vocoder=vw)
        _ENG[dtype] = e
    return _ENG[dtype]


def run(eng, mel, ln):
    """-> (waveforms, upsample_stream_kernel launches, mrf_pair_kernel launches) of one pass"""
    eng.profile(True)
    try:
        eng.profile_read_kinds()
        wav = eng.vocoder(mel, ln).cpu().numpy()
        kinds = eng.profile_read_kinds()
    finally:
        eng.profile(False)
    return wav, kinds["upsample_stream_kernel"][2], kinds["mrf_pair_kernel"][2]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fused_upsamplers_bit_identical(vw, dtype, case, switch):
    T, lens = CASES[case]
    eng = engine_for(dtype, vw)
    rng = np.random.default_rng(1234 + T)
    mel = torch.from_numpy(rng.standard_normal((len(lens), T, 80)).astype(np.float32)).to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32)
    switch("TTS_UP_FUSE", 1)
    fused, n_up_f, n_pair_f = run(eng, mel, ln)
    switch("TTS_UP_FUSE", 0)
    sep, n_up_s, n_pair_s = run(eng, mel, ln)
    assert n_up_f == 0, f"fused run still launched {n_up_f} upsample_stream_kernel"
    assert n_up_s == 2, f"unfused run launched {n_up_s} upsample_stream_kernel, expected 2"
    assert n_pair_f == n_pair_s
    assert np.isfinite(sep).all()
    for b, L in enumerate(lens):
        assert np.array_equal(fused[b], sep[b]), (b, L, float(np.abs(fused[b] - sep[b]).max()))
        assert np.all(fused[b, L * HOP:] == 0), (b, L)
        if L:
            assert np.abs(fused[b, :L * HOP]).max() > 0, (b, L)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_small_grid_keeps_the_upsample_launches(vw, dtype, switch):
    """batch 1 x 16 frames runs short pair tiles: nothing is fused under either setting"""
    eng = engine_for(dtype, vw)
    rng = np.random.default_rng(99)
    mel = torch.from_numpy(rng.standard_normal((1, 16, 80)).astype(np.float32)).to(DEV)
    ln = torch.tensor([16], dtype=torch.int32)
    switch("TTS_UP_FUSE", 1)
    on, n_up_on, _ = run(eng, mel, ln)
    switch("TTS_UP_FUSE", 0)
    off, n_up_off, _ = run(eng, mel, ln)
    assert n_up_on == 2 and n_up_off == 2, (n_up_on, n_up_off)
    assert np.array_equal(on, off)
    assert np.abs(on).max() > 0
