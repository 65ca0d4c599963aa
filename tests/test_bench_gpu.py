"""bench.py's plain run on the GPU, in process on a tiny shape: it measures the headline alone
(nothing that `--full` adds), `--steps` is the number of timed steps, and `--dump-outputs` writes
the last timed step's waveform -- the same bits from run to run, equal to a direct engine call on
the same seeded inputs."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

B, T = 3, 37  # ragged against every tile: odd batch, frames no multiple of a tile


def _bench(monkeypatch, capsys, extra):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--batch", str(B), "--frames", str(T)] + extra)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_alone_and_dumps_its_waveform(monkeypatch, capsys, tmp_path):
    import torch
    import bench
    from gonova_tts_amd.engine import HipEngine
    from gonova_tts_amd.weights import make_vocoder_weights
    calls = []
    real_timed = bench.Ctx.timed

    def timed(self, step, steps, warmup, eng=None):
        calls.append((steps, warmup))
        return real_timed(self, step, steps, warmup, eng)

    monkeypatch.setattr(bench.Ctx, "timed", timed)
    d1, d2 = tmp_path / "a", tmp_path / "b"
    out = _bench(monkeypatch, capsys, ["--steps", "3", "--warmup", "1", "--dump-outputs", str(d1)])
    assert calls == [(3, 1)]  # one timed loop, of --steps steps after --warmup warmups
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "f16" and out["higher_is_better"] is True
    assert out["unit"] == "samples/s" and out["ms_per_step"] > 0
    # value and ms_per_step state the same measurement: samples of the timed steps / their time
    # (ms_per_step is printed to 1 us: half a unit of its last digit either way)
    assert out["value"] == pytest.approx(B * T * 256 / (out["ms_per_step"] * 1e-3),
                                         rel=0.0005 / out["ms_per_step"] + 1e-6)
    for k in ("full_pipeline", "c4", "streaming", "c1", "cpu_baseline"):
        assert k not in out, k
    assert sorted(os.listdir(d1)) == ["wav.npy"]
    w1 = np.load(d1 / "wav.npy")
    assert w1.dtype == np.float32 and w1.shape == (B, T * 256) and np.isfinite(w1).all() and np.abs(w1).max() > 0
    # the same arguments again (another step count): the same inputs, the same waveform
    _bench(monkeypatch, capsys, ["--steps", "1", "--warmup", "0", "--dump-outputs", str(d2)])
    assert np.array_equal(w1, np.load(d2 / "wav.npy"))
    # what a caller of the timed path receives for the bench's seeded inputs
    eng = HipEngine(0, vocoder_dtype="f16", max_batch=B, max_frames=T)
    eng.load_weights(vocoder=make_vocoder_weights(seed=0))
    mel = torch.randn((B, T, 80), generator=torch.Generator(device="cpu").manual_seed(1000)).cuda()
    ref = eng.vocoder(mel).cpu().numpy()
    eng.close()
    assert np.array_equal(w1, ref)
