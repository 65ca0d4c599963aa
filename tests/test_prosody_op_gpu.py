"""variance_adapt_ctl_kernel at op level (tts_op_variance_adapt) on the cases of prosody_cases.py:
durations, frame counts and the frame -> token map per utterance scale against durations_expected,
the controlled pitch / energy against the float64 formula within the fp32 bound, neutral and masked
values bit for bit, x against the existing var_embed_add op on what the kernel wrote, every
utterance alone against itself in the batch, and the refusals.  test_prosody_cpu.py shows what the
bounds reject."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import prosody_cases as pc  # noqa: E402
import rowwise_cases as rc  # noqa: E402
from gonova_tts_amd import engine as eng  # noqa: E402
from test_rowwise_op_gpu import DEV, TORCH, dev, host, ints, log, run  # noqa: E402


def f32dev(a):
    """float32 array -> device, NaN / inf kept"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def bits(t):
    """device tensor -> its bits as a host integer array"""
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def launch(N, D, dt, tcap, sel, override, ctls, null_ctl=False):
    """One launch on the utterances sel -> dict of device outputs (x, p, e in place)."""
    i = pc.op_inputs(N, D, dt)
    Np, B = pc.op_np(N), len(sel)
    x = dev(i["x"][sel], dt)
    p, e = f32dev(i["p"][sel]), f32dev(i["e"][sel])
    d, m, t = (torch.full(s, -7, dtype=torch.int32, device=DEV) for s in ((B, N), (B,), (B, tcap)))
    blk = None if null_ctl else f32dev(pc.block([ctls[b] for b in sel]))
    run(eng.variance_adapt_op, dt, x, None if override else f32dev(i["logd"][sel]), p, e,
        ints([i["lens"][b] for b in sel]), B, N, Np, D, dev(i["we"]), dev(i["be"]), dev(i["wp"]), dev(i["bp"]), tcap,
        d, m, t, override_d=ints(i["ovr"][sel]) if override else None, ctl=blk)
    return dict(x=x, p=p, e=e, dur=d, mel_lens=m, tokmap=t)


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("D", pc.OP_D)
@pytest.mark.parametrize("N", rc.DUR_N)
def test_variance_adapt(N, D, dt):
    i = pc.op_inputs(N, D, dt)
    lens, ctls, Np = i["lens"], pc.op_controls(), pc.op_np(N)
    B = len(lens)
    everyone = list(range(B))
    worst = []
    for tcap in pc.op_tcaps(N):
        for override in (False, True):
            got = launch(N, D, dt, tcap, everyone, override, ctls)
            # durations per utterance scale
            want = pc.op_durations_expected(i["logd"], i["ovr"] if override else None, lens, N, tcap, ctls)
            for name, w in zip(("dur", "mel_lens", "tokmap"), want):
                g = host(got[name])
                assert np.array_equal(g, w), (N, D, dt, tcap, override, name, np.argwhere(g != w)[:4])
            # pitch and energy: the formula within the fp32 bound; neutral and masked bit for bit
            for what, key in (("pitch", "p"), ("energy", "e")):
                ref, bnd = pc.op_adapt_expected(i[key], lens, ctls, what)
                g = host(got[key]).astype(np.float64)
                gb, ib = bits(got[key]), i[key].view(np.int32)
                for b, L in enumerate(lens):
                    assert np.array_equal(gb[b, L:], ib[b, L:]), (N, dt, what, b, "tokens past the length were written")
                    if pc.is_neutral(ctls[b], what):
                        assert np.array_equal(gb[b, :L], ib[b, :L]), (N, dt, what, b, "a neutral utterance changed")
                    elif L:
                        err = np.abs(g[b, :L] - ref[b, :L])
                        print(f"[prosody op] N={N} {what} b={b}: worst {float((err / bnd[b, :L]).max()):.3f} of the bound")
                        assert (err <= bnd[b, :L]).all(), (N, dt, what, b, float((err / bnd[b, :L]).max()))
                        worst.append(float((err / bnd[b, :L]).max()))
            # x: the existing op's chain on the p' / e' the kernel wrote, valid rows; the rest untouched
            x0 = dev(i["x"], dt)
            x2 = x0.clone()
            pw = torch.nan_to_num(got["p"], nan=0.0, posinf=0.0, neginf=0.0)
            ew = torch.nan_to_num(got["e"], nan=0.0, posinf=0.0, neginf=0.0)
            run(eng.var_embed_add_op, dt, x2, B * Np, D, ew, dev(i["we"]), dev(i["be"]), pw, dev(i["wp"]), dev(i["bp"]))
            gx, wx, ox = bits(got["x"]), bits(x2), bits(x0)
            for b, L in enumerate(lens):
                assert np.array_equal(gx[b, :L], wx[b, :L]), (N, D, dt, b, "x differs from var_embed_add")
                assert np.array_equal(gx[b, L:], ox[b, L:]), (N, D, dt, b, "rows past the length were written")
            # own utterance only (the larger cap, both duration forms)
            if tcap == pc.op_tcaps(N)[0]:
                for b in everyone:
                    alone = launch(N, D, dt, tcap, [b], override, ctls)
                    for k in got:
                        assert np.array_equal(bits(alone[k])[0], bits(got[k])[b]), (N, D, dt, override, b, k, "alone")
    log(f"prosody op variance_adapt {dt} N={N} D={D}", worst)


def test_null_controls_are_neutral():
    """ctl == NULL: the plain durations and embedding add, pitch and energy untouched."""
    N, D, dt = 7, 64, "f32"
    i = pc.op_inputs(N, D, dt)
    sel = list(range(len(i["lens"])))
    tcap = pc.op_tcaps(N)[0]
    got = launch(N, D, dt, tcap, sel, False, None, null_ctl=True)
    same = launch(N, D, dt, tcap, sel, False, [pc.controls()] * len(sel))
    for k in got:
        assert np.array_equal(bits(got[k]), bits(same[k])), k
    assert np.array_equal(bits(got["p"]), i["p"].view(np.int32))
    want = pc.op_durations_expected(i["logd"], None, i["lens"], N, tcap, [pc.controls()] * len(sel))
    assert np.array_equal(host(got["dur"]), want[0])


def test_bad_scale_counts_as_one():
    """A duration_scale that is not positive or not finite is treated as 1 by the kernel."""
    N, D, dt = 7, 64, "f32"
    i = pc.op_inputs(N, D, dt)
    sel = list(range(len(i["lens"])))
    tcap = pc.op_tcaps(N)[0]
    bad = [pc.controls(duration_scale=s) for s in (0.0, -2.0, float("nan"), float("inf"), -float("inf"), 1.0)]
    got = launch(N, D, dt, tcap, sel, False, bad)
    want = pc.op_durations_expected(i["logd"], None, i["lens"], N, tcap, [pc.controls()] * len(sel))
    for name, w in zip(("dur", "mel_lens", "tokmap"), want):
        assert np.array_equal(host(got[name]), w), name


def test_refusals():
    """Null buffers, Np < N, B = 0 and a struct size this library does not know: TTS_ERR_INVALID
    with a message, nothing launched (the outputs keep their fill)."""
    N, D, dt = 7, 64, "f32"
    i = pc.op_inputs(N, D, dt)
    B, Np, tcap = len(i["lens"]), pc.op_np(N), 64
    x = dev(i["x"], dt)
    p, e, logd = f32dev(i["p"]), f32dev(i["e"]), f32dev(i["logd"])
    d, m, t = (torch.full(s, -7, dtype=torch.int32, device=DEV) for s in ((B, N), (B,), (B, tcap)))
    par = [dev(i[k]) for k in ("we", "be", "wp", "bp")]
    lens = ints(i["lens"])

    def call(**kw):
        a = dict(x=x, logd=logd, p=p, e=e, lens=lens, B=B, N=N, Np=Np, dur=d, ctl=None)
        a.update(kw)
        eng.variance_adapt_op(dt, a["x"], a["logd"], a["p"], a["e"], a["lens"], a["B"], a["N"], a["Np"], D, *par, tcap,
                              a["dur"], m, t, ctl=a["ctl"])

    for kw, words in ((dict(x=None), "null buffer"), (dict(p=None), "null buffer"), (dict(logd=None), "null buffer"),
                      (dict(dur=None), "null buffer"), (dict(Np=N - 1), "Np >= N"), (dict(B=0), "B, N, D, Tcap > 0")):
        with pytest.raises(RuntimeError, match=words):
            call(**kw)

    class Longer(eng.TtsProsody):
        _fields_ = [("future", eng.ctypes.c_void_p)]

    lib = eng.load_library()
    big = Longer()
    rc_ = lib.tts_op_variance_adapt(0, x.data_ptr(), logd.data_ptr(), p.data_ptr(), e.data_ptr(), lens.data_ptr(), B, N, Np,
                                    D, None, eng.ctypes.cast(eng.ctypes.byref(big), eng.ctypes.POINTER(eng.TtsProsody)),
                                    eng.ctypes.sizeof(big), *(v.data_ptr() for v in par), tcap, d.data_ptr(),
                                    m.data_ptr(), t.data_ptr(), None)
    assert rc_ == -1 and b"tts_prosody" in lib.tts_last_error()
    torch.cuda.synchronize()
    assert (host(d) == -7).all() and (host(m) == -7).all() and (host(t) == -7).all()
    assert np.array_equal(bits(p), i["p"].view(np.int32))
