"""The conv GEMM kernels (csrc/conv_gemm.hip, conv_split.hip, ln_rows.h) at op level, through
tts_op_conv_layer_create / tts_op_conv1d_ex, against the float64 reference and its bound
(oracle/conv.py) on the cases of conv_cases.py: every case, epilogue and input pattern in f16, bf16
and fp32 (split-precision packed and per-utterance, fp32 MFMA with and without split-K), the forms
the grid-size rules pick only on large batches forced through the switches, and the contracts
include/tts_hip.h states for the entry (rows past a length, masked rows, the range word, the
LayerNorm counters, batch invariance).  Every bound comes from the reference alone;
test_conv_op_cpu.py shows what the bounds accept and reject.

Measured worst error / bound per run lands in $PARITY_LOG (profiles/conv_op_parity.json is that
log from an MI355X run): each record's max_abs is the worst ratio (got = 1 + ratio against ones).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
from gonova_tts_amd import engine as eng  # noqa: E402
from oracle import conv as oc  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda:0"
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
NCNT = 64          # LayerNorm row-tile counters (the cases need at most B * ROWS / 32 = 30)
_LAYERS = {}


def layer_for(case, pattern, run, batch):
    form, split, _ = cc.RUNS[run]
    key = (case, pattern, oc.storage(form), split, batch)
    if key not in _LAYERS:
        P, s = cc.problem(case, pattern, "plain", form, batch), cc.shape(case)
        _LAYERS[key] = eng.ConvLayerOp(oc.storage(form), P["w"], P["bias"], dil=s["dil"], pad=s["pad"], split=split)
    return _LAYERS[key]


_DEVICE = {}      # operands already on the device, shared by the runs of a problem


def _dev(a, dt, key=None):
    if key is not None and (key, dt) in _DEVICE:
        return _DEVICE[key, dt]
    with np.errstate(over="ignore", invalid="ignore"):
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(dt).contiguous()
    if key is not None:
        _DEVICE[key, dt] = t
    return t


def launch(case, pattern, epi, run, batch, garbage=None, only=None, cnt=None, poke=None):
    """One tts_op_conv1d_ex launch of a case -> dict(y, ln, lin: float64 arrays with SENTINEL wherever
    nothing was written (None when the case has no such output), flag, kind, kernels, cnt).
    garbage: what x rows past each length hold (default NaN for 16-bit, 1e30 for fp32); only: run
    utterance `only` alone (B = 1); cnt: reuse these counters; poke: (b, row, channel, value) written
    into x before the launch."""
    form, _, ext_f = cc.RUNS[run]
    dt, s = TORCH[oc.storage(form)], cc.shape(case)
    P = cc.problem(case, pattern, epi, form, batch)
    sel = list(range(len(P["lens"]))) if only is None else [only]
    lens = [P["lens"][b] for b in sel]
    B, M, ci = len(sel), s["M"], s["Cin"]
    if garbage is None:
        garbage = 1e30 if dt == torch.float32 else float("nan")
    xkey = None if poke is not None else ("x", case, pattern, batch, only, repr(garbage))
    if xkey is not None and (xkey, dt) in _DEVICE:
        xd = _DEVICE[xkey, dt]
    else:
        x = P["x"][sel].copy()
        for i, L in enumerate(lens):
            x[i, L:] = garbage
        if poke is not None:
            x[poke[0], poke[1], poke[2]] = poke[3]
        xd = _dev(x, dt, xkey)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    y = torch.full((B, cc.ROWS, M), cc.SENTINEL, dtype=dt, device=DEV)
    d = eng.TtsConvDesc()
    d.x, d.sxb, d.sxr, d.x_len, d.x_rows = xd.data_ptr(), cc.ROWS * ci, ci, lens_d.data_ptr(), cc.ROWS
    d.y, d.syb, d.syr, d.y_len, d.y_rows = y.data_ptr(), cc.ROWS * M, M, lens_d.data_ptr(), cc.ROWS
    d.srb, d.srr = cc.ROWS * M, M
    keep = [xd, lens_d, y]
    if P["r1"] is not None:
        r1, r2 = (_dev(P[r][sel], dt, (r, case, pattern, batch, only)) for r in ("r1", "r2"))
        d.r1, d.r2 = r1.data_ptr(), r2.data_ptr()
        keep += [r1, r2]
    d.in_slope, d.alpha, d.out_scale = s["in_slope"], P["alpha"], P["out_scale"]
    d.act_out, d.out_slope = (3, P["out_slope"]) if P["act"] else (0, 0.0)   # ACT_LRELU
    d.B = B
    x_ = eng.TtsConvExt()
    x_.rows_pad, x_.no_split, x_.f32_splitk = ext_f.get("rows_pad", 0), ext_f.get("no_split", 0), ext_f.get("f32_splitk", 0)
    if ext_f.get("ws"):
        n = eng.conv_ws_bytes(s["k"], ci, M, B * cc.ROWS)
        if n:
            ws = torch.empty(n // 4, dtype=torch.float32, device=DEV)
            x_.ws, x_.ws_bytes = ws.data_ptr(), n
            keep.append(ws)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x_.range_flag = flag.data_ptr()
    ln, ln_out, lin_out = P["ln"], None, None
    if ln is not None:
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
        g1, b1 = f32(ln["g1"]), f32(ln["b1"])
        x_.ln_g1, x_.ln_b1, x_.ln_eps = g1.data_ptr(), b1.data_ptr(), ln["eps"]
        keep += [g1, b1]
        if ln["g2"] is not None:
            g2, b2 = f32(ln["g2"]), f32(ln["b2"])
            x_.ln_g2, x_.ln_b2 = g2.data_ptr(), b2.data_ptr()
            keep += [g2, b2]
        if ln["lin_w"] is not None:
            lw = f32(ln["lin_w"])
            lin_out = torch.full((B, cc.ROWS), cc.SENTINEL, dtype=torch.float32, device=DEV)
            x_.ln_lin_w, x_.ln_lin_b, x_.ln_lin_out = lw.data_ptr(), ln["lin_b"], lin_out.data_ptr()
            keep.append(lw)
        else:
            ln_out = torch.full((B, cc.ROWS, M), cc.SENTINEL, dtype=dt, device=DEV)
            x_.ln_out = ln_out.data_ptr()
        cnt = torch.zeros(NCNT, dtype=torch.int32, device=DEV) if cnt is None else cnt
        x_.ln_cnt, x_.ln_cnt_n = cnt.data_ptr(), NCNT
    try:
        kind, kernels = eng.conv1d_ex_op(layer_for(case, pattern, run, batch), d, x_)
        torch.cuda.synchronize()
        host = lambda t: None if t is None else t.float().cpu().numpy().astype(np.float64)
        return dict(y=host(y), ln=host(ln_out), lin=host(lin_out), flag=int(flag.item()), kind=kind, kernels=kernels,
                    cnt=cnt, lens=lens)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error, nothing more is started on the GPU: {e}", returncode=3)
        raise


def ratios(out, case, pattern, epi, run, batch, only=None, ln_in_launch=None, y_written=True):
    """Worst |got - reference| / bound of every utterance and output (a list), after checking what
    the header says about rows at or past each length: y, ln_out and ln_lin_out keep their sentinel
    (ln_lin_out only when the launch applied the LayerNorm itself: the separate LayerNorm + Linear
    launch writes every row), and a launch whose split-K reduce applied the LayerNorm never wrote y."""
    form = cc.RUNS[run][0]
    S = cc.slices_of(case, run)
    refs, bnds = cc.reference(case, pattern, epi, form, batch), cc.bound(case, pattern, epi, form, batch, S=S)
    sel = list(range(len(refs))) if only is None else [only]
    worst = []
    for i, b in enumerate(sel):
        L = out["lens"][i]
        for key in ("y", "ln", "lin"):
            got = out[key]
            if got is None:
                continue
            where = (case, pattern, epi, run, batch, b, key)
            if key == "y" and not y_written:
                assert (got[i] == cc.SENTINEL).all(), (where, "the reduce + LayerNorm launch wrote y")
                continue
            if key != "lin" or ln_in_launch:
                assert (got[i, L:] == cc.SENTINEL).all(), (where, "rows past the length were written")
            if L:
                assert np.isfinite(got[i, :L]).all(), where
                r = np.abs(got[i, :L] - refs[b][key]) / bnds[b][key]
                worst.append(float(r.max()))
    return worst


def rel_error(out, case, pattern, batch):
    """Worst |y - reference| / sum |x||w| of a plain split-precision launch, in units of 2^-21."""
    refs = cc.reference(case, pattern, "plain", "split", batch)
    top = 0.0
    for b, L in enumerate(out["lens"]):
        if L:
            top = max(top, float((np.abs(out["y"][b, :L] - refs[b]["y"]) / refs[b]["base"]["Axw"]).max()))
    return top * 2.0 ** 21


def log(name, worst):
    w = np.asarray(worst if worst else [0.0])
    check(name, 1.0 + w, np.ones_like(w), max_abs_tol=1.0)


# ------------------------------------------------------------------------ against the bound
@pytest.mark.parametrize("case", list(cc.CASES))
@pytest.mark.parametrize("run", list(cc.RUNS))
def test_parity(run, case):
    """Every epilogue, pattern and batch of a case under the reference's bound; the family and the
    kernel count the launcher reports are the ones the shapes predict; rows past each length as the
    header states; masked rows full of NaN (16-bit) / 1e30 (fp32) raise no range flag."""
    worst, rel21 = [], {}
    for epi in cc.EPILOGUES:
        want = cc.expected(case, run, epi)
        for pattern in cc.PATTERNS:
            for batch in cc.BATCHES:
                out = launch(case, pattern, epi, run, batch)
                assert (out["kind"], out["kernels"]) == (want["kind"], want["kernels"]), (case, run, epi, out["kind"], out["kernels"], want)
                assert out["flag"] == 0, (case, run, epi, pattern, batch, "range flag raised by masked rows")
                y_written = not (want["ln_in_launch"] and want["S"] > 1)
                worst += ratios(out, case, pattern, epi, run, batch, ln_in_launch=want["ln_in_launch"], y_written=y_written)
                if cc.RUNS[run][0] == "split" and epi == "plain" and pattern in ("normal", "small") and y_written:
                    rel21[pattern] = max(rel21.get(pattern, 0.0), rel_error(out, case, pattern, batch))
    for pattern, v in rel21.items():   # logged, not bounded: the figure the header's error model quotes
        check(f"conv op {run} case {case} {pattern}: worst |error| / sum|x||w| in units of 2^-21", 1.0 + np.array([v]), np.ones(1))
    log(f"conv op {run} {want['family']} case {case} (cg {want['cg']}, S {want['S']})", worst)


# ------------------------------------------------------------------------------ forced forms
XRES_FORMS = [dict(), dict(TTS_XRES_NARROW=0), dict(TTS_XRES_NARROW=1), dict(TTS_XRES_NARROW=0, TTS_XRES_NT=2),
              dict(TTS_XRES_NARROW=0, TTS_XRES_NT=3), dict(TTS_XRES_NARROW=0, TTS_XRES_NT=4),
              dict(TTS_XRES_NARROW=0, TTS_XRES_DMA=2), dict(TTS_XRES_NARROW=0, TTS_XRES_DMA=3),
              dict(TTS_XRES_NARROW=0, TTS_XRES_NT=4, TTS_XRES_DMA=2),
              dict(TTS_XRES_NARROW=0, TTS_XRES_ORDER=0), dict(TTS_XRES_NARROW=0, TTS_XRES_ORDER=1),
              dict(TTS_XRES_NARROW=0, TTS_XRES_ORDER=2), dict(TTS_XRES_NARROW=1, TTS_XRES_ORDER=0),
              dict(TTS_LN_FUSE=0), dict(TTS_LN_FUSE=7), dict(TTS_LN_FUSE=7, TTS_XRES_NARROW=0),
              dict(TTS_LN_FUSE=7, TTS_XRES_NARROW=0, TTS_XRES_NT=4), dict(TTS_LN_FUSE=7, TTS_XRES_NARROW=0, TTS_XRES_ORDER=0)]
# TTS_XRES_DMA=0 gives a multi-tap layer the channel group its LDS tile allows instead of 64: another
# K order, so only the bound holds; a 1-tap layer keeps its group (the source says so for both)
XRES_DMA_OFF = dict(TTS_XRES_NARROW=0, TTS_XRES_DMA=0)


def apply(switch, form_sw):
    for name in ("TTS_XRES_NARROW", "TTS_XRES_NT", "TTS_XRES_DMA", "TTS_XRES_ORDER", "TTS_LN_FUSE", "TTS_SPLIT_NT1",
                 "TTS_SPLIT_WHOLE"):
        switch(name, form_sw.get(name))


@pytest.mark.parametrize("case", ["d", "e", "f", "h", "i"])
@pytest.mark.parametrize("run", ["f16", "bf16"])
def test_xres_forms(run, case, switch):
    """conv_xres_kernel's tile heights (64 / 96 / 128 rows), narrow 64 x 64 tiles, the DMA forms
    against the register-staged one, the three block orders and the LayerNorm tail: each under the
    bound, all bit-identical to the default form (one channel group, so one K order); with the
    tail the launch reports one kernel, without it two."""
    has_ln = cc.shape(case)["ln"] is not None
    for epi in ("plain", "res"):
        base, worst = None, []
        for fs in XRES_FORMS + [XRES_DMA_OFF]:
            apply(switch, fs)
            out = launch(case, "normal", epi, run, "long")
            assert out["kind"] == cc.PK_CONV_XRES
            fused = has_ln and fs.get("TTS_LN_FUSE") == 7 and fs.get("TTS_XRES_NT") != 3
            assert out["kernels"] == (1 if fused or not has_ln else 2), (case, run, fs, out["kernels"])
            worst += ratios(out, case, "normal", epi, run, "long", ln_in_launch=fused)
            if has_ln:
                assert not out["cnt"].any().item(), (case, run, fs, "LayerNorm counters not back at zero")
            if base is None:
                base = out
            elif fs is not XRES_DMA_OFF or cc.shape(case)["k"] == 1:
                for key in ("y", "ln", "lin"):   # (valid rows: the separate LayerNorm + Linear also writes the others)
                    if base[key] is not None:
                        for i, L in enumerate(out["lens"]):
                            assert np.array_equal(out[key][i, :L], base[key][i, :L]), (case, run, epi, fs, key, "differs from the default form")
        log(f"conv op {run} conv_xres forced forms case {case} {epi}", worst)


SPLITP_FORMS = [dict(), dict(TTS_SPLIT_NT1=0), dict(TTS_SPLIT_NT1=1), dict(TTS_SPLIT_NT1=4), dict(TTS_SPLIT_WHOLE=0),
                dict(TTS_SPLIT_WHOLE=1), dict(TTS_SPLIT_NT1=0, TTS_SPLIT_WHOLE=0), dict(TTS_LN_FUSE=0), dict(TTS_LN_FUSE=7),
                dict(TTS_LN_FUSE=7, TTS_SPLIT_NT1=4), dict(TTS_LN_FUSE=7, TTS_SPLIT_NT1=0, TTS_SPLIT_WHOLE=0)]


@pytest.mark.parametrize("case", ["c", "e", "f", "i", "j"])
def test_packed_split_forms(case, switch):
    """conv_splitp_kernel at 32-, 64- and 128-row tiles, whole-slice staging on and off, and its
    LayerNorm tail: each under the bound and bit-identical to the default form (a row's K order does
    not depend on the tile); one kernel with the tail or one slice, two with a reduce or a separate
    LayerNorm.  The per-utterance kernel (rows_pad = 0) is held to the bound on its own in test_parity."""
    want = cc.expected(case, "split")
    assert want["family"] == "conv_splitp"
    has_ln = cc.shape(case)["ln"] is not None
    for epi in ("plain", "res"):
        base, worst = None, []
        for fs in SPLITP_FORMS:
            apply(switch, fs)
            out = launch(case, "normal", epi, "split", "long")
            assert out["kind"] == cc.PK_CONV_SPLIT
            in_launch = has_ln and (want["ln_in_launch"] if want["S"] > 1 else fs.get("TTS_LN_FUSE") == 7)
            assert out["kernels"] == (2 if want["S"] > 1 else 1) + (1 if has_ln and not in_launch else 0), (case, fs, out["kernels"])
            y_written = not (in_launch and want["S"] > 1)
            worst += ratios(out, case, "normal", epi, "split", "long", ln_in_launch=in_launch, y_written=y_written)
            if has_ln:
                assert not out["cnt"].any().item(), (case, fs, "LayerNorm counters not back at zero")
            if base is None:
                base = out
            else:
                for key in ("y", "ln", "lin"):
                    if base[key] is not None:
                        for i, L in enumerate(out["lens"]):
                            assert np.array_equal(out[key][i, :L], base[key][i, :L]), (case, epi, fs, key, "differs from the default form")
        log(f"conv op split conv_splitp forced forms case {case} {epi}", worst)


def test_packed_split_k_needs_its_workspace():
    """Case i without a workspace runs one slice (one kernel + the LayerNorm launch) under the same bound."""
    run = "split_nows"
    cc.RUNS[run] = ("split", True, dict(rows_pad=cc.ROWS_PAD))
    try:
        out = launch("i", "normal", "plain", run, "long")
        assert (out["kind"], out["kernels"]) == (cc.PK_CONV_SPLIT, 2)
        log("conv op split conv_splitp case i without workspace (S 1)", ratios(out, "i", "normal", "plain", run, "long"))
    finally:
        del cc.RUNS[run]


# ---------------------------------------------------------------------------------- contracts
@pytest.mark.parametrize("case", list(cc.CASES))
@pytest.mark.parametrize("run", list(cc.RUNS))
def test_masked_rows_and_batch_invariance(run, case):
    """What the masked x rows hold -- 3.0, 1e30 (fp32) or NaN -- changes no bit of any output and
    leaves the range word 0; and every utterance run alone (B = 1, another grid) equals its rows in
    the batch bit for bit."""
    fills = [cc.GARBAGE, float("nan")] + ([1e30] if cc.RUNS[run][0] in ("f32", "split") else [])
    for batch in cc.BATCHES:
        outs = [launch(case, "normal", "res", run, batch, garbage=g) for g in fills]
        for o, g in zip(outs, fills):
            assert o["flag"] == 0, (case, run, batch, g)
            for key in ("y", "ln", "lin"):
                if o[key] is not None:
                    for i, L in enumerate(o["lens"]):
                        assert np.array_equal(o[key][i, :L], outs[0][key][i, :L]), (case, run, batch, key, g)
        for b, L in enumerate(cc.BATCHES[batch]):
            alone = launch(case, "normal", "res", run, batch, only=b)
            for key in ("y", "ln", "lin"):
                if alone[key] is not None:
                    assert np.array_equal(alone[key][0, :L], outs[1][key][b, :L]), (case, run, batch, b, key, "alone != in the batch")
                    if key != "lin":
                        assert (alone[key][0, L:] == cc.SENTINEL).all(), (case, run, batch, b, key)


@pytest.mark.parametrize("run", ["split", "split_utt"])
def test_range_flag(run):
    """One valid activation at 65520 (f16 rounds it to inf) or NaN raises the range word of the
    split form; 65504, f16's largest, does not; the fp32 MFMA form never touches the word."""
    for case in ("c", "a"):
        for value, want in ((65504.0, 0), (65520.0, 1), (float("nan"), 1)):
            out = launch(case, "normal", "plain", run, "long", poke=(3, 100, 7, value))
            assert out["flag"] == want, (case, run, value)
    assert launch("c", "normal", "plain", "no_split", "long", poke=(3, 100, 7, 7e4))["flag"] == 0


@pytest.mark.parametrize("run,case,fs", [("f16", "e", dict(TTS_LN_FUSE=7)), ("bf16", "f", dict(TTS_LN_FUSE=7, TTS_XRES_NARROW=0)),
                                         ("split", "e", dict(TTS_LN_FUSE=7)), ("split", "f", dict(TTS_LN_FUSE=7))])
def test_layernorm_counters_are_reusable(run, case, fs, switch):
    """ln_cnt is all zero after a launch with the LayerNorm tail, and a second launch straight
    after it on the same counters gives the same bits."""
    apply(switch, fs)
    first = launch(case, "normal", "res", run, "long")
    assert first["kernels"] == 1 and not first["cnt"].any().item()
    again = launch(case, "normal", "res", run, "long", cnt=first["cnt"])
    assert not again["cnt"].any().item()
    for key in ("y", "ln", "lin"):
        if first[key] is not None:
            assert np.array_equal(first[key], again[key]), (run, case, key)


@pytest.mark.parametrize("run", list(cc.RUNS))
def test_empty_utterance_writes_nothing(run):
    """B = 1 with length 0, with and without a LayerNorm: every output keeps its sentinel (ln_lin_out
    under the separate LayerNorm + Linear launch excepted: it is written for every row)."""
    for case in ("c", "e", "f"):
        out = launch(case, "normal", "res", run, "long", only=0)
        assert out["lens"] == [0]
        for key in ("y", "ln"):
            if out[key] is not None:
                assert (out[key] == cc.SENTINEL).all(), (run, case, key)


def test_op_entry_refuses_what_the_kernels_do_not_take():
    """TTS_ERR_INVALID with a message, nothing launched."""
    z = torch.zeros((1, 32, 64), device=DEV)
    lens = torch.tensor([32], dtype=torch.int32, device=DEV)

    def desc(M, ci, **kw):
        d = eng.TtsConvDesc()
        d.x, d.sxb, d.sxr, d.x_len, d.x_rows = z.data_ptr(), 32 * ci, ci, lens.data_ptr(), 32
        d.y, d.syb, d.syr, d.y_len, d.y_rows = z.data_ptr(), 32 * M, M, lens.data_ptr(), 32
        d.in_slope, d.alpha, d.out_scale, d.B = 1.0, 1.0, 1.0, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    with pytest.raises(RuntimeError, match="split form takes an fp32"):
        eng.ConvLayerOp("f16", np.zeros((8, 8, 1)), split=True)
    wide = eng.ConvLayerOp("f32", np.zeros((8, 8, 67)), pad=33)
    with pytest.raises(RuntimeError, match="receptive field"):
        eng.conv1d_ex_op(wide, desc(8, 8))
    odd = eng.ConvLayerOp("f32", np.zeros((6, 8, 1)))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        eng.conv1d_ex_op(odd, desc(6, 8))
    ok = eng.ConvLayerOp("f32", np.zeros((8, 8, 1)))
    with pytest.raises(RuntimeError, match="up_s"):
        eng.conv1d_ex_op(ok, desc(8, 8, up_s=2))
    ext = eng.TtsConvExt()
    ext.ln_out = z.data_ptr()
    with pytest.raises(RuntimeError, match="ln_g1"):
        eng.conv1d_ex_op(ok, desc(8, 8), ext)
    big = eng.ConvLayerOp("f32", np.zeros((128, 64, 1)))
    ext = eng.TtsConvExt()
    ext.f32_splitk = 1
    with pytest.raises(RuntimeError, match="split-K workspace"):
        eng.conv1d_ex_op(big, desc(128, 64), ext)
    assert eng.conv_ws_bytes(3, 768, 128, 960) == 16 * 960 * 128 * 4 and eng.conv_ws_bytes(1, 32, 64, 960) == 0
    for layer in (wide, odd, ok, big):
        layer.close()
