"""The acoustic model's row-wise kernels (csrc/acoustic_kernels.hip) at op level, through the
tts_op_* entries, on the cases of rowwise_cases.py: the exact ops against the expected bits, the
ops that compute against the float64 reference and its bound (oracle/rowwise.py), in f16, bf16 and
fp32, and the contracts include/tts_hip.h states for each entry -- what is written, zeroed or left
alone at or past a length, that masked input never reaches a valid output whatever it holds, and
that an utterance run alone (B = 1) equals its rows in the batch bit for bit.  Every bound comes
from the reference alone; test_rowwise_op_cpu.py shows what the bounds accept and reject.

Measured worst error / bound per op and dtype lands in $PARITY_LOG (profiles/rowwise_op_parity.json
is that log from an MI355X run): each record's max_abs is the worst ratio (got = 1 + ratio against ones).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rowwise_cases as rc  # noqa: E402
from gonova_tts_amd import engine as eng  # noqa: E402
from oracle import rowwise as rw  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda:0"
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
NAN = float("nan")


def dev(a, dt="f32"):
    """A float64 array of values of dt -> device tensor of dt (converted on the host: exact)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH[dt]).to(DEV).contiguous()


def ints(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def full(shape, dt, value=rc.SENTINEL):
    return torch.full(shape, value, dtype=TORCH[dt], device=DEV)


def host(t):
    return t.cpu().float().numpy() if t.dtype != torch.int32 else t.cpu().numpy()


def run(fn, *a, **kw):
    """One op launch; a device error ends the session (nothing more is started on the GPU)."""
    try:
        fn(*a, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error, nothing more is started on the GPU: {e}", returncode=3)
        raise


def fills(dt):
    """What masked input holds: the default first (NaN in 16-bit, 1e30 in fp32), then the alternatives."""
    return (1e30, NAN, rc.GARBAGE) if dt == "f32" else (NAN, rc.GARBAGE)


def ratio(got, ref, bnd, where):
    assert np.isfinite(got).all(), where
    return float((np.abs(got - ref) / bnd).max()) if ref.size else 0.0


def log(name, worst):
    w = np.asarray(worst if worst else [0.0])
    check(name, 1.0 + w, np.ones_like(w), max_abs_tol=1.0)


# ------------------------------------------------------------------------------------ glu_dwconv
def glu_launch(case, pattern, dt, fill, only=None):
    P = rc.glu_problem(case, pattern, dt)
    k, D = rc.GLU_CASES[case][:2]
    sel = list(range(len(rc.GLU_LENS))) if only is None else [only]
    a = P["a"][sel].copy()
    lens = [rc.GLU_LENS[b] for b in sel]
    for i, L in enumerate(lens):
        a[i, L:] = fill
    out = full((len(sel), rc.GLU_TM, D), dt)
    run(eng.glu_dwconv_op, dt, dev(a, dt), ints(lens), len(sel), rc.GLU_TM, D, dev(P["w"]), k, dev(P["bias"]), out)
    return host(out)


@pytest.mark.parametrize("case,dt", [(c, dt) for c, v in rc.GLU_CASES.items() for dt in v[2]])
def test_glu_dwconv(case, dt):
    """Every pattern under the bound; rows >= len keep the sentinel (length 0: the whole utterance);
    what the masked rows hold changes no valid bit; every utterance alone equals its rows in the batch."""
    worst = {}
    for pattern in rc.GLU_PATTERNS:
        refs, bnds = rc.glu_reference(case, pattern, dt)
        got = glu_launch(case, pattern, dt, fills(dt)[0])
        for b, L in enumerate(rc.GLU_LENS):
            assert (got[b, L:] == rc.SENTINEL).all(), (case, dt, pattern, b, "rows past the length were written")
            worst.setdefault(pattern, []).append(ratio(got[b, :L], refs[b]["y"], bnds[b], (case, dt, pattern, b)))
        print(f"[rowwise op] glu_dwconv {case} {dt} {pattern}: worst {max(worst[pattern]):.3f} of the bound")
        if pattern == "normal":
            for f in fills(dt)[1:]:
                other = glu_launch(case, pattern, dt, f)
                for b, L in enumerate(rc.GLU_LENS):
                    assert rc.same_bits(other[b, :L], got[b, :L]), (case, dt, b, f, "masked rows reached a valid output")
            for b, L in enumerate(rc.GLU_LENS):
                alone = glu_launch(case, pattern, dt, fills(dt)[0], only=b)
                assert rc.same_bits(alone[0, :L], got[b, :L]), (case, dt, b, "alone != in the batch")
                assert (alone[0, L:] == rc.SENTINEL).all()
    for pattern, w in worst.items():
        assert max(w) < 1.0, (case, dt, pattern, max(w))
    log(f"rowwise op glu_dwconv {dt} case {case} ({rc.glu_kernel(*rc.GLU_CASES[case][:2], dt)} kernel)", sum(worst.values(), []))


# ----------------------------------------------------------------------------------- rel_softmax
def sm_launch(Tm, pattern, dt, fill, only=None):
    P = rc.sm_problem(Tm, pattern, dt)
    Sac, Sbd, Sk = rc.sm_extents(Tm)
    sel = list(range(len(P["lens"]))) if only is None else [only]
    lens = [P["lens"][b] for b in sel]
    ac, bd = rc.sm_mask(P["ac"][sel], P["bd"][sel], lens, Tm, fill)
    p = full((len(sel), rc.SM_H, Tm, Sk), dt)
    run(eng.rel_softmax_op, dt, dev(ac, dt), dev(bd, dt), ints(lens), len(sel), rc.SM_H, Tm, Sac, Sbd, Sk, rc.SM_SCALE, p)
    return host(p), lens


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("Tm", rc.SM_TM)
def test_rel_softmax(Tm, dt):
    """Valid rows: columns < len under the bound, their sum within the bound of 1, columns in
    [len, Sk) exactly 0 although the inputs hold NaN there.  Rows in [len, Tm) are computed from
    whatever the inputs hold (the header says so): their columns from max(len, 1) on are 0, for
    length 0 too, where column 0 is read and written."""
    worst = []
    for pattern in rc.SM_PATTERNS:
        refs, bnds = rc.sm_reference(Tm, pattern, dt)
        got, lens = sm_launch(Tm, pattern, dt, NAN)
        for b, L in enumerate(lens):
            where = (Tm, dt, pattern, b)
            assert (got[b, :, :, max(L, 1):] == 0).all(), (where, "columns past the length are not all zero")
            assert not (got[b, :, :, 0] == rc.SENTINEL).any(), (where, "column 0 left unwritten")
            if L:
                v = got[b, :, :L, :L].astype(np.float64)
                worst.append(ratio(v, refs[b]["p"], bnds[b], where))
                assert (np.abs(v.sum(-1) - 1.0) <= bnds[b].sum(-1)).all(), (where, "row sum")
        if pattern == "normal":
            for f in fills(dt)[1:]:
                other, _ = sm_launch(Tm, pattern, dt, f)
                for b, L in enumerate(lens):
                    assert rc.same_bits(other[b, :, :L], got[b, :, :L]), (Tm, dt, b, f, "masked input reached a valid row")
            for b, L in enumerate(lens):
                alone, _ = sm_launch(Tm, pattern, dt, NAN, only=b)
                assert rc.same_bits(alone[0, :, :L], got[b, :, :L]), (Tm, dt, b, "alone != in the batch")
    assert max(worst) < 1.0, (Tm, dt, max(worst))
    log(f"rowwise op rel_softmax {dt} Tm {Tm}", worst)


# ----------------------------------------------------------------------------------- transpose_v
@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("dk", rc.TV_DK)
def test_transpose_v(dk, dt):
    """The bits of v transposed (-0, subnormals, inf, the largest finite value); keys in [len, Sk)
    exactly 0 whatever the rows past the length hold; nothing written past the buffer's Sk columns."""
    qkv, want = rc.tv_inputs(dk, dt)
    D, B = rc.TV_H * dk, len(rc.TV_LENS)
    n = B * rc.TV_H * dk * rc.TV_SK

    def launch(fill, only=None):
        sel = list(range(B)) if only is None else [only]
        x = qkv[sel].copy()
        lens = [rc.TV_LENS[b] for b in sel]
        for i, L in enumerate(lens):
            x[i, L:] = fill
        m = len(sel) * rc.TV_H * dk * rc.TV_SK
        vt = full((m + 256,), dt)
        run(eng.transpose_v_op, dt, dev(x, dt), ints(lens), len(sel), rc.TV_TM, D, rc.TV_H, rc.TV_SK, vt)
        got = host(vt)
        assert (got[m:] == rc.SENTINEL).all(), (dk, dt, "written past the output")
        return got[:m].reshape(len(sel), rc.TV_H, dk, rc.TV_SK)

    for f in fills(dt):
        got = launch(f)
        assert rc.same_bits(got, want), (dk, dt, f, np.argwhere(got.view(np.uint32) != want.astype(np.float32).view(np.uint32))[:4])
    for b in range(B):
        assert rc.same_bits(launch(NAN, only=b)[0], want[b]), (dk, dt, b, "alone")
    assert n == want.size


# ------------------------------------------------------------- pos_bias, var_embed_add, mel_out
@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("shape", list(rc.EW_SHAPES))
def test_pos_bias(shape, dt):
    """One fp32 add, one rounding: the expected bits, on D = 72 and past one trip of the grid-stride loop."""
    rows, D = rc.EW_SHAPES[shape]
    qkv, u, v, (wu, wv) = rc.pb_inputs(shape, dt)
    x = qkv.copy()
    x[:, D:] = NAN      # the k and v slices are not read
    qu, qv = full((rows, D), dt), full((rows, D), dt)
    run(eng.pos_bias_op, dt, dev(x, dt), rows, D, dev(u), dev(v), qu, qv)
    assert rc.same_bits(host(qu), wu) and rc.same_bits(host(qv), wv), (shape, dt)


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("shape", list(rc.EW_SHAPES))
def test_var_embed_add(shape, dt):
    rows, D = rc.EW_SHAPES[shape]
    i, ref, bnd = rc.ve_inputs(shape, dt)
    x = dev(i["x"], dt)
    run(eng.var_embed_add_op, dt, x, rows, D, *(dev(i[k]) for k in ("e", "we", "be", "p", "wp", "bp")))
    r = ratio(host(x).astype(np.float64), ref["y"], bnd, (shape, dt))
    assert r < 1.0, (shape, dt, r)
    log(f"rowwise op var_embed_add {dt} {shape}", [r])


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("shape", list(rc.MEL_SHAPES))
def test_mel_out(shape, dt):
    """Rows below the length copied bit for bit (widened to fp32), the rest of the Tcap rows zeroed;
    input rows at or past the length are not read (they hold NaN)."""
    B, Tin, Tcap, C, lens = rc.MEL_SHAPES[shape]
    x, want = rc.mel_inputs(shape, dt)
    for f in fills(dt):
        xin = x.copy()
        for b, L in enumerate(lens):
            xin[b, L:] = f
        out = full((B, Tcap, C), "f32")
        run(eng.mel_out_op, dt, dev(xin, dt), ints(lens), B, Tin, Tcap, C, out)
        assert rc.same_bits(host(out), want), (shape, dt, f)
    for b, L in enumerate(lens):
        out = full((1, Tcap, C), "f32")
        run(eng.mel_out_op, dt, dev(x[b:b + 1], dt), ints([L]), 1, Tin, Tcap, C, out)
        assert rc.same_bits(host(out)[0], want[b]), (shape, dt, b, "alone")


# ------------------------------------------------------------------------------- embed, regulate
@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("D", rc.EMB_D)
def test_embed(D, dt):
    """table row * sqrt(D), one rounding; ids clamped to the table on both sides, lens clamped to N,
    rows in [len, Tm) zeroed (every row is written), ids past the length not read."""
    ids, table, scale, want = rc.emb_inputs(D, dt)
    B = len(rc.EMB_LENS)
    wild = ids.copy()
    for b, L in enumerate(rc.EMB_LENS):
        wild[b, L:] = 2 ** 31 - 1
    for i in (ids, wild):
        out = full((B, rc.EMB_TM, D), dt)
        run(eng.embed_op, dt, ints(i), ints(rc.EMB_LENS), B, rc.EMB_N, rc.EMB_TM, dev(table, dt), rc.EMB_V, D, scale, out)
        assert rc.same_bits(host(out), want), (D, dt)
    for b, L in enumerate(rc.EMB_LENS):
        out = full((1, rc.EMB_TM, D), dt)
        run(eng.embed_op, dt, ints(ids[b:b + 1]), ints([L]), 1, rc.EMB_N, rc.EMB_TM, dev(table, dt), rc.EMB_V, D, scale, out)
        assert rc.same_bits(host(out)[0], want[b]), (D, dt, b, "alone")


@pytest.mark.parametrize("form", rc.REG_FORMS)
@pytest.mark.parametrize("D", rc.EMB_D)
def test_regulate(D, form):
    """Gathered row * scale, one rounding (fp32 in, 16-bit out included); token -1 rows zeroed; rows in
    [frames, Tout) keep the sentinel."""
    dt_in, dt = form
    enc, tokmap, scale, want = rc.reg_inputs(D, dt_in, dt)
    out = full((rc.REG_B, rc.REG_TOUT, D), dt)
    run(eng.regulate_op, dt_in, dt, dev(enc, dt_in), rc.REG_B, rc.REG_N, D, ints(tokmap), rc.REG_TCAP, rc.REG_FRAMES,
        rc.REG_TOUT, scale, out)
    assert rc.same_bits(host(out), want), (D, form)
    for b in range(rc.REG_B):
        out = full((1, rc.REG_TOUT, D), dt)
        run(eng.regulate_op, dt_in, dt, dev(enc[b:b + 1], dt_in), 1, rc.REG_N, D, ints(tokmap[b:b + 1]), rc.REG_TCAP,
            rc.REG_FRAMES, rc.REG_TOUT, scale, out)
        assert rc.same_bits(host(out)[0], want[b]), (D, form, b, "alone")


# ------------------------------------------------------------------------------------- durations
@pytest.mark.parametrize("N", rc.DUR_N)
def test_durations(N):
    """dur, mel_lens and the frame -> token map as the header states them: predicted and overridden
    durations, every speed (ties to even), zero-duration tokens, the all-zero rule on one utterance of
    a batch, a frame cap below the total, NaN / 1e30 / wild overrides past the length."""
    logd, ovr, lens = rc.dur_inputs(N)
    B = len(lens)

    def launch(tcap, speed, o, sel):
        d, m, t = (torch.full(s, -7, dtype=torch.int32, device=DEV) for s in ((len(sel), N), (len(sel),), (len(sel), tcap)))
        run(eng.durations_op, dev(logd[sel]) if o is None else None, ints([lens[b] for b in sel]), len(sel), N, tcap, d, m, t,
            override_d=None if o is None else ints(o[sel]), speed=speed)
        return host(d), host(m), host(t)

    for tcap in rc.dur_tcaps(N):
        for speed in rc.DUR_SPEEDS:
            for o in (None, ovr):
                want = rw.durations_expected(logd, lens, N, tcap, override_d=o, speed=speed)
                got = launch(tcap, speed, o, list(range(B)))
                for name, g, w in zip(("dur", "mel_lens", "tokmap"), got, want):
                    assert np.array_equal(g, w), (N, tcap, speed, o is not None, name, np.argwhere(g != w)[:4])
                # below the cap's total dur keeps the durations and mel_lens the cap: the caller's sign
                assert (want[0].sum(1) > want[1]).any() == (tcap == rc.dur_tcaps(N)[1]), (N, tcap, speed)
                if speed == 1.5:
                    for b in range(B):
                        alone = launch(tcap, speed, o, [b])
                        for g, w in zip(alone, want):
                            assert np.array_equal(g[0], w[b]), (N, tcap, o is not None, b, "alone")


# -------------------------------------------------------------------------------------- spk_bias
@pytest.mark.parametrize("dt", rc.DTYPES)
def test_spk_bias(dt):
    """E in {1, 64, 300} (past the 256-thread stride), D in {72, 384}: unit, zero (the 1e-12 clamp:
    the bias itself), 1e-20 and 1e3 norms."""
    worst = []
    for E in rc.SPK_E:
        for D in rc.SPK_D:
            e, We, bias = rc.spk_inputs(E, D)
            B = len(rc.SPK_ROWS)
            out = full((B, D), dt)
            run(eng.spk_bias_op, dt, dev(e), B, E, dev(We), dev(bias), D, out)
            got = host(out).astype(np.float64)
            for r in range(B):
                ref = rw.spk_reference(e[r], We, bias)
                worst.append(ratio(got[r], ref["y"], rw.spk_bound(e[r], We, bias, dt, ref), (E, D, dt, r)))
                alone = full((1, D), dt)
                run(eng.spk_bias_op, dt, dev(e[r:r + 1]), 1, E, dev(We), dev(bias), D, alone)
                assert rc.same_bits(host(alone)[0], got[r]), (E, D, dt, r, "alone")
            assert rc.same_bits(got[1], rw.round_to(bias, dt)), (E, D, dt, "zero embedding")
    assert max(worst) < 1.0, (dt, max(worst))
    log(f"rowwise op spk_bias {dt}", worst)


# ------------------------------------------------------------------------------------- LayerNorm
def offset4(a):
    """The fp32 values at a device address 4 bytes past a 16-byte boundary."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = dev(a)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("C", rc.LN_C)
def test_layernorm(C, dt):
    """One and two LayerNorms under the bound (the mean-100 row and the constant row included); gains
    at a 16-byte-aligned address and 4 bytes past one give the same bits; rows >= len are neither
    read (they hold NaN) nor written; an utterance alone equals its rows in the batch."""
    x, par = rc.ln_inputs(C, dt)
    rows, valid = x.shape[0], rc.ln_valid_rows()
    xin = np.full_like(x, NAN)
    xin[valid] = x[valid]
    worst = []
    for two in (False, True):
        ref, bnd = rc.ln_reference(C, dt, two)
        n = 4 if two else 2
        outs = []
        for place in (dev, offset4):
            p = [place(v) for v in par[:n]] + [None] * (4 - n)
            assert all(t is None or t.data_ptr() % 16 == (0 if place is dev else 4) for t in p)
            out = full((rows, C), dt)
            run(eng.layernorm_op, dt, dev(xin, dt), out, rows, C, *p, eps=rc.EPS, lens=ints(rc.LN_LENS), stride=rc.LN_STRIDE)
            outs.append(host(out))
        got = outs[0]
        assert rc.same_bits(outs[0], outs[1]), (C, dt, two, "aligned and offset gains differ")
        masked = np.setdiff1d(np.arange(rows), valid)
        assert (got[masked] == rc.SENTINEL).all(), (C, dt, two, "rows past a length were written")
        worst.append(ratio(got[valid].astype(np.float64), ref["ln"], bnd, (C, dt, two)))
        for b, L in enumerate(rc.LN_LENS):
            rs = slice(b * rc.LN_STRIDE, (b + 1) * rc.LN_STRIDE)
            out = full((rc.LN_STRIDE, C), dt)
            run(eng.layernorm_op, dt, dev(xin[rs], dt), out, rc.LN_STRIDE, C, *p, eps=rc.EPS, lens=ints([L]), stride=rc.LN_STRIDE)
            assert rc.same_bits(host(out), got[rs]), (C, dt, two, b, "alone")
        xd = dev(x, dt)      # without lens, in place: every row
        run(eng.layernorm_op, dt, xd, xd, rows, C, *p, eps=rc.EPS)
        assert rc.same_bits(host(xd)[valid], got[valid]), (C, dt, two, "in place")
    assert max(worst) < 1.0, (C, dt, worst)
    log(f"rowwise op layernorm {dt} C {C} ({rc.ln_kernel(C, dt)})", worst)


@pytest.mark.parametrize("dt", rc.DTYPES)
@pytest.mark.parametrize("C", rc.LNG_C)
@pytest.mark.parametrize("G", rc.LNG_G)
def test_layernorm_groups(G, C, dt):
    """G LayerNorms side by side, in place, ld > G C: each group under the bound with its own gain;
    the gap columns and the rows past each length are left alone (the rows hold NaN before and after)."""
    x, gains, biases = rc.lng_inputs(G, C, dt)
    ref, bnd = rc.lng_reference(G, C, dt)
    rows, ld = x.shape
    valid = rc.ln_valid_rows()
    masked = np.setdiff1d(np.arange(rows), valid)
    xin = x.copy()
    xin[:, G * C:] = rc.SENTINEL
    xin[masked, :G * C] = NAN
    xd = dev(xin, dt)
    run(eng.layernorm_groups_op, dt, xd, rows, C, ld, [dev(g) for g in gains], [dev(b) for b in biases], eps=rc.EPS,
        lens=ints(rc.LN_LENS), stride=rc.LN_STRIDE)
    got = host(xd)
    assert (got[:, G * C:] == rc.SENTINEL).all(), (G, C, dt, "gap columns written")
    assert np.isnan(got[masked, :G * C]).all(), (G, C, dt, "rows past a length written")
    r = ratio(got[valid, :G * C].astype(np.float64), ref, bnd, (G, C, dt))
    assert r < 1.0, (G, C, dt, r)
    for b, L in enumerate(rc.LN_LENS):
        rs = slice(b * rc.LN_STRIDE, (b + 1) * rc.LN_STRIDE)
        xa = dev(xin[rs], dt)
        run(eng.layernorm_groups_op, dt, xa, rc.LN_STRIDE, C, ld, [dev(g) for g in gains], [dev(b_) for b_ in biases], eps=rc.EPS,
            lens=ints([L]), stride=rc.LN_STRIDE)
        assert rc.same_bits(host(xa)[:L], got[rs][:L]), (G, C, dt, b, "alone")
    log(f"rowwise op layernorm_groups {dt} G {G} C {C}", [r])


# -------------------------------------------------------------------------------------- refusals
def test_op_entries_refuse_what_the_kernels_do_not_take():
    """TTS_ERR_INVALID with a message, nothing launched: the output keeps its sentinel."""
    z = full((4096,), "f32")
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)

    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert "invalid argument" in str(ei.value)
        torch.cuda.synchronize()
        assert (host(z) == rc.SENTINEL).all(), (match, "something was launched")

    for k in rc.GLU_REFUSED_K:
        refused("kernel size", eng.glu_dwconv_op, "f32", z, zi, 1, 4, 8, z, k, z, z)
    refused("Tm, D > 0", eng.glu_dwconv_op, "f32", z, zi, 1, 0, 8, z, 7, z, z)
    refused("above the kernels' 512", eng.layernorm_op, "f32", z, z, 2, rc.LN_REFUSED_C, z, z)
    refused("row stride", eng.layernorm_op, "f32", z, z, 2, 8, z, z, lens=zi, stride=0)
    refused("rows, C > 0", eng.layernorm_op, "f32", z, z, 0, 8, z, z)
    refused("1 to 4 groups", eng.layernorm_groups_op, "f32", z, 2, 8, 64, [z] * rc.LNG_REFUSED["groups"], [z] * 5)
    refused("above the kernel's 256", eng.layernorm_groups_op, "f32", z, 2, rc.LNG_REFUSED["C"], 1024, [z], [z])
    refused("below groups", eng.layernorm_groups_op, "f32", z, 2, 8, 23, [z] * 3, [z] * 3)
    refused("row stride", eng.layernorm_groups_op, "f32", z, 2, 8, 8, [z], [z], lens=zi, stride=0)
    refused("not a multiple of H", eng.transpose_v_op, "f32", z, zi, 1, 4, 10, 3, 8, z)
    refused("Sk > 0", eng.transpose_v_op, "f32", z, zi, 1, 4, 8, 2, 0, z)
    refused("Sbd >= 2 Tm - 1", eng.rel_softmax_op, "f32", z, z, zi, 1, 2, 5, 16, 8, 16, 1.0, z)
    refused("Sbd >= 2 Tm - 1", eng.rel_softmax_op, "f32", z, z, zi, 1, 2, 5, 4, 16, 16, 1.0, z)
    refused("above Tcap", eng.regulate_op, "f32", "f32", z, 1, 4, 8, zi, 8, 9, 16, 1.0, z)
    refused("above Tcap", eng.regulate_op, "f32", "f32", z, 1, 4, 8, zi, 16, 9, 8, 1.0, z)
    for dt_in, dt in rc.REG_REFUSED:
        refused("dtype or fp32", eng.regulate_op, dt_in, dt, z, 1, 4, 8, zi, 16, 8, 16, 1.0, z)
    refused("N, Tm, V, D > 0", eng.embed_op, "f32", zi, zi, 1, 4, 4, z, 0, 8, 1.0, z)
    refused("rows, D > 0", eng.pos_bias_op, "f32", z, 4, 0, z, z, z, z)
    refused("rows, D > 0", eng.var_embed_add_op, "f32", z, 0, 8, z, z, z, z, z, z)
    refused("Tin, Tcap, C > 0", eng.mel_out_op, "f32", z, zi, 1, 0, 4, 8, z)
    refused("B, E, D > 0", eng.spk_bias_op, "f32", z, 1, 0, z, z, 8, z)
    refused("B, N, Tcap > 0", eng.durations_op, z, zi, 1, 4, 0, zi, zi, zi)
    refused("speed", eng.durations_op, z, zi, 1, 4, 8, zi, zi, zi, speed=0.0)
    refused("null buffer", eng.glu_dwconv_op, "f32", None, zi, 1, 4, 8, z, 7, z, z)
    with pytest.raises(KeyError):
        eng.pos_bias_op("f64", z, 4, 8, z, z, z, z)
    assert not zi.any().item()
