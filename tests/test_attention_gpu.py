"""The fused relative-position attention kernels (csrc/attention.hip) at op level, through
tts_op_rel_attn, against the float64 reference (oracle/attention.py) on the score patterns and
ragged shapes of attention_cases.py: the lazy online-softmax rescale, P across its whole range, the
relative-shift index map on a random table, both ends of the table, rows past each length, batch
invariance, the two-key-group and key-chunk forms.  Every bound comes from the reference alone
(attention_cases.bound; test_attention_cpu.py shows what the bounds reject).

Kernel forms per run: f16 / bf16 launch rel_attn_kernel (one key group; two under
TTS_ATTN_KSPLIT=1), "split" rel_attn_split_kernel, f32 rel_attn_f32_kernel -- in key chunks with
rel_attn_merge_kernel when the longest utterance exceeds the chunk (every batch here at the default
64), directly otherwise (the utterances run alone, and TTS_ATTN_F32_KC=0).

Measured errors land in $PARITY_LOG (profiles/attention_op_parity.json is that log from an MI355X
run).  The four-launch attention (rel_softmax) has no op entry: it runs through a whole fp32 model
on sharpened weights at the end of this file.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attention_cases as ac  # noqa: E402
from gonova_tts_amd import engine as eng  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda:0"
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "split": torch.float32}
KERNEL_DT = {"f16": "f16", "bf16": "bf16", "f32": "f32", "split": "f32"}
_OUT = {}   # (pattern, shape, form) -> the batch's output under the default switches


def _dev(a, form):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(TORCH[form]).contiguous()


def launch(form, pos_u, pos_v, table, utts, lens, Tm, Tp, rmax, with_ws=True):
    """One tts_op_rel_attn launch -> (out [B, Tp, H, dk] float64 with the sentinel wherever the
    kernel wrote nothing, range flag).  qkv rows past each length hold garbage."""
    B, H = len(lens), pos_u.shape[0]
    D = H * ac.DK
    qkv = np.full((B, Tp, 3 * D), ac.GARBAGE)
    for b, (q, k, v) in enumerate(utts):
        qkv[b, :lens[b]] = np.concatenate([q.reshape(-1, D), k.reshape(-1, D), v.reshape(-1, D)], 1)
    out = torch.full((B, Tp, D), ac.SENTINEL, dtype=TORCH[form], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    nws = eng.rel_attn_ws_bytes(B, Tm, Tp, D, H) if form == "f32" and with_ws else 0
    ws = torch.empty(nws // 4, dtype=torch.float32, device=DEV) if nws else None
    try:
        eng.rel_attn_op(KERNEL_DT[form], torch.from_numpy(pos_u).to(DEV), torch.from_numpy(pos_v).to(DEV), _dev(qkv, form),
                        _dev(table.reshape(2 * rmax, D), form), torch.tensor(lens, dtype=torch.int32, device=DEV), Tm, rmax,
                        ac.SCALE, out, split=form == "split", range_flag=flag, ws=ws)
        torch.cuda.synchronize()
        return out.float().cpu().numpy().astype(np.float64).reshape(B, Tp, H, ac.DK), int(flag.item())
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error, nothing more is started on the GPU: {e}", returncode=3)
        raise


def run_case(pattern, shape, form, cache=True):
    key = (pattern, shape, form)
    if not cache or key not in _OUT:
        c = ac.case_inputs(pattern, shape, form)
        r = launch(form, c["pos_u"], c["pos_v"], c["table"], c["utts"], c["lens"], c["Tm"], c["Tp"], c["rmax"])
        if not cache:
            return r
        _OUT[key] = r
    return _OUT[key]


def check_case(tag, pattern, shape, form, out):
    """Every utterance under the case's bound in both metrics; everything past each length (the
    empty utterance and the pad rows included) as the header says: never written."""
    c, refs, bnd = ac.case_inputs(pattern, shape, form), ac.reference(pattern, shape, form), ac.bound(pattern, shape, form)
    for b, L in enumerate(c["lens"]):
        assert (out[b, L:] == ac.SENTINEL).all(), (tag, pattern, shape, form, b, "rows past the length were written")
    for b, L in enumerate(c["lens"]):
        if L:
            check(f"attn op {tag} {pattern} {shape} {form} b={b} ({L} keys)", out[b, :L], refs[b],
                  rel_rms_tol=bnd[0], max_abs_tol=bnd[1])


FORMS = list(ac.DTYPES)
PATTERN_FORM = [(p, f) for p in ac.PATTERNS for f in FORMS]


@pytest.mark.parametrize("pattern,form", PATTERN_FORM)
def test_parity(pattern, form):
    """Every pattern x form x shape against float64 under the reference's own bound.  H = 3 (shape
    b3) is the regression case of the key-chunk merge, which wrote only the first 384 channels."""
    for shape in ac.SHAPES:
        out, flag = run_case(pattern, shape, form)
        check_case("default", pattern, shape, form, out)
        assert flag == 0, (pattern, shape, form, "range flag raised on in-range operands")


def test_range_flag_raised_past_f16_range():
    """The split form holds each operand as two f16 halves: a k past f16's range (|x| >= 65520)
    raises the range word, as tts_acoustic_range_flag documents; the other forms never touch it."""
    c = ac.case_inputs("flat", "b3", "split")
    utts = [tuple(np.array(a) for a in u) for u in c["utts"]]
    utts[2][1][100, 1, 7] = 7.0e4
    for form, want in (("split", 1), ("f32", 0)):
        _, flag = launch(form, c["pos_u"], c["pos_v"], c["table"], utts, c["lens"], c["Tm"], c["Tp"], c["rmax"])
        assert flag == want, form


@pytest.mark.parametrize("pattern,form", PATTERN_FORM)
def test_batch_invariance(pattern, form):
    """Each utterance run alone -- B = 1, Tm = Tp = rmax = its own length, so another grid, another
    table offset and, in fp32, the direct form below the key chunk -- equals the same utterance
    inside its ragged batch bit for bit."""
    for shape in ac.SHAPES:
        c = ac.case_inputs(pattern, shape, form)
        batch, _ = run_case(pattern, shape, form)
        for b, L in enumerate(c["lens"]):
            if L:
                alone, _ = launch(form, c["pos_u"], c["pos_v"], ac.table(pattern, c["H"], L, form), [c["utts"][b]], (L,), L, L, L)
                assert np.array_equal(alone[0], batch[b, :L]), (pattern, shape, form, b, L)


@pytest.mark.parametrize("form", ["f16", "bf16"])
@pytest.mark.parametrize("pattern", ["ramp", "sharp"])
def test_two_key_groups(pattern, form, switch):
    """TTS_ATTN_KSPLIT=1: the block's keys in two groups merged through LDS, each with its own lazy
    reference max.  The second group holds keys from ceil(len / 64) * 32 on: empty up to 32 keys,
    partial at 33 and 63, whole steps at 64 and 128, several steps with a partial last at 200.  Under
    the same bound as the one-group kernel."""
    switch("TTS_ATTN_KSPLIT", 1)
    for shape in ac.SHAPES:
        out, _ = run_case(pattern, shape, form, cache=False)
        check_case("ksplit", pattern, shape, form, out)


@pytest.mark.parametrize("pattern", ["ramp", "sharp"])
def test_f32_key_chunks(pattern, switch):
    """fp32 key chunks of TTS_ATTN_F32_KC = 0 (off), 32, the default (64) and 96 keys: every
    utterance under the bound, and an utterance that fits one chunk bit-identical to the direct
    form (its merge multiplies by 2^0), as the kernel's header claims."""
    switch("TTS_ATTN_F32_KC", 0)
    direct = {shape: run_case(pattern, shape, "f32", cache=False)[0] for shape in ac.SHAPES}
    for shape in ac.SHAPES:
        check_case("kc=0", pattern, shape, "f32", direct[shape])
    for kc, keys in ((32, 32), (None, 64), (96, 96)):
        switch("TTS_ATTN_F32_KC", kc)
        for shape in ac.SHAPES:
            lens = ac.SHAPES[shape][0]
            out, _ = run_case(pattern, shape, "f32", cache=False)
            check_case(f"kc={keys}", pattern, shape, "f32", out)
            for b, L in enumerate(lens):
                if 0 < L <= keys:
                    assert np.array_equal(out[b, :L], direct[shape][b, :L]), (pattern, shape, kc, b, L)


def test_op_entry_refuses_what_the_kernels_do_not_take():
    """TTS_ERR_INVALID with a message, nothing launched."""
    def call(dtype, H, dk, Tm, Tp, rmax, split=False):
        z = lambda *s: torch.zeros(s, dtype=TORCH[dtype], device=DEV)
        pos = torch.zeros((H, dk), device=DEV)
        eng.rel_attn_op(dtype, pos, pos, z(1, Tp, 3 * H * dk), z(2 * rmax, H * dk),
                        torch.zeros(1, dtype=torch.int32, device=DEV), Tm, rmax, 1.0, z(1, Tp, H * dk), split=split)

    with pytest.raises(RuntimeError, match="below Tm"):
        call("f16", 1, 192, 16, 16, 8)
    with pytest.raises(RuntimeError, match="Tm <= Tp"):
        call("f16", 1, 192, 16, 8, 16)
    with pytest.raises(RuntimeError, match="split form takes fp32"):
        call("f16", 1, 192, 8, 8, 8, split=True)
    with pytest.raises(RuntimeError, match="head size"):
        call("f32", 2, 64, 8, 8, 8)
    call("f32", 2, 192, 8, 8, 8)   # (lens = 0: launches and writes nothing)
    torch.cuda.synchronize()


# ------------------------------------------------------- the four-launch path, through a whole model
@pytest.mark.parametrize("rel_attn", [1, 0])
@pytest.mark.parametrize("name", list(ac.SHARPEN))
def test_sharpened_model_fp32(name, rel_attn, switch):
    """rel_softmax (head sizes other than 192, and 192 under TTS_REL_ATTN=0) on sharper scores:
    acoustic_cases' ragged batch, durations forced, fp32, linear_q / linear_k scaled by
    attention_cases.SHARPEN, against acoustic_forward in float64 at the project's fp32 bar."""
    import acoustic_cases as acs
    switch("TTS_REL_ATTN", rel_attn)
    e = eng.HipEngine(DEV, vocoder_dtype="f32", acoustic_dtype="f32")
    try:
        e.load_weights(acoustic=ac.sharpened_weights(name))
        ids, durs = acs.ragged_inputs(name)
        B, N = len(ids), max(len(x) for x in ids)
        tok, dur = np.zeros((B, N), np.int32), np.zeros((B, N), np.int32)
        for b, (x, d) in enumerate(zip(ids, durs)):
            tok[b, :len(x)], dur[b, :len(x)] = x, d
        try:
            mel, mel_lens = e.acoustic(torch.from_numpy(tok).to(DEV), torch.tensor([len(x) for x in ids], dtype=torch.int32),
                                       acs.T_CAP, durations=torch.from_numpy(dur).to(DEV))
            torch.cuda.synchronize()
        except RuntimeError as err:
            if "HIP error" in str(err) or "illegal memory access" in str(err):
                pytest.exit(f"device error, nothing more is started on the GPU: {err}", returncode=3)
            raise
        mel, mel_lens = mel.cpu().numpy(), mel_lens.cpu().numpy()
    finally:
        e.close()
    refs = ac.sharpened_oracle(name)
    for b, r in enumerate(refs):   # logged first (no bound of its own), then held to the fp32 bar
        L = r.shape[0]
        assert int(mel_lens[b]) == L
        check(f"attn model {name} x{ac.SHARPEN[name]} TTS_REL_ATTN={rel_attn} f32 b={b} ({L} frames)", mel[b, :L], r)
    for b, r in enumerate(refs):
        np.testing.assert_allclose(mel[b, :r.shape[0]], r, atol=ac.FP32_ATOL, rtol=ac.FP32_RTOL, err_msg=f"{name} b={b}")
