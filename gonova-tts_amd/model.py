"""Drop-in model for the reference's synthesis call site.

The reference constructs its model with `ChatterboxTTS.from_pretrained(device=...)`
(`services/tts/core/synthesizer.py:185`) and calls
`model.generate(text, audio_prompt_path=..., exaggeration=..., cfg_weight=0.5,
temperature=0.8)` (`synthesizer.py:344-350`), then `audio.squeeze().cpu().numpy()`
and a float32 cast (`:352-357`).  `GonovaTTS` keeps exactly that duck-typed surface
 and adds `generate_batch` for many sentences at once.

Semantics of the extra arguments: the FastSpeech2 + HiFi-GAN pipeline is
deterministic and has no voice cloning, so `cfg_weight` and `temperature` are accepted
and ignored, and `audio_prompt_path` only selects a stored speaker embedding (the
reference forwards a possibly unsanitised path, `voice_manager.py:166-177`; an audio
prompt is never opened here).  `exaggeration` sets the range of the predicted pitch and
energy contours (0.5 neutral), and `speed`, `pitch` and `energy` are this model's own
prosody controls (prosody.py), applied per utterance on the device.
Output rate is `self.sr` = 22,050 Hz (the reference hard-codes 24 kHz,
`synthesizer.py:119`).
"""
from __future__ import annotations

import os
import threading
from contextlib import contextmanager, nullcontext
from math import gcd
from typing import Dict, List, Optional

import numpy as np

from .config import AcousticConfig, VocoderConfig, SAMPLE_RATE, vocoder_context_frames
from .engine import HipEngine, PROSODY_NEUTRAL, pack_prosody, resample_chunk_counts, resample_history
from .prosody import prosody_controls  # noqa: F401  (public here too)
from .text import tokenize_batch
from .weights import make_acoustic_weights, make_vocoder_weights


def fold_weight_norm(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Fold weight-normalised convolutions into plain weights.

    HiFi-GAN checkpoints are often saved with torch weight norm on (HF's
    `apply_weight_norm`): `<name>.weight_g` / `<name>.weight_v` (torch.nn.utils.weight_norm)
    or `<name>.parametrizations.weight.original0` / `.original1` (the parametrization API).
    Both store w = g * v / ||v|| with the norm over every dim but 0 (torch's default
    dim=0, which HF uses for Conv1d and ConvTranspose1d alike); the result is written
    as `<name>.weight` and the g/v entries are dropped."""
    out = dict(sd)
    pairs = []
    for k in sd:
        if k.endswith(".weight_g"):
            pairs.append((k[: -len(".weight_g")], k, k[:-1] + "v"))
        elif k.endswith(".parametrizations.weight.original0"):
            base = k[: -len(".parametrizations.weight.original0")]
            pairs.append((base, k, k[:-1] + "1"))
    for base, kg, kv in pairs:
        if kv not in sd:
            raise ValueError(f"weight norm: {kg} without {kv}")
        g = np.asarray(sd[kg], np.float64)
        v = np.asarray(sd[kv], np.float64)
        norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape((-1,) + (1,) * (v.ndim - 1))
        out[base + ".weight"] = (g.reshape(norm.shape) * v / norm).astype(np.float32)
        del out[kg], out[kv]
    return out


def load_state_dict(path: str) -> Dict[str, np.ndarray]:
    """Load a local checkpoint without executing code from it (safetensors / npz); weight-norm
    pairs are folded (fold_weight_norm)."""
    if path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return fold_weight_norm({k: np.asarray(v, np.float32) for k, v in load_file(path).items()})
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return fold_weight_norm({k: z[k].astype(np.float32) for k in z.files})
    raise ValueError(f"unsupported checkpoint format: {path}")


class GonovaTTS:
    """FastSpeech2-Conformer + HiFi-GAN V1 on MI355X (HIP kernels via libtts_hip.so)."""

    FRAMES_PER_TOKEN_CAP = 12  # first-pass frame budget per token; exact retry if exceeded

    def __init__(self, engine: HipEngine, acoustic_cfg: AcousticConfig, vocoder_cfg: VocoderConfig,
                 sample_rate: Optional[int] = None):
        self.engine = engine
        self.acoustic_cfg = acoustic_cfg
        self.vocoder_cfg = vocoder_cfg
        # the generator's receptive field in mel frames (per side): what a streaming window carries
        self.receptive_field = max(vocoder_context_frames(vocoder_cfg))
        # output rate: the vocoder's 22,050 Hz, or e.g. 24,000 for clients that assume the
        # reference's hard-coded rate (synthesizer.py:119); converted on the device
        # (tts_resample_poly, scipy.signal.resample_poly semantics)
        self.native_sr = SAMPLE_RATE
        self.sr = int(sample_rate) if sample_rate else SAMPLE_RATE
        self.device = f"cuda:{engine.device_index}"
        self._lock = threading.Lock()

    @classmethod
    def from_pretrained(cls, device: str = "cuda", ckpt_dir: Optional[str] = None, seed: int = 0,
                        vocoder_dtype: str = "f16", acoustic_dtype: str = "bf16", fixed_duration: Optional[int] = None,
                        max_batch: int = 0, max_frames: int = 0, max_tokens: int = 0,
                        sample_rate: Optional[int] = None, speaker_embed_dim: Optional[int] = None,
                        encoder_precision: str = "exact"):
        """Mirror of `ChatterboxTTS.from_pretrained(device=...)` (synthesizer.py:185).

        ckpt_dir: optional directory with `acoustic.safetensors` and `vocoder.safetensors`
        (HF state_dict names); without it the deterministic seeded weights are used
        (no checkpoint is reachable offline).  sample_rate: output rate (default 22,050 Hz;
        24,000 reproduces the rate the reference's clients assume).  speaker_embed_dim: seeded
        multi-speaker weights with a speaker-embedding projection of that size (a checkpoint
        carrying `projection.weight` sets it by itself).  encoder_precision: "exact" (default: the
        encoder and variance predictors keep fp32 activations, so predicted integer durations match
        fp32, HF:181-183) or "fast" (all of the acoustic model in acoustic_dtype)."""
        acfg, vcfg = AcousticConfig(speaker_embed_dim=speaker_embed_dim), VocoderConfig()
        if ckpt_dir:
            aw = load_state_dict(os.path.join(ckpt_dir, "acoustic.safetensors"))
            vw = load_state_dict(os.path.join(ckpt_dir, "vocoder.safetensors"))
            if "projection.weight" in aw:  # multi-speaker checkpoint (HF speaker_embed_dim)
                acfg.speaker_embed_dim = aw["projection.weight"].shape[1] - aw["projection.weight"].shape[0]
        else:
            aw = make_acoustic_weights(seed, acfg, fixed_duration=fixed_duration)
            vw = make_vocoder_weights(seed, vcfg)
        eng = HipEngine(device, vocoder_dtype=vocoder_dtype, acoustic_dtype=acoustic_dtype,
                        max_batch=max_batch, max_frames=max_frames, max_tokens=max_tokens,
                        encoder_precision=encoder_precision)
        eng.load_weights(vocoder=vw, acoustic=aw, vocoder_cfg=vcfg)
        return cls(eng, acfg, vcfg, sample_rate=sample_rate)

    # -------------------------------------------------------------- synthesis
    def _controls(self, prosody, B: int, lens, durations):
        """A call's `prosody` (engine.pack_prosody's forms) -> (float32 [5, B] block or None when
        all neutral, durations, largest duration_scale).  Given durations are scaled here, on the
        host, with the kernel's float32 rint, and go down with a neutral scale: the host then knows
        the frame counts (_mel_lens_host) exactly as the device computes them."""
        ctl = pack_prosody(prosody, B)
        if ctl is None:
            return None, durations, 1.0
        smax = float(ctl[0].max()) if B else 1.0
        if durations is not None:
            durations = scale_durations(durations, ctl[0])
            ctl = ctl.copy()
            ctl[0] = 1.0
            smax = 1.0
            if (ctl == np.asarray(PROSODY_NEUTRAL, np.float32)[:, None]).all():
                ctl = None
        return ctl, durations, smax

    def _frame_budget(self, N: int, smax: float = 1.0) -> int:
        """First-pass frame budget with predicted durations: 12 frames per token, times the
        batch's largest duration_scale when that is above 1 (exact retry if exceeded)."""
        return max(64, int(np.ceil(self.FRAMES_PER_TOKEN_CAP * N * max(1.0, smax))))

    def synthesize_tokens(self, tokens: np.ndarray, lens: np.ndarray, durations: Optional[np.ndarray] = None,
                          stream=None, speaker_embedding: Optional[np.ndarray] = None, host_lens: bool = True,
                          prosody=None):
        """tokens int32 [B, N], lens [B] -> (wav cuda float32 [B, T*hop], wav_lens np.int64 [B]).
        host_lens=False makes no host sync, so a caller can queue several batches back to back
        (dist.ShardedSynthesis), and returns (wav, wav_lens cuda int64 [B], pending): `pending` is
        None when nothing is left to check, else a PendingRange whose `word` the caller reads with
        the lengths at its own sync and whose `resolve(...)` reruns the batch when it is set.

        Range guard (include/tts_hip.h, ABI 4): with the exact encoder of a 16-bit model the
        acoustic forward's range word travels with the one host read this path makes anyway; when a
        split-precision operand was outside f16's range the batch is synthesized again with the
        encoder on the exact fp32 MFMA kernels (`range_fallbacks` counts these); the rerun keeps the
        controls.

        prosody: per-utterance controls in any of engine.pack_prosody's forms (None: neutral);
        a bad value raises ValueError before any GPU work."""
        import torch
        dev = self.engine.torch_device
        B, N = tokens.shape
        ctl, durations, smax = self._controls(prosody, B, lens, durations)
        tok, tl, dd, cb = _upload_i32((tokens, lens, durations, _as_i32(ctl)), dev, stream)
        cb = None if cb is None else cb.view(torch.float32)
        t_cap = self._frame_budget(N, smax)
        if durations is not None:
            t_cap = max(1, int(np.asarray(durations).sum(axis=1).max()))
        args = (tok, tl, dd, t_cap, stream, speaker_embedding, host_lens, cb)
        # the engine's device is the current one for this thread (the streams torch hands out, the
        # ops below): an executor thread of a multi-GPU service starts on device 0
        with torch.cuda.device(self.engine.device_index):
            wav, wav_lens, tripped = self._synthesize_once(*args)
            if tripped is True:  # read on the host already (predicted durations)
                with self._range_fallback():
                    wav, wav_lens, _ = self._synthesize_once(*args)
                tripped = None
            if not host_lens:  # tripped: the unread range word (device) or None; the caller reads it
                pend = PendingRange(self, args[:6] + (True, cb), tripped) if isinstance(tripped, torch.Tensor) else None
                return wav, wav_lens, pend
        return wav, wav_lens

    @property
    def range_fallbacks(self) -> int:
        """Forwards rerun on the fp32 encoder because the exact encoder's range guard tripped."""
        return self.engine.range_fallbacks

    @contextmanager
    def _range_fallback(self):
        import warnings
        self.engine.range_fallbacks += 1
        warnings.warn("acoustic encoder activations outside the f16 range of the split-precision GEMMs: "
                      "rerunning this batch with the encoder on fp32 MFMA (include/tts_hip.h, TTS_ENCODER_F32)",
                      RuntimeWarning, stacklevel=3)
        with self.engine.encoder_f32():
            yield

    def _synthesize_once(self, tok, tl, dd, t_cap, stream, spk, host_lens, ctl=None):
        """-> (wav, wav_lens, range guard tripped: bool, or None when nothing was read); with
        host_lens=False the third item is the forward's range word itself (cuda int32 [1], None
        without the guard), unread.  ctl: the controls' device block (cuda float32 [5, B]) or None"""
        import torch
        mel, mel_lens, dur, rw = self.engine.acoustic(tok, tl, t_cap, durations=dd, stream=stream,
                                                      return_durations=True, speaker_embedding=spk, return_range=True,
                                                      prosody=ctl)
        lens_known = None
        tripped = None
        if dd is None:
            # one host read for the frames the durations need, the frame counts and the range word
            need, lens_known, tripped = _need_and_lens(dur, mel_lens, rw)
            if tripped:
                return None, None, True
            if need > t_cap:  # exact second pass with the predicted durations and a fitting cap
                # (they are scaled already: the second pass runs with a neutral duration_scale)
                mel, mel_lens, dur, rw = self.engine.acoustic(tok, tl, need, durations=dur, stream=stream,
                                                              return_durations=True, speaker_embedding=spk,
                                                              return_range=True, prosody=_unit_scale(ctl))
                need, lens_known, tripped = _need_and_lens(dur, mel_lens, rw)
                if tripped:
                    return None, None, True
            # the vocoder (and the waveform the caller copies to the host) at the frames the
            # durations give, not the 12-per-token budget: half the grid and the bytes at C3's 6
            T_act = max(1, int(lens_known.max())) if len(lens_known) else 1
            if T_act < mel.shape[1] and os.environ.get("TTS_VOC_TRIM", "1") != "0":  # (0: A/B runs)
                mel = mel[:, :T_act].contiguous()
        wav = self.engine.vocoder(mel, mel_lens, stream=stream)
        if self.sr != self.native_sr:
            g = gcd(self.sr, self.native_sr)
            wav, out_lens = self.engine.resample(wav, mel_lens * self.vocoder_cfg.hop, self.sr // g,
                                                 self.native_sr // g, stream=stream)
            out_lens = out_lens.to(torch.int64)
            if not host_lens:
                return wav, out_lens, rw if tripped is None else None
            if tripped is None:
                h, tripped = _read_with_range(out_lens, rw)
                return wav, h, tripped
            return wav, out_lens.cpu().numpy(), tripped
        if host_lens and lens_known is not None:  # already on the host: no second sync
            return wav, lens_known * self.vocoder_cfg.hop, tripped
        wav_lens = mel_lens.to(torch.int64) * self.vocoder_cfg.hop
        if not host_lens:
            return wav, wav_lens, rw if tripped is None else None
        h, tripped = _read_with_range(wav_lens, rw)
        return wav, h, tripped

    # -------------------------------------------------------------- streaming
    # fewest mel frames of context per side; HiFi-GAN V1's receptive field is exactly 13 frames
    # (config.vocoder_context_frames).  A generator with a smaller hop needs more: stream_context.
    STREAM_CONTEXT = 16

    @property
    def stream_context(self) -> int:
        """Mel frames of context per side the streaming windows carry: the loaded generator's
        receptive field (config.vocoder_context_frames; the engine derives the same pair from its
        packed layers, HipEngine.vocoder_context), never fewer than STREAM_CONTEXT -- 16 for V1."""
        return max(self.STREAM_CONTEXT, self.receptive_field)

    def _context(self, context: Optional[int]) -> int:
        """The context a stream runs with: stream_context, or the caller's when it covers the
        receptive field (below it every chunk edge would carry a seam: ValueError)."""
        if context is None:
            return self.stream_context
        rf = self.receptive_field
        if int(context) < rf:
            raise ValueError(f"stream context of {int(context)} frames is below the vocoder's receptive field "
                             f"of {rf} frames")
        return int(context)

    streams_resampled = True  # stream_tokens(output_rate=...) / stream_batch cut a resampled stream too

    def stream_tokens(self, tokens: np.ndarray, lens: np.ndarray, chunk_frames: int = 32,
                      context: Optional[int] = None, durations: Optional[np.ndarray] = None, stream=None,
                      speaker_embedding: Optional[np.ndarray] = None, output_rate: Optional[int] = None,
                      prosody=None):
        """Sub-sentence streaming: one acoustic pass, then the vocoder
        runs on windows [c0 - ctx, c0 + chunk + ctx) and keeps the middle `chunk` frames.
        With ctx >= the receptive field every kept sample is computed from the same inputs
        in the same order as the full-utterance pass, so the concatenated chunks equal it.

        context None: stream_context, the loaded generator's receptive field (at least
        STREAM_CONTEXT); a given context below the receptive field raises ValueError before any
        GPU work.

        Yields (c0, wav_chunk cuda float32 [B, chunk*hop], valid samples per utterance np [B]).
        output_rate None (or the vocoder's 22,050 Hz, whatever `sr` is): native chunks.  Another
        rate: every chunk goes through the chunked resampler (tts_resample_poly_chunk), which
        carries the filter's history between chunks; wav_chunk is then [B, cap] at that rate with
        cap = ceil(chunk*hop*up/down) + n_flush, and the valid counts differ from chunk to chunk
        (an utterance's last chunk also brings the outputs held back until its end is known).  The
        valid parts concatenate to synthesize_tokens' output at that rate, bit for bit.
        prosody: as synthesize_tokens'; with the same controls the two agree bit for bit."""
        import torch
        context = self._context(context)
        with torch.cuda.device(self.engine.device_index):  # (see synthesize_tokens)
            for c0, wav, valid, _ in self._stream_tokens(tokens, lens, chunk_frames, context, durations, stream,
                                                         speaker_embedding, output_rate, prosody):
                yield c0, wav, valid

    def _stream_tokens(self, tokens, lens, chunk_frames, context, durations, stream, speaker_embedding,
                       output_rate=None, prosody=None):
        """stream_tokens' generator; yields a fourth item, ended np bool [B]: the utterance has no
        frame past this chunk."""
        import torch
        ctx = self._context(context)
        dev = self.engine.torch_device
        B, N = tokens.shape
        hop = self.vocoder_cfg.hop
        rs = None
        if output_rate and int(output_rate) != self.native_sr:
            rs = _ChunkResampler(self.engine, B, int(output_rate), self.native_sr, hop, chunk_frames, dev, stream)
        ctl, durations, smax = self._controls(prosody, B, lens, durations)
        tok, tl, dd, cb = _upload_i32((tokens, lens, durations, _as_i32(ctl)), dev, stream)
        cb = None if cb is None else cb.view(torch.float32)
        t_cap = self._frame_budget(N, smax) if durations is None else \
            max(1, int(np.asarray(durations).sum(axis=1).max()))
        spk = speaker_embedding
        mel, mel_lens, dur, rw = self.engine.acoustic(tok, tl, t_cap, durations=dd, stream=stream, return_durations=True,
                                                      speaker_embedding=spk, return_range=True, prosody=cb)
        first = None  # (window end, kept frames, chunk) enqueued ahead of the host read
        if durations is None:
            # The first chunk's window needs no host value when the longest utterance covers it
            # (frames >= chunk + ctx, the usual case): enqueue it before the one host read of the
            # frame counts, so the GPU runs it instead of idling through the round trip.  It is
            # used only if the loop below would make exactly the same call (else recomputed).
            # The read's copies are enqueued before the chunk and waited for by event, so the host
            # has the frame counts while the chunk still runs and hands the chunk over when it is
            # enqueued (a read after the chunk held the host until the chunk ended, then cost a
            # second round trip for the waveform: ~0.15 ms of C5, profiles/r06m/).
            w1 = min(t_cap, chunk_frames + ctx)
            tc = min(chunk_frames, t_cap)
            early = os.environ.get("TTS_STREAM_EARLY", "1") != "0"  # (0: the host read first, A/B runs)
            rd = _HostRead(dur, mel_lens, rw, stream)
            if early:
                win_lens = torch.clamp(mel_lens, min=0, max=w1).to(torch.int32)
                wav = self.engine.vocoder_chunk(mel[:, :w1].contiguous(), win_lens, 0, tc, stream=stream)
                if rs is not None:  # its resample ahead of the read too (discarded with it: chunk 0
                    wav = rs.run(wav, 0, mel_lens)  # starts the history anew)
                first = (w1, tc, wav)
            need, lens_h, tripped = rd.result()  # one host read before the first chunk is handed over
            fell_back = False
            if tripped:  # range guard: the acoustic pass again on the fp32 encoder
                first, fell_back = None, True
                with self._range_fallback():
                    mel, mel_lens, dur = self.engine.acoustic(tok, tl, t_cap, durations=None, stream=stream,
                                                              return_durations=True, speaker_embedding=spk, prosody=cb)
                need, lens_h, _ = _need_and_lens(dur, mel_lens)
            if need > t_cap:
                first = None
                # after a fallback the second pass stays on the fp32 encoder: its activations do not
                # depend on the durations, so the split encoder would overflow again
                with (self.engine.encoder_f32() if fell_back else nullcontext()):
                    # (dur is scaled already: a neutral duration_scale from here on)
                    mel, mel_lens, dur, rw = self.engine.acoustic(tok, tl, need, durations=dur, stream=stream,
                                                                  return_durations=True, speaker_embedding=spk,
                                                                  return_range=True, prosody=_unit_scale(cb))
                need, lens_h, tripped = _need_and_lens(dur, mel_lens, rw)
                if tripped and not fell_back:
                    with self._range_fallback():
                        mel, mel_lens, dur = self.engine.acoustic(tok, tl, need, durations=dur, stream=stream,
                                                                  return_durations=True, speaker_embedding=spk,
                                                                  prosody=_unit_scale(cb))
                    need, lens_h, _ = _need_and_lens(dur, mel_lens)
        else:
            # given durations fix the frame counts on the host: no device sync between the
            # acoustic pass and the first chunk's vocoder launches (same-box C5: neutral, the
            # host enqueues faster than the GPU drains either way)
            lens_h = _mel_lens_host(lens, durations, t_cap)
        T = int(lens_h.max()) if B else 0
        for c0 in range(0, T, chunk_frames):
            tc = min(chunk_frames, T - c0)
            w0 = max(0, c0 - ctx)
            w1 = min(T, c0 + tc + ctx)
            if c0 == 0 and first is not None and first[:2] == (w1, tc):
                wav = first[2]
            else:
                win = mel[:, w0:w1].contiguous()
                win_lens = torch.clamp(mel_lens - w0, min=0, max=w1 - w0).to(torch.int32)
                wav = self.engine.vocoder_chunk(win, win_lens, c0 - w0, tc, stream=stream)
                if rs is not None:
                    wav = rs.run(wav, c0, mel_lens)
            if c0 == 0 and durations is not None and rw is not None:
                # given durations made no host read so far: the range word is read here, where the
                # consumer would wait for this chunk anyway; out of range -> fp32 encoder, chunk again
                if int(rw.item()) != 0:
                    with self._range_fallback():
                        mel, mel_lens = self.engine.acoustic(tok, tl, t_cap, durations=dd, stream=stream,
                                                             speaker_embedding=spk, prosody=cb)
                    win = mel[:, w0:w1].contiguous()
                    win_lens = torch.clamp(mel_lens - w0, min=0, max=w1 - w0).to(torch.int32)
                    wav = self.engine.vocoder_chunk(win, win_lens, c0 - w0, tc, stream=stream)
                    if rs is not None:  # (chunk 0 again: the history starts anew)
                        wav = rs.run(wav, c0, mel_lens)
            first = None
            if rs is not None:
                valid = rs.counts(lens_h, c0, tc)
            else:
                valid = np.clip(lens_h - c0, 0, tc) * hop
            yield c0, wav, valid, lens_h <= c0 + tc

    def _voice_groups(self, n: int, speaker_embeddings):
        """Sentence index groups that share one engine pass: on a multi-speaker model the
        sentences with and without a voice run as two batches (HF skips the projection when no
        embedding is given, HF:1192)."""
        if not self.acoustic_cfg.speaker_embed_dim or speaker_embeddings is None or \
                all(e is None for e in speaker_embeddings):
            return [(list(range(n)), None)]
        with_v = [i for i, e in enumerate(speaker_embeddings) if e is not None]
        without = [i for i, e in enumerate(speaker_embeddings) if e is None]
        groups = [(with_v, np.stack([np.asarray(speaker_embeddings[i], np.float32).reshape(-1) for i in with_v]))]
        if without:
            groups.append((without, None))
        return groups

    def stream_batch(self, texts: List[str], chunk_frames: int = 32,
                     speaker_embeddings: Optional[List[Optional[np.ndarray]]] = None,
                     prosody: Optional[List[Optional[dict]]] = None):
        """Sub-sentence streaming of many sentences in one batched pass (the service's opt-in
        `stream_frames` mode): yields, per vocoder chunk, a list of (sentence index, float32
        samples of that chunk, sentence finished).  A sentence's pieces concatenate to the
        stream_tokens output, which equals the full pass (stream_tokens) -- at `sr`: with an
        output rate other than the vocoder's the chunks come through the chunked resampler
        (stream_tokens(output_rate=sr)) and the pieces concatenate to generate_batch's audio at
        that rate, bit for bit; their lengths then differ from chunk to chunk.
        prosody: optional per-sentence controls (None entries: neutral), as generate_batch's."""
        if not texts:
            return
        _check_per_sentence(prosody, len(texts))
        import torch
        with self._lock, torch.cuda.device(self.engine.device_index):
            for idx, spk in self._voice_groups(len(texts), speaker_embeddings):
                tokens, lens = tokenize_batch([texts[i] for i in idx])
                done = [False] * len(idx)
                for c0, wav, valid, ended in self._stream_tokens(tokens, lens, chunk_frames, None, None, None, spk,
                                                                 self.sr, _pick(prosody, idx)):
                    host = _to_host(wav)
                    out = []
                    for r, i in enumerate(idx):
                        if done[r]:
                            continue
                        # (the piece's length says nothing at a resampled rate: the sentence is
                        # finished with the chunk that holds its last frame)
                        done[r] = bool(ended[r])
                        out.append((i, host[r, :int(valid[r])].astype(np.float32, copy=False), done[r]))
                    yield out
                last = [(i, np.zeros(0, np.float32), True) for r, i in enumerate(idx) if not done[r]]
                if last:  # sentences without a frame
                    yield last

    def generate_batch(self, texts: List[str], speaker_embeddings: Optional[List[Optional[np.ndarray]]] = None,
                       prosody: Optional[List[Optional[dict]]] = None, **_ignored) -> List[np.ndarray]:
        """Synthesize many sentences in one batched pass -> list of float32 waveforms.
        speaker_embeddings: optional per-sentence voice vectors (None entries: no voice).
        prosody: optional per-sentence controls, each None (neutral) or a dict of
        engine.PROSODY_FIELDS scalars (prosody_controls builds one from speed / pitch / energy /
        exaggeration); sentences with different controls share the one pass."""
        if not texts:
            return []
        _check_per_sentence(prosody, len(texts))
        groups = self._voice_groups(len(texts), speaker_embeddings)
        out: List[Optional[np.ndarray]] = [None] * len(texts)
        with self._lock:
            for idx, spk in groups:
                tokens, lens = tokenize_batch([texts[i] for i in idx])
                wav, wav_lens = self.synthesize_tokens(tokens, lens, speaker_embedding=spk,
                                                       prosody=_pick(prosody, idx))
                host = _to_host(wav)
                for r, i in enumerate(idx):
                    out[i] = host[r, : int(wav_lens[r])].astype(np.float32, copy=False)
        return out

    def speaker_embedding(self, audio_prompt_path: Optional[str]) -> Optional[np.ndarray]:
        """The voice for `audio_prompt_path` (the reference's voice_id -> path,
        server.py:127-138): a stored speaker embedding (.npy / .npz / .safetensors, one vector of
        speaker_embed_dim values, loaded without executing anything from the file) when the
        model has a speaker projection; None otherwise.  Audio prompts (.wav) carry no
        embedding here -- the speaker encoder that would compute one is not part of this
        engine -- and are ignored, as before."""
        if not audio_prompt_path or not self.acoustic_cfg.speaker_embed_dim:
            return None
        path = str(audio_prompt_path)
        if path.endswith(".npy"):
            v = np.load(path, allow_pickle=False)
        elif path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                v = z["embedding"] if "embedding" in z.files else z[z.files[0]]
        elif path.endswith(".safetensors"):
            from safetensors.numpy import load_file
            d = load_file(path)
            v = d["embedding"] if "embedding" in d else next(iter(d.values()))
        else:
            return None
        v = np.asarray(v, np.float32).reshape(-1)
        if v.size != self.acoustic_cfg.speaker_embed_dim:
            raise ValueError(f"speaker embedding {path}: {v.size} values, model expects "
                             f"{self.acoustic_cfg.speaker_embed_dim}")
        return v

    def generate(self, text: str, audio_prompt_path: Optional[str] = None, exaggeration: float = 0.5,
                 cfg_weight: float = 0.5, temperature: float = 0.8, speed: float = 1.0, pitch: float = 0.0,
                 energy: float = 0.0, **kwargs):
        """Same call shape as the reference's `model.generate` (synthesizer.py:344-350), plus the
        prosody controls: speed (speaking rate, 0.25..4), pitch and energy (shifts in the
        predictors' normalised units, -4..4) and exaggeration (0.5 neutral; the pitch and energy
        ranges are clip(2 * exaggeration, 0, 4)) -- prosody_controls; a value outside its range
        raises ValueError.  cfg_weight and temperature stay ignored: the model is deterministic.

        Returns a float32 torch tensor of shape (1, N) on the engine device; the
        reference's `audio.squeeze().cpu().numpy()` applies unchanged.  audio_prompt_path
        selects a stored speaker embedding on a multi-speaker model (speaker_embedding())."""
        import torch
        del cfg_weight, temperature, kwargs
        ctl = prosody_controls(speed=speed, pitch=pitch, energy=energy, exaggeration=exaggeration)
        spk = self.speaker_embedding(audio_prompt_path)
        with self._lock:
            tokens, lens = tokenize_batch([text])
            wav, wav_lens = self.synthesize_tokens(tokens, lens,
                                                   speaker_embedding=None if spk is None else spk[None],
                                                   prosody=None if ctl is None else [ctl])
        return wav[:, : int(wav_lens[0])].contiguous().to(torch.float32)


def scale_durations(durations, scale) -> np.ndarray:
    """Given durations under per-utterance duration_scale values, as the kernel computes them:
    rint(float32(max(d, 0)) * float32(scale)), ties to even; a scale of 1 leaves d as it is."""
    d = np.maximum(np.asarray(durations, np.int64), 0)
    sc = np.asarray(scale, np.float32).reshape(-1, 1)
    scaled = np.rint(d.astype(np.float32) * sc).astype(np.int64)
    return np.where(sc == np.float32(1), np.asarray(durations, np.int64), scaled).astype(np.int32)


def _as_i32(ctl):
    """The controls' float32 block as the int32 words _upload_i32 carries (None passes through)."""
    return None if ctl is None else np.ascontiguousarray(ctl, np.float32).view(np.int32)


def _unit_scale(cb):
    """The controls' device block with a neutral duration_scale (the exact second pass feeds
    durations that are scaled already); None passes through."""
    if cb is None:
        return None
    cb = cb.clone()
    cb[0] = 1.0
    return cb


def _check_per_sentence(prosody, n: int):
    if prosody is not None and len(prosody) != n:
        raise ValueError(f"prosody: {len(prosody)} entries for {n} sentences")


def _pick(prosody, idx):
    """The per-sentence controls of the sentences idx (None when none of them has any)."""
    if prosody is None:
        return None
    sel = [prosody[i] for i in idx]
    return None if all(p is None for p in sel) else sel


# Alias with the reference's class name so `from gonova_tts_amd.model import ChatterboxTTS`
# is a one-line swap at synthesizer.py:167.
ChatterboxTTS = GonovaTTS


class PendingRange:
    """The range word of a batch synthesized with host_lens=False, not yet read (dist.ShardedSynthesis
    reads it with the wave lengths at the one sync it makes).  resolve(lens_host, word_host) returns
    the batch's final (wav, wav_lens np.int64) -- the queued result when the word is 0, else the
    batch synthesized again with the encoder on fp32 MFMA (one RuntimeWarning, range_fallbacks + 1)."""

    def __init__(self, model: "GonovaTTS", args, word):
        self.model, self.args, self.word = model, args, word

    def resolve(self, wav, lens_host, word_host: int):
        if not word_host:
            return wav, lens_host
        import torch
        m = self.model
        with torch.cuda.device(m.engine.device_index), m._range_fallback():
            wav, wav_lens, _ = m._synthesize_once(*self.args)
        return wav, np.asarray(wav_lens, np.int64)


class _ChunkResampler:
    """The output-rate stage of one stream_tokens generator: the reduced ratio and the two history
    buffers tts_resample_poly_chunk alternates between (chunk k reads hist[k % 2] and writes the
    other; chunk 0 reads none, so running it again -- an early first chunk recomputed, a range-guard
    rerun -- starts the history anew)."""

    def __init__(self, engine, B, rate, native, hop, chunk_frames, dev, stream):
        import torch
        g = gcd(rate, native)
        self.engine, self.up, self.down = engine, rate // g, native // g
        self.hop, self.chunk_frames, self.stream = hop, chunk_frames, stream
        self.hist = torch.empty((2, B, resample_history(self.up, self.down)[0]), dtype=torch.float32, device=dev)
        self._lens_of = self._in_lens = None

    def run(self, wav, c0, mel_lens):
        """The chunk of frames starting at c0 (wav [B, frames*hop]) -> its samples at the output rate."""
        if self._lens_of is not mel_lens:  # the utterances' final sample counts, already on the device
            self._lens_of, self._in_lens = mel_lens, (mel_lens * self.hop).int()
        k = (c0 // self.chunk_frames) & 1
        out, _ = self.engine.resample_chunk(wav, c0 * self.hop, self._in_lens, self.up, self.down, self.hist[k],
                                            self.hist[1 - k], return_lens=False, stream=self.stream)
        return out

    def counts(self, lens_h, c0, tc):
        """Valid output samples per utterance of that chunk (host arithmetic, no device read)."""
        return resample_chunk_counts(lens_h * self.hop, c0 * self.hop, tc * self.hop, self.up, self.down)


_UPLOAD_STREAMS: Dict[int, object] = {}


def _upload_i32(arrays, dev, stream=None):
    """Host integer arrays (None passes through) -> device int32 tensors, staged through pinned
    memory and copied on a per-device upload stream that `stream` (else the device's current
    stream, the one the engine calls enqueue on) then waits for.  Copied in order on the compute
    stream, a batch's inputs went up only when the previous batch's kernels had finished -- the
    moment dist.ShardedSynthesis (C4) starts that batch's waveform download, which held the small
    uploads (and the GPU) for ~0.7-1.7 ms per batch (profiles/r05zz_c4_gaps.txt).  Issued at once
    on their own stream they land while the previous batch still computes.  The arrays share one
    pinned block and one copy (64-byte aligned segments; the device tensors are views of it):
    the host time before the first kernel of a request is on C5's critical path."""
    import torch
    target = stream if stream is not None else torch.cuda.current_stream(dev)
    idx = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    up = _UPLOAD_STREAMS.get(idx)
    if up is None:
        up = _UPLOAD_STREAMS[idx] = torch.cuda.Stream(device=idx)
    host = [None if a is None else np.ascontiguousarray(a, np.int32) for a in arrays]
    offs, total = [], 0
    for a in host:
        offs.append(total)
        total += 0 if a is None else -(-a.size // 16) * 16
    pinned = torch.empty((max(total, 16),), dtype=torch.int32, pin_memory=True)
    hv = pinned.numpy()
    for a, o in zip(host, offs):
        if a is not None:
            hv[o:o + a.size] = a.reshape(-1)
    with torch.cuda.stream(up):
        blk = pinned.to(dev, non_blocking=True)
    target.wait_stream(up)
    blk.record_stream(target)  # (allocated on the upload stream, used on the target)
    return [None if a is None else blk[o:o + a.size].view(a.shape) for a, o in zip(host, offs)]


def _to_host(t):
    """Device tensor -> numpy copy through a page-locked block of torch's caching host allocator:
    a pinned D2H runs at DMA speed where `.cpu()` stages a pageable copy (C1's 436 KB waveform is
    on the first frame's critical path).  The copy runs on the tensor's device's current stream,
    the one the engine launched on; the returned array keeps the block alive until dropped."""
    import torch
    with torch.cuda.device(t.device):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return h.numpy()


class _HostRead:
    """_need_and_lens without the blocking read: the durations, frame counts and range word are
    copied into page-locked host memory on the compute stream (where the forward enqueued them)
    and an event is recorded after them; result() waits for that event only, not for work the
    caller enqueued afterwards, and sums on the host.  When the three are views of one block (as
    GonovaEngine.acoustic returns them) the block is read with one copy."""

    def __init__(self, dur, mel_lens, rw=None, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(mel_lens.device)
        ts = (dur, mel_lens, rw)
        base = getattr(mel_lens, "_base", None)
        one = base is not None and base.is_contiguous() and base.dtype == torch.int32 and \
            all(t is None or (getattr(t, "_base", None) is base and t.is_contiguous()) for t in ts)
        with torch.cuda.stream(s):
            if one:
                h = torch.empty(base.shape, dtype=base.dtype, pin_memory=True)
                h.copy_(base, non_blocking=True)
                p0 = base.data_ptr()
                self.bufs = [None if t is None else
                             h[(t.data_ptr() - p0) // 4:(t.data_ptr() - p0) // 4 + t.numel()].view(t.shape) for t in ts]
            else:
                self.bufs = []
                for t in ts:
                    if t is None:
                        self.bufs.append(None)
                        continue
                    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    h.copy_(t, non_blocking=True)
                    self.bufs.append(h)
            self.ev = torch.cuda.Event()
            self.ev.record(s)

    def result(self):
        """-> (need, frame counts np.int64 [B], range word set), as _need_and_lens"""
        self.ev.synchronize()
        d, ln, rw = self.bufs
        lens = ln.numpy().astype(np.int64)
        sums = d.numpy().astype(np.int64).sum(axis=1)
        need = int(np.maximum(sums, lens).max()) if len(lens) else 0
        return need, lens, bool(rw is not None and int(rw.numpy()[0]) != 0)


def _need_and_lens(dur, mel_lens, rw=None):
    """One device -> host read: (frames the used durations add up to at most, the frame counts
    np.int64 [B], the range word is set) -- the durations kernel's all-zero rule gives an
    utterance len frames, so the need is the larger of the two per utterance."""
    import torch
    rows = torch.stack([dur.sum(dim=1).to(torch.int64), mel_lens.to(torch.int64)]).reshape(-1)
    if rw is not None:
        rows = torch.cat([rows, rw.to(torch.int64)])
    h = rows.cpu().numpy()
    B = mel_lens.shape[0]
    need = int(np.maximum(h[:B], h[B:2 * B]).max()) if B else 0
    return need, h[B:2 * B].astype(np.int64), bool(rw is not None and h[2 * B] != 0)


def _read_with_range(lens, rw=None):
    """lens (cuda int64 [B]) and the range word in one device -> host read."""
    import torch
    if rw is None:
        return lens.cpu().numpy(), False
    h = torch.cat([lens, rw.to(torch.int64)]).cpu().numpy()
    return h[:-1], bool(h[-1] != 0)


def _mel_lens_host(lens: np.ndarray, durations: np.ndarray, t_cap: int) -> np.ndarray:
    """Frame counts for given durations, as the engine's durations kernel computes them
    (acoustic_kernels.hip: negative durations count 0; an utterance whose durations are all 0
    gets one frame per token, HF:108-109; clamped to the frame cap)."""
    d = np.asarray(durations, np.int64)
    out = np.zeros(len(lens), np.int64)
    for b, L in enumerate(np.asarray(lens, np.int64)):
        L = int(min(L, d.shape[1]))
        s = int(np.maximum(d[b, :L], 0).sum())
        if s == 0 and L > 0:
            s = L
        out[b] = min(s, t_cap)
    return out
