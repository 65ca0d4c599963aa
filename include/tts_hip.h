/*
 * tts_hip.h — C-ABI of libtts_hip.so, the MI355X (gfx950) batched TTS engine.
 *
 * The reference has no C-ABI: its only model boundary is duck-typed Python
 * (SURVEY.md §8b).  Each entry point below replaces one step of that boundary:
 *
 *   tts_engine_create / tts_engine_set_weight / tts_engine_finalize
 *       replace `ChatterboxTTS.from_pretrained(device=self.device)`
 *       (/root/reference/services/tts/core/synthesizer.py:185; device string from
 *       synthesizer.py:130, "cuda:0" from server.py:400-405).  The Python host maps
 *       "cuda:N" to HIP device N and feeds weights by HF state_dict name.
 *   tts_acoustic_forward + tts_vocoder_forward
 *       replace `self.model.generate(text, audio_prompt_path=..., exaggeration=...,
 *       cfg_weight=0.5, temperature=0.8)` (synthesizer.py:344-350) for a whole
 *       batch of sentences at once (tokens -> mel -> waveform).
 *   tts_vocoder_forward_chunk
 *       sub-sentence streaming the reference lacks (synthesizer.py:320-321 yields
 *       one chunk per sentence); exact receptive-field context.
 *   tts_last_error
 *       replaces Python exception text: the host raises RuntimeError(tts_last_error())
 *       so the reference's exception path (synthesizer.py:323-325, 291-294) holds.
 *
 * Conventions
 *   - Every device buffer passed in is caller-owned (PyTorch-ROCm tensors passed by
 *     data_ptr()).  The engine owns its weights and workspace.
 *   - Work is enqueued asynchronously on `stream` (a hipStream_t; NULL = default).
 *   - Return 0 on success, a negative TTS_ERR_* on failure; no C++ exception crosses
 *     the ABI.  Every entry sets the HIP device and takes a per-engine mutex, so any
 *     host thread may call (the reference calls from a ThreadPoolExecutor,
 *     synthesizer.py:312).  The engine's workspace is shared by all calls: a forward
 *     enqueued on a stream other than the previous call's is made to wait (event edge)
 *     for everything the previous call's stream had enqueued, so calls from different
 *     threads / streams run one after another on the device, never interleaved.
 *   - Activations are channels-last: mel [B][T][80] float32 (HF spectrogram layout),
 *     waveform [B][T*256] float32 at 22,050 Hz.  Compute dtype per stage is chosen
 *     at create time; accumulation is always fp32.
 */
#ifndef TTS_HIP_H
#define TTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_OK 0
#define TTS_ERR_INVALID (-1)
#define TTS_ERR_HIP (-2)
#define TTS_ERR_STATE (-3)
#define TTS_ERR_NOMEM (-4)

enum { TTS_DTYPE_F32 = 0, TTS_DTYPE_F16 = 1, TTS_DTYPE_BF16 = 2 };

typedef struct tts_engine tts_engine;

/* ABI history (INTEGRATION.md "Changelog"):
 *   1  tts_config of five ints (no encoder_precision)
 *   2  tts_config gains encoder_precision (sixth int)
 *   3  tts_engine_create_sized / tts_abi_version / tts_get_switch; stream ordering records
 *      on the caller's stream at the end of each call (a caller may destroy its stream after
 *      the call returns)
 *   4  range guard of the exact encoder: tts_acoustic_range_flag / tts_acoustic_set_precision,
 *      TTS_ENCODER_F32
 *   5  tts_device_bytes (the library's device memory per HIP device); additive.  Also under 5,
 *      additive: tts_resample_poly_chunk / tts_resample_history (a caller detects them by symbol),
 *      and tts_vocoder_context (the loaded generator's receptive field in mel frames), and the
 *      op-level tts_op_rel_attn / tts_op_rel_attn_ws_bytes, and the op-level
 *      tts_op_conv_layer_create / _destroy / tts_op_conv1d_ex / tts_op_conv_ws_bytes, and per-utterance
 *      prosody controls: tts_prosody / tts_acoustic_forward_ctl and the op-level tts_op_variance_adapt */
#define TTS_ABI_VERSION 5
int tts_abi_version(void);

/* Engine configuration.  Fields are only ever appended; a caller built against an older
 * header passes its struct's size to tts_engine_create_sized and the fields past it keep
 * their zero defaults. */
typedef struct tts_config {
  int vocoder_dtype;   /* TTS_DTYPE_*: compute/storage dtype of vocoder activations */
  int acoustic_dtype;  /* TTS_DTYPE_*: compute/storage dtype of acoustic activations */
  int max_batch;       /* workspace reservation hints (0 = grow on demand) */
  int max_frames;
  int max_tokens;
  int encoder_precision; /* TTS_ENCODER_*: precision of the acoustic encoder + variance predictors */
} tts_config;

/* Acoustic encoder precision.  EXACT (the default, 0): with a 16-bit acoustic_dtype the encoder,
 * speaker projection and variance predictors keep fp32 activations and run their GEMMs as three
 * f16 MFMAs (~2^-21 relative per product for activations above ~2^-3, an absolute 2^-25 |w| below:
 * tts_op_conv1d_ex's error model), so the predicted integer durations
 * clamp(round(exp(x) - 1), 0) (HF:181-183) match an fp32 evaluation; the decoder and postnet run in
 * acoustic_dtype.  FAST (1): the whole acoustic model runs in acoustic_dtype (durations can
 * round differently near .5).  With acoustic_dtype = F32, EXACT runs the encoder side on the same
 * split-precision GEMMs and attention, and the decoder / postnet GEMMs on the split-precision
 * GEMMs too (round 6; the decoder attention stays on the fp32 kernel; its row stride keeps two
 * pad rows per utterance), and
 * FAST keeps every layer on fp32 MFMA (switch TTS_F32_ENC_SPLIT=0 at finalize: the same). */
enum { TTS_ENCODER_EXACT = 0, TTS_ENCODER_FAST = 1, TTS_ENCODER_F32 = 2 };
/* Range limit of EXACT: its split GEMMs and attention hold every fp32 operand as two f16 halves,
 * so activations must stay below 65504 in magnitude (f16 max); weights are stored at a
 * power-of-two scale per layer (round 6), so any finite weights are taken.  Activations are
 * checked on the device (ABI 4): every split GEMM and the split attention test the f16 high half
 * of each operand they stage and, when one is inf or NaN (|x| >= 65520, or a NaN input), set the
 * engine's range word.  The forward itself stays asynchronous; the caller reads the word with
 * tts_acoustic_range_flag after its next sync and, when it is set, reruns the acoustic forward
 * with TTS_ENCODER_F32 (the same fp32 layers on the exact fp32 MFMA kernels, ~3x slower on the
 * encoder side, no range limit).  TTS_ENCODER_F32 is a run-time setting only
 * (tts_acoustic_set_precision), not a tts_config value. */

/* fp32 vocoders (vocoder_dtype = TTS_DTYPE_F32): the resblock convs of every stage (channel counts
 * divisible by 32, >= 32) run as split-precision GEMMs (three f16 MFMAs per product, ~2^-21 relative above |x| ~ 2^-3, like the exact
 * encoder).  tts_vocoder_forward / _chunk then read the layers' range word once at the end of the
 * call (one sync of `stream`) and, if an activation left f16's range, rerun the forward with every
 * layer on the fp32 MFMA path; 16-bit vocoders are unaffected and stay asynchronous. */

/* Number of HIP devices visible to this process. */
int tts_device_count(void);

/* Device memory this library holds on HIP device `hip_device` (every engine's weights and
 * workspaces, in bytes) -> *bytes.  The reference's /health reports torch's allocator
 * (server.py:456-465: memory_allocated / memory_reserved), which never sees these buffers;
 * the service adds this figure to its "gpu" report.  Needs no GPU work (a host-side count). */
int tts_device_bytes(int hip_device, int64_t* bytes);

/* Engine lifetime (replaces ChatterboxTTS.from_pretrained, synthesizer.py:185).
 * tts_engine_create reads a whole tts_config of THIS header; tts_engine_create_sized reads
 * cfg_size bytes of it (sizeof(tts_config) of the caller's header; smaller = an older layout,
 * the missing fields zero; larger than this library's struct = TTS_ERR_INVALID). */
int tts_engine_create(int hip_device, const tts_config* cfg, tts_engine** out);
int tts_engine_create_sized(int hip_device, const tts_config* cfg, size_t cfg_size, tts_engine** out);
/* Host fp32 tensor in HF state_dict naming (e.g. "resblocks.3.convs1.2.weight"). */
int tts_engine_set_weight(tts_engine* eng, const char* name, const float* host_data,
                          const int64_t* shape, int ndim);
/* Fold / pack / upload every weight set so far; must precede any forward.  A vocoder
 * configuration outside the supported envelope (last stage of 32 channels,
 * channel counts in multiples of 8, k % stride == 0 with an even k - stride, (k - 1) * dilation
 * <= 64) is refused here with TTS_ERR_INVALID and a tts_last_error() text naming the tensor.
 * So is an acoustic model outside its envelope (hidden size a multiple of 64 up
 * to 512, head size a multiple of 16, both stacks alike, conv channels in multiples of 8 in / 4
 * out with odd k <= 65, depthwise k odd <= 129, predictors of 1+ layers of <= 256 channels,
 * postnet of 1+ layers of <= 512, 80 mel bins), with a text beginning "acoustic envelope:". */
int tts_engine_finalize(tts_engine* eng);
/* Pre-size the workspace (so later calls allocate nothing and can be graph-captured). */
int tts_engine_reserve(tts_engine* eng, int max_batch, int max_frames, int max_tokens);
void tts_engine_destroy(tts_engine* eng);

/* Vocoder (replaces the waveform half of model.generate, synthesizer.py:344).
 *   d_mel      [B][T][80] float32, utterance b valid for d_mel_lens[b] <= T frames
 *   d_wav      [B][T*256] float32; samples >= 256*d_mel_lens[b] are written as 0.   */
int tts_vocoder_forward(tts_engine* eng, const float* d_mel, const int32_t* d_mel_lens, int B,
                        int T, float* d_wav, void* stream);

/* Streaming vocoder chunk with exact context: computes the waveform of frames
 * [ctx_left, ctx_left + T_chunk) of each d_mel[b] window [ctx_left + T_chunk + ctx_right][80]
 * (zero context at utterance edges is expressed by the caller passing shorter windows via
 * d_win_lens).  d_wav [B][T_chunk*hop].  Any ctx_left is accepted (at an utterance's edge there
 * is no context to pass); the chunk equals the whole-utterance pass when the window holds, on each
 * side, the frames tts_vocoder_context reports or reaches the utterance's edge. */
int tts_vocoder_forward_chunk(tts_engine* eng, const float* d_mel, const int32_t* d_win_lens,
                              int B, int T_win, int ctx_left, int T_chunk, float* d_wav,
                              void* stream);

/* Host only: the loaded generator's receptive field in mel frames -> *left, *right, the frames
 * of context before and after a chunk that tts_vocoder_forward_chunk needs to reproduce the
 * whole-utterance pass.  Computed from the taps, dilations and strides of the layers finalize
 * packed (13 and 13 for HiFi-GAN V1; it grows as the hop shrinks).  TTS_ERR_STATE before
 * tts_engine_finalize or without a vocoder. */
int tts_vocoder_context(tts_engine* eng, int* left, int* right);

/* Acoustic model (replaces the text->spectrogram half of model.generate).
 *   d_tokens      [B][N] int32 token ids (padding ignored past d_tok_lens[b])
 *   d_dur_override optional [B][N] int32 frame counts (NULL = predicted durations; when given,
 *                  the duration predictor is not run and d_durations returns these counts)
 *   d_mel         [B][Tcap][80] float32 output, d_mel_lens [B] int32 output
 *   d_durations   optional [B][N] int32 output of the durations actually used
 * Frames past Tcap are dropped (d_mel_lens is clamped to Tcap).  With predicted durations and a
 * loose budget (Tcap > 8 N) the call reads the frame counts back once after the variance adaptor
 * (the calling thread waits for the encoder on `stream`) and runs the decoder at the longest
 * utterance's count instead of Tcap; the output is the same (TTS_DEC_TRIM=0: never, 1: at any
 * budget).  Otherwise, and with d_dur_override, the call stays fully asynchronous. */
int tts_acoustic_forward(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens,
                         int B, int N, const int32_t* d_dur_override, float* d_mel,
                         int32_t* d_mel_lens, int Tcap, int32_t* d_durations, void* stream);

/* The same with per-utterance speaker embeddings (HF:1192-1196):
 * d_spk_emb [B][spk_dim] fp32 on the device, spk_dim == tts_acoustic_speaker_dim(); each is
 * L2-normalised, concatenated to every encoder frame and projected back to the hidden size.
 * NULL (or a model without a speaker projection) = tts_acoustic_forward. */
int tts_acoustic_forward_spk(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens,
                             int B, int N, const int32_t* d_dur_override, const float* d_spk_emb,
                             int spk_dim, float* d_mel, int32_t* d_mel_lens, int Tcap,
                             int32_t* d_durations, void* stream);
/* Per-utterance prosody controls (ABI 5, additive; a caller detects tts_acoustic_forward_ctl by
 * symbol).  Five device arrays of B float32 each; a NULL array is neutral for every utterance.
 * Fields are only ever appended: the struct goes by pointer with its size, as tts_config does.
 * For utterance b with len valid tokens:
 *   duration_scale  HF's speaking_speed (HF:104-109): d = rint(float(d) * scale), ties to even, after
 *                   the prediction or the override and before the all-zero rule -- tts_op_durations'
 *                   `speed`.  Above 1 is slower.  1 skips the multiply; a value that is not positive
 *                   or not finite counts as 1.
 *   pitch_range, pitch_shift    p'[t] = m + range * (p[t] - m) + shift on the predicted pitch, in the
 *                   predictor's normalised units, m the fp32 mean of p over the len valid tokens
 *                   (summed in an order len alone fixes).  range 1 with shift 0 keeps p bit for bit.
 *   energy_range, energy_shift  the same on the predicted energy.
 * An utterance's bits depend on its own tokens and its own controls only -- not on B, its
 * neighbours or their controls, or on what the predictions hold past its length. */
typedef struct tts_prosody {
  const float* duration_scale; /* neutral 1 */
  const float* pitch_shift;    /* neutral 0 */
  const float* pitch_range;    /* neutral 1 */
  const float* energy_shift;   /* neutral 0 */
  const float* energy_range;   /* neutral 1 */
} tts_prosody;

/* tts_acoustic_forward_spk with controls: ctl_size = sizeof(tts_prosody) of the caller's header (a
 * shorter, older struct: the missing controls neutral; a longer one, or a size that is no whole
 * number of pointers: TTS_ERR_INVALID).  ctl == NULL is tts_acoustic_forward_spk itself, launch for
 * launch.  With ctl the variance adaptor's durations, the pitch / energy controls and the embedding
 * add run as one launch in place of three (no launch more than without controls), and the call
 * stays asynchronous under the same conditions; the range guard and TTS_ENCODER_F32 apply unchanged. */
int tts_acoustic_forward_ctl(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens,
                             int B, int N, const int32_t* d_dur_override, const float* d_spk_emb,
                             int spk_dim, float* d_mel, int32_t* d_mel_lens, int Tcap,
                             int32_t* d_durations, const tts_prosody* ctl, size_t ctl_size, void* stream);
/* Speaker-embedding size E of the loaded acoustic model (0: single speaker). */
int tts_acoustic_speaker_dim(tts_engine* eng, int* dim);

/* Range guard (ABI 4, TTS_ENCODER_EXACT above): enqueue on `stream` a copy of the engine's
 * range word into *dst (device or host-pinned int32; 1 = some split-precision operand of an
 * acoustic forward enqueued before this call was outside f16's range, 0 = none), then clear the
 * word.  Read *dst after synchronising the stream. */
int tts_acoustic_range_flag(tts_engine* eng, int32_t* dst, void* stream);
/* Encoder precision of later acoustic forwards of a 16-bit model created with EXACT:
 * TTS_ENCODER_EXACT (split-precision, the default) or TTS_ENCODER_F32 (exact fp32 MFMA: the
 * range guard's fallback).  Other models: TTS_ERR_INVALID. */
int tts_acoustic_set_precision(tts_engine* eng, int precision);

/* Live kernel timing for bench.py: with profiling on, every implicit-GEMM launch is
 * bracketed by hipEvents on its own stream; _read() waits for them and returns the summed
 * kernel time (ms), the algorithmic FLOPs of those launches and their count, then resets. */
int tts_engine_profile(tts_engine* eng, int enable);
int tts_engine_profile_read(tts_engine* eng, double* gemm_ms, double* gemm_flops, int* n_launches);
/* The same, split by kernel family into arrays of nkinds entries:
 * 0 = conv_gemm_kernel, 1 = conv_xres_kernel, 2 = (retired: round 1's whole-stage kernel), 3 = mrf_pair_kernel,
 * 4 = mrf_chain_kernel, 5 = upsample_stream_kernel, 6 = conv_split_kernel, 7 = the fused relative-position
 * attention (FLOPs 6*D*B*Tm^2: scores, relative-position scores and P.V at the padded extent), 8 = the
 * acoustic model's other launches (LayerNorm, GLU/depthwise, transposes, variance adaptor; no FLOPs). */
int tts_engine_profile_read_kinds(tts_engine* eng, int nkinds, double* ms, double* flops, int* n_launches);

/* Process-wide switch selecting an alternative kernel path (A/B runs, the parity tests'
 * reference paths): TTS_REL_ATTN, TTS_MRF_FUSED, TTS_MRF_CHAIN, TTS_POST_FUSE, TTS_UP_STREAM,
 * TTS_XRES_NARROW, TTS_XRES_NT, TTS_PAIR_DIV, TTS_ATTN_KSPLIT, TTS_SPLIT_WHOLE, TTS_XRES_DMA,
 * TTS_LN_FUSE, TTS_SPLIT_NT1, TTS_XRES_ORDER, TTS_PAIR_SPLIT, TTS_VP_BATCH, TTS_DEC_TRIM,
 * TTS_ATTN_F32_KC, TTS_F32_ENC_SPLIT, TTS_F32_DEC_SPLIT, TTS_F32_DEC_PACKED, TTS_UP_FUSE.  Each starts from its environment variable, read once; value -1 restores the built-in default.
 * Applies to launches enqueued after the call (use from one thread while no forward runs). */
int tts_set_switch(const char* name, int value);
/* Current value of a switch (-1 = not set), so a caller can restore what it changed. */
int tts_get_switch(const char* name, int* value);

/* Rational-rate resampling of waveforms (22,050 -> 24,000 Hz for
 * clients that assume the reference's hard-coded 24 kHz, synthesizer.py:119 /
 * queue_manager.py:40).  Restates scipy.signal.resample_poly(x, up, down) with its default
 * Kaiser(5.0) FIR and zero padding, per utterance: d_in [B][in_stride] fp32 with d_in_lens[b]
 * valid samples -> d_out [B][out_stride], d_out_lens[b] = min(ceil(len*up/down), out_cap);
 * samples past each length (up to out_cap) are written as 0.  up/down are reduced by their gcd. */
int tts_resample_poly(tts_engine* eng, const float* d_in, int64_t in_stride, const int32_t* d_in_lens, int B,
                      int up, int down, float* d_out, int64_t out_stride, int out_cap, int32_t* d_out_lens,
                      void* stream);
/* Host only: the padded filter taps tts_resample_poly uses (float64, scaled by up); returns the
 * tap count (h filled only when cap >= it), *n_pre_remove = leading outputs scipy discards. */
int tts_resample_filter(int up, int down, double* h, int cap, int* n_pre_remove);

/* The same resampling of a stream that arrives in chunks (sub-sentence streaming at 24 kHz): the
 * outputs of all chunks, one after another, are tts_resample_poly's of the whole input, bit for
 * bit.  Per call, for each utterance b:
 *   d_in       [B][in_stride]: its samples [in_start, in_start + in_count) (the same for every b)
 *   d_in_lens  [b] = n_in, its FINAL total length (known before the first chunk: mel_lens * 256);
 *              samples of d_in at or past n_in are never read into a sum
 *   d_hist_in  [B][n_hist]: the n_hist samples before in_start (not read, may be NULL, when
 *              in_start == 0)
 *   d_hist_out [B][n_hist]: the n_hist samples before in_start + in_count, for the next call
 *              (a buffer other than d_hist_in; in_count < n_hist is fine)
 *   d_out      [B][out_stride]: outputs [emitted(in_start), emitted(in_start + in_count)), then zeros
 *              up to out_cap; d_out_lens[b] (NULL: not written) their count, where
 *              emitted(E) = n_out = ceil(n_in*up/down) if E >= n_in, else
 *                           min(n_out, max(0, ceil(E*up/down) - n_flush))
 *              -- an output is emitted once its newest tap is inside the samples seen, and the
 *              last <= n_flush outputs of an utterance with the chunk it ends in.
 * out_cap must be >= ceil(in_count*up/down) + n_flush (no chunk emits more); n_hist and n_flush
 * come from tts_resample_history (20 and 11 at 160/147).  One kernel launch, no host sync. */
int tts_resample_poly_chunk(tts_engine* eng, const float* d_in, int64_t in_stride, int64_t in_start, int in_count,
                            const int32_t* d_in_lens, int B, int up, int down, const float* d_hist_in,
                            float* d_hist_out, float* d_out, int64_t out_stride, int out_cap, int32_t* d_out_lens,
                            void* stream);
/* Host only: *n_hist = history samples tts_resample_poly_chunk carries between chunks (taps per
 * output - 1), *n_flush = scipy's n_pre_remove (outputs held back until the utterance ends). */
int tts_resample_history(int up, int down, int* n_hist, int* n_flush);

/* Thread-local message describing the last failure on this thread. */
const char* tts_last_error(void);

/* ---- op-level entry used by the parity tests (one implicit-GEMM conv launch) ---- */
typedef struct tts_conv_desc {
  const void* x; int64_t sxb; int32_t sxr; const int32_t* x_len; int32_t x_rows;
  const void* w; int64_t swb; int32_t w_ld;
  const float* bias;
  void* y; int64_t syb; int32_t syr;
  const void* r1; const void* r2; int64_t srb; int32_t srr;
  const int32_t* y_len; int32_t y_rows;
  int32_t M, Cin, taps, dil, pad;
  float in_slope; int32_t act_out; float out_slope; float alpha; float out_scale;
  int32_t up_s, up_cout, up_p; const int32_t* up_len;
  int32_t B;
} tts_conv_desc;

int tts_op_conv1d(int dtype, const tts_conv_desc* desc, void* stream);

/* ---- op-level entry that reaches every conv GEMM form (ABI 5, additive; detected by symbol) ----
 * tts_op_conv1d above can only run conv_gemm_kernel.  Here the layer is packed as the engine packs
 * it at finalize (make_conv: the [M][taps][Cin] copy, the fragment-packed copy of a 16-bit layer
 * with Cin % 64 == 0 and M >= 64, and for an fp32 layer with split != 0 the two-plane f16 copy at a
 * power-of-two scale with its unscale factor), and the launch carries every field the models set.
 *   w     host fp32 in nn.Conv1d layout [M][Cin][k]; bias host fp32 [M] or NULL (zeros)
 *   split fp32 only: also build the split-precision copy (three f16 MFMAs per product)
 * The layer lives on the HIP device current at create; destroy frees its buffers (NULL is fine). */
typedef struct tts_conv_layer tts_conv_layer;
int tts_op_conv_layer_create(int dtype, int split, const float* w, const float* bias, int M, int Cin, int k,
                             int dil, int pad, tts_conv_layer** layer);
void tts_op_conv_layer_destroy(tts_conv_layer* layer);

/* Everything of a launch that tts_conv_desc does not hold.  All-zero = the plain launch. */
typedef struct tts_conv_ext {
  int32_t rows_pad;      /* > 0: the packed-row promise -- x / y / residuals contiguous [B][rows][C], x_rows ==
                            y_rows a multiple of 32, every utterance followed by >= rows_pad masked rows */
  void* ws;              /* fp32 split-K partials (either split-K form), ws_bytes of them; see */
  int64_t ws_bytes;      /* tts_op_conv_ws_bytes.  Without it the packed split form runs one slice. */
  int32_t f32_splitk;    /* fp32 MFMA form (no split copy, or no_split): split K into slices + a reduce */
  int32_t no_split;      /* run an fp32 layer on the fp32 MFMA kernel even where the split form is eligible */
  int32_t* range_flag;   /* device int32 or NULL: the split form ORs 1 into it when the f16 high half of an
                            activation it staged is inf or NaN (|x| >= 65520); never cleared here */
  void* ln_out;          /* LN2?(LN1(y)) rows, y's strides and dtype (NULL: no LayerNorm) */
  const float *ln_g1, *ln_b1, *ln_g2, *ln_b2;  /* device fp32 [M]; ln_g2 NULL: one LayerNorm */
  float ln_eps;
  int32_t* ln_cnt;       /* device int32 [ln_cnt_n] row-tile counters for the in-launch LayerNorm, or NULL */
  int32_t ln_cnt_n;
  const float* ln_lin_w; /* with ln_lin_out: LN1(y) . ln_lin_w + ln_lin_b per row (fp32 [B][y_rows]) instead */
  float ln_lin_b;        /* of ln_out */
  float* ln_lin_out;
  int32_t kind;          /* out: the family the launch ran as (tts_engine_profile_read_kinds' index) */
  int32_t kernels;       /* out: kernels enqueued (the GEMM, + a split-K reduce, + a separate LayerNorm) */
} tts_conv_ext;

/* One conv launch of `layer`: desc's w / swb / w_ld / bias / M / Cin / taps / dil / pad are taken from
 * the layer (what desc holds there is ignored), the transposed-conv mapping (up_s) must be 0, ext
 * may be NULL.  Validated like every model launch (TTS_ERR_INVALID with a message).
 *
 * With len = min(y_len[b], y_rows) (y_rows when y_len is NULL), rows r >= len of utterance b:
 *   y           never written, by any family: conv_gemm_kernel, conv_xres_kernel, both split-precision
 *               kernels and split_reduce_kernel all skip them (a caller that needs zeros there clears
 *               y itself).  Where a split-K reduce applies the LayerNorm (split_reduce_ln_kernel:
 *               ln_out given, no act_out, M <= 512) y is not written at all, valid rows included.
 *   ln_out      never written: the in-launch tails, split_reduce_ln_kernel and the separate LayerNorm
 *               launch all skip them.
 *   ln_lin_out  the families differ: a launch that applies the LayerNorm itself (ln_cnt given, grid
 *               large enough or TTS_LN_FUSE=7) leaves them alone; the separate LayerNorm + Linear launch
 *               writes every row of [B][y_rows], those past len from whatever y holds there.
 * An utterance of length 0 writes nothing (ln_lin_out as above).
 * x rows at or past x_len[b] (x_rows when NULL), rows before the utterance (the left pad) and the pad
 * rows of the packed layout never reach a sum: every kernel replaces them with zeros as it stages
 * them, whatever they hold (NaN and inf included), before the split form's range check, so they
 * never reach the range word either.
 * ln_cnt must be all zero on entry; a launch that used the counters leaves them all zero again (the
 * last M block of a row tile resets its counter), so they serve the next launch on the stream.
 * A row's bits depend on its own utterance only -- not on B, on the other utterances, or on the row
 * tile height the grid picked (the K order comes from the layer shape alone).
 *
 * Error of the split-precision form (fp32 layer, split != 0).  Each fp32 operand is held as two f16
 * halves; the weights are scaled by a power of two per layer, so their low halves stay normal f16
 * down to ~2^-19 max|w|; the activations are NOT scaled.  A product x.w is hi.hi + hi.lo + lo.hi in
 * one fp32 accumulator: the dropped lo.lo term and the two low halves' roundings cost at most
 * 3 * 2^-22 |x||w| while x's low half is a normal f16, i.e. for |x| above ~2^-3.  Below that the low
 * half is a subnormal (spacing 2^-24) and a product is off by up to 2^-25 |w| whatever |x| is: an
 * absolute floor, ~2^-15 relative at |x| = 1e-3 (measured on an MI355X with activations of
 * 2..4 * 2^-12: up to 64 * 2^-21 of sum|x||w|, against 0.5 * 2^-21 at |x| ~ 1; profiles/conv_op_parity.json).
 * The same floor, 2^-25 2^-s |x|, holds for a weight under ~2^-19 of its layer's largest.  The
 * models feed these layers LayerNorm outputs of order one; tests/test_conv_op_gpu.py holds every
 * form to this model (oracle/conv.py), the small activations included. */
int tts_op_conv1d_ex(const tts_conv_layer* layer, const tts_conv_desc* desc, tts_conv_ext* ext, void* stream);
/* Host only: bytes of split-K workspace a launch of this shape over `rows` (= B * y_rows) flat rows
 * can use -- the larger of the packed split form's and the fp32 split-K's partials (0: neither splits). */
int64_t tts_op_conv_ws_bytes(int taps, int Cin, int M, int rows);

/* ---- op-level entry used by the parity tests (one fused relative-position attention) ----
 * (ABI 5, additive; a caller detects it by symbol.)  For utterance b, head h, query i < lens[b]:
 *   S[i][j]  = ((q[i] + pos_u[h]) . k[j] + (q[i] + pos_v[h]) . R[i - j]) * scale,   j < lens[b]
 *   out[b][i][h*192 ..] = softmax_j(S[i]) . v
 * with q / k / v the three D-wide slices of qkv row [b][i] and R[rel] = ptab row rmax - 1 - rel.
 *   dtype      TTS_DTYPE_*: the type of qkv, ptab and out.  split (fp32 only): every product as
 *              three f16 MFMAs (the exact encoder's form); operands must stay inside f16's range
 *   pos_u/v    [H][192] float32; q + pos is one fp32 add, rounded once to dtype
 *   qkv        [B][Tp][3*D], ptab [2*rmax][D], out [B][Tp][D], lens [B] int32 with lens[b] <= Tm
 *   Tm <= Tp, Tm <= rmax, D == H * 192; anything else is TTS_ERR_INVALID with a message
 *   range_flag optional device int32: the split form ORs 1 into it when the f16 high half of an
 *              operand it staged is inf or NaN (tts_acoustic_range_flag's word); never cleared here
 *   ws         optional caller-owned device workspace of ws_bytes for the fp32 (non-split) form's
 *              key chunks; with fewer than tts_op_rel_attn_ws_bytes() the kernel runs one chunk
 * Rows at or past an utterance's length:
 *   out   rows i >= lens[b] are never written (an utterance of length 0 writes nothing).
 *   qkv   the k and v slices of rows j >= lens[b] never reach a sum: the 16-bit and split forms do
 *         not read them, the fp32 form reads rows < Tp and replaces them with zeros.  The q slices
 *         of rows up to the end of the last 64-query tile (clamped to row Tp - 1) are read as
 *         queries whose results are discarded; they stay private to their own row, so any value is
 *         harmless there, except that the split form range-checks them like every operand.
 * A row's bits depend on its own utterance only, never on B or on the other utterances.
 * TTS_ATTN_KSPLIT (16-bit) and TTS_ATTN_F32_KC (fp32) select the alternative forms as in the model. */
int tts_op_rel_attn(int dtype, int split, const float* pos_u, const float* pos_v, const void* qkv,
                    const void* ptab, const int32_t* lens, int B, int Tm, int Tp, int D, int H, int rmax,
                    float scale, void* out, int32_t* range_flag, void* ws, int64_t ws_bytes, void* stream);
/* Host only: bytes of workspace the fp32 form's key chunks need at these extents under the current
 * TTS_ATTN_F32_KC (0: none, one chunk covers Tm). */
int64_t tts_op_rel_attn_ws_bytes(int B, int Tm, int Tp, int D, int H);

/* ---- op-level entries of the acoustic model's row-wise kernels (one launch each) ----
 * (ABI 5, additive; a caller detects them by symbol.)  Every pointer is a device pointer, dtype a
 * TTS_DTYPE_* (the type of every `void*` activation; gains, biases, tables of weights named float
 * are fp32), every buffer dense in the layout given, lens[b] int32.  Null buffers, extents <= 0
 * and whatever else an entry names are TTS_ERR_INVALID with a message, nothing launched.
 * For all of them: input rows that the entry says are masked never reach a valid output, whatever
 * they hold (NaN and inf included), and a valid row's bits depend on its own utterance only -- not
 * on B, on the other utterances or on what lies past its length.
 *
 * embed: out[b][t][:] = round(fp32(table[clamp(ids[b][t], 0, V - 1)][:]) * scale) for t < len,
 *   len = min(lens[b], N): one fp32 multiply, one rounding.  ids [B][N] int32, table [V][D],
 *   out [B][Tm][D].  Rows t in [len, Tm) are written as zeros (Tm < len: only Tm rows exist);
 *   ids at or past len are not read. */
int tts_op_embed(int dtype, const int32_t* ids, const int32_t* lens, int B, int N, int Tm, const void* table, int V,
                 int D, float scale, void* out, void* stream);
/* layernorm: out[r] = LN2?(LN1(in[r])) over C <= 512 channels (more: refused), rows [rows][C];
 *   fp32 two-pass mean / variance (biased, eps inside the root), LN1's result rounded to dtype
 *   before LN2 (g2 / b2 NULL: one LayerNorm).  lens (optional, with stride > 0): row r belongs to
 *   utterance r / stride and is skipped -- neither read nor written -- when r % stride >= lens[b].
 *   in == out is fine.  The gains need 4-byte alignment only: 16-byte-aligned ones load as
 *   vectors in the 16-bit C % 8 == 0 kernel, to the same bits.
 * layernorm_groups: `groups` (1..4) LayerNorms of C <= 256 channels side by side, in place, in rows
 *   of ld >= groups * C elements: channels [i C, (i + 1) C) with g[i] / b[i] (host arrays of device
 *   pointers).  Columns at or past groups * C and rows masked by lens are left alone. */
int tts_op_layernorm(int dtype, const void* in, void* out, int rows, int C, const float* g1, const float* b1,
                     const float* g2, const float* b2, float eps, const int32_t* lens, int stride, void* stream);
int tts_op_layernorm_groups(int dtype, void* x, int rows, int C, int ld, int groups, const float* const* g,
                            const float* const* b, float eps, const int32_t* lens, int stride, void* stream);
/* pos_bias: qu[r][c] = round(fp32(q[r][c]) + u[c]), qv likewise with v: q the first D of the 3 D
 *   columns of qkv row r; qu / qv [rows][D]; u / v fp32 [D].  Every row is read and written (no
 *   lengths: a row stays private to itself). */
int tts_op_pos_bias(int dtype, const void* qkv, int rows, int D, const float* u, const float* v, void* qu, void* qv,
                    void* stream);
/* transpose_v: vt[b][h][d][j] = v[b][j][h dk + d], v the last D columns of qkv [B][Tm][3 D],
 *   dk = D / H (D % H != 0: refused), vt [B][H][dk][Sk].  Bits are copied (-0, subnormals, inf).
 *   With len = min(lens[b], Tm): keys j in [len, Sk) are written as zeros whatever qkv holds there
 *   (those rows are not read); keys j >= Sk are dropped; nothing is written at or past Sk. */
int tts_op_transpose_v(int dtype, const void* qkv, const int32_t* lens, int B, int Tm, int D, int H, int Sk, void* vt,
                       void* stream);
/* rel_softmax: p[b,h][i][j] = softmax_j((ac[b,h][i][j] + bd[b,h][i][Tm - 1 - i + j]) * scale) over
 *   j < len = min(lens[b], Tm); ac [B H][Tm][Sac], bd [B H][Tm][Sbd], p [B H][Tm][Sk] with Sac, Sk
 *   >= Tm and Sbd >= 2 Tm - 1 (else refused).  The maximum is subtracted before the exponential.
 *   Columns j in [len, Sk) of every row are written as zeros; columns >= len of ac and
 *   >= Tm - 1 - i + len of bd row i are not read.  Rows i in [len, Tm) ARE computed, from whatever
 *   ac / bd hold there over the same len keys: a caller masks them downstream (the model's P.V GEMM
 *   does).  An utterance of length 0 is treated as length 1: column 0 of every row is read and
 *   written (1, or NaN when the inputs there are not finite), the rest zeros. */
int tts_op_rel_softmax(int dtype, const void* ac, const void* bd, const int32_t* lens, int B, int H, int Tm, int Sac,
                       int Sbd, int Sk, float scale, void* p, void* stream);
/* glu_dwconv: g[t][c] = a[t][c] * sigmoid(a[t][D + c]); out[t][c] = SiLU(bias[c] + sum_j w[c][j] *
 *   g[t + j - (k - 1) / 2][c]), g outside [0, len) taken as 0, len = min(lens[b], Tm); a [B][Tm][2 D],
 *   out [B][Tm][D], w fp32 [D][k], k odd and <= 129 (else refused).  Rows t >= len of out are never
 *   written and rows >= len of a never read; an utterance of length 0 writes nothing. */
int tts_op_glu_dwconv(int dtype, const void* a, const int32_t* lens, int B, int Tm, int D, const float* w, int k,
                      const float* bias, void* out, void* stream);
/* durations: per utterance, len = min(lens[b], N) (N <= 16383):
 *     d[t] = max(override_d[b][t], 0) when override_d is given, else max(rint(expf(logd[b][t]) - 1), 0),
 *     then rint(d * speed) when speed != 1 (ties to even both times); t >= len: d = 0, logd /
 *     override_d there are not read; if every d is 0 and len > 0, d[t] = 1 for t < len.
 *   dur [B][N]       d, all N entries written, NOT clamped to Tcap
 *   mel_lens [b]     min(sum d, Tcap)
 *   tokmap [B][Tcap] frame f < mel_lens[b]: the token t with sum_{s<t} d[s] <= f < sum_{s<=t} d[s]
 *                    (never one of duration 0); f >= mel_lens[b]: -1.  With sum d > Tcap the map
 *                    holds the first Tcap frames, and sum(dur) > mel_lens tells the caller. */
int tts_op_durations(const float* logd, const int32_t* lens, int B, int N, const int32_t* override_d, float speed,
                     int Tcap, int32_t* dur, int32_t* mel_lens, int32_t* tokmap, void* stream);
/* var_embed_add, in place on x [rows][D]: x = round(round(x + round(e[r] we[c] + be[c])) +
 *   round(p[r] wp[c] + bp[c])), every round to dtype (HF adds the two embeddings one after the
 *   other in the model's dtype); e / p fp32 [rows], we / be / wp / bp fp32 [D].  Every row is
 *   read and written. */
int tts_op_var_embed_add(int dtype, void* x, int rows, int D, const float* e, const float* we, const float* be,
                         const float* p, const float* wp, const float* bp, void* stream);
/* variance_adapt: the controlled forward's variance adaptor, one launch, one block per utterance
 *   (len = min(lens[b], N), N <= 16383, Np >= N else refused).  logd (may be NULL with override_d),
 *   pitch and energy are fp32 [B][Np]; override_d int32 [B][N] or NULL; ctl / ctl_size as for
 *   tts_acoustic_forward_ctl (NULL: all neutral); we / be / wp / bp fp32 [D] as in var_embed_add.
 *     dur [B][N], mel_lens [B], tokmap [B][Tcap]   durations' outputs with speed = duration_scale[b]
 *     pitch, energy   tokens t < len rewritten in place by tts_prosody's formula, a neutral
 *                     quantity left bit for bit; tokens t >= len neither read nor written
 *     x [B][Np][D]    rows t < len get var_embed_add's rounding chain with the rewritten energy and
 *                     pitch; rows t >= len are not touched */
int tts_op_variance_adapt(int dtype, void* x, const float* logd, float* pitch, float* energy, const int32_t* lens,
                          int B, int N, int Np, int D, const int32_t* override_d, const tts_prosody* ctl,
                          size_t ctl_size, const float* we, const float* be, const float* wp, const float* bp, int Tcap,
                          int32_t* dur, int32_t* mel_lens, int32_t* tokmap, void* stream);
/* regulate: out[b][f][:] = round(fp32(enc[b][tokmap[b][f]][:]) * scale) for f < frames; enc [B][N][D]
 *   of dtype_in (dtype, or fp32 with a 16-bit dtype; another pair is refused), tokmap [B][Tcap] with
 *   entries < N, out [B][Tout][D], frames <= Tcap and <= Tout (else refused).  A frame whose token
 *   is negative is written as zeros; rows f in [frames, Tout) are never written. */
int tts_op_regulate(int dtype_in, int dtype, const void* enc, int B, int N, int D, const int32_t* tokmap, int Tcap,
                    int frames, int Tout, float scale, void* out, void* stream);
/* mel_out: out[b][t][:] = fp32(in[b][t][:]) for t < min(mel_lens[b], Tcap), zeros for the other rows
 *   below Tcap; in [B][Tin][C] with mel_lens[b] <= Tin (rows at or past it are not read), out fp32
 *   [B][Tcap][C].  Bits are copied (widened). */
int tts_op_mel_out(int dtype, const void* in, const int32_t* mel_lens, int B, int Tin, int Tcap, int C, float* out,
                   void* stream);
/* spk_bias: out[b][o] = round(bias[o] + (sum_i We[o][i] e[b][i]) / max(||e[b]||, 1e-12)); e fp32
 *   [B][E], We fp32 [D][E], bias fp32 [D], out [B][D].  The norm runs over all E elements. */
int tts_op_spk_bias(int dtype, const float* e, int B, int E, const float* We, const float* bias, int D, void* out,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTS_HIP_H */
