// libtts_hip.so — the engine object and the public C-ABI (include/tts_hip.h).
//
// The engine owns the host weight map until finalize, the two models (vocoder.h, acoustic.h), whose
// device weights and workspaces are sized for [max_batch x max_frames], and the order between
// callers' streams; forwards enqueue kernels on the caller's stream and never allocate once reserved.
// The op-level entries the tests call are in ops.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "acoustic.h"
#include "acoustic_kernels.h"
#include "capi.h"
#include "switches.h"
#include "vocoder.h"

using namespace tts;

static thread_local std::string g_last_error;
void tts::set_last_error(const char* msg) { g_last_error = msg; }

struct tts_engine {
  struct HostTensor { std::vector<int64_t> shape; std::vector<float> data; };
  int device = 0;
  tts_config cfg{};
  std::mutex mu;
  std::map<std::string, HostTensor> host;
  bool finalized = false;

  Vocoder voc;
  AcousticModel ac;
  Profiler prof;

  // polyphase resampler tables, keyed by the reduced (up, down): [up][nq] fp32 on the device
  struct Resampler { int up, down, nq, n_pre_remove; float* hp; };
  std::vector<Resampler> resamplers;

  // The models' workspaces are shared by every call on this engine.  Every enqueuing call records
  // order_ev on its own stream when it returns (CallOrder below); a call on a stream other than
  // the previous call's first waits for that event, so two callers on two streams never
  // overwrite each other's scratch.  The engine touches a caller's stream only inside that
  // caller's own call: a C caller may destroy its stream as soon as the call has returned.
  hipStream_t last_stream = nullptr;
  bool has_last = false;
  hipEvent_t order_ev = nullptr;
  void order_after_previous(hipStream_t s) {
    if (!order_ev) HIP_CHECK(hipEventCreateWithFlags(&order_ev, hipEventDisableTiming));
    if (has_last && s != last_stream) HIP_CHECK(hipStreamWaitEvent(s, order_ev, 0));
  }
  // records order_ev on s after the call's work (also when the call failed midway: whatever it
  // enqueued is then ordered before the next caller's)
  void order_record(hipStream_t s) {
    if (order_ev && hipEventRecord(order_ev, s) == hipSuccess) {
      last_stream = s;
      has_last = true;
    } else {
      // nothing recorded: the next call on any other stream must not wait on a stale record
      // older than this call's work, so fall back to a full device-side ordering point
      hipStreamSynchronize(s);
      has_last = false;
    }
  }
  struct CallOrder {
    tts_engine* e;
    hipStream_t s;
    CallOrder(tts_engine* e_, hipStream_t s_) : e(e_), s(s_) { e->order_after_previous(s); }
    ~CallOrder() { e->order_record(s); }
  };

  // (the vocoder frees its own buffers after this body, with the device still selected)
  ~tts_engine() {
    hipSetDevice(device);
    if (order_ev) hipEventDestroy(order_ev);
    for (auto& r : resamplers) dev_free(r.hp);
    ac.free_all();
  }
};

bool tts::read_prosody(const tts_prosody* ctl, size_t ctl_size, VarianceCtl* out) {
  if (ctl_size > sizeof(tts_prosody) || ctl_size % sizeof(const float*) != 0) return false;
  tts_prosody c{};
  std::memcpy(&c, ctl, ctl_size);
  out->duration_scale = c.duration_scale;
  out->pitch_shift = c.pitch_shift;
  out->pitch_range = c.pitch_range;
  out->energy_shift = c.energy_shift;
  out->energy_range = c.energy_range;
  return true;
}

// tts_acoustic_forward_spk / _ctl: ctl null = the plain variance adaptor launches
static int acoustic_forward_any(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens, int B, int N,
                                const int32_t* d_dur_override, const float* d_spk_emb, int spk_dim, float* d_mel,
                                int32_t* d_mel_lens, int Tcap, int32_t* d_durations, const VarianceCtl* ctl,
                                void* stream) {
  return guarded(eng, [&] {
    if (!eng->finalized) throw TtsError(TTS_ERR_STATE, "finalize first");
    if (!eng->ac.loaded) throw TtsError(TTS_ERR_STATE, "acoustic weights not loaded");
    if (!d_tokens || !d_tok_lens || !d_mel || !d_mel_lens || B <= 0 || N <= 0 || Tcap <= 0)
      throw TtsError(TTS_ERR_INVALID, "bad acoustic args");
    if (d_spk_emb && eng->ac.speaker_dim() && spk_dim != eng->ac.speaker_dim())
      throw TtsError(TTS_ERR_INVALID, "speaker embedding size does not match the model's projection");
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    eng->ac.forward(d_tokens, d_tok_lens, B, N, d_dur_override, d_mel, d_mel_lens, Tcap, d_durations, d_spk_emb,
                    (hipStream_t)stream, ctl);
  });
}

// The polyphase filter of up/down reduced by their gcd (the resampler entries and the engine's tables)
struct ResampleFilter { int up, down, n, n_pre_remove; std::vector<double> h; };
static ResampleFilter resample_filter(int up, int down) {
  const int g = std::gcd(up, down);
  ResampleFilter f{up / g, down / g, 0, 0, {}};
  f.n = resample_design(f.up, f.down, f.h, f.n_pre_remove);
  return f;
}

// the engine's polyphase table for (up, down): designed and uploaded at the reduced pair's first
// use, cached for the engine's life (later calls allocate nothing)
static tts_engine::Resampler resampler_for(tts_engine* eng, int up, int down) {
  const int g = std::gcd(up, down);
  for (auto& r : eng->resamplers)
    if (r.up == up / g && r.down == down / g) return r;
  const ResampleFilter f = resample_filter(up, down);
  const int nq = (f.n + f.up - 1) / f.up;
  std::vector<float> hp((size_t)f.up * nq, 0.f);
  for (int k = 0; k < f.n; ++k) hp[(size_t)(k % f.up) * nq + k / f.up] = (float)f.h[k];
  float* d = upload_f32(hp);
  eng->resamplers.push_back({f.up, f.down, nq, f.n_pre_remove, d});
  return eng->resamplers.back();
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

const char* tts_last_error(void) { return g_last_error.c_str(); }

int tts_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tts_abi_version(void) { return TTS_ABI_VERSION; }

int tts_device_bytes(int hip_device, int64_t* bytes) {
  if (!bytes) return TTS_ERR_INVALID;
  *bytes = (int64_t)tts::dev_bytes(hip_device);
  return 0;
}

int tts_engine_create(int hip_device, const tts_config* cfg, tts_engine** out) {
  return tts_engine_create_sized(hip_device, cfg, cfg ? sizeof(tts_config) : 0, out);
}

int tts_engine_create_sized(int hip_device, const tts_config* cfg, size_t cfg_size, tts_engine** out) {
  return guarded([&] {  // (no engine yet: nothing to lock)
    if (!out) throw TtsError(TTS_ERR_INVALID, "null out");
    *out = nullptr;
    // the fields a caller's struct does not reach keep their zero defaults (ABI 1's five-int
    // struct: cfg_size 20 -> encoder_precision EXACT); a larger struct is a newer header
    if (cfg && cfg_size % sizeof(int) != 0) throw TtsError(TTS_ERR_INVALID, "cfg_size is not a whole number of fields");
    if (cfg && cfg_size > sizeof(tts_config))
      throw TtsError(TTS_ERR_INVALID, "tts_config of " + std::to_string(cfg_size) + " bytes is newer than this library (" +
                                          std::to_string(sizeof(tts_config)) + ")");
    tts_config c{};
    if (cfg) std::memcpy(&c, cfg, cfg_size);
    auto okdt = [](int d) { return d == DT_F32 || d == DT_F16 || d == DT_BF16; };
    if (!okdt(c.vocoder_dtype) || !okdt(c.acoustic_dtype)) throw TtsError(TTS_ERR_INVALID, "bad dtype");
    if (c.encoder_precision != TTS_ENCODER_EXACT && c.encoder_precision != TTS_ENCODER_FAST)
      throw TtsError(TTS_ERR_INVALID, "bad encoder_precision");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    if (hip_device < 0 || hip_device >= n)
      throw TtsError(TTS_ERR_INVALID, "hip device " + std::to_string(hip_device) + " out of range");
    std::unique_ptr<tts_engine> e(new tts_engine());
    e->device = hip_device;
    e->cfg = c;
    HIP_CHECK(hipSetDevice(hip_device));
    *out = e.release();
  });
}

int tts_engine_set_weight(tts_engine* eng, const char* name, const float* host_data, const int64_t* shape,
                          int ndim) {
  return guarded(eng, [&] {
    if (!name || (!host_data) || ndim < 0 || ndim > 8) throw TtsError(TTS_ERR_INVALID, "bad weight args");
    if (eng->finalized) throw TtsError(TTS_ERR_STATE, "engine already finalized");
    tts_engine::HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] < 0) throw TtsError(TTS_ERR_INVALID, "negative dim");
      t.shape.push_back(shape[i]);
      n *= (size_t)shape[i];
    }
    t.data.assign(host_data, host_data + n);
    eng->host[name] = std::move(t);
  });
}

int tts_engine_finalize(tts_engine* eng) {
  return guarded(eng, [&] {
    if (eng->finalized) return;
    const tts_config& cfg = eng->cfg;
    const GetData get = [&](const std::string& n) -> const std::vector<float>* {
      auto it = eng->host.find(n);
      return it == eng->host.end() ? nullptr : &it->second.data;
    };
    const GetShape shape = [&](const std::string& n) -> std::vector<int64_t> {
      auto it = eng->host.find(n);
      return it == eng->host.end() ? std::vector<int64_t>{} : it->second.shape;
    };
    eng->voc.finalize(get, shape, cfg.vocoder_dtype, &eng->prof);
    eng->ac.finalize(get, shape, cfg.acoustic_dtype,
                     cfg.encoder_precision == TTS_ENCODER_EXACT ? DT_F32 : cfg.acoustic_dtype, &eng->prof,
                     cfg.encoder_precision == TTS_ENCODER_EXACT && sw(SW_F32_ENC_SPLIT) != 0);
    if (!eng->voc.loaded() && !eng->ac.loaded) throw TtsError(TTS_ERR_STATE, "no known weights were set");
    eng->host.clear();
    eng->finalized = true;
    if (cfg.max_batch > 0 && cfg.max_frames > 0) eng->voc.reserve(cfg.max_batch, cfg.max_frames);
    if (eng->ac.loaded && cfg.max_batch > 0 && cfg.max_tokens > 0 && cfg.max_frames > 0)
      eng->ac.reserve(cfg.max_batch, cfg.max_tokens, cfg.max_frames);
  });
}

int tts_engine_reserve(tts_engine* eng, int max_batch, int max_frames, int max_tokens) {
  return guarded(eng, [&] {
    if (!eng->finalized) throw TtsError(TTS_ERR_STATE, "finalize first");
    if (max_batch <= 0 || max_frames <= 0) throw TtsError(TTS_ERR_INVALID, "bad reserve sizes");
    eng->voc.reserve(max_batch, max_frames);
    if (eng->ac.loaded && max_tokens > 0) eng->ac.reserve(max_batch, max_tokens, max_frames);
  });
}

void tts_engine_destroy(tts_engine* eng) { delete eng; }

int tts_vocoder_forward(tts_engine* eng, const float* d_mel, const int32_t* d_mel_lens, int B, int T,
                        float* d_wav, void* stream) {
  return guarded(eng, [&] {
    if (!eng->finalized) throw TtsError(TTS_ERR_STATE, "finalize first");
    if (!d_mel || !d_mel_lens || !d_wav || B <= 0 || T <= 0) throw TtsError(TTS_ERR_INVALID, "bad vocoder args");
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    eng->voc.forward(d_mel, d_mel_lens, B, T, d_wav, (long long)T * eng->voc.hop(), (hipStream_t)stream);
  });
}

int tts_vocoder_forward_chunk(tts_engine* eng, const float* d_mel, const int32_t* d_win_lens, int B, int T_win,
                              int ctx_left, int T_chunk, float* d_wav, void* stream) {
  return guarded(eng, [&] {
    if (!eng->finalized) throw TtsError(TTS_ERR_STATE, "finalize first");
    if (!d_mel || !d_win_lens || !d_wav || B <= 0 || T_win <= 0 || ctx_left < 0 || T_chunk <= 0 ||
        ctx_left + T_chunk > T_win)
      throw TtsError(TTS_ERR_INVALID, "bad chunk args");
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    eng->voc.forward_chunk(d_mel, d_win_lens, B, T_win, ctx_left, T_chunk, d_wav, (hipStream_t)stream);
  });
}

int tts_vocoder_context(tts_engine* eng, int* left, int* right) {
  return guarded([&] {  // host only: the engine is locked, but no device is selected and nothing is enqueued
    if (!eng) throw TtsError(TTS_ERR_INVALID, "null engine");
    if (!left || !right) throw TtsError(TTS_ERR_INVALID, "null left / right");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (!eng->finalized || !eng->voc.loaded()) throw TtsError(TTS_ERR_STATE, "vocoder weights not loaded/finalized");
    eng->voc.context(left, right);
  });
}

int tts_acoustic_forward_spk(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens, int B, int N,
                             const int32_t* d_dur_override, const float* d_spk_emb, int spk_dim, float* d_mel,
                             int32_t* d_mel_lens, int Tcap, int32_t* d_durations, void* stream) {
  return acoustic_forward_any(eng, d_tokens, d_tok_lens, B, N, d_dur_override, d_spk_emb, spk_dim, d_mel, d_mel_lens,
                              Tcap, d_durations, nullptr, stream);
}

int tts_acoustic_forward_ctl(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens, int B, int N,
                             const int32_t* d_dur_override, const float* d_spk_emb, int spk_dim, float* d_mel,
                             int32_t* d_mel_lens, int Tcap, int32_t* d_durations, const tts_prosody* ctl,
                             size_t ctl_size, void* stream) {
  VarianceCtl vc;
  const int bad = guarded([&] {  // a bad struct size is rejected before anything else (the engine included)
    if (ctl && !read_prosody(ctl, ctl_size, &vc))
      throw TtsError(TTS_ERR_INVALID, "tts_prosody of " + std::to_string(ctl_size) + " bytes: not a whole struct of this library's " +
                                          std::to_string(sizeof(tts_prosody)) + " bytes or an older, shorter one");
  });
  if (bad) return bad;
  return acoustic_forward_any(eng, d_tokens, d_tok_lens, B, N, d_dur_override, d_spk_emb, spk_dim, d_mel, d_mel_lens,
                              Tcap, d_durations, ctl ? &vc : nullptr, stream);
}

int tts_acoustic_forward(tts_engine* eng, const int32_t* d_tokens, const int32_t* d_tok_lens, int B, int N,
                         const int32_t* d_dur_override, float* d_mel, int32_t* d_mel_lens, int Tcap,
                         int32_t* d_durations, void* stream) {
  return tts_acoustic_forward_spk(eng, d_tokens, d_tok_lens, B, N, d_dur_override, nullptr, 0, d_mel, d_mel_lens,
                                  Tcap, d_durations, stream);
}

int tts_acoustic_speaker_dim(tts_engine* eng, int* dim) {
  return guarded(eng, [&] {
    if (!dim) throw TtsError(TTS_ERR_INVALID, "null dim");
    *dim = eng->ac.loaded ? eng->ac.speaker_dim() : 0;
  });
}

int tts_acoustic_range_flag(tts_engine* eng, int32_t* dst, void* stream) {
  return guarded(eng, [&] {
    if (!eng->finalized || !eng->ac.loaded) throw TtsError(TTS_ERR_STATE, "acoustic weights not loaded");
    if (!dst) throw TtsError(TTS_ERR_INVALID, "null dst");
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    eng->ac.range_flag_to(dst, (hipStream_t)stream);
  });
}

int tts_acoustic_set_precision(tts_engine* eng, int precision) {
  return guarded(eng, [&] {
    if (!eng->finalized || !eng->ac.loaded) throw TtsError(TTS_ERR_STATE, "acoustic weights not loaded");
    if (precision != TTS_ENCODER_EXACT && precision != TTS_ENCODER_F32)
      throw TtsError(TTS_ERR_INVALID, "precision must be TTS_ENCODER_EXACT or TTS_ENCODER_F32");
    if (!eng->ac.split_encoder())
      throw TtsError(TTS_ERR_INVALID, "only a model created with TTS_ENCODER_EXACT switches encoder precision");
    eng->ac.set_encoder_f32(precision == TTS_ENCODER_F32);
  });
}

int tts_engine_profile(tts_engine* eng, int enable) {
  return guarded(eng, [&] { eng->prof.on = enable != 0; });
}

int tts_engine_profile_read(tts_engine* eng, double* gemm_ms, double* gemm_flops, int* n_launches) {
  return guarded(eng, [&] { eng->prof.read(gemm_ms, gemm_flops, n_launches); });
}

int tts_set_switch(const char* name, int value) {
  return guarded([&] {
    if (tts::sw_set(name, value)) throw TtsError(TTS_ERR_INVALID, std::string("unknown switch: ") + (name ? name : "(null)"));
  });
}

int tts_get_switch(const char* name, int* value) {
  return guarded([&] {
    if (!value || tts::sw_get(name, value))
      throw TtsError(TTS_ERR_INVALID, std::string("unknown switch: ") + (name ? name : "(null)"));
  });
}

int tts_engine_profile_read_kinds(tts_engine* eng, int nkinds, double* ms, double* flops, int* n_launches) {
  return guarded(eng, [&] {
    if (nkinds < 1 || !ms || !flops || !n_launches) throw TtsError(TTS_ERR_INVALID, "profile_read_kinds: bad arguments");
    eng->prof.read_kinds(nkinds, ms, flops, n_launches);
  });
}

int tts_resample_filter(int up, int down, double* h, int cap, int* n_pre_remove) {
  int n = 0;
  const int rc = guarded([&] {
    if (up <= 0 || down <= 0) throw TtsError(TTS_ERR_INVALID, "resample: up/down must be positive");
    const ResampleFilter f = resample_filter(up, down);
    if (n_pre_remove) *n_pre_remove = f.n_pre_remove;
    if (h && cap >= f.n) std::copy(f.h.begin(), f.h.end(), h);
    n = f.n;
  });
  return rc ? rc : n;
}

int tts_resample_poly(tts_engine* eng, const float* d_in, int64_t in_stride, const int32_t* d_in_lens, int B,
                      int up, int down, float* d_out, int64_t out_stride, int out_cap, int32_t* d_out_lens,
                      void* stream) {
  return guarded(eng, [&] {
    if (!d_in || !d_in_lens || !d_out || B <= 0 || up <= 0 || down <= 0 || out_cap <= 0 || out_stride < out_cap)
      throw TtsError(TTS_ERR_INVALID, "bad resample args");
    const tts_engine::Resampler rs = resampler_for(eng, up, down);
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    HIP_CHECK(launch_resample_poly(d_in, in_stride, d_in_lens, B, rs.up, rs.down, rs.nq, rs.n_pre_remove, rs.hp, d_out,
                                   out_stride, out_cap, d_out_lens, (hipStream_t)stream));
  });
}

int tts_resample_history(int up, int down, int* n_hist, int* n_flush) {
  return guarded([&] {
    if (up <= 0 || down <= 0) throw TtsError(TTS_ERR_INVALID, "resample: up/down must be positive");
    const ResampleFilter f = resample_filter(up, down);
    if (n_hist) *n_hist = (f.n + f.up - 1) / f.up - 1;
    if (n_flush) *n_flush = f.n_pre_remove;
  });
}

int tts_resample_poly_chunk(tts_engine* eng, const float* d_in, int64_t in_stride, int64_t in_start, int in_count,
                            const int32_t* d_in_lens, int B, int up, int down, const float* d_hist_in,
                            float* d_hist_out, float* d_out, int64_t out_stride, int out_cap, int32_t* d_out_lens,
                            void* stream) {
  return guarded(eng, [&] {
    if (up <= 0 || down <= 0) throw TtsError(TTS_ERR_INVALID, "resample chunk: up/down must be positive");
    if (in_start < 0 || in_count < 0)
      throw TtsError(TTS_ERR_INVALID, "resample chunk: in_start and in_count must be non-negative");
    if (!d_in || !d_in_lens || !d_out || !d_hist_out || B <= 0 || in_stride < in_count || out_stride < out_cap)
      throw TtsError(TTS_ERR_INVALID, "bad resample chunk args");
    if (in_start > 0 && !d_hist_in)
      throw TtsError(TTS_ERR_INVALID, "resample chunk: a chunk after the first needs d_hist_in");
    if (d_hist_in == d_hist_out)
      throw TtsError(TTS_ERR_INVALID, "resample chunk: d_hist_out must not be d_hist_in");
    const tts_engine::Resampler rs = resampler_for(eng, up, down);
    const long long need = ((long long)in_count * rs.up + rs.down - 1) / rs.down + rs.n_pre_remove;
    if (out_cap < need)
      throw TtsError(TTS_ERR_INVALID, "resample chunk: out_cap " + std::to_string(out_cap) + " below ceil(in_count*up/down)"
                     " + n_flush = " + std::to_string(need));
    tts_engine::CallOrder order(eng, (hipStream_t)stream);
    HIP_CHECK(launch_resample_poly_chunk(d_in, in_stride, in_start, in_count, d_in_lens, B, rs.up, rs.down, rs.nq,
                                         rs.n_pre_remove, rs.hp, d_hist_in, d_hist_out, d_out, out_stride, out_cap,
                                         d_out_lens, (hipStream_t)stream));
  });
}

}  // extern "C"
