// HiFi-GAN vocoder runtime (vocoder.cpp): packed weights, workspace and the forward's launch plan.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "runtime.h"

namespace tts {

struct VocoderWeights {
  bool loaded = false;
  float* mean = nullptr;
  float* scale = nullptr;
  bool normalize = false;
  ConvLayer conv_pre;
  std::vector<ConvLayer> ups;  // per stage
  std::vector<int> up_rate;
  std::vector<int> stage_ch;
  // mrf[stage][block][pair][0=conv1,1=conv2]
  std::vector<std::vector<std::vector<std::array<ConvLayer, 2>>>> mrf;
  float* post_w = nullptr;  // fp32 [k][C]
  void* post_wh = nullptr;  // [k][C] in the vocoder dtype (16-bit conv_post kernel), or null
  float post_b = 0.f;
  int post_k = 7, post_c = 32;
  int hop = 256;
};

struct Vocoder {
  // packs the generator from the host weights; without "conv_pre.weight" the vocoder stays unloaded
  void finalize(const GetData& get, const GetShape& shape, int dtype, Profiler* prof);
  // the forward's workspace and forward_chunk's window buffer for [B][T] frames
  void reserve(int B, int T);
  // the generator's receptive field in mel frames (tts_vocoder_context)
  void context(int* left, int* right) const;
  // mel [B][T][Cin] fp32 -> wav [B] rows of swb floats, enqueued on s (the range guard below may sync)
  void forward(const float* mel, const int* mel_lens, int B, int T, float* wav, long long swb, hipStream_t s);
  // streaming: the forward over a window of T_win frames, then frames [ctx_left, ctx_left + T_chunk)
  // of its waveform to wav [B][T_chunk * hop]
  void forward_chunk(const float* mel, const int* win_lens, int B, int T_win, int ctx_left, int T_chunk, float* wav,
                     hipStream_t s);
  bool loaded() const { return w.loaded; }
  int hop() const { return w.hop; }
  ~Vocoder();

  static constexpr int VOC_MAX_STAGES = 7;
  VocoderWeights w;
  int dt = DT_F32;
  Profiler* prof = nullptr;
  std::vector<void*> allocs;  // weight allocations
  void* vbuf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // workspace: the forward's activation buffers
  size_t vbuf_elems = 0;
  void* vmel = nullptr;  // normalized mel in compute dtype
  size_t vmel_elems = 0;
  int* vlens = nullptr;  // [16][max_batch]: rows 0 .. 7 the stage lengths, 8 .. 15 the polyphase row counts
  int vlens_batch = 0;
  float* vchunk_wav = nullptr;  // streaming window output (forward_chunk): [B][T_win * hop] fp32
  size_t vchunk_elems = 0;
  // fp32 vocoder: split-K partials of the resblock convs with >= TTS_VWS_MIN_CIN input channels
  // (ConvParams::f32_splitk; at batch 1 -- C1 -- stage 0 at C = 256 ran on 54 blocks, stage 1 on 213)
  float* vws = nullptr;
  long long vws_bytes = 0;
  // fp32 vocoder: its wide resblock convs run as split-precision GEMMs (finalize), whose
  // operands must stay inside f16's range.  Their range word (vrange) is read back after each
  // forward (one stream sync, fp32 vocoders only); when set, the forward reruns with every layer
  // on the fp32 MFMA path (no_split) -- the vocoder counterpart of the exact encoder's guard.
  bool voc_split = false;
  int* vrange = nullptr;
  int* vrange_h = nullptr;  // pinned
  long long voc_range_fallbacks = 0;

  void reserve_workspace(int B, int T);
  void reserve_chunk(int B, int T_win);
  void forward_once(const float* mel, const int* mel_lens, int B, int T, float* wav, long long swb, hipStream_t s,
                    int no_split);
};

}  // namespace tts
