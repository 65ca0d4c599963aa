// HiFi-GAN vocoder runtime: weight packing, the supported envelope, workspace, the split layers'
// range guard and the forward's launch plan.
#include "vocoder.h"

#include <algorithm>
#include <cmath>

#include "switches.h"

#ifndef TTS_VWS_MIN_CIN
#define TTS_VWS_MIN_CIN 128  // (A/B builds: 64 with TTS_F32_SK_MINM=32)
#endif
#ifndef TTS_VOC_SPLIT_MINC
#define TTS_VOC_SPLIT_MINC 32  // fp32 vocoders: resblock convs with >= this many channels run split-precision
#endif

namespace tts {
namespace {

// TTS_MRF_FUSED=0 selects the unfused per-conv path (A/B and parity tests)
bool mrf_fused_enabled() { return sw(SW_MRF_FUSED) != 0; }
// resblock chain kernel for the HBM-bound resblocks (default on; TTS_MRF_CHAIN=0: pairs only)
bool mrf_chain_enabled() { return sw(SW_MRF_CHAIN) != 0; }
// conv_post inside the vocoder's last pair launch (default on; TTS_POST_FUSE=0: separate launch)
bool post_fuse_enabled() { return sw(SW_POST_FUSE) != 0; }
// streaming upsampler for the small stages (default on; TTS_UP_STREAM=0: conv_xres)
bool up_stream_enabled() { return sw(SW_UP_STREAM) != 0; }
bool up_fuse_enabled() { return sw(SW_UP_FUSE) != 0; }

constexpr float SLOPE = 0.1f;

// the engine's host weights, through finalize's getters
struct Host {
  const GetData& get_data;
  const GetShape& get_shape;
  bool has(const std::string& n) const { return get_data(n) != nullptr; }
  const std::vector<float>& data(const std::string& n) const {
    const std::vector<float>* p = get_data(n);
    if (!p) throw TtsError(TTS_ERR_STATE, "missing weight: " + n);
    return *p;
  }
  std::vector<int64_t> shape(const std::string& n) const { (void)data(n); return get_shape(n); }
};

void* track(Vocoder& voc, void* p) { voc.allocs.push_back(p); return p; }

// a workspace buffer of `have` units regrown to `need` units of `unit` bytes (never shrunk)
template <typename T, typename N>
void grow(T*& p, N& have, N need, size_t unit) {
  if (need <= have) return;
  if (p) dev_free(p);
  p = nullptr; have = 0;
  HIP_CHECK(dev_malloc(&p, (size_t)need * unit));
  have = need;
}

// nn.Conv1d weight [Cout][Cin][k] -> W[Cout][k][Cin]; split: an fp32 layer also gets the
// split-precision packing (three f16 MFMAs per product, conv_split.hip)
ConvLayer pack_conv(Vocoder& voc, const Host& h, const std::string& wname, const std::string& bname, int dil, int pad,
                    bool split = false) {
  const std::vector<int64_t> ws = h.shape(wname);
  if (ws.size() != 3) throw TtsError(TTS_ERR_INVALID, wname + ": expected 3-D conv weight");
  std::vector<float> b;
  if (!bname.empty() && h.has(bname)) b = h.data(bname);
  return make_conv(h.data(wname), (int)ws[0], (int)ws[1], (int)ws[2], b, dil, pad, voc.dt, voc.allocs, nullptr,
                   split && voc.dt == DT_F32);
}

// nn.ConvTranspose1d weight [Cin][Cout][k], stride s, padding p as a polyphase conv:
//   y[u*s + r - p][co] = b[co] + sum_{t<taps} sum_ci x[u + t - (taps-1)][ci] * W[ci][co][r + (taps-1-t)*s]
// i.e. M = s*Cout rows (r, co), taps = k/s, conv pad = taps-1 (oracle: conv_transpose1d).
ConvLayer pack_transposed(Vocoder& voc, const Host& h, const std::string& wname, const std::string& bname, int s) {
  const std::vector<float>& w = h.data(wname);
  const std::vector<int64_t> ws = h.shape(wname);
  const int ci = (int)ws[0], co = (int)ws[1], k = (int)ws[2], dt = voc.dt;
  const int taps = k / s;
  const int M = s * co;
  std::vector<float> p((size_t)M * taps * ci);
  for (int r = 0; r < s; ++r)
    for (int o = 0; o < co; ++o)
      for (int t = 0; t < taps; ++t) {
        const int j = r + (taps - 1 - t) * s;
        for (int c = 0; c < ci; ++c) p[(((size_t)(r * co + o)) * taps + t) * ci + c] = w[((size_t)c * co + o) * k + j];
      }
  ConvLayer L;
  L.w = track(voc, upload(p, dt));
  L.wpk = frag_pack(p, M, taps, ci, dt, voc.allocs);
  if (upsample_stream_supported(dt, ci, M, taps)) L.wup16 = frag_pack_up16(p, M, taps * ci, dt, voc.allocs);
  const auto& bh = h.data(bname);
  std::vector<float> b(M);
  for (int r = 0; r < s; ++r)
    for (int o = 0; o < co; ++o) b[r * co + o] = bh[o];
  L.bias = (float*)track(voc, upload_f32(b));
  L.M = M; L.Cin = ci; L.taps = taps; L.dil = 1; L.pad = taps - 1;
  L.up_s = s; L.up_cout = co; L.up_p = (k - s) / 2;
  return L;
}

struct VocoderShape {
  int nst = 0, nk = 0;                 // stages, resblocks per stage
  std::vector<int> stride;             // [nst]
  std::vector<std::vector<int>> dil;   // [nst * nk][pairs]: conv1's dilation of each pair
};

// check_vocoder_envelope's failure and its checks of one tensor
[[noreturn]] void bad(const std::string& what) { throw TtsError(TTS_ERR_INVALID, "vocoder envelope: " + what); }
std::vector<int64_t> dims(const Host& h, const std::string& n) {
  std::vector<int64_t> s = h.shape(n);
  if (s.size() != 3) bad(n + ": expected a 3-D conv weight");
  return s;
}
// 16-byte rows in every dtype (16-bit: 8 elements)
void ch16(const std::string& n, int64_t c, const char* which) {
  if (c <= 0 || c % 8) bad(n + ": " + which + " channel count " + std::to_string(c) +
                           " is not a multiple of 8 (rows of 16-byte pieces)");
}
void halo(const std::string& n, int64_t k, int64_t d) {
  if (k < 1 || k % 2 == 0) bad(n + ": kernel size " + std::to_string(k) + " is not odd");
  if ((k - 1) * d > CONV_HALO_MAX)
    bad(n + ": receptive field (k-1)*dilation = " + std::to_string((k - 1) * d) + " exceeds " +
        std::to_string(CONV_HALO_MAX) + " rows");
}

// one stage of check_vocoder_envelope: upsampler i (cin input channels) and its resblocks; returns
// the stage's channel count.  rates / dd / dds: the optional __cfg__ tables (dds: dd's shape)
int64_t check_stage(const Host& h, int i, int nk, int64_t cin, const std::vector<float>* rates,
                    const std::vector<float>* dd, const std::vector<int64_t>& dds, VocoderShape& vs) {
  const std::string un = "upsampler." + std::to_string(i) + ".weight";
  const auto us = dims(h, un);
  if (us[0] != cin) bad(un + ": " + std::to_string(us[0]) + " input channels after a layer of " + std::to_string(cin));
  ch16(un, us[1], "output");
  const int64_t k = us[2];
  const int64_t s = rates ? (int64_t)std::lround((*rates)[i]) : k / 2;
  if (s < 1 || k % s || (k - s) % 2)
    bad(un + ": kernel " + std::to_string(k) + " with stride " + std::to_string(s) +
        " (need k % stride == 0 and an even k - stride)");
  if (k / s - 1 > CONV_HALO_MAX)
    bad(un + ": " + std::to_string(k / s) + " taps per phase exceed " + std::to_string(CONV_HALO_MAX + 1));
  vs.stride.push_back((int)s);
  const std::string ub = "upsampler." + std::to_string(i) + ".bias";
  if (!h.has(ub) || (int64_t)h.data(ub).size() != us[1]) bad(ub + ": expected " + std::to_string(us[1]) + " values");
  const int64_t ch = us[1];
  for (int j = 0; j < nk; ++j) {
    const std::string rp = "resblocks." + std::to_string(i * nk + j) + ".";
    const int64_t ks = dims(h, rp + "convs1.0.weight")[2];
    int np = 0;
    while (h.has(rp + "convs1." + std::to_string(np) + ".weight")) ++np;
    if (!dd && np > 3)
      bad(rp + "convs1.3.weight: more than 3 pairs need __cfg__.resblock_dilation_sizes (the default is 1, 3, 5)");
    if (dd && dds[1] < np)
      bad("__cfg__.resblock_dilation_sizes: " + std::to_string(dds[1]) + " dilations for the " + std::to_string(np) +
          " pairs of " + rp + "convs1");
    vs.dil.emplace_back();
    for (int q = 0; q < np; ++q) {
      const int64_t d = dd ? (int64_t)std::lround((*dd)[(size_t)j * dds[1] + q]) : (q == 0 ? 1 : q == 1 ? 3 : 5);
      for (int cv = 0; cv < 2; ++cv) {
        const std::string wn = rp + (cv ? "convs2." : "convs1.") + std::to_string(q) + ".weight";
        if (!h.has(wn)) bad(wn + ": missing");
        const auto ws = dims(h, wn);
        if (ws[0] != ch || ws[1] != ch || ws[2] != ks)
          bad(wn + ": expected [" + std::to_string(ch) + "][" + std::to_string(ch) + "][" + std::to_string(ks) + "]");
        if (cv == 0 && d < 1) bad(wn + ": dilation " + std::to_string(d));
        halo(wn, ks, cv ? 1 : d);
      }
      vs.dil.back().push_back((int)d);
    }
  }
  return ch;
}

// The supported vocoder envelope, checked from the weight shapes and the
// configuration before anything is packed: a configuration passes only if every dtype and every
// kernel-path switch can run it, so nothing that loads fails at its first forward.  Each message
// names the tensor and the limit.  Returns what it read, which finalize packs from.
VocoderShape check_vocoder_envelope(const Host& h) {
  const auto pre = dims(h, "conv_pre.weight");
  ch16("conv_pre.weight", pre[1], "input");
  ch16("conv_pre.weight", pre[0], "output");
  if (pre[2] != 7) bad("conv_pre.weight: kernel size " + std::to_string(pre[2]) + "; conv_pre is padded for 7 taps");
  int nst = 0;
  while (h.has("upsampler." + std::to_string(nst) + ".weight")) ++nst;
  int nres = 0;
  while (h.has("resblocks." + std::to_string(nres) + ".convs1.0.weight")) ++nres;
  if (nst == 0 || nres == 0 || nres % nst)
    bad("resblocks.*: " + std::to_string(nres) + " resblocks do not divide over " + std::to_string(nst) +
        " upsampler stages");
  if (nst > Vocoder::VOC_MAX_STAGES)
    bad("upsampler." + std::to_string(Vocoder::VOC_MAX_STAGES) + ".weight: more than " +
        std::to_string(Vocoder::VOC_MAX_STAGES) + " stages");
  VocoderShape vs;
  vs.nst = nst; vs.nk = nres / nst;
  const std::vector<float>* rates = h.get_data("__cfg__.upsample_rates");
  if (rates && (int)rates->size() != nst)
    bad("__cfg__.upsample_rates: " + std::to_string(rates->size()) + " rates for " + std::to_string(nst) + " stages");
  const std::vector<float>* dd = h.get_data("__cfg__.resblock_dilation_sizes");
  const std::vector<int64_t> dds = dd ? h.shape("__cfg__.resblock_dilation_sizes") : std::vector<int64_t>();
  if (dd && (dds.size() != 2 || dds[0] != vs.nk))
    bad("__cfg__.resblock_dilation_sizes: expected [" + std::to_string(vs.nk) + "][pairs]");
  int64_t cin = pre[0];
  for (int i = 0; i < nst; ++i) cin = check_stage(h, i, vs.nk, cin, rates, dd, dds, vs);
  const auto ps = dims(h, "conv_post.weight");
  if (ps[0] != 1 || ps[1] != cin)
    bad("conv_post.weight: expected [1][" + std::to_string(cin) + "][k] after the last stage");
  if (ps[1] != CONV_POST_CHANNELS)
    bad("conv_post.weight: " + std::to_string(ps[1]) + " input channels; the conv_post kernels take a last stage of " +
        std::to_string(CONV_POST_CHANNELS));
  // (the conv_post kernels take any odd k and the fused form up to 17 taps, but only the 7 taps
  // of every HiFi-GAN generator have been run)
  if (ps[2] != 7) bad("conv_post.weight: kernel size " + std::to_string(ps[2]) + "; conv_post is tested at 7 taps only");
  return vs;
}

// stage i of finalize: the upsampler and its resblocks' conv pairs
void pack_stage(Vocoder& voc, const Host& h, const VocoderShape& vs, int i) {
  VocoderWeights& v = voc.w;
  const int nk = vs.nk, dt = voc.dt;
  const std::string up = "upsampler." + std::to_string(i);
  const int s = vs.stride[i];  // "__cfg__.upsample_rates" if given, else HiFi-GAN V1's k = 2*stride
  v.ups.push_back(pack_transposed(voc, h, up + ".weight", up + ".bias", s));
  v.up_rate.push_back(s);
  v.hop *= s;
  const int ch = (int)h.shape(up + ".weight")[1];
  v.stage_ch.push_back(ch);
  v.mrf[i].resize(nk);
  for (int j = 0; j < nk; ++j) {
    const std::string pre = "resblocks." + std::to_string(i * nk + j) + ".";
    const int ks = (int)h.shape(pre + "convs1.0.weight")[2];
    const std::vector<int>& dils = vs.dil[(size_t)i * nk + j];  // the table's, or the default 1, 3, 5
    const int np = (int)dils.size();
    v.mrf[i][j].resize(np);
    for (int q = 0; q < np; ++q) {
      const int d = dils[q];
      // fp32 vocoders: the wide stages' resblock convs (C >= TTS_VOC_SPLIT_MINC) as split-precision
      // GEMMs -- C1's batch-1 fp32 vocoder ran them on the fp32 MFMA at 15-25 TF/s
      const bool split = dt == DT_F32 && ch >= TTS_VOC_SPLIT_MINC && ch % 32 == 0;
      const std::string c1 = pre + "convs1." + std::to_string(q), c2 = pre + "convs2." + std::to_string(q);
      v.mrf[i][j][q][0] = pack_conv(voc, h, c1 + ".weight", c1 + ".bias", d, (ks * d - d) / 2, split);
      v.mrf[i][j][q][1] = pack_conv(voc, h, c2 + ".weight", c2 + ".bias", 1, (ks - 1) / 2, split);
      // pair-kernel copies (C in {32, 64}, 16-bit): 16x16 fragment-packed
      for (int cv = 0; cv < 2; ++cv) {
        const std::string wn = (cv ? c2 : c1) + ".weight";
        const std::vector<int64_t> cs = h.shape(wn);
        if (mrf_pair_supported(dt, ch, ks) && cs[0] == ch && cs[1] == ch)
          v.mrf[i][j][q][cv].wpk16 = frag_pack16(h.data(wn), ch, ks, dt, voc.allocs);
      }
    }
  }
}

}  // namespace

void Vocoder::finalize(const GetData& get, const GetShape& shape, int dtype, Profiler* prof_) {
  const Host h{get, shape};
  dt = dtype;
  prof = prof_;
  if (!h.has("conv_pre.weight")) return;
  const VocoderShape vs = check_vocoder_envelope(h);
  VocoderWeights& v = w;
  v.conv_pre = pack_conv(*this, h, "conv_pre.weight", "conv_pre.bias", 1, 3);
  if (h.has("mean") && h.has("scale")) {
    v.mean = (float*)track(*this, upload_f32(h.data("mean")));
    v.scale = (float*)track(*this, upload_f32(h.data("scale")));
    v.normalize = true;
  }
  v.hop = 1;
  v.ups.clear(); v.up_rate.clear(); v.stage_ch.clear(); v.mrf.assign(vs.nst, {});
  for (int i = 0; i < vs.nst; ++i) pack_stage(*this, h, vs, i);
  const std::vector<float>& pw = h.data("conv_post.weight");  // [1][C][k]
  const std::vector<int64_t> ps = h.shape("conv_post.weight");
  v.post_c = (int)ps[1];
  v.post_k = (int)ps[2];
  std::vector<float> t((size_t)v.post_k * v.post_c);
  for (int c = 0; c < v.post_c; ++c)
    for (int j = 0; j < v.post_k; ++j) t[(size_t)j * v.post_c + c] = pw[(size_t)c * v.post_k + j];
  v.post_w = (float*)track(*this, upload_f32(t));
  v.post_wh = dt == DT_F32 ? nullptr : track(*this, upload(t, dt));
  v.post_b = h.data("conv_post.bias")[0];
  voc_split = false;
  for (const auto& st : v.mrf)
    for (const auto& rb : st)
      for (const auto& pr : rb) voc_split = voc_split || (dt == DT_F32 && (pr[0].wpk || pr[1].wpk));
  if (voc_split && !vrange) {
    HIP_CHECK(dev_malloc(&vrange, 16));
    HIP_CHECK(hipMemset(vrange, 0, 16));
    track(*this, vrange);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&vrange_h), 16, hipHostMallocDefault));
  }
  v.loaded = true;
}

Vocoder::~Vocoder() {
  for (void* p : allocs) dev_free(p);
  for (void*& p : vbuf) if (p) dev_free(p);
  if (vmel) dev_free(vmel);
  if (vlens) dev_free(vlens);
  if (vchunk_wav) dev_free(vchunk_wav);
  if (vws) dev_free(vws);
  if (vrange_h) hipHostFree(vrange_h);
}

// From the packed layers: the last stage's rows [0, hop - 1] of one frame, taken back through
// every layer in exact integer interval arithmetic.  A conv of `taps` taps, dilation d and left
// padding `pad` reads rows [a - pad, b + (taps-1)*d - pad]; a transposed conv (k = taps*s, stride
// s, padding p) writes output row `to` from the input rows ti with 0 <= to + p - ti*s <= k - 1.
void Vocoder::context(int* left, int* right) const {
  auto fdiv = [](long long x, long long y) { return x >= 0 ? x / y : -((-x + y - 1) / y); };  // floor, y > 0
  auto conv = [](const ConvLayer& L, long long& a, long long& b) {
    a -= L.pad;
    b += (long long)(L.taps - 1) * L.dil - L.pad;
  };
  long long a = -(long long)((w.post_k - 1) / 2), b = w.hop - 1 + (w.post_k - 1) / 2;
  for (int i = (int)w.ups.size() - 1; i >= 0; --i) {
    long long lo = a, hi = b;
    for (const auto& blk : w.mrf[i]) {  // the resblocks read the same rows: the widest counts
      long long ba = a, bb = b;
      for (size_t q = blk.size(); q-- > 0;) {
        conv(blk[q][1], ba, bb);
        conv(blk[q][0], ba, bb);
      }
      lo = std::min(lo, ba);
      hi = std::max(hi, bb);
    }
    const ConvLayer& U = w.ups[i];
    const long long s = U.up_s, k = (long long)U.taps * U.up_s, p = U.up_p;
    a = -fdiv(-(lo + p - (k - 1)), s);  // ceil
    b = fdiv(hi + p, s);
  }
  conv(w.conv_pre, a, b);
  *left = (int)-a;
  *right = (int)b;
}

void Vocoder::reserve(int B, int T) {
  if (!w.loaded) return;
  reserve_workspace(B, T);
  reserve_chunk(B, T);
}

void Vocoder::reserve_workspace(int B, int T) {
  size_t per_frame = (size_t)w.conv_pre.M;  // conv_pre output channels
  size_t cum = 1;
  for (size_t i = 0; i < w.ups.size(); ++i) {
    cum *= w.up_rate[i];
    per_frame = std::max(per_frame, cum * w.stage_ch[i]);
  }
  const size_t need = (size_t)B * T * per_frame;
  if (need > vbuf_elems) {
    for (void*& p : vbuf) { if (p) dev_free(p); p = nullptr; }
    vbuf_elems = 0;
    for (void*& p : vbuf) {
      if (dev_malloc(&p, need * dtype_size(dt)) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        for (void*& q : vbuf) { if (q) dev_free(q); q = nullptr; }  // release the partial set
        throw TtsError(TTS_ERR_HIP, "vocoder workspace: hipMalloc of " + std::to_string(need * dtype_size(dt)) +
                                        " bytes failed");
      }
    }
    vbuf_elems = need;
  }
  grow(vmel, vmel_elems, (size_t)B * T * w.conv_pre.Cin, dtype_size(dt));
  if (dt == DT_F32) {  // split-K partials of the fp32 resblock convs (run_conv)
    long long wsb = 0;
    size_t cum2 = 1;
    for (size_t i = 0; i < w.ups.size(); ++i) {
      cum2 *= w.up_rate[i];
      const int C = w.stage_ch[i];
      if (C >= TTS_VWS_MIN_CIN) wsb = std::max(wsb, f32_splitk_ws_bytes(3, C, C, (long long)B * T * (long long)cum2));
    }
    grow(vws, vws_bytes, wsb, 1);
  }
  grow(vlens, vlens_batch, B, sizeof(int) * 16);
}

void Vocoder::reserve_chunk(int B, int T_win) {
  const size_t need = (size_t)B * T_win * w.hop;
  if (need <= vchunk_elems) return;
  float* old = vchunk_wav;
  vchunk_wav = nullptr; vchunk_elems = 0;
  if (old) HIP_CHECK(dev_free(old));
  HIP_CHECK(dev_malloc(&vchunk_wav, need * 4));
  vchunk_elems = need;
}

// The forward with the split layers' range guard (fp32 vocoders with split-packed convs): one
// read of the range word after the forward, and a rerun on the fp32 MFMA path when it is set.
void Vocoder::forward(const float* mel, const int* mel_lens, int B, int T, float* wav, long long swb, hipStream_t s) {
  if (!voc_split) return forward_once(mel, mel_lens, B, T, wav, swb, s, 0);
  HIP_CHECK(hipMemsetAsync(vrange, 0, 4, s));
  forward_once(mel, mel_lens, B, T, wav, swb, s, 0);
  HIP_CHECK(hipMemcpyAsync(vrange_h, vrange, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (*vrange_h == 0) return;
  ++voc_range_fallbacks;
  forward_once(mel, mel_lens, B, T, wav, swb, s, 1);
}

void Vocoder::forward_chunk(const float* mel, const int* win_lens, int B, int T_win, int ctx_left, int T_chunk,
                            float* wav, hipStream_t s) {
  reserve_chunk(B, T_win);
  forward(mel, win_lens, B, T_win, vchunk_wav, (long long)T_win * w.hop, s);
  HIP_CHECK(hipMemcpy2DAsync(wav, (size_t)T_chunk * w.hop * 4, vchunk_wav + (size_t)ctx_left * w.hop,
                             (size_t)T_win * w.hop * 4, (size_t)T_chunk * w.hop * 4, B, hipMemcpyDeviceToDevice, s));
}

namespace {

// polyphase rows of upsampler i: input row u writes output rows s*u + r - p (r < s), so the
// last output row len*s - 1 needs u up to len + (p - 1) / s: one row past the input for
// p <= s (k <= 3 s), more for longer kernels
int up_extra(const VocoderWeights& v, int i) {
  return 1 + (v.ups[i].up_p > 0 ? (v.ups[i].up_p - 1) / v.ups[i].up_s : 0);
}

// per-stage lengths into vlens: L[i] = len * cum_i (frames of stage i), U[i] = L[i] + up_extra(i)
// (polyphase rows)
void stage_lengths(Vocoder& voc, const int* mel_lens, int B, int T, hipStream_t s) {
  const VocoderWeights& v = voc.w;
  const int nst = (int)v.ups.size();
  if (nst > Vocoder::VOC_MAX_STAGES) throw TtsError(TTS_ERR_INVALID, "too many stages");
  int mult[8], add[8], n = 0;
  int cum = 1;
  mult[n] = 1; add[n] = 0; ++n;  // L0
  for (int i = 0; i < nst; ++i) { cum *= v.up_rate[i]; mult[n] = cum; add[n] = 0; ++n; }
  HIP_CHECK(launch_lens(mel_lens, voc.vlens, B, mult, add, n, T, s));
  cum = 1;
  for (int i = 0; i < nst; ++i) { mult[i] = cum; add[i] = up_extra(v, i); cum *= v.up_rate[i]; }
  HIP_CHECK(launch_lens(mel_lens, voc.vlens + 8 * B, B, mult, add, nst, T, s));
}

// One forward's launch plan and its state.  Activations are [B][rows][C] in the vocoder dtype.
struct Fwd {
  Vocoder& voc;
  const VocoderWeights& v;
  const int B, dt, nst, no_split;  // no_split: the range guard's fallback, split-packed layers on the fp32 MFMA path
  const hipStream_t s;
  float* const wav;  // conv_post's output: [B] rows of swb floats
  const long long swb;
  // XS: the stage's upsampled x; T1: conv1's output; HA / HB: the pairs' alternating outputs;
  // S: the MRF sum, the next stage's input
  void *const XS, *const T1, *const HA, *const HB, *const S;
  int Tin, cin;  // rows and channels of S entering the stage
  // the stage in hand: its channels, rows, batch stride and resblocks
  int ch = 0, Tout = 0, nk = 0;
  long long sb = 0;
  // whether S already holds lrelu(S) for the next upsampler (conv_pre, or a stage whose final MRF
  // sum came from a pair launch that applied it, MrfPairParams::out_act); the upsampler then
  // loads it as is, so the X-resident upsamplers can stage it by LDS-DMA
  bool s_act = true;
  bool post_done = false;  // conv_post ran inside the last pair launch
  bool up_done = false;    // this stage's upsampler ran inside the previous stage's last pair launch (XS is written)
  int* Lp(int i) const { return voc.vlens + i * B; }        // stage lengths
  int* Up(int i) const { return voc.vlens + (8 + i) * B; }  // polyphase rows of upsampler i

  // one implicit-GEMM conv of the forward: x [B][x_rows] -> y [B][y_rows] (+ residuals r1, r2 laid out
  // by srb / srr); up_len: a transposed conv's output lengths
  void run_conv(const ConvLayer& L, const void* x, long long sxb, int sxr, const int* x_len, int x_rows, void* y,
                long long syb, int syr, const int* y_len, int y_rows, float in_slope, const void* r1, const void* r2,
                long long srb, int srr, float out_scale, const int* up_len, int act_out = ACT_NONE,
                float out_slope = 0.f) {
    ConvParams p = conv_params_default();
    p.act_out = act_out; p.out_slope = out_slope;
    p.x = x; p.sxb = sxb; p.sxr = sxr; p.x_len = x_len; p.x_rows = x_rows;
    p.w = L.w; p.w_ld = L.taps * L.Cin; p.wpk = L.wpk; p.w_unscale = L.wpk_unscale;
    p.range_flag = voc.vrange;  // the split-precision layers' range guard (Vocoder::forward)
    p.no_split = no_split;
    p.bias = L.bias;
    p.y = y; p.syb = syb; p.syr = syr;
    p.r1 = r1; p.r2 = r2; p.srb = srb; p.srr = srr;
    p.y_len = y_len; p.y_rows = y_rows;
    p.M = L.M; p.Cin = L.Cin; p.taps = L.taps; p.dil = L.dil; p.pad = L.pad;
    p.in_slope = in_slope; p.out_scale = out_scale;
    p.up_s = L.up_s; p.up_cout = L.up_cout; p.up_p = L.up_p; p.up_len = up_len;
    p.B = B;
    if (dt == DT_F32 && L.Cin >= TTS_VWS_MIN_CIN && !L.up_s && voc.vws) {  // (a layer-shape rule: batch-independent sums)
      p.f32_splitk = 1; p.ws = voc.vws; p.ws_bytes = voc.vws_bytes;
    }
    // algorithmic FLOPs: 2 * Cout * Cin * k per produced row (transposed: per input row, all phases)
    const double fl = 2.0 * L.M * (double)L.Cin * L.taps * (double)B * (L.up_s ? x_rows : y_rows);
    launch_conv_checked(p, dt, s, voc.prof, fl);
  }

  // lrelu -> ConvTranspose1d (polyphase): S -> XS
  void run_upsampler(int i) {
    const ConvLayer& U = v.ups[i];
    const float slope = s_act ? 1.f : SLOPE;
    if (up_done) {
      up_done = false;
    } else if (U.wup16 && up_stream_enabled()) {
      UpsampleParams up{};
      up.x = S; up.sxb = (long long)Tin * cin; up.len = Lp(i); up.up_len = Lp(i + 1);
      up.wpk = U.wup16; up.bias = U.bias; up.y = XS; up.syb = sb;
      up.T = Tin; up.B = B; up.s = U.up_s; up.co = U.up_cout; up.pad = U.up_p; up.slope = slope;
      const double fl = 2.0 * U.M * (double)U.Cin * U.taps * (double)B * Tin;
      voc.prof->launch(PK_UPSAMPLE, fl, s, [&] { return upsample_stream_launch(dt, U.Cin, U.M, up, s); });
    } else {
      run_conv(U, S, (long long)Tin * cin, cin, Lp(i), Tin, XS, sb, ch, Up(i), Tin + up_extra(v, i), slope, nullptr,
               nullptr, 0, 0, 1.f, Lp(i + 1));
    }
    s_act = false;  // until this stage's final MRF sum says otherwise
  }

  // resblock j as single convs: lrelu(h) -> T1 -> conv2 + h (the last one accumulates into S)
  void resblock_convs(int i, int j) {
    const auto& blk = v.mrf[i][j];
    const int np = (int)blk.size();
    const int* len = Lp(i + 1);
    const void* h = XS;
    for (int q = 0; q < np; ++q) {
      run_conv(blk[q][0], h, sb, ch, len, Tout, T1, sb, ch, len, Tout, SLOPE, nullptr, nullptr, 0, 0, 1.f, nullptr);
      const bool last = q == np - 1;
      void* out = last ? S : (q % 2 == 0 ? HA : HB);
      const void* r2 = (last && j > 0) ? S : nullptr;
      const float sc = (last && j == nk - 1) ? 1.0f / (float)nk : 1.f;
      run_conv(blk[q][1], T1, sb, ch, len, Tout, out, sb, ch, len, Tout, SLOPE, h, r2, sb, ch, sc, nullptr);
      h = out;
    }
  }

  // the whole resblock in one launch (HBM-bound resblocks: k = 3 at C <= 64, k = 7 at C = 32)
  void resblock_chain(int i, int j) {
    const auto& blk = v.mrf[i][j];
    const int taps = blk[0][0].taps;
    MrfChainParams cp{};
    cp.x = XS; cp.y = S; cp.len = Lp(i + 1);
    for (int q = 0; q < 3; ++q) {
      cp.w1[q] = blk[q][0].wpk16; cp.w2[q] = blk[q][1].wpk16;
      cp.b1[q] = blk[q][0].bias; cp.b2[q] = blk[q][1].bias;
    }
    cp.T = Tout; cp.B = B; cp.slope = SLOPE;
    cp.accum = j > 0 ? 1 : 0;
    cp.scale = j == nk - 1 ? 1.0f / (float)nk : 1.f;
    const double fl = 2.0 * 2.0 * ch * (double)ch * taps * (double)B * Tout * (int)blk.size();
    voc.prof->launch(PK_MRF_CHAIN, fl, s, [&] { return mrf_chain_launch(dt, ch, taps, cp, s); });
  }

  // resblock j as pair launches: X -> HA -> HB -> S; S accumulates over resblocks.  The stage's last
  // launch may also carry conv_post, the activated store or the next stage's upsampler.
  void resblock_pairs(int i, int j) {
    const auto& blk = v.mrf[i][j];
    const int np = (int)blk.size();
    const void* h = XS;
    for (int q = 0; q < np; ++q) {
      const bool last = q == np - 1;
      MrfPairParams pp{};
      pp.x = h;
      pp.y = last ? S : (q % 2 == 0 ? HA : HB);
      pp.len = Lp(i + 1);
      pp.w1 = blk[q][0].wpk16; pp.w2 = blk[q][1].wpk16;
      pp.b1 = blk[q][0].bias; pp.b2 = blk[q][1].bias;
      pp.T = Tout; pp.B = B; pp.k = blk[q][0].taps; pp.d = blk[q][0].dil;
      pp.slope = SLOPE;
      pp.tbuf = T1;  // (free in the pair path: the channel-split form's t rows)
      pp.accum = (last && j > 0) ? 1 : 0;
      pp.scale = (last && j == nk - 1) ? 1.0f / (float)nk : 1.f;
      if (last && j == nk - 1 && i == nst - 1 && v.post_wh && post_fuse_enabled() &&
          mrf_pair_post_supported(dt, ch, v.post_k)) {
        // the final MRF sum goes straight into conv_post; S is not written
        pp.post_wpk = v.post_wh; pp.post_b = v.post_b; pp.post_slope = 0.01f; pp.post_k = v.post_k;
        pp.wav = wav; pp.swb = swb;
        post_done = true;
      }
      double fl = 2.0 * 2.0 * ch * (double)ch * pp.k * (double)B * Tout;
      // the stage's final MRF sum feeds only the next upsampler: store it activated
      if (last && j == nk - 1 && i + 1 < nst && !pp.post_wpk && mrf_pair_outact_supported(dt, ch, pp.k)) {
        pp.out_act = 1; pp.out_slope = SLOPE;
        s_act = true;
        // ... or, on full-height tiles, run that upsampler in this launch: XS (last read by the
        // third resblock's first pair) receives the next stage's x, S is only read
        const ConvLayer& N = v.ups[i + 1];
        if (N.wup16 && up_stream_enabled() && up_fuse_enabled() && N.Cin == ch && N.M == ch && N.taps == 2 &&
            pp.x != XS && mrf_pair_up_supported(dt, ch, pp)) {
          pp.up_wpk = N.wup16; pp.up_bias = N.bias; pp.up_y = XS;
          pp.up_syb = (long long)Tout * v.up_rate[i + 1] * v.stage_ch[i + 1];
          pp.up_len = Lp(i + 2); pp.up_s = N.up_s; pp.up_co = N.up_cout; pp.up_pad = N.up_p;
          fl += 2.0 * N.M * (double)N.Cin * N.taps * (double)B * Tout;  // the upsample launch's count
          up_done = true;
        }
      }
      voc.prof->launch(PK_MRF_PAIR, fl, s, [&] { return mrf_pair_launch(dt, ch, pp, s); });
      h = pp.y;
    }
  }

  bool pair_capable(int i, int j) const {
    const auto& blk = v.mrf[i][j];
    return std::all_of(blk.begin(), blk.end(), [](const auto& pr) { return pr[0].wpk16 && pr[1].wpk16; });
  }

  // stage i's resblocks: with the fused path on and a pair kernel for any of them, each capable
  // resblock runs as one chain launch or as pair launches, and one without a pair kernel (its k) as
  // single convs in the same S order; otherwise all run as single convs
  void run_resblocks(int i) {
    bool pair_ok = false;
    if (mrf_fused_enabled())
      for (int j = 0; j < nk; ++j) pair_ok = pair_ok || pair_capable(i, j);
    for (int j = 0; j < nk; ++j) {
      const auto& blk = v.mrf[i][j];
      const int np = (int)blk.size();
      int dil[4] = {0, 0, 0, 0};
      for (int q = 0; q < np && q < 4; ++q) dil[q] = blk[q][0].dil;
      if (!pair_ok || !pair_capable(i, j))
        resblock_convs(i, j);
      else if (mrf_chain_enabled() && mrf_chain_supported(dt, ch, blk[0][0].taps, dil, np))
        resblock_chain(i, j);
      else
        resblock_pairs(i, j);
    }
  }
};

}  // namespace

// HiFi-GAN V1 forward (oracle/vocoder.py vocoder_forward; HF:1435-1475).
void Vocoder::forward_once(const float* mel, const int* mel_lens, int B, int T, float* wav, long long swb,
                           hipStream_t s, int no_split) {
  if (!w.loaded) throw TtsError(TTS_ERR_STATE, "vocoder weights not loaded/finalized");
  reserve_workspace(B, T);
  const VocoderWeights& v = w;
  stage_lengths(*this, mel_lens, B, T, s);
  const int cin0 = v.conv_pre.Cin, c0 = v.conv_pre.M;
  HIP_CHECK(launch_mel_in(dt, mel, (long long)T * cin0, cin0, v.normalize ? v.mean : nullptr, v.scale, vmel, B, T,
                          cin0, s));
  Fwd st{*this, v, B, dt, (int)v.ups.size(), no_split, s, wav, swb, vbuf[0], vbuf[1], vbuf[2], vbuf[3], vbuf[4], T, c0};
  // conv_pre: [B][T][80] -> S [B][T][512], stored as lrelu(x, 0.1) -- the activation the first
  // upsampler applies (HF:1455-1458), in the conv's fp32 epilogue: S feeds nothing else
  st.run_conv(v.conv_pre, vmel, (long long)T * cin0, cin0, st.Lp(0), T, st.S, (long long)T * c0, c0, st.Lp(0), T, 1.f,
              nullptr, nullptr, 0, 0, 1.f, nullptr, ACT_LRELU, SLOPE);
  for (int i = 0; i < st.nst; ++i) {
    st.ch = v.stage_ch[i];
    st.Tout = st.Tin * v.up_rate[i];
    st.nk = (int)v.mrf[i].size();
    st.sb = (long long)st.Tout * st.ch;
    st.run_upsampler(i);
    st.run_resblocks(i);
    st.Tin = st.Tout;
    st.cin = st.ch;
  }
  if (!st.post_done)
    HIP_CHECK(launch_conv_post(dt, st.S, st.Lp(st.nst), B, st.Tin, st.cin, v.post_w, v.post_wh, v.post_b, v.post_k,
                               0.01f, wav, swb, s));
}

}  // namespace tts

