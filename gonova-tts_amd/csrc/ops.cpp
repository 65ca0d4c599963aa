// Op-level C entries (tts_op_*, include/tts_hip.h): single kernels and launchers as the tests call
// them.  Each validates what its launcher assumes and its kernel would otherwise read or write out
// of bounds on, then enqueues the one launch the model makes.
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "acoustic_kernels.h"
#include "capi.h"

using namespace tts;

// op-level conv layer (tts_op_conv_layer_create): one make_conv result and the buffers it owns
struct tts_conv_layer {
  int dtype = DT_F32;
  ConvLayer layer;
  std::vector<void*> allocs;
};

namespace {

void op_require(bool ok, const char* op, const std::string& what) {
  if (!ok) throw TtsError(TTS_ERR_INVALID, std::string(op) + ": " + what);
}

void op_dtype(int dt, const char* op) {
  op_require(dt == DT_F32 || dt == DT_F16 || dt == DT_BF16, op, "bad dtype");
}

std::string op_dims(std::initializer_list<std::pair<const char*, long long>> v) {
  std::string s = " (";
  for (const auto& p : v) s += std::string(s.size() > 2 ? ", " : "") + p.first + " " + std::to_string(p.second);
  return s + ")";
}

constexpr int OP_MAX_GRID_YZ = 65535;

// the activations, epilogue and batch of a tts_conv_desc; the caller adds the weights and the
// layer's shape (the desc's own, or a packed layer's)
ConvParams conv_params_of(const tts_conv_desc* d) {
  ConvParams p = conv_params_default();
  p.x = d->x; p.sxb = d->sxb; p.sxr = d->sxr; p.x_len = d->x_len; p.x_rows = d->x_rows;
  p.y = d->y; p.syb = d->syb; p.syr = d->syr;
  p.r1 = d->r1; p.r2 = d->r2; p.srb = d->srb; p.srr = d->srr;
  p.y_len = d->y_len; p.y_rows = d->y_rows;
  p.in_slope = d->in_slope; p.act_out = d->act_out; p.out_slope = d->out_slope;
  p.alpha = d->alpha; p.out_scale = d->out_scale;
  p.B = d->B;
  return p;
}

}  // namespace

extern "C" {

int tts_op_conv1d(int dtype, const tts_conv_desc* d, void* stream) {
  return guarded([&] {
    if (!d) throw TtsError(TTS_ERR_INVALID, "null desc");
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) throw TtsError(TTS_ERR_INVALID, "bad dtype");
    ConvParams p = conv_params_of(d);
    p.w = d->w; p.swb = d->swb; p.w_ld = d->w_ld; p.bias = d->bias;
    p.M = d->M; p.Cin = d->Cin; p.taps = d->taps; p.dil = d->dil; p.pad = d->pad;
    p.up_s = d->up_s; p.up_cout = d->up_cout; p.up_p = d->up_p; p.up_len = d->up_len;
    launch_conv_checked(p, dtype, (hipStream_t)stream, nullptr, 0.0);
  });
}

int tts_op_conv_layer_create(int dtype, int split, const float* w, const float* bias, int M, int Cin, int k, int dil,
                             int pad, tts_conv_layer** layer) {
  return guarded([&] {
    if (!layer) throw TtsError(TTS_ERR_INVALID, "conv layer: null out pointer");
    *layer = nullptr;
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) throw TtsError(TTS_ERR_INVALID, "conv layer: bad dtype");
    if (split && dtype != DT_F32) throw TtsError(TTS_ERR_INVALID, "conv layer: the split form takes an fp32 layer");
    if (!w || M <= 0 || Cin <= 0 || k <= 0 || dil <= 0 || pad < 0)
      throw TtsError(TTS_ERR_INVALID, "conv layer: bad dims");
    const std::vector<float> wv(w, w + (size_t)M * Cin * k);
    const std::vector<float> bv = bias ? std::vector<float>(bias, bias + M) : std::vector<float>();
    // (a throw midway releases the buffers make_conv had allocated)
    std::unique_ptr<tts_conv_layer, void (*)(tts_conv_layer*)> L(new tts_conv_layer, tts_op_conv_layer_destroy);
    L->dtype = dtype;
    L->layer = make_conv(wv, M, Cin, k, bv, dil, pad, dtype, L->allocs, nullptr, split != 0);  // finalize's packing
    *layer = L.release();
  });
}

void tts_op_conv_layer_destroy(tts_conv_layer* layer) {
  if (!layer) return;
  for (void* p : layer->allocs) (void)dev_free(p);
  delete layer;
}

int64_t tts_op_conv_ws_bytes(int taps, int Cin, int M, int rows) {
  if (taps <= 0 || Cin <= 0 || M <= 0 || rows <= 0) return 0;
  return std::max(conv_split_ws_bytes(taps, Cin, M, rows), f32_splitk_ws_bytes(taps, Cin, M, rows));
}

int tts_op_conv1d_ex(const tts_conv_layer* layer, const tts_conv_desc* d, tts_conv_ext* x, void* stream) {
  return guarded([&] {
    if (!layer || !d) throw TtsError(TTS_ERR_INVALID, "conv1d_ex: null layer or desc");
    if (d->up_s) throw TtsError(TTS_ERR_INVALID, "conv1d_ex: the transposed-conv mapping (up_s) is not taken here");
    if (!d->x || !d->y || d->B <= 0) throw TtsError(TTS_ERR_INVALID, "conv1d_ex: null buffer or empty batch");
    const ConvLayer& L = layer->layer;
    ConvParams p = conv_params_of(d);
    p.w = L.w; p.w_ld = L.taps * L.Cin; p.bias = L.bias; p.wpk = L.wpk; p.w_unscale = L.wpk_unscale;
    p.M = L.M; p.Cin = L.Cin; p.taps = L.taps; p.dil = L.dil; p.pad = L.pad;
    if (x) {
      if (x->rows_pad < 0 || x->ws_bytes < 0 || (x->ws_bytes > 0 && !x->ws) || x->ln_cnt_n < 0 || (x->ln_cnt_n > 0 && !x->ln_cnt))
        throw TtsError(TTS_ERR_INVALID, "conv1d_ex: bad rows_pad / workspace / counters");
      if ((x->ln_out || x->ln_lin_out) && (!x->ln_g1 || !x->ln_b1))
        throw TtsError(TTS_ERR_INVALID, "conv1d_ex: a LayerNorm needs ln_g1 and ln_b1");
      if ((x->ln_g2 != nullptr) != (x->ln_b2 != nullptr))
        throw TtsError(TTS_ERR_INVALID, "conv1d_ex: ln_g2 and ln_b2 come together");
      if (x->ln_lin_out && (!x->ln_lin_w || x->ln_out || x->ln_g2))
        throw TtsError(TTS_ERR_INVALID, "conv1d_ex: ln_lin_out takes ln_lin_w, one LayerNorm and no ln_out");
      p.rows_pad = x->rows_pad; p.ws = (float*)x->ws; p.ws_bytes = x->ws ? x->ws_bytes : 0;
      p.f32_splitk = x->f32_splitk; p.no_split = x->no_split; p.range_flag = x->range_flag;
      p.ln_out = x->ln_out; p.ln_g1 = x->ln_g1; p.ln_b1 = x->ln_b1; p.ln_g2 = x->ln_g2; p.ln_b2 = x->ln_b2;
      p.ln_eps = x->ln_eps; p.ln_cnt = x->ln_cnt_n > 0 ? x->ln_cnt : nullptr; p.ln_cnt_n = x->ln_cnt_n;
      p.ln_lin_w = x->ln_lin_w; p.ln_lin_b = x->ln_lin_b; p.ln_lin_out = x->ln_lin_out;
    }
    launch_conv_checked(p, layer->dtype, (hipStream_t)stream, nullptr, 0.0);
    if (x) {
      x->kind = conv_gemm_kind(layer->dtype, p);
      x->kernels = conv_last_kernels();
    }
  });
}

int64_t tts_op_rel_attn_ws_bytes(int B, int Tm, int Tp, int D, int H) {
  if (B <= 0 || Tm <= 0 || Tp < Tm || D <= 0 || H <= 0) return 0;
  return rel_attn_f32_ws_bytes(B, Tm, Tp, D, H);
}

int tts_op_rel_attn(int dtype, int split, const float* pos_u, const float* pos_v, const void* qkv, const void* ptab,
                    const int32_t* lens, int B, int Tm, int Tp, int D, int H, int rmax, float scale, void* out,
                    int32_t* range_flag, void* ws, int64_t ws_bytes, void* stream) {
  return guarded([&] {
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) throw TtsError(TTS_ERR_INVALID, "rel_attn: bad dtype");
    if (split && dtype != DT_F32) throw TtsError(TTS_ERR_INVALID, "rel_attn: the split form takes fp32 operands");
    if (!pos_u || !pos_v || !qkv || !ptab || !lens || !out) throw TtsError(TTS_ERR_INVALID, "rel_attn: null buffer");
    if (B <= 0 || Tm <= 0 || Tp < Tm)
      throw TtsError(TTS_ERR_INVALID, "rel_attn: needs B > 0 and 0 < Tm <= Tp (B " + std::to_string(B) + ", Tm " +
                                          std::to_string(Tm) + ", Tp " + std::to_string(Tp) + ")");
    if (rmax < Tm)
      throw TtsError(TTS_ERR_INVALID, "rel_attn: position table of rmax " + std::to_string(rmax) + " below Tm " + std::to_string(Tm));
    if (H <= 0 || D <= 0 || !rel_attn_supported(dtype, D, H))
      throw TtsError(TTS_ERR_INVALID, "rel_attn: D " + std::to_string(D) + " / H " + std::to_string(H) +
                                          " is not a head size the fused attention takes (192)");
    if (ws_bytes < 0 || (ws_bytes > 0 && !ws)) throw TtsError(TTS_ERR_INVALID, "rel_attn: bad workspace");
    HIP_CHECK(launch_rel_attn(dtype, split != 0, pos_u, pos_v, qkv, ptab, lens, B, Tm, Tp, D, H, rmax, scale, out,
                              (hipStream_t)stream, range_flag, (float*)ws, ws_bytes));
  });
}

// ---- the acoustic model's row-wise kernels (acoustic_kernels.hip) ----

int tts_op_embed(int dtype, const int32_t* ids, const int32_t* lens, int B, int N, int Tm, const void* table, int V,
                 int D, float scale, void* out, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "embed");
    op_require(ids && lens && table && out, "embed", "null buffer");
    op_require(B > 0 && B <= OP_MAX_GRID_YZ && N > 0 && Tm > 0 && V > 0 && D > 0, "embed",
               "needs 0 < B <= 65535 and N, Tm, V, D > 0" + op_dims({{"B", B}, {"N", N}, {"Tm", Tm}, {"V", V}, {"D", D}}));
    HIP_CHECK(launch_embed(dtype, ids, lens, B, N, Tm, table, V, D, scale, out, (hipStream_t)stream));
  });
}

int tts_op_layernorm(int dtype, const void* in, void* out, int rows, int C, const float* g1, const float* b1,
                     const float* g2, const float* b2, float eps, const int32_t* lens, int stride, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "layernorm");
    op_require(in && out && g1 && b1, "layernorm", "null buffer");
    op_require((g2 != nullptr) == (b2 != nullptr), "layernorm", "g2 and b2 come together");
    op_require(rows > 0 && C > 0, "layernorm", "needs rows, C > 0" + op_dims({{"rows", rows}, {"C", C}}));
    op_require(C <= LN_MAX_C, "layernorm", "C " + std::to_string(C) + " above the kernels' " + std::to_string(LN_MAX_C) + " channels");
    op_require(!lens || stride > 0, "layernorm", "lens needs a row stride > 0");
    if (dtype != DT_F32 && C % 8 == 0)  // 16-byte row loads
      op_require(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "layernorm",
                 "16-bit rows of C % 8 == 0 channels must be 16-byte aligned");
    HIP_CHECK(launch_layernorm(dtype, in, out, rows, C, g1, b1, g2, b2, eps, (hipStream_t)stream, lens, stride));
  });
}

int tts_op_layernorm_groups(int dtype, void* x, int rows, int C, int ld, int groups, const float* const* g,
                            const float* const* b, float eps, const int32_t* lens, int stride, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "layernorm_groups");
    op_require(x && g && b, "layernorm_groups", "null buffer");
    op_require(groups >= 1 && groups <= LnGroups::MAXG, "layernorm_groups",
               "takes 1 to " + std::to_string(LnGroups::MAXG) + " groups, not " + std::to_string(groups));
    op_require(rows > 0 && C > 0, "layernorm_groups", "needs rows, C > 0" + op_dims({{"rows", rows}, {"C", C}}));
    op_require(C <= LN_PRED_MAX_C, "layernorm_groups",
               "C " + std::to_string(C) + " above the kernel's " + std::to_string(LN_PRED_MAX_C) + " channels");
    op_require(ld >= (long long)groups * C, "layernorm_groups", "ld " + std::to_string(ld) + " below groups * C");
    op_require(!lens || stride > 0, "layernorm_groups", "lens needs a row stride > 0");
    LnGroups gp{};
    for (int i = 0; i < groups; ++i) {
      op_require(g[i] && b[i], "layernorm_groups", "null gain or bias");
      gp.g[i] = g[i];
      gp.b[i] = b[i];
    }
    HIP_CHECK(launch_layernorm_groups(dtype, x, rows, C, ld, gp, groups, eps, (hipStream_t)stream, lens, stride));
  });
}

int tts_op_pos_bias(int dtype, const void* qkv, int rows, int D, const float* u, const float* v, void* qu, void* qv,
                    void* stream) {
  return guarded([&] {
    op_dtype(dtype, "pos_bias");
    op_require(qkv && u && v && qu && qv, "pos_bias", "null buffer");
    op_require(rows > 0 && D > 0, "pos_bias", "needs rows, D > 0" + op_dims({{"rows", rows}, {"D", D}}));
    HIP_CHECK(launch_pos_bias(dtype, qkv, rows, D, u, v, qu, qv, (hipStream_t)stream));
  });
}

int tts_op_transpose_v(int dtype, const void* qkv, const int32_t* lens, int B, int Tm, int D, int H, int Sk, void* vt,
                       void* stream) {
  return guarded([&] {
    op_dtype(dtype, "transpose_v");
    op_require(qkv && lens && vt, "transpose_v", "null buffer");
    op_require(B > 0 && Tm > 0 && D > 0 && H > 0 && Sk > 0, "transpose_v",
               "needs B, Tm, D, H, Sk > 0" + op_dims({{"B", B}, {"Tm", Tm}, {"D", D}, {"H", H}, {"Sk", Sk}}));
    op_require(D % H == 0, "transpose_v", "D " + std::to_string(D) + " is not a multiple of H " + std::to_string(H));
    op_require((long long)B * H <= OP_MAX_GRID_YZ, "transpose_v", "B * H above 65535");
    if (dtype != DT_F32 && (D / H) % 64 == 0 && Sk % 8 == 0)  // transpose_v16_kernel: 16-byte loads and stores
      op_require(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(vt)) & 15) == 0, "transpose_v",
                 "the 16-bit kernel needs 16-byte-aligned buffers");
    HIP_CHECK(launch_transpose_v(dtype, qkv, lens, B, Tm, D, H, Sk, vt, (hipStream_t)stream));
  });
}

int tts_op_rel_softmax(int dtype, const void* ac, const void* bd, const int32_t* lens, int B, int H, int Tm, int Sac,
                       int Sbd, int Sk, float scale, void* p, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "rel_softmax");
    op_require(ac && bd && lens && p, "rel_softmax", "null buffer");
    op_require(B > 0 && H > 0 && Tm > 0, "rel_softmax", "needs B, H, Tm > 0" + op_dims({{"B", B}, {"H", H}, {"Tm", Tm}}));
    op_require((long long)B * H <= OP_MAX_GRID_YZ, "rel_softmax", "B * H above 65535");
    op_require(Sac >= Tm && Sk >= Tm && Sbd >= 2 * Tm - 1, "rel_softmax",
               "needs Sac >= Tm, Sk >= Tm and Sbd >= 2 Tm - 1" + op_dims({{"Tm", Tm}, {"Sac", Sac}, {"Sbd", Sbd}, {"Sk", Sk}}));
    HIP_CHECK(launch_rel_softmax(dtype, ac, bd, lens, B, H, Tm, Sac, Sbd, Sk, scale, p, (hipStream_t)stream));
  });
}

int tts_op_glu_dwconv(int dtype, const void* a, const int32_t* lens, int B, int Tm, int D, const float* w, int k,
                      const float* bias, void* out, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "glu_dwconv");
    op_require(a && lens && w && bias && out, "glu_dwconv", "null buffer");
    op_require(B > 0 && B <= OP_MAX_GRID_YZ && Tm > 0 && D > 0, "glu_dwconv",
               "needs 0 < B <= 65535 and Tm, D > 0" + op_dims({{"B", B}, {"Tm", Tm}, {"D", D}}));
    op_require(k >= 1 && k % 2 == 1 && k <= GLU_DWCONV_MAX_K, "glu_dwconv",
               "kernel size " + std::to_string(k) + " is not odd and at most " + std::to_string(GLU_DWCONV_MAX_K));
    const int epp = dtype == DT_F32 ? 4 : 8;
    if ((k == 7 || k == 31) && D % epp == 0)  // glu_dwconv_k_kernel: 16-byte loads
      op_require((reinterpret_cast<uintptr_t>(a) & 15) == 0, "glu_dwconv", "the k = 7 / 31 kernels need a 16-byte-aligned input");
    HIP_CHECK(launch_glu_dwconv(dtype, a, lens, B, Tm, D, w, k, bias, out, (hipStream_t)stream));
  });
}

int tts_op_durations(const float* logd, const int32_t* lens, int B, int N, const int32_t* override_d, float speed,
                     int Tcap, int32_t* dur, int32_t* mel_lens, int32_t* tokmap, void* stream) {
  return guarded([&] {
    op_require((logd || override_d) && lens && dur && mel_lens && tokmap, "durations", "null buffer");
    op_require(B > 0 && N > 0 && Tcap > 0, "durations", "needs B, N, Tcap > 0" + op_dims({{"B", B}, {"N", N}, {"Tcap", Tcap}}));
    op_require(((long long)N + 1) * (long long)sizeof(int) <= 64 * 1024, "durations",
               "N " + std::to_string(N) + " tokens do not fit the kernel's 64 KiB prefix-sum tile");
    op_require(speed > 0.f && std::isfinite(speed), "durations", "speed must be positive and finite");
    HIP_CHECK(launch_durations(logd, lens, B, N, override_d, speed, Tcap, dur, mel_lens, tokmap, (hipStream_t)stream));
  });
}

int tts_op_var_embed_add(int dtype, void* x, int rows, int D, const float* e, const float* we, const float* be,
                         const float* p, const float* wp, const float* bp, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "var_embed_add");
    op_require(x && e && we && be && p && wp && bp, "var_embed_add", "null buffer");
    op_require(rows > 0 && D > 0, "var_embed_add", "needs rows, D > 0" + op_dims({{"rows", rows}, {"D", D}}));
    HIP_CHECK(launch_var_embed_add(dtype, x, rows, D, e, we, be, p, wp, bp, (hipStream_t)stream));
  });
}

int tts_op_variance_adapt(int dtype, void* x, const float* logd, float* pitch, float* energy, const int32_t* lens,
                          int B, int N, int Np, int D, const int32_t* override_d, const tts_prosody* ctl,
                          size_t ctl_size, const float* we, const float* be, const float* wp, const float* bp, int Tcap,
                          int32_t* dur, int32_t* mel_lens, int32_t* tokmap, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "variance_adapt");
    op_require(x && (logd || override_d) && pitch && energy && lens && we && be && wp && bp && dur && mel_lens && tokmap,
               "variance_adapt", "null buffer");
    op_require(B > 0 && N > 0 && D > 0 && Tcap > 0, "variance_adapt",
               "needs B, N, D, Tcap > 0" + op_dims({{"B", B}, {"N", N}, {"D", D}, {"Tcap", Tcap}}));
    op_require(Np >= N, "variance_adapt", "needs Np >= N" + op_dims({{"N", N}, {"Np", Np}}));
    op_require(((long long)N + 1) * (long long)sizeof(int) <= 64 * 1024, "variance_adapt",
               "N " + std::to_string(N) + " above the kernel's 16383 tokens (its prefix sums live in LDS)");
    VarianceCtl vc;
    op_require(!ctl || read_prosody(ctl, ctl_size, &vc), "variance_adapt", "bad tts_prosody size");
    HIP_CHECK(launch_variance_adapt(dtype, x, logd, pitch, energy, lens, override_d, vc, B, N, Np, D, Tcap, we, be, wp,
                                    bp, dur, mel_lens, tokmap, (hipStream_t)stream));
  });
}

int tts_op_regulate(int dtype_in, int dtype, const void* enc, int B, int N, int D, const int32_t* tokmap, int Tcap,
                    int frames, int Tout, float scale, void* out, void* stream) {
  return guarded([&] {
    op_dtype(dtype, "regulate");
    op_dtype(dtype_in, "regulate");
    op_require(dtype_in == dtype || dtype_in == DT_F32, "regulate", "the input is of the output's dtype or fp32");
    op_require(enc && tokmap && out, "regulate", "null buffer");
    op_require(B > 0 && B <= OP_MAX_GRID_YZ && N > 0 && D > 0 && Tcap > 0 && Tout > 0 && frames > 0, "regulate",
               "needs 0 < B <= 65535 and N, D, Tcap, Tout, frames > 0" +
                   op_dims({{"B", B}, {"N", N}, {"D", D}, {"Tcap", Tcap}, {"Tout", Tout}, {"frames", frames}}));
    op_require(frames <= Tcap && frames <= Tout, "regulate",
               "frames " + std::to_string(frames) + " above Tcap " + std::to_string(Tcap) + " or Tout " + std::to_string(Tout));
    HIP_CHECK(launch_regulate(dtype_in, dtype, enc, B, N, D, tokmap, Tcap, frames, Tout, scale, out, (hipStream_t)stream));
  });
}

int tts_op_mel_out(int dtype, const void* in, const int32_t* mel_lens, int B, int Tin, int Tcap, int C, float* out,
                   void* stream) {
  return guarded([&] {
    op_dtype(dtype, "mel_out");
    op_require(in && mel_lens && out, "mel_out", "null buffer");
    op_require(B > 0 && B <= OP_MAX_GRID_YZ && Tin > 0 && Tcap > 0 && C > 0, "mel_out",
               "needs 0 < B <= 65535 and Tin, Tcap, C > 0" + op_dims({{"B", B}, {"Tin", Tin}, {"Tcap", Tcap}, {"C", C}}));
    HIP_CHECK(launch_mel_out(dtype, in, mel_lens, B, Tin, Tcap, C, out, (hipStream_t)stream));
  });
}

int tts_op_spk_bias(int dtype, const float* e, int B, int E, const float* We, const float* bias, int D, void* out,
                    void* stream) {
  return guarded([&] {
    op_dtype(dtype, "spk_bias");
    op_require(e && We && bias && out, "spk_bias", "null buffer");
    op_require(B > 0 && E > 0 && D > 0, "spk_bias", "needs B, E, D > 0" + op_dims({{"B", B}, {"E", E}, {"D", D}}));
    HIP_CHECK(launch_spk_bias(dtype, e, B, E, We, bias, D, out, (hipStream_t)stream));
  });
}

}  // extern "C"
