// Rational-rate polyphase resampler for the waveform output:
// 22,050 Hz -> 24,000 Hz (up 160, down 147) for clients that assume the reference's
// hard-coded 24 kHz (synthesizer.py:119, queue_manager.py:40), or any up/down.
//
// Restates scipy.signal.resample_poly(x, up, down) with its default window ('kaiser', 5.0)
// and constant (zero) padding, per utterance:
//   h       = firwin(2*half_len + 1, 1/max(up,down), window=kaiser(5.0)) * up,
//             half_len = 10 * max(up, down)
//   h'      = [zeros(n_pre_pad), h],  n_pre_pad = down - half_len % down
//   y[m]    = sum_k h'[k] * xu[(m + n_pre_remove) * down - k],   n_pre_remove = (half_len + n_pre_pad) / down
//             (xu = x upsampled by zero insertion), m < n_out = ceil(n_in * up / down)
// Polyphase: with t = (m + n_pre_remove) * down only taps k = t mod up + up*q meet a nonzero
// xu, so y[m] = sum_q hp[t mod up][q] * x[t / up - q] -- NQ = ceil(len(h') / up) MACs per
// output (21 at 160/147).  One thread per output sample; coefficients [up][NQ] fp32 are
// read through L1/L2 (13 KB at 160/147), the input window is shared by neighbouring lanes.
//
// A stream that arrives in chunks (sub-sentence streaming) runs resample_poly_chunk_kernel per
// chunk: the same sum, the NQ - 1 samples before the chunk carried in a history buffer, and only
// the outputs emitted whose newest tap the samples seen so far cover.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace tts {

// modified Bessel function of the first kind, order 0 (power series; converges for the
// Kaiser arguments used here, beta <= 20)
static double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

// scipy.signal.resample_poly's default filter (firwin with a symmetric Kaiser(5.0) window,
// DC gain normalised to 1, then scaled by up) after the pre-padding it applies.
// Returns the padded length; h_out (if cap suffices) receives the taps.
int resample_design(int up, int down, std::vector<double>& h, int& n_pre_remove) {
  const int max_rate = up > down ? up : down;
  const double fc = 1.0 / max_rate;
  const int half_len = 10 * max_rate;
  const int n = 2 * half_len + 1;
  const double alpha = 0.5 * (n - 1);
  const double beta = 5.0;
  std::vector<double> f(n);
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const double m = i - alpha;
    const double xx = fc * m;
    const double sinc = xx == 0.0 ? 1.0 : std::sin(M_PI * xx) / (M_PI * xx);
    const double r = 2.0 * i / (n - 1) - 1.0;
    const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
    f[i] = fc * sinc * w;
    s += f[i];
  }
  const int n_pre_pad = down - half_len % down;
  n_pre_remove = (half_len + n_pre_pad) / down;
  h.assign(n_pre_pad + n, 0.0);
  for (int i = 0; i < n; ++i) h[n_pre_pad + i] = f[i] / s * up;
  return (int)h.size();
}

// The tap sum of one output sample: taps q = 0 .. nq-1 in this order, inputs outside [0, n_in)
// skipped.  `x(i)` returns input sample i; the full pass and the chunked pass both sum through
// this one function, so a chunked stream equals the full pass bit for bit.
template <class Load>
__device__ __forceinline__ float resample_tap_sum(const float* __restrict__ hr, int nq, long long base, int n_in,
                                                  Load x) {
  float acc = 0.f;
  for (int q = 0; q < nq; ++q) {
    const long long i = base - q;
    if (i >= 0 && i < n_in) acc = fmaf(hr[q], x(i), acc);
  }
  return acc;
}

// Outputs that need no input at or past sample `end` (an utterance of n_in samples and n_out
// outputs): y[m] reads up to x[(m + n_pre_remove) * down / up], so m < ceil(end*up/down) -
// n_pre_remove; everything once the utterance has ended.
__host__ __device__ inline long long resample_emitted(long long end, long long n_in, long long n_out, int up,
                                                      int down, int n_pre_remove) {
  if (end >= n_in) return n_out;
  const long long e = (end * up + down - 1) / down - n_pre_remove;
  return e < 0 ? 0 : (e < n_out ? e : n_out);
}

__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, long long sxb,
                                                            const int* __restrict__ in_lens, int up, int down,
                                                            int nq, int n_pre_remove, const float* __restrict__ hp,
                                                            float* __restrict__ y, long long syb, int y_cap,
                                                            int* __restrict__ out_lens) {
  const int b = blockIdx.y;
  const int n_in = in_lens[b];
  const long long n_out = ((long long)n_in * up + down - 1) / down;
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m == 0 && out_lens) out_lens[b] = (int)min(n_out, (long long)y_cap);
  if (m >= y_cap) return;
  float* yb = y + (long long)b * syb;
  if (m >= n_out) {  // zero tail, like the vocoder's output past each utterance
    yb[m] = 0.f;
    return;
  }
  const long long t = ((long long)m + n_pre_remove) * down;
  const int ph = (int)(t % up);
  const long long base = t / up;
  const float* hr = hp + (long long)ph * nq;
  const float* xb = x + (long long)b * sxb;
  yb[m] = resample_tap_sum(hr, nq, base, n_in, [xb](long long i) { return xb[i]; });
}

// One chunk of a stream: `cur` holds input samples [in_start, in_start + in_count) of every
// utterance, hist_in the H = nq - 1 samples before in_start (not read when in_start == 0), and
// in_lens the utterances' final lengths.  Writes the outputs [emitted(in_start), emitted(in_start +
// in_count)) -- those whose newest tap lies inside the samples seen so far, and the last
// n_pre_remove outputs of an utterance with the chunk it ends in -- zeros up to y_cap, their
// count, and hist_out = the H samples before in_start + in_count (the tail of hist_in ++ cur;
// samples past an utterance's end as 0: they are never summed).  One thread per output sample;
// block x = 0 of each utterance also moves the history.
__global__ __launch_bounds__(256) void resample_poly_chunk_kernel(
    const float* __restrict__ cur, long long sxb, long long in_start, int in_count, const int* __restrict__ in_lens,
    int up, int down, int nq, int n_pre_remove, const float* __restrict__ hp, const float* __restrict__ hist_in,
    float* __restrict__ hist_out, float* __restrict__ y, long long syb, int y_cap, int* __restrict__ out_lens) {
  const int b = blockIdx.y;
  const int H = nq - 1;
  const int n_in = in_lens[b];
  const long long n_out = ((long long)n_in * up + down - 1) / down;
  const long long in_end = in_start + in_count;
  const long long m_lo = in_start == 0 ? 0 : resample_emitted(in_start, n_in, n_out, up, down, n_pre_remove);
  const long long m_hi = resample_emitted(in_end, n_in, n_out, up, down, n_pre_remove);
  const float* cb = cur + (long long)b * sxb;
  const float* hb = hist_in + (long long)b * H;  // sample i < in_start is hb[H + i - in_start]
  if (blockIdx.x == 0) {
    float* ho = hist_out + (long long)b * H;
    for (int k = threadIdx.x; k < H; k += 256) {
      const long long g = in_end - H + k;
      float v = 0.f;
      if (g >= 0 && g < n_in) v = g >= in_start ? cb[g - in_start] : hb[H + (g - in_start)];
      ho[k] = v;
    }
  }
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0 && out_lens) out_lens[b] = (int)min(m_hi - m_lo, (long long)y_cap);
  if (j >= y_cap) return;
  float* yb = y + (long long)b * syb;
  const long long m = m_lo + j;
  if (m >= m_hi) {
    yb[j] = 0.f;
    return;
  }
  const long long t = (m + n_pre_remove) * down;
  const int ph = (int)(t % up);
  const long long base = t / up;
  yb[j] = resample_tap_sum(hp + (long long)ph * nq, nq, base, n_in, [=](long long i) {
    return i >= in_start ? cb[i - in_start] : hb[H + (i - in_start)];
  });
}

hipError_t launch_resample_poly(const float* x, long long sxb, const int* in_lens, int B, int up, int down, int nq,
                                int n_pre_remove, const float* hp, float* y, long long syb, int y_cap,
                                int* out_lens, hipStream_t s) {
  if (B <= 0 || y_cap <= 0) return hipSuccess;
  dim3 grid((y_cap + 255) / 256, B);
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(256), 0, s, x, sxb, in_lens, up, down, nq, n_pre_remove, hp,
                     y, syb, y_cap, out_lens);
  return hipGetLastError();
}

hipError_t launch_resample_poly_chunk(const float* cur, long long sxb, long long in_start, int in_count,
                                      const int* in_lens, int B, int up, int down, int nq, int n_pre_remove,
                                      const float* hp, const float* hist_in, float* hist_out, float* y,
                                      long long syb, int y_cap, int* out_lens, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  dim3 grid((std::max(y_cap, 1) + 255) / 256, B);  // (block x = 0 always runs: it moves the history)
  hipLaunchKernelGGL(resample_poly_chunk_kernel, grid, dim3(256), 0, s, cur, sxb, in_start, in_count, in_lens, up,
                     down, nq, n_pre_remove, hp, hist_in, hist_out, y, syb, y_cap, out_lens);
  return hipGetLastError();
}

}  // namespace tts
