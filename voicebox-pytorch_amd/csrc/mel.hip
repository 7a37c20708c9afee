// Log-mel front end (LogMelCodec.encode = the arithmetic of the reference's MelVoco.encode, voicebox_pytorch.py:518-541): centred
// reflect-padded framing, Hann window, FFT in the LDS (fp32, twiddles from an fp64-built table), power spectrum, triangular mel
// filters stored as (start, length, weights) runs, 10 log10(max(., 1e-10)).  One kernel; no vendor FFT.
//
// A workgroup serves MEL_FRAMES = 4 consecutive frames of one wave (their reads overlap by n_fft - hop samples and hit the same
// cache lines): two complex FFTs of n_fft points run side by side, 128 threads each, and each carries TWO real frames (frame 2c as
// the real part, frame 2c + 1 as the imaginary part; they are separated afterwards by the symmetry of a real signal's spectrum).
// Radix-2 decimation in time on bit-reversed input, in place.  LDS index i lives at i + (i >> 6): in the first stage a wave touches
// 128 consecutive floats at stride 2, which would be two lanes per bank (64 banks of 4 bytes) -- the skew moves the second half onto
// the odd banks.  Stages with a half-size of 2 .. 16 keep a 2-way conflict (4-way without the skew); from 32 on the accesses are
// consecutive.
#include "common.hpp"

namespace {

constexpr int MEL_FRAMES = 4;
constexpr int MEL_MAX_FFT = 2048;
VBX_DEV int skew(int i) { return i + (i >> 6); }
constexpr int MEL_LD = MEL_MAX_FFT + (MEL_MAX_FFT >> 6);

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ audio, float* __restrict__ out,
                                                     const float* __restrict__ window, const float* __restrict__ tw_re,
                                                     const float* __restrict__ tw_im, const int* __restrict__ fb_start,
                                                     const int* __restrict__ fb_len, const int* __restrict__ fb_off,
                                                     const float* __restrict__ fb_w, long T, int frames, int n_fft, int log2n, int hop,
                                                     int n_mels, int log_out) {
  __shared__ float re[2][MEL_LD], im[2][MEL_LD];
  __shared__ float pw[MEL_FRAMES][MEL_MAX_FFT / 2 + 1];
  const int tid = threadIdx.x, c = tid >> 7, t = tid & 127;  // FFT c, thread t of 128
  const int f0 = blockIdx.x * MEL_FRAMES, b = blockIdx.y;
  const float* a = audio + (long)b * T;
  const int half_n = n_fft >> 1;

  // framing: sample j of frame f is a[reflect(f * hop + j - n_fft / 2)] * window[j]; stored bit-reversed
  for (int j = t; j < n_fft; j += 128) {
    const float w = window[j];
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int f = f0 + 2 * c + h;
      if (f < frames && w != 0.f) {
        long p = (long)f * hop + j - half_n;
        if (p < 0) p = -p;
        if (p >= T) p = 2 * (T - 1) - p;
        v[h] = a[p] * w;
      }
    }
    const int r = skew((int)(__brev((unsigned)j) >> (32 - log2n)));
    re[c][r] = v[0];
    im[c][r] = v[1];
  }
  __syncthreads();
  for (int s = 0; s < log2n; s++) {
    const int half = 1 << s, tstep = half_n >> s;
    for (int q = t; q < half_n; q += 128) {
      const int pos = q & (half - 1);
      const int i0 = skew(((q >> s) << (s + 1)) + pos), i1 = skew(((q >> s) << (s + 1)) + pos + half);
      const float wr = tw_re[pos * tstep], wi = tw_im[pos * tstep];
      const float xr = re[c][i1], xi = im[c][i1];
      const float br = xr * wr - xi * wi, bi = xr * wi + xi * wr;
      const float ar = re[c][i0], ai = im[c][i0];
      re[c][i0] = ar + br; im[c][i0] = ai + bi;
      re[c][i1] = ar - br; im[c][i1] = ai - bi;
    }
    __syncthreads();
  }
  // separate the two real frames: A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2i);  power = |.|^2
  for (int k = t; k <= half_n; k += 128) {
    const int i0 = skew(k), i1 = skew((n_fft - k) & (n_fft - 1));
    const float zr = re[c][i0], zi = im[c][i0], nr = re[c][i1], ni = im[c][i1];
    const float ar = 0.5f * (zr + nr), ai = 0.5f * (zi - ni);
    const float br = 0.5f * (zi + ni), bi = -0.5f * (zr - nr);
    pw[2 * c][k] = ar * ar + ai * ai;
    pw[2 * c + 1][k] = br * br + bi * bi;
  }
  __syncthreads();
  for (int i = tid; i < MEL_FRAMES * n_mels; i += 256) {
    const int fl = i / n_mels, m = i - fl * n_mels;
    const int f = f0 + fl;
    if (f >= frames) continue;
    const int st = fb_start[m], len = fb_len[m];
    const float* w = fb_w + fb_off[m];
    float s = 0.f;
    for (int k = 0; k < len; k++) s += pw[fl][st + k] * w[k];
    if (log_out) s = 10.0f * log10f(fmaxf(s, 1e-10f));
    out[((long)b * frames + f) * n_mels + m] = s;
  }
}

}  // namespace

extern "C" int vbx_logmel(const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im,
                          const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft,
                          int hop, int n_mels, int log_out, void* stream) {
  VBX_REQUIRE(audio && out && window && tw_re && tw_im && fb_start && fb_len && fb_off && fb_w && B > 0 && B <= 65535,
              "vbx_logmel: bad args");
  VBX_REQUIRE(n_fft >= 256 && n_fft <= MEL_MAX_FFT && (n_fft & (n_fft - 1)) == 0, "vbx_logmel: n_fft must be a power of two in 256 .. 2048");
  VBX_REQUIRE(hop > 0 && n_mels > 0 && T > n_fft / 2, "vbx_logmel: the wave must be longer than n_fft / 2 samples (reflect padding)");
  int log2n = 0;
  while ((1 << log2n) < n_fft) log2n++;
  const int frames = (int)(1 + T / hop);
  hipLaunchKernelGGL(logmel_kernel, dim3(cdiv(frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out, window, tw_re,
                     tw_im, fb_start, fb_len, fb_off, fb_w, T, frames, n_fft, log2n, hop, n_mels, log_out);
  VBX_LAUNCH_CHECK();
  return 0;
}
