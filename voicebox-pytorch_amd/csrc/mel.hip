// Log-mel front end (LogMelCodec.encode = the arithmetic of the reference's MelVoco.encode, voicebox_pytorch.py:518-541): centred
// reflect-padded framing, Hann window, FFT in the LDS (fft_lds.hpp: fp32, twiddles from an fp64-built table), power spectrum,
// triangular mel filters stored as (start, length, weights) runs, 10 log10(max(., 1e-10)).  One kernel; no vendor FFT.
//
// A workgroup serves MEL_FRAMES = 4 consecutive frames of one wave (their reads overlap by n_fft - hop samples and hit the same
// cache lines): the two transforms of fft_lds.hpp, each carrying two real frames (frame 2c and frame 2c + 1), in the skewed layout
// described there.
#include "fft_lds.hpp"

namespace {

constexpr int MEL_FRAMES = 4;
constexpr int MEL_LD = fft_ld(FFT_MAX);

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ audio, float* __restrict__ out,
                                                     const float* __restrict__ window, const float* __restrict__ tw_re,
                                                     const float* __restrict__ tw_im, const int* __restrict__ fb_start,
                                                     const int* __restrict__ fb_len, const int* __restrict__ fb_off,
                                                     const float* __restrict__ fb_w, long T, int frames, int n_fft, int log2n, int hop,
                                                     int n_mels, int log_out) {
  __shared__ float re[2][MEL_LD], im[2][MEL_LD];
  __shared__ float pw[MEL_FRAMES][FFT_MAX / 2 + 1];
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
    const int r = fft_brev(j, log2n);
    re[c][r] = v[0];
    im[c][r] = v[1];
  }
  __syncthreads();
  fft_lds<false>(re[c], im[c], tw_re, tw_im, log2n, half_n, t);
  for (int k = t; k <= half_n; k += 128) {  // power = |.|^2 of the two frames
    const FftPair z = fft_split(re[c], im[c], k, n_fft);
    pw[2 * c][k] = z.ar * z.ar + z.ai * z.ai;
    pw[2 * c + 1][k] = z.br * z.br + z.bi * z.bi;
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
  if (int rc = fft_check_size("vbx_logmel", n_fft)) return rc;
  VBX_REQUIRE(hop > 0 && n_mels > 0 && T > n_fft / 2, "vbx_logmel: the wave must be longer than n_fft / 2 samples (reflect padding)");
  const int frames = (int)(1 + T / hop);
  hipLaunchKernelGGL(logmel_kernel, dim3(cdiv(frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out, window, tw_re,
                     tw_im, fb_start, fb_len, fb_off, fb_w, T, frames, n_fft, fft_log2(n_fft), hop, n_mels, log_out);
  VBX_LAUNCH_CHECK();
  return 0;
}
