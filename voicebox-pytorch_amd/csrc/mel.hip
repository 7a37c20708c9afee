// The two mel front ends, one kernel body (mel_kernel<VOC>): reflect-padded framing, Hann window, FFT in the LDS (fft_lds.hpp: fp32,
// twiddles from an fp64-built table), triangular mel filters stored as (start, length, weights) runs.  No vendor FFT.
//
//   VOC = false  vbx_logmel: LogMelCodec.encode = the arithmetic of the reference's MelVoco.encode (voicebox_pytorch.py:518-541):
//                centred framing (pad = n_fft / 2, 1 + T / hop frames), power spectrum, 10 log10(max(., 1e-10)).
//   VOC = true   vbx_melspec: HiFiGANMelCodec.encode = HiFi-GAN's / BigVGAN's meldataset.mel_spectrogram: center=False framing over a
//                reflect pad of `pad` samples (frame f starts at f * hop - pad), magnitude sqrt(re^2 + im^2 + 1e-9), ln(max(., 1e-5))
//                (taken in fp64 and rounded once), then (x - mean) * inv_std, written frames-major or channel-first.
//
// A workgroup serves MEL_FRAMES = 4 consecutive frames of one wave (their reads overlap by n_fft - hop samples and hit the same
// cache lines): the two transforms of fft_lds.hpp, each carrying two real frames (frame 2c and frame 2c + 1), in the skewed layout
// described there.
#include "fft_lds.hpp"

namespace {

constexpr int MEL_FRAMES = 4;
constexpr int MEL_LD = fft_ld(FFT_MAX);

// LENS (vbx_logmel_lens / vbx_melspec_lens, include/vbx.h "ragged waves"): row b is the wave of lens[b] samples it would be alone --
// read below lens[b] only, reflected about lens[b], frames_b frames of its own; a frame past frames_b is staged as zeros (as a frame
// past the end always was: the partner of an odd last frame in the shared transform) and STORED as 0.0.
template <bool VOC, bool LENS>
__global__ __launch_bounds__(256) void mel_kernel(const float* __restrict__ audio, float* __restrict__ out,
                                                  const float* __restrict__ window, const float* __restrict__ tw_re,
                                                  const float* __restrict__ tw_im, const int* __restrict__ fb_start,
                                                  const int* __restrict__ fb_len, const int* __restrict__ fb_off,
                                                  const float* __restrict__ fb_w, long T, int frames, int n_fft, int log2n, int hop,
                                                  int n_mels, int log_out, int pad_arg, float mean, float inv_std, int channel_first,
                                                  const int* __restrict__ lens) {
  __shared__ float re[2][MEL_LD], im[2][MEL_LD];
  __shared__ float pw[MEL_FRAMES][FFT_MAX / 2 + 1];
  const int tid = threadIdx.x, c = tid >> 7, t = tid & 127;  // FFT c, thread t of 128
  const int f0 = blockIdx.x * MEL_FRAMES, b = blockIdx.y;
  const float* a = audio + (long)b * T;  // T is still the pitch here
  const int half_n = n_fft >> 1;
  const int pad = VOC ? pad_arg : half_n;
  const long Tpad = T;       // the row pitch of audio
  const int frames_ld = frames;  // ... and of out
  if (LENS) {  // the row's own length, held inside what the launch was validated for: pad < T_b <= T, at least one frame
    const long lo = VOC ? (pad + 1 > n_fft - 2 * pad ? pad + 1 : n_fft - 2 * pad) : half_n + 1;
    const long l = lens[b];
    T = l < lo ? lo : (l > Tpad ? Tpad : l);
    frames = VOC ? (int)(1 + (T + 2L * pad - n_fft) / hop) : (int)(1 + T / hop);
    if (f0 >= frames) {  // a group wholly behind the row: nothing to transform
      for (int i = tid; i < MEL_FRAMES * n_mels; i += 256) {
        const int fl = i / n_mels, m = i - fl * n_mels, f = f0 + fl;
        if (f < frames_ld) out[VOC && channel_first ? ((long)b * n_mels + m) * frames_ld + f : ((long)b * frames_ld + f) * n_mels + m] = 0.f;
      }
      return;
    }
  }

  // framing: sample j of frame f is a[reflect(f * hop + j - pad)] * window[j]; stored bit-reversed.  pad < T, and the last frame
  // ends at most pad samples past T, so one reflection per side lands inside [0, T) (one frame may take both)
  for (int j = t; j < n_fft; j += 128) {
    const float w = window[j];
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int f = f0 + 2 * c + h;
      if (f < frames && w != 0.f) {
        long p = (long)f * hop + j - pad;
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
  for (int k = t; k <= half_n; k += 128) {  // power = |.|^2 of the two frames; VOC: the magnitude sqrt(|.|^2 + 1e-9)
    const FftPair z = fft_split(re[c], im[c], k, n_fft);
    if (VOC) {
      pw[2 * c][k] = sqrtf(z.ar * z.ar + z.ai * z.ai + 1e-9f);
      pw[2 * c + 1][k] = sqrtf(z.br * z.br + z.bi * z.bi + 1e-9f);
    } else {
      pw[2 * c][k] = z.ar * z.ar + z.ai * z.ai;
      pw[2 * c + 1][k] = z.br * z.br + z.bi * z.bi;
    }
  }
  __syncthreads();
  for (int i = tid; i < MEL_FRAMES * n_mels; i += 256) {
    // channel-first output: the frame is the fast index, so the 4 frames of a filter are one 16-byte run of a row of out
    const int fl = VOC && channel_first ? i % MEL_FRAMES : i / n_mels;
    const int m = VOC && channel_first ? i / MEL_FRAMES : i - fl * n_mels;
    const int f = f0 + fl;
    if (LENS && f >= frames && f < frames_ld)
      out[VOC && channel_first ? ((long)b * n_mels + m) * frames_ld + f : ((long)b * frames_ld + f) * n_mels + m] = 0.f;
    if (f >= frames) continue;
    const int st = fb_start[m], len = fb_len[m];
    const float* w = fb_w + fb_off[m];
    float s = 0.f;
    for (int k = 0; k < len; k++) s += pw[fl][st + k] * w[k];
    if (VOC) {
      // the logarithm in fp64, rounded once: the device's logf is within 2 ulp (1.7 measured at 1e-5), silence must be ln(1e-5) to 1
      s = ((float)log((double)fmaxf(s, 1e-5f)) - mean) * inv_std;  // mean 0, inv_std 1: the plain logarithm, exactly
      out[channel_first ? ((long)b * n_mels + m) * frames_ld + f : ((long)b * frames_ld + f) * n_mels + m] = s;
    } else {
      if (log_out) s = 10.0f * log10f(fmaxf(s, 1e-10f));
      out[((long)b * frames_ld + f) * n_mels + m] = s;
    }
  }
}

}  // namespace

static int logmel_launch(const int* lens, const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im,
                          const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft,
                          int hop, int n_mels, int log_out, void* stream) {
  VBX_REQUIRE(audio && out && window && tw_re && tw_im && fb_start && fb_len && fb_off && fb_w && B > 0 && B <= 65535,
              "vbx_logmel: bad args");
  if (int rc = fft_check_size("vbx_logmel", n_fft)) return rc;
  VBX_REQUIRE(hop > 0 && n_mels > 0 && T > n_fft / 2, "vbx_logmel: the wave must be longer than n_fft / 2 samples (reflect padding)");
  const int frames = (int)(1 + T / hop);
  if (lens)
    hipLaunchKernelGGL((mel_kernel<false, true>), dim3(cdiv(frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out, window,
                       tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, T, frames, n_fft, fft_log2(n_fft), hop, n_mels, log_out, 0, 0.f, 1.f, 0,
                       lens);
  else
    hipLaunchKernelGGL((mel_kernel<false, false>), dim3(cdiv(frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out, window,
                       tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, T, frames, n_fft, fft_log2(n_fft), hop, n_mels, log_out, 0, 0.f, 1.f, 0,
                       (const int*)nullptr);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_logmel(const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im,
                          const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft,
                          int hop, int n_mels, int log_out, void* stream) {
  return logmel_launch(nullptr, audio, out, window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, B, T, n_fft, hop, n_mels, log_out, stream);
}

extern "C" int vbx_logmel_lens(const float* audio, const int* lens, float* out, const float* window, const float* tw_re,
                               const float* tw_im, const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B,
                               long T, int n_fft, int hop, int n_mels, int log_out, void* stream) {
  VBX_REQUIRE(lens, "vbx_logmel_lens: lens is NULL (vbx_logmel is the entry without lengths)");
  return logmel_launch(lens, audio, out, window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, B, T, n_fft, hop, n_mels, log_out, stream);
}

static int melspec_launch(const int* lens, const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im,
                           const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft,
                           int hop, int pad, int n_mels, float mean, float inv_std, int channel_first, void* stream) {
  VBX_REQUIRE(audio && out && window && tw_re && tw_im && fb_start && fb_len && fb_off && fb_w && B > 0 && B <= 65535,
              "vbx_melspec: bad args");
  if (int rc = fft_check_size("vbx_melspec", n_fft)) return rc;
  VBX_REQUIRE(hop > 0 && hop <= n_fft && n_mels > 0 && pad >= 0 && pad <= n_fft / 2, "vbx_melspec: need 0 < hop <= n_fft, n_mels > 0 and "
              "0 <= pad <= n_fft / 2");
  VBX_REQUIRE(T > pad && T + 2L * pad >= n_fft, "vbx_melspec: the wave must be longer than the reflect pad and fill one frame with it");
  const long frames = 1 + (T + 2L * pad - n_fft) / hop;
  VBX_REQUIRE(frames <= 0x7fffffffL, "vbx_melspec: too many frames");
  if (lens)
    hipLaunchKernelGGL((mel_kernel<true, true>), dim3(cdiv((int)frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out,
                       window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, T, (int)frames, n_fft, fft_log2(n_fft), hop, n_mels, 1, pad,
                       mean, inv_std, channel_first, lens);
  else
    hipLaunchKernelGGL((mel_kernel<true, false>), dim3(cdiv((int)frames, MEL_FRAMES), B), dim3(256), 0, (hipStream_t)stream, audio, out,
                       window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, T, (int)frames, n_fft, fft_log2(n_fft), hop, n_mels, 1, pad,
                       mean, inv_std, channel_first, (const int*)nullptr);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_melspec(const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im,
                           const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft,
                           int hop, int pad, int n_mels, float mean, float inv_std, int channel_first, void* stream) {
  return melspec_launch(nullptr, audio, out, window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, B, T, n_fft, hop, pad, n_mels, mean,
                        inv_std, channel_first, stream);
}

extern "C" int vbx_melspec_lens(const float* audio, const int* lens, float* out, const float* window, const float* tw_re,
                                const float* tw_im, const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B,
                                long T, int n_fft, int hop, int pad, int n_mels, float mean, float inv_std, int channel_first,
                                void* stream) {
  VBX_REQUIRE(lens, "vbx_melspec_lens: lens is NULL (vbx_melspec is the entry without lengths)");
  return melspec_launch(lens, audio, out, window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w, B, T, n_fft, hop, pad, n_mels, mean,
                        inv_std, channel_first, stream);
}
