// Vocoder-free decode of LogMelCodec: mel -> linear magnitude (least-squares inverse of the HTK filter bank, clamped at zero), then
// Griffin-Lim phase recovery (the published torchaudio.functional.griffinlim loop, power = 1, length = None) -- fp32, FFT in the
// LDS, no vendor FFT, no host synchronisation inside the loop.  Two launches per iteration:
//
//   synthesis  A = normalise(R - m T) (on the fly from the two kept spectra), A * magnitude -> inverse FFT -> times window ->
//              frame buffer [B, frames, win_length] (only the samples under the window; the rest of a frame is multiplied by zero)
//   analysis   overlap-add as a GATHER straight out of the frame buffer (each wave sample sums the <= ceil(win / hop) frames that
//              cover it in ascending frame order, times the reciprocal window-square envelope: fixed order, no atomics, bit-identical
//              reruns) -> reflect-padded framing -> times window -> FFT -> R [B, frames, n_fft / 2 + 1]
//
// The wave itself is materialised once, after the last synthesis.  R_k and R_{k-1} (= T_k) live in two buffers that swap roles:
// the unit phasor A_{k+1} = (R_k - m T_k) / (|R_k - m T_k| + 1e-16) is never stored, the synthesis forms it in the order of the
// formula (subtract, then divide).  All spectra are frame-major ([B, frames, bins], interleaved re / im) so a workgroup reads and
// writes whole rows.
//
// A workgroup serves GL_FRAMES = 4 consecutive frames with the two transforms of fft_lds.hpp (protocol and LDS layout there), each
// carrying two real frames.  Before an inverse transform the imaginary parts of the DC and Nyquist bins are DROPPED (a
// complex-to-real transform ignores them; a random initial phase makes them non-zero); its exact factor 1 / n_fft is applied with
// the window.  The LDS is sized per launch (n_fft and hop dependent), so the default codec takes 21 KiB a workgroup instead of the
// 2048-point worst case.
//
// gl_synth_kernel<true> is the same synthesis at n_fft = 5 * 2^m (320, 640, 1280: fft_lds.hpp's mixed-radix inverse), a separate
// instantiation that only vbx_istft / vbx_istft_trim launch; the analysis step, and with it vbx_griffinlim, stays at powers of two.
// vbx_istft_trim is the overlap-add with any trim (Vocos's padding="same" keeps frames * hop samples).
#include "fft_lds.hpp"

namespace {

constexpr int GL_FRAMES = 4;
constexpr int GL_MAX_LDS = 64 * 1024;
constexpr int MM_FRAMES = 8;

// wave sample t (0 <= t < (frames - 1) * hop) of batch row `fb`: the frames g with 0 <= n - g * hop < win cover it, n counted from
// the first sample under the window of frame 0
VBX_DEV float ola_sample(const float* __restrict__ fb, const float* __restrict__ renv, long t, int frames, int hop, int win, int left,
                         int half_n) {
  const long n = t + half_n - left;
  const long num = n - win + 1;
  const int g0 = num <= 0 ? 0 : (int)((num + hop - 1) / hop);
  const long gl = n / hop;
  const int g1 = gl > frames - 1 ? frames - 1 : (int)gl;
  float s = 0.f;
  for (int g = g0; g <= g1; g++) s += fb[(long)g * win + (n - (long)g * hop)];
  return s * renv[t];
}

// R5: n_fft = 5 * 2^log2n (log2n is then m of fft_lds.hpp), else n_fft = 2^log2n
template <bool R5>
__global__ __launch_bounds__(256) void gl_synth_kernel(const float2* __restrict__ P, const float2* __restrict__ Q,
                                                       const float* __restrict__ mag, float* __restrict__ fb,
                                                       const float* __restrict__ window, const float* __restrict__ tw_re,
                                                       const float* __restrict__ tw_im, float m, int first, int frames, int n_fft,
                                                       int log2n, int win, int left) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, c = tid >> 7, t = tid & 127;
  const int f0 = blockIdx.x * GL_FRAMES, b = blockIdx.y;
  const int half_n = n_fft >> 1, nb = half_n + 1, ld = fft_ld(n_fft);
  float* re = smem + c * ld;
  float* im = smem + (2 + c) * ld;

  for (int k = t; k <= half_n; k += 128) {
    float x[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int f = f0 + 2 * c + h;
      if (f < frames) {
        const long o = ((long)b * frames + f) * nb + k;
        const float2 p = P[o];
        float ar = p.x, ai = p.y;
        if (!first) {  // A = R - m T;  A / (|A| + 1e-16)
          const float2 q = Q[o];
          ar = p.x - m * q.x;
          ai = p.y - m * q.y;
          const float d = hypotf(ar, ai) + 1e-16f;
          ar /= d;
          ai /= d;
        }
        const float g = mag[o];
        x[h][0] = ar * g;
        x[h][1] = ai * g;
      }
    }
    if (k == 0 || k == half_n) x[0][1] = x[1][1] = 0.f;
    const int r = R5 ? fft_map5(k, log2n) : fft_brev(k, log2n);
    re[r] = x[0][0] - x[1][1];
    im[r] = x[0][1] + x[1][0];
    if (k > 0 && k < half_n) {  // Z[N - k] = conj(X0[k]) + i conj(X1[k])
      const int r2 = R5 ? fft_map5(n_fft - k, log2n) : fft_brev(n_fft - k, log2n);
      re[r2] = x[0][0] + x[1][1];
      im[r2] = x[1][0] - x[0][1];
    }
  }
  __syncthreads();
  if constexpr (R5) fft_lds5_inverse(re, im, tw_re, tw_im, log2n, n_fft, t);
  else fft_lds<true>(re, im, tw_re, tw_im, log2n, half_n, t);
  const float inv_n = 1.0f / (float)n_fft;
  for (int j = t; j < win; j += 128) {
    const float w = window[left + j] * inv_n;  // 1 / n_fft is a power of two: exact (R5: two more roundings, inv_n's and the product's)
    const int i = fft_skew(left + j);
    const int f = f0 + 2 * c;
    if (f < frames) fb[((long)b * frames + f) * win + j] = re[i] * w;
    if (f + 1 < frames) fb[((long)b * frames + f + 1) * win + j] = im[i] * w;
  }
}

__global__ __launch_bounds__(256) void gl_analysis_kernel(const float* __restrict__ fb, float2* __restrict__ R,
                                                          const float* __restrict__ window, const float* __restrict__ tw_re,
                                                          const float* __restrict__ tw_im, const float* __restrict__ renv, int frames,
                                                          int n_fft, int log2n, int win, int left, int hop) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, c = tid >> 7, t = tid & 127;
  const int f0 = blockIdx.x * GL_FRAMES, b = blockIdx.y;
  const int half_n = n_fft >> 1, nb = half_n + 1, ld = fft_ld(n_fft);
  float* re = smem + c * ld;
  float* im = smem + (2 + c) * ld;
  float* seg = smem + 4 * ld;  // the wave under the windows of this workgroup's frames, reflect padding resolved
  const long L = (long)(frames - 1) * hop;
  const int nvalid = frames - f0 < GL_FRAMES ? frames - f0 : GL_FRAMES;
  const int seg_n = (nvalid - 1) * hop + win;
  const float* fbb = fb + (long)b * frames * win;

  for (int i = tid; i < seg_n; i += 256) {
    long p = (long)f0 * hop + left + i - half_n;
    if (p < 0) p = -p;
    if (p >= L) p = 2 * (L - 1) - p;
    seg[i] = ola_sample(fbb, renv, p, frames, hop, win, left, half_n);
  }
  __syncthreads();
  for (int j = t; j < n_fft; j += 128) {
    float v[2] = {0.f, 0.f};
    if (j >= left && j < left + win) {
      const float w = window[j];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int fl = 2 * c + h;
        if (fl < nvalid) v[h] = seg[fl * hop + j - left] * w;
      }
    }
    const int r = fft_brev(j, log2n);
    re[r] = v[0];
    im[r] = v[1];
  }
  __syncthreads();
  fft_lds<false>(re, im, tw_re, tw_im, log2n, half_n, t);
  for (int k = t; k <= half_n; k += 128) {
    const FftPair z = fft_split(re, im, k, n_fft);
    const int f = f0 + 2 * c;
    if (f < frames) R[((long)b * frames + f) * nb + k] = make_float2(z.ar, z.ai);
    if (f + 1 < frames) R[((long)b * frames + f + 1) * nb + k] = make_float2(z.br, z.bi);
  }
}

__global__ __launch_bounds__(256) void gl_ola_kernel(const float* __restrict__ fb, float* __restrict__ wave,
                                                     const float* __restrict__ renv, int frames, int win, int left, int hop,
                                                     int half_n) {
  const long L = (long)(frames - 1) * hop;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t < L) wave[(long)b * L + t] = ola_sample(fb + (long)b * frames * win, renv, t, frames, hop, win, left, half_n);
}

// samples [trim, trim + out_len) of the overlap-add, counted from the first sample of frame 0's n_fft-point transform; a sample before
// the first window (win < n_fft, trim < left) is zero
__global__ __launch_bounds__(256) void gl_ola_trim_kernel(const float* __restrict__ fb, float* __restrict__ wave,
                                                          const float* __restrict__ renv, int frames, int win, int left, int hop,
                                                          int trim, long out_len) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t < out_len)
    wave[(long)b * out_len + t] = t + trim < left ? 0.f : ola_sample(fb + (long)b * frames * win, renv, t, frames, hop, win, left, trim);
}

// MM_FRAMES frames of one batch row: dB -> power (in fp64: 10^(x / 10) amplifies the rounding of x / 10 by x ln 10 / 10), the frames'
// mel vectors in the LDS, thread k = one frequency bin against column k of pinv(fb^T) stored mel-major (consecutive lanes read
// consecutive floats), clamp at zero, square root.  Output frame-major [B, frames, bins].
__global__ __launch_bounds__(256) void mel_to_mag_kernel(const float* __restrict__ mel, float* __restrict__ mag,
                                                         const float* __restrict__ pinv_t, int frames, int n_mels, int nb, int log_in) {
  extern __shared__ float smem[];  // [MM_FRAMES][n_mels]
  const int tid = threadIdx.x, f0 = blockIdx.x * MM_FRAMES, b = blockIdx.y;
  for (int i = tid; i < MM_FRAMES * n_mels; i += 256) {
    const int fl = i / n_mels, f = f0 + fl;
    float v = 0.f;
    if (f < frames) {
      v = mel[((long)b * frames + f0) * n_mels + i];
      if (log_in) v = (float)pow(10.0, (double)v / 10.0);
    }
    smem[i] = v;
  }
  __syncthreads();
  for (int k = tid; k < nb; k += 256) {
    float acc[MM_FRAMES];
#pragma unroll
    for (int fl = 0; fl < MM_FRAMES; fl++) acc[fl] = 0.f;
    for (int mi = 0; mi < n_mels; mi++) {
      const float w = pinv_t[(long)mi * nb + k];
#pragma unroll
      for (int fl = 0; fl < MM_FRAMES; fl++) acc[fl] = fmaf(w, smem[fl * n_mels + mi], acc[fl]);
    }
#pragma unroll
    for (int fl = 0; fl < MM_FRAMES; fl++)
      if (f0 + fl < frames) mag[((long)b * frames + f0 + fl) * nb + k] = sqrtf(fmaxf(acc[fl], 0.f));
  }
}

}  // namespace

extern "C" int vbx_mel_to_mag(const float* mel, float* mag, const float* pinv_t, int B, int frames, int n_mels, int n_bins, int log_in,
                              void* stream) {
  VBX_REQUIRE(mel && mag && pinv_t && B > 0 && B <= 65535 && frames > 0 && n_bins > 0, "vbx_mel_to_mag: bad args");
  VBX_REQUIRE(n_mels > 0 && MM_FRAMES * n_mels * (int)sizeof(float) <= GL_MAX_LDS, "vbx_mel_to_mag: n_mels must be in 1 .. 2048");
  hipLaunchKernelGGL(mel_to_mag_kernel, dim3(cdiv(frames, MM_FRAMES), B), dim3(256), MM_FRAMES * n_mels * sizeof(float),
                     (hipStream_t)stream, mel, mag, pinv_t, frames, n_mels, n_bins, log_in);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_griffinlim_lds_bytes(int n_fft, int win, int hop) {
  return (int)sizeof(float) * (4 * fft_ld(n_fft) + (GL_FRAMES - 1) * hop + win);
}

extern "C" int vbx_griffinlim(const float* mag, float* spec_a, float* spec_b, float* fb, float* wave, const float* window,
                              const float* tw_re, const float* tw_im, const float* renv, int B, int frames, int n_fft, int win, int hop,
                              int n_iter, float m, void* stream) {
  VBX_REQUIRE(mag && spec_a && spec_b && fb && wave && window && tw_re && tw_im && renv && B > 0 && B <= 65535 && n_iter >= 0,
              "vbx_griffinlim: bad args");
  if (int rc = fft_check_size("vbx_griffinlim", n_fft)) return rc;
  VBX_REQUIRE(win > 0 && win <= n_fft && hop > 0 && hop <= win, "vbx_griffinlim: need 0 < hop <= win_length <= n_fft");
  VBX_REQUIRE(frames > 1 && (long)(frames - 1) * hop > n_fft / 2 && (long)(frames - 1) * hop + n_fft < 2147483647L,
              "vbx_griffinlim: (frames - 1) * hop must exceed n_fft / 2 (reflect padding of the analysis step)");
  const int lds = vbx_griffinlim_lds_bytes(n_fft, win, hop);
  VBX_REQUIRE(lds <= GL_MAX_LDS, "vbx_griffinlim: 3 * hop + win_length does not fit the LDS beside a %d-point transform", n_fft);
  const int log2n = fft_log2(n_fft);
  const int left = (n_fft - win) / 2, half_n = n_fft / 2;
  const long L = (long)(frames - 1) * hop;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(frames, GL_FRAMES), B), block(256);
  const size_t lds_synth = sizeof(float) * 4 * fft_ld(n_fft);
  float2* p = (float2*)spec_a;  // R_k (before the first analysis: the initial unit phasors)
  float2* q = (float2*)spec_b;  // T_k = R_{k-1}
  for (int k = 0; k <= n_iter; k++) {
    // k = 0: A_0 as given;  k = 1: T_0 = 0 (whatever finite values q holds are multiplied by m = 0);  k >= 2: the momentum term is live
    hipLaunchKernelGGL(gl_synth_kernel<false>, grid, block, lds_synth, st, (const float2*)p, (const float2*)q, mag, fb, window, tw_re, tw_im,
                       k >= 2 ? m : 0.f, k == 0 ? 1 : 0, frames, n_fft, log2n, win, left);
    if (k == n_iter) break;
    hipLaunchKernelGGL(gl_analysis_kernel, grid, block, (size_t)lds, st, (const float*)fb, q, window, tw_re, tw_im, renv, frames, n_fft,
                       log2n, win, left, hop);
    float2* tmp = p; p = q; q = tmp;
  }
  hipLaunchKernelGGL(gl_ola_kernel, dim3(cdiv(L, 256), B), block, 0, st, (const float*)fb, wave, renv, frames, win, left, hop, half_n);
  VBX_LAUNCH_CHECK();
  return 0;
}

// the synthesis launch of one inverse STFT: the power-of-two or the mixed-radix instantiation by n_fft (checked by the caller)
static void istft_synth(const float* mag, const float* spec, float* fb, const float* window, const float* tw_re, const float* tw_im,
                        int B, int frames, int n_fft, int win, hipStream_t st) {
  const dim3 grid(cdiv(frames, GL_FRAMES), B), block(256);
  const size_t lds = sizeof(float) * 4 * fft_ld(n_fft);
  const int left = (n_fft - win) / 2;
  if (fft_is_radix5(n_fft))
    hipLaunchKernelGGL(gl_synth_kernel<true>, grid, block, lds, st, (const float2*)spec, (const float2*)spec, mag, fb, window, tw_re,
                       tw_im, 0.f, 1, frames, n_fft, fft_log2(n_fft / 5), win, left);
  else
    hipLaunchKernelGGL(gl_synth_kernel<false>, grid, block, lds, st, (const float2*)spec, (const float2*)spec, mag, fb, window, tw_re,
                       tw_im, 0.f, 1, frames, n_fft, fft_log2(n_fft), win, left);
}

// One inverse STFT (torch.istft, center = True, length = None) of mag * phasor: the synthesis and overlap-add launches above alone,
// so nothing of the analysis step's reflect padding is demanded -- two frames are enough (csrc/vocos.hip's last step).
extern "C" int vbx_istft(const float* mag, const float* spec, float* fb, float* wave, const float* window, const float* tw_re,
                         const float* tw_im, const float* renv, int B, int frames, int n_fft, int win, int hop, void* stream) {
  VBX_REQUIRE(mag && spec && fb && wave && window && tw_re && tw_im && renv && B > 0 && B <= 65535, "vbx_istft: bad args");
  if (int rc = fft_check_size_inverse("vbx_istft", n_fft)) return rc;
  VBX_REQUIRE(win > 0 && win <= n_fft && hop > 0 && hop <= win, "vbx_istft: need 0 < hop <= win_length <= n_fft");
  VBX_REQUIRE(frames > 1 && (long)(frames - 1) * hop + n_fft < 2147483647L, "vbx_istft: need at least two frames");
  const int left = (n_fft - win) / 2;
  const long L = (long)(frames - 1) * hop;
  hipStream_t st = (hipStream_t)stream;
  istft_synth(mag, spec, fb, window, tw_re, tw_im, B, frames, n_fft, win, st);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_ola_kernel, dim3(cdiv(L, 256), B), dim3(256), 0, st, (const float*)fb, wave, renv, frames, win, left, hop,
                     n_fft / 2);
  VBX_LAUNCH_CHECK();
  return 0;
}

// vbx_istft with any trim: wave [B, out_len] = samples [trim, trim + out_len) of the (frames - 1) * hop + n_fft samples the frames'
// windowed inverse transforms add up to, times renv [out_len].  One frame is enough.  Same summation order as vbx_istft.
extern "C" int vbx_istft_trim(const float* mag, const float* spec, float* fb, float* wave, const float* window, const float* tw_re,
                              const float* tw_im, const float* renv, int B, int frames, int n_fft, int win, int hop, int trim,
                              long out_len, void* stream) {
  VBX_REQUIRE(mag && spec && fb && wave && window && tw_re && tw_im && renv && B > 0 && B <= 65535, "vbx_istft_trim: bad args");
  if (int rc = fft_check_size_inverse("vbx_istft_trim", n_fft)) return rc;
  VBX_REQUIRE(win > 0 && win <= n_fft && hop > 0 && hop <= win, "vbx_istft_trim: need 0 < hop <= win_length <= n_fft");
  VBX_REQUIRE(frames > 0 && (long)(frames - 1) * hop + n_fft < 2147483647L, "vbx_istft_trim: need at least one frame");
  VBX_REQUIRE(trim >= 0 && out_len > 0 && trim + out_len <= (long)(frames - 1) * hop + n_fft,
              "vbx_istft_trim: [trim, trim + out_len) must lie inside the (frames - 1) * hop + n_fft samples");
  hipStream_t st = (hipStream_t)stream;
  istft_synth(mag, spec, fb, window, tw_re, tw_im, B, frames, n_fft, win, st);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_ola_trim_kernel, dim3((unsigned)cdiv(out_len, 256), B), dim3(256), 0, st, (const float*)fb, wave, renv, frames,
                     win, (n_fft - win) / 2, hop, trim, out_len);
  VBX_LAUNCH_CHECK();
  return 0;
}
