// The n_fft-point complex FFT in the LDS that csrc/mel.hip (logmel_kernel) and csrc/griffinlim.hip (gl_synth_kernel,
// gl_analysis_kernel) share: fp32, twiddles from an fp64-built table (tw_re / tw_im [n_fft / 2] = cos / -sin(2 pi k / n_fft)), no
// vendor FFT.
//
// Protocol.  A workgroup of 256 threads runs two transforms side by side, 128 threads each (c = tid >> 7 picks the transform and
// its re / im arrays, t = tid & 127 is the thread within it), and each transform carries TWO real frames: forward, frame 2c is the
// real part and frame 2c + 1 the imaginary part, separated afterwards by the symmetry of a real signal's spectrum (fft_split);
// inverse, Z[k] = X0[k] + i X1[k] with both spectra extended by their Hermitian symmetry, so Re z = x0 and Im z = x1.  The caller
// stores its input BIT-REVERSED (fft_brev), synchronises, and calls fft_lds from all 256 threads: radix-2 decimation in time, in
// place, one __syncthreads() per stage, the result in natural order.  The inverse uses the conjugate twiddles of the same table; its
// factor 1 / n_fft is the caller's.
//
// Layout.  Index i lives at fft_skew(i) = i + (i >> 6), so an array takes fft_ld(n_fft) floats: in the first stage a wave touches
// 128 consecutive floats at stride 2, which would be two lanes per bank (64 banks of 4 bytes) -- the skew moves the second half onto
// the odd banks.  Stages with a half-size of 2 .. 16 keep a 2-way conflict (4-way without the skew); from 32 on the accesses are
// consecutive.
#pragma once
#include "common.hpp"

constexpr int FFT_MAX = 2048;

VBX_DEV int fft_skew(int i) { return i + (i >> 6); }
constexpr int fft_ld(int n_fft) { return n_fft + (n_fft >> 6); }
// where element j of the input goes
VBX_DEV int fft_brev(int j, int log2n) { return fft_skew((int)(__brev((unsigned)j) >> (32 - log2n))); }

// in-place radix-2 DIT over bit-reversed input: forward (twiddle e^{-i ..}) or INVERSE (its conjugate).  All 256 threads call it.
template <bool INVERSE>
VBX_DEV void fft_lds(float* re, float* im, const float* __restrict__ tw_re, const float* __restrict__ tw_im, int log2n, int half_n,
                     int t) {
  for (int s = 0; s < log2n; s++) {
    const int half = 1 << s, tstep = half_n >> s;
    for (int q = t; q < half_n; q += 128) {
      const int pos = q & (half - 1);
      const int i0 = fft_skew(((q >> s) << (s + 1)) + pos), i1 = fft_skew(((q >> s) << (s + 1)) + pos + half);
      const float wr = tw_re[pos * tstep], wi = INVERSE ? -tw_im[pos * tstep] : tw_im[pos * tstep];
      const float xr = re[i1], xi = im[i1];
      const float br = xr * wr - xi * wi, bi = xr * wi + xi * wr;
      const float ar = re[i0], ai = im[i0];
      re[i0] = ar + br; im[i0] = ai + bi;
      re[i1] = ar - br; im[i1] = ai - bi;
    }
    __syncthreads();
  }
}

// bin k of the two real frames a forward transform carried: A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2i)
struct FftPair { float ar, ai, br, bi; };
VBX_DEV FftPair fft_split(const float* re, const float* im, int k, int n_fft) {
  const int i0 = fft_skew(k), i1 = fft_skew((n_fft - k) & (n_fft - 1));
  const float zr = re[i0], zi = im[i0], nr = re[i1], ni = im[i1];
  return FftPair{0.5f * (zr + nr), 0.5f * (zi - ni), 0.5f * (zi + ni), -0.5f * (zr - nr)};
}

// ---- host side
static inline int fft_log2(int n_fft) {
  int log2n = 0;
  while ((1 << log2n) < n_fft) log2n++;
  return log2n;
}
static inline int fft_check_size(const char* who, int n_fft) {
  VBX_REQUIRE(n_fft >= 256 && n_fft <= FFT_MAX && (n_fft & (n_fft - 1)) == 0, "%s: n_fft must be a power of two in 256 .. 2048", who);
  return 0;
}
