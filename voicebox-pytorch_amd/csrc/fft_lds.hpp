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
//
// Mixed radix (inverse only: gl_synth_kernel<true>).  n_fft = 5 M, M = 2^m in 64 .. 256 (320, 640, 1280), decimation in time with the
// radix-5 stage last: X[k + q M] = sum_r W5^{-q r} (W_N^{-r k} X_r[k]) for the inverse, X_r the M-point transform of the elements
// j = 5 a + r.  The caller stores element j at fft_map5(j) = r M + bitrev_m(a), so the five sub-arrays are contiguous, each
// bit-reversed; fft_lds5_inverse runs the m radix-2 stages over all 5 M / 2 butterflies at once (every radix-2 block lies inside one
// sub-array; W_M^p = W_N^{5 p}, so the SAME [n_fft / 2] table serves, read at 5 times the stride) and then one in-place radix-5 pass:
// thread k reads r M + k and writes q M + k, consecutive in k, one __syncthreads() after it.  r k reaches 4 (M - 1) > n_fft / 2: the
// pass reads the table at r k - n_fft / 2 and negates (W^{j + N/2} = -W^j).
#pragma once
#include "common.hpp"

constexpr int FFT_MAX = 2048;

VBX_DEV int fft_skew(int i) { return i + (i >> 6); }
constexpr int fft_ld(int n_fft) { return n_fft + (n_fft >> 6); }
// where element j of the input goes
VBX_DEV int fft_brev(int j, int log2n) { return fft_skew((int)(__brev((unsigned)j) >> (32 - log2n))); }

// in-place radix-2 DIT over bit-reversed input: forward (twiddle e^{-i ..}) or INVERSE (its conjugate).  All 256 threads call it.
// TWMUL = 5 is the radix-2 part of the mixed-radix transform: log2n = m stages over half_n = 5 M / 2 butterflies, table stride times 5.
template <bool INVERSE, int TWMUL = 1>
VBX_DEV void fft_lds(float* re, float* im, const float* __restrict__ tw_re, const float* __restrict__ tw_im, int log2n, int half_n,
                     int t) {
  for (int s = 0; s < log2n; s++) {
    const int half = 1 << s, tstep = TWMUL * ((half_n / TWMUL) >> s);
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

// where element j = 5 a + r of the input of a 5 * 2^m-point transform goes
VBX_DEV int fft_map5(int j, int m) {
  const int a = j / 5, r = j - 5 * a;
  return fft_skew((r << m) + (int)(__brev((unsigned)a) >> (32 - m)));
}

// cos / sin of 2 pi / 5 and 4 pi / 5: fp32 roundings of the fp64 values
constexpr float FFT_C1 = (float)0.30901699437494742, FFT_C2 = (float)-0.80901699437494742;
constexpr float FFT_S1 = (float)0.95105651629515357, FFT_S2 = (float)0.58778525229247313;

// the INVERSE 5 * 2^m-point transform over input stored by fft_map5, result in natural order.  All 256 threads call it.
VBX_DEV void fft_lds5_inverse(float* re, float* im, const float* __restrict__ tw_re, const float* __restrict__ tw_im, int m, int n_fft,
                              int t) {
  const int half_n = n_fft >> 1, M = 1 << m;
  fft_lds<true, 5>(re, im, tw_re, tw_im, m, half_n, t);
  for (int k = t; k < M; k += 128) {
    float yr[5], yi[5];
    yr[0] = re[fft_skew(k)];
    yi[0] = im[fft_skew(k)];
#pragma unroll
    for (int r = 1; r < 5; r++) {
      int j = r * k;  // < 4 M = 1.6 * half_n
      const bool neg = j >= half_n;
      j = neg ? j - half_n : j;
      float wr = tw_re[j], wi = -tw_im[j];  // conj(W_N^j) = e^{+2 pi i j / N}
      if (neg) { wr = -wr; wi = -wi; }
      const int i = fft_skew((r << m) + k);
      const float xr = re[i], xi = im[i];
      yr[r] = xr * wr - xi * wi;
      yi[r] = xr * wi + xi * wr;
    }
    const float t1r = yr[1] + yr[4], t1i = yi[1] + yi[4], t2r = yr[2] + yr[3], t2i = yi[2] + yi[3];
    const float t3r = yr[1] - yr[4], t3i = yi[1] - yi[4], t4r = yr[2] - yr[3], t4i = yi[2] - yi[3];
    const float m1r = yr[0] + FFT_C1 * t1r + FFT_C2 * t2r, m1i = yi[0] + FFT_C1 * t1i + FFT_C2 * t2i;
    const float m2r = yr[0] + FFT_C2 * t1r + FFT_C1 * t2r, m2i = yi[0] + FFT_C2 * t1i + FFT_C1 * t2i;
    const float n1r = FFT_S1 * t3r + FFT_S2 * t4r, n1i = FFT_S1 * t3i + FFT_S2 * t4i;
    const float n2r = FFT_S2 * t3r - FFT_S1 * t4r, n2i = FFT_S2 * t3i - FFT_S1 * t4i;
    // X[k + q M] = sum_r y_r e^{+2 pi i q r / 5}:  X1, X4 = m1 +- i n1;  X2, X3 = m2 +- i n2
    re[fft_skew(k)] = yr[0] + t1r + t2r;
    im[fft_skew(k)] = yi[0] + t1i + t2i;
    re[fft_skew(M + k)] = m1r - n1i;
    im[fft_skew(M + k)] = m1i + n1r;
    re[fft_skew(2 * M + k)] = m2r - n2i;
    im[fft_skew(2 * M + k)] = m2i + n2r;
    re[fft_skew(3 * M + k)] = m2r + n2i;
    im[fft_skew(3 * M + k)] = m2i - n2r;
    re[fft_skew(4 * M + k)] = m1r + n1i;
    im[fft_skew(4 * M + k)] = m1i - n1r;
  }
  __syncthreads();
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
// the mixed-radix sizes 5 * 2^m, m = 6 .. 8, which only the inverse-only entry points serve
static inline bool fft_is_radix5(int n_fft) { return n_fft == 320 || n_fft == 640 || n_fft == 1280; }
static inline int fft_check_size_inverse(const char* who, int n_fft) {
  VBX_REQUIRE(fft_is_radix5(n_fft) || (n_fft >= 256 && n_fft <= FFT_MAX && (n_fft & (n_fft - 1)) == 0),
              "%s: n_fft must be a power of two in 256 .. 2048 or one of 320, 640, 1280", who);
  return 0;
}
