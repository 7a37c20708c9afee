// Sample-rate conversion in front of a codec (voicebox_pytorch_amd.resample; the reference resamples x1 and cond before
// audio_enc_dec.encode, voicebox_pytorch.py:1359-1371): the polyphase windowed-sinc FIR of torchaudio.functional.resample,
//   y[q * nw + p] = sum_k h[p][k] * x[q * orig + k - width],   x = 0 outside [0, L),   p in [0, nw), k in [0, K),
// with orig : nw the reduced rate pair.  One kernel, fp32, no atomics; every output sample is one serial sum in tap order, so a rerun
// gives the same bits.
//
// The bank arrives COMPACTED and run-major: of row h[p][.] only the run [start[p], start[p] + len[p]) that holds its non-zero taps
// (with the Hann window everything past the clamp rounds to exactly 0.0f: 7 .. 13 % of a deep bank is left; a Kaiser bank has no
// zeros and its runs are whole rows), stored as taps[i][p] = h[p][start[p] + i], i < run_max.  Lanes walk consecutive output samples
// = consecutive phases, so at step i a wave reads consecutive floats of taps -- through L1 / L2, the bank is never staged (dense it
// reaches 412 KB for common pairs, more than the LDS).  A workgroup serves T consecutive output samples of one row and stages their
// input span, (frames touched - 1) * orig + K samples, in the LDS once, zero-filled past both ends of the row: no padded copy of the
// wave exists in HBM.  Input reads of neighbouring phases fall on the same or neighbouring LDS words (orig / nw apart on average).
#include "common.hpp"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;          // output samples per workgroup, halved until the input span fits
constexpr int RS_LDS_FLOATS = 16384;   // 64 KiB: the span of a tile, and so the longest filter (K) that is served

// frames of orig input samples that T consecutive outputs can touch beyond their first one, whatever phase the tile starts at
inline long rs_extra_frames(int T, int nw) { return ((long)nw - 1 + T - 1) / nw; }

// LENS (vbx_resample_lens, include/vbx.h "ragged waves"): row r is the wave of lens[r] samples it would be alone -- staged as zeros
// from lens[r] on, its outputs from ceil(nw lens[r] / orig) on stored as 0.0.
template <bool LENS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const float* __restrict__ taps, const int* __restrict__ start,
                                                              const int* __restrict__ len, int rows, long L, long Lout, int orig,
                                                              int nw, int width, int K, int run_max, int T, const int* __restrict__ lens) {
  extern __shared__ float xs[];
  const int tid = threadIdx.x;
  const long o0 = (long)blockIdx.x * T;                       // first output sample of the tile
  const int nout = (int)(Lout - o0 < T ? Lout - o0 : T);
  const long q_lo = o0 / nw;                                  // its frame
  const int r0 = (int)(o0 - q_lo * nw);                       // and phase
  const int span = ((r0 + nout - 1) / nw) * orig + K;         // <= rs_extra_frames(T, nw) * orig + K <= RS_LDS_FLOATS (host)
  const long in0 = q_lo * orig - width;                       // input sample held by xs[0]; negative at the head of a row
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* xr = x + (long)row * L;
    long Lb = L, Lob = Lout;
    if (LENS) {
      const long l = lens[row];
      Lb = l < 1 ? 1 : (l > L ? L : l);
      Lob = (Lb * nw + orig - 1) / orig;  // <= Lout: the host checked Lout = ceil(nw L / orig)
      if (o0 >= Lob) {  // a tile wholly behind the row (the same for every thread: no barrier is skipped by some)
        for (int j = tid; j < nout; j += RS_THREADS) y[(long)row * Lout + o0 + j] = 0.f;
        continue;
      }
    }
    for (int i = tid; i < span; i += RS_THREADS) {
      const long g = in0 + i;
      xs[i] = (g >= 0 && g < Lb) ? xr[g] : 0.f;
    }
    __syncthreads();
    for (int j = tid; j < nout; j += RS_THREADS) {
      const int jj = r0 + j, dq = jj / nw, p = jj - dq * nw;
      const int s = start[p] > 0 ? start[p] : 0;
      int n = len[p] < run_max ? len[p] : run_max;            // a run stays inside the compacted bank ...
      n = n < K - s ? n : K - s;                              // ... and inside the row: reads never leave the staged span
      const float* xp = xs + dq * orig + s;
      const float* hp = taps + p;
      float acc = 0.f;
      int i = 0;
      for (; i + 4 <= n; i += 4) {  // four taps in flight; the sum keeps its tap order
        const float h0 = hp[(long)i * nw], h1 = hp[(long)(i + 1) * nw], h2 = hp[(long)(i + 2) * nw], h3 = hp[(long)(i + 3) * nw];
        acc = fmaf(h0, xp[i], acc);
        acc = fmaf(h1, xp[i + 1], acc);
        acc = fmaf(h2, xp[i + 2], acc);
        acc = fmaf(h3, xp[i + 3], acc);
      }
      for (; i < n; i++) acc = fmaf(hp[(long)i * nw], xp[i], acc);
      y[(long)row * Lout + o0 + j] = (LENS && o0 + j >= Lob) ? 0.f : acc;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int vbx_resample_max_taps(void) { return RS_LDS_FLOATS; }

static int resample_launch(const int* lens, const float* x, float* y, const float* taps, const int* start, const int* len, int rows, long L, long Lout,
                            int orig, int nw, int width, int K, int run_max, void* stream) {
  VBX_REQUIRE(x && y && taps && start && len && rows > 0, "vbx_resample: bad args");
  VBX_REQUIRE(L > 0 && L <= 2147483647L, "vbx_resample: rows of 1 .. 2^31 - 1 samples (got %ld)", L);
  VBX_REQUIRE(orig > 0 && nw > 0 && width >= 0 && K >= orig && run_max > 0 && run_max <= K, "vbx_resample: bad filter geometry");
  const long frames = (L + orig - 1) / orig;  // ceil(nw * L / orig) <= nw * ceil(L / orig): every output reads a staged frame
  VBX_REQUIRE(Lout > 0 && Lout <= frames * nw, "vbx_resample: at most nw * ceil(L / orig) output samples per row (got %ld)", Lout);
  VBX_REQUIRE(K <= RS_LDS_FLOATS, "vbx_resample: a filter of %d taps does not fit the LDS (at most %d)", K, RS_LDS_FLOATS);
  int T = RS_TILE;
  while (T > 1 && rs_extra_frames(T, nw) * orig + K > RS_LDS_FLOATS) T >>= 1;
  const long span = rs_extra_frames(T, nw) * orig + K;  // T = 1: no extra frame, K floats
  const long tiles = (Lout + T - 1) / T;
  VBX_REQUIRE(span <= RS_LDS_FLOATS && tiles <= 2147483647L, "vbx_resample: too many output tiles (%ld)", tiles);
  const dim3 grid((unsigned)tiles, rows < 65535 ? rows : 65535);
  if (lens) {
    VBX_REQUIRE(Lout == (L * nw + orig - 1) / orig, "vbx_resample_lens: Lout must be ceil(nw * L / orig) (got %ld)", Lout);
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), (size_t)span * sizeof(float), (hipStream_t)stream, x, y, taps, start,
                       len, rows, L, Lout, orig, nw, width, K, run_max, T, lens);
  } else {
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), (size_t)span * sizeof(float), (hipStream_t)stream, x, y, taps, start,
                       len, rows, L, Lout, orig, nw, width, K, run_max, T, (const int*)nullptr);
  }
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_resample(const float* x, float* y, const float* taps, const int* start, const int* len, int rows, long L, long Lout,
                            int orig, int nw, int width, int K, int run_max, void* stream) {
  return resample_launch(nullptr, x, y, taps, start, len, rows, L, Lout, orig, nw, width, K, run_max, stream);
}

extern "C" int vbx_resample_lens(const float* x, const int* lens, float* y, const float* taps, const int* start, const int* len, int rows,
                                 long L, long Lout, int orig, int nw, int width, int K, int run_max, void* stream) {
  VBX_REQUIRE(lens, "vbx_resample_lens: lens is NULL (vbx_resample is the entry without lengths)");
  return resample_launch(lens, x, y, taps, start, len, rows, L, Lout, orig, nw, width, K, run_max, stream);
}
