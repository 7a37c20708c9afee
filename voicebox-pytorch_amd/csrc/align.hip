// Aligner primitives (voicebox_pytorch_amd.maximum_path / forward_sum_loss / ForwardSumLoss; what the reference's DurationPredictor
// training branch takes from naturalspeech2_pytorch, voicebox_pytorch.py:841-876): monotonic alignment search and the forward-sum
// (CTC) loss.  Both are recurrences over the T query frames; a workgroup owns one batch row and a thread owns one key, for all T.
//
//   vbx_maximum_path      Q[y][x] = max(Q[y-1][x], Q[y-1][x-1]) + value[y][x] over the reachable band, then the backtrack from
//                         key_len - 1 (a tie stays on the key); path 0 / 1 [B, T, K] and durations int64 [B, K]
//   vbx_forward_sum_fwd   per frame lse = logsumexp(blank, keys < key_len) (one wave per frame, every CU), then the CTC alpha
//                         recursion with target 1 .. key_len; nll = -log Z per row, 0 for a row without a monotonic path
//   vbx_forward_sum_bwd   the beta recursion from the end and the gradient through the fused pad + mask + log-softmax
//
// The serial loop holds row t - 1 of the table in registers.  The neighbour key's value comes by a wave shuffle; across a wave
// boundary it crosses two LDS words that alternate with the parity of t, so a step costs ONE barrier (none when K <= 64).  The
// inputs of AL_PF steps are fetched ahead of the steps that use them: the loads do not depend on the recurrence.
//
// maximum_path never stores the fp32 table.  Per row and wave it keeps the 64 decision bits of the backtrack ("this cell was reached
// from the key on its left") as one ballot word, stored by lane 0.  The backtrack index moves at most one column per row, so for 64
// rows at a time lane r of wave 0 fetches the two words around the index for row y - r, and the 64 steps run on wave-uniform
// values read with readlane.  The 64 columns cross the LDS and EVERY thread writes its column of those 64 path rows (zeros and
// the single one) and counts its own duration: no atomics, no thread writes another thread's cell.
//
// forward-sum: thread j owns label j (extended state 2 j + 1) and the blank after it (2 j + 2); the leading blank (state 0) can
// only be reached from itself, so it is a running sum kept by every thread and used by thread 0.  The occupancies of all
// extended states of a frame sum to one, so d nll / d x[t][j] = softmax(t)[j] - occupancy(t, label j) and the backward needs alpha of the
// LABEL states only: alpha is kept as [B, T, K], not [B, T, 2 K + 1], and no blank occupancy is ever summed.
// The states (alpha, beta, lse) are fp64 sums of fp32-evaluated libm terms (see al_lae2); maximum_path is fp32 throughout.  No
// atomics, a fixed order of every sum, nothing that depends on B.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int AL_MAXK = 1024;  // one thread per key
constexpr int AL_PF = 8;       // steps whose inputs are fetched ahead of the serial loop

#define AL_NINF (-__builtin_inff())

// a length as the kernels use it: clamped into [0, full], so that no length can index outside the tensors
VBX_DEV int al_len(const int* lens, int b, int full) {
  const int v = lens ? lens[b] : full;
  return v < 0 ? 0 : (v > full ? full : v);
}

VBX_DEV unsigned long long al_readlane64(unsigned long long v, int r) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, r);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), r);
  return ((unsigned long long)hi << 32) | lo;
}

// The forward-sum states are kept in fp64 and their transcendental parts are taken in fp32: log(exp(a) + exp(b)) = max + a term in
// [0, log 3] whose fp32 error is absolute, ~1e-7, whatever the magnitude of the states -- which grows with T, so an fp32 state
// would lose ulp(|alpha|) per frame (1e-3 at T = 2500).  The fp64 part of a step is a few additions.
VBX_DEV double al_lae2(double a, double b) {
  const double m = fmax(a, b);
  if (m == (double)AL_NINF) return m;
  return m + (double)log1pf(expf((float)(fmin(a, b) - m)));  // -inf - m = -inf: exp gives 0
}
// three terms: the largest contributes exactly 1, so the sum lies in [1, 3]
VBX_DEV double al_lae3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == (double)AL_NINF) return m;
  return m + (double)logf(expf((float)(a - m)) + expf((float)(b - m)) + expf((float)(c - m)));
}
VBX_DEV double al_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(AL_MAXK) void maximum_path_kernel(const float* __restrict__ value, const int* __restrict__ qlens,
                                                               const int* __restrict__ klens, float* __restrict__ path,
                                                               long* __restrict__ dur, unsigned long long* __restrict__ bits, int T,
                                                               int K, int W) {
  __shared__ float edge[2][AL_MAXK / 64];  // Q of lane 63 of every wave, by the parity of the row
  __shared__ int cols[64];                 // the path's column in the 64 rows of one backtrack batch
  __shared__ int next_idx;
  const int b = blockIdx.x, x = threadIdx.x, lane = x & 63, wave = x >> 6;
  const int q = al_len(qlens, b, T), k = al_len(klens, b, K);
  const bool feasible = k >= 1 && q >= k;
  const float* v = value + (long)b * T * K;
  float* p = path + (long)b * T * K;
  unsigned long long* bw = bits + (long)b * T * W;
  int count = 0;

  if (feasible) {
    float prev = AL_NINF;  // Q[y - 1][x]
    for (int y0 = 0; y0 < q; y0 += AL_PF) {
      float val[AL_PF];
#pragma unroll
      for (int i = 0; i < AL_PF; i++) val[i] = x < k && y0 + i < q ? v[(long)(y0 + i) * K + x] : 0.f;
#pragma unroll
      for (int i = 0; i < AL_PF; i++) {
        const int y = y0 + i;
        if (y >= q) break;
        float left = __shfl_up(prev, 1, 64);
        if (lane == 0) left = wave > 0 && y > 0 ? edge[(y + 1) & 1][wave - 1] : AL_NINF;
        const bool in = x < k && x <= y && x >= k + y - q;   // the reachable band
        const bool move = x != 0 && (x == y || prev < left);  // strict: a tie stays on the key
        float cur = AL_NINF;
        if (in) cur = y == 0 ? val[i] : (move ? left : prev) + val[i];
        const unsigned long long word = __ballot(in && move);
        if (lane == 0 && y > 0) bw[(long)y * W + wave] = word;
        prev = cur;
        if (W > 1) {
          if (lane == 63) edge[y & 1][wave] = cur;
          __syncthreads();
        }
      }
    }
    __threadfence_block();  // the ballot words are read back by wave 0
    __syncthreads();

    int idx = k - 1;
    for (int y = q - 1; y >= 0; y -= 64) {
      const int n = y + 1 < 64 ? y + 1 : 64;
      if (wave == 0) {
        idx = __builtin_amdgcn_readfirstlane(idx);
        const int wh = idx >> 6, yy = y - lane;
        unsigned long long hi = 0, lo = 0;  // row 0 has no decision: the index is 0 there
        if (yy >= 1) {
          hi = bw[(long)yy * W + wh];
          if (wh > 0) lo = bw[(long)yy * W + wh - 1];
        }
        int mycol = 0;
        for (int r = 0; r < n; r++) {
          if (lane == r) mycol = idx;
          const unsigned long long h = al_readlane64(hi, r), l = al_readlane64(lo, r);
          const unsigned long long w = (idx >> 6) == wh ? h : l;  // idx >= idx0 - 63: one of the two words
          idx -= (int)((w >> (idx & 63)) & 1ull);
        }
        if (lane < n) cols[lane] = mycol;
        if (lane == 0) next_idx = idx;
      }
      __syncthreads();
      idx = next_idx;
      if (x < K) {
        for (int r = 0; r < n; r++) {
          const bool on = cols[r] == x;
          p[(long)(y - r) * K + x] = on ? 1.f : 0.f;
          count += on ? 1 : 0;
        }
      }
      __syncthreads();
    }
  }
  if (x < K) {
    for (int t = feasible ? q : 0; t < T; t++) p[(long)t * K + x] = 0.f;
    dur[(long)b * K + x] = count;
  }
}

// one wave per frame: lse[b][t] = logsumexp(blank, x[b][t][0 .. key_len)) in fp64 (fp32 exponentials, summed in fp64 in a fixed
// order); frames past query_len get 0 and are never read
__global__ __launch_bounds__(256) void forward_sum_lse_kernel(const float* __restrict__ x, const int* __restrict__ klens,
                                                              const int* __restrict__ qlens, float blank, double* __restrict__ lse,
                                                              long rows, int T, int K) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int b = (int)(row / T), t = (int)(row - (long)b * T);
  const int q = al_len(qlens, b, T), k = al_len(klens, b, K);
  if (t >= q) {
    if (lane == 0) lse[row] = 0.0;
    return;
  }
  const float* xr = x + row * K;
  float m = blank;
  for (int j = lane; j < k; j += 64) m = fmaxf(m, xr[j]);
  m = wave_max(m);
  double s = 0.0;
  for (int j = lane; j < k; j += 64) s += (double)expf(xr[j] - m);
  s = al_wave_sum(s) + (double)expf(blank - m);
  if (lane == 0) lse[row] = (double)m + log(s);
}

__global__ __launch_bounds__(AL_MAXK) void forward_sum_fwd_kernel(const float* __restrict__ x, const int* __restrict__ klens,
                                                                  const int* __restrict__ qlens, float blank,
                                                                  const double* __restrict__ lse, double* __restrict__ alpha,
                                                                  float* __restrict__ nll, double* __restrict__ logz, int T, int K) {
  __shared__ double edge[2][AL_MAXK / 64][2];  // (label, blank after it) of lane 63 of every wave, by the parity of t
  const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6, nw = blockDim.x >> 6;
  const int q = al_len(qlens, b, T), k = al_len(klens, b, K);
  if (!(k >= 1 && q >= k)) {  // no monotonic path: loss 0 (zero_infinity)
    if (j == 0) { nll[b] = 0.f; logz[b] = 0.0; }
    return;
  }
  const bool act = j < k;
  const double ninf = (double)AL_NINF;
  const float* xr = x + (long)b * T * K;
  const double* lr = lse + (long)b * T;
  double* ar = alpha ? alpha + (long)b * T * K : nullptr;
  // before the first frame: all the mass on the leading blank
  double a = ninf, bl = ninf, b0 = 0.0;
  for (int t0 = 0; t0 < q; t0 += AL_PF) {
    float xv[AL_PF];
    double ls[AL_PF];
#pragma unroll
    for (int i = 0; i < AL_PF; i++) {
      const bool live = t0 + i < q;
      xv[i] = act && live ? xr[(long)(t0 + i) * K + j] : 0.f;
      ls[i] = live ? lr[t0 + i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < AL_PF; i++) {
      const int t = t0 + i;
      if (t >= q) break;
      double pa = __shfl_up(a, 1, 64), pb = __shfl_up(bl, 1, 64);  // label j - 1 and the blank between
      if (lane == 0) {
        if (wave > 0 && t > 0) {
          pa = edge[(t + 1) & 1][wave - 1][0];
          pb = edge[(t + 1) & 1][wave - 1][1];
        } else {
          pa = ninf;
          pb = wave == 0 ? b0 : ninf;
        }
      }
      const double lpb = (double)blank - ls[i], lpj = (double)xv[i] - ls[i];
      const double na = act ? al_lae3(a, pb, pa) + lpj : ninf;
      const double nb = act ? al_lae2(bl, a) + lpb : ninf;
      b0 += lpb;
      a = na;
      bl = nb;
      if (act && ar) ar[(long)t * K + j] = a;
      if (nw > 1) {
        if (lane == 63) { edge[t & 1][wave][0] = a; edge[t & 1][wave][1] = bl; }
        __syncthreads();
      }
    }
  }
  if (j == k - 1) {
    const double lz = al_lae2(bl, a);
    const bool ok = lz > ninf && lz < -ninf;  // false for a NaN too
    nll[b] = ok ? (float)-lz : 0.f;
    logz[b] = lz;
  }
}

__global__ __launch_bounds__(AL_MAXK) void forward_sum_bwd_kernel(const float* __restrict__ x, const int* __restrict__ klens,
                                                                  const int* __restrict__ qlens, float blank,
                                                                  const double* __restrict__ lse, const double* __restrict__ alpha,
                                                                  const double* __restrict__ logz, const float* __restrict__ gout,
                                                                  float* __restrict__ grad, int T, int K) {
  __shared__ double edge[2][AL_MAXK / 64];  // beta of the label of lane 0 of every wave, by the parity of t
  const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6, nw = blockDim.x >> 6;
  const int q = al_len(qlens, b, T), k = al_len(klens, b, K);
  const double ninf = (double)AL_NINF;
  const double lz = logz[b];
  const float g = gout[b];
  const bool ok = k >= 1 && q >= k && lz > ninf && lz < -ninf;
  const bool act = j < k;
  const float* xr = x + (long)b * T * K;
  const double* lr = lse + (long)b * T;
  const double* ar = alpha + (long)b * T * K;
  float* gr = grad + (long)b * T * K;
  if (ok) {
    // after the last frame: all the mass on the trailing blank (the blank after label k - 1)
    double a = ninf, bl = j == k - 1 ? 0.0 : ninf;
    for (int t0 = q - 1; t0 >= 0; t0 -= AL_PF) {
      float xv[AL_PF];
      double ls[AL_PF], al[AL_PF];
#pragma unroll
      for (int i = 0; i < AL_PF; i++) {
        const bool live = t0 - i >= 0;
        xv[i] = act && live ? xr[(long)(t0 - i) * K + j] : 0.f;
        al[i] = act && live ? ar[(long)(t0 - i) * K + j] : 0.0;
        ls[i] = live ? lr[t0 - i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < AL_PF; i++) {
        const int t = t0 - i;
        if (t < 0) break;
        double na = __shfl_down(a, 1, 64);  // beta of label j + 1
        if (lane == 63) na = wave + 1 < nw && t < q - 1 ? edge[(t + 1) & 1][wave + 1] : ninf;
        const double lpb = (double)blank - ls[i], lpj = (double)xv[i] - ls[i];
        double nla = ninf, nbl = ninf;
        if (act) {
          nla = al_lae3(a, bl, na) + lpj;
          nbl = al_lae2(bl, na) + lpb;
        }
        a = nla;
        bl = nbl;
        // softmax share minus the occupancy of label j at frame t
        if (j < K) gr[(long)t * K + j] = act ? g * (expf((float)lpj) - expf((float)(al[i] + a - lpj - lz))) : 0.f;
        if (nw > 1) {
          if (lane == 0) edge[t & 1][wave] = a;
          __syncthreads();
        }
      }
    }
  }
  if (j < K)
    for (int t = ok ? q : 0; t < T; t++) gr[(long)t * K + j] = 0.f;
}

int al_check(int B, int T, int K, const char* who) {
  VBX_REQUIRE(K >= 1 && K <= AL_MAXK, "%s: the number of keys must be in 1 .. %d (got %d)", who, AL_MAXK, K);
  VBX_REQUIRE(B >= 1 && T >= 1, "%s: need B >= 1 and T >= 1", who);
  VBX_REQUIRE((long)B * T < (1L << 31), "%s: too many frames", who);
  return 0;
}

}  // namespace

extern "C" int vbx_maximum_path(const float* value, const int* query_lens, const int* key_lens, float* path, long* durations,
                                unsigned long long* bits, int B, int T, int K, void* stream) {
  VBX_REQUIRE(value && path && durations && bits, "vbx_maximum_path: null operand");
  if (int rc = al_check(B, T, K, "vbx_maximum_path")) return rc;
  const int W = cdiv(K, 64);
  hipLaunchKernelGGL(maximum_path_kernel, dim3(B), dim3(64 * W), 0, (hipStream_t)stream, value, query_lens, key_lens, path, durations,
                     bits, T, K, W);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_forward_sum_fwd(const float* x, const int* key_lens, const int* query_lens, float blank_logprob, double* lse,
                                   double* alpha, float* nll, double* logz, int B, int T, int K, void* stream) {
  VBX_REQUIRE(x && lse && nll && logz, "vbx_forward_sum_fwd: null operand");
  if (int rc = al_check(B, T, K, "vbx_forward_sum_fwd")) return rc;
  VBX_REQUIRE(isfinite(blank_logprob), "vbx_forward_sum_fwd: blank_logprob must be finite");
  const long rows = (long)B * T;
  hipLaunchKernelGGL(forward_sum_lse_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, key_lens, query_lens,
                     blank_logprob, lse, rows, T, K);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(forward_sum_fwd_kernel, dim3(B), dim3(64 * cdiv(K, 64)), 0, (hipStream_t)stream, x, key_lens, query_lens,
                     blank_logprob, lse, alpha, nll, logz, T, K);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_forward_sum_bwd(const float* x, const int* key_lens, const int* query_lens, float blank_logprob, const double* lse,
                                   const double* alpha, const double* logz, const float* grad_nll, float* grad, int B, int T, int K,
                                   void* stream) {
  VBX_REQUIRE(x && lse && alpha && logz && grad_nll && grad, "vbx_forward_sum_bwd: null operand");
  if (int rc = al_check(B, T, K, "vbx_forward_sum_bwd")) return rc;
  hipLaunchKernelGGL(forward_sum_bwd_kernel, dim3(B), dim3(64 * cdiv(K, 64)), 0, (hipStream_t)stream, x, key_lens, query_lens,
                     blank_logprob, lse, alpha, logz, grad_nll, grad, T, K);
  VBX_LAUNCH_CHECK();
  return 0;
}
