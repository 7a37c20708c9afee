// The Aligner network (voicebox_pytorch_amd.Aligner / aligner_attention; the convolutional attention of "One TTS Alignment To Rule
// Them All" / RAD-TTS, which the reference's DurationPredictor takes from naturalspeech2_pytorch): the distance attention, its
// backward, and the small kernels around the convolution stacks, which themselves are vbx_gemm launches.
//
//   vbx_aligner_attn_fwd   logprob[t][j] = -tau * sum_c (q[t][c] - k[j][c])^2 and attn = softmax_j of it with masked keys filled
//                          with -FLT_MAX, in ONE launch.  A workgroup owns 32 query frames of one batch row; the row's key
//                          encodings pass through the LDS 64 keys at a time, lane = key, a wave holds 8 frames' sums in registers.
//                          The B x T x K x A difference tensor is never stored.  Every (t, j) cell belongs to one thread, which
//                          writes its logprob and reads it back for the softmax of its wave's rows.
//   vbx_aligner_attn_bwd   G = g_logprob + mask * attn * (g_attn - sum_j attn * g_attn)  (one wave per row), then
//                          dq[t] = -2 tau sum_j G[t][j] (q[t] - k[j]) and dk[j] = -2 tau sum_t G[t][j] (k[j] - q[t]): the SAME kernel
//                          with the roles of the two tensors exchanged.  A workgroup owns 16 rows of the tensor it differentiates and
//                          walks the other tensor 64 rows at a time through the LDS, in index order: one thread, one fixed-order
//                          fmaf chain per output element.  No atomics.
//   vbx_aligner_pack       the 16-bit GEMM operand row of a k-tap Conv1d (k = 1 or 3, zero padding at the ends of the tensor),
//                          column c * k + tap -- the weight's own [Cout, Cin * k] view, so no weight is ever permuted -- with the
//                          ReLU of the layer before applied on read; fp16, bf16 (backward) or the three-piece fp16 row
//                          [hi | hi 2^-8 | lo 2^8] that gives a layer in front of a ReLU fp32-accurate pre-activations
//   vbx_aligner_relu_bwd   g *= (pre > 0) in place and a bf16 copy (the operand of the dgrad / wgrad GEMMs)
//   vbx_aligner_fold       dx(t) = d[t + 1][tap 0] + d[t][tap 1] + d[t - 1][tap 2] of the dgrad's packed-layout output
//
// The sum of squares is the DIRECT form, an fp32 fmaf chain over the channels in index order: the expanded form
// |q|^2 + |k|^2 - 2 q.k cancels (1.2e5 units of 2^-24 at a common offset of 100), and the encodings are never rounded to fp16.
// fp32 throughout; nothing depends on B, so a row alone gives the bits it gives inside a batch.
#include <float.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int AA_MAXA = 128;  // attention channels: a 64-key chunk of that width is 33 KiB of LDS
constexpr int AA_TQ = 32;     // query frames per workgroup of the forward (4 waves x 8)
constexpr int AA_KC = 64;     // keys (forward) / rows of the other tensor (backward) per LDS chunk
constexpr int AA_TO = 16;     // rows a workgroup of the backward owns
constexpr int AA_ITEMS = AA_TO * AA_MAXA / 256;  // output elements per thread of the backward, at most

__global__ __launch_bounds__(256) void aligner_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const uint8_t* __restrict__ mask, float tau, float* attn, float* logp,
                                                               int T, int K, int A) {
  __shared__ float ks[AA_KC][AA_MAXA + 1];             // odd stride: lane = key reads without bank conflicts
  __shared__ __attribute__((aligned(16))) float qs[AA_MAXA][AA_TQ];  // transposed: the 8 frames of a wave are two 16-byte broadcasts
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < AA_TQ * A; i += 256) {
    const int tl = i / A, c = i - tl * A, t = t0 + tl;
    qs[c][tl] = t < T ? q[((long)b * T + t) * A + c] : 0.f;
  }
  for (int kc0 = 0; kc0 < K; kc0 += AA_KC) {
    __syncthreads();  // the chunk before has been read (first round: nothing yet)
    for (int i = tid; i < AA_KC * A; i += 256) {
      const int jl = i / A, c = i - jl * A, j = kc0 + jl;
      ks[jl][c] = j < K ? k[((long)b * K + j) * A + c] : 0.f;
    }
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; r++) acc[r] = 0.f;
    for (int c = 0; c < A; c++) {
      const float kv = ks[lane][c];
      const f32x4 qa = *(const f32x4*)&qs[c][wave * 8], qb = *(const f32x4*)&qs[c][wave * 8 + 4];
      float d;
      d = qa.x - kv; acc[0] = fmaf(d, d, acc[0]);
      d = qa.y - kv; acc[1] = fmaf(d, d, acc[1]);
      d = qa.z - kv; acc[2] = fmaf(d, d, acc[2]);
      d = qa.w - kv; acc[3] = fmaf(d, d, acc[3]);
      d = qb.x - kv; acc[4] = fmaf(d, d, acc[4]);
      d = qb.y - kv; acc[5] = fmaf(d, d, acc[5]);
      d = qb.z - kv; acc[6] = fmaf(d, d, acc[6]);
      d = qb.w - kv; acc[7] = fmaf(d, d, acc[7]);
    }
    const int j = kc0 + lane;
    if (j < K) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const int t = t0 + wave * 8 + r;
        if (t < T) logp[((long)b * T + t) * K + j] = -tau * acc[r];
      }
    }
  }
  // the masked softmax of this wave's rows: lane reads back the cells (j = lane + 64 n) it wrote itself
  const uint8_t* mrow = mask ? mask + (long)b * K : nullptr;
  for (int r = 0; r < 8; r++) {
    const int t = t0 + wave * 8 + r;
    if (t >= T) break;  // wave-uniform
    const float* lrow = logp + ((long)b * T + t) * K;
    float* arow = attn + ((long)b * T + t) * K;
    float m = -FLT_MAX;
    for (int j = lane; j < K; j += 64) m = fmaxf(m, (mrow && !mrow[j]) ? -FLT_MAX : lrow[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < K; j += 64) s += expf(((mrow && !mrow[j]) ? -FLT_MAX : lrow[j]) - m);
    s = wave_sum(s);
    for (int j = lane; j < K; j += 64) arow[j] = expf(((mrow && !mrow[j]) ? -FLT_MAX : lrow[j]) - m) / s;
  }
}

// one wave per (b, t): G = g_logprob + mask * attn * (g_attn - sum_j attn * g_attn)
__global__ __launch_bounds__(256) void aligner_attn_gmap_kernel(const float* __restrict__ attn, const float* __restrict__ glp,
                                                                const float* __restrict__ ga, const uint8_t* __restrict__ mask,
                                                                float* __restrict__ G, long rows, int T, int K) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / T;
  const float* ar = attn + row * K;
  const float* gr = ga + row * K;
  const uint8_t* mrow = mask ? mask + b * K : nullptr;
  float s = 0.f;
  for (int j = lane; j < K; j += 64) s = fmaf(ar[j], gr[j], s);
  s = wave_sum(s);
  for (int j = lane; j < K; j += 64) {
    float v = (mrow && !mrow[j]) ? 0.f : ar[j] * (gr[j] - s);
    if (glp) v += glp[row * K + j];
    G[row * K + j] = v;
  }
}

// dx[o][c] = -2 tau sum_r G(o, r) (x[o][c] - y[r][c]), r = 0 .. Nr - 1 in order.  DK = false: x = q, y = k, G(o, r) = G[o][r];
// DK = true: x = k, y = q, G(o, r) = G[r][o] (G is [B, T, K] either way).
template <bool DK>
__global__ __launch_bounds__(256) void aligner_attn_grad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ G, float tau, float* __restrict__ dx, int No,
                                                                int Nr, int T, int K, int A) {
  __shared__ float ys[AA_KC][AA_MAXA];
  __shared__ float gs[AA_TO][AA_KC + 1];
  const int b = blockIdx.y, o0 = blockIdx.x * AA_TO, tid = threadIdx.x, items = AA_TO * A;
  float acc[AA_ITEMS], xv[AA_ITEMS];
  int ol[AA_ITEMS], cc[AA_ITEMS];
#pragma unroll
  for (int n = 0; n < AA_ITEMS; n++) {
    const int idx = tid + n * 256;
    const bool live = idx < items;
    ol[n] = live ? idx / A : 0;
    cc[n] = live ? idx - ol[n] * A : 0;
    const int o = o0 + ol[n];
    xv[n] = live && o < No ? x[((long)b * No + o) * A + cc[n]] : 0.f;
    acc[n] = 0.f;
  }
  for (int r0 = 0; r0 < Nr; r0 += AA_KC) {
    __syncthreads();
    for (int i = tid; i < AA_KC * A; i += 256) {
      const int rl = i / A, c = i - rl * A, r = r0 + rl;
      ys[rl][c] = r < Nr ? y[((long)b * Nr + r) * A + c] : 0.f;
    }
    for (int i = tid; i < AA_TO * AA_KC; i += 256) {
      int o_l, r_l;
      if (DK) { r_l = i / AA_TO; o_l = i - r_l * AA_TO; } else { o_l = i / AA_KC; r_l = i - o_l * AA_KC; }
      const int o = o0 + o_l, r = r0 + r_l;
      float g = 0.f;
      if (o < No && r < Nr) g = DK ? G[((long)b * T + r) * K + o] : G[((long)b * T + o) * K + r];
      gs[o_l][r_l] = g;
    }
    __syncthreads();
    const int nr = Nr - r0 < AA_KC ? Nr - r0 : AA_KC;
    for (int rl = 0; rl < nr; rl++) {
#pragma unroll
      for (int n = 0; n < AA_ITEMS; n++) acc[n] = fmaf(gs[ol[n]][rl], xv[n] - ys[rl][cc[n]], acc[n]);
    }
  }
  const float s = -2.f * tau;
#pragma unroll
  for (int n = 0; n < AA_ITEMS; n++) {
    const int idx = tid + n * 256, o = o0 + ol[n];
    if (idx < items && o < No) dx[((long)b * No + o) * A + cc[n]] = s * acc[n];
  }
}

__global__ __launch_bounds__(256) void aligner_pack_kernel(const float* __restrict__ x, u16* __restrict__ out, long total, int T, int C,
                                                           int taps, int relu, int channel_first, int fmt) {
  const long kc = (long)C * taps;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / C;
    const int c = (int)(i - m * C);
    const long b = m / T;
    const int t = (int)(m - b * T);
    u16* o = out + m * (fmt == 2 ? 3 * kc : kc) + (long)c * taps;
    for (int tap = 0; tap < taps; tap++) {
      const int tt = t + tap - (taps >> 1);
      float v = 0.f;
      if (tt >= 0 && tt < T) v = channel_first ? x[(b * C + c) * T + tt] : x[(b * T + tt) * C + c];
      if (relu) v = v < 0.f ? 0.f : v;
      if (fmt == 1) {
        o[tap] = f32_to_bf16(v);
      } else {
        const u16 hi = f32_to_f16_sat(v);
        o[tap] = hi;
        if (fmt == 2) {  // [hi | hi 2^-8 | lo 2^8]: the three-piece operand of the model's precise mode (vbx_split3_f16)
          const float h = f16_to_f32(hi);
          o[kc + tap] = f32_to_f16(h * 0.00390625f);
          o[2 * kc + tap] = f32_to_f16_sat((v - h) * 256.f);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void aligner_relu_bwd_kernel(float* __restrict__ g, const float* __restrict__ pre,
                                                               u16* __restrict__ gb, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float v = g[i];
    if (pre) {
      v = pre[i] > 0.f ? v : 0.f;
      g[i] = v;
    }
    gb[i] = f32_to_bf16(v);
  }
}

__global__ __launch_bounds__(256) void aligner_fold_kernel(const float* __restrict__ d, float* __restrict__ dx, long total, int T, int C,
                                                           int channel_first) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / C;
    const int c = (int)(i - m * C);
    const long b = m / T;
    const int t = (int)(m - b * T);
    const long ld = 3L * C;
    float s = t + 1 < T ? d[(m + 1) * ld + 3 * c] : 0.f;
    s += d[m * ld + 3 * c + 1];
    s += t > 0 ? d[(m - 1) * ld + 3 * c + 2] : 0.f;
    dx[channel_first ? (b * C + c) * T + t : i] = s;
  }
}

int aa_check(int B, int T, int K, int A, const char* who) {
  VBX_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && K >= 1, "%s: need 1 <= B <= 65535, T >= 1, K >= 1 (got %d, %d, %d)", who, B, T, K);
  VBX_REQUIRE(A >= 1 && A <= AA_MAXA, "%s: the attention channels must be in 1 .. %d (got %d)", who, AA_MAXA, A);
  VBX_REQUIRE((long)B * T < (1L << 31), "%s: too many frames", who);
  return 0;
}

int aa_blocks(long total) {
  const long b = (total + 255) / 256;
  return (int)(b > 8192 ? 8192 : b);
}

}  // namespace

extern "C" int vbx_aligner_attn_max_channels(void) { return AA_MAXA; }

extern "C" int vbx_aligner_attn_fwd(const float* q, const float* k, const uint8_t* mask, float temperature, float* attn, float* logprob,
                                    int B, int T, int K, int A, void* stream) {
  VBX_REQUIRE(q && k && attn && logprob, "vbx_aligner_attn_fwd: null operand");
  if (int rc = aa_check(B, T, K, A, "vbx_aligner_attn_fwd")) return rc;
  hipLaunchKernelGGL(aligner_attn_fwd_kernel, dim3(cdiv(T, AA_TQ), B), dim3(256), 0, (hipStream_t)stream, q, k, mask, temperature, attn,
                     logprob, T, K, A);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_aligner_attn_bwd(const float* q, const float* k, const uint8_t* mask, const float* attn, const float* g_logprob,
                                    const float* g_attn, float temperature, float* gmap, float* dq, float* dk, int B, int T, int K, int A,
                                    void* stream) {
  VBX_REQUIRE(q && k && (g_logprob || g_attn), "vbx_aligner_attn_bwd: null operand");
  VBX_REQUIRE(!g_attn || (attn && gmap), "vbx_aligner_attn_bwd: g_attn needs attn and the gmap scratch");
  if (int rc = aa_check(B, T, K, A, "vbx_aligner_attn_bwd")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* G = g_logprob;
  if (g_attn) {
    const long rows = (long)B * T;
    hipLaunchKernelGGL(aligner_attn_gmap_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, attn, g_logprob, g_attn, mask, gmap, rows, T, K);
    VBX_LAUNCH_CHECK();
    G = gmap;
  }
  if (dq) {
    hipLaunchKernelGGL(aligner_attn_grad_kernel<false>, dim3(cdiv(T, AA_TO), B), dim3(256), 0, st, q, k, G, temperature, dq, T, K, T, K, A);
    VBX_LAUNCH_CHECK();
  }
  if (dk) {
    hipLaunchKernelGGL(aligner_attn_grad_kernel<true>, dim3(cdiv(K, AA_TO), B), dim3(256), 0, st, k, q, G, temperature, dk, K, T, T, K, A);
    VBX_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int vbx_aligner_pack(const float* x, void* out, int B, int T, int C, int taps, int relu, int channel_first, int fmt,
                                void* stream) {
  VBX_REQUIRE(x && out && B >= 1 && T >= 1 && C >= 1, "vbx_aligner_pack: bad args");
  VBX_REQUIRE(fmt >= 0 && fmt <= 2, "vbx_aligner_pack: fmt is 0 (fp16), 1 (bf16) or 2 (fp16 hi | hi 2^-8 | lo 2^8), got %d", fmt);
  VBX_REQUIRE(taps == 1 || taps == 3, "vbx_aligner_pack: 1 or 3 taps (got %d)", taps);
  const long total = (long)B * T * C;
  hipLaunchKernelGGL(aligner_pack_kernel, dim3(aa_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, (u16*)out, total, T, C, taps, relu,
                     channel_first, fmt);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_aligner_relu_bwd(float* g, const float* pre, void* g_bf16, long n, void* stream) {
  VBX_REQUIRE(g && g_bf16 && n >= 1, "vbx_aligner_relu_bwd: bad args");
  hipLaunchKernelGGL(aligner_relu_bwd_kernel, dim3(aa_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, pre, (u16*)g_bf16, n);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_aligner_fold(const float* d, float* dx, int B, int T, int C, int channel_first, void* stream) {
  VBX_REQUIRE(d && dx && B >= 1 && T >= 1 && C >= 1, "vbx_aligner_fold: bad args");
  const long total = (long)B * T * C;
  hipLaunchKernelGGL(aligner_fold_kernel, dim3(aa_blocks(total)), dim3(256), 0, (hipStream_t)stream, d, dx, total, T, C, channel_first);
  VBX_LAUNCH_CHECK();
  return 0;
}
