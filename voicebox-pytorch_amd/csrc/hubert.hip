// HubertWithKmeans (voicebox-pytorch_amd/hubert.py): HuBERT base (Hsu et al. 2021, "HuBERT: self-supervised speech representation
// learning by masked prediction of hidden units") up to one encoder layer, then a k-means codebook: waves into semantic token ids on
// the device, inference only.  The launch sequence of one call at the base widths:
//
//   vbx_hubert_conv0_stats   wave fp32 [B, T] -> one (shift, sum, sum of squares) record per (row, chunk of 256 positions, channel) of
//                            the 1 -> C first convolution, then mean / rstd per (row, channel): the records combined in fp64, in order
//   vbx_hubert_conv0_apply   the same 10-tap fmaf chain again, GroupNorm(C, C) (over time), erf-GELU -> fp16 [B, L0, C]
//   vbx_hubert_conv  x 6     k 2 / 3, stride 2, no padding, no bias, erf-GELU: the implicit-GEMM tile core of seanet_tile.hpp
//   vbx_hubert_layernorm16   feature_projection.layer_norm over the fp16 rows -> fp16
//   vbx_gemm                 NT, VBX_EPI_F32: the projection C -> D with its bias -> x fp32 [B * N, D]
//   vbx_hubert_posconv       the grouped positional convolution (one product per group, K = k * D / groups, zero padding resolved as
//                            the span is staged, the dropped last sample never computed), bias, erf-GELU, + x -> fp32
//   vbx_hubert_layernorm     encoder.layer_norm -> fp32 rows and their fp16 copy (the next product's operand)
//   per layer 1 .. output_layer:
//     vbx_gemm               NT, VBX_EPI_F32: [q | k | v] = x16 . [Wq | Wk | Wv]^T + bias -> fp32 [B * N, 3D]
//     vbx_hubert_split_heads q16 (times vbx_attn_q_prescale(dim_head ** -0.5)), k16, v16 fp16 [B, H, N, 64]
//     vbx_attn_fwd           no mask
//     vbx_gemm               NT, VBX_EPI_F32: out_proj with bias and the residual;  vbx_hubert_layernorm
//     vbx_gemm               NT, VBX_EPI_GELU: intermediate_dense;  vbx_gemm NT, VBX_EPI_F32: output_dense with bias and the residual
//     vbx_hubert_layernorm
//   vbx_kmeans_assign        the Euclidean argmin over the codebook, fp32 throughout -> int64 [B, N]
//
// Precision contract (include/vbx.h): fp16 channel-last activations rounded once where they are stored, fp16 weights, every product's
// sum fp32 on v_mfma_f32_16x16x32_f16 in ascending k, norms / GELU (libm's erff) / statistics fp32.  Plain launches, no atomics, no
// workgroup waits for another: the same bits on every run, and a batch row's result does not depend on its neighbours.
//
// HubertLargeWithKmeans (the LARGE form: feat_extract_norm "layer", the pre-LN encoder of do_stable_layer_norm, an optional convolution
// bias) keeps the projection, the positional convolution, the products, the attention and the k-means of the sequence above; what differs:
//
//   vbx_wave_normalize       (normalize_wave=True only) per row (x - mean) / sqrt(var + eps): shifted sums per chunk of 4096 samples,
//                            combined in order in fp64, applied in fp64 -> fp32; with lens over the row's own samples, zeros past them
//   vbx_hubert_conv0_ln      the same fmaf chain, + bias, LayerNorm over the C channels of the position (two passes, fp32), erf-GELU
//                            -> fp16 [B, L0, C]: ONE launch, no statistic over time, no records
//   vbx_hubert_conv_ln x 6   the tile core as in vbx_hubert_conv; the fp32 sums (+ bias) of the workgroup's TT positions x C channels
//                            wait in the LDS beside the span, then LayerNorm over each position's channels, erf-GELU -> fp16
//                            -- or, where vbx_hubert_conv_ln_route says so (long rows at 512 channels), the pair vbx_hubert_conv_f32
//                            (the fp32 sums to memory, unrounded) + vbx_hubert_ln_gelu (one wave per position): the same bits, faster there
//   vbx_hubert_layernorm16, vbx_gemm (projection), vbx_hubert_posconv: as above -- and NO encoder.layer_norm here
//   per layer 1 .. output_layer (eight launches, as above):
//     vbx_hubert_layernorm   layer_norm(x) -> the fp16 operand only (x, the fp32 residual stream, is never normalised in place)
//     vbx_gemm q | k | v;  vbx_hubert_split_heads;  vbx_attn_fwd;  vbx_gemm out_proj + bias + x
//     vbx_hubert_layernorm   final_layer_norm(x) -> the fp16 operand only
//     vbx_gemm intermediate_dense (GELU);  vbx_gemm output_dense + bias + x
//   vbx_hubert_layernorm     encoder.layer_norm -> fp32, only where output_layer == num_hidden_layers
#include "seanet_tile.hpp"  // sn_tile_product, sn_pick_tile, sn_blocks_per_item, sn_launch

namespace {

constexpr int HB_CHUNK = 256;                          // positions per statistics record
constexpr int HB_MAX_K0 = 16, HB_MAX_S0 = 16, HB_MAX_C = 512;  // the first convolution's taps and stride, the extractor's channels
constexpr int HB_KM_ROWS = 4, HB_KM_MAX_D = 2048, HB_KM_MAX_K = 4096;

// ---------------------------------------------------------------------------------------------------- conv0 + GroupNorm
// The value both passes compute for (position t, channel c): acc = 0; acc = fmaf(w[c][tap], x[t * s0 + tap], acc) for tap = 0 .. k0 - 1.
// Workgroup (chunk, row): thread c walks the chunk's positions for channels c and c + 256.  A record is (K, S1, S2): K the chunk's first
// value, S1 = sum(v - K), S2 = sum((v - K)^2) -- shifted sums: a row with a large mean loses nothing to cancellation.
__global__ __launch_bounds__(256) void hubert_conv0_stats_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ rec,
                                                                 int T, int L0, int C, int k0, int s0, int chunks) {
  __shared__ float sw[HB_MAX_K0 * HB_MAX_C];                        // [tap][C]
  __shared__ float sx[(HB_CHUNK - 1) * HB_MAX_S0 + HB_MAX_K0];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
  const int t0 = chunk * HB_CHUNK;
  const int n = min(HB_CHUNK, L0 - t0);
  const int span = (n - 1) * s0 + k0;
  const float* xb = x + (long)b * T + (long)t0 * s0;  // the last tap read is (L0 - 1) * s0 + k0 - 1 <= T - 1
  for (int e = tid; e < span; e += 256) sx[e] = xb[e];
  for (int e = tid; e < k0 * C; e += 256) {
    const int tap = e / C, c = e - tap * C;
    sw[e] = w[c * k0 + tap];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float K = 0.f, S1 = 0.f, S2 = 0.f;
    for (int t = 0; t < n; t++) {
      float acc = 0.f;
      for (int tap = 0; tap < k0; tap++) acc = fmaf(sw[tap * C + c], sx[t * s0 + tap], acc);
      if (t == 0) K = acc;
      const float d = acc - K;
      S1 += d;
      S2 = fmaf(d, d, S2);
    }
    float* r = rec + (((long)b * chunks + chunk) * C + c) * 3;
    r[0] = K, r[1] = S1, r[2] = S2;
  }
}

// one thread per (row, channel): the chunk records in ascending order, in fp64 -> (mean, 1 / sqrt(biased variance + eps))
__global__ __launch_bounds__(256) void hubert_conv0_finalize_kernel(const float* __restrict__ rec, float* __restrict__ stats, int BC, int L0, int C,
                                                                    int chunks, float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= BC) return;
  const int b = i / C, c = i - b * C;
  const float* r = rec + ((long)b * chunks * C + c) * 3;
  double sum = 0.0;
  for (int ch = 0; ch < chunks; ch++) {
    const int n = min(HB_CHUNK, L0 - ch * HB_CHUNK);
    const float* q = r + (long)ch * C * 3;
    sum += (double)n * (double)q[0] + (double)q[1];
  }
  const double mean = sum / (double)L0;
  double m2 = 0.0;
  for (int ch = 0; ch < chunks; ch++) {
    const int n = min(HB_CHUNK, L0 - ch * HB_CHUNK);
    const float* q = r + (long)ch * C * 3;
    const double s1 = (double)q[1], mc = (double)q[0] + s1 / (double)n, dm = mc - mean;
    m2 += ((double)q[2] - s1 * s1 / (double)n) + (double)n * dm * dm;  // Chan et al.: M2 = sum M2_i + sum n_i (mean_i - mean)^2
  }
  const double var = m2 > 0.0 ? m2 / (double)L0 : 0.0;
  stats[2 * (long)i] = (float)mean;
  stats[2 * (long)i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// one thread per (position, eight channels): the fmaf chain again (the pre-norm tensor is never stored), normalise, affine, GELU, fp16
__global__ __launch_bounds__(256) void hubert_conv0_apply_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ stats,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, u16* __restrict__ y,
                                                                 int T, int L0, int C, int k0, int s0) {
  __shared__ float sw[HB_MAX_K0 * HB_MAX_C];
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k0 * C; e += 256) {
    const int tap = e / C, c = e - tap * C;
    sw[e] = w[c * k0 + tap];
  }
  __syncthreads();
  const int groups = C >> 3;
  const long e = (long)blockIdx.x * 256 + tid;
  if (e >= (long)L0 * groups) return;
  const int pos = (int)(e / groups), c0 = (int)(e - (long)pos * groups) * 8;
  const float* xb = x + (long)b * T + (long)pos * s0;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
  for (int tap = 0; tap < k0; tap++) {
    const float xv = xb[tap];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(sw[tap * C + c0 + j], xv, acc[j]);
  }
  const float* st = stats + 2 * ((long)b * C + c0);
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = gelu_erf_libm(fmaf((acc[j] - st[2 * j]) * st[2 * j + 1], gamma[c0 + j], beta[c0 + j]));
  *reinterpret_cast<uint4*>(y + ((long)b * L0 + pos) * C + c0) =
      make_uint4(pack_f16x2(acc[0], acc[1]), pack_f16x2(acc[2], acc[3]), pack_f16x2(acc[4], acc[5]), pack_f16x2(acc[6], acc[7]));
}

// ---------------------------------------------------------------------------------------------------- the strided convolutions
struct HbConv {
  const u16* x;  // [B, L, C]
  const u16* w;  // [C, k * C], column tap * C + c
  u16* y;        // [B, Lout, C]
  int L, Lout, C, k, TT;
};

// A workgroup owns TT consecutive output positions of one batch row and all C channels: it stages positions 2 t0 .. 2 (t0 + TT - 1) + k - 1
// (zeros past the row: only outputs past Lout read them, and those are not stored) and runs the product on the span in place.
template <int MG>
__global__ __launch_bounds__(256) void hubert_conv_kernel(HbConv p) {
  extern __shared__ __attribute__((aligned(16))) u16 hb_lds[];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH, c8 = p.C >> 3;
  const int span = (p.TT - 1) * 2 + p.k;
  const u16* xb = p.x + (long)b * p.L * p.C;
  for (int e = tid; e < span * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = t0 * 2 + pos;
    *reinterpret_cast<uint4*>(hb_lds + pos * ld + c) = i < p.L ? *reinterpret_cast<const uint4*>(xb + (long)i * p.C + c) : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.C, c = kk - tap * p.C;
    base = hb_lds + tap * ld + c, ldr = 2 * ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t < p.Lout) p.y[((long)b * p.Lout + t) * p.C + n] = f32_to_f16(gelu_erf_libm(v));
    };
  };
  sn_tile_product<MG, true>(p.w, p.C, p.k * p.C, p.TT >> 4, rows, store);  // k 3 at C = 16 (mod 32): K = 48 has a tail
}

size_t hb_conv_lds(int TT, int C, int k) { return (size_t)((TT - 1) * 2 + k) * (C + SN_PADH) * sizeof(u16); }
int hb_conv_tile(int C, int k) {
  return sn_pick_tile([&](int TT) { return hb_conv_lds(TT, C, k); });
}
int hb_conv_check(int C, int k) {
  VBX_REQUIRE(C >= 16 && C % 16 == 0 && C <= HB_MAX_C, "vbx_hubert_conv: channels must be a multiple of 16 up to %d (got %d)", HB_MAX_C, C);
  VBX_REQUIRE(k == 2 || k == 3, "vbx_hubert_conv: kernel_size must be 2 or 3 (got %d)", k);
  return 0;
}

// ---------------------------------------------------------------------------------------------------- LayerNorm
// one wave per row: mean, then the sum of squared deviations, then the affine; fp32 throughout.  IN16: the row is fp16.
template <bool IN16>
__global__ __launch_bounds__(256) void hubert_layernorm_kernel(const void* __restrict__ xv, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ y32, u16* __restrict__ y16, long M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* x32 = reinterpret_cast<const float*>(xv) + row * D;
  const u16* x16 = reinterpret_cast<const u16*>(xv) + row * D;
  auto at = [&](int i) __attribute__((always_inline)) { return IN16 ? f16_to_f32(x16[i]) : x32[i]; };
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += at(i);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int i = lane; i < D; i += 64) {
    const float d = at(i) - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  for (int i = lane; i < D; i += 64) {
    const float v = fmaf((at(i) - mean) * rstd, gamma[i], beta[i]);
    if (y32) y32[row * D + i] = v;
    if (y16) y16[row * D + i] = f32_to_f16_sat(v);
  }
}

// ---------------------------------------------------------------------------------------------------- the positional convolution
struct HbPos {
  const float* x;     // [B, N, D] fp32: rounded to fp16 as it is staged, and the residual added in the epilogue
  const u16* w;       // [D, k * Dg], row = output channel, column tap * Dg + ci (weight norm folded)
  const float* bias;  // [D]
  float* y;           // [B, N, D] = gelu(conv + bias) + x
  int N, D, Dg, G, k, TT;
};

// Workgroup (tile, group, row): out[t][o] = sum_{tap, ci} w[o][tap * Dg + ci] x[t + tap - k / 2][g * Dg + ci] for t0 <= t < t0 + TT, the
// Dg output channels of group g.  Positions t0 - k / 2 .. t0 + TT - 1 + k / 2 - 1 of the group's channels sit in the LDS, zeros outside
// [0, N): Conv1d(padding = k / 2) computes N + 1 positions of which the module drops the last -- position N is simply never asked for.
template <int MG>
__global__ __launch_bounds__(256) void hubert_posconv_kernel(HbPos p) {
  extern __shared__ __attribute__((aligned(16))) u16 hb_lds[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int g = blockIdx.x % p.G, t0 = (blockIdx.x / p.G) * p.TT;
  const int ld = p.Dg + SN_PADH, c8 = p.Dg >> 3;
  const int span = p.TT - 1 + p.k, pad = p.k >> 1;
  const float* xb = p.x + (long)b * p.N * p.D + g * p.Dg;
  for (int e = tid; e < span * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = t0 - pad + pos;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i >= 0 && i < p.N) {
      const float4 lo = *reinterpret_cast<const float4*>(xb + (long)i * p.D + c), hi = *reinterpret_cast<const float4*>(xb + (long)i * p.D + c + 4);
      v = make_uint4(pack_f16x2_sat(lo.x, lo.y), pack_f16x2_sat(lo.z, lo.w), pack_f16x2_sat(hi.x, hi.y), pack_f16x2_sat(hi.z, hi.w));
    }
    *reinterpret_cast<uint4*>(hb_lds + pos * ld + c) = v;
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.Dg, c = kk - tap * p.Dg;
    base = hb_lds + tap * ld + c, ldr = ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias[g * p.Dg + n]](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t >= p.N) return;
      const long o = ((long)b * p.N + t) * p.D + g * p.Dg + n;
      p.y[o] = gelu_erf_libm(v + bv) + p.x[o];
    };
  };
  sn_tile_product<MG, true>(p.w + (long)g * p.Dg * p.k * p.Dg, p.Dg, p.k * p.Dg, p.TT >> 4, rows, store);
}

size_t hb_pos_lds(int TT, int Dg, int k) { return (size_t)(TT - 1 + k) * (Dg + SN_PADH) * sizeof(u16); }
int hb_pos_tile(int Dg, int k) {
  return sn_pick_tile([&](int TT) { return hb_pos_lds(TT, Dg, k); });
}
int hb_pos_check(int Dg, int k) {
  VBX_REQUIRE(Dg >= 8 && Dg % 8 == 0, "vbx_hubert_posconv: channels per group must be a multiple of 8 (got %d)", Dg);
  VBX_REQUIRE(k >= 2 && k % 2 == 0 && k <= 256, "vbx_hubert_posconv: kernel_size must be even, 2 .. 256 (got %d)", k);
  return 0;
}

// ---------------------------------------------------------------------------------------------------- head split
// qkv fp32 [M, 3D] (M = B * N; columns [q | k | v], each H heads of 64) -> fp16 [B, H, N, 64]; one thread per eight elements
__global__ __launch_bounds__(256) void hubert_split_heads_kernel(const float* __restrict__ qkv, u16* __restrict__ q16, u16* __restrict__ k16,
                                                                 u16* __restrict__ v16, long M, int N, int H, float q_prescale) {
  const int D = H * 64, per_row = 3 * D / 8;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * per_row) return;
  const long row = e / per_row;
  const int col = (int)(e - row * per_row) * 8;
  const int which = col / D, h = (col - which * D) >> 6, d = col & 63;
  const long bi = row / N, n = row - bi * N;
  const float4 lo = *reinterpret_cast<const float4*>(qkv + row * 3 * D + col), hi = *reinterpret_cast<const float4*>(qkv + row * 3 * D + col + 4);
  const float s = which == 0 ? q_prescale : 1.0f;
  u16* dst = (which == 0 ? q16 : (which == 1 ? k16 : v16)) + ((bi * H + h) * N + n) * 64 + d;
  *reinterpret_cast<uint4*>(dst) = make_uint4(pack_f16x2_sat(lo.x * s, lo.y * s), pack_f16x2_sat(lo.z * s, lo.w * s),
                                              pack_f16x2_sat(hi.x * s, hi.y * s), pack_f16x2_sat(hi.z * s, hi.w * s));
}

// ---------------------------------------------------------------------------------------------------- k-means
// A workgroup holds HB_KM_ROWS feature rows in the LDS; wave w walks codes w, w + 4, ...: d = sum_i (h_i - c_i)^2 with lane l summing
// i = 4 l + 256 j in ascending j, then the xor tree over the lanes -- a fixed order per (row, code), whatever the batch.  The first
// strictly smaller distance wins inside a wave (ascending codes); across the four waves the smaller distance, then the lower index.
__global__ __launch_bounds__(256) void hubert_kmeans_kernel(const float* __restrict__ h, const float* __restrict__ cent, long long* __restrict__ ids,
                                                            long M, int D, int K) {
  __shared__ __attribute__((aligned(16))) float sh[HB_KM_ROWS * HB_KM_MAX_D];
  __shared__ float sd[4][HB_KM_ROWS];
  __shared__ int sk[4][HB_KM_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long r0 = (long)blockIdx.x * HB_KM_ROWS;
  const int nr = (int)min((long)HB_KM_ROWS, M - r0);
  for (int e = tid; e < HB_KM_ROWS * D; e += 256) {
    const int r = e / D;
    sh[e] = r < nr ? h[(r0 + r) * D + (e - r * D)] : 0.f;
  }
  __syncthreads();
  float best[HB_KM_ROWS];
  int bk[HB_KM_ROWS];
#pragma unroll
  for (int r = 0; r < HB_KM_ROWS; r++) best[r] = INFINITY, bk[r] = K;
  for (int k = wave; k < K; k += 4) {
    const float* c = cent + (long)k * D;
    float acc[HB_KM_ROWS];
#pragma unroll
    for (int r = 0; r < HB_KM_ROWS; r++) acc[r] = 0.f;
    for (int i = lane * 4; i < D; i += 256) {
      const float4 cv = *reinterpret_cast<const float4*>(c + i);
#pragma unroll
      for (int r = 0; r < HB_KM_ROWS; r++) {
        const float4 hv = *reinterpret_cast<const float4*>(sh + r * D + i);
        const float d0 = hv.x - cv.x, d1 = hv.y - cv.y, d2 = hv.z - cv.z, d3 = hv.w - cv.w;
        acc[r] = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, acc[r]))));
      }
    }
#pragma unroll
    for (int r = 0; r < HB_KM_ROWS; r++) {
      const float d = wave_sum(acc[r]);
      if (d < best[r] || bk[r] == K) best[r] = d, bk[r] = k;  // bk == K: nothing taken yet (a NaN distance still yields a valid index)
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < HB_KM_ROWS; r++) sd[wave][r] = best[r], sk[wave][r] = bk[r];
  }
  __syncthreads();
  if (tid < nr) {
    float d = sd[0][tid];
    int k = sk[0][tid];
    for (int w = 1; w < 4; w++) {
      const float dw = sd[w][tid];
      const int kw = sk[w][tid];
      if (kw < K && (k >= K || dw < d || (dw == d && kw < k))) d = dw, k = kw;
    }
    ids[r0 + tid] = (long long)k;
  }
}

// ---------------------------------------------------------------------------------------------------- ragged waves (include/vbx.h)
// Second kernels beside the plain ones above, which are not touched: the same arithmetic in the same order about the row's own
// length.  lens[b] is clamped here, so no value of the table can become an address.
VBX_DEV int hb_row_l0(const int* __restrict__ lens, int b, int T, int k0, int s0) {
  return (min(max(lens[b], k0), T) - k0) / s0 + 1;  // 1 .. L0
}

// hubert_conv0_stats_kernel over the first L0_b positions: the same 256-position chunks from position 0.  A chunk at or past L0_b
// leaves before it reads anything (its record is never read either); the last live chunk takes n = L0_b - t0.
__global__ __launch_bounds__(256) void hubert_conv0_stats_lens_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                                      const float* __restrict__ w, float* __restrict__ rec, int T, int C, int k0,
                                                                      int s0, int chunks) {
  __shared__ float sw[HB_MAX_K0 * HB_MAX_C];                        // [tap][C]
  __shared__ float sx[(HB_CHUNK - 1) * HB_MAX_S0 + HB_MAX_K0];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
  const int L0 = hb_row_l0(lens, b, T, k0, s0);
  const int t0 = chunk * HB_CHUNK;
  if (t0 >= L0) return;  // uniform over the workgroup
  const int n = min(HB_CHUNK, L0 - t0);
  const int span = (n - 1) * s0 + k0;
  const float* xb = x + (long)b * T + (long)t0 * s0;  // the last tap read is (L0_b - 1) * s0 + k0 - 1 <= lens[b] - 1
  for (int e = tid; e < span; e += 256) sx[e] = xb[e];
  for (int e = tid; e < k0 * C; e += 256) {
    const int tap = e / C, c = e - tap * C;
    sw[e] = w[c * k0 + tap];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float K = 0.f, S1 = 0.f, S2 = 0.f;
    for (int t = 0; t < n; t++) {
      float acc = 0.f;
      for (int tap = 0; tap < k0; tap++) acc = fmaf(sw[tap * C + c], sx[t * s0 + tap], acc);
      if (t == 0) K = acc;
      const float d = acc - K;
      S1 += d;
      S2 = fmaf(d, d, S2);
    }
    float* r = rec + (((long)b * chunks + chunk) * C + c) * 3;
    r[0] = K, r[1] = S1, r[2] = S2;
  }
}

// hubert_conv0_finalize_kernel over the row's live chunks only, divided by L0_b; `chunks` is the pitch of the records
__global__ __launch_bounds__(256) void hubert_conv0_finalize_lens_kernel(const float* __restrict__ rec, const int* __restrict__ lens,
                                                                         float* __restrict__ stats, int BC, int T, int C, int k0, int s0, int chunks,
                                                                         float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= BC) return;
  const int b = i / C, c = i - b * C;
  const int L0 = hb_row_l0(lens, b, T, k0, s0);
  const int live = (L0 + HB_CHUNK - 1) / HB_CHUNK;  // <= chunks
  const float* r = rec + ((long)b * chunks * C + c) * 3;
  double sum = 0.0;
  for (int ch = 0; ch < live; ch++) {
    const int n = min(HB_CHUNK, L0 - ch * HB_CHUNK);
    const float* q = r + (long)ch * C * 3;
    sum += (double)n * (double)q[0] + (double)q[1];
  }
  const double mean = sum / (double)L0;
  double m2 = 0.0;
  for (int ch = 0; ch < live; ch++) {
    const int n = min(HB_CHUNK, L0 - ch * HB_CHUNK);
    const float* q = r + (long)ch * C * 3;
    const double s1 = (double)q[1], mc = (double)q[0] + s1 / (double)n, dm = mc - mean;
    m2 += ((double)q[2] - s1 * s1 / (double)n) + (double)n * dm * dm;
  }
  const double var = m2 > 0.0 ? m2 / (double)L0 : 0.0;
  stats[2 * (long)i] = (float)mean;
  stats[2 * (long)i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// hubert_conv0_apply_kernel; a position at or past L0_b stores fp16 zeros and reads neither the wave nor the statistics
__global__ __launch_bounds__(256) void hubert_conv0_apply_lens_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                                      const float* __restrict__ w, const float* __restrict__ stats,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      u16* __restrict__ y, int T, int L0, int C, int k0, int s0) {
  __shared__ float sw[HB_MAX_K0 * HB_MAX_C];
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k0 * C; e += 256) {
    const int tap = e / C, c = e - tap * C;
    sw[e] = w[c * k0 + tap];
  }
  __syncthreads();
  const int groups = C >> 3;
  const long e = (long)blockIdx.x * 256 + tid;
  if (e >= (long)L0 * groups) return;
  const int pos = (int)(e / groups), c0 = (int)(e - (long)pos * groups) * 8;
  u16* yo = y + ((long)b * L0 + pos) * C + c0;
  if (pos >= hb_row_l0(lens, b, T, k0, s0)) {
    *reinterpret_cast<uint4*>(yo) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const float* xb = x + (long)b * T + (long)pos * s0;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
  for (int tap = 0; tap < k0; tap++) {
    const float xv = xb[tap];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(sw[tap * C + c0 + j], xv, acc[j]);
  }
  const float* st = stats + 2 * ((long)b * C + c0);
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = gelu_erf_libm(fmaf((acc[j] - st[2 * j]) * st[2 * j + 1], gamma[c0 + j], beta[c0 + j]));
  *reinterpret_cast<uint4*>(yo) =
      make_uint4(pack_f16x2(acc[0], acc[1]), pack_f16x2(acc[2], acc[3]), pack_f16x2(acc[4], acc[5]), pack_f16x2(acc[6], acc[7]));
}

// hubert_posconv_kernel with the row's own frame count N_b = lens[b] (clamped into 1 .. N): positions >= N_b are staged as zeros, as
// Conv1d(padding = k / 2) of the row alone sees them, whatever x holds there; output rows N_b .. N - 1 are stored as 0.0 without a
// product, and a tile wholly past N_b stages nothing.
struct HbPosLens : HbPos {
  const int* lens;  // [B] frames
};
template <int MG>
__global__ __launch_bounds__(256) void hubert_posconv_lens_kernel(HbPosLens p) {
  extern __shared__ __attribute__((aligned(16))) u16 hb_lds[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int g = blockIdx.x % p.G, t0 = (blockIdx.x / p.G) * p.TT;
  const int Nb = min(max(p.lens[b], 1), p.N);
  if (t0 >= Nb) {  // uniform over the workgroup
    const int rows = min(p.TT, p.N - t0), c4 = p.Dg >> 2;
    for (int e = tid; e < rows * c4; e += 256) {
      const int r = e / c4, c = (e - r * c4) * 4;
      *reinterpret_cast<float4*>(p.y + ((long)b * p.N + t0 + r) * p.D + g * p.Dg + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int ld = p.Dg + SN_PADH, c8 = p.Dg >> 3;
  const int span = p.TT - 1 + p.k, pad = p.k >> 1;
  const float* xb = p.x + (long)b * p.N * p.D + g * p.Dg;
  for (int e = tid; e < span * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = t0 - pad + pos;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i >= 0 && i < Nb) {
      const float4 lo = *reinterpret_cast<const float4*>(xb + (long)i * p.D + c), hi = *reinterpret_cast<const float4*>(xb + (long)i * p.D + c + 4);
      v = make_uint4(pack_f16x2_sat(lo.x, lo.y), pack_f16x2_sat(lo.z, lo.w), pack_f16x2_sat(hi.x, hi.y), pack_f16x2_sat(hi.z, hi.w));
    }
    *reinterpret_cast<uint4*>(hb_lds + pos * ld + c) = v;
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.Dg, c = kk - tap * p.Dg;
    base = hb_lds + tap * ld + c, ldr = ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias[g * p.Dg + n]](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t >= p.N) return;
      const long o = ((long)b * p.N + t) * p.D + g * p.Dg + n;
      if (t >= Nb) {
        p.y[o] = 0.f;
        return;
      }
      p.y[o] = gelu_erf_libm(v + bv) + p.x[o];
    };
  };
  sn_tile_product<MG, true>(p.w + (long)g * p.Dg * p.k * p.Dg, p.Dg, p.k * p.Dg, p.TT >> 4, rows, store);
}

// ---------------------------------------------------------------------------------------------------- the large form (include/vbx.h)
// conv0 + bias + LayerNorm over the channels + GELU.  Workgroup (tile of HB_LN0_POS positions, row): the tile's samples and the
// weights sit in the LDS; a wave owns a position at a time, lane l its channels 8 l .. 8 l + 7 (lanes at or past C / 8 hold nothing and
// add zeros to the two wave sums).  Nothing runs over time: a position reads only its own k0 samples.
constexpr int HB_LN0_POS = 64;
__global__ __launch_bounds__(256) void hubert_conv0_ln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, u16* __restrict__ y,
                                                              int T, int L0, int C, int k0, int s0, float eps) {
  __shared__ __attribute__((aligned(16))) float sw[HB_MAX_K0 * HB_MAX_C];  // [tap][C]
  __shared__ float sx[(HB_LN0_POS - 1) * HB_MAX_S0 + HB_MAX_K0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  const int t0 = blockIdx.x * HB_LN0_POS;
  const int n = min(HB_LN0_POS, L0 - t0);
  const int span = (n - 1) * s0 + k0;
  const float* xb = x + (long)b * T + (long)t0 * s0;  // the last tap read is (L0 - 1) * s0 + k0 - 1 <= T - 1
  for (int e = tid; e < span; e += 256) sx[e] = xb[e];
  for (int e = tid; e < k0 * C; e += 256) {
    const int tap = e / C, c = e - tap * C;
    sw[e] = w[c * k0 + tap];
  }
  __syncthreads();
  const int c0 = lane * 8;
  const bool has = c0 < C;
  float bv[8], gm[8], bt[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    bv[j] = (has && bias) ? bias[c0 + j] : 0.f;
    gm[j] = has ? gamma[c0 + j] : 0.f;
    bt[j] = has ? beta[c0 + j] : 0.f;
  }
  const float invC = 1.0f / (float)C;
  for (int t = wave; t < n; t += 4) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = 0.f;
    if (has) {
      for (int tap = 0; tap < k0; tap++) {
        const float xv = sx[t * s0 + tap];
        const float4 lo = *reinterpret_cast<const float4*>(sw + tap * C + c0), hi = *reinterpret_cast<const float4*>(sw + tap * C + c0 + 4);
        acc[0] = fmaf(lo.x, xv, acc[0]), acc[1] = fmaf(lo.y, xv, acc[1]), acc[2] = fmaf(lo.z, xv, acc[2]), acc[3] = fmaf(lo.w, xv, acc[3]);
        acc[4] = fmaf(hi.x, xv, acc[4]), acc[5] = fmaf(hi.y, xv, acc[5]), acc[6] = fmaf(hi.z, xv, acc[6]), acc[7] = fmaf(hi.w, xv, acc[7]);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      acc[j] += bv[j];
      s += acc[j];
    }
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
    if (has) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = acc[j] - mean;
        q = fmaf(d, d, q);
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * invC + eps);
    if (has) {
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = gelu_erf_libm(fmaf((acc[j] - mean) * rstd, gm[j], bt[j]));
      *reinterpret_cast<uint4*>(y + ((long)b * L0 + t0 + t) * C + c0) =
          make_uint4(pack_f16x2(acc[0], acc[1]), pack_f16x2(acc[2], acc[3]), pack_f16x2(acc[4], acc[5]), pack_f16x2(acc[6], acc[7]));
    }
  }
}

// LayerNorm over the C <= 512 channels of one position + affine + erf-GELU, by one wave: lane l holds channels 8 l .. 8 l + 7 (lanes at
// or past C / 8 hold nothing and add zeros), sums them in ascending order, then the xor tree; two passes (the mean, then the squared
// deviations), fp32; one 16-byte fp16 store per lane.  src: the fp32 pre-norm values of the position (LDS or memory), 16-byte aligned.
VBX_DEV void hb_row_ln_gelu(const float* src, const float* __restrict__ gamma, const float* __restrict__ beta, u16* __restrict__ dst, int C, float eps,
                            int lane) {
  const int c0 = lane * 8;
  const bool has = c0 < C;
  const float invC = 1.0f / (float)C;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = 0.f;
  if (has) {
    const float4 lo = *reinterpret_cast<const float4*>(src + c0), hi = *reinterpret_cast<const float4*>(src + c0 + 4);
    v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; j++) sum += v[j];
  const float mean = wave_sum(sum) * invC;
  float q = 0.f;
  if (has) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float d = v[j] - mean;
      q = fmaf(d, d, q);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * invC + eps);
  if (has) {
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = gelu_erf_libm(fmaf((v[j] - mean) * rstd, gamma[c0 + j], beta[c0 + j]));
    *reinterpret_cast<uint4*>(dst + c0) = make_uint4(pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3]), pack_f16x2(v[4], v[5]), pack_f16x2(v[6], v[7]));
  }
}

// hubert_conv_kernel with the large form's epilogue.  The workgroup owns all C channels of its TT positions, so a position's LayerNorm
// needs no other workgroup: the tile core hands every fp32 sum (+ bias) to an fp32 tile [TT][C + 4] in the LDS BESIDE the span (other
// waves still read the span while one stores), and after one barrier a wave normalises a position at a time from those unrounded sums.
struct HbConvLn : HbConv {
  const float* bias;   // [C] or null
  const float* gamma;  // [C]
  const float* beta;   // [C]
  float eps;
};
constexpr int HB_PADF = 4;  // fp32 elements of padding per row of the sum tile: the four row groups of an MFMA result land 16 banks apart

template <int MG>
__global__ __launch_bounds__(256) void hubert_conv_ln_kernel(HbConvLn p) {
  extern __shared__ __attribute__((aligned(16))) u16 hb_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, t0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH, c8 = p.C >> 3, ldf = p.C + HB_PADF;
  const int span = (p.TT - 1) * 2 + p.k;
  float* sums = reinterpret_cast<float*>(hb_lds + span * ld);  // span * ld * 2 bytes is a multiple of 16
  const u16* xb = p.x + (long)b * p.L * p.C;
  for (int e = tid; e < span * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = t0 * 2 + pos;
    *reinterpret_cast<uint4*>(hb_lds + pos * ld + c) = i < p.L ? *reinterpret_cast<const uint4*>(xb + (long)i * p.C + c) : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.C, c = kk - tap * p.C;
    base = hb_lds + tap * ld + c, ldr = 2 * ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias ? p.bias[n] : 0.f](int m, float v) __attribute__((always_inline)) { sums[m * ldf + n] = v + bv; };
  };
  sn_tile_product<MG, true>(p.w, p.C, p.k * p.C, p.TT >> 4, rows, store);
  __syncthreads();
  const int live = min(p.TT, p.Lout - t0);
  for (int m = wave; m < live; m += 4)
    hb_row_ln_gelu(sums + m * ldf, p.gamma, p.beta, p.y + ((long)b * p.Lout + t0 + m) * p.C, p.C, p.eps, lane);
}

// The same convolution as an fp32 intermediate plus a row kernel, for the shapes where the fused kernel's smaller tile costs more than
// the round trip through memory (vbx_hubert_conv_ln_route): hubert_conv_kernel's tile, the fp32 sum (+ bias) stored UNROUNDED to
// s fp32 [B, Lout, C]; then one wave per position runs hb_row_ln_gelu on it -- the same code on the same values: the same bits.
struct HbConvF32 : HbConv {
  const float* bias;  // [C] or null
  float* s;           // [B, Lout, C]
};
template <int MG>
__global__ __launch_bounds__(256) void hubert_conv_f32_kernel(HbConvF32 p) {
  extern __shared__ __attribute__((aligned(16))) u16 hb_lds[];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH, c8 = p.C >> 3;
  const int span = (p.TT - 1) * 2 + p.k;
  const u16* xb = p.x + (long)b * p.L * p.C;
  for (int e = tid; e < span * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = t0 * 2 + pos;
    *reinterpret_cast<uint4*>(hb_lds + pos * ld + c) = i < p.L ? *reinterpret_cast<const uint4*>(xb + (long)i * p.C + c) : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.C, c = kk - tap * p.C;
    base = hb_lds + tap * ld + c, ldr = 2 * ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias ? p.bias[n] : 0.f](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t < p.Lout) p.s[((long)b * p.Lout + t) * p.C + n] = v + bv;
    };
  };
  sn_tile_product<MG, true>(p.w, p.C, p.k * p.C, p.TT >> 4, rows, store);
}

__global__ __launch_bounds__(256) void hubert_ln_gelu_kernel(const float* __restrict__ s, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             u16* __restrict__ y, long M, int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // uniform over the wave
  hb_row_ln_gelu(s + row * C, gamma, beta, y + row * C, C, eps, threadIdx.x & 63);
}

size_t hb_conv_ln_lds(int TT, int C, int k) { return hb_conv_lds(TT, C, k) + (size_t)TT * (C + HB_PADF) * sizeof(float); }
// A 32-position tile in the whole LDS (133 KiB at C = 512, one workgroup per CU) was measured against this pick's 16: 1.94 ms against
// 2.02 ms at 8 x 15 999 positions, 0.067 against 0.051 ms at 8 x 499 -- no gain.
int hb_conv_ln_tile(int C, int k) {
  return sn_pick_tile([&](int TT) { return hb_conv_ln_lds(TT, C, k); });
}

// ---------------------------------------------------------------------------------------------------- wave normalisation
// (x - mean) / sqrt(var + eps) per row, biased variance.  Workgroup (chunk of HB_WN_CHUNK samples, row): one record (K, S1, S2) with K
// the chunk's first sample, S1 = sum(x - K), S2 = sum((x - K)^2) -- thread t sums samples t, t + 256, ... in ascending order, then the
// xor tree of the wave and the four waves in order.  A second launch combines a row's records in ascending order in fp64 (as
// hubert_conv0_finalize_kernel) into (mean, 1 / sqrt(var + eps)), kept in fp64; a third applies them in fp64 and rounds once to fp32.
constexpr int HB_WN_CHUNK = 4096;
VBX_DEV int hb_wn_len(const int* __restrict__ lens, int b, int T) { return lens ? min(max(lens[b], 1), T) : T; }

__global__ __launch_bounds__(256) void wave_normalize_stats_kernel(const float* __restrict__ x, const int* __restrict__ lens, float* __restrict__ rec,
                                                                   int T, int chunks) {
  __shared__ float red[8];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
  const int Tb = hb_wn_len(lens, b, T);
  const long t0 = (long)chunk * HB_WN_CHUNK;
  if (t0 >= Tb) return;  // uniform over the workgroup; the record is never read
  const int n = (int)min((long)HB_WN_CHUNK, Tb - t0);
  const float* xb = x + (long)b * T + t0;
  const float K = xb[0];
  float S1 = 0.f, S2 = 0.f;
  for (int e = tid; e < n; e += 256) {
    const float d = xb[e] - K;
    S1 += d;
    S2 = fmaf(d, d, S2);
  }
  S1 = wave_sum(S1), S2 = wave_sum(S2);
  if ((tid & 63) == 0) red[(tid >> 6) * 2] = S1, red[(tid >> 6) * 2 + 1] = S2;
  __syncthreads();
  if (tid == 0) {
    float* r = rec + ((long)b * chunks + chunk) * 3;
    r[0] = K, r[1] = ((red[0] + red[2]) + red[4]) + red[6], r[2] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// one thread per row
__global__ __launch_bounds__(64) void wave_normalize_finalize_kernel(const float* __restrict__ rec, const int* __restrict__ lens,
                                                                     double* __restrict__ stats, int B, int T, int chunks, float eps) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int Tb = hb_wn_len(lens, b, T);
  const int live = (Tb + HB_WN_CHUNK - 1) / HB_WN_CHUNK;  // <= chunks
  const float* r = rec + (long)b * chunks * 3;
  double sum = 0.0;
  for (int ch = 0; ch < live; ch++) {
    const int n = min(HB_WN_CHUNK, Tb - ch * HB_WN_CHUNK);
    sum += (double)n * (double)r[3 * (long)ch] + (double)r[3 * (long)ch + 1];
  }
  const double mean = sum / (double)Tb;
  double m2 = 0.0;
  for (int ch = 0; ch < live; ch++) {
    const int n = min(HB_WN_CHUNK, Tb - ch * HB_WN_CHUNK);
    const float* q = r + 3 * (long)ch;
    const double s1 = (double)q[1], mc = (double)q[0] + s1 / (double)n, dm = mc - mean;
    m2 += ((double)q[2] - s1 * s1 / (double)n) + (double)n * dm * dm;
  }
  const double var = m2 > 0.0 ? m2 / (double)Tb : 0.0;
  stats[2 * (long)b] = mean;
  stats[2 * (long)b + 1] = 1.0 / sqrt(var + (double)eps);
}

// one thread per four samples; a sample at or past the row's length is written as 0 and not read
__global__ __launch_bounds__(256) void wave_normalize_apply_kernel(const float* x, const int* __restrict__ lens,
                                                                   const double* __restrict__ stats, float* y, int T) {
  const int b = blockIdx.y;
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= T) return;
  const int Tb = hb_wn_len(lens, b, T);
  const double mean = stats[2 * (long)b], rstd = stats[2 * (long)b + 1];
  const int n = (int)min(4L, T - e0);
  for (int j = 0; j < n; j++) {
    const long o = (long)b * T + e0 + j;
    y[o] = e0 + j < Tb ? (float)(((double)x[o] - mean) * rstd) : 0.f;
  }
}

}  // namespace

extern "C" int vbx_hubert_conv0_chunks(int L0) { return L0 >= 1 ? cdiv(L0, HB_CHUNK) : 0; }

static int hb_conv0_check(const char* who, int B, long T, int C, int k0, int s0, long* L0) {
  VBX_REQUIRE(B >= 1 && B <= 65535, "%s: need B in 1 .. 65535", who);
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= HB_MAX_C, "%s: channels must be a multiple of 8 up to %d (got %d)", who, HB_MAX_C, C);
  VBX_REQUIRE(k0 >= 1 && k0 <= HB_MAX_K0 && s0 >= 1 && s0 <= HB_MAX_S0, "%s: kernel_size in 1 .. %d and stride in 1 .. %d (got %d, %d)", who,
              HB_MAX_K0, HB_MAX_S0, k0, s0);
  VBX_REQUIRE(T >= k0 && T < (1L << 31), "%s: the wave is shorter than one kernel, or too long", who);
  *L0 = (T - k0) / s0 + 1;
  return 0;
}

extern "C" int vbx_hubert_conv0_stats(const float* wave, const float* w, float* records, float* stats, int B, long T, int C, int k0, int s0,
                                      float eps, void* stream) {
  VBX_REQUIRE(wave && w && records && stats, "vbx_hubert_conv0_stats: null operand");
  long L0;
  if (int rc = hb_conv0_check("vbx_hubert_conv0_stats", B, T, C, k0, s0, &L0)) return rc;
  const int chunks = cdiv(L0, HB_CHUNK);
  hipLaunchKernelGGL(hubert_conv0_stats_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, wave, w, records, (int)T, (int)L0, C, k0, s0, chunks);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(hubert_conv0_finalize_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, records, stats, B * C, (int)L0, C,
                     chunks, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_conv0_apply(const float* wave, const float* w, const float* stats, const float* gamma, const float* beta, void* y_f16,
                                      int B, long T, int C, int k0, int s0, void* stream) {
  VBX_REQUIRE(wave && w && stats && gamma && beta && y_f16, "vbx_hubert_conv0_apply: null operand");
  long L0;
  if (int rc = hb_conv0_check("vbx_hubert_conv0_apply", B, T, C, k0, s0, &L0)) return rc;
  hipLaunchKernelGGL(hubert_conv0_apply_kernel, dim3(cdiv(L0 * (C / 8), 256), B), dim3(256), 0, (hipStream_t)stream, wave, w, stats, gamma, beta,
                     (u16*)y_f16, (int)T, (int)L0, C, k0, s0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_conv_tile(int C, int k) {
  if (int rc = hb_conv_check(C, k)) return rc;
  return hb_conv_tile(C, k);  // never 0: 16 positions of 512 channels at k 3 take 34 KiB
}

extern "C" int vbx_hubert_conv(const void* x_f16, const void* w_f16, void* y_f16, int B, int L, int C, int k, void* stream) {
  VBX_REQUIRE(x_f16 && w_f16 && y_f16, "vbx_hubert_conv: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= k && L < (1 << 30), "vbx_hubert_conv: need B in 1 .. 65535 and kernel_size <= L < 2^30");
  if (int rc = hb_conv_check(C, k)) return rc;
  HbConv p;
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.y = (u16*)y_f16, p.L = L, p.Lout = (L - k) / 2 + 1, p.C = C, p.k = k;
  int TT = hb_conv_tile(C, k);
  while (TT > 16 && TT / 2 >= p.Lout) TT >>= 1;  // a short row: no tile of absent positions is staged or multiplied
  p.TT = TT;
  const size_t bytes = hb_conv_lds(TT, C, k);
  const int MG = sn_blocks_per_item(C / 16, TT / 16), blocks = cdiv(p.Lout, TT);
  if (MG == 4) return sn_launch<hubert_conv_kernel<4>>("vbx_hubert_conv", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hubert_conv_kernel<2>>("vbx_hubert_conv", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hubert_conv_kernel<1>>("vbx_hubert_conv", p, blocks, B, bytes, (hipStream_t)stream);
}

static int hb_ln_check(const char* who, const void* x, const float* g, const float* b, long M, int D) {
  VBX_REQUIRE(x && g && b, "%s: null operand", who);
  VBX_REQUIRE(M >= 1 && M < (1L << 31) && D >= 1 && D <= 8192, "%s: need rows >= 1 and D in 1 .. 8192", who);
  return 0;
}

extern "C" int vbx_hubert_layernorm(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_f16, long M, int D, float eps,
                                    void* stream) {
  if (int rc = hb_ln_check("vbx_hubert_layernorm", x, gamma, beta, M, D)) return rc;
  VBX_REQUIRE(y_f32 || y_f16, "vbx_hubert_layernorm: no output");
  hipLaunchKernelGGL(hubert_layernorm_kernel<false>, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, (const void*)x, gamma, beta, y_f32,
                     (u16*)y_f16, M, D, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_layernorm16(const void* x_f16, const float* gamma, const float* beta, void* y_f16, long M, int D, float eps, void* stream) {
  if (int rc = hb_ln_check("vbx_hubert_layernorm16", x_f16, gamma, beta, M, D)) return rc;
  VBX_REQUIRE(y_f16, "vbx_hubert_layernorm16: no output");
  hipLaunchKernelGGL(hubert_layernorm_kernel<true>, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x_f16, gamma, beta, (float*)nullptr,
                     (u16*)y_f16, M, D, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_posconv_tile(int Dg, int k) {
  if (int rc = hb_pos_check(Dg, k)) return rc;
  const int TT = hb_pos_tile(Dg, k);
  if (!TT) {
    vbx_set_error("vbx_hubert_posconv: 16 output positions of this convolution do not fit the LDS");
    return VBX_EINVAL;
  }
  return TT;
}

extern "C" int vbx_hubert_posconv(const float* x, const void* w_f16, const float* bias, float* y, int B, int N, int D, int groups, int k,
                                  void* stream) {
  VBX_REQUIRE(x && w_f16 && bias && y && x != y, "vbx_hubert_posconv: null operand, or y aliases x");
  VBX_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N < (1 << 24), "vbx_hubert_posconv: need B in 1 .. 65535 and N in 1 .. 2^24");
  VBX_REQUIRE(groups >= 1 && D >= groups && D % groups == 0, "vbx_hubert_posconv: groups must divide D");
  const int Dg = D / groups;
  if (int rc = hb_pos_check(Dg, k)) return rc;
  int TT = hb_pos_tile(Dg, k);
  VBX_REQUIRE(TT > 0, "vbx_hubert_posconv: 16 output positions of this convolution do not fit the LDS");
  while (TT > 16 && TT / 2 >= N) TT >>= 1;
  HbPos p;
  p.x = x, p.w = (const u16*)w_f16, p.bias = bias, p.y = y, p.N = N, p.D = D, p.Dg = Dg, p.G = groups, p.k = k, p.TT = TT;
  const long blocks = (long)cdiv(N, TT) * groups;
  VBX_REQUIRE(blocks < (1L << 31), "vbx_hubert_posconv: too many tiles");
  const size_t bytes = hb_pos_lds(TT, Dg, k);
  const int MG = sn_blocks_per_item((Dg + 15) / 16, TT / 16);
  if (MG == 4) return sn_launch<hubert_posconv_kernel<4>>("vbx_hubert_posconv", p, (int)blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hubert_posconv_kernel<2>>("vbx_hubert_posconv", p, (int)blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hubert_posconv_kernel<1>>("vbx_hubert_posconv", p, (int)blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_hubert_split_heads(const float* qkv, void* q16, void* k16, void* v16, int B, int N, int H, float q_prescale, void* stream) {
  VBX_REQUIRE(qkv && q16 && k16 && v16, "vbx_hubert_split_heads: null operand");
  VBX_REQUIRE(B >= 1 && N >= 1 && H >= 1 && q_prescale > 0.f, "vbx_hubert_split_heads: bad dims");
  const long M = (long)B * N, items = M * (3 * H * 8);
  VBX_REQUIRE(items / 256 < (1L << 31) - 1, "vbx_hubert_split_heads: too large");
  hipLaunchKernelGGL(hubert_split_heads_kernel, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)stream, qkv, (u16*)q16, (u16*)k16, (u16*)v16, M, N, H,
                     q_prescale);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_kmeans_assign(const float* h, const float* centers, long long* ids, long M, int D, int K, void* stream) {
  VBX_REQUIRE(h && centers && ids, "vbx_kmeans_assign: null operand");
  VBX_REQUIRE(D >= 8 && D % 8 == 0 && D <= HB_KM_MAX_D, "vbx_kmeans_assign: D must be a multiple of 8 up to %d (got %d)", HB_KM_MAX_D, D);
  VBX_REQUIRE(K >= 1 && K <= HB_KM_MAX_K, "vbx_kmeans_assign: K must be in 1 .. %d (got %d)", HB_KM_MAX_K, K);
  VBX_REQUIRE(M >= 1 && M < (1L << 31), "vbx_kmeans_assign: need 1 <= rows < 2^31");
  hipLaunchKernelGGL(hubert_kmeans_kernel, dim3(cdiv(M, HB_KM_ROWS)), dim3(256), 0, (hipStream_t)stream, h, centers, ids, M, D, K);
  VBX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------- ragged waves: the entries
extern "C" int vbx_hubert_conv0_stats_lens(const float* wave, const int* lens, const float* w, float* records, float* stats, int B, long T, int C,
                                           int k0, int s0, float eps, void* stream) {
  VBX_REQUIRE(wave && w && records && stats, "vbx_hubert_conv0_stats_lens: null operand");
  VBX_REQUIRE(lens, "vbx_hubert_conv0_stats_lens: lens is NULL (vbx_hubert_conv0_stats is the entry without lengths)");
  long L0;
  if (int rc = hb_conv0_check("vbx_hubert_conv0_stats_lens", B, T, C, k0, s0, &L0)) return rc;
  const int chunks = cdiv(L0, HB_CHUNK);
  hipLaunchKernelGGL(hubert_conv0_stats_lens_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, wave, lens, w, records, (int)T, C, k0, s0,
                     chunks);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(hubert_conv0_finalize_lens_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, records, lens, stats, B * C,
                     (int)T, C, k0, s0, chunks, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_conv0_apply_lens(const float* wave, const int* lens, const float* w, const float* stats, const float* gamma,
                                           const float* beta, void* y_f16, int B, long T, int C, int k0, int s0, void* stream) {
  VBX_REQUIRE(wave && w && stats && gamma && beta && y_f16, "vbx_hubert_conv0_apply_lens: null operand");
  VBX_REQUIRE(lens, "vbx_hubert_conv0_apply_lens: lens is NULL (vbx_hubert_conv0_apply is the entry without lengths)");
  long L0;
  if (int rc = hb_conv0_check("vbx_hubert_conv0_apply_lens", B, T, C, k0, s0, &L0)) return rc;
  hipLaunchKernelGGL(hubert_conv0_apply_lens_kernel, dim3(cdiv(L0 * (C / 8), 256), B), dim3(256), 0, (hipStream_t)stream, wave, lens, w, stats, gamma,
                     beta, (u16*)y_f16, (int)T, (int)L0, C, k0, s0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_posconv_lens(const float* x, const int* lens, const void* w_f16, const float* bias, float* y, int B, int N, int D,
                                       int groups, int k, void* stream) {
  VBX_REQUIRE(x && w_f16 && bias && y && x != y, "vbx_hubert_posconv_lens: null operand, or y aliases x");
  VBX_REQUIRE(lens, "vbx_hubert_posconv_lens: lens is NULL (vbx_hubert_posconv is the entry without lengths)");
  VBX_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N < (1 << 24), "vbx_hubert_posconv_lens: need B in 1 .. 65535 and N in 1 .. 2^24");
  VBX_REQUIRE(groups >= 1 && D >= groups && D % groups == 0, "vbx_hubert_posconv_lens: groups must divide D");
  const int Dg = D / groups;
  if (int rc = hb_pos_check(Dg, k)) return rc;
  int TT = hb_pos_tile(Dg, k);
  VBX_REQUIRE(TT > 0, "vbx_hubert_posconv_lens: 16 output positions of this convolution do not fit the LDS");
  while (TT > 16 && TT / 2 >= N) TT >>= 1;  // the plain entry's tile at N: the grid does not depend on the lengths
  HbPosLens p;
  p.x = x, p.w = (const u16*)w_f16, p.bias = bias, p.y = y, p.N = N, p.D = D, p.Dg = Dg, p.G = groups, p.k = k, p.TT = TT, p.lens = lens;
  const long blocks = (long)cdiv(N, TT) * groups;
  VBX_REQUIRE(blocks < (1L << 31), "vbx_hubert_posconv_lens: too many tiles");
  const size_t bytes = hb_pos_lds(TT, Dg, k);
  const int MG = sn_blocks_per_item((Dg + 15) / 16, TT / 16);
  if (MG == 4) return sn_launch<hubert_posconv_lens_kernel<4>>("vbx_hubert_posconv_lens", p, (int)blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hubert_posconv_lens_kernel<2>>("vbx_hubert_posconv_lens", p, (int)blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hubert_posconv_lens_kernel<1>>("vbx_hubert_posconv_lens", p, (int)blocks, B, bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------- the large form: the entries
extern "C" int vbx_hubert_conv0_ln_tile(void) { return HB_LN0_POS; }

extern "C" int vbx_hubert_conv0_ln(const float* wave, const float* w, const float* bias, const float* gamma, const float* beta, void* y_f16, int B,
                                   long T, int C, int k0, int s0, float eps, void* stream) {
  VBX_REQUIRE(wave && w && gamma && beta && y_f16, "vbx_hubert_conv0_ln: null operand");
  long L0;
  if (int rc = hb_conv0_check("vbx_hubert_conv0_ln", B, T, C, k0, s0, &L0)) return rc;
  VBX_REQUIRE(C % 16 == 0, "vbx_hubert_conv0_ln: channels must be a multiple of 16 up to %d (got %d)", HB_MAX_C, C);
  hipLaunchKernelGGL(hubert_conv0_ln_kernel, dim3(cdiv(L0, HB_LN0_POS), B), dim3(256), 0, (hipStream_t)stream, wave, w, bias, gamma, beta,
                     (u16*)y_f16, (int)T, (int)L0, C, k0, s0, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hubert_conv_ln_tile(int C, int k) {
  if (int rc = hb_conv_check(C, k)) return rc;
  return hb_conv_ln_tile(C, k);  // never 0: 16 positions of 512 channels at k 3 take 34 KiB of span and 33 KiB of sums
}

extern "C" int vbx_hubert_conv_ln(const void* x_f16, const void* w_f16, const float* bias, const float* gamma, const float* beta, void* y_f16, int B,
                                  int L, int C, int k, float eps, void* stream) {
  VBX_REQUIRE(x_f16 && w_f16 && gamma && beta && y_f16, "vbx_hubert_conv_ln: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= k && L < (1 << 30), "vbx_hubert_conv_ln: need B in 1 .. 65535 and kernel_size <= L < 2^30");
  if (int rc = hb_conv_check(C, k)) return rc;
  HbConvLn p;
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.y = (u16*)y_f16, p.L = L, p.Lout = (L - k) / 2 + 1, p.C = C, p.k = k;
  p.bias = bias, p.gamma = gamma, p.beta = beta, p.eps = eps;
  int TT = hb_conv_ln_tile(C, k);
  while (TT > 16 && TT / 2 >= p.Lout) TT >>= 1;  // a short row: no tile of absent positions is staged or multiplied
  p.TT = TT;
  const size_t bytes = hb_conv_ln_lds(TT, C, k);
  const int MG = sn_blocks_per_item(C / 16, TT / 16), blocks = cdiv(p.Lout, TT);
  if (MG == 4) return sn_launch<hubert_conv_ln_kernel<4>>("vbx_hubert_conv_ln", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hubert_conv_ln_kernel<2>>("vbx_hubert_conv_ln", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hubert_conv_ln_kernel<1>>("vbx_hubert_conv_ln", p, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_hubert_conv_f32(const void* x_f16, const void* w_f16, const float* bias, float* s_f32, int B, int L, int C, int k, void* stream) {
  VBX_REQUIRE(x_f16 && w_f16 && s_f32, "vbx_hubert_conv_f32: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= k && L < (1 << 30), "vbx_hubert_conv_f32: need B in 1 .. 65535 and kernel_size <= L < 2^30");
  if (int rc = hb_conv_check(C, k)) return rc;
  HbConvF32 p;
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.y = nullptr, p.L = L, p.Lout = (L - k) / 2 + 1, p.C = C, p.k = k, p.bias = bias, p.s = s_f32;
  int TT = hb_conv_tile(C, k);
  while (TT > 16 && TT / 2 >= p.Lout) TT >>= 1;
  p.TT = TT;
  const size_t bytes = hb_conv_lds(TT, C, k);
  const int MG = sn_blocks_per_item(C / 16, TT / 16), blocks = cdiv(p.Lout, TT);
  if (MG == 4) return sn_launch<hubert_conv_f32_kernel<4>>("vbx_hubert_conv_f32", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hubert_conv_f32_kernel<2>>("vbx_hubert_conv_f32", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hubert_conv_f32_kernel<1>>("vbx_hubert_conv_f32", p, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_hubert_ln_gelu(const float* s_f32, const float* gamma, const float* beta, void* y_f16, long M, int C, float eps, void* stream) {
  VBX_REQUIRE(s_f32 && gamma && beta && y_f16, "vbx_hubert_ln_gelu: null operand");
  VBX_REQUIRE(M >= 1 && M < (1L << 31), "vbx_hubert_ln_gelu: need 1 <= rows < 2^31");
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= HB_MAX_C, "vbx_hubert_ln_gelu: channels must be a multiple of 8 up to %d (got %d)", HB_MAX_C, C);
  hipLaunchKernelGGL(hubert_ln_gelu_kernel, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, s_f32, gamma, beta, (u16*)y_f16, M, C, eps);
  VBX_LAUNCH_CHECK();
  return 0;
}

// 1: the pair (vbx_hubert_conv_f32 + vbx_hubert_ln_gelu) is the faster way at this shape, 0: the fused kernel.  The pair wins where the
// fp32 sums cost the fused kernel tile height (its tile is smaller than vbx_hubert_conv's) AND the grid is more than HB_PAIR_BLOCKS
// workgroups.  The rule rests on ONE measured shape on one MI355X (8 x 160 000 samples at C = 512, profiles/hubert_large_times.json):
// there it falls between layer 4 (8 x 125 = 1000 workgroups, the pair faster) and layer 5 (8 x 63 = 504, the fused kernel faster);
// no other batch size was measured.  The two routes give the same bits, so only speed hangs on it.
constexpr long HB_PAIR_BLOCKS = 512;
extern "C" int vbx_hubert_conv_ln_route(int B, int L, int C, int k) {
  if (int rc = hb_conv_check(C, k)) return rc;
  VBX_REQUIRE(B >= 1 && L >= k, "vbx_hubert_conv_ln_route: need B >= 1 and L >= kernel_size");
  const int TT = hb_conv_ln_tile(C, k);
  const long Lout = (L - k) / 2 + 1;
  return (TT < hb_conv_tile(C, k) && (long)B * ((Lout + TT - 1) / TT) > HB_PAIR_BLOCKS) ? 1 : 0;
}

extern "C" int vbx_wave_normalize_chunk(void) { return HB_WN_CHUNK; }

extern "C" int vbx_wave_normalize(const float* x, const int* lens, float* y, float* records, double* stats, int B, long T, float eps, void* stream) {
  VBX_REQUIRE(x && y && records && stats, "vbx_wave_normalize: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T < (1L << 31), "vbx_wave_normalize: need B in 1 .. 65535 and 1 <= T < 2^31");
  VBX_REQUIRE(eps > 0.f, "vbx_wave_normalize: eps must be positive");
  const int chunks = cdiv(T, HB_WN_CHUNK);
  hipLaunchKernelGGL(wave_normalize_stats_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, x, lens, records, (int)T, chunks);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(wave_normalize_finalize_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, records, lens, stats, B, (int)T, chunks, eps);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(wave_normalize_apply_kernel, dim3(cdiv(T, 1024), B), dim3(256), 0, (hipStream_t)stream, x, lens, stats, y, (int)T);
  VBX_LAUNCH_CHECK();
  return 0;
}
