// HiFiGANGenerator (voicebox-pytorch_amd/hifigan.py): the generator of HiFi-GAN (Kong et al. 2020, "HiFi-GAN: generative adversarial
// networks for efficient and high fidelity speech synthesis") on the device, inference only: mels into a wave.  The launch sequence
// of one call (V1: 4 stages, 3 residual blocks of 3 dilations each):
//
//   vbx_hifigan_pack      mel fp32 [B, M, T] channel-first -> fp16 [B, T, ceil8(M)], optionally log(max(mel, 1e-5)), rounded once
//   vbx_hifigan_conv      conv_pre: k 7, zero padding, no activation
//   per stage (rate u):
//     vbx_hifigan_convtr  leaky ReLU 0.1, transposed convolution k 2u, stride u, padding u / 2, C -> C / 2, ONE product over rows
//                         [a_j | a_{j-1}]; its staging sums the (up to three) residual blocks' outputs of the stage before and divides
//                         by their count: the multi-receptive-field mean costs no launch and no tensor
//     per residual block, per dilation d:
//       vbx_hifigan_respair   x + c2(lrelu(c1(lrelu(x)))) in ONE launch where it is faster (narrow stages), else
//       vbx_hifigan_conv x 2  c1 (k, dilation d), then c2 (k, dilation 1) with x added in the epilogue
//   vbx_hifigan_post      the same multi-input mean, leaky ReLU 0.01, k 7, C -> 1, fp32 weights, tanhf: the wave fp32 [B, T * hop]
// (the fused pair serves the widths where it measured faster: HiFiGANGenerator.FUSE_MAX_CHANNELS, profiles/hifigan_times.json)
//
// Precision contract (include/vbx.h): SEANet's.  Activations fp16 channel-last, rounded once, stored BEFORE the leaky ReLU (the
// residual reads them un-activated); the leaky ReLU is x > 0 ? x : x * slope in fp32, applied when an operand is staged and rounded
// to fp16 there; weights fp16; every sum fp32 on v_mfma_f32_16x16x32_f16 in ascending column order.  All paddings are zeros and are
// resolved as a workgroup stages its span: it reads its own batch row only, inside [0, L).  Plain launches, no atomics: the same
// bits on every run, and a batch row's result does not depend on its neighbours.  What the BigVGAN family (bigvgan.hip) needs as well
// -- the mean of up to three inputs, the span staging, the convolution's product, the transposed convolution -- is in hifigan_tile.hpp.
#include "hifigan_tile.hpp"

namespace {

// A workgroup owns TT consecutive positions of one batch row and all Co channels: it stages TT + (k - 1) dil positions (zero padded,
// activated) and runs the product; row m of the A operand is the k runs of C channels at LDS rows m + tap * dil.
template <int MG>
__global__ __launch_bounds__(256) void hifigan_conv_kernel(HgConv p) {
  extern __shared__ __attribute__((aligned(16))) u16 hg_lds[];
  const int b = blockIdx.y, t0 = blockIdx.x * p.TT;
  hg_stage_span(hg_lds, p.C + SN_PADH, p.x + (long)b * p.L * p.C, t0 - p.pad, p.TT + (p.k - 1) * p.dil, p.L, p.C, p.act, p.slope);
  __syncthreads();
  hg_conv_product<MG>(p, hg_lds, b, t0);
}

template <bool TAIL, class ARows, class Store>
VBX_DEV void hg_product(int mg, const u16* w, int N, int Ktot, int MT, const ARows& rows, const Store& store) {
  if (mg == 4) sn_tile_product<4, TAIL>(w, N, Ktot, MT, rows, store);
  else if (mg == 2) sn_tile_product<2, TAIL>(w, N, Ktot, MT, rows, store);
  else sn_tile_product<1, TAIL>(w, N, Ktot, MT, rows, store);
}

struct HgPair {
  const u16* x;          // [B, L, C]
  const u16 *w1, *w2;    // [C, k * C] each
  const float *b1, *b2;  // [C]
  u16* y;                // [B, L, C]
  int L, C, k, dil, pad1, pad2, TT, MR, mg1, mg2, Ktot;
  float slope;
};

// y = x + c2(lrelu(c1(lrelu(x)))) in one launch, bit-equal to two hifigan_conv_kernel launches.  A workgroup owns TT positions from t0:
// c2 (dilation 1) needs c1 at positions t0 - pad2 .. t0 + TT - 1 + pad2, MR = the next multiple of 16 rows; c1 (dilation d) needs x at
// MR + (k - 1) d positions from t0 - pad2 - pad1.  Phase 1 multiplies the staged span and leaves lrelu(fp16(c1 + b1)), rounded to fp16
// as the operand -- what the second launch would have staged from the stored tensor -- in the LDS; an intermediate position outside
// [0, L) is c2's zero padding and is stored as ZERO, not as c1 evaluated past the row.  Phase 2 multiplies those rows and adds x; it
// runs over MR rows as well (MR / 16 is even, TT / 16 is odd and would leave one row block per work item: four times the weight
// loads), over 16 more zero rows of the intermediate, and drops the rows from TT on.
__global__ __launch_bounds__(256) void hifigan_respair_kernel(HgPair p) {
  extern __shared__ __attribute__((aligned(16))) u16 hg_lds[];
  const int b = blockIdx.y, t0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH;
  const int xrows = p.MR + (p.k - 1) * p.dil;
  u16* xs = hg_lds;
  u16* hs = hg_lds + xrows * ld;
  const u16* xb = p.x + (long)b * p.L * p.C;
  hg_stage_span(xs, ld, xb, t0 - p.pad2 - p.pad1, xrows, p.L, p.C, 1, p.slope);
  for (int e = threadIdx.x; e < 16 * (p.C >> 3); e += 256)
    *reinterpret_cast<uint4*>(hs + (p.MR + e / (p.C >> 3)) * ld + (e % (p.C >> 3)) * 8) = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  {
    auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
      const int tap = kk / p.C, c = kk - tap * p.C;
      base = xs + tap * p.dil * ld + c, ldr = ld;
    };
    auto store = [&](int n) __attribute__((always_inline)) {
      return [&, n, bv = p.b1[n]](int m, float v) __attribute__((always_inline)) {
        const int i = t0 - p.pad2 + m;
        u16 h = 0;
        if (i >= 0 && i < p.L) h = f32_to_f16(hg_lrelu(f16_to_f32(f32_to_f16(v + bv)), p.slope));
        hs[m * ld + n] = h;
      };
    };
    hg_product<true>(p.mg1, p.w1, p.C, p.Ktot, p.MR >> 4, rows, store);
  }
  __syncthreads();
  {
    auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
      const int tap = kk / p.C, c = kk - tap * p.C;
      base = hs + tap * ld + c, ldr = ld;
    };
    auto store = [&](int n) __attribute__((always_inline)) {
      return [&, n, bv = p.b2[n]](int m, float v) __attribute__((always_inline)) {
        const int t = t0 + m;
        if (m >= p.TT || t >= p.L) return;
        const long o = (long)t * p.C + n;
        p.y[(long)b * p.L * p.C + o] = f32_to_f16((v + bv) + f16_to_f32(xb[o]));
      };
    };
    hg_product<true>(p.mg2, p.w2, p.C, p.Ktot, p.MR >> 4, rows, store);
  }
}

// conv_post, C -> 1: one thread per output sample.  The operand lrelu(mean of the inputs), fp32 and not rounded again, is staged once
// per workgroup (256 + k - 1 positions, 32 channels at a time, rows 33 floats apart: conflict-free) instead of once per tap; the
// k * C products are ONE fmaf chain on the bias: per chunk of 32 channels tap-major, then channel (for C <= 32: tap-major, then
// channel).  A tap in the zero padding multiplies a staged zero and leaves the sum as it is.  tanhf on the sum.
constexpr int HG_POST_CH = 32, HG_POST_LD = HG_POST_CH + 1;

__global__ __launch_bounds__(256) void hifigan_post_kernel(HgIn in, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, int T, int C, int k, float slope) {
  extern __shared__ __attribute__((aligned(16))) float hg_sw[];  // [k][C] weights, then [256 + k - 1][33] operands
  float* sx = hg_sw + k * C;
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k * C; e += 256) hg_sw[e] = w[e];
  const long p0 = (long)blockIdx.x * 256, pos = p0 + tid;
  const long rowoff = (long)b * T * C;
  const int rows = 256 + k - 1;
  float acc = bias[0];
  for (int c0 = 0; c0 < C; c0 += HG_POST_CH) {
    const int cw = C - c0 < HG_POST_CH ? C - c0 : HG_POST_CH, g8 = cw >> 3;
    __syncthreads();  // the chunk before is consumed (first pass: nothing to wait for but the weights' stores below)
    for (int e = tid; e < rows * g8; e += 256) {
      const int r = e / g8, c = (e - r * g8) * 8;
      const long i = p0 + r - (k >> 1);
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (i >= 0 && i < T) hg_read8(in, rowoff + i * C + c0 + c, slope, a);
#pragma unroll
      for (int j = 0; j < 8; j++) sx[r * HG_POST_LD + c + j] = a[j];
    }
    __syncthreads();
    for (int tap = 0; tap < k; tap++)
      for (int c = 0; c < cw; c++) acc = fmaf(hg_sw[tap * C + c0 + c], sx[(tid + tap) * HG_POST_LD + c], acc);
  }
  if (pos < T) y[(long)b * T + pos] = tanhf(acc);
}

// mel fp32 [B, M, T] channel-first -> fp16 [B, T, Mp] channel-last, Mp = ceil8(M), the columns from M on zero; rounded once; with
// `log` the value is logf(fmaxf(mel, 1e-5f)) first.  A 32 x 32 tile through the LDS.
__global__ __launch_bounds__(256) void hifigan_pack_kernel(const float* __restrict__ z, u16* __restrict__ y, int M, int Mp, int T, int log) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int d = d0 + r, t = t0 + tx;
    float v = 0.f;
    if (d < M && t < T) {
      v = z[((long)b * M + d) * T + t];
      if (log) v = logf(fmaxf(v, 1e-5f));
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int t = t0 + r, d = d0 + tx;
    if (t < T && d < Mp) y[((long)b * T + t) * Mp + d] = f32_to_f16(tile[tx][r]);
  }
}

// the fused pair's tiles: TT positions with MR = TT + 16 intermediate rows (k - 1 <= 10 of them are c2's halo)
int hg_pair_tile(int L) { return L > 48 ? 112 : (L > 16 ? 48 : 16); }

}  // namespace

extern "C" int vbx_hifigan_pack(const float* mel, void* y_f16, int B, int M, int T, int log, void* stream) {
  VBX_REQUIRE(mel && y_f16 && B >= 1 && B <= 65535 && M >= 1 && M <= 512 && T >= 1, "vbx_hifigan_pack: need B in 1 .. 65535, n_mels in 1 .. 512, T >= 1");
  const int Mp = (M + 7) / 8 * 8;
  hipLaunchKernelGGL(hifigan_pack_kernel, dim3(cdiv(T, 32), cdiv(Mp, 32), B), dim3(256), 0, (hipStream_t)stream, mel, (u16*)y_f16, M, Mp, T,
                     log ? 1 : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_hifigan_conv_tile(int C, int k, int dilation) {
  if (int rc = hg_conv_check("vbx_hifigan_conv", C, k, dilation)) return rc;
  const int TT = hg_conv_tile(C, k, dilation);
  if (!TT) {
    vbx_set_error("vbx_hifigan_conv: 16 output positions of this convolution do not fit the LDS");
    return VBX_EINVAL;
  }
  return TT;
}

extern "C" int vbx_hifigan_conv(const void* x_f16, const void* w_f16, const float* bias, const void* res_f16, void* y_f16, int B, int L, int C,
                                int Co, int k, int dilation, int act, float slope, void* stream) {
  HgConv p;
  if (int rc = hg_conv_setup("vbx_hifigan_conv", p, x_f16, w_f16, bias, res_f16, y_f16, B, L, C, Co, k, dilation)) return rc;
  p.act = act ? 1 : 0, p.slope = slope;
  const size_t bytes = hg_conv_lds(p.TT, C, k, dilation);
  const int MG = sn_blocks_per_item((Co + 15) / 16, p.TT / 16), blocks = cdiv(L, p.TT);
  if (MG == 4) return sn_launch<hifigan_conv_kernel<4>>("vbx_hifigan_conv", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hifigan_conv_kernel<2>>("vbx_hifigan_conv", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hifigan_conv_kernel<1>>("vbx_hifigan_conv", p, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_hifigan_respair_max_channels(void) { return HG_PAIR_MAX_C; }

extern "C" int vbx_hifigan_respair(const void* x_f16, const void* w1_f16, const float* bias1, const void* w2_f16, const float* bias2,
                                   void* y_f16, int B, int L, int C, int k, int dilation, float slope, void* stream) {
  VBX_REQUIRE(x_f16 && w1_f16 && bias1 && w2_f16 && bias2 && y_f16, "vbx_hifigan_respair: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1 << 30), "vbx_hifigan_respair: need B in 1 .. 65535, L in 1 .. 2^30 - 1");
  if (int rc = hg_conv_check("vbx_hifigan_respair", C, k, dilation)) return rc;
  VBX_REQUIRE(C <= HG_PAIR_MAX_C, "vbx_hifigan_respair: C must be at most %d (got %d)", HG_PAIR_MAX_C, C);
  HgPair p;
  p.x = (const u16*)x_f16, p.w1 = (const u16*)w1_f16, p.w2 = (const u16*)w2_f16, p.b1 = bias1, p.b2 = bias2, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.k = k, p.dil = dilation, p.pad1 = (k - 1) * dilation / 2, p.pad2 = (k - 1) / 2;
  p.TT = hg_pair_tile(L), p.MR = p.TT + 16, p.Ktot = k * C, p.slope = slope;
  const int NT = (C + 15) / 16;
  p.mg1 = p.mg2 = sn_blocks_per_item(NT, p.MR / 16);
  const size_t bytes = (size_t)(2 * p.MR + 16 + (k - 1) * dilation) * (C + SN_PADH) * sizeof(u16);  // at most 392 rows of 72: 56 KiB
  return sn_launch<hifigan_respair_kernel>("vbx_hifigan_respair", p, cdiv(L, p.TT), B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_hifigan_convtr(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const void* w_f16,
                                  const float* bias, void* y_f16, int B, int L, int C, int stride, float slope, void* stream) {
  return hg_convtr_launch("vbx_hifigan_convtr", HG_MAX_C, x0_f16, x1_f16, x2_f16, inputs, w_f16, bias, y_f16, B, L, C, stride, slope, stream);
}

extern "C" int vbx_hifigan_post(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* w, const float* bias,
                                float* y, int B, int T, int C, int k, float slope, void* stream) {
  HgIn in;
  if (int rc = hg_in(in, x0_f16, x1_f16, x2_f16, inputs, "vbx_hifigan_post")) return rc;
  VBX_REQUIRE(w && bias && y && B >= 1 && B <= 65535 && T >= 1 && T < (1 << 30), "vbx_hifigan_post: need B in 1 .. 65535, T in 1 .. 2^30 - 1");
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= HG_POST_MAX_C, "vbx_hifigan_post: C must be a multiple of 8 up to %d (got %d)", HG_POST_MAX_C, C);
  VBX_REQUIRE(k >= 1 && k <= HG_MAX_K && (k & 1), "vbx_hifigan_post: the kernel must be odd, at most %d (got %d)", HG_MAX_K, k);
  hipLaunchKernelGGL(hifigan_post_kernel, dim3(cdiv(T, 256), B), dim3(256), ((size_t)k * C + (256 + k - 1) * HG_POST_LD) * sizeof(float), (hipStream_t)stream, in, w, bias, y,
                     T, C, k, slope);
  VBX_LAUNCH_CHECK();
  return 0;
}
