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
// bits on every run, and a batch row's result does not depend on its neighbours.
#include "seanet_tile.hpp"

namespace {

constexpr int HG_FILL_WGS = 256;  // a launch with fewer workgroups than the MI355X has CUs takes a smaller tile (same bits: a sum's order does not depend on the tile)
constexpr int HG_MAX_K = 11, HG_MAX_DIL = 12, HG_MAX_C = 1024, HG_MAX_STRIDE = 8, HG_PAIR_MAX_C = 64, HG_POST_MAX_C = 512;

VBX_DEV float hg_lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }

// up to three fp16 tensors of one shape, read as their mean: ((x0 + x1) + x2) / n in fp32 (n = 2: an exact halving; n = 3: an IEEE division)
struct HgIn {
  const u16* x[3];
  int n;
};

VBX_DEV float hg_mean(float a, float b, float c, int n) { return n == 1 ? a : (n == 2 ? (a + b) * 0.5f : ((a + b) + c) / 3.0f); }

// eight channels at element offset `off` as fp32: the mean of the inputs, then the leaky ReLU (slope 1 leaves the value alone)
VBX_DEV void hg_read8(const HgIn& in, long off, float slope, float out[8]) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 v0 = *reinterpret_cast<const uint4*>(in.x[0] + off);
  const uint4 v1 = in.n > 1 ? *reinterpret_cast<const uint4*>(in.x[1] + off) : z;
  const uint4 v2 = in.n > 2 ? *reinterpret_cast<const uint4*>(in.x[2] + off) : z;
  const unsigned a[4] = {v0.x, v0.y, v0.z, v0.w}, b[4] = {v1.x, v1.y, v1.z, v1.w}, c[4] = {v2.x, v2.y, v2.z, v2.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[2 * i] = hg_lrelu(hg_mean(f16_to_f32((u16)(a[i] & 0xFFFFu)), f16_to_f32((u16)(b[i] & 0xFFFFu)), f16_to_f32((u16)(c[i] & 0xFFFFu)), in.n), slope);
    out[2 * i + 1] = hg_lrelu(hg_mean(f16_to_f32((u16)(a[i] >> 16)), f16_to_f32((u16)(b[i] >> 16)), f16_to_f32((u16)(c[i] >> 16)), in.n), slope);
  }
}

VBX_DEV uint4 hg_stage8(const HgIn& in, long off, float slope) {
  float f[8];
  hg_read8(in, off, slope, f);
  return make_uint4(pack_f16x2(f[0], f[1]), pack_f16x2(f[2], f[3]), pack_f16x2(f[4], f[5]), pack_f16x2(f[6], f[7]));
}

VBX_DEV uint4 hg_lrelu8(uint4 v, float slope) {
  unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++)
    w[i] = pack_f16x2(hg_lrelu(f16_to_f32((u16)(w[i] & 0xFFFFu)), slope), hg_lrelu(f16_to_f32((u16)(w[i] >> 16)), slope));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// `rows` LDS rows of C channels (row stride ld) from positions i0, i0 + 1, ... of batch row xb [L, C]: zeros outside [0, L), else the
// stored value, through the leaky ReLU when act
VBX_DEV void hg_stage_span(u16* s, int ld, const u16* xb, int i0, int rows, int L, int C, int act, float slope) {
  const int c8 = C >> 3;
  for (int e = threadIdx.x; e < rows * c8; e += 256) {
    const int pos = e / c8, c = (e - pos * c8) * 8;
    const int i = i0 + pos;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i >= 0 && i < L) {
      v = *reinterpret_cast<const uint4*>(xb + (long)i * C + c);
      if (act) v = hg_lrelu8(v, slope);
    }
    *reinterpret_cast<uint4*>(s + pos * ld + c) = v;
  }
}

struct HgConv {
  const u16* x;       // [B, L, C]
  const u16* w;       // [Co, k * C], column tap * C + c
  const float* bias;  // [Co]
  const u16* res;     // [B, L, Co] or NULL: added in fp32 before the one rounding
  u16* y;             // [B, L, Co]
  int L, C, Co, k, dil, pad, act, TT, Ktot;
  float slope;
};

// A workgroup owns TT consecutive positions of one batch row and all Co channels: it stages TT + (k - 1) dil positions (zero padded,
// activated) and runs the product; row m of the A operand is the k runs of C channels at LDS rows m + tap * dil.
template <int MG>
__global__ __launch_bounds__(256) void hifigan_conv_kernel(HgConv p) {
  extern __shared__ __attribute__((aligned(16))) u16 hg_lds[];
  const int b = blockIdx.y, t0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH;
  hg_stage_span(hg_lds, ld, p.x + (long)b * p.L * p.C, t0 - p.pad, p.TT + (p.k - 1) * p.dil, p.L, p.C, p.act, p.slope);
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.C, c = kk - tap * p.C;
    base = hg_lds + tap * p.dil * ld + c, ldr = ld;
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias[n]](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t >= p.L) return;
      const long o = ((long)b * p.L + t) * p.Co + n;
      float s = v + bv;
      if (p.res) s += f16_to_f32(p.res[o]);
      p.y[o] = f32_to_f16(s);
    };
  };
  sn_tile_product<MG, true>(p.w, p.Co, p.Ktot, p.TT >> 4, rows, store);
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

struct HgConvTr {
  HgIn in;            // [B, L, C] each; their mean is activated as it is staged
  const u16* w;       // [r * Co, 2C]: row p * Co + o = [W[:, o, p] | W[:, o, p + r]]
  const float* bias;  // [Co]
  u16* y;             // [B, L * r, Co]
  int L, C, Co, r, left, TT, N, Ktot;
  float slope;
};

// ConvTranspose1d(C, C / 2, 2 r, stride r, padding r / 2), r even, as ONE product over rows j = 0 .. L with the operand row
// [a_j | a_{j-1}] (a_{-1} = a_L = 0): the r Co results of row j are the contiguous run of output positions from j r - r / 2 on (row 0
// drops its phases below r / 2, row L keeps only those).  LDS row m holds position j0 - 1 + m.
template <int MG>
__global__ __launch_bounds__(256) void hifigan_convtr_kernel(HgConvTr p) {
  extern __shared__ __attribute__((aligned(16))) u16 hg_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, j0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH;
  {
    const int c8 = p.C >> 3;
    const long rowoff = (long)b * p.L * p.C;
    for (int e = tid; e < (p.TT + 1) * c8; e += 256) {
      const int pos = e / c8, c = (e - pos * c8) * 8;
      const int i = j0 - 1 + pos;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (i >= 0 && i < p.L) v = hg_stage8(p.in, rowoff + (long)i * p.C + c, p.slope);
      *reinterpret_cast<uint4*>(hg_lds + pos * ld + c) = v;
    }
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    base = kk < p.C ? hg_lds + ld + kk : hg_lds + (kk - p.C), ldr = ld;
  };
  const long Lout = (long)p.L * p.r;
  auto store = [&](int n) __attribute__((always_inline)) {
    const int ph = n / p.Co, o = n - ph * p.Co;
    return [&, ph, o, bv = p.bias[o]](int m, float v) __attribute__((always_inline)) {
      const int j = j0 + m;
      const long t = (long)j * p.r + (ph - p.left);
      if (j <= p.L && t >= 0 && t < Lout) p.y[((long)b * Lout + t) * p.Co + o] = f32_to_f16(v + bv);
    };
  };
  sn_tile_product<MG, false>(p.w, p.N, p.Ktot, p.TT >> 4, rows, store);
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

int hg_conv_check(const char* who, int C, int k, int dil) {
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= HG_MAX_C, "%s: C must be a multiple of 8 in 8 .. %d (got %d)", who, HG_MAX_C, C);
  VBX_REQUIRE(k >= 1 && k <= HG_MAX_K && (k & 1), "%s: the kernel must be odd, at most %d (got %d)", who, HG_MAX_K, k);
  VBX_REQUIRE(dil >= 1 && dil <= HG_MAX_DIL, "%s: the dilation must be in 1 .. %d (got %d)", who, HG_MAX_DIL, dil);
  return 0;
}

size_t hg_conv_lds(int TT, int C, int k, int dil) { return (size_t)(TT + (k - 1) * dil) * (C + SN_PADH) * sizeof(u16); }

int hg_conv_tile(int C, int k, int dil) {
  return sn_pick_tile([=](int TT) { return hg_conv_lds(TT, C, k, dil); });
}

size_t hg_convtr_lds(int TT, int C) { return (size_t)(TT + 1) * (C + SN_PADH) * sizeof(u16); }

int hg_convtr_tile(int C) {
  return sn_pick_tile([=](int TT) { return hg_convtr_lds(TT, C); });
}

// the fused pair's tiles: TT positions with MR = TT + 16 intermediate rows (k - 1 <= 10 of them are c2's halo)
int hg_pair_tile(int L) { return L > 48 ? 112 : (L > 16 ? 48 : 16); }

int hg_in(HgIn& in, const void* x0, const void* x1, const void* x2, int n, const char* who) {
  VBX_REQUIRE(n >= 1 && n <= 3 && x0 && (n < 2 || x1) && (n < 3 || x2), "%s: 1 .. 3 inputs, none of them null", who);
  in.x[0] = (const u16*)x0, in.x[1] = n > 1 ? (const u16*)x1 : nullptr, in.x[2] = n > 2 ? (const u16*)x2 : nullptr, in.n = n;
  return 0;
}

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
  VBX_REQUIRE(x_f16 && w_f16 && bias && y_f16, "vbx_hifigan_conv: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1 << 30) && Co >= 1 && Co <= 4096, "vbx_hifigan_conv: need B in 1 .. 65535, L in 1 .. 2^30 - 1, Co in 1 .. 4096");
  if (int rc = hg_conv_check("vbx_hifigan_conv", C, k, dilation)) return rc;
  int TT = hg_conv_tile(C, k, dilation);
  VBX_REQUIRE(TT > 0, "vbx_hifigan_conv: 16 output positions of this convolution do not fit the LDS");
  while (TT > 16 && TT / 2 >= L) TT >>= 1;  // a short row: no tile of padding positions is staged or multiplied
  while (TT > 16 && (long)cdiv(L, TT) * B < HG_FILL_WGS) TT >>= 1;  // a small launch: more, smaller workgroups
  HgConv p;
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.bias = bias, p.res = (const u16*)res_f16, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.Co = Co, p.k = k, p.dil = dilation, p.pad = (k - 1) * dilation / 2, p.act = act ? 1 : 0, p.TT = TT, p.Ktot = k * C;
  p.slope = slope;
  const size_t bytes = hg_conv_lds(TT, C, k, dilation);
  const int MG = sn_blocks_per_item((Co + 15) / 16, TT / 16), blocks = cdiv(L, TT);
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
  HgConvTr p;
  if (int rc = hg_in(p.in, x0_f16, x1_f16, x2_f16, inputs, "vbx_hifigan_convtr")) return rc;
  VBX_REQUIRE(w_f16 && bias && y_f16, "vbx_hifigan_convtr: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "vbx_hifigan_convtr: need B in 1 .. 65535, L >= 1");
  VBX_REQUIRE(C >= 16 && C % 16 == 0 && C <= HG_MAX_C, "vbx_hifigan_convtr: C must be a multiple of 16 in 16 .. %d (got %d)", HG_MAX_C, C);
  VBX_REQUIRE(stride >= 2 && stride <= HG_MAX_STRIDE && stride % 2 == 0, "vbx_hifigan_convtr: the rate must be even, in 2 .. %d (got %d)",
              HG_MAX_STRIDE, stride);
  VBX_REQUIRE((long)L * stride < (1L << 30), "vbx_hifigan_convtr: row too long");
  int TT = hg_convtr_tile(C);
  VBX_REQUIRE(TT > 0, "vbx_hifigan_convtr: 16 rows of this transposed convolution do not fit the LDS");
  const int rows = L + 1;
  while (TT > 16 && TT / 2 >= rows) TT >>= 1;  // a short row: no tile of rows that store nothing
  while (TT > 16 && (long)cdiv(rows, TT) * B < HG_FILL_WGS) TT >>= 1;  // a small launch: more, smaller workgroups
  p.w = (const u16*)w_f16, p.bias = bias, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.Co = C / 2, p.r = stride, p.left = stride / 2, p.TT = TT, p.N = stride * (C / 2), p.Ktot = 2 * C, p.slope = slope;
  const size_t bytes = hg_convtr_lds(TT, C);
  const int MG = sn_blocks_per_item((p.N + 15) / 16, TT / 16), blocks = cdiv(rows, TT);
  if (MG == 4) return sn_launch<hifigan_convtr_kernel<4>>("vbx_hifigan_convtr", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hifigan_convtr_kernel<2>>("vbx_hifigan_convtr", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hifigan_convtr_kernel<1>>("vbx_hifigan_convtr", p, blocks, B, bytes, (hipStream_t)stream);
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
