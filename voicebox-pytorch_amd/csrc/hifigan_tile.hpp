// What the HiFi-GAN family (hifigan.hip) and the BigVGAN family (bigvgan.hip) share on the tile core of seanet_tile.hpp: the
// multi-input mean, the staged span, the convolution's product and epilogue, the transposed convolution and the tile choices.  Moved
// unchanged out of hifigan.hip; everything is file-local to the translation unit that includes it.
#pragma once
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

// the product and the epilogue of a convolution whose span of TT + (k - 1) dil positions from t0 - pad is staged at lds (row stride
// C + SN_PADH): row m of the A operand is the k runs of C channels at LDS rows m + tap * dil
template <int MG>
VBX_DEV void hg_conv_product(const HgConv& p, const u16* lds, int b, int t0) {
  const int ld = p.C + SN_PADH;
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    const int tap = kk / p.C, c = kk - tap * p.C;
    base = lds + tap * p.dil * ld + c, ldr = ld;
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

int hg_in(HgIn& in, const void* x0, const void* x1, const void* x2, int n, const char* who) {
  VBX_REQUIRE(n >= 1 && n <= 3 && x0 && (n < 2 || x1) && (n < 3 || x2), "%s: 1 .. 3 inputs, none of them null", who);
  in.x[0] = (const u16*)x0, in.x[1] = n > 1 ? (const u16*)x1 : nullptr, in.x[2] = n > 2 ? (const u16*)x2 : nullptr, in.n = n;
  return 0;
}

// the checks and the tile of a convolution launch, shared by the entry points that differ only in how the span is staged
int hg_conv_setup(const char* who, HgConv& p, const void* x_f16, const void* w_f16, const float* bias, const void* res_f16, void* y_f16, int B,
                  int L, int C, int Co, int k, int dilation) {
  VBX_REQUIRE(x_f16 && w_f16 && bias && y_f16, "%s: null operand", who);
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1 << 30) && Co >= 1 && Co <= 4096, "%s: need B in 1 .. 65535, L in 1 .. 2^30 - 1, Co in 1 .. 4096", who);
  if (int rc = hg_conv_check(who, C, k, dilation)) return rc;
  int TT = hg_conv_tile(C, k, dilation);
  VBX_REQUIRE(TT > 0, "%s: 16 output positions of this convolution do not fit the LDS", who);
  while (TT > 16 && TT / 2 >= L) TT >>= 1;  // a short row: no tile of padding positions is staged or multiplied
  while (TT > 16 && (long)cdiv(L, TT) * B < HG_FILL_WGS) TT >>= 1;  // a small launch: more, smaller workgroups
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.bias = bias, p.res = (const u16*)res_f16, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.Co = Co, p.k = k, p.dil = dilation, p.pad = (k - 1) * dilation / 2, p.act = 0, p.TT = TT, p.Ktot = k * C;
  p.slope = 1.0f;
  return 0;
}

// vbx_hifigan_convtr / vbx_bigvgan_convtr: one kernel, the entry points differ in the width they accept
int hg_convtr_launch(const char* who, int max_c, const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const void* w_f16,
                     const float* bias, void* y_f16, int B, int L, int C, int stride, float slope, void* stream) {
  HgConvTr p;
  if (int rc = hg_in(p.in, x0_f16, x1_f16, x2_f16, inputs, who)) return rc;
  VBX_REQUIRE(w_f16 && bias && y_f16, "%s: null operand", who);
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "%s: need B in 1 .. 65535, L >= 1", who);
  VBX_REQUIRE(C >= 16 && C % 16 == 0 && C <= max_c, "%s: C must be a multiple of 16 in 16 .. %d (got %d)", who, max_c, C);
  VBX_REQUIRE(stride >= 2 && stride <= HG_MAX_STRIDE && stride % 2 == 0, "%s: the rate must be even, in 2 .. %d (got %d)", who, HG_MAX_STRIDE,
              stride);
  VBX_REQUIRE((long)L * stride < (1L << 30), "%s: row too long", who);
  int TT = hg_convtr_tile(C);
  VBX_REQUIRE(TT > 0, "%s: 16 rows of this transposed convolution do not fit the LDS", who);
  const int rows = L + 1;
  while (TT > 16 && TT / 2 >= rows) TT >>= 1;  // a short row: no tile of rows that store nothing
  while (TT > 16 && (long)cdiv(rows, TT) * B < HG_FILL_WGS) TT >>= 1;  // a small launch: more, smaller workgroups
  p.w = (const u16*)w_f16, p.bias = bias, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.Co = C / 2, p.r = stride, p.left = stride / 2, p.TT = TT, p.N = stride * (C / 2), p.Ktot = 2 * C, p.slope = slope;
  const size_t bytes = hg_convtr_lds(TT, C);
  const int MG = sn_blocks_per_item((p.N + 15) / 16, TT / 16), blocks = cdiv(rows, TT);
  if (MG == 4) return sn_launch<hifigan_convtr_kernel<4>>(who, p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<hifigan_convtr_kernel<2>>(who, p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<hifigan_convtr_kernel<1>>(who, p, blocks, B, bytes, (hipStream_t)stream);
}

}  // namespace
