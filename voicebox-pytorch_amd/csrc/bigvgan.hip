// BigVGANGenerator (voicebox-pytorch_amd/bigvgan.py): the generator of BigVGAN (Lee et al. 2023, "BigVGAN: a universal neural vocoder
// with large-scale training") on the device, inference only.  It is HiFi-GAN's generator (hifigan.hip; the shared device code is
// hifigan_tile.hpp) with every leaky ReLU replaced by Activation1d: up-sample by 2 with a 12-tap Kaiser-sinc filter, the periodic
// snake function per channel, low-pass and down-sample by 2 with 12 taps -- and with NO activation in front of the transposed
// convolutions.  The launch sequence of one call:
//
//   vbx_hifigan_pack, vbx_hifigan_conv (conv_pre)
//   per stage: vbx_bigvgan_convtr   the transposed convolution on the mean of the residual blocks before it, not activated
//     per residual convolution: vbx_bigvgan_act + vbx_hifigan_conv(act = 0), or vbx_bigvgan_conv: the same bits in one launch, the
//                               activated tensor never leaves the LDS
//   vbx_bigvgan_post                A of the mean, k 7, C -> 1, tanhf or a clamp to [-1, 1]
//
// A(x)[t], per channel, in closed form (both replicate paddings of the published modules written as clamps):
//   u[m] = 2 sum_i f_u[m + 5 - 2 i] x[clamp(i, 0, L - 1)]   over the six i with 0 <= m + 5 - 2 i <= 11, m in [0, 2 L)
//   s[m] = u[m] + inv_beta sin^2(alpha u[m])
//   y[t] = sum_{tau = 0 .. 11} f_d[tau] s[clamp(2 t + tau - 5, 0, 2 L - 1)]
// The two clamps act on different signals.  ORDER OF OPERATIONS (include/vbx.h; bv_s and bv_y below are the only implementation, so
// every kernel here gives the same bits for the same x): both sums are fmaf chains from 0.f in ascending i / tau; u = 2 * sum;
// a = alpha * u (one rounded product, not contracted); sn = sinf(a) (the accurate library form); s = fmaf(inv_beta, sn * sn, u).
// Everything fp32; x is the fp32 mean ((x0 + x1) + x2) / n of the fp16 inputs; y is rounded to fp16 once.
//
// Each s[m] feeds six outputs.  A thread owns two channels and a RUN of consecutive positions and keeps the twelve s values of
// the current output in registers: a step computes two new ones (from a rolling window of six x) and shifts.  Only the first
// output of a run pays for ten more; runs are as long as the launch's parallelism allows.
#include "hifigan_tile.hpp"

namespace {

constexpr int BV_MAX_C = 1536, BV_TAPS = 12;

struct BvAct {
  const float* alpha;  // [C]
  const float* invb;   // [C]: 1 / (beta + 1e-9), or 1 / (alpha + 1e-9) for snake
  const float* fu;     // [12]
  const float* fd;     // [12]
};

struct BvFilt {
  float fu[BV_TAPS], fd[BV_TAPS];
};

VBX_DEV BvFilt bv_filters(const BvAct& a) {
  BvFilt f;
#pragma unroll
  for (int i = 0; i < BV_TAPS; i++) f.fu[i] = a.fu[i], f.fd[i] = a.fd[i];
  return f;
}

// s[m] from the six x values it reads, xw[q] = x[clamp(i_lo + q)], i_lo = floor((m - 5) / 2): the tap of xw[q] is f_u[m + 5 - 2 (i_lo + q)]
// = f_u[11 - 2 q] for even m, f_u[10 - 2 q] for odd m
VBX_DEV float bv_s(const float xw[6], bool odd, const BvFilt& f, float alpha, float invb) {
#pragma clang fp contract(off)
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < 6; q++) acc = fmaf(odd ? f.fu[10 - 2 * q] : f.fu[11 - 2 * q], xw[q], acc);
  const float u = 2.0f * acc;
  const float a = alpha * u;
  const float sn = sinf(a);
  const float sq = sn * sn;
  return fmaf(invb, sq, u);
}

VBX_DEV float bv_y(const float S[BV_TAPS], const BvFilt& f) {
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < BV_TAPS; t++) acc = fmaf(f.fd[t], S[t], acc);
  return acc;
}

// channels c, c + 1 of position clamp(i, 0, L - 1) of one batch row (rowoff: the row's element offset + c): the mean of the inputs
VBX_DEV void bv_x2(const HgIn& in, long rowoff, int C, int L, int i, float& a, float& b) {
  const long off = rowoff + (long)(i < 0 ? 0 : (i >= L ? L - 1 : i)) * C;
  const unsigned v0 = *reinterpret_cast<const unsigned*>(in.x[0] + off);
  const unsigned v1 = in.n > 1 ? *reinterpret_cast<const unsigned*>(in.x[1] + off) : 0u;
  const unsigned v2 = in.n > 2 ? *reinterpret_cast<const unsigned*>(in.x[2] + off) : 0u;
  a = hg_mean(f16_to_f32((u16)(v0 & 0xFFFFu)), f16_to_f32((u16)(v1 & 0xFFFFu)), f16_to_f32((u16)(v2 & 0xFFFFu)), in.n);
  b = hg_mean(f16_to_f32((u16)(v0 >> 16)), f16_to_f32((u16)(v1 >> 16)), f16_to_f32((u16)(v2 >> 16)), in.n);
}

// A(x)[t] for t = ta .. tb - 1 (0 <= ta < tb <= L) and the channels c, c + 1: emit(t, y0, y1) is handed the fp32 results
template <class Emit>
VBX_DEV void bv_run(const HgIn& in, long rowoff, int C, int L, int ta, int tb, const BvFilt& f, const float al[2], const float ib[2],
                    const Emit& emit) {
  float S[2][BV_TAPS], X[2][6];
  const int last = 2 * L - 1;
  // the ten values s[clamp(2 ta - 5 + idx)], idx = 0 .. 9, from memory
  for (int idx = 0; idx < 10; idx++) {
    int m = 2 * ta - 5 + idx;
    m = m < 0 ? 0 : (m > last ? last : m);
    const int ilo = (m - 5) >> 1;
    float xw[2][6];
#pragma unroll
    for (int q = 0; q < 6; q++) bv_x2(in, rowoff, C, L, ilo + q, xw[0][q], xw[1][q]);
    const float s0 = bv_s(xw[0], m & 1, f, al[0], ib[0]), s1 = bv_s(xw[1], m & 1, f, al[1], ib[1]);
#pragma unroll
    for (int j = 0; j < 10; j++)
      if (j == idx) S[0][j] = s0, S[1][j] = s1;  // a register array: no dynamic index
  }
#pragma unroll
  for (int q = 0; q < 5; q++) bv_x2(in, rowoff, C, L, ta + q, X[0][q], X[1][q]);
  for (int t = ta; t < tb; t++) {
    bv_x2(in, rowoff, C, L, t + 5, X[0][5], X[1][5]);
    const bool in1 = 2 * t + 5 <= last, in2 = 2 * t + 6 <= last;  // past the row: s is clamped, the value before is repeated
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
      S[ch][10] = in1 ? bv_s(X[ch], true, f, al[ch], ib[ch]) : S[ch][9];
      S[ch][11] = in2 ? bv_s(X[ch], false, f, al[ch], ib[ch]) : S[ch][10];
    }
    emit(t, bv_y(S[0], f), bv_y(S[1], f));
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
#pragma unroll
      for (int j = 0; j < 10; j++) S[ch][j] = S[ch][j + 2];
#pragma unroll
      for (int q = 0; q < 5; q++) X[ch][q] = X[ch][q + 1];
    }
  }
}

// ---- the stand-alone activation: a work item is (run of R positions, channel pair); neighbouring threads take neighbouring pairs
__global__ __launch_bounds__(256) void bigvgan_act_kernel(HgIn in, BvAct a, u16* __restrict__ y, int L, int C, int R) {
  const BvFilt f = bv_filters(a);
  const int pairs = C >> 1, b = blockIdx.y;
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  const int run = (int)(item / pairs), c = (int)(item - (long)run * pairs) * 2;
  const int ta = run * R;
  if (ta >= L) return;
  const int tb = ta + R < L ? ta + R : L;
  const float al[2] = {a.alpha[c], a.alpha[c + 1]}, ib[2] = {a.invb[c], a.invb[c + 1]};
  const long rowoff = (long)b * L * C + c;
  bv_run(in, rowoff, C, L, ta, tb, f, al, ib,
         [&](int t, float y0, float y1) __attribute__((always_inline)) { *reinterpret_cast<unsigned*>(y + rowoff + (long)t * C) = pack_f16x2(y0, y1); });
}

// `rows` LDS rows (stride ld, u16) of channels c0 .. c0 + cw - 1 from positions i0, i0 + 1, ... of one batch row: fp16(A(x)) inside
// [0, L), ZEROS outside (the convolution's padding; A's own clamps stop at the row ends).  The valid positions are cut into as many
// runs as give every thread an item.
VBX_DEV void bv_stage_span(u16* s, int ld, const HgIn& in, long rowoff, int C, int c0, int cw, int i0, int rows, int L, const BvAct& a,
                           const BvFilt& f) {
  const int ia = i0 < 0 ? 0 : i0, ib_ = i0 + rows < L ? i0 + rows : L;
  const int pairs = cw >> 1;
  for (int e = threadIdx.x; e < rows * pairs; e += 256) {  // the padding rows
    const int pos = e / pairs, c = (e - pos * pairs) * 2;
    const int i = i0 + pos;
    if (i < 0 || i >= L) *reinterpret_cast<unsigned*>(s + pos * ld + c) = 0u;
  }
  if (ib_ <= ia) return;
  const int want = pairs >= 256 ? 1 : 256 / pairs;
  int R = (ib_ - ia + want - 1) / want;
  R = R < 8 ? 8 : R;
  const int runs = (ib_ - ia + R - 1) / R;
  for (int e = threadIdx.x; e < runs * pairs; e += 256) {
    const int run = e / pairs, c = (e - run * pairs) * 2;
    const int ta = ia + run * R, tb = ta + R < ib_ ? ta + R : ib_;
    const float al[2] = {a.alpha[c0 + c], a.alpha[c0 + c + 1]}, ib[2] = {a.invb[c0 + c], a.invb[c0 + c + 1]};
    bv_run(in, rowoff + c0 + c, C, L, ta, tb, f, al, ib, [&](int t, float y0, float y1) __attribute__((always_inline)) {
      *reinterpret_cast<unsigned*>(s + (t - i0) * ld + c) = pack_f16x2(y0, y1);
    });
  }
}

struct BvConv {
  HgConv c;
  BvAct a;
};

// vbx_hifigan_conv's kernel with A computed while the span is staged
template <int MG>
__global__ __launch_bounds__(256) void bigvgan_conv_kernel(BvConv q) {
  extern __shared__ __attribute__((aligned(16))) u16 hg_lds[];
  const HgConv& p = q.c;
  const int b = blockIdx.y, t0 = blockIdx.x * p.TT;
  HgIn in;
  in.x[0] = p.x, in.x[1] = in.x[2] = nullptr, in.n = 1;
  const BvFilt f = bv_filters(q.a);
  bv_stage_span(hg_lds, p.C + SN_PADH, in, (long)b * p.L * p.C, p.C, 0, p.C, t0 - p.pad, p.TT + (p.k - 1) * p.dil, p.L, q.a, f);
  __syncthreads();
  hg_conv_product<MG>(p, hg_lds, b, t0);
}

// conv_post on fp16(A(mean of the inputs)): vbx_hifigan_post's kernel (the same staging shape, the same fmaf chain) with the operand
// staged as fp16 in the LDS; bias NULL is zero; final 0: tanhf, 1: a clamp to [-1, 1]
constexpr int BV_POST_CH = 32, BV_POST_LD = BV_POST_CH + 2;  // u16 rows of 34: an odd number of words

__global__ __launch_bounds__(256) void bigvgan_post_kernel(HgIn in, BvAct a, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, int T, int C, int k, int final) {
  extern __shared__ __attribute__((aligned(16))) float bv_sw[];  // [k][C] weights, then u16 [256 + k - 1][34] operands
  u16* sx = reinterpret_cast<u16*>(bv_sw + k * C);
  const BvFilt f = bv_filters(a);
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k * C; e += 256) bv_sw[e] = w[e];
  const long p0 = (long)blockIdx.x * 256, pos = p0 + tid;
  const int rows = 256 + k - 1;
  float acc = bias ? bias[0] : 0.f;
  for (int c0 = 0; c0 < C; c0 += BV_POST_CH) {
    const int cw = C - c0 < BV_POST_CH ? C - c0 : BV_POST_CH;
    __syncthreads();  // the chunk before is consumed
    bv_stage_span(sx, BV_POST_LD, in, (long)b * T * C, C, c0, cw, (int)(p0 - (k >> 1)), rows, T, a, f);
    __syncthreads();
    for (int tap = 0; tap < k; tap++)
      for (int c = 0; c < cw; c++) acc = fmaf(bv_sw[tap * C + c0 + c], f16_to_f32(sx[(tid + tap) * BV_POST_LD + c]), acc);
  }
  if (pos < T) y[(long)b * T + pos] = final ? fminf(fmaxf(acc, -1.0f), 1.0f) : tanhf(acc);
}

int bv_act_check(const char* who, BvAct& a, const float* alpha, const float* inv_beta, const float* f_u, const float* f_d) {
  VBX_REQUIRE(alpha && inv_beta && f_u && f_d, "%s: null activation operand (alpha, inv_beta, f_u, f_d)", who);
  a.alpha = alpha, a.invb = inv_beta, a.fu = f_u, a.fd = f_d;
  return 0;
}

}  // namespace

extern "C" int vbx_bigvgan_act(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* alpha,
                               const float* inv_beta, const float* f_u, const float* f_d, void* y_f16, int B, int L, int C, void* stream) {
  HgIn in;
  BvAct a;
  if (int rc = hg_in(in, x0_f16, x1_f16, x2_f16, inputs, "vbx_bigvgan_act")) return rc;
  if (int rc = bv_act_check("vbx_bigvgan_act", a, alpha, inv_beta, f_u, f_d)) return rc;
  VBX_REQUIRE(y_f16 && B >= 1 && B <= 65535 && L >= 1 && L < (1 << 29), "vbx_bigvgan_act: need B in 1 .. 65535, L in 1 .. 2^29 - 1");
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= BV_MAX_C, "vbx_bigvgan_act: C must be a multiple of 8 in 8 .. %d (got %d)", BV_MAX_C, C);
  int R = 32;  // positions per run: shorter while the launch has fewer items than the device has lanes to fill
  while (R > 8 && (long)cdiv(L, R) * (C / 2) * B < 256L * 1024) R >>= 1;
  const long blocks = ((long)cdiv(L, R) * (C / 2) + 255) / 256;
  VBX_REQUIRE(blocks < (1L << 31), "vbx_bigvgan_act: row too long");
  hipLaunchKernelGGL(bigvgan_act_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, in, a, (u16*)y_f16, L, C, R);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_bigvgan_conv_tile(int C, int k, int dilation) {
  if (int rc = hg_conv_check("vbx_bigvgan_conv", C, k, dilation)) return rc;
  const int TT = hg_conv_tile(C, k, dilation);  // the activation's window lives in registers: no scratch beside the span
  if (!TT) {
    vbx_set_error("vbx_bigvgan_conv: 16 output positions of this convolution do not fit the LDS");
    return VBX_EINVAL;
  }
  return TT;
}

extern "C" int vbx_bigvgan_conv(const void* x_f16, const float* alpha, const float* inv_beta, const float* f_u, const float* f_d,
                                const void* w_f16, const float* bias, const void* res_f16, void* y_f16, int B, int L, int C, int Co, int k,
                                int dilation, void* stream) {
  BvConv q;
  if (int rc = bv_act_check("vbx_bigvgan_conv", q.a, alpha, inv_beta, f_u, f_d)) return rc;
  if (int rc = hg_conv_setup("vbx_bigvgan_conv", q.c, x_f16, w_f16, bias, res_f16, y_f16, B, L, C, Co, k, dilation)) return rc;
  const int TT = q.c.TT;
  const size_t bytes = hg_conv_lds(TT, C, k, dilation);
  const int MG = sn_blocks_per_item((Co + 15) / 16, TT / 16), blocks = cdiv(L, TT);
  if (MG == 4) return sn_launch<bigvgan_conv_kernel<4>>("vbx_bigvgan_conv", q, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<bigvgan_conv_kernel<2>>("vbx_bigvgan_conv", q, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<bigvgan_conv_kernel<1>>("vbx_bigvgan_conv", q, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_bigvgan_convtr(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const void* w_f16,
                                  const float* bias, void* y_f16, int B, int L, int C, int stride, void* stream) {
  return hg_convtr_launch("vbx_bigvgan_convtr", BV_MAX_C, x0_f16, x1_f16, x2_f16, inputs, w_f16, bias, y_f16, B, L, C, stride, 1.0f, stream);
}

extern "C" int vbx_bigvgan_post(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* alpha,
                                const float* inv_beta, const float* f_u, const float* f_d, const float* w, const float* bias, float* y, int B,
                                int T, int C, int k, int final, void* stream) {
  HgIn in;
  BvAct a;
  if (int rc = hg_in(in, x0_f16, x1_f16, x2_f16, inputs, "vbx_bigvgan_post")) return rc;
  if (int rc = bv_act_check("vbx_bigvgan_post", a, alpha, inv_beta, f_u, f_d)) return rc;
  VBX_REQUIRE(w && y && B >= 1 && B <= 65535 && T >= 1 && T < (1 << 29), "vbx_bigvgan_post: need B in 1 .. 65535, T in 1 .. 2^29 - 1");
  VBX_REQUIRE(C >= 8 && C % 8 == 0 && C <= HG_POST_MAX_C, "vbx_bigvgan_post: C must be a multiple of 8 up to %d (got %d)", HG_POST_MAX_C, C);
  VBX_REQUIRE(k >= 1 && k <= HG_MAX_K && (k & 1), "vbx_bigvgan_post: the kernel must be odd, at most %d (got %d)", HG_MAX_K, k);
  VBX_REQUIRE(final == 0 || final == 1, "vbx_bigvgan_post: final is 0 (tanh) or 1 (clamp), got %d", final);
  const size_t bytes = (size_t)k * C * sizeof(float) + (size_t)(256 + k - 1) * BV_POST_LD * sizeof(u16);
  hipLaunchKernelGGL(bigvgan_post_kernel, dim3(cdiv(T, 256), B), dim3(256), bytes, (hipStream_t)stream, in, a, w, bias, y, T, C, k, final);
  VBX_LAUNCH_CHECK();
  return 0;
}
