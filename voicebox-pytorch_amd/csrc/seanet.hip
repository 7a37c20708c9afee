// SEANetEncoder (voicebox-pytorch_amd/seanet.py): EnCodec's encoder (Defossez et al. 2022, "High fidelity neural audio compression":
// a stack of reflect-padded convolutions with ELU, four strided downsampling stages, a 2-layer LSTM with a skip, a final
// convolution) on the device, inference only.  The launch sequence of one encode at the published 24 kHz widths:
//
//   vbx_seanet_conv0   wave fp32 [B, T] -> fp16 [B, T, nf]: the 1 -> nf first convolution, fp32 weights, plain VALU
//   per stage:
//     vbx_seanet_conv  ELU, k 3 (dilated), d -> d / 2
//     vbx_seanet_conv  [ELU(h) | x] . [W_1x1 | W_shortcut]^T + (b_1x1 + b_shortcut): the block's tail and its shortcut in ONE product
//     vbx_seanet_conv  ELU, k 2r, stride r, d -> 2d
//   vbx_gemm           NT, VBX_EPI_F32: x . W_ih0^T + (b_ih0 + b_hh0) for all steps
//   vbx_lstm           T + layers - 1 launches of the step kernel (layer 1 runs one step behind layer 0), skip add in the epilogue
//   vbx_seanet_conv    ELU, k 7, fp32 output [B, frames, dimension]
//
// Precision contract (include/vbx.h): activations fp16 channel-last, rounded once, stored BEFORE the ELU (the shortcut reads them
// un-activated; ELU is applied in fp32 when an operand is staged and the result rounded to fp16 as the MFMA operand); weights
// fp16; every sum fp32 on v_mfma_f32_16x16x32_f16.  SConv1d's reflect padding, its `extra` right padding and pad1d's short-input
// rule (append zeros, reflect, cut) are resolved when a workgroup stages its input span: it reads its own batch row only, inside
// [0, L).  Plain launches, no atomics, no workgroup waits for another: the same bits on every run, and a batch row's result does
// not depend on its neighbours.
//
// SEANetDecoder (the same file's `decoder.*`), under the same contract; the launch sequence of one decode:
//
//   vbx_seanet_pack_latents  z fp32 [B, D, frames] channel-first -> fp16 [B, frames, D], rounded once
//   vbx_seanet_conv          k 7, D -> 16 nf;  vbx_gemm + vbx_lstm as above
//   per stage (ratio r):
//     vbx_seanet_convtr      ELU, transposed convolution k 2r, stride r, d -> d / 2: ONE product over rows [a_j | a_{j-1}], j = 0 .. L
//     vbx_seanet_conv x 2    the Resnet block as in the encoder
//   vbx_seanet_conv_out      ELU (fp32, not rounded again), k 7, nf -> 1, fp32 weights, plain VALU: the wave fp32 [B, frames * hop]
//
// Causal mode (CausalSEANetEncoder / CausalSEANetDecoder: the published 24 kHz model) runs the same launches through the entry points
// that carry the side: vbx_seanet_conv_c / _conv0_c / _conv_out_c (causal: all of padding_total on the left) and vbx_seanet_convtr_t
// (trim_left: how much of padding_total is cut in front).  Only sn_pads and SnConvTr::left differ; the products do not.
#include "seanet_tile.hpp"  // the tile core shared with hifigan.hip: sn_tile_product, sn_pick_tile, sn_blocks_per_item, sn_launch

namespace {

constexpr int SN_MAX_K = 16, SN_MAX_STRIDE = 8, SN_MAX_DIL = 4, SN_MAX_C = 1024;

struct SnConv {
  const u16* x1;      // [B, L, C1]
  const u16* x2;      // [B, L, C2] or NULL: K-concatenated behind x1's k * C1 columns (k = 1, stride = 1), never activated
  const u16* w;       // [Co, Ktot], column tap * C1 + c, then C2 columns
  const float* bias;  // [Co]
  void* y;            // [B, Lout, Co] fp16 or fp32
  int L, Lout, C1, C2, Co, k, stride, dil, pad_left, Lz, elu1, out_f32, TT, Ktot;
  const int* lens;    // [B] or NULL (the LENS instantiations only): the rows' own input lengths, see "ragged waves" in include/vbx.h
  int causal;
};

VBX_DEV float sn_elu(float x) { return x > 0.f ? x : expm1f(x); }

VBX_DEV uint4 sn_elu8(uint4 v) {
  unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++)
    w[i] = pack_f16x2(sn_elu(f16_to_f32((u16)(w[i] & 0xFFFFu))), sn_elu(f16_to_f32((u16)(w[i] >> 16))));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// padded position q (0 = the first sample of the left padding) -> index into the row, or -1 for one of pad1d's appended zeros.
// Lz = max(L, max(pad_left, pad_right + extra) + 1) is the length pad1d reflects about; one reflection per side suffices:
// both paddings are at most Lz - 1, so the left one mirrors into [1, Lz - 1] and the right one into [0, Lz - 2] -- in the causal
// form (pad_left = padding_total, pad_right = 0) as in the non-causal one.
VBX_DEV int sn_src(int q, int pad_left, int L, int Lz) {
  int i = q - pad_left;
  if (i < 0) i = -i;
  if (i >= Lz) i = 2 * (Lz - 1) - i;
  return i < L ? i : -1;
}

// SConv1d's padding: (k_eff - stride) split with the larger half on the left -- causal: all of it on the left --, `extra` on the
// right so that the last window is whole; Lz is the length pad1d reflects about (sn_src)
struct SnPads { int left, Lz; };
__host__ __device__ inline SnPads sn_pads(int k, int stride, int dil, int L, int Lout, int causal) {
  const int total = (k - 1) * dil + 1 - stride, extra = Lout * stride - L;
  const int right = causal ? 0 : total / 2, left = total - right, maxpad = left > right + extra ? left : right + extra;
  return SnPads{left, L > maxpad ? L : maxpad + 1};
}

// LENS (vbx_seanet_conv_lens): L, Lout, Lz are the row's own, by the arithmetic of sn_pads from lens[b]; p.L / p.Lout stay the
// pitches of the buffers.  The row is read below its length only and positions from its Lout on are stored as zeros.
// A workgroup owns TT consecutive output positions of one batch row and all Co channels: it stages the input span ((TT - 1) * stride
// + k_eff positions, channel-last, padding resolved, ELU applied) and the second input's TT positions, then runs the product.
template <int MG, bool LENS = false>
__global__ __launch_bounds__(256) void seanet_conv_kernel(SnConv p) {
  extern __shared__ __attribute__((aligned(16))) u16 sn_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * p.TT;
  int L = p.L, Lout = p.Lout, Lz = p.Lz;
  if (LENS) {
    const int l = p.lens[b];
    L = l < 1 ? 1 : (l > p.L ? p.L : l);
    Lout = (L + p.stride - 1) / p.stride;
    Lz = sn_pads(p.k, p.stride, p.dil, L, Lout, p.causal).Lz;
    if (t0 >= Lout) {  // a tile wholly behind the row
      const int n = (p.Lout - t0 < p.TT ? p.Lout - t0 : p.TT) * p.Co;
      const long o = ((long)b * p.Lout + t0) * p.Co;
      const int esz = p.out_f32 ? 4 : 2;
      if ((p.Co * esz) % 16 == 0 && (reinterpret_cast<size_t>(p.y) & 15) == 0) {  // whole 16-byte pieces from an aligned start
        uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<char*>(p.y) + o * esz);
        for (int e = tid; e < n * esz / 16; e += 256) dst[e] = make_uint4(0u, 0u, 0u, 0u);
      } else {
        for (int e = tid; e < n; e += 256) {
          if (p.out_f32) reinterpret_cast<float*>(p.y)[o + e] = 0.f;
          else reinterpret_cast<u16*>(p.y)[o + e] = 0;
        }
      }
      return;
    }
  }
  const int ld1 = p.C1 + SN_PADH, ld2 = p.C2 + SN_PADH;
  const int keff = (p.k - 1) * p.dil + 1;
  const int span = (p.TT - 1) * p.stride + keff;
  u16* s1 = sn_lds;
  u16* s2 = sn_lds + span * ld1;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  {
    const int c8 = p.C1 >> 3;
    const u16* xb = p.x1 + (long)b * p.L * p.C1;
    const int padded = (Lout - 1) * p.stride + keff;  // = L + padding_total + extra
    for (int e = tid; e < span * c8; e += 256) {
      const int pos = e / c8, c = (e - pos * c8) * 8;
      const int q = t0 * p.stride + pos;
      uint4 v = zero;
      if (q < padded) {
        const int i = sn_src(q, p.pad_left, L, Lz);
        if (i >= 0) {
          v = *reinterpret_cast<const uint4*>(xb + (long)i * p.C1 + c);
          if (p.elu1) v = sn_elu8(v);
        }
      }
      *reinterpret_cast<uint4*>(s1 + pos * ld1 + c) = v;
    }
  }
  if (p.C2) {
    const int c8 = p.C2 >> 3;
    const u16* xb = p.x2 + (long)b * p.L * p.C2;
    for (int e = tid; e < p.TT * c8; e += 256) {
      const int pos = e / c8, c = (e - pos * c8) * 8;
      const int t = t0 + pos;
      *reinterpret_cast<uint4*>(s2 + pos * ld2 + c) = t < L ? *reinterpret_cast<const uint4*>(xb + (long)t * p.C2 + c) : zero;
    }
  }
  __syncthreads();
  // row m of the A operand: the k runs of C1 channels at positions m * stride + tap * dil of the span, then x2's C2 channels at
  // position m.  C1, C2 are multiples of 8: the eight columns lie in one tap of one input.
  const int K1 = p.k * p.C1;
  auto rows = [&](int kk, const u16*& base, int& ld) __attribute__((always_inline)) {
    if (kk < K1) {
      const int tap = kk / p.C1, c = kk - tap * p.C1;
      base = s1 + tap * p.dil * ld1 + c, ld = p.stride * ld1;
    } else {
      base = s2 + (kk - K1), ld = ld2;
    }
  };
  auto store = [&](int n) __attribute__((always_inline)) {
    return [&, n, bv = p.bias[n]](int m, float v) __attribute__((always_inline)) {
      const int t = t0 + m;
      if (t >= p.Lout) return;
      const long o = ((long)b * p.Lout + t) * p.Co + n;
      if (LENS && t >= Lout) {
        if (p.out_f32) reinterpret_cast<float*>(p.y)[o] = 0.f;
        else reinterpret_cast<u16*>(p.y)[o] = 0;
        return;
      }
      if (p.out_f32) reinterpret_cast<float*>(p.y)[o] = v + bv;
      else reinterpret_cast<u16*>(p.y)[o] = f32_to_f16(v + bv);
    };
  };
  sn_tile_product<MG, true>(p.w, p.Co, p.Ktot, p.TT >> 4, rows, store);
}

// the first convolution: one thread per (position, eight output channels), the k taps as an fmaf chain on the bias in tap order
template <bool LENS>
__global__ __launch_bounds__(256) void seanet_conv0_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, u16* __restrict__ y, int T, int nf, int k,
                                                           int pad_left, int Lz, const int* __restrict__ lens, int causal) {
  __shared__ float sw[SN_MAX_K * 64 + 64];  // [k][nf] taps, then the bias
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k * nf; e += 256) {
    const int tap = e / nf, c = e - tap * nf;
    sw[e] = w[c * k + tap];
  }
  for (int e = tid; e < nf; e += 256) sw[k * nf + e] = bias[e];
  __syncthreads();
  const int groups = nf >> 3;
  const long e = (long)blockIdx.x * 256 + tid;
  if (e >= (long)T * groups) return;
  const int pos = (int)(e / groups), c0 = (int)(e - (long)pos * groups) * 8;
  const float* xb = x + (long)b * T;
  int Tb = T;
  if (LENS) {  // the row's own length and the length its padding reflects about; past it the row is stored as zeros
    const int l = lens[b];
    Tb = l < 1 ? 1 : (l > T ? T : l);
    Lz = sn_pads(k, 1, 1, Tb, Tb, causal).Lz;
    if (pos >= Tb) {
      *reinterpret_cast<uint4*>(y + ((long)b * T + pos) * nf + c0) = make_uint4(0u, 0u, 0u, 0u);
      return;
    }
  }
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = sw[k * nf + c0 + j];
  for (int tap = 0; tap < k; tap++) {
    const int i = sn_src(pos + tap, pad_left, Tb, Lz);
    const float xv = i >= 0 ? xb[i] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(sw[tap * nf + c0 + j], xv, acc[j]);
  }
  *reinterpret_cast<uint4*>(y + ((long)b * T + pos) * nf + c0) =
      make_uint4(pack_f16x2(acc[0], acc[1]), pack_f16x2(acc[2], acc[3]), pack_f16x2(acc[4], acc[5]), pack_f16x2(acc[6], acc[7]));
}

struct SnLstm {
  const float* xproj;  // [B * T, 4H] = x . W_ih0^T + b_ih0 + b_hh0
  const u16* w0;       // [4H, H]  W_hh0
  const u16* w1;       // [4H, 2H] [W_ih1 | W_hh1]
  const float* bias1;  // [4H] b_ih1 + b_hh1
  u16 *h0, *h1;        // [B, T, H] every step's h as the next product's operand (step t reads row t - 1 and writes row t)
  float* c;            // [layers, B, H]
  const u16* x;        // [B, T, H] the LSTM's input, for the skip
  u16* y16;            // [B, T, H] h_last + x, rounded once
  float* y32;          // the same before the rounding, or NULL
  int B, T, H, layers, s;
};

VBX_DEV float sn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One time step: workgroup (u, layer, m) owns hidden units [16u, 16u + 16) of `layer` at time t = s - layer for batch rows
// [16m, 16m + 16), all four gates (rows j, H + j, 2H + j, 3H + j of the weight), so the cell update needs nothing from another
// workgroup.  The four waves split K; wave w then finishes accumulator register w (batch row 16m + 4 (lane / 16) + w).
// What a step reads (h0 row t - 1 resp. h0 row t and h1 row t - 1 for layer 1) was written by EARLIER launches only.
__global__ __launch_bounds__(256) void seanet_lstm_step_kernel(SnLstm p) {
  __shared__ float red[4][4][4][64];  // [wave][gate][register][lane]
  const int layer = blockIdx.y, t = p.s - layer;
  if (t < 0 || t >= p.T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * 16, b0 = blockIdx.z * 16;
  const int H = p.H, K = layer ? 2 * H : H;
  const u16* w = layer ? p.w1 : p.w0;
  const int brow = b0 + fr;
  const bool bvalid = brow < p.B;
  const f16x8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the zero initial state: layer 0 at t = 0 has no product at all, layer 1 at t = 0 only its input half
  const int ksteps = (layer ? (t > 0 ? K : H) : (t > 0 ? K : 0)) >> 5;
  for (int ks = wave; ks < ksteps; ks += 4) {
    const int kk = ks * 32 + g * 8;
    f16x8 a = hz;
    if (bvalid) {
      if (layer == 0) a = *reinterpret_cast<const f16x8*>(p.h0 + ((long)brow * p.T + t - 1) * H + kk);
      else if (kk < H) a = *reinterpret_cast<const f16x8*>(p.h0 + ((long)brow * p.T + t) * H + kk);
      else a = *reinterpret_cast<const f16x8*>(p.h1 + ((long)brow * p.T + t - 1) * H + kk - H);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const f16x8 bf = *reinterpret_cast<const f16x8*>(w + (long)(q * H + u0 + fr) * K + kk);
      acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bf, acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int r = 0; r < 4; r++) red[wave][q][r][lane] = acc[q][r];
  __syncthreads();
  const int bb = b0 + g * 4 + wave, j = u0 + fr;
  if (bb >= p.B) return;
  float pre[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float sum = ((red[0][q][wave][lane] + red[1][q][wave][lane]) + red[2][q][wave][lane]) + red[3][q][wave][lane];
    pre[q] = sum + (layer ? p.bias1[q * H + j] : p.xproj[((long)bb * p.T + t) * 4 * H + q * H + j]);
  }
  const float ig = sn_sigmoid(pre[0]), fg = sn_sigmoid(pre[1]), gg = tanhf(pre[2]), og = sn_sigmoid(pre[3]);
  const long ci = ((long)layer * p.B + bb) * H + j;
  const float cn = fmaf(fg, t > 0 ? p.c[ci] : 0.f, ig * gg);
  p.c[ci] = cn;
  const float h = og * tanhf(cn);
  const long o = ((long)bb * p.T + t) * H + j;
  (layer ? p.h1 : p.h0)[o] = f32_to_f16(h);
  if (layer == p.layers - 1) {
    const float yv = h + f16_to_f32(p.x[o]);
    p.y16[o] = f32_to_f16(yv);
    if (p.y32) p.y32[o] = yv;
  }
}

// ---------------------------------------------------------------------------------------------------- SEANetDecoder
// EnCodec's decoder (voicebox-pytorch_amd/seanet.py: SEANetDecoder) runs vbx_seanet_pack_latents, vbx_seanet_conv (first convolution
// and the Resnet blocks, as in the encoder), vbx_gemm + vbx_lstm, per stage vbx_seanet_convtr, and vbx_seanet_conv_out.

struct SnConvTr {
  const u16* x;       // [B, L, C], activated with ELU as it is staged
  const u16* w;       // [r * Co, 2C]: row p * Co + o = [W[:, o, p] | W[:, o, p + r]]
  const float* bias;  // [Co]
  u16* y;             // [B, L * r, Co]
  int L, C, Co, r, left, TT, N, Ktot;
};

// SConvTranspose1d with k = 2 r (`left` samples trimmed in front: r - r / 2 non-causal, r - ceil(r * trim_right_ratio) causal) as
// ONE product over rows j = 0 .. L: the operand row is [a_j | a_{j-1}] (a = ELU(x),
// a_{-1} = a_L = 0), its N = r * Co results are the contiguous run of r output positions from trimmed position j * r - left on.  A
// workgroup owns TT consecutive rows j of one batch row: positions j0 - 1 .. j0 + TT - 1 sit in the LDS (LDS row m holds position
// j0 - 1 + m), and row m of the A operand reads LDS row m + 1 for its first C columns and LDS row m for the other C, in place (C is
// a multiple of 16: the eight columns lie in one of the two halves).  Column n is phase n / Co of channel
// n % Co; row 0 drops its phases below `left`, row L keeps only those (none at left = 0: the host then launches rows 0 .. L - 1):
// every output element is written by exactly one lane of one workgroup.
template <int MG>
__global__ __launch_bounds__(256) void seanet_convtr_kernel(SnConvTr p) {
  extern __shared__ __attribute__((aligned(16))) u16 sn_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, j0 = blockIdx.x * p.TT;
  const int ld = p.C + SN_PADH;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  {
    const int c8 = p.C >> 3;
    const u16* xb = p.x + (long)b * p.L * p.C;
    for (int e = tid; e < (p.TT + 1) * c8; e += 256) {
      const int pos = e / c8, c = (e - pos * c8) * 8;
      const int i = j0 - 1 + pos;
      uint4 v = zero;
      if (i >= 0 && i < p.L) v = sn_elu8(*reinterpret_cast<const uint4*>(xb + (long)i * p.C + c));
      *reinterpret_cast<uint4*>(sn_lds + pos * ld + c) = v;
    }
  }
  __syncthreads();
  auto rows = [&](int kk, const u16*& base, int& ldr) __attribute__((always_inline)) {
    base = kk < p.C ? sn_lds + ld + kk : sn_lds + (kk - p.C), ldr = ld;
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

// the last convolution, nf -> 1: one thread per output sample, the k * nf products as ONE fmaf chain on the bias, tap-major then
// channel; ELU in fp32 on the stored fp16 value, not rounded again
__global__ __launch_bounds__(256) void seanet_conv_out_kernel(const u16* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y, int T, int nf, int k,
                                                              int pad_left, int Lz) {
  __shared__ float sw[7 * 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int e = tid; e < k * nf; e += 256) sw[e] = w[e];
  __syncthreads();
  const long pos = (long)blockIdx.x * 256 + tid;
  if (pos >= T) return;
  const u16* xb = x + (long)b * T * nf;
  float acc = bias[0];
  for (int tap = 0; tap < k; tap++) {
    const int i = sn_src((int)pos + tap, pad_left, T, Lz);
    if (i < 0) continue;  // one of pad1d's appended zeros: ELU(0) = 0 adds nothing
    for (int c = 0; c < nf; c += 8) {
      const uint4 v = *reinterpret_cast<const uint4*>(xb + (long)i * nf + c);
      const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int h = 0; h < 4; h++) {
        acc = fmaf(sw[tap * nf + c + 2 * h], sn_elu(f16_to_f32((u16)(u[h] & 0xFFFFu))), acc);
        acc = fmaf(sw[tap * nf + c + 2 * h + 1], sn_elu(f16_to_f32((u16)(u[h] >> 16))), acc);
      }
    }
  }
  y[(long)b * T + pos] = acc;
}

// latents fp32 [B, D, T] channel-first -> fp16 [B, T, D] channel-last, rounded once: a 32 x 32 tile through the LDS
__global__ __launch_bounds__(256) void seanet_pack_latents_kernel(const float* __restrict__ z, u16* __restrict__ y, int D, int T) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int d = d0 + r, t = t0 + tx;
    tile[r][tx] = (d < D && t < T) ? z[((long)b * D + d) * T + t] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int t = t0 + r, d = d0 + tx;
    if (t < T && d < D) y[((long)b * T + t) * D + d] = f32_to_f16(tile[tx][r]);
  }
}

int sn_convtr_check(int C, int stride) {
  VBX_REQUIRE(C >= 16 && C % 16 == 0 && C <= SN_MAX_C, "vbx_seanet_convtr: C must be a multiple of 16 in 16 .. %d (got %d)", SN_MAX_C, C);
  VBX_REQUIRE(stride >= 2 && stride <= SN_MAX_STRIDE, "vbx_seanet_convtr: stride must be in 2 .. %d (got %d)", SN_MAX_STRIDE, stride);
  return 0;
}

int sn_conv_check(int C1, int C2, int k, int stride, int dil) {
  VBX_REQUIRE(C1 >= 8 && C1 % 8 == 0 && C1 <= SN_MAX_C, "vbx_seanet_conv: C1 must be a multiple of 8 in 8 .. %d (got %d)", SN_MAX_C, C1);
  VBX_REQUIRE(C2 >= 0 && C2 % 8 == 0 && C2 <= SN_MAX_C, "vbx_seanet_conv: C2 must be 0 or a multiple of 8 up to %d (got %d)", SN_MAX_C, C2);
  VBX_REQUIRE(k >= 1 && k <= SN_MAX_K && stride >= 1 && stride <= SN_MAX_STRIDE && dil >= 1 && dil <= SN_MAX_DIL,
              "vbx_seanet_conv: need k in 1 .. %d, stride in 1 .. %d, dilation in 1 .. %d", SN_MAX_K, SN_MAX_STRIDE, SN_MAX_DIL);
  VBX_REQUIRE((k - 1) * dil + 1 >= stride, "vbx_seanet_conv: the kernel must span its stride");
  VBX_REQUIRE(!C2 || (k == 1 && stride == 1), "vbx_seanet_conv: a second input needs k = 1, stride = 1");
  return 0;
}

size_t sn_convtr_lds(int TT, int C) { return (size_t)(TT + 1) * (C + SN_PADH) * sizeof(u16); }

size_t sn_conv_lds(int TT, int C1, int C2, int k, int stride, int dil) {
  const size_t span = (size_t)(TT - 1) * stride + (k - 1) * dil + 1;
  return (span * (C1 + SN_PADH) + (C2 ? (size_t)TT * (C2 + SN_PADH) : 0)) * sizeof(u16);
}

int sn_conv_tile(int C1, int C2, int k, int stride, int dil) {
  return sn_pick_tile([=](int TT) { return sn_conv_lds(TT, C1, C2, k, stride, dil); });
}

int sn_convtr_tile(int C) {
  return sn_pick_tile([=](int TT) { return sn_convtr_lds(TT, C); });
}

int sn_lstm_check(const SnLstm& p) {
  VBX_REQUIRE(p.xproj && p.w0 && p.h0 && p.c && p.x && p.y16, "vbx_lstm: null operand");
  VBX_REQUIRE(p.layers == 1 || (p.layers == 2 && p.w1 && p.bias1 && p.h1), "vbx_lstm: 1 or 2 layers, the second with its operands");
  VBX_REQUIRE(p.H >= 32 && p.H % 32 == 0 && p.H <= 1024, "vbx_lstm: H must be a multiple of 32 in 32 .. 1024 (got %d)", p.H);
  VBX_REQUIRE(p.B >= 1 && p.T >= 1 && cdiv(p.B, 16) <= 65535, "vbx_lstm: need B >= 1 and T >= 1");
  VBX_REQUIRE((long)p.B * p.T * 4 * p.H < (1L << 40), "vbx_lstm: too large");
  return 0;
}

}  // namespace

extern "C" int vbx_seanet_conv_tile(int C1, int C2, int k, int stride, int dilation) {
  if (int rc = sn_conv_check(C1, C2, k, stride, dilation)) return rc;
  const int TT = sn_conv_tile(C1, C2, k, stride, dilation);
  if (!TT) {
    vbx_set_error("vbx_seanet_conv: 16 output positions of this convolution do not fit the LDS");
    return VBX_EINVAL;
  }
  return TT;
}

static int sn_conv_launch(const int* lens, const void* x1_f16, const void* x2_f16, const void* w_f16, const float* bias, void* y, int B, int L, int C1,
                                 int C2, int Co, int k, int stride, int dilation, int elu1, int out_f32, int causal, void* stream) {
  VBX_REQUIRE(x1_f16 && w_f16 && bias && y && (x2_f16 || !C2), "vbx_seanet_conv: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && Co >= 1 && Co <= 4096, "vbx_seanet_conv: need B in 1 .. 65535, L >= 1, Co in 1 .. 4096");
  if (int rc = sn_conv_check(C1, C2, k, stride, dilation)) return rc;
  int TT = sn_conv_tile(C1, C2, k, stride, dilation);
  VBX_REQUIRE(TT > 0, "vbx_seanet_conv: 16 output positions of this convolution do not fit the LDS");
  while (TT > 16 && TT / 2 >= cdiv(L, stride)) TT >>= 1;  // a short row: no tile of padding positions is staged or multiplied
  SnConv p;
  p.x1 = (const u16*)x1_f16, p.x2 = C2 ? (const u16*)x2_f16 : nullptr, p.w = (const u16*)w_f16, p.bias = bias, p.y = y;
  p.L = L, p.Lout = cdiv(L, stride), p.C1 = C1, p.C2 = C2, p.Co = Co, p.k = k, p.stride = stride, p.dil = dilation;
  const SnPads pads = sn_pads(k, stride, dilation, L, p.Lout, causal);
  p.pad_left = pads.left, p.Lz = pads.Lz;
  p.elu1 = elu1 ? 1 : 0, p.out_f32 = out_f32 ? 1 : 0, p.TT = TT, p.Ktot = k * C1 + C2;
  p.lens = lens, p.causal = causal ? 1 : 0;
  VBX_REQUIRE((long)L * stride < (1L << 30), "vbx_seanet_conv: row too long");
  const size_t bytes = sn_conv_lds(TT, C1, C2, k, stride, dilation);
  const int MG = sn_blocks_per_item((Co + 15) / 16, TT / 16), blocks = cdiv(p.Lout, TT);
  if (lens) {
    if (MG == 4) return sn_launch<seanet_conv_kernel<4, true>>("vbx_seanet_conv_lens", p, blocks, B, bytes, (hipStream_t)stream);
    if (MG == 2) return sn_launch<seanet_conv_kernel<2, true>>("vbx_seanet_conv_lens", p, blocks, B, bytes, (hipStream_t)stream);
    return sn_launch<seanet_conv_kernel<1, true>>("vbx_seanet_conv_lens", p, blocks, B, bytes, (hipStream_t)stream);
  }
  if (MG == 4) return sn_launch<seanet_conv_kernel<4>>("vbx_seanet_conv", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<seanet_conv_kernel<2>>("vbx_seanet_conv", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<seanet_conv_kernel<1>>("vbx_seanet_conv", p, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_seanet_conv_c(const void* x1_f16, const void* x2_f16, const void* w_f16, const float* bias, void* y, int B, int L, int C1,
                                 int C2, int Co, int k, int stride, int dilation, int elu1, int out_f32, int causal, void* stream) {
  return sn_conv_launch(nullptr, x1_f16, x2_f16, w_f16, bias, y, B, L, C1, C2, Co, k, stride, dilation, elu1, out_f32, causal, stream);
}

extern "C" int vbx_seanet_conv_lens(const void* x1_f16, const void* x2_f16, const int* lens, const void* w_f16, const float* bias, void* y,
                                    int B, int L, int C1, int C2, int Co, int k, int stride, int dilation, int elu1, int out_f32, int causal,
                                    void* stream) {
  VBX_REQUIRE(lens, "vbx_seanet_conv_lens: lens is NULL (vbx_seanet_conv_c is the entry without lengths)");
  return sn_conv_launch(lens, x1_f16, x2_f16, w_f16, bias, y, B, L, C1, C2, Co, k, stride, dilation, elu1, out_f32, causal, stream);
}

extern "C" int vbx_seanet_conv(const void* x1_f16, const void* x2_f16, const void* w_f16, const float* bias, void* y, int B, int L, int C1,
                               int C2, int Co, int k, int stride, int dilation, int elu1, int out_f32, void* stream) {
  return vbx_seanet_conv_c(x1_f16, x2_f16, w_f16, bias, y, B, L, C1, C2, Co, k, stride, dilation, elu1, out_f32, 0, stream);
}

static int sn_conv0_launch(const int* lens, const float* wave, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k,
                                  int causal, void* stream) {
  VBX_REQUIRE(wave && w && bias && y_f16 && B >= 1 && B <= 65535 && T >= 1, "vbx_seanet_conv0: bad args");
  VBX_REQUIRE(nf >= 8 && nf % 8 == 0 && nf <= 64, "vbx_seanet_conv0: n_filters must be a multiple of 8 up to 64 (got %d)", nf);
  VBX_REQUIRE(k >= 1 && k <= SN_MAX_K && (k & 1), "vbx_seanet_conv0: kernel_size must be odd, at most %d (got %d)", SN_MAX_K - 1, k);
  VBX_REQUIRE((long)T * (nf / 8) < (1L << 31) * 256, "vbx_seanet_conv0: row too long");
  const SnPads pads = sn_pads(k, 1, 1, T, T, causal);
  const dim3 grid(cdiv((long)T * (nf / 8), 256), B);
  if (lens)
    hipLaunchKernelGGL(seanet_conv0_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, wave, w, bias, (u16*)y_f16, T, nf, k, pads.left,
                       pads.Lz, lens, causal ? 1 : 0);
  else
    hipLaunchKernelGGL(seanet_conv0_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, wave, w, bias, (u16*)y_f16, T, nf, k, pads.left,
                       pads.Lz, (const int*)nullptr, causal ? 1 : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_seanet_conv0_c(const float* wave, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k,
                                  int causal, void* stream) {
  return sn_conv0_launch(nullptr, wave, w, bias, y_f16, B, T, nf, k, causal, stream);
}

extern "C" int vbx_seanet_conv0_lens(const float* wave, const int* lens, const float* w, const float* bias, void* y_f16, int B, int T, int nf,
                                     int k, int causal, void* stream) {
  VBX_REQUIRE(lens, "vbx_seanet_conv0_lens: lens is NULL (vbx_seanet_conv0_c is the entry without lengths)");
  return sn_conv0_launch(lens, wave, w, bias, y_f16, B, T, nf, k, causal, stream);
}

extern "C" int vbx_seanet_conv0(const float* wave, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k,
                                void* stream) {
  return vbx_seanet_conv0_c(wave, w, bias, y_f16, B, T, nf, k, 0, stream);
}

static SnLstm sn_lstm_desc(const float* xproj, const void* w_hh0, const void* w_cat1, const float* bias1, void* h0, void* h1, float* c,
                           const void* x, void* y16, float* y32, int B, int T, int H, int layers) {
  SnLstm p;
  p.xproj = xproj, p.w0 = (const u16*)w_hh0, p.w1 = (const u16*)w_cat1, p.bias1 = bias1, p.h0 = (u16*)h0, p.h1 = (u16*)h1, p.c = c;
  p.x = (const u16*)x, p.y16 = (u16*)y16, p.y32 = y32, p.B = B, p.T = T, p.H = H, p.layers = layers, p.s = 0;
  return p;
}

extern "C" int vbx_lstm_step(const float* xproj, const void* w_hh0, const void* w_cat1, const float* bias1, void* h0, void* h1, float* c,
                             const void* x, void* y16, float* y32, int B, int T, int H, int layers, int s, void* stream) {
  SnLstm p = sn_lstm_desc(xproj, w_hh0, w_cat1, bias1, h0, h1, c, x, y16, y32, B, T, H, layers);
  if (int rc = sn_lstm_check(p)) return rc;
  VBX_REQUIRE(s >= 0 && s < T + layers - 1, "vbx_lstm_step: step %d outside 0 .. T + layers - 2", s);
  p.s = s;
  hipLaunchKernelGGL(seanet_lstm_step_kernel, dim3(H / 16, layers, cdiv(B, 16)), dim3(256), 0, (hipStream_t)stream, p);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_lstm(const float* xproj, const void* w_hh0, const void* w_cat1, const float* bias1, void* h0, void* h1, float* c,
                        const void* x, void* y16, float* y32, int B, int T, int H, int layers, void* stream) {
  SnLstm p = sn_lstm_desc(xproj, w_hh0, w_cat1, bias1, h0, h1, c, x, y16, y32, B, T, H, layers);
  if (int rc = sn_lstm_check(p)) return rc;
  for (int s = 0; s < T + layers - 1; s++) {
    p.s = s;
    hipLaunchKernelGGL(seanet_lstm_step_kernel, dim3(H / 16, layers, cdiv(B, 16)), dim3(256), 0, (hipStream_t)stream, p);
  }
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_seanet_convtr_tile(int C, int stride) {
  if (int rc = sn_convtr_check(C, stride)) return rc;
  const int TT = sn_convtr_tile(C);
  if (!TT) {
    vbx_set_error("vbx_seanet_convtr: 16 rows of this transposed convolution do not fit the LDS");
    return VBX_EINVAL;
  }
  return TT;
}

extern "C" int vbx_seanet_convtr_t(const void* x_f16, const void* w_f16, const float* bias, void* y_f16, int B, int L, int C, int stride,
                                   int trim_left, void* stream) {
  VBX_REQUIRE(x_f16 && w_f16 && bias && y_f16, "vbx_seanet_convtr: null operand");
  VBX_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "vbx_seanet_convtr: need B in 1 .. 65535, L >= 1");
  if (int rc = sn_convtr_check(C, stride)) return rc;
  VBX_REQUIRE(trim_left >= 0 && trim_left <= stride, "vbx_seanet_convtr_t: trim_left must be in 0 .. stride (got %d, stride %d)", trim_left,
              stride);
  VBX_REQUIRE((long)L * stride < (1L << 30), "vbx_seanet_convtr: row too long");
  int TT = sn_convtr_tile(C);
  VBX_REQUIRE(TT > 0, "vbx_seanet_convtr: 16 rows of this transposed convolution do not fit the LDS");
  const int rows = trim_left ? L + 1 : L;  // nothing trimmed in front: row L lies wholly behind the output
  while (TT > 16 && TT / 2 >= rows) TT >>= 1;  // a short row: no tile of rows that store nothing
  SnConvTr p;
  p.x = (const u16*)x_f16, p.w = (const u16*)w_f16, p.bias = bias, p.y = (u16*)y_f16;
  p.L = L, p.C = C, p.Co = C / 2, p.r = stride, p.left = trim_left, p.TT = TT, p.N = stride * (C / 2), p.Ktot = 2 * C;
  const size_t bytes = sn_convtr_lds(TT, C);
  const int MG = sn_blocks_per_item((p.N + 15) / 16, TT / 16), blocks = cdiv(rows, TT);
  if (MG == 4) return sn_launch<seanet_convtr_kernel<4>>("vbx_seanet_convtr", p, blocks, B, bytes, (hipStream_t)stream);
  if (MG == 2) return sn_launch<seanet_convtr_kernel<2>>("vbx_seanet_convtr", p, blocks, B, bytes, (hipStream_t)stream);
  return sn_launch<seanet_convtr_kernel<1>>("vbx_seanet_convtr", p, blocks, B, bytes, (hipStream_t)stream);
}

extern "C" int vbx_seanet_convtr(const void* x_f16, const void* w_f16, const float* bias, void* y_f16, int B, int L, int C, int stride,
                                 void* stream) {
  return vbx_seanet_convtr_t(x_f16, w_f16, bias, y_f16, B, L, C, stride, stride - stride / 2, stream);
}

extern "C" int vbx_seanet_conv_out_c(const void* x_f16, const float* w, const float* bias, float* y, int B, int T, int nf, int k,
                                     int causal, void* stream) {
  VBX_REQUIRE(x_f16 && w && bias && y && B >= 1 && B <= 65535 && T >= 1, "vbx_seanet_conv_out: bad args");
  VBX_REQUIRE(nf >= 8 && nf % 8 == 0 && nf <= 64, "vbx_seanet_conv_out: n_filters must be a multiple of 8 up to 64 (got %d)", nf);
  VBX_REQUIRE(k >= 1 && k <= 7 && (k & 1), "vbx_seanet_conv_out: last_kernel_size must be odd, at most 7 (got %d)", k);
  VBX_REQUIRE(T < (1 << 30), "vbx_seanet_conv_out: row too long");
  const SnPads pads = sn_pads(k, 1, 1, T, T, causal);
  hipLaunchKernelGGL(seanet_conv_out_kernel, dim3(cdiv(T, 256), B), dim3(256), 0, (hipStream_t)stream, (const u16*)x_f16, w, bias, y, T, nf,
                     k, pads.left, pads.Lz);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_seanet_conv_out(const void* x_f16, const float* w, const float* bias, float* y, int B, int T, int nf, int k,
                                   void* stream) {
  return vbx_seanet_conv_out_c(x_f16, w, bias, y, B, T, nf, k, 0, stream);
}

extern "C" int vbx_seanet_pack_latents(const float* z, void* y_f16, int B, int D, int T, void* stream) {
  VBX_REQUIRE(z && y_f16 && B >= 1 && B <= 65535 && D >= 1 && D <= 65535 * 32 && T >= 1, "vbx_seanet_pack_latents: bad args");
  hipLaunchKernelGGL(seanet_pack_latents_kernel, dim3(cdiv(T, 32), cdiv(D, 32), B), dim3(256), 0, (hipStream_t)stream, z, (u16*)y_f16, D, T);
  VBX_LAUNCH_CHECK();
  return 0;
}
