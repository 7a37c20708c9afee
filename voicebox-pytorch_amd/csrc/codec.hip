// Codec-latent front / back end of VoiceBox(audio_enc_dec = codec) with latent_dim != dim (voicebox_pytorch.py:911-914, 964-966,
// 1000-1048): the fused proj_in + mask + null-cond kernel that writes the to_embed operand, the reduction of its weight gradient,
// and the masked MSE / column copy at a latent width that is not a multiple of 8 (the prediction lives in a padded buffer).
#include "common.hpp"

namespace {

constexpr int PI_TM = 32;   // rows of x AND of cond per workgroup (64 activation rows against one weight panel)
constexpr int PI_TN = 64;   // output columns per workgroup: 16 per wave
constexpr int PI_KC = 128;  // K chunk staged in the LDS
constexpr int PI_LD = PI_KC + 8;  // row stride 272 bytes: consecutive rows start 4 banks apart

// out[row, 0:D]           = x[row] . W^T + b
// out[row, D+E : 2D+E]    = drop[b] ? null_cond : (cmask[row] ? 0 : cond[row] . W^T + b)
// computed transposed (C^T[n][m] = sum_k W[n][k] X[m][k]) so that a lane holds four consecutive output columns of one row.
// xcb (training): the bf16 operand of the weight gradient, [2M, Kp]: rows 0..M-1 = x, rows M..2M-1 = cond with the rows that pass no
// gradient (cond_mask set, dropped sample) zeroed; column L = 1 on every row that counts, so that column L of dY^T . xcb is d(bias).
__global__ __launch_bounds__(256) void proj_in_embed_kernel(const float* __restrict__ x, const float* __restrict__ cond,
                                                            const u16* __restrict__ wh, const float* __restrict__ bias,
                                                            const uint8_t* __restrict__ cmask, const uint8_t* __restrict__ drop,
                                                            const float* __restrict__ null_cond, u16* __restrict__ out,
                                                            u16* __restrict__ outb, u16* __restrict__ xcb, long M, int N, int L,
                                                            int Kp, int D, int Ke, int cond_col) {
  __shared__ __attribute__((aligned(16))) u16 sA[2 * PI_TM * PI_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * PI_TM;
  const int n0 = blockIdx.y * PI_TN + wave * 16;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Kp; k0 += PI_KC) {
    const int kc = (Kp - k0) < PI_KC ? (Kp - k0) : PI_KC;  // multiple of 32
    if (k0) __syncthreads();
    for (int i = tid; i < 2 * PI_TM * PI_KC; i += 256) {
      const int r = i / PI_KC, c = i - r * PI_KC;
      if (c >= kc) continue;
      const bool is_cond = r >= PI_TM;
      const long row = m0 + (is_cond ? r - PI_TM : r);
      const int k = k0 + c;
      float v = 0.f;
      if (row < M && k < L) v = (is_cond ? cond : x)[row * L + k];
      sA[r * PI_LD + c] = f32_to_f16_sat(v);
      if (xcb && blockIdx.y == 0 && row < M) {
        bool keep = true;
        if (is_cond) keep = !(drop && drop[row / N]) && !(cmask && cmask[row]);
        const float o = keep ? (k == L ? 1.0f : v) : 0.f;
        xcb[((is_cond ? M : 0) + row) * Kp + k] = f32_to_bf16(o);
      }
    }
    __syncthreads();
    for (int kk = 0; kk < kc; kk += 32) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(wh + (long)(n0 + (lane & 15)) * Kp + k0 + kk + (lane >> 4) * 8);
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const f16x8 b = *reinterpret_cast<const f16x8*>(sA + (t * 16 + (lane & 15)) * PI_LD + kk + (lane >> 4) * 8);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  // epilogue: lane holds columns n0 + (lane >> 4) * 4 + 0..3 of activation row t * 16 + (lane & 15)
  const int nc = n0 + (lane >> 4) * 4;
  const float4 bv = *reinterpret_cast<const float4*>(bias + nc);
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const bool is_cond = t >= 2;
    const long row = m0 + (t & 1) * 16 + (lane & 15);
    if (row >= M) continue;
    float v0 = acc[t][0] + bv.x, v1 = acc[t][1] + bv.y, v2 = acc[t][2] + bv.z, v3 = acc[t][3] + bv.w;
    if (is_cond) {
      if (drop && drop[row / N]) {
        const float4 nv = *reinterpret_cast<const float4*>(null_cond + nc);
        v0 = nv.x; v1 = nv.y; v2 = nv.z; v3 = nv.w;
      } else if (cmask && cmask[row]) {
        v0 = v1 = v2 = v3 = 0.f;
      }
    }
    const long oo = row * Ke + (is_cond ? cond_col : 0) + nc;
    *reinterpret_cast<uint2*>(out + oo) = make_uint2(pack_f16x2_sat(v0, v1), pack_f16x2_sat(v2, v3));
    if (outb) *reinterpret_cast<uint2*>(outb + oo) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
  }
}

// the cond_emb columns [D, D+E) of the same operand rows (the resize of pack_embed_text_kernel, ops.hip)
__global__ void embed_text_cols_kernel(const uint8_t* __restrict__ drop, const long* __restrict__ ids, int T,
                                       const float* __restrict__ table, int E, long null_id, u16* __restrict__ out,
                                       u16* __restrict__ outb, int B, int N, int col0, int Ke) {
  const long total = (long)B * N * E;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / E;
    const int e = (int)(i - row * E);
    const int b = (int)(row / N), n = (int)(row - (long)b * N);
    const bool dropped = drop && drop[b];
    int i0, i1;
    float lam;
    interp_src(n, N, T, i0, i1, lam);
    const long id0 = dropped ? null_id : ids[(long)b * T + i0], id1 = dropped ? null_id : ids[(long)b * T + i1];
    const float r0 = table[id0 * E + e], r1 = table[id1 * E + e];
    const float v = (T == N) ? r0 : ((1.0f - lam) * r0 + lam * r1);
    const long oo = row * Ke + col0 + e;
    out[oo] = f32_to_f16_sat(v);
    if (outb) outb[oo] = f32_to_bf16(v);
  }
}

// embed_text_cols_kernel with the row's own token and frame counts (include/vbx.h, vbx_io.tok_lens; the resize of
// pack_embed_text_lens_kernel, ops.hip): both clamped here, zeros from frame N_b on
__global__ void embed_text_cols_lens_kernel(const uint8_t* __restrict__ drop, const long* __restrict__ ids, int T,
                                            const int* __restrict__ tok_lens, const int* __restrict__ key_lens, int R,
                                            const float* __restrict__ table, int E, long null_id, u16* __restrict__ out,
                                            u16* __restrict__ outb, int B, int N, int col0, int Ke) {
  const long total = (long)B * N * E;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / E;
    const int e = (int)(i - row * E);
    const int b = (int)(row / N), n = (int)(row - (long)b * N);
    const int Tb = min(max(tok_lens[b], 1), T), Nb = min(max(key_lens[b] - R, 1), N);
    const long oo = row * Ke + col0 + e;
    if (n >= Nb) {
      out[oo] = 0;
      if (outb) outb[oo] = 0;
      continue;
    }
    const bool dropped = drop && drop[b];
    int i0, i1;
    float lam;
    interp_src(n, Nb, Tb, i0, i1, lam);
    const long id0 = dropped ? null_id : ids[(long)b * T + i0], id1 = dropped ? null_id : ids[(long)b * T + i1];
    const float r0 = table[id0 * E + e], r1 = table[id1 * E + e];
    const float v = (Tb == Nb) ? r0 : ((1.0f - lam) * r0 + lam * r1);
    out[oo] = f32_to_f16_sat(v);
    if (outb) outb[oo] = f32_to_bf16(v);
  }
}

// slabs [splits][D][Kp] of dY^T . xcb  ->  d(proj_in.weight) [D, L] (columns 0..L-1) and d(proj_in.bias) [D] (column L)
__global__ void proj_in_wgrad_reduce_kernel(const float* __restrict__ slabs, int splits, int D, int Kp, int L,
                                            float* __restrict__ dw, float* __restrict__ db) {
  const long total = (long)D * Kp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / Kp), c = (int)(i - (long)r * Kp);
    if (c > L) continue;
    float s = 0.f;
    for (int k = 0; k < splits; k++) s += slabs[(long)k * total + i];
    if (c < L) dw[(long)r * L + c] = s;
    else db[r] = s;
  }
}

// masked MSE with a padded prediction: pred [B*N, ldp], target [B*N, D]; same partial layout as mse_fwd_kernel (ops.hip)
constexpr int MSE_SPLITS = 64;
__global__ __launch_bounds__(256) void mse_fwd_ld_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ lmask, float* __restrict__ per_b, int B,
                                                          int N, int D) {
  __shared__ float red[8];
  const int b = blockIdx.y, sp = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f, cnt = 0.f;
  for (int n = sp * 4 + wave; n < N; n += 4 * MSE_SPLITS) {
    if (!lmask[(long)b * N + n]) continue;
    const float* p = pred + ((long)b * N + n) * ldp;
    const float* t = target + ((long)b * N + n) * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float a = p[c] - t[c];
      s += a * a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    acc += s / (float)D;
    cnt += 1.f;
  }
  if (lane == 0) { red[wave] = acc; red[4 + wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* part = per_b + 2 * B + ((long)b * MSE_SPLITS + sp) * 2;
    part[0] = red[0] + red[1] + red[2] + red[3];
    part[1] = red[4] + red[5] + red[6] + red[7];
  }
}
__global__ void mse_mean_ld_kernel(float* __restrict__ per_b, float* __restrict__ loss, int B) {
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int b = 0; b < B; b++) {
    const float2 pc = *reinterpret_cast<const float2*>(per_b + 2 * B + ((long)b * MSE_SPLITS + lane) * 2);
    float num = pc.x, cnt = pc.y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    const float den = fmaxf(cnt, 1e-5f);
    if (lane == 0) {
      per_b[b] = num / den;
      per_b[B + b] = den;
    }
    s += num / den;
  }
  if (lane == 0) loss[0] = s / (float)B;
}
// dpred bf16 [B*N, ldp] = gscale * 2 (p - t) / D * mask / (den[b] * B), zero in the pad columns
__global__ void mse_bwd_ld_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ target,
                                  const uint8_t* __restrict__ lmask, const float* __restrict__ per_b,
                                  const float* __restrict__ gscale, u16* __restrict__ dpb, int B, int N, int D) {
  const long total = (long)B * N * ldp;
  const float gs = gscale ? gscale[0] : 1.0f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / ldp;
    const int c = (int)(i - row * ldp), b = (int)(row / N);
    float o = 0.f;
    if (c < D && lmask[row]) o = gs * 2.0f / ((float)D * per_b[B + b] * (float)B) * (pred[i] - target[row * D + c]);
    dpb[i] = f32_to_bf16(o);
  }
}
__global__ void copy_cols_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, long rows, int cols) {
  const long total = rows * cols;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cols;
    dst[i] = src[r * lds + (i - r * cols)];
  }
}

inline int grid_for(long n, int cap = 4096) {
  long b = (n + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vbx_proj_in_kp(int L) { return (L + 1 + 31) / 32 * 32; }

extern "C" int vbx_proj_in_embed(const float* x, const float* cond, const void* w_f16, const float* bias, const uint8_t* cond_mask,
                                 const uint8_t* drop_mask, const float* null_cond, void* out_f16, void* out_bf16, void* xc_bf16,
                                 int B, int N, int L, int D, int E, void* stream) {
  VBX_REQUIRE(x && cond && w_f16 && bias && out_f16 && B > 0 && N > 0, "vbx_proj_in_embed: bad args");
  VBX_REQUIRE(L >= 8 && L <= 1024 && D > 0 && D % PI_TN == 0 && E >= 0 && E % 8 == 0,
              "vbx_proj_in_embed: latent_dim must be in 8 .. 1024, dim a multiple of 64, dim_cond_emb a multiple of 8");
  VBX_REQUIRE(!drop_mask || null_cond, "vbx_proj_in_embed: a drop mask needs null_cond");
  const long M = (long)B * N;
  hipLaunchKernelGGL(proj_in_embed_kernel, dim3((unsigned)cdiv(M, PI_TM), D / PI_TN), dim3(256), 0, ST, x, cond, (const u16*)w_f16,
                     bias, cond_mask, drop_mask, null_cond, (u16*)out_f16, (u16*)out_bf16, (u16*)xc_bf16, M, N, L, vbx_proj_in_kp(L),
                     D, 2 * D + E, D + E);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_embed_text_cols(const uint8_t* drop_mask, const long* ids, int T, const float* table, int E, long null_id,
                                   void* out_f16, void* out_bf16, int B, int N, int col0, int ld, void* stream) {
  VBX_REQUIRE(ids && table && out_f16 && T > 0 && E > 0 && col0 >= 0 && ld >= col0 + E, "vbx_embed_text_cols: bad args");
  hipLaunchKernelGGL(embed_text_cols_kernel, dim3(grid_for((long)B * N * E)), dim3(256), 0, ST, drop_mask, ids, T, table, E, null_id,
                     (u16*)out_f16, (u16*)out_bf16, B, N, col0, ld);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_embed_text_cols_lens(const uint8_t* drop_mask, const long* ids, int T, const int* tok_lens, const int* key_lens, int R,
                                        const float* table, int E, long null_id, void* out_f16, void* out_bf16, int B, int N, int col0,
                                        int ld, void* stream) {
  VBX_REQUIRE(ids && table && out_f16 && T > 0 && E > 0 && col0 >= 0 && ld >= col0 + E, "vbx_embed_text_cols_lens: bad args");
  VBX_REQUIRE(tok_lens && key_lens && R >= 0, "vbx_embed_text_cols_lens: needs tok_lens and key_lens (vbx_embed_text_cols is the entry without)");
  hipLaunchKernelGGL(embed_text_cols_lens_kernel, dim3(grid_for((long)B * N * E)), dim3(256), 0, ST, drop_mask, ids, T, tok_lens, key_lens, R,
                     table, E, null_id, (u16*)out_f16, (u16*)out_bf16, B, N, col0, ld);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_proj_in_wgrad_reduce(const float* slabs, int splits, int D, int L, float* dw, float* db, void* stream) {
  VBX_REQUIRE(slabs && splits >= 1 && D > 0 && L > 0 && dw && db, "vbx_proj_in_wgrad_reduce: bad args");
  const int Kp = vbx_proj_in_kp(L);
  hipLaunchKernelGGL(proj_in_wgrad_reduce_kernel, dim3(grid_for((long)D * Kp)), dim3(256), 0, ST, slabs, splits, D, Kp, L, dw, db);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_masked_mse_fwd_ld(const float* pred, int ldp, const float* target, const uint8_t* loss_mask, float* per_b,
                                     float* loss, int B, int N, int D, void* stream) {
  VBX_REQUIRE(pred && target && loss_mask && per_b && loss && D > 0 && ldp >= D, "vbx_masked_mse_fwd_ld: bad args");
  hipLaunchKernelGGL(mse_fwd_ld_kernel, dim3(MSE_SPLITS, B), dim3(256), 0, ST, pred, ldp, target, loss_mask, per_b, B, N, D);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(mse_mean_ld_kernel, dim3(1), dim3(64), 0, ST, per_b, loss, B);
  VBX_LAUNCH_CHECK();
  return 0;
}
extern "C" int vbx_masked_mse_bwd_ld(const float* pred, int ldp, const float* target, const uint8_t* loss_mask, const float* per_b,
                                     const float* gscale, void* dpred_bf16, int B, int N, int D, void* stream) {
  VBX_REQUIRE(pred && target && loss_mask && per_b && dpred_bf16 && D > 0 && ldp >= D, "vbx_masked_mse_bwd_ld: bad args");
  hipLaunchKernelGGL(mse_bwd_ld_kernel, dim3(grid_for((long)B * N * ldp)), dim3(256), 0, ST, pred, ldp, target, loss_mask, per_b,
                     gscale, (u16*)dpred_bf16, B, N, D);
  VBX_LAUNCH_CHECK();
  return 0;
}
extern "C" int vbx_copy_cols_f32(const float* src, int ld_src, float* dst, long rows, int cols, void* stream) {
  VBX_REQUIRE(src && dst && rows > 0 && cols > 0 && ld_src >= cols, "vbx_copy_cols_f32: bad args");
  hipLaunchKernelGGL(copy_cols_kernel, dim3(grid_for(rows * cols)), dim3(256), 0, ST, src, ld_src, dst, rows, cols);
  VBX_LAUNCH_CHECK();
  return 0;
}
