// DurationPredictor training (voicebox_pytorch.py:841-876): the head (to_pred + masked L1 over the predicted durations), its backward
// and the deterministic gradient of the phoneme embedding table.  fp32 throughout, no atomics; every sum runs in an order fixed by
// the shapes alone (never by the grid), so reruns are bit-identical and a batch row gives the same bits alone as inside a batch.
// Contract and error bounds: include/vbx.h.
#include "common.hpp"

namespace {

constexpr int HB_ROWS = 32;  // rows of hid per workgroup of the head backward: one dw / db partial each

// d[r] = hid[r,:] . w + b: one wave per row, the arithmetic of rowdot_kernel (ops.hip) term for term -- the durations of a
// training forward are the bits that eval mode returns for the same hidden state.
__global__ __launch_bounds__(256) void head_rowdot_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, long rows, int D) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s = 0.f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 a = *reinterpret_cast<const float4*>(x + r * D + d), b = *reinterpret_cast<const float4*>(w + d);
    s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  s = wave_sum(s);
  if (lane == 0) out[r] = s + (bias ? bias[0] : 0.f);
}

// ONE workgroup walks the batch rows in order.  Row b: thread t adds positions t, t + 256, ... in ascending order, the 64 lanes of a
// wave combine in the xor butterfly, thread 0 adds the four waves 0..3; then loss = (sum_b num_b / max(den_b, 1e-5)) / B in ascending
// b.  Nothing here depends on the other rows of the batch, and a [1, n] call divides by 1.
__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ d, const float* __restrict__ t,
                                                        const uint8_t* __restrict__ m, float* __restrict__ num, float* __restrict__ den,
                                                        float* __restrict__ loss, int B, int n) {
  __shared__ float sn[4], sd[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float total = 0.f;
  for (int b = 0; b < B; b++) {
    float pn = 0.f, pd = 0.f;
    for (int i = tid; i < n; i += 256) {
      const long r = (long)b * n + i;
      if (m[r]) {
        pn += fabsf(d[r] - t[r]);
        pd += 1.0f;
      }
    }
    pn = wave_sum(pn);
    pd = wave_sum(pd);
    if (lane == 0) { sn[wv] = pn; sd[wv] = pd; }
    __syncthreads();
    if (tid == 0) {
      const float nb = ((sn[0] + sn[1]) + sn[2]) + sn[3], db = ((sd[0] + sd[1]) + sd[2]) + sd[3];
      num[b] = nb;
      den[b] = db;
      total += nb / fmaxf(db, 1e-5f);
    }
    __syncthreads();
  }
  if (tid == 0) loss[0] = total / (float)B;
}

// g_r = gscale * m * sign(d - t) / (B * max(den_b, 1e-5)); dhid[r,:] = g_r * w; partial c (rows [32 c, 32 c + 32)) of
// dw = sum_r g_r hid[r,:] and db = sum_r g_r, rows ascending.  part is [chunks][D + 4]: column D holds the db partial.
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ hid, const float* __restrict__ w,
                                                       const float* __restrict__ d, const float* __restrict__ t,
                                                       const uint8_t* __restrict__ m, const float* __restrict__ den,
                                                       const float* __restrict__ gscale, float* __restrict__ dhid,
                                                       float* __restrict__ part, long rows, int B, int n, int D) {
  __shared__ float g[HB_ROWS];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * HB_ROWS;
  const int nr = (int)((rows - r0) < HB_ROWS ? (rows - r0) : HB_ROWS);
  if (tid < HB_ROWS) {
    float v = 0.f;
    if (tid < nr) {
      const long r = r0 + tid;
      const float diff = d[r] - t[r];
      const float s = !m[r] ? 0.f : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));  // sign(0) = 0 (and NaN -> 0) as torch's l1_loss
      const float gs = gscale ? gscale[0] : 1.f;
      v = (gs * s) / ((float)B * fmaxf(den[r / n], 1e-5f));
    }
    g[tid] = v;
  }
  __syncthreads();
  float* prow = part + (long)blockIdx.x * (D + 4);
  for (int c = tid * 4; c < D; c += 1024) {
    const float4 wv = *reinterpret_cast<const float4*>(w + c);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < nr; i++) {
      const float gi = g[i];
      const long o = (r0 + i) * D + c;
      const float4 h = *reinterpret_cast<const float4*>(hid + o);
      *reinterpret_cast<float4*>(dhid + o) = make_float4(gi * wv.x, gi * wv.y, gi * wv.z, gi * wv.w);
      acc.x += gi * h.x; acc.y += gi * h.y; acc.z += gi * h.z; acc.w += gi * h.w;
    }
    *reinterpret_cast<float4*>(prow + c) = acc;
  }
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < nr; i++) s += g[i];
    prow[D] = s;
  }
}
// dw[c] = sum over the partials in ascending order, db = the same over column D
__global__ void head_bwd_reduce_kernel(const float* __restrict__ part, int chunks, int D, float* __restrict__ dw, float* __restrict__ db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > D) return;
  float s = 0.f;
  for (int k = 0; k < chunks; k++) s += part[(long)k * (D + 4) + c];
  if (c < D) dw[c] = s; else db[0] = s;
}

// One workgroup per table row v.  The ids are scanned in tiles of 256 positions: every wave ballots "max(ids[r], 0) == v", the four
// 64-bit masks go through LDS, and every thread (one column e, + 256, ...) walks the set bits from the lowest up -- ascending r.
__global__ __launch_bounds__(256) void phoneme_emb_bwd_kernel(const long* __restrict__ ids, const float* __restrict__ ga, int lda,
                                                              const float* __restrict__ gb, float* __restrict__ gtable, long R, int E) {
  __shared__ unsigned long long hit[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long v = blockIdx.x;
  constexpr int EMAX = 8;  // columns per thread: E <= 2048
  float acc[EMAX];
#pragma unroll
  for (int j = 0; j < EMAX; j++) acc[j] = 0.f;
  for (long base = 0; base < R; base += 256) {
    const long r = base + tid;
    bool match = false;
    if (r < R) {
      long id = ids[r];
      id = id < 0 ? 0 : id;
      match = id == v;
    }
    const unsigned long long bal = __ballot(match);
    if (lane == 0) hit[wv] = bal;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
      unsigned long long bits = hit[q];
      while (bits) {  // four hits at a time: their loads are in flight together, the additions stay in ascending r
        long rr[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
          rr[h] = bits ? base + q * 64 + __builtin_ctzll(bits) : -1;
          bits &= bits - 1;  // 0 stays 0
        }
#pragma unroll
        for (int j = 0; j < EMAX; j++) {
          const int e = tid + j * 256;
          if (e < E) {
            float x[4];
#pragma unroll
            for (int h = 0; h < 4; h++) {
              x[h] = 0.f;
              if (rr[h] >= 0) {
                x[h] = ga ? ga[rr[h] * lda + e] : gb[rr[h] * E + e];
                if (ga && gb) x[h] += gb[rr[h] * E + e];
              }
            }
#pragma unroll
            for (int h = 0; h < 4; h++)
              if (rr[h] >= 0) acc[j] += x[h];
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < EMAX; j++) {
    const int e = tid + j * 256;
    if (e < E) gtable[v * E + e] = acc[j];
  }
}

// Length regulator of sample(lens="durations"): one workgroup per batch row.  Phoneme i with ids[i] != -1 owns rep_i =
// int(max(durations[i], 1)) frames (torch's clamp(min=1).int(): truncation; a NaN counts 1), a -1 padding phoneme owns none.  Thread t
// takes the contiguous phonemes [t c, t c + c), c = ceil(K / 256): its own sum, an exclusive scan of the 256 sums through LDS, then it
// writes its phonemes' runs; lens[b] = the row total, frames [lens[b], Nmax) get id 0.  aligned == NULL: lens only.  Frames at or past
// Nmax are never written.
constexpr int LR_THREADS = 256;
VBX_DEV long lr_reps(long id, float d) { return id == -1 ? 0L : (long)fminf(fmaxf(d, 1.0f), 1073741824.0f); }
__global__ __launch_bounds__(LR_THREADS) void length_regulate_kernel(const long* __restrict__ ids, const float* __restrict__ dur,
                                                                     long* __restrict__ aligned, int* __restrict__ lens, int K,
                                                                     int Nmax) {
  __shared__ long scan[LR_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int c = (K + LR_THREADS - 1) / LR_THREADS;
  const int i0 = min(tid * c, K), i1 = min(i0 + c, K);
  const long* idr = ids + (long)b * K;
  const float* dr = dur + (long)b * K;
  long mine = 0;
  for (int i = i0; i < i1; i++) mine += lr_reps(idr[i], dr[i]);
  scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < LR_THREADS; off <<= 1) {  // inclusive scan
    const long add = tid >= off ? scan[tid - off] : 0L;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const long total = scan[LR_THREADS - 1];
  if (tid == 0) lens[b] = (int)(total < 2147483647L ? total : 2147483647L);
  if (!aligned) return;
  long* out = aligned + (long)b * Nmax;
  long pos = scan[tid] - mine;
  for (int i = i0; i < i1 && pos < Nmax; i++) {
    const long id = idr[i], end = pos + lr_reps(id, dr[i]);
    for (long j = pos; j < end && j < Nmax; j++) out[j] = id;
    pos = end;
  }
  for (long j = total + tid; j < Nmax; j += LR_THREADS) out[j] = 0;
}

// ---- DurationPredictor front end over codec latents (attach_codec(), voicebox_pytorch.py:776, :793-823): one launch writes the
// to_embed operand [B n, E + D] = [ to_phoneme_emb(max(ids, 0)) | cond'' ],
//   cond''[b, r] = r >= S ? 0 : drop[b] ? null_cond : cmask[b, r] ? 0 : latent[b, r] . W^T + bias
// -- proj_in at length S, then the mask (a masked row is 0, not the bias), then the drop, then curtail_or_pad to n.  The product has
// the arithmetic of proj_in_embed_kernel (codec.hip): operands rounded once to fp16 (saturating), W pre-packed [D, Kp], fp32 sums
// on v_mfma_f32_16x16x32_f16 in ascending k, computed transposed (C^T[d][row] = sum_k W[d][k] X[row][k]) so that a lane holds four
// consecutive output columns of one row; bias added in fp32; one rounding on store.  A workgroup owns 32 rows x 64 columns (16 per
// wave); the workgroups of column block 0 also gather the embedding columns and write lcb.
// lcb (training) bf16 [B n, Kp]: the operand of the weight gradient -- the latent row with column L = 1 on the rows that pass a
// gradient to proj_in, all zero on the others (r >= S, cond_mask set, dropped sample), so d cond''^T . lcb = [ d weight | d bias ].
constexpr int PL_TM = 32;           // rows per workgroup
constexpr int PL_TN = 64;           // output columns per workgroup
constexpr int PL_KC = 128;          // K chunk staged in the LDS
constexpr int PL_LD = PL_KC + 8;    // row stride 272 bytes: consecutive rows start 4 banks apart

VBX_DEV uint4 pl_pack8_h(const float v[8]) {
  return make_uint4(pack_f16x2_sat(v[0], v[1]), pack_f16x2_sat(v[2], v[3]), pack_f16x2_sat(v[4], v[5]), pack_f16x2_sat(v[6], v[7]));
}
VBX_DEV uint4 pl_pack8_b(const float v[8]) {
  return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

__global__ __launch_bounds__(256) void pack_phoneme_latent_kernel(const long* __restrict__ ids, const float* __restrict__ table, int E,
                                                                  const float* __restrict__ latent, int S, int L, int Kp,
                                                                  const u16* __restrict__ wh, const float* __restrict__ bias,
                                                                  const uint8_t* __restrict__ cmask, const uint8_t* __restrict__ drop,
                                                                  const float* __restrict__ null_cond, u16* __restrict__ out,
                                                                  u16* __restrict__ outb, float* __restrict__ emb32,
                                                                  u16* __restrict__ lcb, long M, int N, int D) {
  __shared__ __attribute__((aligned(16))) u16 sA[PL_TM * PL_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * PL_TM;
  const int n0 = blockIdx.y * PL_TN + wave * 16;
  const int ld = E + D;

  if (blockIdx.y == 0) {  // columns 0:E, pack_phoneme_kernel's gather (ops.hip): the same bits
    const int ce = E / 8;
    for (int i = tid; i < PL_TM * ce; i += 256) {
      const int r = i / ce, c = i - r * ce;
      const long row = m0 + r;
      if (row >= M) continue;
      long id = ids[row];
      id = id < 0 ? 0 : id;  // -1 = padding, clamped (:811)
      const float* src = table + id * E + c * 8;
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = src[k];
      *reinterpret_cast<uint4*>(out + row * ld + c * 8) = pl_pack8_h(v);
      if (outb) *reinterpret_cast<uint4*>(outb + row * ld + c * 8) = pl_pack8_b(v);
      if (emb32) {
        *reinterpret_cast<float4*>(emb32 + row * E + c * 8) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(emb32 + row * E + c * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
    }
  }

  f32x4 acc[2];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Kp; k0 += PL_KC) {
    const int kc = (Kp - k0) < PL_KC ? (Kp - k0) : PL_KC;  // multiple of 32
    if (k0) __syncthreads();
    for (int i = tid; i < PL_TM * PL_KC; i += 256) {
      const int r = i / PL_KC, c = i - r * PL_KC;
      if (c >= kc) continue;
      const long row = m0 + r;
      const int k = k0 + c;
      const int b = (int)(row / N), pos = (int)(row - (long)b * N);
      const bool in = row < M && pos < S;  // curtail_or_pad: rows past S hold no latent
      const long crow = (long)b * S + pos;
      float v = 0.f;
      if (in && k < L) v = latent[crow * L + k];
      sA[r * PL_LD + c] = f32_to_f16_sat(v);
      if (lcb && blockIdx.y == 0 && row < M) {
        const bool keep = in && !(drop && drop[b]) && !(cmask && cmask[crow]);
        lcb[row * Kp + k] = f32_to_bf16(keep ? (k == L ? 1.0f : v) : 0.f);
      }
    }
    __syncthreads();
    for (int kk = 0; kk < kc; kk += 32) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(wh + (long)(n0 + (lane & 15)) * Kp + k0 + kk + (lane >> 4) * 8);
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const f16x8 bfr = *reinterpret_cast<const f16x8*>(sA + (t * 16 + (lane & 15)) * PL_LD + kk + (lane >> 4) * 8);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bfr, acc[t], 0, 0, 0);
      }
    }
  }
  // epilogue: lane holds columns n0 + (lane >> 4) * 4 + 0..3 of row t * 16 + (lane & 15)
  const int nc = n0 + (lane >> 4) * 4;
  const float4 bv = *reinterpret_cast<const float4*>(bias + nc);
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const long row = m0 + t * 16 + (lane & 15);
    if (row >= M) continue;
    const int b = (int)(row / N), pos = (int)(row - (long)b * N);
    float v0 = acc[t][0] + bv.x, v1 = acc[t][1] + bv.y, v2 = acc[t][2] + bv.z, v3 = acc[t][3] + bv.w;
    if (pos >= S) {
      v0 = v1 = v2 = v3 = 0.f;
    } else if (drop && drop[b]) {
      const float4 nv = *reinterpret_cast<const float4*>(null_cond + nc);
      v0 = nv.x; v1 = nv.y; v2 = nv.z; v3 = nv.w;
    } else if (cmask && cmask[(long)b * S + pos]) {
      v0 = v1 = v2 = v3 = 0.f;
    }
    const long oo = row * ld + E + nc;
    *reinterpret_cast<uint2*>(out + oo) = make_uint2(pack_f16x2_sat(v0, v1), pack_f16x2_sat(v2, v3));
    if (outb) *reinterpret_cast<uint2*>(outb + oo) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vbx_duration_head_fwd(const float* hid, const float* w, const float* bias, const float* target, const uint8_t* loss_mask,
                                     float* durations, float* num, float* den, float* loss, int B, int n, int D, void* stream) {
  VBX_REQUIRE(hid && w && bias && target && loss_mask && durations && num && den && loss, "vbx_duration_head_fwd: null pointer");
  VBX_REQUIRE(B > 0 && n > 0 && D > 0 && D % 4 == 0 && (long)B * n < (1L << 31), "vbx_duration_head_fwd: bad dims B=%d n=%d D=%d", B, n, D);
  const long rows = (long)B * n;
  hipLaunchKernelGGL(head_rowdot_kernel, dim3((unsigned)cdiv(rows, 4L)), dim3(256), 0, ST, hid, w, bias, durations, rows, D);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_loss_kernel, dim3(1), dim3(256), 0, ST, durations, target, loss_mask, num, den, loss, B, n);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" long vbx_duration_head_bwd_scratch_floats(int B, int n, int D) { return (long)cdiv((long)B * n, HB_ROWS) * (D + 4); }

extern "C" int vbx_duration_head_bwd(const float* hid, const float* w, const float* durations, const float* target,
                                     const uint8_t* loss_mask, const float* den, const float* gscale, float* dhid, float* dw, float* db,
                                     float* scratch, int B, int n, int D, void* stream) {
  VBX_REQUIRE(hid && w && durations && target && loss_mask && den && dhid && dw && db && scratch, "vbx_duration_head_bwd: null pointer");
  VBX_REQUIRE(B > 0 && n > 0 && D > 0 && D % 4 == 0 && (long)B * n < (1L << 31), "vbx_duration_head_bwd: bad dims B=%d n=%d D=%d", B, n, D);
  const long rows = (long)B * n;
  const int chunks = cdiv(rows, HB_ROWS);
  hipLaunchKernelGGL(head_bwd_kernel, dim3(chunks), dim3(256), 0, ST, hid, w, durations, target, loss_mask, den, gscale, dhid, scratch,
                     rows, B, n, D);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_bwd_reduce_kernel, dim3(cdiv(D + 1, 256)), dim3(256), 0, ST, scratch, chunks, D, dw, db);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_phoneme_emb_bwd(const long* ids, const float* g_packed, int ld_packed, const float* g_emb, float* gtable, long rows,
                                   int V, int E, void* stream) {
  VBX_REQUIRE(ids && gtable && (g_packed || g_emb), "vbx_phoneme_emb_bwd: null pointer (one of the two gradients is required)");
  VBX_REQUIRE(rows > 0 && V > 0 && E > 0 && E <= 2048 && (!g_packed || ld_packed >= E), "vbx_phoneme_emb_bwd: bad dims rows=%ld V=%d E=%d ld=%d",
              rows, V, E, ld_packed);
  hipLaunchKernelGGL(phoneme_emb_bwd_kernel, dim3(V), dim3(256), 0, ST, ids, g_packed, ld_packed, g_emb, gtable, rows, E);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_length_regulate(const long* ids, const float* durations, long* aligned, int* lens, int B, int K, int Nmax,
                                   void* stream) {
  VBX_REQUIRE(ids && durations && lens, "vbx_length_regulate: null pointer");
  VBX_REQUIRE(B > 0 && K > 0 && (!aligned || Nmax > 0), "vbx_length_regulate: bad dims B=%d K=%d Nmax=%d", B, K, Nmax);
  hipLaunchKernelGGL(length_regulate_kernel, dim3(B), dim3(LR_THREADS), 0, ST, ids, durations, aligned, lens, K, aligned ? Nmax : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}

static int pack_phoneme_latent(const char* who, const long* ids, const float* table, int E, const float* latent, int S, int L,
                               const void* w_f16, const float* bias, const uint8_t* cond_mask, const uint8_t* drop_mask,
                               const float* null_cond, void* out_f16, void* out_bf16, float* emb_f32, void* lc_bf16, int B, int N, int D,
                               void* stream) {
  VBX_REQUIRE(ids && table && latent && w_f16 && bias && out_f16 && B > 0 && N > 0 && S > 0 && (long)B * N < (1L << 31) &&
                  (long)B * S < (1L << 31),
              "%s: bad args", who);
  VBX_REQUIRE(L >= 8 && L <= 1024 && D > 0 && D % PL_TN == 0 && E > 0 && E % 8 == 0,
              "%s: latent_dim must be in 8 .. 1024, dim a multiple of 64, dim_phoneme_emb a multiple of 8 (got %d, %d, %d)", who, L, D, E);
  VBX_REQUIRE(!drop_mask || null_cond, "%s: a drop mask needs null_cond", who);
  const long M = (long)B * N;
  hipLaunchKernelGGL(pack_phoneme_latent_kernel, dim3((unsigned)cdiv(M, PL_TM), D / PL_TN), dim3(256), 0, ST, ids, table, E, latent, S, L,
                     vbx_proj_in_kp(L), (const u16*)w_f16, bias, cond_mask, drop_mask, null_cond, (u16*)out_f16, (u16*)out_bf16, emb_f32,
                     (u16*)lc_bf16, M, N, D);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_pack_phoneme_latent(const long* ids, const float* table, int E, const float* latent, int S, int L, const void* w_f16,
                                       const float* bias, const uint8_t* cond_mask, const uint8_t* drop_mask, const float* null_cond,
                                       void* out_f16, int B, int N, int D, void* stream) {
  return pack_phoneme_latent("vbx_pack_phoneme_latent", ids, table, E, latent, S, L, w_f16, bias, cond_mask, drop_mask, null_cond, out_f16,
                             nullptr, nullptr, nullptr, B, N, D, stream);
}

extern "C" int vbx_pack_phoneme_latent_train(const long* ids, const float* table, int E, const float* latent, int S, int L,
                                             const void* w_f16, const float* bias, const uint8_t* cond_mask, const uint8_t* drop_mask,
                                             const float* null_cond, void* out_f16, void* out_bf16, float* emb_f32, void* lc_bf16, int B,
                                             int N, int D, void* stream) {
  VBX_REQUIRE(out_bf16 && lc_bf16, "vbx_pack_phoneme_latent_train: null pointer");
  return pack_phoneme_latent("vbx_pack_phoneme_latent_train", ids, table, E, latent, S, L, w_f16, bias, cond_mask, drop_mask, null_cond,
                             out_f16, out_bf16, emb_f32, lc_bf16, B, N, D, stream);
}
