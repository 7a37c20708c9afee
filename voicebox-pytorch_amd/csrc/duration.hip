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
