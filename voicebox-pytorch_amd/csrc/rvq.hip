// Residual vector quantizer (voicebox_pytorch_amd.ResidualVQ / EncodecVocoCodec; the RVQ of EnCodec as the reference's EncodecVoco
// uses it, voicebox_pytorch.py:551-592): the nearest-codeword search of decode_to_codes and the gather-sum of
// Vocos.codes_to_features / EncodecWrapper's get_emb_from_indices.
//
//   vbx_rvq_norms    |c|^2 of every codeword, fp32 [Q, K] (once per codebook version)
//   vbx_rvq_encode   per frame r_0 = x;  code_q = argmin_k |c_qk|^2 - 2 r_q . c_qk (lowest index on an exact tie);
//                    r_{q+1} = r_q - c_q[code_q];  quantized = c_0[code_0] + c_1[code_1] + ...
//   vbx_rvq_decode   the gather-sum alone, row-major or channel-first
//
// The search is fp32 throughout.  The dot products run on v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain at
// the fp32 vector rate: codewords on the rows, the tile's 32 frames on the columns, so a lane holds 16 candidates of ONE frame
// and the running (min, index) never leaves the lane inside a stage.  The k order is lane half h, step s -> component h * D / 2 + s:
// the same order for every codeword, so duplicated codewords give identical distances and the tie rule decides.
//
// A workgroup owns 32 frames for all Q stages.  Its residual tile stays in the LDS; the stage's codebook streams through two LDS
// buffers of CH codewords: of the workgroup's eight waves, four multiply the current chunk while the other four fetch the next
// one (every workgroup reads the same codebook: L2 traffic).  Wave w < 4 multiplies codewords [32 w, 32 w + 32) of a chunk.  Rows are padded by 4 floats, so the 16
// lanes of a ds_read_b128 group fall on 16 different 16-byte slots ((D + 4) / 4 is odd).  No atomics, no host synchronisation:
// the same bits on every run.
#include <atomic>

#include "common.hpp"

namespace {

constexpr int RQ_T = 32;        // frames per workgroup = columns of one MFMA
constexpr int RQ_PAD = 4;       // floats of padding per LDS row
constexpr int RQ_NV = 16;       // float4 a loading thread moves per chunk: CH * D / 4 <= 256 * RQ_NV
constexpr int RQ_LDS_MAX = 160 * 1024;

__host__ __device__ inline int rq_ld(int D) { return D + RQ_PAD; }
// LDS floats: residual tile, two codebook buffers and their |c|^2, the tile's codes [32][Q], the cross-wave (distance, index) pairs [4][32]
__host__ __device__ inline size_t rq_lds_bytes(int D, int Q, int CH) {
  return ((size_t)(RQ_T + 2 * CH) * rq_ld(D) + 2 * CH + (size_t)RQ_T * Q + 2 * 4 * RQ_T) * sizeof(float);
}
inline int rq_chunk(int D, int Q) {  // the largest of 128 / 64 / 32 codewords whose two buffers fit beside the residual tile
  for (int ch = 128; ch > 32; ch >>= 1)
    if (rq_lds_bytes(D, Q, ch) <= (size_t)RQ_LDS_MAX && (long)ch * D / 4 <= 256L * RQ_NV) return ch;
  return 32;
}

// (d, i) <- the better of (d, i) and (od, oi): the smaller distance, the lower index on an exact tie
VBX_DEV void rq_take(float& d, int& i, float od, int oi) {
  if (od < d || (od == d && oi < i)) { d = od; i = oi; }
}

__global__ __launch_bounds__(256) void rvq_norms_kernel(const float* __restrict__ cb, float* __restrict__ norms, int rows, int D) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float4* c = reinterpret_cast<const float4*>(cb + (long)r * D);
  float s = 0.f;
  for (int i = 0; i < D / 4; i++) {
    const float4 v = c[i];
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  norms[r] = s;
}

__global__ __launch_bounds__(512) void rvq_encode_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                         const float* __restrict__ norms, long* __restrict__ codes,
                                                         float* __restrict__ quant, long M, int N, int D, int K, int Q, int CH,
                                                         int codes_qn) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ld = rq_ld(D), D4 = D >> 2;
  float* res = lds;                                 // [32][ld]
  float* buf = res + RQ_T * ld;                     // [2][CH][ld]
  float* nbuf = buf + 2 * CH * ld;                  // [2][CH] the chunk's |c|^2
  int* tcodes = reinterpret_cast<int*>(nbuf + 2 * CH);  // [32][Q]
  float* red_d = reinterpret_cast<float*>(tcodes + RQ_T * Q);  // [4][32]
  int* red_i = reinterpret_cast<int*>(red_d + 4 * RQ_T);        // [4][32]
  const long m0 = (long)blockIdx.x * RQ_T;
  const int nch = (K + CH - 1) / CH, total = Q * nch;
  const int per_chunk = CH * D4;  // float4 of one chunk
  const int bpc = CH >> 5;        // 32-codeword blocks per chunk = waves that multiply
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const f32x4 zerov = {0.f, 0.f, 0.f, 0.f};

  // Waves 0 .. 3 multiply, waves 4 .. 7 load: a SIMD holds one of each, so the address arithmetic and the LDS stores of the next
  // chunk issue in the shadow of the other wave's MFMAs.  A chunk is CH contiguous rows of the codebook: float4 e of the chunk
  // comes from float4 k0 * D4 + e of the stage's table and goes to row e / D4 of the padded LDS image (offsets fixed per thread,
  // taken once); rows past K are written as zeros (a fetch past the table reads its last float4, always a valid address).
  const bool loader = wave >= 4;
  const int ltid = tid - 256;
  int loff[RQ_NV];
#pragma unroll
  for (int j = 0; j < RQ_NV; j++) {
    const int e = j * 256 + (ltid < 0 ? 0 : ltid);
    loff[j] = 4 * e + (e / D4) * RQ_PAD;
  }
  const int table4 = K * D4;  // <= 4096 * 64
  // The loaders run one chunk ahead of their own stores: RQ_FETCH(g + 2) is issued right after RQ_STAGE(g + 1), so a fetch has a
  // whole chunk of multiplication to land.  Nothing reads the fetched registers before RQ_STAGE (a select there would put the
  // wait behind the fetch).  `full` (the same for every thread): the chunk lies inside the table, so an index clamped to the chunk (its float4 count need
  // not be a multiple of 256) is inside the table too, and no zeros are needed.
  f32x4 pre[RQ_NV];  // native vectors: they stay in registers
  float pren = 0.f;  // |c|^2 of codeword k0 + ltid of the chunk
#define RQ_FETCH(g_)                                                                                    \
  do {                                                                                                  \
    const int q_ = (g_) / nch, k0_ = ((g_) - q_ * nch) * CH, e0_ = k0_ * D4;                            \
    const f32x4* src_ = reinterpret_cast<const f32x4*>(cb) + (long)q_ * table4;                         \
    if (k0_ + CH <= K) {                                                                                \
      _Pragma("unroll") for (int j = 0; j < RQ_NV; j++)                                                 \
        if (j * 256 < per_chunk) pre[j] = src_[e0_ + min(j * 256 + ltid, per_chunk - 1)]; /* in the chunk */ \
      pren = norms[(long)q_ * K + k0_ + (ltid < CH ? ltid : 0)];                                        \
    } else {                                                                                            \
      _Pragma("unroll") for (int j = 0; j < RQ_NV; j++) {                                               \
        const int i_ = e0_ + j * 256 + ltid;                                                            \
        if (j * 256 < per_chunk) pre[j] = src_[i_ < table4 ? i_ : table4 - 1];                          \
      }                                                                                                 \
      pren = norms[(long)q_ * K + (k0_ + ltid < K ? k0_ + ltid : K - 1)];                               \
    }                                                                                                   \
  } while (0)
#define RQ_STAGE(g_)                                                                                    \
  do {                                                                                                  \
    const int k0_ = ((g_) % nch) * CH, e0_ = k0_ * D4;                                                  \
    float* dst_ = buf + ((g_) & 1) * CH * ld;                                                           \
    if (k0_ + CH <= K) {                                                                                \
      _Pragma("unroll") for (int j = 0; j < RQ_NV; j++)                                                 \
        if (j * 256 + ltid < per_chunk) *reinterpret_cast<f32x4*>(dst_ + loff[j]) = pre[j];             \
    } else {                                                                                            \
      _Pragma("unroll") for (int j = 0; j < RQ_NV; j++)                                                 \
        if (j * 256 + ltid < per_chunk)                                                                 \
          *reinterpret_cast<f32x4*>(dst_ + loff[j]) = e0_ + j * 256 + ltid < table4 ? pre[j] : zerov;   \
    }                                                                                                   \
    if (ltid < CH) nbuf[((g_) & 1) * CH + ltid] = pren;                                                 \
  } while (0)

  for (int e = tid; e < RQ_T * D4; e += 512) {  // the residual tile r_0 = x; frames past M are zeros (their codes are not stored)
    const int f = e / D4, c4 = e - f * D4;
    *reinterpret_cast<float4*>(res + f * ld + 4 * c4) = m0 + f < M ? reinterpret_cast<const float4*>(x + (m0 + f) * D)[c4] : zero4;
  }
  if (loader) {
    RQ_FETCH(0);
    RQ_STAGE(0);
    if (total > 1) RQ_FETCH(1);
  }
  __syncthreads();

  const int fr = lane & 31, h = lane >> 5;
  for (int q = 0; q < Q; q++) {
    float best = __builtin_inff();
    int bidx = 0;
    for (int c = 0; c < nch; c++) {
      const int g = q * nch + c;
      if (loader) {
        if (g + 1 < total) RQ_STAGE(g + 1);  // into the buffer that chunk g - 1 was read from, before the last barrier
        if (g + 2 < total) RQ_FETCH(g + 2);
      } else if (wave < bpc) {
        const int kb = c * CH + wave * 32;  // first codeword of this wave's block
        const float* ap = buf + (g & 1) * CH * ld + (wave * 32 + fr) * ld + h * (D >> 1);
        const float* bp = res + fr * ld + h * (D >> 1);
        const float* nb = nbuf + (g & 1) * CH + wave * 32;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // one step ahead: the reads of step t + 1 are in flight under the four MFMAs of step t (the read past the last step lands
        // in the row's padding or the next row, inside the LDS, and is not used)
        float4 a = *reinterpret_cast<const float4*>(ap), b = *reinterpret_cast<const float4*>(bp);
        for (int t = 0; t < (D >> 3); t++) {
          const float4 an = *reinterpret_cast<const float4*>(ap + 4 * t + 4);
          const float4 bn = *reinterpret_cast<const float4*>(bp + 4 * t + 4);
          __builtin_amdgcn_sched_barrier(0);  // keep the reads of step t + 1 in front of the MFMAs of step t
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
          a = an;
          b = bn;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {  // ascending k inside the lane: a strict < keeps the lowest index
          const int k = kb + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float d = fmaf(-2.0f, acc[r], nb[k - kb]);
          if (k < K && d < best) { best = d; bidx = k; }
        }
      }
      __syncthreads();
    }
    // the frame's two lane halves, then the waves
    rq_take(best, bidx, __shfl_xor(best, 32, 64), __shfl_xor(bidx, 32, 64));
    if (!loader && lane < 32) { red_d[wave * RQ_T + lane] = best; red_i[wave * RQ_T + lane] = bidx; }
    __syncthreads();
    if (tid < RQ_T) {
      float d = red_d[tid];
      int i = red_i[tid];
      for (int w = 1; w < bpc; w++) rq_take(d, i, red_d[w * RQ_T + tid], red_i[w * RQ_T + tid]);
      tcodes[tid * Q + q] = i;
    }
    __syncthreads();
    if (q + 1 < Q) {
      const float4* cq = reinterpret_cast<const float4*>(cb + (long)q * K * D);
      for (int e = tid; e < RQ_T * D4; e += 512) {
        const int f = e / D4, c4 = e - f * D4;
        float4* rp = reinterpret_cast<float4*>(res + f * ld + 4 * c4);
        float4 r = *rp;
        const float4 cw = cq[(long)tcodes[f * Q + q] * D4 + c4];
        r.x -= cw.x; r.y -= cw.y; r.z -= cw.z; r.w -= cw.w;
        *rp = r;
      }
      __syncthreads();
    }
  }

  for (int e = tid; e < RQ_T * Q; e += 512) {
    int f, q;
    if (codes_qn) { q = e / RQ_T; f = e - q * RQ_T; } else { f = e / Q; q = e - f * Q; }  // consecutive lanes, consecutive addresses
    const long m = m0 + f;
    if (m >= M) continue;
    const long b = m / N, n = m - b * N;
    codes[codes_qn ? (b * Q + q) * N + n : m * Q + q] = tcodes[f * Q + q];
  }
  if (quant) {
    for (int e = tid; e < RQ_T * D4; e += 512) {
      const int f = e / D4, c4 = e - f * D4;
      if (m0 + f >= M) continue;
      float4 a = reinterpret_cast<const float4*>(cb)[(long)tcodes[f * Q] * D4 + c4];
      for (int q = 1; q < Q; q++) {
        const float4 cw = reinterpret_cast<const float4*>(cb + (long)q * K * D)[(long)tcodes[f * Q + q] * D4 + c4];
        a.x += cw.x; a.y += cw.y; a.z += cw.z; a.w += cw.w;
      }
      reinterpret_cast<float4*>(quant + (m0 + f) * D)[c4] = a;
    }
  }
}

// A workgroup sums the codewords of 32 consecutive frames.  Row-major output goes straight to memory; channel-first output
// [B, D, N] crosses a [32][D + 1] LDS tile so that consecutive lanes store consecutive frames.
__global__ __launch_bounds__(256) void rvq_decode_kernel(const long* __restrict__ codes, const float* __restrict__ cb,
                                                         float* __restrict__ out, long M, int N, int D, int K, int Q, int codes_qn,
                                                         int ch_first) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // ch_first: [32][D + 1]
  const int tid = threadIdx.x, D4 = D >> 2;
  const long m0 = (long)blockIdx.x * RQ_T;
  for (int e = tid; e < RQ_T * D4; e += 256) {
    const int f = e / D4, c4 = e - f * D4;
    const long m = m0 + f;
    if (m >= M) continue;
    const long b = m / N, n = m - b * N;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < Q; q++) {
      const long k = codes[codes_qn ? (b * Q + q) * N + n : m * Q + q];
      if (k < 0 || k >= K) continue;  // contributes zero, never dereferenced
      const float4 cw = reinterpret_cast<const float4*>(cb + (long)q * K * D)[k * D4 + c4];
      a.x += cw.x; a.y += cw.y; a.z += cw.z; a.w += cw.w;
    }
    if (ch_first) {
      float* t = tile + f * (D + 1) + 4 * c4;
      t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
      reinterpret_cast<float4*>(out + m * D)[c4] = a;
    }
  }
  if (!ch_first) return;
  __syncthreads();
  for (int e = tid; e < RQ_T * D; e += 256) {
    const int d = e / RQ_T, f = e - d * RQ_T;
    const long m = m0 + f;
    if (m >= M) continue;
    const long b = m / N, n = m - b * N;
    out[(b * D + d) * N + n] = tile[f * (D + 1) + d];
  }
}

int rq_check(int D, int K, int Q, long M, int N, const char* who) {
  VBX_REQUIRE(D >= 8 && D <= 256 && D % 8 == 0, "%s: dim must be a multiple of 8 in 8 .. 256 (got %d)", who, D);
  VBX_REQUIRE(K >= 2 && K <= 4096, "%s: codebook_size must be in 2 .. 4096 (got %d)", who, K);
  VBX_REQUIRE(Q >= 1 && Q <= 32, "%s: num_quantizers must be in 1 .. 32 (got %d)", who, Q);
  VBX_REQUIRE(M >= 1 && N >= 1 && M % N == 0, "%s: need B >= 1 and N >= 1", who);
  VBX_REQUIRE((M + RQ_T - 1) / RQ_T < (1L << 31), "%s: too many frames", who);
  return 0;
}

#undef RQ_FETCH
#undef RQ_STAGE

}  // namespace

extern "C" int vbx_rvq_norms(const float* codebooks, float* norms, int Q, int K, int D, void* stream) {
  VBX_REQUIRE(codebooks && norms, "vbx_rvq_norms: null operand");
  if (int rc = rq_check(D, K, Q, 1, 1, "vbx_rvq_norms")) return rc;
  hipLaunchKernelGGL(rvq_norms_kernel, dim3(cdiv((long)Q * K, 256)), dim3(256), 0, (hipStream_t)stream, codebooks, norms, Q * K, D);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_rvq_encode(const float* x, const float* codebooks, const float* norms, long* codes, float* quantized, int B, int N,
                              int D, int K, int Q, int codes_qn, void* stream) {
  VBX_REQUIRE(x && codebooks && norms && codes, "vbx_rvq_encode: null operand");
  VBX_REQUIRE(B >= 1 && N >= 1, "vbx_rvq_encode: need B >= 1 and N >= 1");
  const long M = (long)B * N;
  if (int rc = rq_check(D, K, Q, M, N, "vbx_rvq_encode")) return rc;
  const int CH = rq_chunk(D, Q);
  const size_t bytes = rq_lds_bytes(D, Q, CH);
  VBX_REQUIRE(bytes <= (size_t)RQ_LDS_MAX && (long)CH * D / 4 <= 256L * RQ_NV, "vbx_rvq_encode: the tile does not fit the LDS");
  // more than 64 KiB of dynamic LDS has to be allowed once per device; a repeated call from a second thread is harmless
  static std::atomic<unsigned long long> allowed{0};
  int dev = 0;
  VBX_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "vbx_rvq_encode: no current device");
  if (!(allowed.load(std::memory_order_acquire) >> dev & 1)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rvq_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       RQ_LDS_MAX);
    VBX_REQUIRE(e == hipSuccess, "vbx_rvq_encode: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    allowed.fetch_or(1ull << dev, std::memory_order_release);
  }
  hipLaunchKernelGGL(rvq_encode_kernel, dim3(cdiv(M, RQ_T)), dim3(512), bytes, (hipStream_t)stream, x, codebooks, norms, codes,
                     quantized, M, N, D, K, Q, CH, codes_qn ? 1 : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_rvq_decode(const long* codes, const float* codebooks, float* out, int B, int N, int D, int K, int Q, int codes_qn,
                              int channel_first, void* stream) {
  VBX_REQUIRE(codes && codebooks && out, "vbx_rvq_decode: null operand");
  VBX_REQUIRE(B >= 1 && N >= 1, "vbx_rvq_decode: need B >= 1 and N >= 1");
  const long M = (long)B * N;
  if (int rc = rq_check(D, K, Q, M, N, "vbx_rvq_decode")) return rc;
  const size_t bytes = channel_first ? (size_t)RQ_T * (D + 1) * sizeof(float) : 0;
  hipLaunchKernelGGL(rvq_decode_kernel, dim3(cdiv(M, RQ_T)), dim3(256), bytes, (hipStream_t)stream, codes, codebooks, out, M, N, D, K,
                     Q, codes_qn ? 1 : 0, channel_first ? 1 : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}
