// k-means FIT on the device (voicebox_pytorch_amd.KMeans / kmeans_plusplus, voicebox-pytorch_amd/kmeans.py): one step is
// search -> accumulate by id -> update, all fp32 data, no float atomics, no host synchronisation; reruns give the same bits.
//
//   vbx_kmeans_norms        |c|^2 of every centre, a wave per centre (once per step)
//   vbx_kmeans_search       id = argmin_k |c_k|^2 - 2 h . c_k on v_mfma_f32_32x32x2_f32 (the lowest index on an exact tie), then the
//                           row's min distance sum_i (h_i - c_i)^2 by differences; a dead row (n >= lens[b]) is never read: id K
//   vbx_kmeans_accumulate   per-cluster sums [K, D], counts [K] and the inertia: a stable counting sort of the row indices by id,
//                           then sums in an order that depends on the member rows' RANKS inside their cluster only
//   vbx_kmeans_update       c' = (c w + S) / (w + n) (minibatch) or S / n (Lloyd) where n > 0, else c; w' = w + n (or n)
//   vbx_kmeans_plusplus     D^2 sampling (Arthur & Vassilvitskii 2007), one candidate per step, from given uniforms u [K]
//
// SEARCH.  A workgroup of four waves owns RT = 32 rows (16 above D = 1024, where 32 rows no longer fit beside the codebook
// buffers: the MFMA's upper 16 columns then repeat the lower and are ignored).  The row tile stays in the LDS for the whole
// codebook; the codebook streams through two LDS buffers in stages of 128 centres x DC components (DC = 32, or 16 where the
// tile leaves less room): every thread fetches the next stage into registers (its places in a stage never change: no index
// arithmetic in the loop), multiplies the current one and then stores the fetched one, one barrier per stage.  Wave w multiplies
// centres [32 w, 32 w + 32) of the stage: centres on the MFMA's rows, the tile's rows on its columns, so a lane holds 16
// candidates of ONE row and the running (min, index) stays in the lane.  The
// k order of a (row, centre) pair is: D chunks ascending; inside a chunk of dc components lane half h, step s -> component
// h * dc / 2 + s, the two halves interleaved by the MFMA -- the same for every centre and every row, whatever the batch, so
// duplicated centres give identical distances and the tie rule decides.
//
// ACCUMULATE.  ids -> per-tile histograms (integer LDS atomics: the counts do not depend on their order) -> an exclusive scan over
// the tiles per cluster and over the clusters -> a stable scatter: order[] lists the rows of cluster 0 in ascending row index, then
// cluster 1, ...  Cluster k's members, by rank r = 0 .. n_k - 1 in that order, are summed as
//     P_j = ((x_{64 j} + x_{64 j + 1}) + ...) + x_{64 j + 63}        one workgroup per (k, j), left to right
//     S_k = ((P_0 + P_1) + P_2) + ...                                left to right
// per component: a function of the members' ranks alone, not of the tiling, the batch shape or the other clusters.  The min
// distances follow the same route in fp64 (Q_j per (k, j), left to right); the inertia is the sum of all Q in the order
// lane l: Q_l + Q_{l + 64} + ... (ascending), then the xor tree over the 64 lanes.
//
// K-MEANS++.  p_i = min over the chosen rows of sum_d (x_id - x_cd)^2 by differences (a chosen row: exactly 0).  Running sum, fp64:
// block b = rows [64 b, 64 b + 64) has B_b = xor-tree sum of its p; range t (of 1024) = cdiv(blocks, 1024) consecutive blocks, summed
// left to right; the ranges by a Hillis-Steele scan; inside the block an inclusive Hillis-Steele scan over its 64 rows.  The pick is
// the first row with p > 0 whose running sum reaches u_j * total; total == 0 (and step 0): live row number floor(u_j * M_live).
#include <atomic>

#include "common.hpp"

namespace {

constexpr int KM_CH = 128;     // centres per stage = 32 per wave
constexpr int KM_PAD = 4;      // floats of padding per LDS row: (D + 4) / 4 and (DC + 4) / 4 are odd, ds_read_b128 groups do not collide
constexpr int KM_DC = 32;      // the widest D chunk of a stage
constexpr int KM_NV = KM_CH * KM_DC / 4 / 256;  // float4 a thread fetches per stage
constexpr int KM_LDS_MAX = 160 * 1024;
constexpr int KM_MAX_D = 2048, KM_MAX_K = 4096;
constexpr int KM_SEG = 64;     // members per first-level partial sum
constexpr int KM_SORT_TILES = 512;
constexpr int KM_PP_ROWS = 64; // rows per block of the k-means++ running sum

inline int km_tile(int D) { return D <= 1024 ? 32 : 16; }
// LDS bytes: the row tile, two codebook buffers, the cross-wave (distance, index) pairs [4][32], the tile's ids and live flags [32]
inline size_t km_lds_bytes(int D, int RT, int DC) {
  return ((size_t)RT * (D + KM_PAD) + 2 * (size_t)KM_CH * (DC + KM_PAD) + 2 * 4 * 32 + 2 * 32) * sizeof(float);
}
inline int km_dchunk(int D) { return km_lds_bytes(D, km_tile(D), KM_DC) <= (size_t)KM_LDS_MAX ? KM_DC : KM_DC / 2; }

VBX_DEV void km_take(float& d, int& i, float od, int oi) {
  if (od < d || (od == d && oi < i)) { d = od; i = oi; }
}
VBX_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// row m of [B, N] under lens (NULL: every row lives)
VBX_DEV bool km_live(const int* __restrict__ lens, long m, int N) {
  if (!lens) return true;
  const long b = m / N;
  return (int)(m - b * N) < lens[b];
}

// a wave per centre: lane l sums components 4 l + 256 j in ascending j, then the xor tree
__global__ __launch_bounds__(256) void km_norms_kernel(const float* __restrict__ c, float* __restrict__ norms, int K, int D) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= K) return;
  const float* p = c + (long)r * D;
  float a = 0.f;
  for (int i = lane * 4; i < D; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    a = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, a))));
  }
  a = wave_sum(a);
  if (lane == 0) norms[r] = a;
}

// NT steps of four MFMAs with every operand read issued first: the waits then fall one by one in front of the MFMAs
template <int NT>
VBX_DEV void km_mma(const float* ap, const float* bp, f32x16& acc) {
  float4 a[NT], b[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    a[t] = *reinterpret_cast<const float4*>(ap + 4 * t);
    b[t] = *reinterpret_cast<const float4*>(bp + 4 * t);
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].x, b[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].y, b[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].z, b[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].w, b[t].w, acc, 0, 0, 0);
  }
}

__global__ __launch_bounds__(256) void km_search_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                        const float* __restrict__ norms, const int* __restrict__ lens,
                                                        int* __restrict__ ids, float* __restrict__ mind, long M, int N, int D, int K,
                                                        int RT, int DC) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ldh = D + KM_PAD, ldc = DC + KM_PAD, D4 = D >> 2;
  float* tile = lds;                               // [RT][ldh]
  float* cbuf = tile + RT * ldh;                   // [2][128][ldc]
  float* red_d = cbuf + 2 * KM_CH * ldc;           // [4][32]
  int* red_i = reinterpret_cast<int*>(red_d + 4 * 32);  // [4][32]
  int* sid = red_i + 4 * 32;                       // [32]
  int* slive = sid + 32;                           // [32]
  const long m0 = (long)blockIdx.x * RT;
  const f32x4 zerov = {0.f, 0.f, 0.f, 0.f};

  if (tid < 32) slive[tid] = tid < RT && m0 + tid < M && km_live(lens, m0 + tid, N) ? 1 : 0;
  __syncthreads();
  for (int e = tid; e < RT * D4; e += 256) {  // dead rows and rows past M are zeros in the LDS; their memory is never read
    const int f = e / D4, c4 = e - f * D4;
    *reinterpret_cast<f32x4*>(tile + f * ldh + 4 * c4) = slive[f] ? reinterpret_cast<const f32x4*>(x + (m0 + f) * D)[c4] : zerov;
  }

  const int nd = (D + DC - 1) / DC, nk = (K + KM_CH - 1) / KM_CH;
  // stage (kc, dc): centres [128 kc, 128 kc + 128) x components [DC dc, DC dc + dcur).  Float4 e = 256 j + tid of a stage is component
  // group e % (DC / 4) of centre e / (DC / 4), the same place in every stage (taken once); centres past K and components past D are zeros
  const int qs = DC == KM_DC ? 3 : 2;  // log2(DC / 4)
  f32x4 pre[KM_NV];
  int gcode[KM_NV], gcol[KM_NV], goff[KM_NV], loff[KM_NV];
#pragma unroll
  for (int j = 0; j < KM_NV; j++) {
    const int e = j * 256 + tid;
    gcode[j] = e >> qs;
    gcol[j] = 4 * (e & ((1 << qs) - 1));
    goff[j] = gcode[j] * D + gcol[j];
    loff[j] = gcode[j] * ldc + gcol[j];
  }
  auto fetch = [&](int kc, int dc) {
    const int d0 = dc * DC, dcur = min(DC, D - d0), k0 = kc * KM_CH;
    const float* src = cb + (long)k0 * D + d0;
#pragma unroll
    for (int j = 0; j < KM_NV; j++) {
      pre[j] = zerov;
      if (gcode[j] < KM_CH && k0 + gcode[j] < K && gcol[j] < dcur) pre[j] = *reinterpret_cast<const f32x4*>(src + goff[j]);
    }
  };
  auto stage = [&](int buf) {
    float* dst = cbuf + buf * KM_CH * ldc;
#pragma unroll
    for (int j = 0; j < KM_NV; j++)
      if (gcode[j] < KM_CH) *reinterpret_cast<f32x4*>(dst + loff[j]) = pre[j];
  };
  fetch(0, 0);
  stage(0);
  __syncthreads();

  const int fr = lane & 31, h = lane >> 5;
  float best = __builtin_inff();
  int bidx = 0, s = 0;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < nk; kc++) {
    for (int dc = 0; dc < nd; dc++, s++) {
      const int d0 = dc * DC, dcur = min(DC, D - d0), half = dcur >> 1;
      const bool more = dc + 1 < nd || kc + 1 < nk;
      if (more) fetch(dc + 1 < nd ? kc : kc + 1, dc + 1 < nd ? dc + 1 : 0);  // in flight under this stage's MFMAs
      if (dc == 0) {
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
      }
      const float* ap = cbuf + (s & 1) * KM_CH * ldc + (wave * 32 + fr) * ldc + h * half;
      const float* bp = tile + (fr & (RT - 1)) * ldh + d0 + h * half;
      if (dcur == 32) {
        km_mma<4>(ap, bp, acc);
      } else if (dcur == 16) {
        km_mma<2>(ap, bp, acc);
      } else {
        for (int t = 0; t < (dcur >> 3); t++) km_mma<1>(ap + 4 * t, bp + 4 * t, acc);
      }
      if (dc == nd - 1) {
        const int kb = kc * KM_CH + wave * 32;
#pragma unroll
        for (int r = 0; r < 16; r++) {  // ascending k inside the lane: a strict < keeps the lowest index
          const int k = kb + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (k < K) {
            const float d = fmaf(-2.0f, acc[r], norms[k]);
            if (d < best) { best = d; bidx = k; }
          }
        }
      }
      // the buffer the next stage goes to was last read in stage s - 1: every wave has passed the barrier that ended it
      if (more) stage((s + 1) & 1);
      __syncthreads();
    }
  }

  km_take(best, bidx, __shfl_xor(best, 32, 64), __shfl_xor(bidx, 32, 64));  // the row's two lane halves, then the waves
  if (lane < 32) { red_d[wave * 32 + lane] = best; red_i[wave * 32 + lane] = bidx; }
  __syncthreads();
  if (tid < 32) {
    float d = red_d[tid];
    int i = red_i[tid];
    for (int w = 1; w < 4; w++) km_take(d, i, red_d[w * 32 + tid], red_i[w * 32 + tid]);
    sid[tid] = i;
    if (tid < RT && m0 + tid < M) ids[m0 + tid] = slive[tid] ? i : K;
  }
  __syncthreads();
  // the min distance by differences: lane l sums components 4 l + 256 j in ascending j, then the xor tree (vbx_kmeans_assign's order)
  for (int f = wave; f < RT; f += 4) {
    const long m = m0 + f;
    if (m >= M) break;
    float d = 0.f;
    if (slive[f]) {
      const float* c = cb + (long)sid[f] * D;
      float a = 0.f;
      for (int i = lane * 4; i < D; i += 256) {
        const float4 cv = *reinterpret_cast<const float4*>(c + i), hv = *reinterpret_cast<const float4*>(tile + f * ldh + i);
        const float d0 = hv.x - cv.x, d1 = hv.y - cv.y, d2 = hv.z - cv.z, d3 = hv.w - cv.w;
        a = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, a))));
      }
      d = wave_sum(a);
    }
    if (lane == 0) mind[m] = d;
  }
}

// ------------------------------------------------------------------------------------------------ accumulate by id
// tile geometry of the counting sort: at most KM_SORT_TILES tiles of R rows, R a multiple of 256
inline long km_sort_rows(long M) {
  const long per = (M + 256L * KM_SORT_TILES - 1) / (256L * KM_SORT_TILES);
  return 256 * (per < 1 ? 1 : per);
}
inline long km_items(long M, int K) { return K + M / KM_SEG + 1; }  // >= sum_k ceil(n_k / 64)
inline size_t km_align(size_t b) { return (b + 255) & ~(size_t)255; }
struct KmScratch {
  size_t thist, tbase, offsets, segoff, order, dpart, part, bytes;
};
inline KmScratch km_scratch(long M, int D, int K) {
  KmScratch s;
  const long R = km_sort_rows(M), T = (M + R - 1) / R, items = km_items(M, K);
  size_t o = 0;
  s.thist = o; o += km_align((size_t)T * K * sizeof(int));
  s.tbase = o; o += km_align((size_t)T * K * sizeof(int));
  s.offsets = o; o += km_align((size_t)(K + 1) * sizeof(int));
  s.segoff = o; o += km_align((size_t)(K + 1) * sizeof(int));
  s.order = o; o += km_align((size_t)M * sizeof(int));
  s.dpart = o; o += km_align((size_t)items * sizeof(double));
  s.part = o; o += km_align((size_t)items * D * sizeof(float));
  s.bytes = o;
  return s;
}

__global__ __launch_bounds__(256) void km_hist_kernel(const int* __restrict__ ids, int* __restrict__ thist, long M, long R, int K) {
  extern __shared__ int hist[];  // [K]
  for (int k = threadIdx.x; k < K; k += 256) hist[k] = 0;
  __syncthreads();
  const long r0 = (long)blockIdx.x * R, r1 = min(M, r0 + R);
  for (long m = r0 + threadIdx.x; m < r1; m += 256) {
    const int id = ids[m];
    if ((unsigned)id < (unsigned)K) atomicAdd(&hist[id], 1);  // integer: the count does not depend on the order
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) thist[(long)blockIdx.x * K + k] = hist[k];
}

// per cluster: tbase[t][k] <- rows of cluster k in the tiles before t; counts[k] <- all of them
__global__ __launch_bounds__(64) void km_scan_tiles_kernel(const int* __restrict__ thist, int* __restrict__ tbase,
                                                           int* __restrict__ counts, int T, int K) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  int run = 0;
#pragma unroll 8
  for (int t = 0; t < T; t++) {
    const int v = thist[(long)t * K + k];
    tbase[(long)t * K + k] = run;
    run += v;
  }
  counts[k] = run;
}

// one workgroup: offsets[k] = sum of counts before k, segoff[k] = sum of ceil(counts / 64) before k, k = 0 .. K
__global__ __launch_bounds__(1024) void km_scan_clusters_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                                int* __restrict__ segoff, int K) {
  __shared__ int sa[1024], sb[1024];
  const int tid = threadIdx.x;
  int c[4], g[4], ca = 0, ga = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int k = 4 * tid + i;
    c[i] = k < K ? counts[k] : 0;
    g[i] = (c[i] + KM_SEG - 1) / KM_SEG;
    ca += c[i];
    ga += g[i];
  }
  sa[tid] = ca;
  sb[tid] = ga;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int va = tid >= off ? sa[tid - off] : 0, vb = tid >= off ? sb[tid - off] : 0;
    __syncthreads();
    sa[tid] += va;
    sb[tid] += vb;
    __syncthreads();
  }
  int ra = sa[tid] - ca, rb = sb[tid] - ga;  // exclusive
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int k = 4 * tid + i;
    if (k < K) { offsets[k] = ra; segoff[k] = rb; }
    ra += c[i];
    rb += g[i];
  }
  if (tid == 1023) { offsets[K] = sa[1023]; segoff[K] = sb[1023]; }
}

// one wave per tile, 64 rows at a time in ascending order: the lanes that hold the same id take consecutive places in lane order
__global__ __launch_bounds__(64) void km_scatter_kernel(const int* __restrict__ ids, const int* __restrict__ tbase,
                                                        const int* __restrict__ offsets, int* __restrict__ order, long M, long R, int K) {
  extern __shared__ int cur[];  // [K]: the next place of cluster k
  const int lane = threadIdx.x;
  for (int k = lane; k < K; k += 64) cur[k] = offsets[k] + tbase[(long)blockIdx.x * K + k];
  __syncthreads();
  const long r0 = (long)blockIdx.x * R, r1 = min(M, r0 + R);
  for (long base = r0; base < r1; base += 64) {
    const long m = base + lane;
    const int id = m < r1 ? ids[m] : -1;
    const bool act = (unsigned)id < (unsigned)K;
    unsigned long long todo = __ballot(act);
    while (todo) {  // one round per distinct id of the 64 rows; `todo` is the same in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int lid = __shfl(id, leader, 64);
      const bool mine = act && id == lid;
      const unsigned long long same = __ballot(mine);
      const int place = cur[lid];
      __builtin_amdgcn_wave_barrier();
      if (mine) order[place + __popcll(same & ((1ull << lane) - 1ull))] = (int)m;
      if (lane == leader) cur[lid] = place + __popcll(same);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
}

// item -> (cluster k, segment j): P_j of the header, components [256 y, 256 y + 256) per workgroup, and Q_j in fp64
__global__ __launch_bounds__(64) void km_segsum_kernel(const float* __restrict__ x, const float* __restrict__ mind,
                                                       const int* __restrict__ order, const int* __restrict__ offsets,
                                                       const int* __restrict__ segoff, float* __restrict__ part,
                                                       double* __restrict__ dpart, int D, int K) {
  __shared__ int rows[KM_SEG];
  const int item = blockIdx.x, lane = threadIdx.x, D4 = D >> 2;
  if (item >= segoff[K]) return;
  int lo = 0, hi = K;  // segoff[lo] <= item < segoff[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (segoff[mid] <= item) lo = mid; else hi = mid;
  }
  const int start = offsets[lo] + (item - segoff[lo]) * KM_SEG, cnt = min(KM_SEG, offsets[lo + 1] - start);
  rows[lane] = lane < cnt ? order[start + lane] : 0;
  __syncthreads();
  const int c4 = blockIdx.y * 64 + lane;
  if (c4 < D4) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    f32x4 s = x4[(long)rows[0] * D4 + c4];
#pragma unroll 4
    for (int r = 1; r < cnt; r++) s += x4[(long)rows[r] * D4 + c4];
    reinterpret_cast<f32x4*>(part)[(long)item * D4 + c4] = s;
  }
  if (blockIdx.y == 0 && lane == 0) {
    double a = (double)mind[rows[0]];
    for (int r = 1; r < cnt; r++) a += (double)mind[rows[r]];
    dpart[item] = a;
  }
}

// blockIdx.x < K: S_k of the header (zeros for an empty cluster); blockIdx.x == K: the inertia
__global__ __launch_bounds__(64) void km_combine_kernel(const float* __restrict__ part, const double* __restrict__ dpart,
                                                        const int* __restrict__ segoff, float* __restrict__ sums,
                                                        double* __restrict__ inertia64, float* __restrict__ inertia32, int D, int K) {
  const int k = blockIdx.x, lane = threadIdx.x, D4 = D >> 2;
  if (k == K) {
    if (blockIdx.y) return;
    const int n = segoff[K];
    double a = 0.0;
    for (int i = lane; i < n; i += 64) a += dpart[i];
    a = wave_sum_f64(a);
    if (lane == 0) { inertia64[0] = a; inertia32[0] = (float)a; }
    return;
  }
  const int c4 = blockIdx.y * 64 + lane;
  if (c4 >= D4) return;
  const int s0 = segoff[k], s1 = segoff[k + 1];
  const f32x4* p4 = reinterpret_cast<const f32x4*>(part);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (s1 > s0) {
    s = p4[(long)s0 * D4 + c4];
    for (int i = s0 + 1; i < s1; i++) s += p4[(long)i * D4 + c4];
  }
  reinterpret_cast<f32x4*>(sums)[(long)k * D4 + c4] = s;
}

__global__ __launch_bounds__(256) void km_update_kernel(const float* __restrict__ c, const long long* __restrict__ w,
                                                        const float* __restrict__ sums, const int* __restrict__ counts,
                                                        float* __restrict__ c_out, long long* __restrict__ w_out, int K, int D, int lloyd) {
  const int D4 = D >> 2;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)K * D4) return;
  const int k = (int)(e / D4);
  const int n = counts[k];
  const long long wk = w[k];
  f32x4 v = reinterpret_cast<const f32x4*>(c)[e];
  if (n > 0) {
    const f32x4 s = reinterpret_cast<const f32x4*>(sums)[e];
    if (lloyd) {
      v = s / (float)n;
    } else {
      const float wf = (float)wk, wn = (float)(wk + n);
      v = (v * wf + s) / wn;
    }
  }
  reinterpret_cast<f32x4*>(c_out)[e] = v;
  if (e == (long)k * D4) w_out[k] = lloyd ? (long long)n : wk + n;
}

// ------------------------------------------------------------------------------------------------ k-means++
// p <- min(p, |x - x_c|^2) with c = chosen[j] (j == 0: p <- the distance), 0 for a dead row; B_b of the header
__global__ __launch_bounds__(256) void km_pp_dist_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                         const long long* __restrict__ chosen, int j, float* __restrict__ p,
                                                         double* __restrict__ bsum, long M, int N, int D) {
  __shared__ float sp[KM_PP_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xc = x + (long)chosen[j] * D;
  f32x4 cv[KM_MAX_D / 256];
#pragma unroll
  for (int i = 0; i < KM_MAX_D / 256; i++) {
    const int d = lane * 4 + 256 * i;
    cv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (d < D) cv[i] = *reinterpret_cast<const f32x4*>(xc + d);
  }
  const long r0 = (long)blockIdx.x * KM_PP_ROWS;
  for (int q = 0; q < KM_PP_ROWS / 4; q++) {
    const int f = wave * (KM_PP_ROWS / 4) + q;
    const long m = r0 + f;
    float pv = 0.f;
    if (m < M) {  // the same for the whole wave, and so is the row's life
      if (km_live(lens, m, N)) {
        const float* xr = x + m * D;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < KM_MAX_D / 256; i++) {
          const int d = lane * 4 + 256 * i;
          if (d < D) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(xr + d);
            const float d0 = hv.x - cv[i].x, d1 = hv.y - cv[i].y, d2 = hv.z - cv[i].z, d3 = hv.w - cv[i].w;
            a = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, a))));
          }
        }
        const float d = wave_sum(a);
        pv = j == 0 ? d : fminf(p[m], d);
      }
      if (lane == 0) p[m] = pv;
    }
    if (lane == 0) sp[f] = pv;
  }
  __syncthreads();
  if (wave == 0) {
    const double a = wave_sum_f64((double)sp[lane]);
    if (lane == 0) bsum[blockIdx.x] = a;
  }
}

// one workgroup: chosen[j] <- the pick of step j, centers[j] <- that row.  uniform != 0 (step 0): live row floor(u_j * M_live).
__global__ __launch_bounds__(1024) void km_pp_pick_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                          const float* __restrict__ p, const double* __restrict__ bsum,
                                                          const float* __restrict__ u, int j, int uniform,
                                                          long long* __restrict__ chosen, float* __restrict__ centers, long M, int N,
                                                          int D) {
  __shared__ double sc[1024], ts[1024];
  __shared__ int s_first;
  __shared__ long s_row, s_blk;
  __shared__ double s_run;
  const int tid = threadIdx.x;
  const long nb = (M + KM_PP_ROWS - 1) / KM_PP_ROWS, per = (nb + 1023) / 1024;
  double total = 0.0, target = 0.0;
  if (tid == 0) { s_first = 1024; s_row = 0; s_blk = -1; s_run = 0.0; }
  if (!uniform) {
    const long b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    double a = 0.0;
    for (long b = b0; b < b1; b++) a += bsum[b];
    ts[tid] = a;
    sc[tid] = a;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const double v = tid >= off ? sc[tid - off] : 0.0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    total = sc[1023];
    if (!(total > 0.0)) uniform = 1;  // every live row coincides with a chosen one
  }
  __syncthreads();
  if (!uniform) {
    target = (double)u[j] * total;
    if (ts[tid] > 0.0 && sc[tid] >= target) atomicMin(&s_first, tid);
  }
  __syncthreads();
  if (tid == 0) {
    if (uniform) {
      long row = 0;
      if (!lens) {
        long r = (long)((double)u[j] * (double)M);
        row = r < M - 1 ? r : M - 1;
      } else {
        const long B = M / N;
        long live = 0;
        for (long b = 0; b < B; b++) live += min(max(lens[b], 0), N);
        if (live > 0) {
          long r = (long)((double)u[j] * (double)live);
          r = r < live - 1 ? r : live - 1;
          for (long b = 0; b < B; b++) {
            const long l = min(max(lens[b], 0), N);
            if (r < l) { row = b * N + r; break; }
            r -= l;
          }
        }  // no live row at all (undefined, memory-safe): row 0
      }
      s_row = row < 0 ? 0 : row;
    } else {
      int t = s_first;
      if (t == 1024) {  // rounding only: the last range that holds anything
        for (t = 1023; t > 0 && !(ts[t] > 0.0); t--) {}
      }
      double run = t > 0 ? sc[t - 1] : 0.0, run_last = run;
      const long b0 = min(nb, t * per), b1 = min(nb, b0 + per);
      long found = -1, last = b0;
      for (long b = b0; b < b1; b++) {
        const double v = bsum[b];
        if (v > 0.0) {
          last = b;
          run_last = run;
          if (run + v >= target) { found = b; break; }
        }
        run += v;
      }
      if (found < 0) { found = last; run = run_last; }
      s_blk = found;
      s_run = run;
    }
  }
  __syncthreads();
  if (!uniform && tid < 64) {
    const long m = s_blk * KM_PP_ROWS + tid;
    const float pv = m < M ? p[m] : 0.f;
    double a = (double)pv;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double v = __shfl_up(a, off, 64);
      if (tid >= off) a += v;
    }
    const unsigned long long hit = __ballot(pv > 0.f && s_run + a >= target), any = __ballot(pv > 0.f);
    int sel = 0;
    if (hit) sel = __ffsll((long long)hit) - 1;
    else if (any) sel = 63 - __clzll((long long)any);
    if (tid == 0) {
      const long row = s_blk * KM_PP_ROWS + sel;
      s_row = row < M ? row : M - 1;
    }
  }
  __syncthreads();
  const long row = s_row;
  if (tid == 0) chosen[j] = row;
  for (int i = tid; i < D; i += 1024) centers[(long)j * D + i] = x[row * D + i];
}

int km_check(long M, int N, int D, int K, const char* who) {
  VBX_REQUIRE(D >= 8 && D % 8 == 0 && D <= KM_MAX_D, "%s: D must be a multiple of 8 up to %d (got %d)", who, KM_MAX_D, D);
  VBX_REQUIRE(K >= 1 && K <= KM_MAX_K, "%s: K must be in 1 .. %d (got %d)", who, KM_MAX_K, K);
  VBX_REQUIRE(M >= 1 && M < (1L << 31), "%s: need 1 <= rows < 2^31", who);
  VBX_REQUIRE(N >= 1 && M % N == 0, "%s: rows must be B * N with N >= 1", who);
  return 0;
}

}  // namespace

extern "C" int vbx_kmeans_search_tile(int D) { return km_tile(D); }
extern "C" int vbx_kmeans_search_chunk(int D) { return km_dchunk(D); }

extern "C" int vbx_kmeans_norms(const float* centers, float* norms, int K, int D, void* stream) {
  VBX_REQUIRE(centers && norms, "vbx_kmeans_norms: null operand");
  if (int rc = km_check(1, 1, D, K, "vbx_kmeans_norms")) return rc;
  hipLaunchKernelGGL(km_norms_kernel, dim3(cdiv(K, 4)), dim3(256), 0, (hipStream_t)stream, centers, norms, K, D);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_kmeans_search(const float* x, const float* centers, const float* norms, const int* lens, int* ids, float* mind,
                                 long M, int N, int D, int K, void* stream) {
  VBX_REQUIRE(x && centers && norms && ids && mind, "vbx_kmeans_search: null operand");
  if (int rc = km_check(M, N, D, K, "vbx_kmeans_search")) return rc;
  const int RT = km_tile(D), DC = km_dchunk(D);
  const size_t bytes = km_lds_bytes(D, RT, DC);
  VBX_REQUIRE(bytes <= (size_t)KM_LDS_MAX, "vbx_kmeans_search: the tile does not fit the LDS");
  // more than 64 KiB of dynamic LDS has to be allowed once per device; a repeated call from a second thread is harmless
  static std::atomic<unsigned long long> allowed{0};
  int dev = 0;
  VBX_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "vbx_kmeans_search: no current device");
  if (!(allowed.load(std::memory_order_acquire) >> dev & 1)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(km_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       KM_LDS_MAX);
    VBX_REQUIRE(e == hipSuccess, "vbx_kmeans_search: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    allowed.fetch_or(1ull << dev, std::memory_order_release);
  }
  hipLaunchKernelGGL(km_search_kernel, dim3(cdiv(M, RT)), dim3(256), bytes, (hipStream_t)stream, x, centers, norms, lens, ids, mind, M,
                     N, D, K, RT, DC);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" long vbx_kmeans_accumulate_scratch_bytes(long M, int D, int K) {
  if (M < 1 || M >= (1L << 31) || D < 8 || D > KM_MAX_D || D % 8 || K < 1 || K > KM_MAX_K) return -1;
  return (long)km_scratch(M, D, K).bytes;
}

extern "C" int vbx_kmeans_accumulate(const float* x, const int* ids, const float* mind, float* sums, int* counts, double* inertia64,
                                     float* inertia32, void* scratch, long M, int D, int K, void* stream) {
  VBX_REQUIRE(x && ids && mind && sums && counts && inertia64 && inertia32 && scratch, "vbx_kmeans_accumulate: null operand");
  if (int rc = km_check(M, 1, D, K, "vbx_kmeans_accumulate")) return rc;
  const KmScratch s = km_scratch(M, D, K);
  char* base = static_cast<char*>(scratch);
  int* thist = reinterpret_cast<int*>(base + s.thist);
  int* tbase = reinterpret_cast<int*>(base + s.tbase);
  int* offsets = reinterpret_cast<int*>(base + s.offsets);
  int* segoff = reinterpret_cast<int*>(base + s.segoff);
  int* order = reinterpret_cast<int*>(base + s.order);
  double* dpart = reinterpret_cast<double*>(base + s.dpart);
  float* part = reinterpret_cast<float*>(base + s.part);
  const long R = km_sort_rows(M);
  const int T = (int)((M + R - 1) / R), items = (int)km_items(M, K), ych = cdiv(D / 4, 64);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(km_hist_kernel, dim3(T), dim3(256), K * sizeof(int), st, ids, thist, M, R, K);
  hipLaunchKernelGGL(km_scan_tiles_kernel, dim3(cdiv(K, 64)), dim3(64), 0, st, thist, tbase, counts, T, K);
  hipLaunchKernelGGL(km_scan_clusters_kernel, dim3(1), dim3(1024), 0, st, counts, offsets, segoff, K);
  hipLaunchKernelGGL(km_scatter_kernel, dim3(T), dim3(64), K * sizeof(int), st, ids, tbase, offsets, order, M, R, K);
  hipLaunchKernelGGL(km_segsum_kernel, dim3(items, ych), dim3(64), 0, st, x, mind, order, offsets, segoff, part, dpart, D, K);
  hipLaunchKernelGGL(km_combine_kernel, dim3(K + 1, ych), dim3(64), 0, st, part, dpart, segoff, sums, inertia64, inertia32, D, K);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_kmeans_update(const float* centers, const long long* w, const float* sums, const int* counts, float* centers_out,
                                 long long* w_out, int K, int D, int lloyd, void* stream) {
  VBX_REQUIRE(centers && w && sums && counts && centers_out && w_out, "vbx_kmeans_update: null operand");
  VBX_REQUIRE(centers != centers_out && w != w_out, "vbx_kmeans_update: the outputs must be buffers of their own");
  if (int rc = km_check(1, 1, D, K, "vbx_kmeans_update")) return rc;
  hipLaunchKernelGGL(km_update_kernel, dim3(cdiv((long)K * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, centers, w, sums, counts,
                     centers_out, w_out, K, D, lloyd ? 1 : 0);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" long vbx_kmeans_plusplus_blocks(long M) { return M < 1 ? -1 : (M + KM_PP_ROWS - 1) / KM_PP_ROWS; }

extern "C" int vbx_kmeans_plusplus(const float* x, const int* lens, const float* u, float* p, double* bsum, long long* chosen,
                                   float* centers, long M, int N, int D, int K, void* stream) {
  VBX_REQUIRE(x && u && p && bsum && chosen && centers, "vbx_kmeans_plusplus: null operand");
  if (int rc = km_check(M, N, D, K, "vbx_kmeans_plusplus")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)((M + KM_PP_ROWS - 1) / KM_PP_ROWS);
  hipLaunchKernelGGL(km_pp_pick_kernel, dim3(1), dim3(1024), 0, st, x, lens, p, bsum, u, 0, 1, chosen, centers, M, N, D);
  for (int j = 1; j < K; j++) {
    hipLaunchKernelGGL(km_pp_dist_kernel, dim3(nb), dim3(256), 0, st, x, lens, chosen, j - 1, p, bsum, M, N, D);
    hipLaunchKernelGGL(km_pp_pick_kernel, dim3(1), dim3(1024), 0, st, x, lens, p, bsum, u, j, 0, chosen, centers, M, N, D);
  }
  VBX_LAUNCH_CHECK();
  return 0;
}
