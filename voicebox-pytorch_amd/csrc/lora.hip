// LoRA adapters on the fp32 master weights (voicebox_pytorch_amd/lora.py, dp.TrainStep): the adapted matrix lives in its own slot of
// the flat parameter buffer as W = W0 + s . B . A (A [r, K], B [N, r], s = alpha / r), so every forward, backward and sampler kernel
// serves the adapted model from the packed copies it already reads.  Two grouped entry points over one device descriptor table
// (all targets of all layers; a step adds three launches, not 4 L):
//
//   vbx_lora_apply   W[n, k] = fmaf(s, sum_j B[n, j] A[j, k], W0[n, k])      (j ascending, one fmaf chain per element)
//   vbx_lora_grad    dB[n, j] = s . sum_k dW[n, k] A[j, k],   dA[j, k] = s . sum_n B[n, j] dW[n, k]   from the dW [N, K] the unchanged
//                    backward left in the frozen weight's range of the gradient buffer
//
// fp32 fmaf chains on the vector ALU, not the fp32 MFMA: at r <= 64 the arithmetic is 4 r flops per dW element read (2.4 GFLOP per
// step at dim 512 / depth 12 / r = 16), under a tenth of what the HBM read of dW costs in time, the chains give the contract's
// summation order directly, and ranks that are no multiple of the MFMA's k need no padding rules.
//
// vbx_lora_grad reads dW from HBM once.  A workgroup owns a tile of LG_ROWS rows x LG_COLS columns of one matrix and walks it in
// sub-blocks of 32 rows: thread t loads column t of the sub-block (32 coalesced row reads) into the LDS, reads it back for the dA
// products (its own column: sum over the tile's rows, kept in RP accumulators across the sub-blocks) and shares it for
// the dB products (each wave sums over 64 of the tile's 256 columns, the waves' partials are added in wave order).  The tile leaves a
// partial dA [r, LG_COLS] per row tile and a partial dB [32, r] per column tile in scratch; lora_reduce_kernel sums the partials in
// ascending tile order and applies s.  No atomics: the same bits on every run, and a matrix's result does not depend on the other
// entries of the table.
#include "common.hpp"

namespace {

constexpr int LA_ROWS = 32;    // rows of W per workgroup of vbx_lora_apply
constexpr int LG_ROWS = 128;   // rows of dW per tile of vbx_lora_grad
constexpr int LG_COLS = 256;   // columns per tile = threads per workgroup
constexpr int LG_SUB = 32;     // rows per sub-block
constexpr int LG_LD = LG_COLS + 4;  // LDS row stride (floats): 16-byte aligned rows, rows 4 banks apart
constexpr int LORA_MAX_RANK = 64;

VBX_DEV int lora_cdiv(int a, int b) { return (a + b - 1) / b; }
// the descriptor whose [first, first + count) interval of a grid prefix holds `idx`: last d with key(d) <= idx
template <typename KeyFn>
VBX_DEV int lora_find(int n, long idx, KeyFn key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key(mid) <= idx) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void lora_apply_kernel(float* __restrict__ flat, const float* __restrict__ w0,
                                                         const float* __restrict__ lflat, const vbx_lora_desc* __restrict__ descs, int n) {
  __shared__ float Bs[LA_ROWS][LORA_MAX_RANK];
  const int di = lora_find(n, (long)blockIdx.x, [&](int d) { return descs[d].blk0; });
  const vbx_lora_desc d = descs[di];
  const int n0 = (int)((long)blockIdx.x - d.blk0) * LA_ROWS;
  const int k = blockIdx.y * 256 + threadIdx.x;
  if ((long)blockIdx.y * 256 >= d.K) return;  // (block-uniform: the grid's y extent is the widest matrix of the table)
  const float* A = lflat + d.a_off;
  const float* B = lflat + d.b_off;
  for (int i = threadIdx.x; i < LA_ROWS * d.r; i += 256) {
    const int rn = i / d.r, j = i - rn * d.r;
    Bs[rn][j] = n0 + rn < d.N ? B[(long)(n0 + rn) * d.r + j] : 0.f;
  }
  __syncthreads();
  if (k >= d.K) return;
  float acc[LA_ROWS];
#pragma unroll
  for (int rn = 0; rn < LA_ROWS; rn++) acc[rn] = 0.f;
  for (int j = 0; j < d.r; j++) {
    const float a = A[(long)j * d.K + k];
#pragma unroll
    for (int rn = 0; rn < LA_ROWS; rn++) acc[rn] = fmaf(Bs[rn][j], a, acc[rn]);
  }
  const float* src = w0 + d.w0_off;
  float* dst = flat + d.w_off;
#pragma unroll
  for (int rn = 0; rn < LA_ROWS; rn++) {
    if (n0 + rn < d.N) {
      const long o = (long)(n0 + rn) * d.K + k;
      const float w = src[o];
      dst[o] = acc[rn] == 0.f ? w : fmaf(d.scale, acc[rn], w);  // (B = 0: the bits of W0, its signed zeros included)
    }
  }
}

// RP: the table's largest rank rounded up to 8 / 16 / 32 / 64; ranks past a matrix's own r multiply zeros and are not stored.
// The next sub-block's column of dW is loaded into registers before the current one is multiplied: without it the HBM latency of
// every sub-block stood between two barriers and the launch took 220 us instead of 117 us (profiles/finetune_kernel_stats.txt).
// dA: thread t owns column t of the tile, rows ascending; B[n, j] is a broadcast read of the sub-block's rows in the LDS.
// dB: wave w takes columns [64 w, 64 w + 64) of the tile; lane (row pair p, rank quarter q) holds rows 2 p, 2 p + 1 x ranks q + 4 i
// in registers (2 + RP / 4 LDS reads of 16 bytes per 2 RP fused multiply-adds); the four waves' partials meet in the LDS and are
// added in wave order.
template <int RP>
__global__ __launch_bounds__(256) void lora_grad_kernel(const float* __restrict__ gflat, const float* __restrict__ lflat,
                                                        const vbx_lora_desc* __restrict__ descs, int n, float* __restrict__ scratch) {
  constexpr int NJ = RP / 4;  // ranks per lane in the dB products
  __shared__ __attribute__((aligned(16))) float dws[LG_SUB][LG_LD];
  __shared__ __attribute__((aligned(16))) float As[RP][LG_LD];
  __shared__ __attribute__((aligned(16))) float Bs[LG_SUB][RP];
  __shared__ float pbs[4][LG_SUB][RP + 1];
  const int di = lora_find(n, (long)blockIdx.x, [&](int d) { return descs[d].tile0; });
  const vbx_lora_desc d = descs[di];
  const int kt = lora_cdiv(d.K, LG_COLS);
  const int t = (int)((long)blockIdx.x - d.tile0);
  const int rt = t / kt, ct = t - rt * kt;  // row tile, column tile
  const int tid = threadIdx.x;
  const int k = ct * LG_COLS + tid;
  const bool kin = k < d.K;
  const float* A = lflat + d.a_off;
  const float* B = lflat + d.b_off;
  const float* dW = gflat + d.w_off;
  for (int j = 0; j < RP; j++) As[j][tid] = (j < d.r && kin) ? A[(long)j * d.K + k] : 0.f;
  float accA[RP];
#pragma unroll
  for (int j = 0; j < RP; j++) accA[j] = 0.f;
  const int wave = tid >> 6, lane = tid & 63;
  const int rp = lane >> 2, jq = lane & 3;  // dB products: rows 2 rp, 2 rp + 1 of the sub-block, ranks jq + 4 i
  float* pb = scratch + d.pb_off + (long)ct * d.N * d.r;
  const int rows_end = min(d.N, (rt + 1) * LG_ROWS);
  float pre[LG_SUB];  // this thread's column of the sub-block to come
#pragma unroll
  for (int rn = 0; rn < LG_SUB; rn++) pre[rn] = (kin && rt * LG_ROWS + rn < d.N) ? dW[(long)(rt * LG_ROWS + rn) * d.K + k] : 0.f;
  for (int n0 = rt * LG_ROWS; n0 < rows_end; n0 += LG_SUB) {
    __syncthreads();  // the previous sub-block's readers of dws / Bs / pbs are done (first pass: As is complete after the next barrier)
    for (int i = tid; i < LG_SUB * RP; i += 256) {
      const int rn = i / RP, j = i - rn * RP;
      Bs[rn][j] = (j < d.r && n0 + rn < d.N) ? B[(long)(n0 + rn) * d.r + j] : 0.f;
    }
#pragma unroll
    for (int rn = 0; rn < LG_SUB; rn++) dws[rn][tid] = pre[rn];
    const int n1 = n0 + LG_SUB;
    if (n1 < rows_end) {
#pragma unroll
      for (int rn = 0; rn < LG_SUB; rn++) pre[rn] = (kin && n1 + rn < d.N) ? dW[(long)(n1 + rn) * d.K + k] : 0.f;
    }
    __syncthreads();
    // dA: this thread's column (read back from its own LDS slots), rows ascending
#pragma unroll 2
    for (int rn = 0; rn < LG_SUB; rn++) {
      const float w = dws[rn][tid];
#pragma unroll
      for (int j4 = 0; j4 < RP; j4 += 4) {
        const float4 b = *reinterpret_cast<const float4*>(&Bs[rn][j4]);
        accA[j4 + 0] = fmaf(b.x, w, accA[j4 + 0]);
        accA[j4 + 1] = fmaf(b.y, w, accA[j4 + 1]);
        accA[j4 + 2] = fmaf(b.z, w, accA[j4 + 2]);
        accA[j4 + 3] = fmaf(b.w, w, accA[j4 + 3]);
      }
    }
    // dB: this wave's 64 columns, ascending
    float acc0[NJ], acc1[NJ];
#pragma unroll
    for (int i = 0; i < NJ; i++) acc0[i] = acc1[i] = 0.f;
    for (int c = wave * 64; c < wave * 64 + 64; c += 4) {
      const float4 w0 = *reinterpret_cast<const float4*>(&dws[2 * rp][c]);
      const float4 w1 = *reinterpret_cast<const float4*>(&dws[2 * rp + 1][c]);
#pragma unroll
      for (int i = 0; i < NJ; i++) {
        const float4 a = *reinterpret_cast<const float4*>(&As[jq + 4 * i][c]);
        acc0[i] = fmaf(w0.x, a.x, acc0[i]);
        acc0[i] = fmaf(w0.y, a.y, acc0[i]);
        acc0[i] = fmaf(w0.z, a.z, acc0[i]);
        acc0[i] = fmaf(w0.w, a.w, acc0[i]);
        acc1[i] = fmaf(w1.x, a.x, acc1[i]);
        acc1[i] = fmaf(w1.y, a.y, acc1[i]);
        acc1[i] = fmaf(w1.z, a.z, acc1[i]);
        acc1[i] = fmaf(w1.w, a.w, acc1[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < NJ; i++) {
      pbs[wave][2 * rp][jq + 4 * i] = acc0[i];
      pbs[wave][2 * rp + 1][jq + 4 * i] = acc1[i];
    }
    __syncthreads();
    for (int o = tid; o < LG_SUB * RP; o += 256) {
      const int rn = o / RP, j = o - rn * RP;
      if (j < d.r && n0 + rn < d.N)
        pb[(long)(n0 + rn) * d.r + j] = ((pbs[0][rn][j] + pbs[1][rn][j]) + pbs[2][rn][j]) + pbs[3][rn][j];
    }
  }
  if (kin) {
    float* pa = scratch + d.pa_off + (long)rt * d.r * d.K;
#pragma unroll
    for (int j = 0; j < RP; j++)
      if (j < d.r) pa[(long)j * d.K + k] = accA[j];
  }
}

// dA[j, k] = s . sum over row tiles, dB[n, j] = s . sum over column tiles, both in ascending tile order
__global__ __launch_bounds__(256) void lora_reduce_kernel(const vbx_lora_desc* __restrict__ descs, int n, const float* __restrict__ scratch,
                                                          float* __restrict__ glflat) {
  const int di = lora_find(n, (long)blockIdx.x, [&](int d) { return descs[d].red0; });
  const vbx_lora_desc d = descs[di];
  const long e = ((long)blockIdx.x - d.red0) * 256 + threadIdx.x;
  const long na = (long)d.r * d.K, nb = (long)d.N * d.r;
  if (e < na) {
    const int rtiles = lora_cdiv(d.N, LG_ROWS);
    const float* p = scratch + d.pa_off + e;
    float s = 0.f;
    for (int i = 0; i < rtiles; i++) s += p[(long)i * na];
    glflat[d.a_off + e] = d.scale * s;
  } else if (e < na + nb) {
    const int ctiles = lora_cdiv(d.K, LG_COLS);
    const float* p = scratch + d.pb_off + (e - na);
    float s = 0.f;
    for (int i = 0; i < ctiles; i++) s += p[(long)i * nb];
    glflat[d.b_off + (e - na)] = d.scale * s;
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

// Validates a HOST descriptor table against the sizes of the buffers it indexes and fills its launch fields.
extern "C" int vbx_lora_plan(vbx_lora_desc* descs, int n, long flat_floats, long w0_floats, long lflat_floats, long* apply_blocks,
                             long* grad_tiles, long* reduce_blocks, long* scratch_floats, int* max_rank, int* max_k) {
  VBX_REQUIRE(descs && n > 0 && apply_blocks && grad_tiles && reduce_blocks && scratch_floats && max_rank && max_k, "vbx_lora_plan: bad args");
  long blk = 0, tile = 0, red = 0, scr = 0;
  int mr = 0, mk = 0;
  for (int i = 0; i < n; i++) {
    vbx_lora_desc& d = descs[i];
    VBX_REQUIRE(d.N > 0 && d.K > 0 && d.r >= 1 && d.r <= LORA_MAX_RANK, "vbx_lora_plan: entry %d: N %d, K %d, rank %d (rank must be 1 .. 64)",
                i, d.N, d.K, d.r);
    const long nk = (long)d.N * d.K;
    VBX_REQUIRE(d.w_off >= 0 && d.w_off + nk <= flat_floats, "vbx_lora_plan: entry %d: weight range outside the flat buffer", i);
    VBX_REQUIRE(d.w0_off >= 0 && d.w0_off + nk <= w0_floats, "vbx_lora_plan: entry %d: range outside the W0 store", i);
    VBX_REQUIRE(d.a_off >= 0 && d.a_off + (long)d.r * d.K <= lflat_floats && d.b_off >= 0 && d.b_off + (long)d.N * d.r <= lflat_floats,
                "vbx_lora_plan: entry %d: adapter range outside the adapter buffer", i);
    const long rtiles = cdiv(d.N, LG_ROWS), ctiles = cdiv(d.K, LG_COLS);
    d.blk0 = blk;
    d.tile0 = tile;
    d.red0 = red;
    d.pa_off = scr;
    d.pb_off = scr + rtiles * d.r * d.K;
    scr = d.pb_off + ctiles * d.N * d.r;
    blk += cdiv(d.N, LA_ROWS);
    tile += rtiles * ctiles;
    red += cdiv((long)d.r * d.K + (long)d.N * d.r, 256);
    mr = d.r > mr ? d.r : mr;
    mk = d.K > mk ? d.K : mk;
  }
  VBX_REQUIRE(blk < (1L << 31) && tile < (1L << 31) && red < (1L << 31), "vbx_lora_plan: table too large for one launch");
  *apply_blocks = blk; *grad_tiles = tile; *reduce_blocks = red; *scratch_floats = scr; *max_rank = mr; *max_k = mk;
  return 0;
}

extern "C" int vbx_lora_apply(float* flat, const float* w0, const float* lflat, const vbx_lora_desc* descs_dev, int n, long apply_blocks,
                              int max_k, void* stream) {
  VBX_REQUIRE(flat && w0 && lflat && descs_dev && n > 0 && apply_blocks > 0 && apply_blocks < (1L << 31) && max_k > 0,
              "vbx_lora_apply: bad args");
  hipLaunchKernelGGL(lora_apply_kernel, dim3((unsigned)apply_blocks, (unsigned)cdiv(max_k, 256)), dim3(256), 0, ST, flat, w0, lflat,
                     descs_dev, n);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_lora_grad(const float* gflat, const float* lflat, float* glflat, const vbx_lora_desc* descs_dev, int n, long grad_tiles,
                             long reduce_blocks, int max_rank, float* scratch, void* stream) {
  VBX_REQUIRE(gflat && lflat && glflat && descs_dev && scratch && n > 0 && grad_tiles > 0 && grad_tiles < (1L << 31) && reduce_blocks > 0 &&
                  reduce_blocks < (1L << 31) && max_rank >= 1 && max_rank <= LORA_MAX_RANK,
              "vbx_lora_grad: bad args");
  const dim3 grid((unsigned)grad_tiles), block(256);
  if (max_rank <= 8) hipLaunchKernelGGL(lora_grad_kernel<8>, grid, block, 0, ST, gflat, lflat, descs_dev, n, scratch);
  else if (max_rank <= 16) hipLaunchKernelGGL(lora_grad_kernel<16>, grid, block, 0, ST, gflat, lflat, descs_dev, n, scratch);
  else if (max_rank <= 32) hipLaunchKernelGGL(lora_grad_kernel<32>, grid, block, 0, ST, gflat, lflat, descs_dev, n, scratch);
  else hipLaunchKernelGGL(lora_grad_kernel<64>, grid, block, 0, ST, gflat, lflat, descs_dev, n, scratch);
  VBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)reduce_blocks), block, 0, ST, descs_dev, n, scratch, glflat);
  VBX_LAUNCH_CHECK();
  return 0;
}
