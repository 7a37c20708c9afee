// The implicit-GEMM tile core of the convolution families (seanet.hip, hifigan.hip): a workgroup stages a span of a channel-last fp16
// activation in the LDS and multiplies operand rows read IN PLACE from it with an fp16 weight matrix on v_mfma_f32_16x16x32_f16;
// the tile size is picked by the LDS bytes of the span.  Included by each family's translation unit; everything is file-local.
#pragma once
#include <atomic>

#include "common.hpp"

namespace {

constexpr int SN_PADH = 8;              // fp16 elements of padding per LDS row: rows stride * (C + 8) apart spread over the banks
constexpr int SN_LDS_PREF = 80 * 1024;  // the tile grows while two workgroups still share a CU ...
constexpr int SN_LDS_MAX = 160 * 1024;  // ... and the smallest tile may take the whole LDS (512 -> 1024, k 16, s 8: 138 KiB)

// The product both tiled kernels run once their span is staged in the LDS: out[m][n] = sum_kk A[m][kk] w[n][kk] over the tile's MT * 16
// rows m and N columns n, every sum fp32 on v_mfma_f32_16x16x32_f16 in ascending kk.  Work items are (16 columns) x (MG blocks of 16
// rows), dealt to the four waves; the weight fragments come straight from memory (every workgroup reads the same matrix: L2
// traffic).  TAIL: Ktot need not be a multiple of 32, past it a step takes zeros.  rows(kk, base, ld) says where the eight A columns
// from kk on live: row m's at base + m * ld, read in place (no im2col copy anywhere).  store(n)(m, v) is handed every out[m][n], n < N.
template <int MG, bool TAIL, class ARows, class Store>
VBX_DEV void sn_tile_product(const u16* __restrict__ w, int N, int Ktot, int MT, const ARows& rows, const Store& store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NT = (N + 15) >> 4, items = NT * (MT / MG);
  const int fr = lane & 15, g = lane >> 4;
  const int ksteps = (Ktot + 31) >> 5;
  const f16x8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int it = wave; it < items; it += 4) {
    const int nt = it % NT, mg = it / NT;
    const int n = nt * 16 + fr;
    const u16* wrow = w + (long)(n < N ? n : N - 1) * Ktot;  // a column past N multiplies the last row again and is not stored
    f32x4 acc[MG];
#pragma unroll
    for (int i = 0; i < MG; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ks++) {
      const int kk = ks * 32 + g * 8;
      f16x8 bf = hz, af[MG];
#pragma unroll
      for (int i = 0; i < MG; i++) af[i] = hz;
      if (!TAIL || kk < Ktot) {  // the weight fragment is asked for first: rows' address arithmetic runs under its latency
        bf = *reinterpret_cast<const f16x8*>(wrow + kk);
        const u16* base;
        int ld;
        rows(kk, base, ld);
#pragma unroll
        for (int i = 0; i < MG; i++) af[i] = *reinterpret_cast<const f16x8*>(base + ((mg * MG + i) * 16 + fr) * ld);
      }
#pragma unroll
      for (int i = 0; i < MG; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf, acc[i], 0, 0, 0);
    }
    if (n < N) {
      const auto put = store(n);
#pragma unroll
      for (int i = 0; i < MG; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++) put((mg * MG + i) * 16 + g * 4 + r, acc[i][r]);
      }
    }
  }
}

// the largest tile of 128 .. 32 rows that leaves room for a second workgroup on the CU, else 16 rows in the whole LDS; 0: none fits
template <class F>
int sn_pick_tile(F bytes_for_tile) {
  for (int TT = 128; TT >= 16; TT >>= 1)
    if (bytes_for_tile(TT) <= (size_t)(TT > 16 ? SN_LDS_PREF : SN_LDS_MAX)) return TT;
  return 0;
}

// row blocks per work item (NT column blocks, MT row blocks in the tile): as many as divide the tile while every wave still gets an item
int sn_blocks_per_item(int NT, int MT) { return (MT % 4 == 0 && NT * MT / 4 >= 4) ? 4 : ((MT % 2 == 0 && NT * MT / 2 >= 4) ? 2 : 1); }

// one launch of a tiled kernel.  More than 64 KiB of dynamic LDS has to be allowed once per kernel and device; a repeated call from
// a second thread is harmless.
template <auto Kernel, class P>
int sn_launch(const char* who, const P& p, int blocks, int B, size_t bytes, hipStream_t st) {
  static std::atomic<unsigned long long> allowed{0};
  int dev = 0;
  VBX_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "%s: no current device", who);
  if (!(allowed.load(std::memory_order_acquire) >> dev & 1)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SN_LDS_MAX);
    VBX_REQUIRE(e == hipSuccess, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
    allowed.fetch_or(1ull << dev, std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks, B), dim3(256), bytes, st, p);
  VBX_LAUNCH_CHECK();
  return 0;
}

}  // namespace
