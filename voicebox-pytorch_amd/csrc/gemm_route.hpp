// Which kernel serves a vbx_gemm descriptor: the one place where that is decided (host only, no HIP: tests/native/gemm_route_check.cpp
// replays it with g++).  vbx_gemm = validate -> gemm_route -> switch -> launch; vbx_gemm_route exports the answer without launching.
// Every rule was measured in situ on the model's shapes (bench.py's stage table); GEMM variants have to be judged there, not back to back.
#pragma once
#include <stddef.h>
#include "../../include/vbx.h"

namespace gemm_route {

struct Facts {
  int path;    // vbx_gemm_select: 0 automatic, 1 the 128-wide kernels only, 2 / 3 gemm3 / gemm4 wherever they serve,
               // 4 = 0 with the weight-stationary kernel on whatever VBX_GEMM5 says
  bool gemm5;  // VBX_GEMM5 preset (on unless VBX_GEMM5=0)
  int cus;     // CUs a gemm5 launch may use on the current device (vbx_gemm5_cu_limit applied)
};

inline long cdivl(long a, long b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// gemm5.hip, the weight-stationary kernel: K = 512 linear layers with a row-wise epilogue (to_qkv, FeedForward-in) and the plain bf16
// NT product.  One workgroup per CU holds a panel of 4 x 64 output features, so N / 256 panels must fit the CUs it may use.
inline bool gemm5_serves(const vbx_gemm_desc* d, int cus) {
  if (d->mode != VBX_GEMM_NT || d->K != 512 || !aligned16(d->A) || !aligned16(d->B)) return false;
  if (((long)d->M + 32) * d->lda * 2 >= (1L << 31) || d->M >= (1 << 22)) return false;  // 32-bit buffer offsets of the activation stream
  long nslab;
  switch (d->epilogue) {
    case VBX_EPI_QKV: {
      const int ntrain = (d->qb != nullptr) + (d->kb != nullptr) + (d->v != nullptr) + (d->q_rnorm != nullptr) + (d->k_rnorm != nullptr);
      if (!d->v16 || (ntrain != 0 && ntrain != 5)) return false;  // the fp16 v; all of the backward's copies or none
      if ((long)d->M * d->H * 64 >= (1L << 31)) return false;
      nslab = d->N / 64;
      break;
    }
    case VBX_EPI_GEGLU:
      if (d->ldc % 8 || (d->C2 != nullptr) != (d->C3 != nullptr)) return false;  // training writes both copies, inference neither
      if ((long)d->M * d->N >= (1L << 31) || (long)d->M * d->ldc >= (1L << 31)) return false;
      nslab = d->N / 64;
      break;
    case VBX_EPI_BF16:
      if (d->f16 || d->bias || d->N < 512 || d->N % 64 || (long)d->M * d->ldc >= (1L << 31)) return false;
      nslab = cdivl(d->N, 64);
      break;
    default: return false;
  }
  return cdivl(nslab, 4) <= cus;
}

// gemm3.hip (256 x 256) and gemm4.hip (128 x 256): every NT / NN combination gemm.hip serves (gemm3 also TN / split-K) except the bf16
// epilogue on fp16 operands and the GELU epilogue; their LDS-DMA staging needs K in whole 16-byte pieces.
inline bool wide_tile_serves(const vbx_gemm_desc* d, int tile) {
  if (d->epilogue == VBX_EPI_GELU) return false;  // the 128-wide kernels' functor only (gemm.hip EpiGELU)
  if (d->K % 8 || (d->epilogue == VBX_EPI_BF16 && d->mode == VBX_GEMM_NT && d->f16)) return false;
  return tile == VBX_GEMM_KERNEL_GEMM3 || d->mode != VBX_GEMM_TN;
}

// gemm.hip's three tiles (NT / NN; the TN split-K launches always use the 128-row tile):
//  * one-round 160-row tiles (gemm_kernel_bm160k64) when 128-row tiles would put two on a few CUs, and for half a batch (the sampler
//    integrates the two halves concurrently, solver.py): 104 such workgroups, one per CU -- two of these launches from the two
//    streams then share the chip (16-interval sample 82.7 -> 79.1 ms in the same run against the 64- / 128-row tiles); 96 tiles is
//    the smallest one-round grid served;
//  * k-loop-dominated GEMMs with a light epilogue (K >= 1024, plain bf16 / fp32 stores) also run on that 64-deep tile when they need
//    MORE than one round -- the N = 1024 GEMMs of the dim-1024 model (BASELINE config 3): dgrad FeedForward-in 155 -> 132 us,
//    FeedForward-out 96 -> 80 us, train step 20.08 -> 19.65 ms in the same run.  At K = 512 the same tile loses to the 128 x 256 tile
//    (dgrad FeedForward-out 27.8 vs 20.6 us);
//  * N = dim GEMMs (out-proj, ff-out, dgrads into the residual width) with fewer than ~1.5 workgroups per CU of 128-row tiles: halve
//    the tile height (64 x 128) to fill the chip.  Measured (same run): NN dgrads 410 -> 500 TF, NT out-proj (K=1024) +8 %, NT
//    ff-out (K=1408) -5 % -- hence NN or K <= 1024 only.
// Tried and removed (numbers from the same-run A/Bs): 128x256 tiles with 4 waves of 64x128 -- main loop 30 % faster in a K sweep
// (727 -> 935 TF/s), isolated to_qkv / FeedForward-in launches 3-8 % faster, train step 1 % SLOWER (2 instead of 3 workgroups per CU,
// the ~14 us VALU epilogues overlap less); the same tile with 8 waves of 64x64 -- back-to-back launches 16 % faster (FeedForward-in
// 45.4 -> 38.3 us), 128-forward sample 3 % SLOWER (375 -> 387 ms); 160-row tiles with a 3-slot ring for the wide GEMMs -- sample
// 1.5 % slower; the 160-row tile for every multi-round GEMM.
inline int tile128_family(const vbx_gemm_desc* d) {
  if (d->mode == VBX_GEMM_TN) return VBX_GEMM_KERNEL_BM128;
  const long tiles_n = cdivl(d->N, 128), t128 = cdivl(d->M, 128) * tiles_n, t160 = cdivl(d->M, 160) * tiles_n;
  const bool light = d->epilogue == VBX_EPI_BF16 || d->epilogue == VBX_EPI_F32;
  if ((t128 > 256 && t160 <= 256) || (t160 <= 256 && t160 >= 96) || (light && d->K >= 1024 && t160 > 256)) return VBX_GEMM_KERNEL_BM160;
  if (t128 < 384 && (d->mode == VBX_GEMM_NN || d->K <= 1024)) return VBX_GEMM_KERNEL_BM64;
  return VBX_GEMM_KERNEL_BM128;
}

// Automatic choice (path 0):
//  * the layer's four split-K weight gradients run as ONE grouped gemm3 launch (vbx_gemm_tn_splitk_grouped): 92 us against 4 x 38 us;
//  * the other NT / NN GEMMs stay on the 128-wide kernels except the cases below: at K = dim = 512 a tile's k-loop (12-14 us for
//    256 x 256) is followed by a VALU-bound epilogue of the same order (qk-norm + rotary 10-13 us, GEGLU 5.5 us:
//    tools/native/gemm_trace.cpp) during which the matrix pipes idle; three independent 128 x 128 workgroups per CU overlap the two
//    phases better than one 256 x 256 or two lock-stepped 128 x 256 workgroups (a start-phase stagger of the co-resident workgroups
//    did not help either; its busy-wait was removed, docs/history.md); the N = dim GEMMs have too few wide tiles.
// Paths 2 / 3 force the wide tiles for measurements (tools/native/gemm3_check).
inline int route(const vbx_gemm_desc* d, const Facts& f) {
  if (f.path == 1) return tile128_family(d);
  if (f.path == 2) return wide_tile_serves(d, VBX_GEMM_KERNEL_GEMM3) ? VBX_GEMM_KERNEL_GEMM3 : tile128_family(d);
  if ((f.gemm5 || f.path == 4) && f.path != 3 && gemm5_serves(d, f.cus)) return VBX_GEMM_KERNEL_GEMM5;
  bool wide;
  if (f.path == 3) {
    wide = d->mode != VBX_GEMM_TN;
  } else {
    const bool fills = cdivl(d->M, 128) * cdivl(d->N, 256) >= 256;  // a full round of 128 x 256 tiles, two per CU
    // inference-mode FeedForward-in (GEGLU epilogue writing only the fp16 activations: no pre-activation copy, no bf16 copy) is the
    // one wide NT GEMM where the 128 x 256 two-per-CU tile wins: 34.1 us against 40.7 us back to back.  (The training FeedForward-in
    // on the same tile: 55.5 vs 55.7 us -- no change, it stays on the 128-wide kernel.)
    const bool ffin_eval = d->mode == VBX_GEMM_NT && d->epilogue == VBX_EPI_GEGLU && !d->C2 && !d->C3;
    // The K = dim dgrads into wide outputs (NN, plain bf16 epilogue: the to_out and FeedForward-out dgrads, N = 1024 / 1408) run on
    // the 128 x 256 tile since its epilogue stores whole rows through LDS (gemm_epi3.hpp): in the train step 24.8 -> 21.9 us and
    // 26.9 -> 25.6 us per launch, step 10.60 -> 10.48 ms in the same run.
    const bool dgrad_wide = d->mode == VBX_GEMM_NN && d->epilogue == VBX_EPI_BF16 && d->K <= 512;
    wide = fills && (ffin_eval || dgrad_wide);
    // (Tried: to_qkv of HALF a batch -- 792 tiles of 128 x 128 on 768 slots, 24 of them alone at the end -- as 396 tiles of 128 x 256
    //  in one round: 16-interval sample 83.2 vs 83.1 ms.  The other half batch's stream already fills that tail.)
    // (Tried: the 256 x 256 tile for the wide K = dim GEMMs of HALF a batch -- 17 x 12 / 17 x 11 tiles fit the chip in one round, and in
    //  the sampler the other half batch's stream could fill its epilogue phases: 16-interval sample 80.2 -> 80.5-82.8 ms.  No.)
    // (Tried: gemm3 for K >= 1024 with >= 256 tiles -- the dim-1024 model's to_qkv / FeedForward-in / FeedForward dgrad.  Back to
    //  back it wins (K sweep: K = 1024 68 vs 78 us); in the dim-1024 train step it lost 1.5 % in the same run, 21.1 -> 21.4 ms.)
  }
  return wide && wide_tile_serves(d, VBX_GEMM_KERNEL_GEMM4) ? VBX_GEMM_KERNEL_GEMM4 : tile128_family(d);
}

}  // namespace gemm_route
