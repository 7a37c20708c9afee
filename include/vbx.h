/*
 * vbx.h -- C ABI of libvbx_hip.so: the MI355X (gfx950) native hot path of
 * lucidrains/voicebox-pytorch (VoiceBox transformer fwd/bwd + CFM sampling loop).
 *
 * The reference has NO FFI / plugin interface: its "operators" are ATen calls made
 * from Python modules.  Each entry point below therefore cites the reference *Python call site*
 * (file:line under /root/reference/voicebox_pytorch/) whose ATen work it replaces.  A maintainer
 * binds these with ctypes.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers owned by the caller
 *    (PyTorch-allocated); the library never allocates or frees device memory and never
 *    synchronises, so every entry point is hipGraph-capture safe.
 *  - work is enqueued on `stream` (a hipStream_t passed as void*; 0 = default stream).
 *  - return 0 on success; negative = VBX_E* argument error (checked before launch);
 *    positive = hipError_t of the launch.  vbx_last_error() returns a thread-local message.
 *  - dtypes: bf16/fp16 tensors are raw 16-bit; masks are uint8 (torch.bool); statistics fp32.
 *  - activations are token-major: row r = b * Np + n  (Np = frames + register tokens).
 */
#ifndef VBX_H
#define VBX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBX_VERSION 1

enum { VBX_OK = 0, VBX_EINVAL = -1, VBX_EUNSUPPORTED = -2, VBX_EWORKSPACE = -3 };

int vbx_version(void);
const char* vbx_last_error(void);
/* Device sanity: returns 0 iff device `dev` reports gcnArchName gfx950. */
int vbx_check_device(int dev);

/* ------------------------------------------------------------------ GEMM (MFMA bf16, fp32 acc) */
/* mode: how the two operands are laid out (contraction index k):
 *   NT: A[M,K] (k contiguous), B[N,K] (k contiguous)  -> C[M,N] = A . B^T    nn.Linear forward
 *   NN: A[M,K] (k contiguous), B[K,N] (n contiguous)  -> C[M,N] = A . B      dgrad  (dX = dY . W)
 *   TN: A[K,M] (m contiguous), B[K,N] (n contiguous)  -> C[M,N] = A^T . B    wgrad  (dW = dY^T . X)
 * Replaces every nn.Linear / F.linear on the path (voicebox_pytorch.py:314-315,320,333,345,348,
 * 938,966,1078,1092) and their autograd backward.
 * Argument contract (anything else is VBX_EINVAL, from vbx_gemm and vbx_gemm_route alike, before anything is launched):
 *  - lda, ldb, ldc and N are multiples of 8 (16-byte rows) and cover their rows: lda >= K (NT / NN) or M (TN), ldb >= K (NT) or N
 *    (NN / TN), ldc >= N for VBX_EPI_BF16 / F32 / GELU (VBX_EPI_GEGLU's ldc is the row of its [M, N/2] result; QKV has none);
 *  - K is a multiple of 8 in NT and in NN: the k-contiguous operands are staged in 16-byte pieces, so a ragged K would make the
 *    kernels read a row's padding A[row, K .. lda) and multiply it by zeros -- a NaN or Inf there (torch.empty) would poison the
 *    output row.  TN takes any K (both operands are k-strided) and needs M to be a multiple of 8;
 *  - within these rules the kernels read nothing outside A[.., :K] / B's logical extent and write nothing outside C[:M, :N]:
 *    row padding, the rows behind the last and the columns N .. ldc of an output are never touched (tests/test_gemm_edges_gpu.py). */
enum { VBX_GEMM_NT = 0, VBX_GEMM_NN = 1, VBX_GEMM_TN = 2 };

enum {
  VBX_EPI_BF16 = 0,       /* C bf16 [M,ldc]   (+bias if given)                                     */
  VBX_EPI_F32 = 1,        /* C fp32 [M,ldc]   (+bias) (+resid fp32 [M,ldc]) ; optional bf16 copy   */
  VBX_EPI_QKV = 2,        /* to_qkv + MultiheadRMSNorm + rotary (voicebox_pytorch.py:320-328)       */
  VBX_EPI_GEGLU = 3,      /* FeedForward[0] + GEGLU (voicebox_pytorch.py:338-340,345)               */
  VBX_EPI_SPLITK = 4,     /* fp32 partial slabs [splits][M][N] for TN wgrad                        */
  VBX_EPI_GELU = 5        /* C fp16 [M,ldc] = gelu_erf(acc + bias): NT, fp16 operands (f16 = 1), bias required; the 128-wide tiles */
};

typedef struct {
  int mode, epilogue;
  int M, N, K;
  int lda, ldb, ldc;
  const void* A;            /* bf16 */
  const void* B;            /* bf16 */
  void* C;                  /* per epilogue */
  const float* bias;        /* [N] or NULL */
  const float* resid;       /* EPI_F32: fp32 [M,ldc] added, or NULL */
  void* C2;                 /* EPI_F32: optional bf16 copy [M,ldc]; EPI_GEGLU: bf16 pre-activation [M,N] or NULL */
  int splits;               /* EPI_SPLITK: number of K splits (>=1) */
  /* EPI_QKV: N = 3*H*64.  rows r = b*Np + n. */
  int Np, H;
  float qk_scale;           /* sqrt(dim_head) (MultiheadRMSNorm.scale); <= 0 disables qk-norm */
  const float* q_gamma;     /* [H,64] */
  const float* k_gamma;     /* [H,64] */
  const float* rot_cos;     /* [Np,32] fp32 (host-built table, rotary freqs are (ang,ang)) */
  const float* rot_sin;     /* [Np,32] */
  void* q16; void* k16;     /* fp16 [B,H,Np,64]  : operands of QK^T */
  void* qb;  void* kb;      /* bf16 [B,H,Np,64]  : backward operands (may be NULL in eval) */
  void* v;                  /* bf16 [B,H,Np,64] */
  float* q_rnorm; float* k_rnorm; /* fp32 [B,H,Np] 1/max(|t|,1e-12) (may be NULL in eval) */
  int f16;                  /* 1: A and B hold fp16 (not bf16) -- NT mode only (the forward GEMMs).  Everything that
                             * feeds the attention logits 10*q.k (|q|=|k|=8, std ~80) is precision critical: bf16
                             * operands (2^-9) perturb the logits by ~0.2, fp16 (2^-11) by ~0.05 at the same MFMA
                             * rate; the backward GEMMs keep bf16 (gradient range).  With f16=1 EPI_GEGLU writes
                             * C as fp16. */
  void* v16;                /* EPI_QKV: fp16 copy of v [B,H,Np,64] (forward P.V operand); v (bf16) may then be NULL */
  void* C3;                 /* EPI_GEGLU: optional bf16 copy of C [M,ldc] (wgrad operand) */
  float q_prescale;         /* EPI_QKV: q16 is written as q-hat * q_prescale (vbx_attn_q_prescale(scale): the attention kernels'
                             * contract); <= 0 means 1.  qb / k16 / kb are never scaled. */
} vbx_gemm_desc;

int vbx_gemm(const vbx_gemm_desc* d, void* stream);
/* Tuning knob (results are identical up to fp32 summation order): which tile serves vbx_gemm / the grouped launch.
 * 0 automatic per shape (default; the environment preset VBX_GEMM_PATH was last in commit bb5b90c), 1 the 128-wide kernels only, 2 the 256 x 256
 * 8-wave kernel (gemm3.hip) wherever it can serve, 3 the 128 x 256 two-workgroups-per-CU kernel (gemm4.hip) wherever it can,
 * 4 = 0 with the weight-stationary kernel (gemm5.hip) on even when VBX_GEMM5=0.  Not thread safe; call before launching work. */
int vbx_gemm_select(int path);
/* Round 6: to_qkv and FeedForward-in at K = 512 (NT, VBX_EPI_QKV / VBX_EPI_GEGLU, every backward copy or none) run on the
 * WEIGHT-STATIONARY kernel (csrc/gemm5.hip): one 4-wave workgroup per CU keeps a 256-feature weight panel in its registers and walks
 * 32-row activation blocks; the epilogue of a block runs inside the next block's MFMA stream.  It owns a whole CU (512 registers
 * per lane, 128 KiB LDS), so two such launches on two streams cannot share CUs: a caller that runs two of them concurrently
 * (the sampler's two half-batch streams) gives each a share with vbx_gemm5_cu_limit(n) -- the launches then use at most n CUs
 * (0 = all; process-global, read at launch, i.e. baked into a captured graph).  VBX_GEMM5=0 / vbx_gemm_select(1): the tiled kernels.
 * vbx_gemm_select(4): as 0 with this kernel forced on even when VBX_GEMM5=0. */
int vbx_gemm5_cu_limit(int n);
/* Which kernel vbx_gemm would launch for this descriptor right now (selected path, VBX_GEMM5, CU count of the current device and
 * vbx_gemm5_cu_limit, 16-byte alignment of A / B): one of VBX_GEMM_KERNEL_*, or the negative error code vbx_gemm would return.
 * Launches nothing; pointer fields are only tested for null and for alignment, so a caller without buffers passes placeholders.
 * The rules live in one function, csrc/gemm_route.hpp. */
enum {
  VBX_GEMM_KERNEL_GEMM3 = 3,   /* gemm3.hip: 256 x 256 tile, 8 waves */
  VBX_GEMM_KERNEL_GEMM4 = 4,   /* gemm4.hip: 128 x 256 tile, two workgroups per CU */
  VBX_GEMM_KERNEL_GEMM5 = 5,   /* gemm5.hip: weight-stationary, one workgroup per CU */
  VBX_GEMM_KERNEL_BM64 = 64,   /* gemm.hip: 64 x 128 tile */
  VBX_GEMM_KERNEL_BM128 = 128, /* gemm.hip: 128 x 128 tile (every TN / split-K launch outside gemm3) */
  VBX_GEMM_KERNEL_BM160 = 160  /* gemm.hip: 160 x 128 tile, 64-deep k-steps */
};
int vbx_gemm_route(const vbx_gemm_desc* d);
/* n (1..4) TN / VBX_EPI_SPLITK GEMMs in ONE launch of the 256 x 256 tile (same slab layout and results as n vbx_gemm calls):
 * the four weight-gradient GEMMs of a layer are 8-24 such tiles each; together, with 3 K-splits, they fill 198 CUs (92 us in
 * situ against 4 x 38 us as separate 128-wide launches).  With vbx_gemm_select(1) it falls back to n separate launches. */
int vbx_gemm_tn_splitk_grouped(const vbx_gemm_desc* descs, int n, void* stream);
/* Sum split-K slabs [splits][M][N] and scatter into dst (fp32): dst[rowmap(i)][j] (+)= sum_s slab.
 * rowmap: 0 identity; 1 GEGLU de-interleave with (F, Fp): packed row p -> ((p%128)<64 ?
 * (p/128)*64+p%128 : F + (p/128)*64 + p%128-64), rows/cols beyond the valid range dropped. */
int vbx_splitk_reduce(const float* slabs, int splits, int M, int N, float* dst, int dst_rows, int dst_cols,
                      int dst_ld, int rowmap, int F, int accumulate, void* stream);

/* ------------------------------------------------------------------ norms */
/* AdaptiveRMSNorm / RMSNorm forward (voicebox_pytorch.py:246-247, 270-276):
 * y[r,:] = x[r,:]/max(|x[r,:]|,1e-12)*sqrt(D) * gamma[b(r),:] + beta[b(r),:]  -> bf16.
 * gamma/beta: fp32 with batch stride gb_stride (0 for the non-adaptive RMSNorm), beta may be NULL.
 * Rows: for each batch b, rows n in [n0, n0+rows_per_batch) of x (row stride Np per batch);
 * output y is dense [B*rows_per_batch, D]. */
int vbx_rmsnorm_fwd(const float* x, const float* gamma, const float* beta, long gb_stride, void* y_bf16,
                    void* y_f16 /* optional fp16 copy (same dense layout); y_bf16 may then be NULL */,
                    int B, int Np, int n0, int rows_per_batch, int D, void* stream);
/* same, fp32 output rows [B*rows_per_batch, D] (final norm of a standalone Transformer.forward, :479) */
int vbx_rmsnorm_fwd_f32(const float* x, const float* gamma, const float* beta, long gb_stride, float* y_f32, int B, int Np,
                        int n0, int rows_per_batch, int D, void* stream);
/* backward: dx_out = dx_in (or 0 if NULL) + d/dx ; partial dgamma/dbeta sums per row chunk:
 * part[b][chunk][2][D] (chunk count = vbx_rmsnorm_bwd_chunks(rows_per_batch)).  dy is dense bf16 [B*rows, D].
 * dx tensors have the same (Np, n0) row addressing as x.  dxb: optional bf16 copy of dx_out (same addressing). */
int vbx_rmsnorm_bwd_chunks(int rows_per_batch);
int vbx_rmsnorm_bwd(const float* x, const float* gamma, long gb_stride, const void* dy_bf16, const float* dx_in,
                    float* dx_out, void* dxb_bf16, float* part,
                    float* colpart /* optional [B][chunks][D]: per-chunk column sums of dx_in (a fused bias gradient) */,
                    int B, int Np, int n0, int rows_per_batch, int D, void* stream);

/* ------------------------------------------------------------------ attention */
/* Attend.forward math path (attend.py:121-135): softmax(scale * q k^T + key-pad mask) v, fused
 * flash-style (scores never materialised).  q16,k16,v16 fp16 are [B,H,Np,64]; mask uint8
 * [B,Np] or NULL; lse fp32 [B,H,Np] in log2 units (m + log2 l).
 * CONTRACT (round 5, every vbx_attn_* entry point): q16 holds q PRE-MULTIPLIED by scale * log2(e) (vbx_attn_q_prescale(scale)),
 * so that q16 . k16 is directly the exponent of exp2 -- the kernels fold the softmax statistics into the MFMA accumulator
 * (csrc/attn_bwd_fold.inc) and have no per-element scale multiply left.  The to_qkv epilogue writes it that way
 * (vbx_gemm_desc.q_prescale); a caller with plain fp32 q multiplies before rounding to fp16.  qb (the bf16 backward operand)
 * stays UNSCALED; `scale` remains the multiplier of dq / dk, which are gradients w.r.t. the unscaled q / k.
 * MASKS: a masked key gets weight 0.  A batch whose mask is all False follows attend.py:126 (masked_fill with -finfo.max, then
 * softmax), i.e. a UNIFORM softmax over all Np keys (logits taken as 0): out_i = sum_j keep_ij * rk * v_j / Np (keep = 1, rk = 1
 * without dropout), lse = log2(Np), dv_j = sum_i keep_ij * rk * dO_i / Np, dq = dk = 0 (and, in the fused backward, a zero d(q, k)
 * block and zero gamma partials).  Every forward and backward entry point, vbx_attn_fwd_f32* included, implements this. */
float vbx_attn_q_prescale(float scale);
int vbx_attn_fwd(const void* q16, const void* k16, const void* v16 /* fp16 */, const uint8_t* mask,
                 void* out16 /* fp16 [B,Np,H*64] */, void* out_bf16 /* optional bf16 copy (backward operand) */,
                 float* lse, int B, int H, int Np, float scale, void* stream);
/* backward (autograd of attend.py:121-135).  dout bf16 [B,Np,H*64]; qb,kb bf16 copies of q,k; delta fp32 [B,H,Np] scratch;
 * dq,dk fp32 [B,H,Np,64]; dv is written bf16 token-major at dv[(b*Np+n)*dv_ld + h*64 + d].
 * One kernel family serves it: the TWO-BODY kernel -- dq and dk/dv bodies in one launch, S / dP evaluated in both, no inter-workgroup
 * waits, deterministic.  By default its softmax statistics are folded into the MFMA accumulator (csrc/attn_bwd_fold.inc: P = exp2(-(L - q.k))
 * with L added inside the matrix pipe); vbx_attn_bwd_select(3) runs the same bodies without the fold (the environment
 * switch VBX_ATTN_BWD_FOLD=0 that did the same was last in commit bb5b90c) (round 3's
 * arithmetic -- what attention dropout always uses); the two differ by fp32 rounding of the exponent only.  Tail tiles of <= 16 rows
 * (Np % 128 <= 16: the register tokens) run a 16 x 16 MFMA role with their ring rows split over the waves (csrc/attn_bwd_ragged.inc).
 * Round 3's ONE-PASS chain kernel (select 2: S / dP once, dq summed by an ordered chain of workgroups through device memory) was correct
 * and 30 - 60 % slower; it was removed in round 6 (docs/history.md): vbx_attn_bwd_select(2) returns VBX_EUNSUPPORTED and
 * vbx_attn_bwd_scratch_bytes() 0.  `scratch` stays in the signatures for ABI stability and is ignored (pass NULL).
 * vbx_attn_bwd_select: 0 automatic (= 1), 1 folded two-body, 3 unfolded two-body. */
size_t vbx_attn_bwd_scratch_bytes(int B, int H, int Np);
int vbx_attn_bwd_select(int variant);
int vbx_attn_bwd_variant(void); /* always 1 (two-body) since round 6 */
int vbx_attn_bwd(const void* q16, const void* k16, const void* qb, const void* kb, const void* v,
                 const uint8_t* mask, const void* out /* forward output [B,Np,H*64]; NULL: `delta` already holds rowsum(dO * O)
                                                         (the caller's own) and the pass that computes it is skipped */, int out_is_f16,
                 const void* dout, const float* lse, float* delta, float* dq, float* dk, void* dv, int dv_ld, int B, int H,
                 int Np, float scale, void* scratch, void* stream);
/* backward of MultiheadRMSNorm + rotary (voicebox_pytorch.py:286-287,199): consumes dq/dk fp32
 * [B,H,Np,64] and the saved q16/k16 + rnorm, writes d(raw q|k) bf16 into dqkv[(b*Np+n)*ld + which*H*64
 * + h*64 + d] and partial gamma grads gpart[2][vbx_qknorm_rope_bwd_gpart_rows(B)][H][64]. */
/* delta[b,h,n] = sum_j P[n,j] dP[n,j] from the attention backward's own operands (P = exp2(q16 . k16 - lse), masked keys 0;
 * dP = dO . V^T over the bf16 v), for a following vbx_attn_bwd* call with out = NULL ("delta is already written").  The default pass
 * inside those calls, rowsum(dO * O), reads the forward's fp16 output, which was summed from the fp16 copy of v: the same number
 * mathematically, but dS = P (dP - delta) is then a small difference of two terms whose roundings of v differ by 2^-9, multiplied by
 * scale |q| |k| on the way to q and k.  Under a dense loss over many rows that averages out; under a loss on a handful of rows of a
 * short sequence it is most of d(q), d(k) and the qk-norm gammas (one token: P = 1, the exact dS is 0, everything that arrives is that
 * rounding difference).  Cost is quadratic in Np (fp32 VALU, one workgroup per 64 queries of a head); the stage runtime uses it for the
 * stand-alone stack at Np <= VBX_ATTN_DELTA_CONSISTENT_MAX_NP without attention dropout.  q16, k16 fp16 and v bf16 [B,H,Np,64], dout
 * bf16 [B*Np, H*64], lse / delta fp32 [B,H,Np], mask [B,Np] or NULL.  No atomics, reruns bit-identical.  B * H <= 65535. */
#define VBX_ATTN_DELTA_CONSISTENT_MAX_NP 256
int vbx_attn_delta_consistent(const void* q16, const void* k16, const void* v, const uint8_t* mask, const void* dout, const float* lse,
                              float* delta, int B, int H, int Np, void* stream);
/* vbx_attn_bwd with the backward of rotary + MultiheadRMSNorm (vbx_qknorm_rope_bwd) folded into the epilogues of its two kernels:
 * no fp32 dq / dk round trip; writes d(qkv) bf16 [B*Np, ld] (q | k | v blocks of H*64 columns) directly.  gpart: partial gamma
 * gradients [2][B * vbx_attn_bwd_fused_tiles(Np)][H][64] (q then k), to be summed over the rows (qk_scale > 0 only). */
int vbx_attn_bwd_fused_tiles(int Np);
int vbx_attn_bwd_fused(const void* q16, const void* k16, const void* qb, const void* kb, const void* v, const uint8_t* mask,
                       const void* out, int out_is_f16, const void* dout, const float* lse, float* delta, const float* q_rnorm,
                       const float* k_rnorm, const float* q_gamma, const float* k_gamma, const float* rot_cos, const float* rot_sin,
                       float qk_scale, void* dqkv, int ld, float* gpart, int B, int H, int Np, float scale, void* scratch,
                       void* stream);
/* ---- training-time dropout (attend.py:131 attention probabilities, voicebox_pytorch.py:346 GEGLU output)
 * The mask is a pure function of (seed, stream_id, element index) through Philox4x32-10, 16 random bits per element: an element is
 * kept iff its lot < thr16 = round((1 - p) * 65536), survivors are scaled by vbx_dropout_keep_scale(p) = 65536 / thr16 (exactly
 * unbiased for the realised keep rate).  Counters: attention element (bh, q, key) -> (4 * (key / 32) + (key % 32) / 8, q, bh, stream_id),
 * lot key % 8; FeedForward element (row, col) -> (col / 8, row, 0, stream_id), lot col % 8; Philox key = (seed low, seed high);
 * lot e of a call = 16-bit half e % 2 (low first) of output word e / 2.  The runtime uses stream_id = 2 * layer (attention) and
 * 2 * layer + 1 (FeedForward) with one seed per forward (vbx_io.drop_seed).
 * vbx_attn_dropout_bits writes one layer's keep bits in both orientations the kernels read: bits_rm [B*H][Np][W] (bit key % 32 of
 * word key / 32) and bits_cm [B*H][Np keys][W] (bit q % 32 of word q / 32), W = vbx_dropout_bits_words(Np) 32-bit words per row.
 * The *_dropout attention entry points take them: the forward keeps the softmax statistics of the undropped probabilities; the
 * backward runs on the two-body kernel.  vbx_dropout_rows drops a [rows, cols] 16-bit matrix in place (fp16 copy and / or bf16
 * copy of the same values; cols and ld multiples of 8) -- applied to the GEGLU output in the forward and to its gradient in the
 * backward. */
int vbx_dropout_bits_words(int Np);
float vbx_dropout_keep_scale(float p);
int vbx_attn_dropout_bits(void* bits_rm, void* bits_cm, int BH, int Np, unsigned long long seed, unsigned stream_id, float p,
                          void* stream);
int vbx_dropout_rows(void* x_f16, void* x_bf16, long rows, int cols, int ld, unsigned long long seed, unsigned stream_id, float p,
                     void* stream);
/* the same mask (same seed / stream_id / element index) on an fp32 matrix: precise mode's unrounded GEGLU output */
int vbx_dropout_rows_f32(float* x, long rows, int cols, int ld, unsigned long long seed, unsigned stream_id, float p, void* stream);
/* vbx_attn_fwd for prefix lengths (inference; the sampler's lens=): key_lens int32 [B] on the device, key_lens[b] >= 1; keys at or
 * past key_lens[b] are masked whatever `mask` (the equivalent prefix mask, or NULL) says.  A workgroup of batch row b walks
 * ceil(key_lens[b] / 64) key tiles instead of ceil(Np / 64) (the DMA ring prefetches against the same bound); a 128-row query tile
 * wholly at or past key_lens[b] writes zeros and lse 1e30 and leaves.  Every output row and lse of a query < key_lens[b] is bit-equal
 * to vbx_attn_fwd with the prefix mask: a skipped tile would add +0 to l and O, and max(m, -inf) = m.  Rows >= key_lens[b] are
 * padding.  The forward clamps key_lens[b] into [0, Np] (the backward entry points below into [1, Np]): at 0 every tile of the batch
 * row is dead, so all its rows are zeros with lse 1e30 and no K or V row is read; callers pass >= 1.
 * The benchmark's kernel is a separate instantiation and is not changed by this one. */
int vbx_attn_fwd_lens(const void* q16, const void* k16, const void* v16, const uint8_t* mask, const int* key_lens, void* out16,
                      void* out_bf16, float* lse, int B, int H, int Np, float scale, void* stream);
/* ------------------------------------------------------------------ attention backward with prefix lengths (training, lens=)
 * vbx_attn_bwd_lens / vbx_attn_bwd_fused_lens: the arguments of vbx_attn_bwd / vbx_attn_bwd_fused plus key_lens, int32 [B] on the
 * device, 1 <= key_lens[b] <= Np (the kernel clamps into that range: no value can become an out-of-range bound).  Keys at or past
 * key_lens[b] are dead whatever `mask` (the equivalent prefix mask, or NULL) says.  The length-aware kernel does not read `mask` at
 * all -- the lengths say the same, and the per-block mask byte loads are what a masked backward costs over a plain one; only the
 * fallbacks below read it.
 *  - PRECONDITION: query rows at or past key_lens[b] are padding and dout is ZERO there.  The train step guarantees it: their loss is
 *    masked and every layer between the loss and the attention output is row-wise or (GateLoop) causal towards the front.
 *  - Under it dq, dk, dv (resp. dqkv and gpart) equal what vbx_attn_bwd / vbx_attn_bwd_fused give with the prefix mask: bit for bit
 *    on rows < key_lens[b], zero on the rows at or past it.  Every row < Np of every output is written (the caller does not pre-zero).
 *  - dq role (128 query rows per workgroup): walks ceil(key_lens[b] / 64) key tiles instead of ceil(Np / 64), the DMA ring prefetches
 *    against the same bound, the last walked tile clamps its rows and compares its keys against key_lens[b].  dk/dv role (128 keys
 *    per workgroup): walks ceil(key_lens[b] / 64) query tiles.  A skipped tile would have contributed P = 0 (dead keys) or
 *    dO = delta = 0 (dead queries), i.e. +-0, to every sum.  A 128-row tile of either role wholly at or past key_lens[b] issues no
 *    DMA, writes zero rows (fused form: zero dqkv columns and a zero gpart record) and leaves.
 *  - Launch order, XCD map and the <= 16-row ragged tail role (Np % 128 in 1..16) are those of vbx_attn_bwd.  delta comes from the
 *    same streaming pass.  No atomics; reruns are bit-identical.  No empty-batch pass: key_lens >= 1.
 *  - The kernel is a further instantiation of the folded two-body backward; the existing kernels are not changed by it.  There is no
 *    length-aware form of attention dropout, of vbx_attn_bwd_select(3) or of precise mode: callers run the masked entry points with
 *    the prefix mask bytes there (the same values).  Under vbx_attn_bwd_select(3) these two entry points do that themselves and
 *    then require `mask`. */
int vbx_attn_bwd_lens(const void* q16, const void* k16, const void* qb, const void* kb, const void* v, const uint8_t* mask,
                      const int* key_lens, const void* out, int out_is_f16, const void* dout, const float* lse, float* delta,
                      float* dq, float* dk, void* dv, int dv_ld, int B, int H, int Np, float scale, void* scratch, void* stream);
int vbx_attn_bwd_fused_lens(const void* q16, const void* k16, const void* qb, const void* kb, const void* v, const uint8_t* mask,
                            const int* key_lens, const void* out, int out_is_f16, const void* dout, const float* lse, float* delta,
                            const float* q_rnorm, const float* k_rnorm, const float* q_gamma, const float* k_gamma,
                            const float* rot_cos, const float* rot_sin, float qk_scale, void* dqkv, int ld, float* gpart, int B,
                            int H, int Np, float scale, void* scratch, void* stream);
/* ------------------------------------------------------------------ packed rows (inference; the sampler's lens= with pack=True)
 * A ragged batch of B rows with len_b frames each runs as ONE batch row of Mp rows.
 *  - A segment is one batch row: R register rows, then len_b frame rows, then dead rows up to the next multiple of
 *    VBX_PACK_ALIGN = 128, the attention query tile.  A query tile and a 64-row conv_embed chunk belong to exactly one segment.
 *  - Segments follow each other in batch order.  Mp = sum of the segment sizes, optionally rounded up (the sampler's pack_bucket, a
 *    multiple of 128); rows past the last segment are dead.
 *  - Device tables, int32, S segments: seg_start[S] (a multiple of 128), seg_klen[S] = R + len_b >= 1 (the live rows = the keys of
 *    the segment), tile_seg[Mp / 128] = the segment of the tile, or -1 past the last segment; and the rotary tables rot_cos /
 *    rot_sin [Mp, 32] gathered by each row's index inside its own segment (registers at position -10000, frame n at n), dead rows
 *    taking row 0.  The kernels index by these tables without checking them: the caller validates them on the host (starts aligned
 *    and ascending, 1 <= klen, seg_start + align(klen) <= Mp, tile_seg agreeing with the starts) before they reach the device.
 *  - Dead rows are finite but otherwise unspecified after the first layer.  No live row depends on them (the attention kernel
 *    never loads a row outside the live keys of the query's segment, the convolution reads 0 outside 0 <= n < len_b, every other
 *    kernel is row-wise), and the caller never reads them back.
 * vbx_attn_fwd_segs: q16 / k16 / v16 [1, H, Mp, 64], out [Mp, H * 64], lse [H, Mp].  The workgroup of query tile t reads
 * s = tile_seg[t] and walks ceil(seg_klen[s] / 64) key tiles from row seg_start[s]; only the last, partial tile compares key < klen
 * (no mask bytes), and its DMA re-reads row seg_start[s] + seg_klen[s] - 1 instead of anything past it.  Every live query row and
 * lse is bit-equal to vbx_attn_fwd_lens on the segment alone (B = 1, Np = its aligned size, key_lens = klen, mask NULL); a dead
 * query row, and every row of a tile with s < 0, gets zeros and lse 1e30 whatever q / k / v hold there.  Grid fixed by (Mp / 128, H),
 * the XCD-aware order of vbx_attn_fwd.  A fourth instantiation of the forward body: the other three are not changed by it. */
#define VBX_PACK_ALIGN 128
int vbx_attn_fwd_segs(const void* q16, const void* k16, const void* v16, const int* seg_start, const int* seg_klen,
                      const int* tile_seg, void* out16, void* out_bf16, float* lse, int H, int Mp, float scale, void* stream);
/* ------------------------------------------------------------------ ragged waves (the front ends' lens=; wrapper(wave, wave_lens=))
 * A padded batch of waves [B, T] whose row b holds lens[b] real samples.  The *_lens entries below are their plain siblings with one
 * more argument, a DEVICE table const int* lens [B] in the units of that launch's INPUT, and the contract
 *  - row b is read only at positions < lens[b] (what lies behind may be anything, NaN included);
 *  - every padding (reflection, zero fill, pad1d's short-input rule, `extra`) is resolved about lens[b], by the arithmetic the plain
 *    entry applies to T;
 *  - outputs at or past the row's own output length are STORED as exactly 0.0 (never skipped: the buffers are not cleared);
 *  - so row b of the result, up to its own output length, is bit-equal to the plain entry on the row alone, x[b, :lens[b]].
 * The grids, the tiles and the pitches of the buffers are those of the plain entry at T; a workgroup wholly behind its row only
 * stores zeros.  An entry of lens outside the range the plain entry accepts for T is CLAMPED into it by the kernel (the host
 * wrappers validate or clamp before; no bound reaches an address unchecked).  Plain vector loads and stores, no atomics, no
 * workgroup waits for another: reruns are bit-identical.  The plain entries launch the instantiations they always launched.
 *   vbx_logmel_lens        frames_b = 1 + lens[b] / hop, reflection p >= len -> 2 (len - 1) - p; n_fft / 2 < lens[b] <= T.  A frame
 *                          f >= frames_b is staged as zeros, as frames past the end always were (it shares a complex transform
 *                          with frame f - 1 when f is odd).
 *   vbx_melspec_lens       frames_b = 1 + (lens[b] + 2 pad - n_fft) / hop; max(pad + 1, n_fft - 2 pad) <= lens[b] <= T.
 *   vbx_resample_lens      zero fill from lens[r] on; outputs from ceil(nw lens[r] / orig) on are 0.0; Lout = ceil(nw L / orig);
 *                          1 <= lens[r] <= L.
 *   vbx_seanet_conv0_lens  L_b = lens[b], 1 <= L_b <= T: Lz (the length pad1d reflects about) from L_b; rows from L_b on are 0.
 *   vbx_seanet_conv_lens   L_b = lens[b], Lout_b = ceil(L_b / stride), `extra` and Lz from them; pad_left does not depend on L.  The
 *                          second input (x2) is read at t < L_b; positions from Lout_b on are 0.  The NEXT launch takes the table
 *                          ceil(lens / stride).
 * vbx_lstm needs no such entry: the recurrence runs forward, steps below the row's length cannot see what follows them.
 *
 * HubertWithKmeans(wave, lens=) -- the one front end whose FIRST layer is not local: GroupNorm(C, C) takes its statistics over time.
 *   vbx_hubert_conv0_stats_lens   lens[b] samples, k0 <= lens[b] <= T: row b's statistics run over L0_b = (lens[b] - k0) / s0 + 1
 *                          positions.  The chunks are the plain entry's 256-position chunks from position 0; a workgroup whose chunk
 *                          starts at or past L0_b leaves before it reads anything, the last live chunk takes n = L0_b - t0, and the
 *                          finalize pass combines the live chunks alone, in the same ascending fp64 order, and divides by L0_b: the
 *                          statistics are bit-equal to those of the row alone.  records keeps the pitch vbx_hubert_conv0_chunks(L0).
 *   vbx_hubert_conv0_apply_lens   the plain apply's arithmetic at positions < L0_b; a position at or past L0_b stores fp16 zeros and
 *                          reads neither the wave nor the statistics -- this is what frees the result of the padding's content.
 *   vbx_hubert_conv        runs UNCHANGED.  It has no padding: with L_b live inputs and Lout_b = (L_b - k) / 2 + 1 live outputs, the
 *                          last live output reads inputs up to 2 (Lout_b - 1) + k - 1 <= L_b - 1, so a live output reads live
 *                          inputs only.  Outputs at or past Lout_b read stored zeros and at most k - 1 live values: finite, and read
 *                          by no live position of any later layer, by the same argument one layer on.  The caller maps the table
 *                          through (l - k) / 2 + 1 alongside.
 *   vbx_hubert_posconv_lens       lens[b] = N_b frames, 1 <= N_b <= N: positions >= N_b (not >= N) are staged as zeros, which is what
 *                          Conv1d(padding = k / 2) of the row alone sees there, whatever x holds; output rows N_b .. N - 1 are
 *                          stored as 0.0 without a product and a tile wholly past N_b stages nothing.  The tile is the plain
 *                          entry's at N.
 *   the encoder layers     vbx_attn_fwd_lens with key_lens = the frame lengths and mask NULL; the products, the LayerNorms and
 *                          vbx_hubert_split_heads are row-wise and run as they are.  Dead rows stay finite and feed no live row.
 *                          The caller zero-fills the dead frames of the last layer's output and the dead ids after
 *                          vbx_kmeans_assign (id 0: always a valid index of an embedding table).
 * Bit-equality to the row alone holds where vbx_gemm_route answers the same for M = B * N and M = N_b (it changes kernel at tile
 * counts of 96, 256 and 384 only) -- the tile core of the convolutions gives the same bits at every tile height. */
int vbx_logmel_lens(const float* audio, const int* lens, float* out, const float* window, const float* tw_re, const float* tw_im,
                    const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft, int hop,
                    int n_mels, int log_out, void* stream);
int vbx_melspec_lens(const float* audio, const int* lens, float* out, const float* window, const float* tw_re, const float* tw_im,
                     const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft, int hop,
                     int pad, int n_mels, float mean, float inv_std, int channel_first, void* stream);
int vbx_resample_lens(const float* x, const int* lens, float* y, const float* taps, const int* start, const int* len, int rows, long L,
                      long Lout, int orig, int nw, int width, int K, int run_max, void* stream);
int vbx_seanet_conv0_lens(const float* wave, const int* lens, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k,
                          int causal, void* stream);
int vbx_seanet_conv_lens(const void* x1_f16, const void* x2_f16, const int* lens, const void* w_f16, const float* bias, void* y, int B,
                         int L, int C1, int C2, int Co, int k, int stride, int dilation, int elu1, int out_f32, int causal, void* stream);
int vbx_hubert_conv0_stats_lens(const float* wave, const int* lens, const float* w, float* records, float* stats, int B, long T, int C,
                                int k0, int s0, float eps, void* stream);
int vbx_hubert_conv0_apply_lens(const float* wave, const int* lens, const float* w, const float* stats, const float* gamma,
                                const float* beta, void* y_f16, int B, long T, int C, int k0, int s0, void* stream);
int vbx_hubert_posconv_lens(const float* x, const int* lens, const void* w_f16, const float* bias, float* y, int B, int N, int D,
                            int groups, int k, void* stream);
int vbx_attn_fwd_dropout(const void* q16, const void* k16, const void* v16, const uint8_t* mask, void* out16, void* out_bf16,
                         float* lse, int B, int H, int Np, float scale, const void* bits_rm, float p, void* stream);
int vbx_attn_bwd_dropout(const void* q16, const void* k16, const void* qb, const void* kb, const void* v, const uint8_t* mask,
                         const void* out, int out_is_f16, const void* dout, const float* lse, float* delta, float* dq, float* dk,
                         void* dv, int dv_ld, int B, int H, int Np, float scale, const void* bits_rm, const void* bits_cm, float p,
                         void* stream);
/* bits_rm == NULL: identical to vbx_attn_bwd_fused */
int vbx_attn_bwd_fused_dropout(const void* q16, const void* k16, const void* qb, const void* kb, const void* v, const uint8_t* mask,
                               const void* out, int out_is_f16, const void* dout, const float* lse, float* delta,
                               const float* q_rnorm, const float* k_rnorm, const float* q_gamma, const float* k_gamma,
                               const float* rot_cos, const float* rot_sin, float qk_scale, void* dqkv, int ld, float* gpart, int B,
                               int H, int Np, float scale, void* scratch, const void* bits_rm, const void* bits_cm, float p,
                               void* stream);
int vbx_qknorm_rope_bwd(const float* dq, const float* dk, const void* q16, const void* k16, const float* q_rnorm,
                        const float* k_rnorm, const float* q_gamma, const float* k_gamma, const float* rot_cos,
                        const float* rot_sin, float qk_scale, void* dqkv, int ld, float* gpart, int B, int H, int Np,
                        float q16_scale /* the factor q16 carries: vbx_attn_q_prescale(scale) */, void* stream);

/* ------------------------------------------------------------------ small / memory-bound ops */
/* x_cat bf16 [B*N, 2*D] = (x, cond * ~cond_mask)   (voicebox_pytorch.py:1035,1075-1076) */
int vbx_pack_embed_input(const float* x, const float* cond, const uint8_t* cond_mask, void* out_f16,
                         void* out_bf16 /* optional copy: wgrad operand */, int B, int N, int D, void* stream);
/* ConvPositionEmbed + residual + register tokens (voicebox_pytorch.py:220-233,1080,422-425):
 * xs[b, R+n, :] = e[b,n,:] + mask*gelu(conv(mask*e)[b,n,:] + bias);  xs[b, r<R, :] = reg[r,:]. */
/* text-conditioned embed input (condition_on_text = True, voicebox_pytorch.py:1035-1076):
 * out[b*N+n, :] = [ x | cond_emb | cond' ] as fp16 (+bf16), width 2*D + E, with
 *   cond'    = drop[b] ? null_cond : cond * ~cond_mask                       (:1035, :1043-1048; drop_mask may be NULL)
 *   cond_emb = table[drop[b] ? null_id : ids[b, .]] resized from T tokens to N frames by interpolate_1d (:89-107, :1057-1066):
 *              F.interpolate bilinear, align_corners=False (identity when T == N).
 * vbx_cond_emb_bwd scatters d(cond_emb) (bf16 [B*N, E], row stride ld) into the table gradient with fp32 atomics. */
int vbx_pack_embed_input_text(const float* x, const float* cond, const uint8_t* cond_mask, const uint8_t* drop_mask,
                              const float* null_cond, const long* ids, int T, const float* table, int E, long null_id,
                              void* out_f16, void* out_bf16, int B, int N, int D, void* stream);
/* Codec-latent models (vbx_model.Lc): the to_embed operand rows [ x' | cond_emb | cond' ] (fp16, + bf16 when out_bf16), width 2*D + E:
 *   x'    = x . W^T + b                                                    x, cond fp32 [B*N, L];  W = proj_in.weight [D, L]
 *   cond' = drop[b] ? null_cond : (cond_mask[row] ? 0 : cond . W^T + b)     (:1000-1006, :1035, :1043-1048; null_cond is D wide)
 * One launch, both products on the matrix cores against one weight panel: w_f16 is the fp16 copy of W, [D, Kp] row-major with
 * Kp = vbx_proj_in_kp(L) (= L + 1 rounded up to 32) and zeros in columns L .. Kp-1; bias / null_cond fp32.  The cond_emb columns are
 * NOT written (vbx_embed_text_cols).  xc_bf16 (training, may be NULL): the operand of the weight gradient, bf16 [2*B*N, Kp] = x rows
 * then cond rows, the cond rows that pass no gradient (cond_mask set, dropped sample) zeroed, column L = 1 on every row that counts:
 * dY^T . xc with dY = [dx' ; dcond'] is [ d(proj_in.weight) | d(proj_in.bias) ] (vbx_proj_in_wgrad_reduce). */
int vbx_proj_in_kp(int L);
int vbx_proj_in_embed(const float* x, const float* cond, const void* w_f16, const float* bias, const uint8_t* cond_mask,
                      const uint8_t* drop_mask, const float* null_cond, void* out_f16, void* out_bf16, void* xc_bf16, int B, int N,
                      int L, int D, int E, void* stream);
/* columns [col0, col0 + E) of the same rows (row stride ld): cond_emb as vbx_pack_embed_input_text computes it */
int vbx_embed_text_cols(const uint8_t* drop_mask, const long* ids, int T, const float* table, int E, long null_id, void* out_f16,
                        void* out_bf16, int B, int N, int col0, int ld, void* stream);
/* ---- per-row token resize (ragged batches with token ids at another frame rate; vbx_io.tok_lens)
 * vbx_pack_embed_input_text, vbx_embed_text_cols and vbx_cond_emb_bwd stretch T tokens to N frames with ONE ratio T / N for the batch.  Their *_lens
 * siblings stretch row b's own T_b = tok_lens[b] tokens to its own N_b = key_lens[b] - R frames, as the row alone would:
 *  - frame n < N_b: the same interpolate_1d source (i0, i1, lam) computed from (n, N_b, T_b) over ids[b, :T_b]; T_b == N_b is the
 *    identity, as T == N is above.  Bit-equal to the plain entry on the row alone (B = 1, N = N_b, T = T_b, ids[b, :T_b]).
 *  - frame n >= N_b: the cond_emb columns are 0; the x and cond' columns (vbx_pack_embed_input_text_lens) are written as ever.  The
 *    backward adds nothing to the table for such a frame.
 *  - tok_lens [B] and key_lens [B] int32 on the device; the kernels clamp T_b into 1 .. T and N_b into 1 .. N, so no value of a
 *    table becomes an out-of-range index.  R: the register rows key_lens counts in front of the frames (0: key_lens holds frames).
 *  - drop_mask / null_id as above.  Second kernels: the plain entries launch the kernels they always launched. */
int vbx_pack_embed_input_text_lens(const float* x, const float* cond, const uint8_t* cond_mask, const uint8_t* drop_mask,
                                   const float* null_cond, const long* ids, int T, const int* tok_lens, const int* key_lens, int R,
                                   const float* table, int E, long null_id, void* out_f16, void* out_bf16, int B, int N, int D,
                                   void* stream);
int vbx_embed_text_cols_lens(const uint8_t* drop_mask, const long* ids, int T, const int* tok_lens, const int* key_lens, int R,
                             const float* table, int E, long null_id, void* out_f16, void* out_bf16, int B, int N, int col0, int ld,
                             void* stream);
int vbx_cond_emb_bwd_lens(const void* demb_bf16, int ld, const long* ids, int T, const int* tok_lens, const int* key_lens, int R,
                          const uint8_t* drop_mask, long null_id, float* gtable, int B, int N, int E, void* stream);
/* split-K slabs [splits][D][Kp] of dY^T . xc  ->  dw fp32 [D, L], db fp32 [D] */
int vbx_proj_in_wgrad_reduce(const float* slabs, int splits, int D, int L, float* dw, float* db, void* stream);
/* vbx_masked_mse_fwd / _bwd with the prediction (and d(pred), bf16, pad columns zeroed) in rows of ldp >= D floats, any D */
int vbx_masked_mse_fwd_ld(const float* pred, int ldp, const float* target, const uint8_t* loss_mask, float* per_b, float* loss, int B,
                          int N, int D, void* stream);
int vbx_masked_mse_bwd_ld(const float* pred, int ldp, const float* target, const uint8_t* loss_mask, const float* per_b,
                          const float* gscale, void* dpred_bf16, int B, int N, int D, void* stream);
/* dst [rows, cols] = src[:, 0:cols] (row stride ld_src) */
int vbx_copy_cols_f32(const float* src, int ld_src, float* dst, long rows, int cols, void* stream);
/* Log-mel front end (LogMelCodec.encode; the arithmetic of MelVoco.encode, voicebox_pytorch.py:518-541, torchaudio defaults):
 * out fp32 [B, 1 + T / hop, n_mels] from audio fp32 [B, T], T > n_fft / 2: centred frames with reflect padding, times window[n_fft]
 * (the periodic Hann window of win_length samples centred in n_fft, zeros around it), fp32 FFT in the LDS (n_fft a power of two in
 * 256 .. 2048; tw_re / tw_im [n_fft / 2] = cos / -sin(2 pi k / n_fft), built in fp64), power spectrum, mel filter m = the run of
 * fb_len[m] weights fb_w[fb_off[m] ..] over the bins from fb_start[m] (fb_start[m] + fb_len[m] <= n_fft / 2 + 1), then
 * 10 log10(max(., 1e-10)) when log_out.  One launch. */
int vbx_logmel(const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im, const int* fb_start,
               const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft, int hop, int n_mels, int log_out,
               void* stream);
/* The vocoders' own mel front end (HiFiGANMelCodec.encode / mel_spectrogram; the arithmetic of HiFi-GAN's and BigVGAN's
 * meldataset.mel_spectrogram at center = False), the sibling of vbx_logmel on the same transform and the same filter runs:
 * audio fp32 [B, T] is reflect-padded by `pad` samples on both sides (HiFi-GAN: pad = (n_fft - hop) / 2; 0 <= pad <= n_fft / 2, T > pad,
 * T + 2 pad >= n_fft: one reflection per side suffices, and one frame may reflect on both), frame f = the n_fft samples from
 * f * hop - pad, frames = 1 + (T + 2 pad - n_fft) / hop, times window[n_fft], fp32 FFT in the LDS (sizes and tables as vbx_logmel),
 * mag = sqrtf(re^2 + im^2 + 1e-9f), mel filter runs as vbx_logmel (the caller passes Slaney-scale, area-normalised weights),
 * out = (ln(max(mel, 1e-5f)) - mean) * inv_std -- the accurate sqrtf, the logarithm taken in fp64 and rounded once to fp32 (the device's
 * logf is a 2-ulp function: silence would miss ln(1e-5) by 1.7 ulp); mean = 0, inv_std = 1 give the plain logarithm exactly.
 * channel_first = 0: out [B, frames, n_mels] (a codec's latents); 1: out [B, n_mels, frames] (what the generators take) -- the same
 * bits, transposed.  One launch, no atomics: reruns are bit-identical and a row does not depend on the rows beside it. */
int vbx_melspec(const float* audio, float* out, const float* window, const float* tw_re, const float* tw_im, const int* fb_start,
                const int* fb_len, const int* fb_off, const float* fb_w, int B, long T, int n_fft, int hop, int pad, int n_mels,
                float mean, float inv_std, int channel_first, void* stream);
/* Vocoder-free decode (LogMelCodec.mel_to_magnitude / griffin_lim; csrc/griffinlim.hip).
 * vbx_mel_to_mag: mel fp32 [B, frames, n_mels] (dB when log_in, else power) -> mag fp32 [B, frames, n_bins] (frame-major)
 *   = sqrt(max(pinv(fb^T) @ P, 0)), P = 10^(mel / 10) or mel; pinv_t [n_mels, n_bins] is the pseudo-inverse (taken in fp64 on the
 *   host) stored mel-major.
 * vbx_griffinlim: the torchaudio.functional.griffinlim loop (power = 1, length = None) with m = momentum / (1 + momentum):
 *   mag [B, frames, n_bins], n_bins = n_fft / 2 + 1; spec_a [B, frames, n_bins, 2] holds the initial unit phasors (re, im) on entry,
 *   spec_a / spec_b are the two kept spectra and are overwritten; fb [B, frames, win] is the frame buffer; wave [B, (frames - 1) * hop]
 *   the result; window / tw_re / tw_im as vbx_logmel; renv [(frames - 1) * hop] the reciprocal window-square envelope of the kept
 *   range.  2 n_iter + 2 launches, no host synchronisation.  Needs 0 < hop <= win <= n_fft, (frames - 1) * hop > n_fft / 2 and
 *   vbx_griffinlim_lds_bytes(n_fft, win, hop) <= 65536. */
int vbx_mel_to_mag(const float* mel, float* mag, const float* pinv_t, int B, int frames, int n_mels, int n_bins, int log_in,
                   void* stream);
int vbx_griffinlim_lds_bytes(int n_fft, int win, int hop);
int vbx_griffinlim(const float* mag, float* spec_a, float* spec_b, float* fb, float* wave, const float* window, const float* tw_re,
                   const float* tw_im, const float* renv, int B, int frames, int n_fft, int win, int hop, int n_iter, float m,
                   void* stream);
/* vbx_istft: one torch.istft (center = True, length = None) of mag * phasor -- the synthesis and overlap-add launches of
 *   vbx_griffinlim alone (what n_iter = 0 runs), without the analysis step's demand on the length: frames >= 2 is enough.
 *   mag [B, frames, n_bins], spec [B, frames, n_bins, 2] the unit phasors (re, im), read only; fb, wave, window, tw_re, tw_im, renv
 *   as vbx_griffinlim.  Two launches, the same bits on every run. */
int vbx_istft(const float* mag, const float* spec, float* fb, float* wave, const float* window, const float* tw_re, const float* tw_im,
              const float* renv, int B, int frames, int n_fft, int win, int hop, void* stream);
/* vbx_istft_trim: the same two launches with any trim (Vocos's ISTFT at padding = "same"; the center trim gives vbx_istft's bits).
 *   The frames' windowed inverse transforms add up to (frames - 1) * hop + n_fft samples, frame g starting at g * hop; wave
 *   [B, out_len] is samples [trim, trim + out_len) of that sum, each times renv [out_len], summed over the covering frames in
 *   ascending frame order (no atomics, the same bits on every run).  "same": trim = (win - hop) / 2, out_len = (frames - 1) * hop +
 *   win - 2 trim;  "center": trim = n_fft / 2, out_len = (frames - 1) * hop.  frames >= 1, trim >= 0, out_len >= 1, trim + out_len
 *   within the sum.
 * Sizes of the two inverse-only entries: n_fft a power of two in 256 .. 2048, OR 5 * 2^m = 320, 640, 1280 (a mixed-radix transform,
 *   csrc/fft_lds.hpp: radix-2 stages, one radix-5 pass).  The tables are the SAME at every size: tw_re / tw_im [n_fft / 2] =
 *   cos / -sin(2 pi k / n_fft); the radix-5 pass reaches the upper half of the circle through W^(j + n_fft / 2) = -W^j, no full
 *   table is passed.  1 / n_fft is applied in fp32 with the window (exact at a power of two, two roundings more otherwise).
 *   vbx_logmel and vbx_griffinlim (forward transforms) refuse 320 / 640 / 1280. */
int vbx_istft_trim(const float* mag, const float* spec, float* fb, float* wave, const float* window, const float* tw_re,
                   const float* tw_im, const float* renv, int B, int frames, int n_fft, int win, int hop, int trim, long out_len,
                   void* stream);
/* Vocos decoder (voicebox_pytorch_amd.VocosDecoder; csrc/vocos.hip): the kernels around the GEMMs of a ConvNeXt backbone + ISTFT head.
 * vbx_vocos_kp: Kp = 7 * C rounded up to a multiple of 32, the K of the embedding GEMM.
 * vbx_vocos_pack_input: features x fp32 [B, C, frames] -> the im2col operand of the 7-tap input convolution, fp16 [B * frames, Kp]:
 *   column tap * C + c of row (b, t) = x[b, c, t + tap - 3], zero outside [0, frames) of THAT batch element, zero columns from 7 * C
 *   to Kp; log_in takes log(max(x, 1e-7)) first (the padding stays zero).  The matching weight is W[d, tap * C + c] = w[d, c, tap].
 *   C <= 512.
 * vbx_vocos_dwconv_ln: x fp32 [B, frames, D] -> y fp16 [B * frames, D] = LayerNorm_D(conv)(eps, biased variance, two passes) * ln_w
 *   + ln_b with conv[b, t, d] = conv_bias[d] + sum_k taps[k, d] * x[b, t + k - 3, d] (taps fp32 [7, D], tap-major; zero padding per
 *   batch element); taps = NULL: the LayerNorm of x itself.  fp32 throughout, one rounding (saturating) to fp16.  D a multiple of
 *   64, at most 2048.
 * vbx_vocos_head: h fp32 [rows, ld] (columns [0, n_bins) log-magnitude m, [n_bins, 2 n_bins) phase p) -> mag fp32 [rows, n_bins] =
 *   min(exp(m), 100) and phasor fp32 [rows, n_bins, 2] = (cos p, sin p), the operands of vbx_istft; libm-accurate exp / sin / cos. */
int vbx_vocos_kp(int C);
int vbx_vocos_pack_input(const float* x, void* out_f16, int B, int C, int frames, int log_in, void* stream);
int vbx_vocos_dwconv_ln(const float* x, const float* taps, const float* conv_bias, const float* ln_w, const float* ln_b, void* y_f16,
                        int B, int frames, int D, float eps, void* stream);
int vbx_vocos_head(const float* h, float* mag, float* phasor, long rows, int n_bins, int ld, void* stream);
/* Residual vector quantizer (voicebox_pytorch_amd.ResidualVQ / EncodecVocoCodec; csrc/rvq.hip): the RVQ of an EnCodec-style codec,
 * codebooks fp32 [Q, K, D].  D a multiple of 8 in 8 .. 256, K in 2 .. 4096 (any value), Q in 1 .. 32, any B * N >= 1; everything
 * else returns VBX_EINVAL.  Codes are int64, laid out [B, N, Q] (codes_qn = 0) or [B, Q, N] (codes_qn = 1, what the reference's
 * decode_to_codes returns).  No atomics, no host synchronisation: the same bits on every run.
 * vbx_rvq_norms: norms fp32 [Q, K] = |c_qk|^2, an fp32 fmaf chain over the D components (error <= (D + 1) 2^-24 |c|^2).
 * vbx_rvq_encode: x fp32 [B * N, D] -> codes and, unless NULL, quantized fp32 [B * N, D].  Per frame, r_0 = x and for q = 0 .. Q-1:
 *   code_q = argmin_k norms[q][k] - 2 r_q . c_qk, the LOWEST index on an exact tie;  r_{q+1} = r_q - c_q[code_q] in fp32;
 *   quantized = c_0[code_0] + c_1[code_1] + ..., summed in that order in fp32.  The search is fp32 throughout (fp32-input MFMA =
 *   an fmaf chain per dot product, the same component order for every codeword), so for the r_q rebuilt from the earlier codes
 *     d(code_q) - min_k d(k) <= (D + 2) 2^-23 (|r_q| + max_k |c_qk|)^2,   d(k) = |c_qk|^2 - 2 r_q . c_qk  exactly.
 *   norms must be vbx_rvq_norms of the same codebooks.  One launch, a workgroup per 32 frames.
 * vbx_rvq_decode: codes -> out fp32 = sum over q = 0 .. Q-1, in that order in fp32, of c_q[code_q]: row-major [B * N, D]
 *   (channel_first = 0, the latents) or [B, D, N] (channel_first = 1, what VocosDecoder takes).  An index outside [0, K)
 *   contributes zero and is never dereferenced. */
int vbx_rvq_norms(const float* codebooks, float* norms, int Q, int K, int D, void* stream);
int vbx_rvq_encode(const float* x, const float* codebooks, const float* norms, long* codes, float* quantized, int B, int N, int D,
                   int K, int Q, int codes_qn, void* stream);
int vbx_rvq_decode(const long* codes, const float* codebooks, float* out, int B, int N, int D, int K, int Q, int codes_qn,
                   int channel_first, void* stream);
/* SEANet encoder (voicebox_pytorch_amd.SEANetEncoder; csrc/seanet.hip): EnCodec's encoder -- reflect-padded convolutions with ELU,
 * strided downsampling, an LSTM with a skip, a final convolution -- inference only.  PRECISION CONTRACT: activations between layers
 * are fp16, channel-last [B, L, C], rounded ONCE and stored before the activation (the Resnet shortcut reads them un-activated);
 * weights are fp16 (weight norm folded in fp32 first); every sum is fp32 on the matrix cores (v_mfma_f32_16x16x32_f16); ELU is
 * x > 0 ? x : expm1f(x) in fp32, applied when an operand is staged and rounded to fp16 there; the first convolution reads the fp32
 * wave with fp32 weights (an fmaf chain on the bias, in tap order); LSTM gates, cell state and the skip add are fp32 with libm's
 * expf / tanhf, h is rounded to fp16 only as the next step's matrix operand; the final convolution writes fp32.  No atomics: reruns
 * are bit-identical, and a batch row's result does not depend on its neighbours.
 * SConv1d (non-causal): k_eff = (k - 1) dilation + 1, padding_total = k_eff - stride, extra = ceil(L / stride) stride - L,
 * pad_right = padding_total / 2, pad_left = padding_total - pad_right; reflect padding by (pad_left, pad_right + extra) with pad1d's
 * short-input rule (L <= max pad: append max - L + 1 zeros, reflect, cut them off again); Lout = ceil(L / stride).
 * SConv1d (causal, what the published 24 kHz model is built with): the same k_eff, padding_total, extra and Lout; reflect padding
 * by (padding_total, extra) -- all of padding_total on the left, only extra on the right -- with the same short-input rule, now at
 * max pad = max(padding_total, extra).  Either form resolves a padded position with ONE reflection per side: pad1d reflects about a
 * row of Lz = max(L, max pad + 1) samples (the appended zeros included), and each padding is at most Lz - 1.  The largest
 * padding_total the SEANet classes ask for is 8 (k = 16 at stride 8; k = 3 at dilation 4).
 * vbx_seanet_conv_c / vbx_seanet_conv0_c / vbx_seanet_conv_out_c: vbx_seanet_conv / _conv0 / _conv_out with `causal` (0: the
 *   non-causal padding, nonzero: the causal one); the entry points without the suffix are these at causal = 0, bit for bit.  The
 *   products, their order, the tiles and the stores do not depend on `causal`: only which sample a padded position reads.
 * vbx_seanet_conv: y [B, Lout, Co] (fp16, or fp32 when out_f32) = conv(elu1 ? ELU(x1) : x1) + bias with w fp16 [Co, k * C1 + C2],
 *   column tap * C1 + c; a second input x2 [B, L, C2] (needs k = 1, stride = 1; never activated) is K-concatenated as columns
 *   k * C1 .. : the Resnet block's tail and its shortcut in one product.  C1, C2 multiples of 8 up to 1024, k <= 16, stride <= 8,
 *   dilation <= 4.  A workgroup owns up to vbx_seanet_conv_tile(...) output positions of one row: the largest of 128 .. 32 whose
 *   span fits 80 KiB of LDS, else 16 within 160 KiB (negative: not even that fits); fewer on a row shorter than the tile.
 * vbx_seanet_conv0: wave fp32 [B, T] -> y fp16 [B, T, nf], w fp32 [nf, k], k odd, nf a multiple of 8 up to 64.
 * vbx_lstm_step: step s of T + layers - 1: layer 0 at time s and layer 1 at time s - 1 in ONE plain launch (each reads only what
 *   earlier launches wrote).  xproj fp32 [B * T, 4H] = x W_ih0^T + b_ih0 + b_hh0 (a vbx_gemm); w_hh0 fp16 [4H, H]; w_cat1 fp16
 *   [4H, 2H] = [W_ih1 | W_hh1]; bias1 = b_ih1 + b_hh1; gate order i, f, g, o; h0 / h1 fp16 [B, T, H] and c fp32 [layers, B, H] are
 *   work buffers (zero initial state, nothing to clear); y16 (and y32 unless NULL) [B, T, H] = h_last + x.  H a multiple of 32 up to
 *   1024.  vbx_lstm: all the steps in order. */
int vbx_seanet_conv_tile(int C1, int C2, int k, int stride, int dilation);
int vbx_seanet_conv(const void* x1_f16, const void* x2_f16, const void* w_f16, const float* bias, void* y, int B, int L, int C1, int C2,
                    int Co, int k, int stride, int dilation, int elu1, int out_f32, void* stream);
int vbx_seanet_conv0(const float* wave, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k, void* stream);
int vbx_seanet_conv_c(const void* x1_f16, const void* x2_f16, const void* w_f16, const float* bias, void* y, int B, int L, int C1, int C2,
                      int Co, int k, int stride, int dilation, int elu1, int out_f32, int causal, void* stream);
int vbx_seanet_conv0_c(const float* wave, const float* w, const float* bias, void* y_f16, int B, int T, int nf, int k, int causal,
                       void* stream);
int vbx_lstm_step(const float* xproj, const void* w_hh0, const void* w_cat1, const float* bias1, void* h0, void* h1, float* c,
                  const void* x, void* y16, float* y32, int B, int T, int H, int layers, int s, void* stream);
int vbx_lstm(const float* xproj, const void* w_hh0, const void* w_cat1, const float* bias1, void* h0, void* h1, float* c, const void* x,
             void* y16, float* y32, int B, int T, int H, int layers, void* stream);
/* SEANet decoder (voicebox_pytorch_amd.SEANetDecoder; csrc/seanet.hip): EnCodec's decoder -- a first convolution, an LSTM with a
 * skip, per ratio (ELU, strided transposed convolution, Resnet blocks), ELU, a last convolution to one channel -- inference only, under
 * the encoder's PRECISION CONTRACT above: fp16 channel-last activations rounded once and stored before the ELU, fp16 weights folded
 * in fp32, fp32 sums on v_mfma_f32_16x16x32_f16, no atomics, reruns bit-identical, a batch row independent of its neighbours.  The
 * first convolution, the Resnet blocks and the LSTM are vbx_seanet_conv / vbx_gemm / vbx_lstm unchanged.
 * vbx_seanet_pack_latents: z fp32 [B, D, T] channel-first -> y fp16 [B, T, D], rounded once.
 * vbx_seanet_convtr: the non-causal SConvTranspose1d with k = 2 stride, and only that form.  x fp16 [B, L, C] (ELU applied in fp32 as it
 *   is staged, rounded to fp16 as the operand) -> y fp16 [B, L stride, Co], Co = C / 2.  padding_total = k - stride = r is trimmed:
 *   right = r / 2, left = r - right.  Untrimmed position j r + p (0 <= p < r) = b[o] + sum_c a[j, c] W[c, o, p] + a[j - 1, c] W[c, o, p + r]
 *   with a[-1] = a[L] = 0: one product over rows j = 0 .. L with the operand row [a_j | a_{j-1}] (K = 2C) and the packed weight
 *   w fp16 [r Co, 2C], row p Co + o = [W[:, o, p] | W[:, o, p + r]]; the r Co results of row j are the contiguous run from trimmed
 *   position j r - left on (row 0 drops its phases p < left, row L keeps only those).  bias fp32 [Co] is added in the epilogue.  C a
 *   multiple of 16 up to 1024, stride in 2 .. 8.  vbx_seanet_convtr_tile(C, stride) is an UPPER bound on the rows j of one batch row
 *   that a workgroup owns: the largest of 128 .. 32 whose tile + 1 staged positions fit 80 KiB of LDS, else 16 within 160 KiB
 *   (negative: not served); it depends on C alone (stride is only range-checked), and a launch with fewer than tile / 2 + 1 product
 *   rows (L + 1) halves it, down to 16.
 * vbx_seanet_convtr_t: the same product with the trim given: trim_left samples are cut in front and padding_total - trim_left
 *   behind, 0 <= trim_left <= stride (anything else: VBX_EINVAL).  The causal SConvTranspose1d trims padding_right =
 *   ceil(padding_total trim_right_ratio) behind and trim_left = padding_total - padding_right in front: 0 at the published ratio 1.0,
 *   where the first L stride untrimmed samples are the output.  vbx_seanet_convtr is this at trim_left = stride - stride / 2, bit
 *   for bit.  At trim_left = 0 row j = L stores nothing and is not launched: L product rows, and the halving rule counts those.
 * vbx_seanet_conv_out: the last convolution, the mirror of vbx_seanet_conv0: x fp16 [B, T, nf] -> y fp32 [B, T] = bias[0] +
 *   sum_tap sum_c w[tap, c] ELU(x[pad(t + tap), c]); w fp32 [k, nf], k odd and at most 7, nf a multiple of 8 up to 64; SConv1d's reflect
 *   padding with pad1d's short-input rule; ELU in fp32 on the stored fp16 value, NOT rounded again; one fp32 fmaf chain on the bias,
 *   tap-major then channel. */
int vbx_seanet_pack_latents(const float* z, void* y_f16, int B, int D, int T, void* stream);
int vbx_seanet_convtr_tile(int C, int stride);
int vbx_seanet_convtr(const void* x_f16, const void* w_f16, const float* bias, void* y_f16, int B, int L, int C, int stride, void* stream);
int vbx_seanet_conv_out(const void* x_f16, const float* w, const float* bias, float* y, int B, int T, int nf, int k, void* stream);
int vbx_seanet_convtr_t(const void* x_f16, const void* w_f16, const float* bias, void* y_f16, int B, int L, int C, int stride, int trim_left,
                        void* stream);
int vbx_seanet_conv_out_c(const void* x_f16, const float* w, const float* bias, float* y, int B, int T, int nf, int k, int causal,
                          void* stream);
/* HiFi-GAN generator (voicebox_pytorch_amd.HiFiGANGenerator; csrc/hifigan.hip): conv_pre, per stage (leaky ReLU, transposed
 * convolution, the mean of up to three residual blocks), leaky ReLU, conv_post, tanh -- inference only, on SEANet's tile core
 * (csrc/seanet_tile.hpp) and under SEANet's PRECISION CONTRACT: activations fp16 channel-last [B, L, C], rounded ONCE and stored
 * BEFORE the activation (the residual reads them un-activated); leaky ReLU is x > 0 ? x : x * slope in fp32, applied when an operand
 * is staged and rounded to fp16 there; weights fp16 (weight norm folded in fp32 first); every sum fp32 on v_mfma_f32_16x16x32_f16 in
 * ascending column order; all paddings are ZEROS; no atomics, reruns bit-identical, a batch row independent of its neighbours.
 * Error bounds against fp64 on the same fp16 operands (tests/test_hifigan_gpu.py): a sum of n fp32 terms in any order is within
 * (n - 1) 2^-24 (1 + o(1)) of sum |terms|, so
 *   vbx_hifigan_conv    |err| <= (k C + 3) 2^-24 (sum |w a| + |b| + |res|) + 2^-11 |y| + 2^-25: k C products, the bias and the residual
 *                       are k C + 2 terms, one more for slack; then the fp16 store (half an ulp, 2^-25 below the normal range)
 *   vbx_hifigan_convtr  |err| <= (2 C + 2) 2^-24 (sum |w a| + |b|) + 2^-11 |y| + 2^-25
 *   vbx_hifigan_post    |err| <= (k C + 2) 2^-24 (sum |w a| + |b|) + 2^-22: the fp32 fmaf chain (tanh is 1-Lipschitz, so the error of its
 *                       argument passes at most unchanged), then tanhf within 4 fp32 ulps of |y| <= 1; no fp16 store
 * The leaky ReLU and the n = 2, 3 mean are single correctly rounded fp32 operations (a product, a sum, a division), so the staged
 * operand is reproduced exactly on the host and the bounds carry no term for it.
 * vbx_hifigan_pack: mel fp32 [B, M, T] channel-first -> y fp16 [B, T, Mp], Mp = M rounded up to a multiple of 8, columns M .. Mp - 1
 *   zero; log != 0: logf(fmaxf(mel, 1e-5f)) first.  M in 1 .. 512.
 * vbx_hifigan_conv: y fp16 [B, L, Co] = conv(act ? lrelu(x) : x) + bias (+ res), x fp16 [B, L, C], w fp16 [Co, k C], column tap * C + c,
 *   k odd and at most 11, dilation 1 .. 12, zero padding (k - 1) dilation / 2 on both sides; res fp16 [B, L, Co] or NULL is added in
 *   fp32 as (sum + bias) + res before the one rounding.  C a multiple of 8 up to 1024.  A workgroup owns up to
 *   vbx_hifigan_conv_tile(C, k, dilation) positions of one row: the largest of 128 .. 32 whose span of tile + (k - 1) dilation positions
 *   fits 80 KiB of LDS, else 16 within 160 KiB (negative: not even that fits); fewer on a row shorter than the tile.
 * vbx_hifigan_respair: y = x + c2(lrelu(c1(lrelu(x)))), c1 with the given dilation, c2 with dilation 1, both k taps and C -> C, in ONE
 *   launch: the intermediate lives in the LDS, rounded to fp16 exactly where vbx_hifigan_conv would have stored it, and is ZERO at
 *   positions outside [0, L) (c2's padding).  BIT-EQUAL to vbx_hifigan_conv(x, w1, b1, NULL, h, act = 1) followed by
 *   vbx_hifigan_conv(h, w2, b2, res = x, y, act = 1).  C a multiple of 8 up to vbx_hifigan_respair_max_channels() = 64.
 * vbx_hifigan_convtr: ConvTranspose1d(C, C / 2, 2 stride, stride, padding stride / 2) in vbx_seanet_convtr_t's one-product form at
 *   trim_left = stride / 2: w fp16 [stride Co, 2C], row p Co + o = [W[:, o, p] | W[:, o, p + stride]].  The operand is
 *   lrelu(mean of `inputs` tensors x0 .. x2 fp16 [B, L, C]): ((x0 + x1) + x2) / inputs in fp32, rounded to fp16 once.  y fp16
 *   [B, L stride, C / 2].  C a multiple of 16 up to 1024, stride even in 2 .. 8.
 * vbx_hifigan_post: y fp32 [B, T] = tanhf(bias[0] + sum_tap sum_c w[tap, c] lrelu(mean of the inputs)[t + tap - k / 2, c]), zero
 *   padded, w fp32 [k, C]; the operand stays fp32 (not rounded again); one fmaf chain on the bias: per chunk of 32 channels tap-major,
 *   then channel (C <= 32: tap-major, then channel).  C a multiple of 8 up to 512, k odd and at most 11.
 * vbx_hifigan_conv and vbx_hifigan_convtr halve their tile, down to 16, while a launch has fewer than 256 workgroups (one per CU of an
 *   MI355X); an element's sum does not depend on the tile, so the bits do not either. */
int vbx_hifigan_pack(const float* mel, void* y_f16, int B, int M, int T, int log, void* stream);
int vbx_hifigan_conv_tile(int C, int k, int dilation);
int vbx_hifigan_conv(const void* x_f16, const void* w_f16, const float* bias, const void* res_f16, void* y_f16, int B, int L, int C, int Co,
                     int k, int dilation, int act, float slope, void* stream);
int vbx_hifigan_respair_max_channels(void);
int vbx_hifigan_respair(const void* x_f16, const void* w1_f16, const float* bias1, const void* w2_f16, const float* bias2, void* y_f16, int B,
                        int L, int C, int k, int dilation, float slope, void* stream);
int vbx_hifigan_convtr(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const void* w_f16, const float* bias,
                       void* y_f16, int B, int L, int C, int stride, float slope, void* stream);
int vbx_hifigan_post(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* w, const float* bias, float* y,
                     int B, int T, int C, int k, float slope, void* stream);
/* BigVGAN generator (voicebox_pytorch_amd.BigVGANGenerator; csrc/bigvgan.hip on csrc/hifigan_tile.hpp): HiFi-GAN's generator with
 * every leaky ReLU replaced by Activation1d A (2x up-sampling with a 12-tap filter f_u, the snake function per channel, 12-tap
 * low-pass f_d and 2x down-sampling) and no activation in front of the transposed convolutions.  The PRECISION CONTRACT is
 * HiFi-GAN's above: fp16 channel-last activations rounded once where stored, fp32 sums, no atomics, reruns bit-identical, a batch
 * row independent of its neighbours.  Per channel, x the fp32 mean ((x0 + x1) + x2) / n of the fp16 inputs at one position:
 *   u[m] = 2 sum_i f_u[m + 5 - 2 i] x[clamp(i, 0, L - 1)]   over the six i with 0 <= m + 5 - 2 i <= 11, m in [0, 2 L)
 *   s[m] = u[m] + inv_beta sin^2(alpha u[m])
 *   A(x)[t] = sum_{tau = 0 .. 11} f_d[tau] s[clamp(2 t + tau - 5, 0, 2 L - 1)]
 * (the replicate paddings of the published modules as clamps: x is clamped to [0, L), s to [0, 2 L)).  ORDER OF OPERATIONS, all
 * fp32: acc = 0; acc = fmaf(f_u[m + 5 - 2 i], x[clamp(i)], acc) for the six i ASCENDING; u = 2 acc; a = alpha * u (one rounded
 * product); sn = sinf(a), the accurate library sine, never the fast intrinsic; s = fmaf(inv_beta, sn * sn, u) with sn * sn rounded;
 * acc = 0; acc = fmaf(f_d[tau], s[clamp(2 t + tau - 5)], acc) for tau = 0 .. 11 ASCENDING; the result is rounded to fp16 once.  Every
 * kernel below evaluates A by this one sequence, whatever its tiling: the same x give the same bits.  alpha, inv_beta: fp32 [C] on
 * the device (inv_beta = 1 / (beta + 1e-9), or 1 / (alpha + 1e-9) for snake, computed by the caller); f_u, f_d: fp32 [12] on the device.
 * Error bound of vbx_bigvgan_act against fp64 on the same inputs and parameters (eps = 2^-24; second-order terms are covered by
 * the slack of one term in each sum):
 *   E_u[m] = 7 eps 2 sum_i |f_u x|                                          six fmaf roundings and one of slack; the doubling is exact
 *   E_s[m] = (1 + alpha inv_beta) E_u + inv_beta (eps |alpha u| + 2^-20 + eps) + eps |s|
 *            the error of u and the rounding of the argument a pass through |ds/du| = |1 + inv_beta alpha sin(2 a)| <= 1 + alpha
 *            inv_beta; sinf within 4 ulp of a value of at most 1 is 2^-21, doubled by the square (|d sn^2| <= 2 |sn| |d sn|); the
 *            rounding of sn * sn; the rounding of the last fmaf
 *   |err[t]| <= sum_tau |f_d[tau]| E_s[clamp(2 t + tau - 5)] + 13 eps sum_tau |f_d s| + 2^-11 |y| + 2^-25
 *            twelve fmaf roundings and one of slack, then the fp16 store
 * The 4 ulp of sinf is the figure of the OpenCL C specification (full profile), which the device library's sine is built to; it is
 * ASSUMED here, not measured.
 * vbx_bigvgan_act: y fp16 [B, L, C] = fp16(A(mean of `inputs` tensors x0 .. x2 fp16 [B, L, C])).  C a multiple of 8 up to 1536,
 *   L in 1 .. 2^29 - 1.  Each s[m] is computed once per run of up to 32 positions that a thread walks with the twelve s of the
 *   current output in registers.
 * vbx_bigvgan_conv: y fp16 [B, L, Co] = conv(A(x)) + bias (+ res), A computed while the span is staged into the LDS: BIT-EQUAL to
 *   vbx_bigvgan_act followed by vbx_hifigan_conv(act = 0) with the same operands.  A span position outside [0, L) is the convolution's
 *   ZERO padding, not A evaluated past the row.  Limits and tile (vbx_bigvgan_conv_tile) are vbx_hifigan_conv's: the activation's
 *   window lives in registers and takes no LDS beside the span.
 * vbx_bigvgan_convtr: vbx_hifigan_convtr without an activation, C a multiple of 16 up to 1536; up to 1024 BIT-EQUAL to
 *   vbx_hifigan_convtr(slope = 1.0), whose own limit stays 1024; its bound holds with the plain mean as the operand.
 * vbx_bigvgan_post: y fp32 [B, T] = final(bias[0] + sum w[tap, c] fp16(A(mean of the inputs))[t + tap - k / 2, c]), zero padded, w fp32
 *   [k, C], bias NULL = 0, the fmaf chain of vbx_hifigan_post; final 0: tanhf, 1: fminf(fmaxf(., -1), 1).  With a bias and final = 0
 *   BIT-EQUAL to vbx_bigvgan_act followed by vbx_hifigan_post(inputs = 1, slope = 1.0).  Against fp64 on vbx_bigvgan_act's own output:
 *   vbx_hifigan_post's bound, for final = 1 without the tanhf term: (k C + 2) 2^-24 (sum |w a| + |b|) (a clamp is 1-Lipschitz and
 *   exact).  C a multiple of 8 up to 512, k odd and at most 11. */
int vbx_bigvgan_act(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* alpha, const float* inv_beta,
                    const float* f_u, const float* f_d, void* y_f16, int B, int L, int C, void* stream);
int vbx_bigvgan_conv_tile(int C, int k, int dilation);
int vbx_bigvgan_conv(const void* x_f16, const float* alpha, const float* inv_beta, const float* f_u, const float* f_d, const void* w_f16,
                     const float* bias, const void* res_f16, void* y_f16, int B, int L, int C, int Co, int k, int dilation, void* stream);
int vbx_bigvgan_convtr(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const void* w_f16, const float* bias,
                       void* y_f16, int B, int L, int C, int stride, void* stream);
int vbx_bigvgan_post(const void* x0_f16, const void* x1_f16, const void* x2_f16, int inputs, const float* alpha, const float* inv_beta,
                     const float* f_u, const float* f_d, const float* w, const float* bias, float* y, int B, int T, int C, int k, int final,
                     void* stream);
/* Aligner primitives (voicebox_pytorch_amd.maximum_path / forward_sum_loss; csrc/align.hip): monotonic alignment search and the
 * forward-sum (CTC) loss over an attention map fp32 [B, T, K], T query frames by K keys.  K in 1 .. 1024, any T >= 1, B * T < 2^31;
 * everything else returns VBX_EINVAL.  query_lens / key_lens: int32 [B] on the device, NULL = T / K; a length is clamped into
 * [0, T] / [0, K].  A row with key_len == 0 or query_len < key_len has no monotonic path: a defined all-zero result, no error.
 * One workgroup per batch row, no atomics, no host synchronisation: the same bits on every run and for a row
 * alone or inside a batch.
 * vbx_maximum_path: Q[y][x] = max(Q[y-1][x], Q[y-1][x-1]) + value[y][x] over the band max(0, k + y - q) <= x <= min(k - 1, y)
 *   (a predecessor outside it is excluded), then from idx = k - 1 at y = q - 1 downwards: path[y][idx] = 1 and idx -= 1 iff
 *   idx != 0 and (idx == y or Q[y-1][idx] < Q[y-1][idx-1]) -- a tie STAYS on the key.  path fp32 [B, T, K] is written whole
 *   (zeros at t >= q and keys >= k), durations int64 [B, K] = path summed over t.  The returned path is exactly optimal for the
 *   table as rounded in fp32 (one addition per cell).  bits: scratch, B * T * ceil(K / 64) 64-bit words, contents undefined.
 * vbx_forward_sum_fwd: per frame t < q the log-softmax over {blank_logprob, value[t][0 .. k)}, then CTC with blank 0 and target
 *   1 .. k:  nll fp32 [B] = -log Z, 0 for a row without a path or with a non-finite Z (zero_infinity); NOT divided by key_len.
 *   Scratch kept for the backward: lse fp64 [B, T], alpha fp64 [B, T, K] (the label states; NULL when no backward follows),
 *   logz fp64 [B].  Inputs, exponentials and logarithms are fp32; the running log-probabilities, whose magnitude grows with T, are
 *   summed in fp64.  Two launches: the normalisers on every CU, then the recursion.
 * vbx_forward_sum_bwd: grad fp32 [B, T, K] = grad_nll[b] * d nll[b] / d value, through the pad + mask + log-softmax; written whole,
 *   exactly 0 at t >= q, at keys >= k and on rows whose nll is 0 by the rule above. */
int vbx_maximum_path(const float* value, const int* query_lens, const int* key_lens, float* path, long* durations,
                     unsigned long long* bits, int B, int T, int K, void* stream);
int vbx_forward_sum_fwd(const float* value, const int* key_lens, const int* query_lens, float blank_logprob, double* lse, double* alpha,
                        float* nll, double* logz, int B, int T, int K, void* stream);
int vbx_forward_sum_bwd(const float* value, const int* key_lens, const int* query_lens, float blank_logprob, const double* lse,
                        const double* alpha, const double* logz, const float* grad_nll, float* grad, int B, int T, int K, void* stream);
/* The Aligner network (voicebox_pytorch_amd.Aligner / aligner_attention; csrc/aligner.hip): the distance attention of "One TTS
 * Alignment To Rule Them All" / RAD-TTS over encodings q fp32 [B, T, A] and k fp32 [B, K, A], 1 <= A <= vbx_aligner_attn_max_channels()
 * (128: a 64-key chunk of that width fills the LDS tile), 1 <= B <= 65535, B * T < 2^31, any K >= 1; everything else VBX_EINVAL.
 * mask uint8 [B, K], non-zero = a real key, NULL = all real.  fp32 throughout, no atomics, no host synchronisation; the same bits on
 * every run and for a row alone or inside a batch.  u = 2^-24 below.
 * vbx_aligner_attn_fwd, one launch: logprob[b][t][j] = -temperature * sum_c (q[b][t][c] - k[b][j][c])^2, NOT masked, the sum an fp32
 *   fmaf chain over c = 0 .. A - 1 of the rounded differences (never |q|^2 + |k|^2 - 2 q.k, never a 16-bit copy of the encodings):
 *     |logprob - ref| <= (A + 4) u |ref|,  ref the fp64 value from the same fp32 q, k and temperature.
 *   attn[b][t][.] = softmax_j(mask ? logprob : -FLT_MAX) with libm's expf (1 ulp): a masked key gets exactly 0, a row with every key
 *   masked exactly 1 / K.  Against the fp64 softmax p of the kernel's OWN logprob x (m = its row maximum over the kept keys):
 *     |attn - p| <= (|x - m| + sum_j p_j |x_j - m| + ceil(K / 64) + 16) u p + 2^-126
 *   (the subtraction x - m rounds once, which exp turns into |x - m| u; expf and its rounding 4 u per term, in the numerator and,
 *   weighted by p, in the sum; the sum of K positive terms, one serial chain per lane and a 6-step tree, ceil(K / 64) + 6 u; the
 *   division 1 u; 2^-126 where expf underflows).
 * vbx_aligner_attn_bwd: with G = g_logprob + mask * attn * (g_attn - sum_j attn * g_attn) (the masked softmax's backward: no gradient
 *   reaches a filled key, not even on a fully masked row),
 *     dq[b][t][c] = -2 temperature sum_j G[t][j] (q[t][c] - k[j][c]),   dk[b][j][c] = +2 temperature sum_t G[t][j] (q[t][c] - k[j][c]),
 *   each ONE thread's fmaf chain over j = 0 .. K - 1 (t = 0 .. T - 1) in index order, inside the workgroup that owns 16 rows of dq
 *   (dk).  g_logprob or g_attn may be NULL (not both); attn and gmap (scratch, fp32 [B, T, K]) are needed only with g_attn; dq or dk
 *   may be NULL and is then not computed.  With gh = |g_logprob| + attn (|g_attn| + sum_j attn |g_attn|) (what |G| is bounded by)
 *     |dq - ref| <= (K + 32) u 2 temperature sum_j gh[t][j] |q[t][c] - k[j][c]|,   |dk - ref| <= (T + 32) u 2 temperature sum_t (same),
 *   ref in fp64 from the same fp32 operands (n terms of a chain: n + 1; the difference and the final scale: 2; G's own rounding, a
 *   ceil(K / 64) + 6 dot product, the subtraction, the product and the sum: ceil(K / 64) + 10, K <= 1024 assumed for the constant 32;
 *   beyond that it is K + ceil(K / 64) + 16).
 * The convolution stacks are vbx_gemm launches around three small kernels:
 * vbx_aligner_pack: x fp32 [B, T, C] (channel_first: [B, C, T]) -> out 16-bit [B * T, C * taps] (fmt 2: three times as wide), taps
 *   1 or 3, out[b * T + t][c * taps + tap] = act(x[b][t + tap - taps / 2][c]), 0 outside 0 <= t' < T (nn.Conv1d's zero padding of
 *   the padded batch), act = max(., 0) with relu.  fmt 0: fp16 (saturating); 1: bfloat16; 2: the three-piece fp16 row
 *   [hi | hi 2^-8 | lo 2^8] of the precise mode (vbx_split3_f16), to be multiplied with [W_hi | W_lo 2^8 | W_hi 2^-8]: products to
 *   fp32 accuracy on the same GEMM tiles.  Column c * taps + tap is the Conv1d weight's own [Cout, Cin * taps] view: the forward
 *   is NT against it, the dgrad NN, the wgrad TN lands in the weight's layout.
 * vbx_aligner_relu_bwd: g fp32 [n] *= (pre > 0) in place (pre NULL: unchanged) and g_bf16 = bfloat16(g).
 * vbx_aligner_fold: d fp32 [B * T, 3 C] (the dgrad in the packed layout) -> dx[b][t][c] = d[t + 1][3 c] + d[t][3 c + 1] + d[t - 1][3 c + 2]
 *   within a batch row, fp32 [B, T, C] or, channel_first, [B, C, T]. */
int vbx_aligner_attn_max_channels(void);
int vbx_aligner_attn_fwd(const float* q, const float* k, const uint8_t* mask, float temperature, float* attn, float* logprob, int B, int T,
                         int K, int A, void* stream);
int vbx_aligner_attn_bwd(const float* q, const float* k, const uint8_t* mask, const float* attn, const float* g_logprob,
                         const float* g_attn, float temperature, float* gmap, float* dq, float* dk, int B, int T, int K, int A,
                         void* stream);
int vbx_aligner_pack(const float* x, void* out, int B, int T, int C, int taps, int relu, int channel_first, int fmt, void* stream);
int vbx_aligner_relu_bwd(float* g, const float* pre, void* g_bf16, long n, void* stream);
int vbx_aligner_fold(const float* d, float* dx, int B, int T, int C, int channel_first, void* stream);
/* Sample-rate conversion (voicebox_pytorch_amd.resample; csrc/resample.hip): the polyphase windowed-sinc FIR of
 * torchaudio.functional.resample for the REDUCED rate pair orig : nw,
 *   y[r][q * nw + p] = sum_k h[p][k] * x[r][q * orig + k - width],  x = 0 outside [0, L),  p < nw, k < K = 2 * width + orig,
 * x fp32 [rows, L] (1 <= L <= 2^31 - 1), y fp32 [rows, Lout], Lout <= nw * ceil(L / orig) (the caller keeps ceil(nw * L / orig)).
 * The bank is passed compacted: start / len int32 [nw] give, per phase, the run of taps that holds every non-zero of h[p][.]
 * (start[p] + len[p] <= K, len[p] <= run_max), taps fp32 [run_max, nw] holds taps[i][p] = h[p][start[p] + i] (zero past len[p]).
 * Taps outside a run must be exactly 0.0f in the dense bank, so leaving them out changes nothing.  One launch on `stream`, no
 * atomics, the same bits on every run.  K <= vbx_resample_max_taps() (a tile's input span is staged in 64 KiB of LDS). */
int vbx_resample_max_taps(void);
int vbx_resample(const float* x, float* y, const float* taps, const int* start, const int* len, int rows, long L, long Lout, int orig,
                 int nw, int width, int K, int run_max, void* stream);
/* the same rows unrounded (fp32 [B*N, 2*D + E]): precise mode's to_embed operand */
int vbx_embed_input_text_f32(const float* x, const float* cond, const uint8_t* cond_mask, const uint8_t* drop_mask,
                             const float* null_cond, const long* ids, int T, const float* table, int E, long null_id,
                             float* out_f32, int B, int N, int D, void* stream);
int vbx_cond_emb_bwd(const void* demb_bf16, int ld, const long* ids, int T, const uint8_t* drop_mask, long null_id,
                     float* gtable, int B, int N, int E, void* stream);
/* DurationPredictor front end (voicebox_pytorch.py:793-823): out fp16 [B*N, E+D] = [ to_phoneme_emb(max(ids,0)) | cond'' ] with
 * cond'' = curtail_or_pad(where(drop[b], null_cond, cond * ~cond_mask), N); ids [B,N] (-1 = padding), cond fp32 [B,S,D],
 * cond_mask [B,S] (may be NULL), drop_mask [B] (may be NULL).  Feeds vbx_gemm (to_embed, f16 operands). */
int vbx_pack_phoneme_input(const long* ids, const float* table, int E, const float* cond, int S, const uint8_t* cond_mask,
                           const uint8_t* drop_mask, const float* null_cond, void* out_f16, int B, int N, int D, void* stream);
/* The training forward's variant: the same fp16 rows (bit for bit) and, in the same launch, out_bf16 [B*N, E+D], the operand of the
 * to_embed weight gradient, and emb_f32 [B*N, E], the gathered embedding rows unrounded (the aligner's keys).  Either may be NULL. */
int vbx_pack_phoneme_input_train(const long* ids, const float* table, int E, const float* cond, int S, const uint8_t* cond_mask,
                                 const uint8_t* drop_mask, const float* null_cond, void* out_f16, void* out_bf16, float* emb_f32, int B,
                                 int N, int D, void* stream);
/* The same operand for a DurationPredictor over codec latents (attach_codec(); csrc/duration.hip): latent fp32 [B, S, L] goes
 * through proj_in inside the launch,
 *   cond''[b, r] = r >= S ? 0 : drop[b] ? null_cond : cond_mask[b, r] ? 0 : latent[b, r] . W^T + bias      (voicebox_pytorch.py:776-819)
 * -- proj_in at length S, then the mask (a masked row is 0, not the bias), then the drop, then curtail_or_pad to N.  Columns 0:E are
 * the bits vbx_pack_phoneme_input writes.  The product has vbx_proj_in_embed's arithmetic: latents and W rounded once to fp16
 * (saturating), w_f16 = W packed [D, Kp], Kp = vbx_proj_in_kp(L), zero past column L (vbx_pack_weight); fp32 sums in ascending k on
 * v_mfma_f32_16x16x32_f16, bias (fp32 [D]) added in fp32, one rounding to fp16 on store: per element within
 * (L + 2) 2^-24 (sum |w x| + |b|) + 2^-11 |y| of the exact value on the rounded operands.  L in 8 .. 1024, D a multiple of 64, E of 8.
 * _train writes in the same launch out_bf16 [B*N, E+D] and emb_f32 [B*N, E] (may be NULL) as vbx_pack_phoneme_input_train does, and
 * lc_bf16 [B*N, Kp], the operand of proj_in's weight gradient: the latent row with column L = 1, ALL zero on the rows that pass no
 * gradient to proj_in (r >= S, cond_mask set, dropped sample), zero past column L: (d cond'')^T . lc = [ d weight | d bias ], which
 * vbx_proj_in_wgrad_reduce splits.  One launch, no atomics: reruns are bit-identical, and a batch row gives the same bits alone. */
int vbx_pack_phoneme_latent(const long* ids, const float* table, int E, const float* latent, int S, int L, const void* w_f16,
                            const float* bias, const uint8_t* cond_mask, const uint8_t* drop_mask, const float* null_cond, void* out_f16,
                            int B, int N, int D, void* stream);
int vbx_pack_phoneme_latent_train(const long* ids, const float* table, int E, const float* latent, int S, int L, const void* w_f16,
                                  const float* bias, const uint8_t* cond_mask, const uint8_t* drop_mask, const float* null_cond,
                                  void* out_f16, void* out_bf16, float* emb_f32, void* lc_bf16, int B, int N, int D, void* stream);
/* ------------------------------------------------------------------ DurationPredictor training (csrc/duration.hip)
 * The loss of voicebox_pytorch.py:858-866 taken on the PREDICTED durations (the reference writes it on the hidden state, which only
 * broadcasts at degenerate shapes).  All of it fp32, no atomics; every sum runs in an order fixed by the shapes alone, so reruns are
 * bit-identical and a batch row gives the same durations / num / den alone as inside a batch.
 *
 * vbx_duration_head_fwd (two launches): durations[r] = hid[r,:] . w + bias[0] with vbx_rowdot's arithmetic (the same bits);
 *   num[b] = sum_n m |d - t|, den[b] = sum_n m over loss_mask m [B, n] (uint8), loss[0] = (1/B) sum_b num[b] / max(den[b], 1e-5).
 *   Bounds: |d - d64| <= (D + 2) 2^-24 (sum |x w| + |b|); the loss on the kernel's own d within (n + B + 4) 2^-24 of its fp64 value.
 * vbx_duration_head_bwd (two launches): g_r = gscale[0] m sign(d - t) / (B max(den[b], 1e-5)), sign(0) = 0 as torch's l1_loss;
 *   gscale is a device scalar (NULL = 1).  dhid[r,:] = g_r w (fp32 only: the stack's backward takes fp32), two roundings;
 *   dw[D] = sum_r g_r hid[r,:] and db[1] = sum_r g_r through one partial per 32 rows (rows ascending) and one ascending sum over the
 *   partials: within (B n + 2) 2^-24 sum |terms|.  scratch: vbx_duration_head_bwd_scratch_floats(B, n, D) floats.
 * vbx_phoneme_emb_bwd (one launch, one workgroup per table row): gtable[v,:] = sum over the rows r with max(ids[r], 0) == v, in
 *   ascending r, of g_packed[r, 0:E] (row stride ld_packed) + g_emb[r, 0:E] (dense) -- the two consumers of the embedding, either may
 *   be NULL.  Rows of unused ids are exactly 0; every row of gtable [V, E] is written.  Padding positions (-1, clamped to 0)
 *   contribute whatever gradient reaches them, as in the reference.  E <= 2048.  Within (count_v + 2) 2^-24 sum |terms|. */
int vbx_duration_head_fwd(const float* hid, const float* w, const float* bias, const float* target, const uint8_t* loss_mask,
                          float* durations, float* num, float* den, float* loss, int B, int n, int D, void* stream);
long vbx_duration_head_bwd_scratch_floats(int B, int n, int D);
int vbx_duration_head_bwd(const float* hid, const float* w, const float* durations, const float* target, const uint8_t* loss_mask,
                          const float* den, const float* gscale, float* dhid, float* dw, float* db, float* scratch, int B, int n, int D,
                          void* stream);
/* Length regulator (sample(lens="durations")): ids int64 [B][K] (-1 = padding phoneme), durations fp32 [B][K] -> lens int32 [B],
 * lens[b] = sum over ids != -1 of int(max(durations, 1)) (truncation; padding phonemes own no frames), and, unless aligned is NULL,
 * aligned int64 [B][Nmax]: phoneme i's id over its run of frames, 0 from lens[b] on; frames >= Nmax are not written.  One workgroup
 * per row: a prefix sum over K, each thread writes the runs of its phonemes.  Call once with aligned NULL, read lens, allocate. */
int vbx_length_regulate(const long* ids, const float* durations, long* aligned, int* lens, int B, int K, int Nmax, void* stream);
int vbx_phoneme_emb_bwd(const long* ids, const float* g_packed, int ld_packed, const float* g_emb, float* gtable, long rows, int V,
                        int E, void* stream);
/* to_pred = Linear(dim, 1) + squeeze (voicebox_pytorch.py:672-675): out[r] = x[r,:] . w + bias[0]  (bias may be NULL). */
int vbx_rowdot(const float* x, const float* w, const float* bias, float* out, long rows, int D, void* stream);
/* standalone Transformer.forward (voicebox_pytorch.py:417-431, :476-477): residual stream [B,N+R,D] = register tokens (rows
 * n < R) followed by x [B,N,D]; backward: dx = rows n >= R of dxs, dreg[R,D] = sum over the batch of rows n < R. */
int vbx_stack_input(const float* x, const float* reg, float* xs, int B, int N, int R, int D, void* stream);
int vbx_stack_input_bwd(const float* dxs, float* dx, float* dreg /* may be NULL */, int B, int N, int R, int D, void* stream);
/* u-net skip connection (voicebox_pytorch.py:458-463): cat [rows, 2*D] = (x | scale * skip) as fp16 and / or bf16 (the combiner's GEMM operand);
 * backward: dcat fp32 [rows, 2*D] = d(cat) -> dx = dcat[:, :D] (+ bf16 copy), dskip = scale * dcat[:, D:]; and the deferred add of a
 * stored dskip into the gradient of the layer input it was taken from: dx += dskip (+ bf16 copy). */
int vbx_unet_cat(const float* x, const float* skip, float scale, void* cat_f16, void* cat_bf16, long rows, int D, void* stream);
int vbx_unet_split(const float* dcat, float scale, float* dx, void* dx_bf16, float* dskip, long rows, int D, void* stream);
int vbx_unet_addskip(float* dx, void* dx_bf16, const float* dskip, long n, void* stream);
int vbx_convpos_fwd(const float* e, const float* w, const float* bias, const uint8_t* mask, const float* reg,
                    float* xs, int B, int N, int R, int D, int ksize, void* stream);
/* vbx_convpos_fwd with libm's erff in the GELU instead of the fast path's Abramowitz-Stegun form (precise mode) */
int vbx_convpos_fwd_libm(const float* e, const float* w, const float* bias, const uint8_t* mask, const float* reg,
                         float* xs, int B, int N, int R, int D, int ksize, void* stream);
/* conv_embed over packed rows (see "packed rows"): e [Mp, D] = to_embed over every packed row (its register and dead rows are
 * computed and not read), xs [Mp, D]: register rows = reg [R, D], frame row n of a segment = e + GELU(conv) with taps outside
 * 0 <= n < len_b reading 0 (tap order and GELU of vbx_convpos_fwd: a frame is bit-equal to vbx_convpos_fwd on the row alone), dead
 * rows exactly 0.  seg_klen[s] = R + len_b. */
int vbx_convpos_fwd_segs(const float* e, const float* w, const float* bias, const float* reg, const int* seg_start,
                         const int* seg_klen, const int* tile_seg, float* xs, int Mp, int R, int D, int ksize, void* stream);
/* ksize: any odd kernel size <= 31 (the reference default is 31, voicebox_pytorch.py:893; one unrolled instantiation per size).
 * backward: de = dxs[:,R:] + conv-transpose(...) ; dw/db partials [chunks][D][ksize+1]; dreg [R,D]. */
int vbx_convpos_bwd(const float* e, const float* w, const float* bias, const uint8_t* mask, const float* dxs,
                    float* dpre_tmp /* fp32 [B,N,D] scratch */, float* de, void* de_bf16,
                    float* wpart /* [chunks][D][64]: k<ksize weight grads, [63] bias grad */, float* dreg, int B, int N,
                    int R, int D, int ksize, void* stream);
int vbx_convpos_bwd_chunks(int B, int N);
/* dw[d][k] = sum_chunks wpart[.][d][k], db[d] = sum_chunks wpart[.][d][63] */
int vbx_conv_wgrad_finalize(const float* wpart, int chunks, int D, int ksize, float* dw, float* db, void* stream);
/* time embedding: LearnedSinusoidalPosEmb -> Linear -> SiLU (voicebox_pytorch.py:163-167,916-920) */
int vbx_time_embed_fwd(const float* times, const float* w_sin, const float* w1, const float* b1, float* four,
                       float* pre, float* temb, int B, int D, int Th, void* stream);
int vbx_time_embed_bwd_scratch_floats(int B, int D);
int vbx_time_embed_bwd(const float* times, const float* w_sin, const float* w1, const float* four, const float* pre,
                       const float* dtemb, float* dw_sin, float* dw1, float* db1, float* scratch /* vbx_time_embed_bwd_scratch_floats */, int B,
                       int D, int Th, void* stream);
/* all adaLN projections at once: ada[b][j] = bias[j] + sum_t temb[b][t] * W[j][t],  W fp16 [J,Th]
 * (J = depth*2 norms*(gamma,beta)*D) (voicebox_pytorch.py:273). */
int vbx_adaln_proj_fwd(const float* temb, const void* w_bf16, const float* bias, float* ada, int B, int Th, int J,
                       int group /* output layout ada[j/group][b][j%group]; <=0 or J: plain [b][j] */, void* stream);
/* dW[j][t] = sum_b dada[b][j]*temb[b][t] (fp32 [J,Th]), dbias[j] = sum_b dada[b][j],
 * dtemb[b][t] = sum_j dada[b][j] * W[j][t]. */
int vbx_adaln_proj_bwd(const float* temb, const void* w_bf16, const float* dada, float* dw, float* dbias, float* dtemb,
                       float* scratch, int B, int Th, int J, int accumulate_dtemb, void* stream);
int vbx_adaln_proj_bwd_scratch_floats(int B, int Th, int J);
/* d(time_emb) of EVERY layer's projections in one launch (+ one reduction): dtemb[b][t] = sum over l, j of dada[l][b][j] * W[l][j][t];
 * W fp16 [L][J][Th] (the packed arena's order), dada fp32 [L][B][J], scratch vbx_adaln_dtemb_all_scratch_floats() floats.  With the
 * weight gradient kept in factor form (vbx_model.adaln_factors) and the bias gradient taken from the norm partial records, this is all
 * that is left of the adaLN backward: once per step instead of two launches per layer. */
long vbx_adaln_dtemb_all_scratch_floats(int L, int B, int Th, int J);
int vbx_adaln_dtemb_all(const void* w_f16, const float* dada, float* dtemb, float* scratch, int L, int B, int Th, int J, void* stream);
/* reduce rmsnorm_bwd partials over chunks: out[b][2][D] = sum_chunk part[b][chunk][2][D] */
int vbx_reduce_norm_partials(const float* part, float* out, long out_b_stride, int B, int chunks, int D, int sum_batch,
                             void* stream);
/* out[d] = sum_{b,chunk} colpart[b][chunk][d]  (the fused column sums of vbx_rmsnorm_bwd) */
int vbx_reduce_col_partials(const float* colpart, float* out, float* tmp /* B*D floats */, int B, int chunks, int D,
                            void* stream);
/* GEGLU backward on the interleaved pre-activation (voicebox_pytorch.py:338-340) */
int vbx_geglu_bwd(const void* h1_bf16, const void* dg_bf16, void* dh1_bf16, int M, int Fp, void* stream);
/* column sums: out[c] (+)= sum_r in[r][c]   (bias grads) ; rowmap as in vbx_splitk_reduce */
int vbx_colsum_bf16(const void* in_bf16, int M, int C, int ld, float* out, int out_len, int rowmap, int F,
                    float* scratch, void* stream);
int vbx_colsum_f32(const float* in, int M, int C, int ld, float* out, float* scratch, void* stream);
int vbx_colsum_scratch_floats(int M, int C);
/* out[j] (+)= sum_{i<rows} in[i*ld + j], j < cols   (partials -> gradients) */
int vbx_sum_rows_f32(const float* in, long rows, long ld, float* out, long cols, int accumulate, void* stream);
/* rows of the gpart buffer of vbx_qknorm_rope_bwd per `which`: gpart is [2][rows][H][64] */
int vbx_qknorm_rope_bwd_gpart_rows(int B);
/* masked MSE (voicebox_pytorch.py:1099-1115): loss scalar fp32; per_b: vbx_masked_mse_scratch_floats(B) floats
 * ([0,B) per-sample loss, [B,2B) denominators, then partial sums). */
int vbx_masked_mse_scratch_floats(int B);
int vbx_masked_mse_fwd(const float* pred, const float* target, const uint8_t* loss_mask, float* per_b, float* loss,
                       int B, int N, int D, void* stream);
int vbx_masked_mse_bwd(const float* pred, const float* target, const uint8_t* loss_mask, const float* per_b,
                       const float* gscale /* device scalar d(loss) or NULL (=1) */, float* dpred, void* dpred_bf16, int B,
                       int N, int D, void* stream);
/* CFM inputs (voicebox_pytorch.py:1404-1410): w = (1-(1-sigma)t)x0 + t x1 ; flow = x1-(1-sigma)x0 */
int vbx_cfm_inputs(const float* x1, const float* x0, const float* times, float sigma, float* w, float* flow, int B,
                   long per_batch, void* stream);
/* Span mask and loss mask of the CFM objective from the drawn numbers (voicebox_pytorch.py:121-150, :1099), as masks.py computes
 * them with torch, operation by operation in the same types -- equal byte for byte:
 *   lengths = trunc(frac[b] * N) (one fp32 product), start = max(fp32(N - lengths) * rand[b], 0), end = start + fp32(lengths),
 *   cond_mask[b][n] = trunc(start) <= n < trunc(end);  loss_mask = cond_mask & pad_mask & (n < key_lens[b] - R).
 * frac, rand fp32 [B]; pad_mask uint8 [B, N] or NULL; key_lens int32 [B] (R + the row's frame count, vbx_io.key_lens) or NULL;
 * cond_mask, loss_mask uint8 [B, N] (0 / 1; loss_mask may be NULL).  vbx_cfm_inputs_masks is vbx_cfm_inputs and vbx_span_masks in one
 * launch (per_batch = N * the latent width); both leave what the separate launches leave. */
int vbx_span_masks(const float* frac, const float* rand, const uint8_t* pad_mask, const int* key_lens, int R, int B, int N,
                   uint8_t* cond_mask, uint8_t* loss_mask, void* stream);
int vbx_cfm_inputs_masks(const float* x1, const float* x0, const float* times, float sigma, float* w, float* flow, int B, long per_batch,
                         const float* frac, const float* rand, const uint8_t* pad_mask, const int* key_lens, int R, int N,
                         uint8_t* cond_mask, uint8_t* loss_mask, void* stream);
/* The finishing kernels of vbx_model_backward_embed in two launches, each job with the body, the block indices and so the bits of
 * its own kernel:
 *   vbx_embed_bwd_tail1 = the d(register tokens) launch of vbx_convpos_bwd (dreg [R, D] from dxs [B, Np, D]; R = 0: none),
 *                         vbx_conv_wgrad_finalize(wpart, chunks, D, ksize, dw, db) and the first two launches of vbx_time_embed_bwd
 *                         (dw1, db1; the d(four) partials into tscratch, vbx_time_embed_bwd_scratch_floats(B, D) floats);
 *   vbx_embed_bwd_tail2 = vbx_splitk_reduce(slabs, splits, M, N, dst, M, N, N, 0, 0, 0), the second stage of vbx_colsum_f32 over
 *                         the slabs vbx_colsum_f32_partials left in cs_scratch (C columns -> dbias) and the third launch of
 *                         vbx_time_embed_bwd (d(four) = the sum of the partials, into tscratch[0 .. B * D));
 *   vbx_time_embed_bwd_wsin = the fourth launch of vbx_time_embed_bwd (dfour = tscratch). */
int vbx_embed_bwd_tail1(const float* dxs, float* dreg, int B, int Np, int R, int D, const float* wpart, int chunks, int ksize, float* dw,
                        float* db, const float* four, const float* pre, const float* dtemb, const float* w1, float* dw1, float* db1,
                        float* tscratch, int Th, void* stream);
int vbx_embed_bwd_tail2(const float* slabs, int splits, int M, int N, float* dst, const float* cs_scratch, int C, float* dbias,
                        float* tscratch, int B, int D, void* stream);
int vbx_time_embed_bwd_wsin(const float* times, const float* four, const float* dfour, float* dw_sin, int B, int D, void* stream);
/* first stage of vbx_colsum_f32 only: scratch[vbx_colsum_slabs()][C] */
int vbx_colsum_f32_partials(const float* in, int M, int C, int ld, float* scratch, void* stream);
/* y_out = y + coef[idx] * f   (ODE midpoint axpy; coef device-resident so graphs hold no host scalars) */
int vbx_axpy_dev(const float* y, const float* f, const float* coef, int idx, float* out, long n, void* stream);
/* hipGraph-replayable ODE step helpers (replace the host-side loop of torchdiffeq.odeint, call site
 * voicebox_pytorch.py:1295): dt comes from a device table [2*intervals] indexed by a device counter,
 * slot 0/1 of interval i at table[2*i + slot] (the times likewise: vbx_ode_stage_time with stride 2). */
int vbx_axpy_ctr(const float* y, const float* f, const float* table, const int* counter, int slot, float* out, long n,
                 void* stream);
int vbx_counter_add(int* counter, int inc, void* stream);
/* Sampling: every batch element of a call shares the ODE time, and the grid is known up front, so the time embedding + the adaLN
 * projections of ALL time points (voicebox_pytorch.py:1082, :273 -- a 100 MB weight stream per function evaluation at dim 512 / depth
 * 12) are evaluated once per sample() into table [stride * intervals][L][G] (G = 4 * D: gamma1 | beta1 | gamma2 | beta2 of a layer; stride >= 1
 * time points per interval); this copies the slice of time point stride * counter + slot, 0 <= slot < stride, into the runtime's ada
 * [L][B][G] (vbx_io.ada_table / ada_stride make vbx_model_forward do it). */
int vbx_ada_select(float* ada, int L, int B, int G, const float* table, const int* counter, int stride, int slot, void* stream);
/* ------------------------------------------------------------------ ODE solvers (csrc/ode.hip; solver.py RKSampler / Dopri5Sampler)
 * torchdiffeq.odeint's euler, rk4 (3/8 rule) and dopri5 (call site voicebox_pytorch.py:1295; restated in tests/ode_ref.py -- parity
 * with the library UNPINNED).  States are fp32 [n] (n = B * N * D, a multiple of 4, 16-byte aligned); k is a HOST array of S <= 7
 * device pointers (the stage derivatives), read at launch -- captured graphs keep them.  Nothing here reads a host scalar that
 * changes between replays: fixed grids index device tables with a device counter, dopri5 reads its fp64 step state.
 * Fixed grids: out = y + sum_j c_j k_j, c_j = table[(stride * counter[0] + row) * ld + j] (one row per stage input and one for the
 * step's weights; RKSampler builds them on the host in fp32), and times[b] = table[stride * counter[0] + slot] for every b. */
#define VBX_ODE_MAX_STAGES 7
int vbx_ode_combine(float* out, const float* y, const float* const* k, int S, const float* table, int ld, const int* counter,
                    int stride, int row, long n, void* stream);
int vbx_ode_stage_time(float* times, int B, const float* table, const int* counter, int stride, int slot, void* stream);
/* dopri5 step state: VBX_DP_STATE doubles of device memory.  The host writes T (= t0), TEND, ATOL, RTOL and zeroes the rest before
 * the initial step; afterwards only vbx_ode_norm's controller writes it.  T / DT: start and size of the next attempt (fp64); T0 / T1
 * / DT32: the last accepted step (DT32 = fp32(dt)); H0 / D1: initial-step intermediates; NFE, ACCEPTED, REJECTED: counts; LAST: the
 * last attempt was accepted; DONE: T >= TEND; BAD: 1 non-finite error norm, 2 step-size underflow (the host raises). */
enum {
  VBX_DP_T = 0, VBX_DP_DT, VBX_DP_T0, VBX_DP_T1, VBX_DP_DT32, VBX_DP_RATIO, VBX_DP_H0, VBX_DP_D1, VBX_DP_NFE, VBX_DP_ACCEPTED,
  VBX_DP_REJECTED, VBX_DP_LAST, VBX_DP_DONE, VBX_DP_BAD, VBX_DP_ATOL, VBX_DP_RTOL, VBX_DP_TEND, VBX_DP_STATE = 20
};
/* out = y + sum_j (beta_j * fp32(state[dt_slot])) k_j, beta a HOST array of S fp32 tableau entries; dt_slot VBX_DP_DT (a stage input)
 * or VBX_DP_H0 (the initial-step probe y0 + h0 f0, beta = {1}) */
int vbx_ode_combine_dp(float* out, const float* y, const float* const* k, const float* beta, int S, const double* state, int dt_slot,
                       long n, void* stream);
/* times[b] = STAGE: fp32(T) + alpha * fp32(DT) in fp32; END (c = 1): the fp32 value below fp32(T + DT) (torchdiffeq Perturb.PREV);
 * PROBE: fp32(T + H0) */
enum { VBX_ODE_TIME_TABLE = 0, VBX_ODE_TIME_STAGE = 1, VBX_ODE_TIME_END = 2, VBX_ODE_TIME_PROBE = 3 };
int vbx_ode_stage_time_dp(float* times, int B, const double* state, float alpha, int mode, void* stream);
/* RMS norms over the whole state and the step-size control, deterministic, two launches: per-workgroup fp64 partial sums of squares
 * into slab (vbx_ode_norm_slab_doubles(n) doubles), then one workgroup sums it in a fixed order and updates state.
 *   ERROR (S = 7, c = the error weights): ratio = rms(err / (atol + rtol max(|y0|, |y1|))), err = sum_j (c_j fp32(DT)) k_j, not
 *     stored; accept iff ratio <= 1 (T0, T1, DT32, T advance; DONE), DT *= min(10, max(0.9 ratio^-1/5, ratio < 1 ? 1 : 0.2)) (x10
 *     at ratio 0); NFE += 6 nfe_per_eval.
 *   INIT0 (S = 1, k = {f0}): d0 = rms(y0 / scale), d1 = rms(f0 / scale), scale = atol + |y0| rtol -> H0 = d0 < 1e-5 || d1 < 1e-5 ?
 *     1e-6 : 0.01 d0 / d1 (fp32); NFE += nfe_per_eval.
 *   INIT1 (S = 2, k = {f0, f1}): d2 = rms((f1 - f0) / scale) / H0 -> DT = min(100 H0, (0.01 / max(d1, d2))^1/5) (1e-3 H0, at least
 *     1e-6, when both are <= 1e-15); NFE += nfe_per_eval. */
enum { VBX_ODE_NORM_ERROR = 0, VBX_ODE_NORM_INIT0 = 1, VBX_ODE_NORM_INIT1 = 2 };
enum { VBX_ODE_CTRL_STEP = 0, VBX_ODE_CTRL_INIT0 = 1, VBX_ODE_CTRL_INIT1 = 2 };
long vbx_ode_norm_slab_doubles(long n);
int vbx_ode_norm(double* state, double* slab, int mode, const float* y0, const float* y1, const float* const* k, const float* c, int S,
                 long n, int nfe_per_eval, void* stream);
/* vbx_ode_norm over the real frames of a padded batch (sample(lens=)): the state is [B][N][row_elems], N = n / (B row_elems),
 * row_elems a multiple of 4; every element of a frame >= lens[b] (int32 [B], device) leaves both the sums of squares and the count
 * (n becomes row_elems sum_b lens[b]) and is not read.  Same two launches, same grid and summation order: with lens == NULL or every
 * lens[b] == N the state gets the bits vbx_ode_norm writes. */
int vbx_ode_norm_lens(double* state, double* slab, int mode, const float* y0, const float* y1, const float* const* k, const float* c,
                      int S, long n, int nfe_per_eval, const int* lens, int B, int row_elems, void* stream);
/* x[b][n][:] = 0 for n >= lens[b]; x fp32 [B][N][D], lens int32 [B] on the device */
int vbx_zero_tail_rows(float* x, const int* lens, int B, int N, int D, void* stream);
/* after an attempt: if LAST && !DONE, y <- y1 and k1 <- k7 (first-same-as-last); the last accepted step stays for vbx_ode_dense */
int vbx_ode_commit(float* y, float* k1, const float* y1, const float* k7, const double* state, long n, void* stream);
/* dense output at TEND inside the last accepted step [T0, T1] (torchdiffeq _interp_fit / _interp_evaluate): y_mid = y0 + sum_j
 * (mid_j DT32) k_j, then the quartic through y0, y_mid, y1 with slopes DT32 k1 and DT32 k7, at x = fp32((TEND - T0) / (T1 - T0));
 * k = k1 .. k7, mid a HOST array of 7 fp32 */
int vbx_ode_dense(float* out, const float* y0, const float* y1, const float* const* k, const float* mid, const double* state, long n,
                  void* stream);
/* Occupies `stream` with one idle wave for `us` microseconds (0 .. 10000).  The sampler integrates the two halves of a batch as two
 * graphs on two streams and starts the second one ~60 us late, so that different kernels of the two forwards overlap (attention
 * beside GEMMs) instead of the same ones: 16 intervals 81.7 -> 80.1 ms (tools/sample_offset.py). */
int vbx_stream_delay(float us, void* stream);
/* fp32 -> bf16 and/or fp16 weight packing with optional row map / K padding:
 * dst[p][c] = (src row of p valid && c < src_cols) ? src[row][c] : 0 ; dst is [dst_rows, dst_cols] */
int vbx_pack_weight(const float* src, int src_rows, int src_cols, void* dst_bf16 /* or NULL */, void* dst_f16 /* or NULL */,
                    int dst_rows, int dst_cols, int rowmap, int F, void* stream);
int vbx_pack_bias(const float* src, int n, float* dst, int dst_n, int rowmap, int F, void* stream);
/* ------------------------------------------------------------------ GateLoop (optional layer, use_gateloop_layers)
 * gateloop_transformer.SimpleGateLoopLayer(dim, post_ln=True), call sites voicebox_pytorch.py:399,465-466 (third-party,
 * restated in oracle/restate.py:gateloop -- parity unpinned).  qkva = RMSNorm(x) W^T is produced by vbx_rmsnorm_fwd +
 * vbx_gemm; these entries are the gated linear scan and the post-LayerNorm.
 * scan fwd: a = sigmoid(qkva[..,2D:]); h_t = a_t h_{t-1} + qkva[..,D:2D]_t; s_t = qkva[..,:D]_t h_t.
 *   qkva [B,Np,3D] fp32, s [B,Np,D] fp32, hstate [B,Np,D] fp32 or NULL (kept for the backward).
 * scan bwd: ds [B,Np,D] fp32 -> d(qkva) bf16 [B,Np,3D] (sigmoid derivative applied). */
int vbx_gateloop_scan_fwd(const float* qkva, float* s, float* hstate, int B, int Np, int D, void* stream);
int vbx_gateloop_scan_bwd(const float* qkva, const float* hstate, const float* ds, void* dqkva_bf16, int B, int Np, int D,
                          void* stream);
/* y = LayerNorm(s) * w + bias (+ resid), rows of D (biased variance, eps as nn.LayerNorm). */
int vbx_layernorm_fwd(const float* s, const float* w, const float* bias, const float* resid, float* y, long rows, int D,
                      float eps, void* stream);
/* ds and per-16-row partial records part[B][ceil(Np/16)][2][D] (dw | dbias), to be summed by vbx_reduce_norm_partials. */
int vbx_layernorm_bwd(const float* s, const float* w, const float* dy, float* ds, float* part, int B, int Np, int D, float eps,
                      void* stream);

/* Several vbx_splitk_reduce jobs in one launch (e.g. the four weight gradients of a layer, each with its own slab region). */
#define VBX_SKR_MAX 6
typedef struct {
  const float* slabs;
  float* dst;
  float* sq;  /* NULL, or vbx_splitk_reduce_blocks(M, N) floats: sq[b] = sum of squares of the values block b stored (a fixed summation
                 order: the same bits on every run) -- the gradient-norm terms of this tensor without a second pass over it */
  int splits, M, N, dst_rows, dst_cols, dst_ld, rowmap, F, block0, pad_;
} vbx_skr_job;
typedef struct {
  vbx_skr_job job[VBX_SKR_MAX];
  int n;
} vbx_skr_jobs;
int vbx_splitk_reduce_multi(const vbx_skr_jobs* jobs, void* stream);
int vbx_splitk_reduce_blocks(int M, int N); /* blocks (= sq partials) of one job */
/* Several small column reductions in one launch: for job i, out[b][map(c)] = sum over r < rows of
 * src[b*src_bstride + r*row_stride + c], c < cols, b < batches; map = identity or the GEGLU row un-interleave (rowmap = 1, F), columns
 * mapping outside [0, dst_len) are dropped.  block0 is filled in by the library. */
#define VBX_MR_MAX 48
typedef struct {
  const float* src;
  float* dst;
  long src_bstride, dst_bstride, row_stride;
  int rows, cols, batches, dst_len, rowmap, F, block0, pad_;
} vbx_mr_job;
typedef struct {
  vbx_mr_job job[VBX_MR_MAX];
  int n;
} vbx_mr_jobs;
int vbx_multi_reduce(const vbx_mr_jobs* jobs, void* stream);
/* vbx_splitk_reduce_multi(sjobs) and vbx_multi_reduce(mjobs) as ONE launch (the end of a layer's backward); results bit-identical */
int vbx_layer_reduce(const vbx_skr_jobs* sjobs, const vbx_mr_jobs* mjobs, void* stream);
/* vbx_geglu_bwd that also writes per-slab column sums of dh1: scratch[vbx_geglu_bwd_colsum_slabs()][2*Fp] (same interleaved column
 * order as dh1; finish with vbx_multi_reduce + the GEGLU row un-interleave) -- the FeedForward[0].bias gradient without a second
 * pass over dh1 */
int vbx_geglu_bwd_colsum_slabs(void);
int vbx_geglu_bwd_colsum(const void* h1_bf16, const void* dg_bf16, void* dh1_bf16, int M, int Fp, float* scratch, void* stream);
/* first stage of vbx_colsum_bf16 only: scratch[vbx_colsum_slabs()][C] partial column sums (finish with vbx_multi_reduce) */
int vbx_colsum_bf16_partials(const void* in_bf16, int M, int C, int ld, float* scratch, void* stream);
int vbx_colsum_slabs(void);

/* fused Adam (torch.optim.Adam semantics, no weight decay/amsgrad) over a flat fp32 buffer; grads are
 * pre-multiplied by *gscale (device scalar, e.g. clip coefficient) if non-NULL. */
int vbx_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  int step, const float* gscale, void* stream);
/* Adam over the flat buffer that ALSO refreshes the packed fp16/bf16 operand copies of the weights it updates, so the
 * next forward needs no vbx_model_pack_weights pass (62 pack launches and a second read of every parameter per step).
 * The flat buffer is described by segments [off, off+count) that tile [0, n): plain ones (dst all NULL) and packed ones
 * (a [rows, cols] weight written to dst_bf16 / dst_f16 with row stride dst_ld, or a bias copied to dst_f32; rowmap = 1
 * applies the GEGLU row interleave of vbx_pack_weight).  vbx_model_adam_segments() writes the table of a model into
 * HOST memory (returns the count, or a negative VBX_E* code; call with out = NULL to size it); the caller keeps a DEVICE
 * copy and hands it to vbx_adam_step_packed(). */
typedef struct {
  long off, count;  /* floats, inside the flat buffer */
  void* dst_bf16;
  void* dst_f16;
  float* dst_f32;
  int cols, dst_ld, rowmap, F;
  long block0;      /* first 2048-element block of this segment in the launch grid */
} vbx_adam_seg;
int vbx_adam_step_packed(float* p, const float* g, float* m, float* v, const vbx_adam_seg* segs_dev, int nsegs,
                         long total_blocks, float lr, float beta1, float beta2, float eps, int step, const float* gscale,
                         void* stream);
/* sum of squares of a flat buffer -> out[0] (two-stage, deterministic) ; scratch >= 1024 floats */
int vbx_sumsq(const float* x, long n, float* out, float* scratch, void* stream);
/* ---- adaLN projection weight gradients in FACTOR form (round 5; vbx_model.adaln_factors).  The gradient of a layer's adaLN weight
 * block W_l [J4 = 4 D, Th] (voicebox_pytorch.py:256-276: to_gamma / to_beta of the two AdaptiveRMSNorms, contiguous) is
 * dada_l^T . temb with dada_l [B, J4] and temb [B, Th] -- half of all parameters, defined by B * (J4 + Th) numbers.  In factor
 * mode the backward entry points leave that block of the gradient buffer UNWRITTEN and the optimizer works from the factors:
 *   vbx_sumsq_adaln_factors : the L * B * B terms (dada_l[b] . dada_l[b']) (temb[b] . temb[b']) whose sum over (b, b') is
 *                             |dada_l^T . temb|_F^2 -> out[(l * B + b) * B + b'];
 *   vbx_sumsq_ranges        : sum of squares over n <= 64 ranges [lo, hi) of x (host array of 2 n longs, multiples of 4 floats)
 *                             plus n_extra values already stored at scratch[1024 ..) -> out[0]; scratch >= 1024 + n_extra floats;
 *   vbx_adam_adaln_factors  : torch.optim.Adam (as vbx_adam_step) on the L blocks at flat offsets w_off[l] with the gradient
 *                             expanded on the fly, refreshing the fp16 operand copies dst_f16[l] ([J4][Th]; may be NULL).
 * vbx_model_adaln_factors gives the factor pointers and the block offsets of a model's training arena. */
int vbx_sumsq_adaln_factors(const float* dada /* [L][B][J4] */, const float* temb /* [B][Th] */, int L, int B, int J4, int Th,
                            float* out /* [L * B * B] */, void* stream);
/* dw [J4, Th] = dada^T . temb for any B (the data-parallel exchange gathers every rank's factors and expands the summed gradient
 * locally: dp.GradBucketReducer(adaln_factors=...)) */
int vbx_adaln_expand_dw(const float* temb /* [B][Th] */, const float* dada /* [B][J4] */, float* dw, int B, int Th, int J4, int reserved,
                        void* stream);
int vbx_sumsq_ranges(const float* x, const long* ranges /* host [2 n] */, int n, int n_extra, float* out, float* scratch, void* stream);
int vbx_adam_adaln_factors(float* p, float* m, float* v, const long* w_off /* host [L] */, void* const* dst_f16 /* host [L] or NULL */,
                           const float* dada, const float* temb, int L, int B, int J4, int Th, float lr, float beta1, float beta2,
                           float eps, int step, const float* gscale, void* stream);
/* ---- EMA of the weights inside the Adam launches (dp.TrainStep(ema_decay=)).  The three _ema entry points are the Adam entry points
 * above with two more arguments behind v: `ema`, an fp32 buffer with the layout of p, and the decay d = ema_decay.  The thread that
 * stores the updated fp32 weight p' (and its fp16 / bf16 copies) also reads and writes the element of `ema` at the same index:
 *     e' = fmaf(d, e - p', p')                                   (fp32; one subtraction, one fused multiply-add)
 * Rules that take no tolerance: d == 0 stores the bits of p'; e == p' stores the bits of p' (p' = -0 excepted: the sum is +0); an
 * element the launch does not touch -- a frozen range or a gap the segment table leaves out, padding, anything behind n -- keeps its
 * bits; reruns are bit-identical (no atomics).  Per element, given the device's own p' and the previous e,
 *     |e' - exact| <= u (d |e - p'| + |exact|),   exact = p' + d (e - p'),   u = 2^-24
 * (two roundings: the subtraction's, scaled by d, and the fused multiply-add's).  p, m, v and every operand copy get the bits the entry point without _ema gives them; those
 * entry points and the kernels they launch are unchanged (the EMA = false instantiation of the same template).
 * Refused (VBX_EINVAL, nothing launched): ema == NULL, ema == p, an `ema` whose address differs from p's modulo 16 bytes (the 16-byte
 * accesses of the vector arms are taken at the same element index in both), ema_decay outside [0, 1), and whatever the entry point
 * without _ema refuses. */
int vbx_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, float ema_decay, long n, float lr, float beta1,
                      float beta2, float eps, int step, const float* gscale, void* stream);
int vbx_adam_step_packed_ema(float* p, const float* g, float* m, float* v, float* ema, float ema_decay, const vbx_adam_seg* segs_dev,
                             int nsegs, long total_blocks, float lr, float beta1, float beta2, float eps, int step, const float* gscale,
                             void* stream);
int vbx_adam_adaln_factors_ema(float* p, float* m, float* v, float* ema, float ema_decay, const long* w_off /* host [L] */,
                               void* const* dst_f16 /* host [L] or NULL */, const float* dada, const float* temb, int L, int B, int J4,
                               int Th, float lr, float beta1, float beta2, float eps, int step, const float* gscale, void* stream);
/* a[i] <-> b[i] for i < n, in place: 16-byte accesses when both pointers are 16-byte aligned (scalar ones otherwise) and a scalar
 * tail of n % 4 elements.  The buffers must not overlap; n > 0.  (TrainStep.ema_weights() serves the average without a temporary.) */
int vbx_swap_f32(float* a, float* b, long n, void* stream);
/* gradient-clip coefficient for a buffer holding the SUM over `world` ranks (inv_world = 1/world):
 * norm = sqrt(sumsq)*inv_world; coef[0] = min(1, max_norm/(norm+1e-6)) * inv_world (max_norm <= 0: no clipping);
 * coef[1] = norm.  (accelerator.clip_grad_norm_, trainer.py:274-275) */
int vbx_clip_coef(const float* sumsq, float max_norm, float inv_world, float* coef /* [2] */, void* stream);

/* ---- LoRA adapters on the fp32 master weights (csrc/lora.hip; voicebox_pytorch_amd/lora.py, dp.TrainStep).  An adapted matrix
 * W [N, K] (an nn.Linear weight's own [out, in] layout, in its slot of the flat parameter buffer) holds W0 + scale . B . A with
 * A [r, K], B [N, r], 1 <= r <= 64, scale = alpha / r.  W0 lives in a separate store; A and B in a small flat buffer `lflat` whose
 * layout the gradient buffer `glflat` shares.  One descriptor per adapted matrix; a table covers all targets of all layers and every
 * entry point below is ONE grouped launch over it (vbx_lora_grad: two).  vbx_lora_plan checks a HOST table against the buffer sizes
 * (every range inside its buffer) and fills the launch fields; the caller keeps a DEVICE copy of the filled table.
 *   vbx_lora_apply  per element: acc = 0; for j ascending: acc = fmaf(B[n, j], A[j, k], acc); W[n, k] = fmaf(scale, acc, W0[n, k]).
 *                   |W - exact| <= (r + 2) 2^-24 (|W0| + |scale| sum_j |B A|) per element; acc == 0 (B = 0) stores the bits of W0;
 *                   reruns are bit-identical.
 *   vbx_lora_grad   reads dW [N, K] at w_off of `gflat` (the materialised weight gradient the backward wrote there) ONCE and writes
 *                   dB[n, j] = scale . sum_k dW[n, k] A[j, k] and dA[j, k] = scale . sum_n B[n, j] dW[n, k] into glflat at b_off / a_off.
 *                   fp32 fmaf chains in a fixed order (tiles of 128 rows x 256 columns, ascending inside a tile, tile partials added
 *                   in ascending order), no atomics: reruns are bit-identical and an entry's result does not depend on the rest of
 *                   the table.  Per element |dB - exact| <= (K + 2) 2^-24 |scale| sum_k |dW A| and
 *                   |dA - exact| <= (N + 2) 2^-24 |scale| sum_n |B dW|.  scratch: scratch_floats of vbx_lora_plan. */
typedef struct {
  long w_off;        /* W in the flat parameter buffer, dW in the flat gradient buffer (floats) */
  long w0_off;       /* W0 in the W0 store */
  long a_off, b_off; /* A [r, K] and B [N, r] in lflat; dA and dB in glflat */
  int N, K, r;
  float scale;
  long blk0, tile0, red0, pa_off, pb_off; /* filled by vbx_lora_plan: grid prefixes and the partials' places in scratch */
} vbx_lora_desc;
int vbx_lora_plan(vbx_lora_desc* descs_host, int n, long flat_floats, long w0_floats, long lflat_floats, long* apply_blocks,
                  long* grad_tiles, long* reduce_blocks, long* scratch_floats, int* max_rank, int* max_k);
int vbx_lora_apply(float* flat, const float* w0, const float* lflat, const vbx_lora_desc* descs_dev, int n, long apply_blocks, int max_k,
                   void* stream);
int vbx_lora_grad(const float* gflat, const float* lflat, float* glflat, const vbx_lora_desc* descs_dev, int n, long grad_tiles,
                  long reduce_blocks, int max_rank, float* scratch, void* stream);

/* ------------------------------------------------------------------ stage-level runtime
 * The whole VoiceBox forward / backward as native sequences of launches (no host sync, no allocation:
 * hipGraph-capturable).  Replaces VoiceBox.forward (voicebox_pytorch.py:987-1115) incl.
 * Transformer.forward (:412-479) and, for the backward entry points, their autograd graph.
 * The caller (Python) owns three arenas: flat fp32 parameters (+ same-layout gradients), the packed
 * bf16 weight arena and the activation arena (sizes from the *_bytes queries). */
enum { VBX_P_SINW = 0, VBX_P_T1W, VBX_P_T1B, VBX_P_EMBW, VBX_P_EMBB, VBX_P_CONVW, VBX_P_CONVB, VBX_P_REG, VBX_P_FNG,
       VBX_P_PREDW,
       VBX_P_CEMB /* to_cond_emb.weight [num_cond_tokens + 1, E], read only when vbx_model.E > 0 */,
       VBX_P_PINW /* proj_in.weight [D, Lc] and */, VBX_P_PINB /* proj_in.bias [D], read only when vbx_model.Lc > 0 */, VBX_NG };
/* per layer; the four adaLN weights, and the four adaLN biases, must be contiguous in this order; so must the GateLoop
 * post-LayerNorm weight and bias (GLLNW, GLLNB).  The four GL* slots are read only when vbx_model.gateloop != 0. */
enum { VBX_L_G1W = 0, VBX_L_B1W, VBX_L_G2W, VBX_L_B2W, VBX_L_G1B, VBX_L_B1B, VBX_L_G2B, VBX_L_B2B, VBX_L_QG, VBX_L_KG,
       VBX_L_QKVW, VBX_L_OUTW, VBX_L_FF1W, VBX_L_FF1B, VBX_L_FF2W, VBX_L_FF2B, VBX_L_GLG, VBX_L_GLW, VBX_L_GLLNW, VBX_L_GLLNB,
       VBX_L_N1G, VBX_L_N2G /* plain RMSNorm gammas, read only when vbx_model.plain_norm != 0 */,
       VBX_L_SKW, VBX_L_SKB /* u-net skip combiner Linear(2 * dim, dim) of the second-half layers, read only when vbx_model.unet != 0 */,
       VBX_NL };

typedef struct {
  int B, N, R, D, H, F, Th, L, ksize;
  int qk_norm;            /* attn_qk_norm (voicebox_pytorch.py:897) */
  float attn_scale;       /* Attend scale: 10 with qk-norm, dim_head^-0.5 otherwise (:304, attend.py:111) */
  int training;           /* 1: keep every activation needed by the backward entry points */
  float* params;          /* flat fp32 master parameters */
  float* grads;           /* flat fp32 gradients, same offsets (NULL in eval) */
  const long* off;        /* HOST array [VBX_NG + L*VBX_NL] of offsets (in floats) into params/grads */
  void* wpack;            /* packed bf16 weight arena */
  void* act;              /* activation arena */
  const float* rot_cos;   /* [N+R,32] host-built rotary tables (voicebox_pytorch.py:184-191,436-443) */
  const float* rot_sin;
  int gateloop;           /* use_gateloop_layers (:898): x = GateLoop(x) + x in front of every attention block (:465-466) */
  int stack_only;         /* 1: standalone Transformer.forward (:412-479): io->x is the stack input [B,N,D], io->cond the adaptive
                             norm condition [B,Th] (unused with plain_norm), io->pred the final-norm output [B,N,D]; the backward
                             entry points take d(output) in io->target and write io->dx / io->dcond */
  int E;                  /* dim_cond_emb of a text-conditioned model (condition_on_text, :931-940), 0 = unconditional:
                             to_embed is Linear(2*D + E, D) over [x | cond_emb | cond] (:1071-1076) */
  int V1;                 /* rows of the conditioning embedding table (num_cond_tokens + 1) */
  int plain_norm;         /* 1: non-adaptive RMSNorm (adaptive_rmsnorm = False, :386-389): gammas at VBX_L_N1G / VBX_L_N2G */
  float attn_dropout;     /* attn_dropout (:895, attend.py:131) and ff_dropout (:891, :346) of the module: applied in a forward whose */
  float ff_dropout;       /* vbx_io.dropout != 0 (nn.Dropout: module.training), keyed by vbx_io.drop_seed; with attn_dropout > 0 the
                             arena holds the attention keep bits (per layer when training != 0, for the backward) */
  int Din;                /* dim_in (:884,905): width of x / cond / target / pred and of null_cond; to_embed is Linear(2*Din + E, D)
                             (:938), to_pred Linear(D, Din) (:964-966).  0 = D.  Multiple of 8. */
  int precise;            /* 1: exact-operand forward (see "precise mode" below): every forward matrix product to fp32 accuracy;
                             needs wpack3 (vbx_model_precise_wpack_bytes, filled by vbx_model_pack_weights_precise) and pscratch
                             (vbx_model_precise_scratch_bytes).  The backward entry points are unchanged (bf16 operands). */
  void* wpack3;           /* precise mode: hi/lo-split fp16 weights, K-concatenated */
  void* pscratch;         /* precise mode: fp32 intermediates + the K-concatenated activation operand */
  int unet;               /* use_unet_skip_connection (voicebox_pytorch.py:368-369,391-398,453-463; stack_only models: VoiceBox never
                             enables it): layer l >= L / 2 starts with x = Linear(2 * dim, dim)(cat(x, skip_scale * input of layer L-1-l)) */
  float skip_scale;       /* skip_connect_scale (:390), 2^-0.5 by default */
  int adaln_factors;      /* 1 (training, adaptive norms): vbx_model_backward_layer does NOT write the gradients of the adaLN projection
                             WEIGHTS (slots VBX_L_G1W .. VBX_L_B2W) -- they stay in factor form (vbx_model_adaln_factors; the
                             optimizer expands them, see vbx_adam_adaln_factors) and vbx_model_adam_segments leaves those blocks
                             out of the fused Adam's table.  Biases, d(time_emb) and every other gradient are unchanged. */
  int defer_reduce;       /* 1: the caller runs vbx_model_backward_layer for L-1 .. 0 and reads NO gradient before layer 0 has
                             returned (no per-stage gradient exchange): every layer keeps its partial records (norm gamma / beta, bias
                             column sums, qk-norm gammas) in its own arena region and layer 0 reduces them all in two launches
                             instead of one launch per layer.  0 (default): each layer's small gradients are final when it returns.
                             Same per-tensor summation order either way. */
  float* sq_partials;     /* NULL, or vbx_model_sq_partials(m, NULL) floats of device memory: the slab reduce of every layer's four
                             weight-gradient matrices (to_qkv, to_out, FeedForward in / out) also leaves the sums of squares of what it
                             stored, one float per block -- the gradient norm then needs no second pass over those tensors (their
                             flat ranges: vbx_model_sq_partials).  Meaningful only when the norm is taken over THIS backward's
                             gradient (no accumulation, no exchange in between). */
  int Lc;                 /* latent_dim of a codec-latent model whose latent width differs from D (VoiceBox(audio_enc_dec = codec),
                             voicebox_pytorch.py:911-914, 964-966, 1000-1006), 0 = none.  x / cond / target / pred are Lc wide (8 .. 1024,
                             any value); proj_in = Linear(Lc, D) at VBX_P_PINW / VBX_P_PINB is applied to x and to cond by
                             vbx_proj_in_embed, to_embed is Linear(2*D + E, D), to_pred Linear(D, Lc), null_cond is D wide.  Din must be
                             0 or D.  Operand copies are zero-padded inside the arenas (proj_in K to vbx_proj_in_kp(Lc), to_pred N to a
                             multiple of 8).  Not served by precise mode. */
  int packed;             /* 1: packed rows (see "packed rows"; inference only): B must be 1 and N = Mp, a multiple of VBX_PACK_ALIGN.  The
                             layout has no register rows of its own -- Np = N = Mp, M0 = M, rot_cos / rot_sin are [Mp, 32] in the packed
                             order, x / cond / cond_mask / pred are [1, Mp, .] -- and R and the register parameter go to
                             vbx_convpos_fwd_segs only.  vbx_model_forward runs vbx_convpos_fwd_segs and vbx_attn_fwd_segs with the
                             tables of vbx_io in place of vbx_convpos_fwd and vbx_attn_fwd*, the final norm and to_pred over all Mp
                             rows, every other launch as usual with M = Mp.  Exact where all rows share the time point (the sampler).
                             Not served: training, precise, gateloop, stack_only, an attn_mask, key_lens (VBX_EINVAL).  0 = none. */
} vbx_model;

typedef struct {
  const float* x;               /* [B,N,D]  (w in training, y in sampling) */
  const float* cond;            /* [B,N,D] */
  const uint8_t* cond_mask;     /* [B,N] 1 = frame is to be infilled (conditioning zeroed there, :1035) */
  const uint8_t* attn_mask;     /* [B,N] self_attn_mask or NULL */
  const uint8_t* attn_mask_p;   /* [B,N+R] = attn_mask left-padded with True for the registers (:428), or NULL */
  const uint8_t* loss_mask;     /* [B,N] cond_mask & attn_mask (:1099); required when target is given */
  const float* times;           /* [B] */
  const float* target;          /* [B,N,D] or NULL */
  float* pred;                  /* [B,N,D] output */
  float* loss;                  /* [1] output when target != NULL */
  const long* cond_ids;         /* E > 0: [B,T] conditioning token ids (int64) */
  int T;                        /* E > 0: tokens per sample */
  long null_id;                 /* E > 0: id substituted where drop_mask is set (null_cond_id, :933) */
  const uint8_t* drop_mask;     /* E > 0: [B] classifier-free-guidance drop mask (:1040-1053) or NULL */
  const float* null_cond;       /* E > 0: [D] null_cond parameter (:944), required with drop_mask */
  float* dx;                    /* stack_only backward: [B,N,D] gradient of the stack input */
  float* dcond;                 /* stack_only backward: [B,Th] gradient of the adaptive-norm condition (NULL with plain_norm) */
  int dropout;                  /* 1: apply the model's attn_dropout / ff_dropout in this forward (the module is in train() mode) */
  unsigned long long drop_seed; /* Philox key of this forward's masks (the backward entry points must see the same io) */
  const float* ada_table;       /* inference only, or NULL: precomputed adaLN projections [ada_stride * intervals][L][4 * D] (vbx_ada_select); */
  const int* ada_counter;       /* the forward then skips the time embedding and the projection GEMV and takes time point         */
  int ada_slot;                 /* ada_stride * ada_counter[0] + ada_slot of the table (`times` is not read)                     */
  int ada_stride;               /* time points per interval of ada_table, >= 1 (midpoint 2, euler 1, rk4 4); 0 <= ada_slot < ada_stride */
  const int* key_lens;          /* NULL, or [B] int32 on the device, key_lens[b] = R + len_b >= 1 where attn_mask_p is the prefix mask
                                   n < key_lens[b] (lens= of the sampler and of the train step).  The fast-path forward then runs
                                   vbx_attn_fwd_lens and the backward vbx_attn_bwd_fused_lens: tiles past the length are not walked.
                                   Must stay alive (and unchanged) until the backward of this forward has run.  Requires attn_mask_p,
                                   which the convolution, the loss and the fallbacks keep reading: attention dropout and precise
                                   mode ignore key_lens (mask only). */
  const int* seg_start;         /* vbx_model.packed only (NULL otherwise): the device tables of "packed rows", validated by the caller: */
  const int* seg_klen;          /* seg_start / seg_klen int32 [segments], tile_seg int32 [Mp / 128]                                    */
  const int* tile_seg;
  const int* tok_lens;          /* NULL, or [B] int32 on the device, 1 <= tok_lens[b] <= T; requires key_lens.  Row b's T_b = tok_lens[b]
                                   token ids are resized to its own N_b = key_lens[b] - R frames (vbx_pack_embed_input_text_lens,
                                   vbx_embed_text_cols_lens, vbx_cond_emb_bwd_lens) instead of T ids to N frames.  Must stay alive
                                   until the backward.  VBX_EINVAL in precise mode and on packed rows.  LAST: zero-initialised
                                   callers built against the struct without it keep their meaning. */
} vbx_io;

size_t vbx_model_wpack_bytes(const vbx_model* m);
size_t vbx_model_act_bytes(const vbx_model* m);
int vbx_model_pack_weights(const vbx_model* m, void* stream);
/* factor form of the adaLN weight gradients of the last backward (valid until the next forward of this arena): dada [L][B][4 D],
 * temb [B][Th]; w_off[l] = flat offset of layer l's weight block, dst_f16[l] = its fp16 operand copy in the wpack arena (HOST arrays
 * of L entries each, either may be NULL) */
int vbx_model_adaln_factors(const vbx_model* m, const float** dada, const float** temb, long* w_off, void** dst_f16);
/* floats vbx_model.sq_partials must hold (0: this configuration does not serve it), and -- ranges != NULL -- the 4 * L flat ranges
 * [lo, hi) of the gradient buffer they cover, in ascending order */
long vbx_model_sq_partials(const vbx_model* m, long* ranges /* host [4 * L][2] or NULL */);
/* segment table for vbx_adam_step_packed (see there) */
int vbx_model_adam_segments(const vbx_model* m, long n_flat, vbx_adam_seg* out, int max_segs, long* total_blocks);
int vbx_model_forward(const vbx_model* m, const vbx_io* io, void* stream);
/* adaLN projections of n <= 16 conditioning rows temb [n, Th] with the model's packed weights -> ada [L][n][4 * D] (what the forward
 * computes per call; the sampler tabulates it over its time grid, see vbx_ada_select) */
int vbx_model_adaln_table(const vbx_model* m, const float* temb, int n, float* ada, void* stream);
/* backward: head (loss, to_pred, final norm) -> layers L-1..0 -> embed (conv, to_embed, time MLP).  Each call
 * finishes the gradients of its own parameters, so the caller can all-reduce them while the next runs. */
int vbx_model_backward_head(const vbx_model* m, const vbx_io* io, const float* gscale, void* stream);
int vbx_model_backward_layer(const vbx_model* m, const vbx_io* io, int layer, void* stream);
int vbx_model_backward_embed(const vbx_model* m, const vbx_io* io, void* stream);
/* Weight gradients beside the dx chain.  Nothing in a layer's backward reads its four weight gradients, so a backward with
 * vbx_model.defer_reduce = 1 (no GateLoop, no u-net, grouped GEMMs) submits each layer's grouped weight-gradient launch and its slab
 * reduce to a low-priority side stream of the library (one per device, created on first use), where they fill the CUs that the
 * next layer's dgrads, norms and attention tail leave idle.  The four operands that the chain would overwrite under them live in
 * two (dxb: three) copies indexed by layer and the side stream has slab regions of its own; events order the rest
 * (csrc/wgrad_overlap_plan.hpp).  vbx_model_backward_embed -- always the last call of a backward -- ends with the caller's stream
 * waiting for the side stream, and vbx_model_backward_head begins with the same wait.  Same kernels, same reduction order:
 * gradients and sq_partials are bit-identical to the in-line order.  In line instead: every other backward, a capturing stream,
 * while vbx_prof_enable(1) is on, and with vbx_wgrad_overlap(0) (environment VBX_WGRAD_OVERLAP=0 presets it; 1 = default).
 * Not thread safe; call between backwards. */
int vbx_wgrad_overlap(int on);
/* vbx_model_backward_embed runs its finishing kernels in two multi-job launches (vbx_embed_bwd_tail1 / _tail2; models without
 * proj_in): 1 = default.  0: one launch each, as before.  The grouped form stores the bits of the separate launches; the switch exists
 * for A/B timing and for the test that compares the two. */
int vbx_embed_tail_grouped(int on);
/* how many layers this process has submitted to the side stream so far (tests: the path that ran is the path that was meant) */
int vbx_wgrad_overlap_forks(void);
/* tests only: one idle wave (vbx_stream_delay) of side_us microseconds in front of every side-stream submission and of main_us at
 * the start of every layer on the caller's stream, 0 .. 2000 each (0, 0 = off): a missing wait of the schedule then shows as a
 * wrong gradient even at small shapes. */
int vbx_wgrad_overlap_delay(float side_us, float main_us);

/* tests/debug only: device pointer of a named tensor inside the activation arena (NULL if unknown) */
void* vbx_model_debug_ptr(const vbx_model* m, const char* name, int layer);

/* ------------------------------------------------------------------ precise mode (exact-operand forward)
 * The fast path rounds every forward GEMM / attention operand to fp16; at the reference's own initialisation (qk-normed logits of
 * std ~80, a chaotic 12-layer map) that moves the loss by O(1e-3).  With vbx_model.precise = 1 vbx_model_forward evaluates
 * the same VoiceBox.forward (voicebox_pytorch.py:987-1115) with every matrix product to fp32 accuracy:
 *  - nn.Linear (:320,333,345,348,1078,1092): the same vbx_gemm tiles with both operands split into fp16 hi + lo parts and concatenated
 *    along K -- A' = [A_hi | A_hi 2^-8 | A_lo 2^8] (vbx_split3_f16), W' = [W_hi | W_lo 2^8 | W_hi 2^-8] (vbx_pack_weight3), K' = 3K,
 *    VBX_EPI_F32 (the powers of two keep the lo parts of small weights out of the fp16 subnormals);
 *  - MultiheadRMSNorm + rotary (:286-287,193-199, 323-328) and GEGLU (:338-340) as fp32 kernels on the fp32 GEMM results
 *    (vbx_qknorm_rope_f32, vbx_geglu_f32), which also write the fp16 / bf16 copies the backward entry points read;
 *  - Attend (attend.py:121-135) as an fp32 FMA flash kernel (vbx_attn_fwd_f32), q / k / v / P never rounded;
 *  - AdaptiveRMSNorm's to_gamma / to_beta (:273) from the fp32 master weights (vbx_adaln_proj_f32);
 *  - text conditioning (:1056-1078): the fp32 rows of vbx_embed_input_text_f32 through the same split GEMM (K = 2 * Din + E);
 *  - GateLoop (:465-466): its to_qkva projection through the split GEMM, scan and LayerNorm are fp32 on both paths;
 *  - dropout (attend.py:131, :346): the fast path's Philox masks (vbx_attn_dropout_bits, vbx_dropout_rows[_f32]) on the unrounded
 *    probabilities / GEGLU output, so a precise step and a fast step with the same seed drop the same elements.
 * Serves VoiceBox (not the standalone Transformer stack, u-net skips or plain RMSNorm); those return VBX_EINVAL. */
/* dst fp16 [rows, 3*Kp] = [hi | hi 2^-8 | lo 2^8] of src fp32 [rows, K] (row stride ld floats), columns K..Kp zero; Kp % 8 == 0 */
int vbx_split3_f16(const float* src, long rows, int K, long ld, void* dst_f16, int Kp, void* stream);
/* dst fp16 [dst_rows, 3*dst_cols] = [hi | lo 2^8 | hi 2^-8] of the weight, rows mapped / padded as vbx_pack_weight does */
int vbx_pack_weight3(const float* src, int src_rows, int src_cols, void* dst_f16, int dst_rows, int dst_cols, int rowmap, int F,
                     void* stream);
/* raw fp32 [B*Np, 3*H*64] (to_qkv output) -> q, k (qk-normed when qk_scale > 0, rotated) and v, head-major [B,H,Np,64]: fp32 plus the
 * optional fp16 / bf16 copies and 1/max(|.|,1e-12) rows the backward reads (any of q16 .. k_rnorm may be NULL) */
int vbx_qknorm_rope_f32(const float* raw, int B, int H, int Np, float qk_scale, const float* q_gamma, const float* k_gamma,
                        const float* rot_cos, const float* rot_sin, float* q32, float* k32, float* v32, void* q16, void* k16,
                        void* qb, void* kb, void* v_bf16, void* v16, float* q_rnorm, float* k_rnorm,
                        float q16_scale /* q16 = q * q16_scale: vbx_attn_q_prescale(scale), the attention kernels' contract */,
                        void* stream);
/* attend.py:121-135 in fp32: q, k, v fp32 [B,H,Np,64] -> out32 fp32 [B,Np,H*64] (+ optional fp16 / bf16 copies, log2-LSE [B,H,Np]) */
int vbx_attn_fwd_f32(const float* q, const float* k, const float* v, const uint8_t* mask, float* out32, void* out16, void* out_bf16,
                     float* lse, int B, int H, int Np, float scale, void* stream);
/* ... with attention dropout: bits_rm / p as in vbx_attn_fwd_dropout (the statistics stay those of the undropped probabilities) */
int vbx_attn_fwd_f32_dropout(const float* q, const float* k, const float* v, const uint8_t* mask, float* out32, void* out16,
                             void* out_bf16, float* lse, int B, int H, int Np, float scale, const void* bits_rm, float p, void* stream);
/* GEGLU (libm erff) on the fp32 pre-activation h1 [M, 2*Fp] in the packed column order (128-column blocks: 64 "x", their 64 "gate"):
 * g32 [M, Fp] (+ optional fp16 / bf16 copies of g and the bf16 pre-activation the backward reads) */
int vbx_geglu_f32(const float* h1, float* g32, void* g16, void* g_bf16, void* h1_bf16, long M, int Fp, void* stream);
/* vbx_adaln_proj_fwd with fp32 weights W [J, Th] */
int vbx_adaln_proj_f32(const float* temb, const float* w, const float* bias, float* ada, int B, int Th, int J, int group, void* stream);
size_t vbx_model_precise_wpack_bytes(const vbx_model* m);
size_t vbx_model_precise_scratch_bytes(const vbx_model* m);
int vbx_model_pack_weights_precise(const vbx_model* m, void* stream);

/* ------------------------------------------------------------------ HuBERT + k-means (csrc/hubert.hip, voicebox-pytorch_amd/hubert.py)
 * HuBERT base (feat_extract_norm "group", post-LN encoder, no convolution bias) up to one encoder layer, then the nearest row of a
 * k-means codebook: what audiolm_pytorch's HubertWithKmeans computes, inference only.  The encoder layers run on vbx_gemm
 * (NT, f16 = 1, VBX_EPI_F32 / VBX_EPI_GELU) and vbx_attn_fwd (mask NULL) as they are; the entry points below are what sits between.
 * WHERE A TENSOR IS ROUNDED (tests/hubert_ref.py, emulate=True, rounds exactly here and nowhere else):
 *  - the wave, the first convolution's weights and its fmaf chain are fp32; GroupNorm's statistics are taken over those unrounded
 *    values; (v - mean) * rstd * gamma + beta and erf-GELU are fp32; the result is rounded ONCE to fp16 [B, L0, C];
 *  - every later convolution: fp16 input as stored, weights rounded to fp16, fp32 sum, erf-GELU in fp32, rounded once to fp16;
 *  - feature_projection.layer_norm reads the fp16 rows, works in fp32 and rounds its result to fp16 (the projection's operand); the
 *    projection's weight is rounded to fp16, its sum and bias are fp32 and the result x stays fp32;
 *  - the positional convolution rounds x to fp16 as it stages it and its weight (weight norm folded in fp32) to fp16; sum, bias,
 *    erf-GELU and the + x (the UNROUNDED fp32 x) are fp32 and the result stays fp32;
 *  - every encoder LayerNorm reads fp32 and writes fp32 (the residual stream, never rounded) plus an fp16 copy (the operand of the
 *    next product);
 *  - per layer: the q | k | v, out_proj, intermediate_dense and output_dense weights are rounded to fp16; q | k | v sum + bias is
 *    fp32, then q * vbx_attn_q_prescale(dim_head ** -0.5), k and v are each rounded once to fp16; the attention output is fp16
 *    (vbx_attn_fwd's own contract: its probabilities are fp16 operands of P.V inside the kernel, which the emulation does not
 *    mirror); out_proj / output_dense: fp32 sum + bias + fp32 residual, not rounded; gelu(intermediate_dense) is rounded to fp16
 *    (VBX_EPI_GELU: erf by Abramowitz-Stegun 7.1.26, |error| <= 6e-7);
 *  - vbx_kmeans_assign is fp32 throughout.
 * Every entry point is a plain launch (or two), without atomics: reruns give the same bits, and a batch row's result is bit-equal to
 * that row computed alone. */
/* The first convolution (1 -> C, kernel k0 <= 16, stride s0 <= 16, no padding, no bias: L0 = (T - k0) / s0 + 1 positions) and the
 * statistics of GroupNorm(C, C): per (row, channel) the mean and biased variance over TIME of the fp32 value
 * v[t][c] = fmaf chain over tap = 0 .. k0 - 1 of w[c][tap] * wave[t * s0 + tap], started at 0.  One record (K, S1, S2) per (row, chunk
 * of 256 positions, channel): K the chunk's first value, S1 = sum(v - K), S2 = sum((v - K)^2) in fp32 -- shifted, so a large mean
 * costs nothing; a second launch combines the records of a (row, channel) in ascending order in fp64 (Chan et al.'s pairwise update)
 * into stats[b][c] = (mean, 1 / sqrt(var + eps)).  wave fp32 [B, T]; w fp32 [C, k0]; records fp32 [B, vbx_hubert_conv0_chunks(L0), C, 3]
 * (scratch); stats fp32 [B, C, 2].  C a multiple of 8 up to 512. */
int vbx_hubert_conv0_chunks(int L0);
int vbx_hubert_conv0_stats(const float* wave, const float* w, float* records, float* stats, int B, long T, int C, int k0, int s0,
                           float eps, void* stream);
/* ... and the pass that writes y fp16 [B, L0, C] = gelu((v - mean) * rstd * gamma + beta): v is computed again by the same chain (the
 * same bits as in the statistics pass); the fp32 pre-norm tensor is never stored. */
int vbx_hubert_conv0_apply(const float* wave, const float* w, const float* stats, const float* gamma, const float* beta, void* y_f16,
                           int B, long T, int C, int k0, int s0, void* stream);
/* Conv1d(C, C, k, stride 2, no padding, no bias) + erf-GELU on the implicit-GEMM tile core (csrc/seanet_tile.hpp): x fp16 [B, L, C],
 * w fp16 [C, k * C] (row = output channel, column tap * C + c), y fp16 [B, (L - k) / 2 + 1, C].  k 2 or 3, C a multiple of 16 up to
 * 512, L >= k.  vbx_hubert_conv_tile: the output positions a workgroup owns before a short row shrinks it (tests stand on both sides). */
int vbx_hubert_conv_tile(int C, int k);
int vbx_hubert_conv(const void* x_f16, const void* w_f16, void* y_f16, int B, int L, int C, int k, void* stream);
/* LayerNorm over the last axis, one wave per row, two passes (mean, then squared deviations), fp32: x fp32 [M, D] -> y_f32 and / or
 * y_f16 (either may be NULL; the fp16 copy saturates at +-65504).  vbx_hubert_layernorm16 reads fp16 rows and writes fp16. */
int vbx_hubert_layernorm(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_f16, long M, int D, float eps,
                         void* stream);
int vbx_hubert_layernorm16(const void* x_f16, const float* gamma, const float* beta, void* y_f16, long M, int D, float eps, void* stream);
/* HubertPositionalConvEmbedding + the residual: y = gelu(conv(x)[:N] + bias) + x with conv = Conv1d(D, D, k, padding k / 2, groups),
 * k even, so that of the N + 1 positions the convolution has the last is dropped -- it is never computed.  One product per (tile of
 * positions, group) with K = k * D / groups; the zero padding is resolved while the span is staged from x fp32 [B, N, D] (rounded to
 * fp16 there).  w fp16 [D, k * D / groups]: row = output channel, column tap * (D / groups) + input channel within the group, weight
 * norm folded by the caller.  bias fp32 [D]; y fp32 [B, N, D], not x.  D / groups a multiple of 8; vbx_hubert_posconv_tile:
 * positions per workgroup, or VBX_EINVAL where 16 positions do not fit the LDS. */
int vbx_hubert_posconv_tile(int channels_per_group, int k);
int vbx_hubert_posconv(const float* x, const void* w_f16, const float* bias, float* y, int B, int N, int D, int groups, int k, void* stream);
/* qkv fp32 [B * N, 3 * H * 64] (columns [q | k | v], bias already added) -> q16 = fp16(q * q_prescale), k16, v16 fp16 [B, H, N, 64]:
 * vbx_attn_fwd's operands (q_prescale = vbx_attn_q_prescale(scale), its contract).  Each element rounded once, saturating. */
int vbx_hubert_split_heads(const float* qkv, void* q16, void* k16, void* v16, int B, int N, int H, float q_prescale, void* stream);
/* ids[r] = argmin_k |h[r] - centers[k]|^2, fp32 throughout: d = sum_i (h_i - c_i)^2 as differences (no |h|^2 - 2 h.c + |c|^2
 * cancellation), summed in a fixed order per (row, code).  CONTRACT: d(ids[r]) - min_k d(k), both evaluated exactly, is at most
 * (D + 2) * 2^-23 * (|h[r]| + max_k |c_k|)^2, and among codes whose computed distances are equal the lowest index wins (duplicate
 * rows of the codebook: the first).  h fp32 [M, D], centers fp32 [K, D], ids int64 [M].  D a multiple of 8 up to 2048, K 1 .. 4096. */
int vbx_kmeans_assign(const float* h, const float* centers, long long* ids, long M, int D, int K, void* stream);
/* THE LARGE FORM (HubertLargeWithKmeans: feat_extract_norm "layer", do_stable_layer_norm, an optional convolution bias -- what
 * transformers.HubertModel computes for hubert-large-ll60k).  The projection, the positional convolution, the five products, the head
 * split, the attention and the k-means are the entry points above with their contracts; the sequence is in csrc/hubert.hip's header.
 * WHERE A TENSOR IS ROUNDED (tests/hubert_large_ref.py, emulate=True, rounds exactly here and nowhere else):
 *  - vbx_wave_normalize: fp32 in, statistics and (x - mean) * rstd in fp64, rounded once to fp32;
 *  - the first convolution: fp32 wave, fp32 weights, the fmaf chain of vbx_hubert_conv0_apply, + bias, LayerNorm over the C channels of
 *    the position in fp32 on those unrounded values, erf-GELU in fp32, rounded ONCE to fp16 [B, L0, C];
 *  - every later convolution: fp16 input as stored, weights rounded to fp16, fp32 sum, + fp32 bias; LayerNorm over the C channels
 *    from those fp32 sums (NOTHING is rounded before the norm and no intermediate goes to memory), affine, erf-GELU, rounded once to fp16;
 *  - feature_projection.layer_norm, the projection and the positional convolution: as in the base form; there is no LayerNorm after
 *    the positional convolution -- its fp32 result is the residual stream x;
 *  - per layer: layer_norm(x) and final_layer_norm(x) read the fp32 stream and write ONLY the fp16 operand of the next product
 *    (vbx_hubert_layernorm with y_f32 NULL: the norm in fp32, rounded once); out_proj / output_dense add the UNNORMALISED fp32 x;
 *    everything else per layer as in the base form;
 *  - encoder.layer_norm reads and writes fp32 and runs only where hidden_states[num_hidden_layers] is asked for.
 * Plain launches without atomics: the same bits on every run, a batch row's result bit-equal to that row alone.  No statistic runs
 * over time, so ragged waves (lens) need no kernel of their own before the positional convolution: a frame inside a row's count reads
 * only that row's own samples, and the frames past it are zeroed by vbx_hubert_posconv_lens and at the end. */
/* y fp16 [B, L0, C] = gelu(LayerNorm_C(v + bias) * gamma + beta), v the fmaf chain of vbx_hubert_conv0_stats, L0 = (T - k0) / s0 + 1.
 * One launch; LayerNorm two-pass in fp32 (the mean, then the squared deviations) over the C values of a position, one wave per position,
 * lane l sums its channels 8 l .. 8 l + 7 in ascending order, then the xor tree.  bias fp32 [C] or NULL; gamma, beta fp32 [C].
 * k0, s0 <= 16; C a multiple of 16 up to 512.  vbx_hubert_conv0_ln_tile: the positions a workgroup owns. */
int vbx_hubert_conv0_ln_tile(void);
int vbx_hubert_conv0_ln(const float* wave, const float* w, const float* bias, const float* gamma, const float* beta, void* y_f16, int B,
                        long T, int C, int k0, int s0, float eps, void* stream);
/* vbx_hubert_conv with the large form's epilogue: y fp16 [B, (L - k) / 2 + 1, C] = gelu(LayerNorm_C(conv(x) + bias) * gamma + beta).
 * The workgroup that owns TT positions owns all their C channels: its fp32 sums wait in an fp32 tile [TT][C + 4] in the LDS beside the
 * staged span, and each position is normalised from them (two-pass, fp32, as above).  The tile is the largest whose span PLUS sums fit
 * as csrc/seanet_tile.hpp picks (at C = 512: 16 positions, 66 KiB, against vbx_hubert_conv's 32).  bias fp32 [C] or NULL.
 * vbx_hubert_conv_ln_tile: the positions a workgroup owns before a short row shrinks it. */
int vbx_hubert_conv_ln_tile(int C, int k);
int vbx_hubert_conv_ln(const void* x_f16, const void* w_f16, const float* bias, const float* gamma, const float* beta, void* y_f16, int B,
                       int L, int C, int k, float eps, void* stream);
/* The same layer as an fp32 intermediate plus a row kernel, for the shapes where that is faster (vbx_hubert_conv_ln_route: 1 where
 * the fused kernel's tile is smaller than vbx_hubert_conv's AND its grid is more than 512 workgroups, so that twice the workgroups
 * re-reading the weight from L2 bound it; 0: the fused kernel).  vbx_hubert_conv_f32: vbx_hubert_conv's tile, the fp32 sum + bias
 * stored UNROUNDED to s fp32 [B, (L - k) / 2 + 1, C].  vbx_hubert_ln_gelu: y fp16 [M, C] = gelu(LayerNorm_C(s) * gamma + beta), one wave
 * per row, the code of the fused epilogue on the same values.  The sum of an output does not depend on the tile's height, so the pair
 * and vbx_hubert_conv_ln give the SAME BITS: the route is a matter of speed only, and a row alone may take another route than its
 * batch.  Nothing is rounded before the norm either way.  C a multiple of 8 (16 for the convolution) up to 512. */
int vbx_hubert_conv_ln_route(int B, int L, int C, int k);
int vbx_hubert_conv_f32(const void* x_f16, const void* w_f16, const float* bias, float* s_f32, int B, int L, int C, int k, void* stream);
int vbx_hubert_ln_gelu(const float* s_f32, const float* gamma, const float* beta, void* y_f16, long M, int C, float eps, void* stream);
/* y[b][t] = (x[b][t] - mean_b) / sqrt(var_b + eps), biased variance, over the row's T samples -- with lens int32 [B] (or NULL) over
 * its first len_b = clamp(lens[b], 1, T) samples, and y[b][t] = 0 for t >= len_b (x is not read there).  One record (K, S1, S2) per
 * (row, chunk of vbx_wave_normalize_chunk() = 4096 samples): K the chunk's first sample, S1 = sum(x - K), S2 = sum((x - K)^2) in fp32
 * in a fixed order -- shifted, so a DC offset costs nothing; a second launch combines a row's records in ascending order in fp64 into
 * stats[b] = (mean, 1 / sqrt(var + eps)), kept in fp64; a third computes (x - mean) * rstd in fp64 and rounds once.  A single sample
 * gives 0.  x, y fp32 [B, T] (y may be x); records fp32 [B, ceil(T / chunk), 3] and stats fp64 [B, 2] are scratch.  No atomics, the
 * same bits on every run, a row's result independent of its neighbours. */
int vbx_wave_normalize_chunk(void);
int vbx_wave_normalize(const float* x, const int* lens, float* y, float* records, double* stats, int B, long T, float eps, void* stream);

/* ------------------------------------------------------------------ k-means fit (csrc/kmeans.hip, voicebox-pytorch_amd/kmeans.py)
 * One step of MiniBatchKMeans.partial_fit at reassignment_ratio = 0 (or of Lloyd's algorithm) is
 *   vbx_kmeans_norms -> vbx_kmeans_search -> vbx_kmeans_accumulate -> vbx_kmeans_update
 * on one stream: assign with the OLD centres, sum the members of every cluster, move the centres.  fp32 data throughout, no float
 * atomics, no host synchronisation; every entry point gives the same bits on every run.  x fp32 [M, D] (M = B * N rows), centres fp32
 * [K, D]; D a multiple of 8 up to 2048, K 1 .. 4096, 1 <= M < 2^31.  lens int32 [B] or NULL: row m = b * N + n LIVES iff n < lens[b]
 * (NULL: every row); a dead row is never read, whatever it holds. */
/* norms[k] = |c_k|^2, fp32: lane l of a wave sums components 4 l + 256 j in ascending j by fmaf, then the xor tree over the 64 lanes */
int vbx_kmeans_norms(const float* centers, float* norms, int K, int D, void* stream);
/* ids[m] = argmin_k (norms[k] - 2 x_m . c_k) for a live row, the dot product an fp32 fmaf chain on v_mfma_f32_32x32x2_f32 in an
 * order that is the same for every (row, centre) pair (csrc/kmeans.hip); K for a dead row.  CONTRACT, vbx_kmeans_assign's and
 * vbx_rvq_encode's: d(ids[m]) - min_k d(k), both evaluated exactly, is at most (D + 2) * 2^-23 * (|x_m| + max_k |c_k|)^2, and among
 * centres whose computed values are equal the lowest index wins.  mind[m] = sum_i (x_mi - c_i)^2 for the centre taken, by differences
 * (component 4 l + 256 j in lane l, ascending j, then the xor tree over the 64 lanes); 0.0 for a dead row.  ids int32 [M], mind fp32
 * [M].  vbx_kmeans_search_tile: the rows a workgroup owns (32; 16 above D = 1024); vbx_kmeans_search_chunk: the components of one
 * stage of the codebook stream (32 or 16) -- tests stand on both sides of either. */
int vbx_kmeans_search_tile(int D);
int vbx_kmeans_search_chunk(int D);
int vbx_kmeans_search(const float* x, const float* centers, const float* norms, const int* lens, int* ids, float* mind, long M, int N,
                      int D, int K, void* stream);
/* sums[k] = sum of the rows with ids[m] == k, counts[k] = their number (ids outside 0 .. K - 1 belong to no cluster: dead rows),
 * inertia = the sum of mind over those rows.  SUMMATION ORDER: cluster k's members in ascending row index, r = 0 .. n_k - 1;
 * P_j = ((x_{64 j} + x_{64 j + 1}) + ...) + x_{64 j + 63} and S_k = ((P_0 + P_1) + P_2) + ..., both left to right, per component -- a function of
 * the members' ranks alone: the same bits for any batch shape that lists the same live rows in the same order, and on every run.
 * mind takes the same route in fp64 (Q_j); the inertia adds all Q_j, clusters ascending, as lane l: Q_l + Q_{l + 64} + ... then the xor
 * tree over 64 lanes, and is stored in fp64 and rounded once to fp32.  sums fp32 [K, D] (zeros for an empty cluster), counts int32
 * [K]; scratch: vbx_kmeans_accumulate_scratch_bytes(M, D, K) bytes, 256-byte aligned (-1: a shape outside the limits). */
long vbx_kmeans_accumulate_scratch_bytes(long M, int D, int K);
int vbx_kmeans_accumulate(const float* x, const int* ids, const float* mind, float* sums, int* counts, double* inertia64,
                          float* inertia32, void* scratch, long M, int D, int K, void* stream);
/* One launch.  lloyd == 0: c' = (c * (float)w + S) / (float)(w + n) where n = counts[k] > 0, w' = w + n; lloyd != 0: c' = S / (float)n
 * where n > 0, w' = n.  A centre with n == 0 keeps its bits.  fp32 multiply, add and correctly rounded divide.  The outputs are
 * buffers of their own (w int64 [K]): nothing written here is read by a launch of the same step. */
int vbx_kmeans_update(const float* centers, const long long* w, const float* sums, const int* counts, float* centers_out,
                      long long* w_out, int K, int D, int lloyd, void* stream);
/* k-means++ (Arthur & Vassilvitskii 2007), plain D^2 sampling, one candidate per step, from given uniforms u fp32 [K] in [0, 1):
 * 2 K - 1 launches, the chosen index of a step read by the next launch from device memory.  Step 0 takes live row number
 * floor(u_0 * M_live) (the product in fp64).  Step j: p_i = min over the chosen rows c of sum_d (x_id - x_cd)^2 by differences (mind's
 * order), exactly 0 for a chosen row and for a dead one; the pick is the first row with p_i > 0 whose running sum reaches
 * (double)u_j * total.  RUNNING SUM, fp64: block b = rows [64 b, 64 b + 64) has B_b = the xor-tree sum of its p; range t of 1024 =
 * ceil(blocks / 1024) consecutive blocks added left to right; the ranges by a Hillis-Steele scan; inside a block an inclusive
 * Hillis-Steele scan over its rows.  total == 0 (every live row coincides with a chosen one): live row floor(u_j * M_live).
 * chosen int64 [K], centers fp32 [K, D] = the chosen rows; scratch p fp32 [M], bsum fp64 [vbx_kmeans_plusplus_blocks(M)].  Fewer
 * live rows than K: rows repeat; no live row: row 0 is read (the caller refuses both where it can see lens). */
long vbx_kmeans_plusplus_blocks(long M);
int vbx_kmeans_plusplus(const float* x, const int* lens, const float* u, float* p, double* bsum, long long* chosen, float* centers,
                        long M, int N, int D, int K, void* stream);

/* ------------------------------------------------------------------ in-situ stage timing (measurement only)
 * While enabled, vbx_model_forward / vbx_model_backward_* bracket each MFMA stage of a layer (to_qkv, attention forward, to_out,
 * ff_in, ff_out, the four dgrads, attention backward, the weight-gradient launch) with a pair of HIP events recorded on the
 * caller's stream, i.e. the launches are timed where they run -- between their real neighbours -- not back to back in
 * isolation.  vbx_prof_collect synchronises on the recorded events, aggregates by label and disables the recording.
 * Not hipGraph-capture safe: do not enable around a capture.  bench.py's roofline.kernels come from here.
 * While enabled the weight gradients run in line on the caller's stream (see vbx_wgrad_overlap): the events bracket launches of
 * that stream, and the table stays the serial per-stage account -- its "wgrad (4 GEMMs)" row is the launch on its own, and the sum
 * of the rows exceeds the step that runs with the overlap on. */
typedef struct {
  char label[24];
  int calls;
  float total_us;
} vbx_prof_entry;
int vbx_prof_enable(int on);
int vbx_prof_collect(vbx_prof_entry* out, int max_entries); /* returns the number of labels (<= max_entries) */

/* ------------------------------------------------------------------ hardware probes (tests only) */
int vbx_probe_tr16(const void* in_u16_4096, const int* lane_elem_off, void* out_u16_256, void* stream);
int vbx_probe_mfma(int which, const float* a, const float* b, float* c, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VBX_H */
