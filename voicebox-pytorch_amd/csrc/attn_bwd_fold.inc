// Round 5: the two-body attention backward with the softmax statistics FOLDED INTO THE MATRIX PIPE (included inside attn.hip's
// anonymous namespace, after the LDS-DMA bodies whose ring, swizzle and epilogues it shares).
//
// The round-3/4 census of a 32 x 32 block of the dk/dv body: 16 MFMAs and 64 VALU, of which 16 v_fma (s * scale2 - L),
// 16 v_sub (dP - delta) -- a third of the block's vector instructions -- exist only to subtract a per-row constant from an MFMA
// result.  The MFMA adds a C operand for free, so the constant goes there:
//   * q16 arrives PRE-SCALED by scale * log2(e) (contract of every vbx_attn_* entry point since round 5, include/vbx.h), so
//     Q . K^T is already in the exp2 domain;
//   * the stationary fragments are NEGATED once per workgroup (K and V in the dk/dv body, Q and dO in the dq body), and the C
//     operand of the first MFMA of each chain holds L (log2-sum-exp of the row) resp. delta:
//         s'  = L     - Q . K^T      ->  P = exp2(-s')              (v_exp_f32 with the free source negation)
//         dp' = delta - dO . V^T     -> -dS = P * dp'
//     The sign of dS is carried to the end: dK = -(scale) * (-dS)^T . Q, dQ = -(scale) * (-dS) . K.
//   * dk/dv body: L and delta of the block's 32 rows are the 16-register tuples the body already read from the LDS ring
//     (4 x ds_read_b128 each) -- they ARE the C operands, no move; dq body: the lane's L lives in ONE persistent 16-register
//     tuple (the chains' operand reads are serialised to make room); its delta stays a VALU add (a second tuple spills).
// Per block: dk/dv 80 -> 48 VALU (exp, mul, 2 x cvt_pk per element pair), dq 72 -> 56.  Rows past Np keep L = 1e30 from the
// constant page: s' = 1e30, P = exp2(-1e30) = 0.  Dropout stays on the unfolded bodies (its keep / 1/keep factor sits between dP
// and delta).
//
// The 16 exponentials of a block depend only on the S chain, so they are issued BETWEEN the four dependent MFMAs of the dP chain
// (sched_group_barrier: 1 MFMA, 4 TRANS), where the wave would otherwise wait for the matrix pipe.

// (The timing ablations of the dk/dv body -- no exponentials, one MFMA per chain, no fragment / statistics reads, no DMA, no barrier --
//  were compile-time arms of this file; they were removed, their figures are in profiles/r06_attn_bwd_ablation.txt and docs/history.md.)
VBX_DEV f32x16 cat16(const f32x4& a, const f32x4& b, const f32x4& c, const f32x4& d) {
  typedef __attribute__((ext_vector_type(8))) float f32x8;
  const f32x8 lo = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  const f32x8 hi = __builtin_shufflevector(c, d, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}
VBX_DEV f16x8 neg_f16x8(f16x8 v) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  u32x4 w = __builtin_bit_cast(u32x4, v);
  w ^= 0x80008000u;
  return __builtin_bit_cast(f16x8, w);
}
VBX_DEV bf16x8 neg_bf16x8(bf16x8 v) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  u32x4 w = __builtin_bit_cast(u32x4, v);
  w ^= 0x80008000u;
  return __builtin_bit_cast(bf16x8, w);
}
VBX_DEV float exp2_neg(float x) { return __builtin_amdgcn_exp2f(-x); }  // v_exp_f32 v, -v

// 1 MFMA, then 4 transcendental VALU: the scheduling pattern of a dP chain with the block's exponentials in its gaps
#define FOLD_SGB_MFMA_EXP()                               \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      \
  __builtin_amdgcn_sched_group_barrier(0x400, 4, 0)

// Length-aware instantiations (LENS; vbx_attn_bwd_lens / vbx_attn_bwd_fused_lens, include/vbx.h): keys at or past kend = key_lens[b] are
// dead whatever `mask` says, and query rows at or past it carry dO = 0 (the caller's precondition).  Both bodies then walk
// ceil(kend / 64) ring tiles instead of ceil(Np / 64) -- a skipped tile would have had P = 0 (dead keys) or dO = delta = 0 (dead
// queries), i.e. +-0 added to every sum -- and a 128-row tile wholly at or past kend writes zeros and leaves before any DMA.  With
// LENS = false `kend` IS Np and the bodies compile to the instructions they had (profiles/train_lens_attn.txt).
//
// The zero rows of a wholly dead tile: fp32 rows of x32 [B,H,Np,64] (unfused dq / dk), bf16 rows of the fused epilogue's dqkv block
// with its zero gamma-partial record, and (dk/dv role) the bf16 dv rows.
VBX_DEV void attn_bwd_zero_tile(float* __restrict__ x32, const QKBwd& f, u16* __restrict__ dv, int dv_ld, int b, int h, int H, int tile,
                                int Np) {
  const int tid = threadIdx.x;
  const long bh = (long)b * H + h;
  const int row0 = tile * 128;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  if (f.dqkv) {
    for (int i = tid; i < 128 * 8; i += 256) {
      const int n = row0 + (i >> 3);
      if (n < Np) *reinterpret_cast<uint4*>(f.dqkv + ((long)b * Np + n) * f.ld + f.col0 + h * 64 + (i & 7) * 8) = z;
    }
    if (f.qk_scale > 0.f && f.gpart && tid < 64) f.gpart[(((long)b * ((Np + 127) >> 7) + tile) * H + h) * 64 + tid] = 0.f;
  } else {
    for (int i = tid; i < 128 * 16; i += 256) {
      const int n = row0 + (i >> 4);
      if (n < Np) *reinterpret_cast<uint4*>(x32 + (bh * Np + n) * 64 + (i & 15) * 4) = z;
    }
  }
  if (dv) {
    for (int i = tid; i < 128 * 8; i += 256) {
      const int n = row0 + (i >> 3);
      if (n < Np) *reinterpret_cast<uint4*>(dv + ((long)b * Np + n) * dv_ld + h * 64 + (i & 7) * 8) = z;
    }
  }
}

template <bool LENS>
VBX_DEV void attn_bwd_dkdv_fold_body(char* smem, int wg_id, const u16* __restrict__ q16, const u16* __restrict__ qb16,
                                     const u16* __restrict__ k16, const u16* __restrict__ vv, const uint8_t* __restrict__ mask,
                                     const u16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
                                     float* __restrict__ dk, u16* __restrict__ dv, int dv_ld, int H, int Np, float scale, int BH,
                                     int xmap, const QKBwd& fk, const int* __restrict__ key_lens) {
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnCoord co = attn_coord_id(wg_id, H, Np, BH, xmap);
  if (!co.ok) return;
  ATTN_TRACE_BEGIN();
  const int h = co.h, b = co.b;
  const long bh = (long)b * H + h;
  int kend = Np;  // uniform over the workgroup
  if constexpr (LENS) {
    kend = min(max(key_lens[b], 1), Np);
    if (co.tile * 128 >= kend) {  // dead keys only: zero dk / dv rows (and gamma partials), no DMA
      attn_bwd_zero_tile(dk, fk, dv, dv_ld, b, h, H, co.tile, Np);
      ATTN_TRACE_END(2);
      return;
    }
  }
  const u16* qbase = q16 + bh * Np * 64;
  const u16* qbbase = qb16 + bh * Np * 64;
  const u16* dobase = dout + (long)b * Np * (H * 64) + h * 64;
  const int key0 = co.tile * 128 + wave * 32;
  const bool active = key0 < Np;
  const int key = key0 + (lane & 31);
  const int keyc = min(key, Np - 1);
  bool kvalid = key < kend;
  if (kvalid && mask) kvalid = mask[(long)b * Np + key] != 0;
  const int ntiles = (kend + 63) / 64;  // query tiles: rows at or past kend carry dO = 0

  f16x8 kf[4];   // -K
  bf16x8 vf[4];  // -V
#pragma unroll
  for (int t = 0; t < 4; t++) {
    kf[t] = neg_f16x8(*reinterpret_cast<const f16x8*>(k16 + (bh * Np + keyc) * 64 + 16 * t + 8 * hi));
    vf[t] = neg_bf16x8(*reinterpret_cast<const bf16x8*>(vv + (bh * Np + keyc) * 64 + 16 * t + 8 * hi));
  }
#pragma unroll
  for (int t = 0; t < 4; t++) {  // retire the per-lane fragment loads before any LDS-DMA is in flight
    asm volatile("" ::"v"(kf[t]));
    asm volatile("" ::"v"(vf[t]));
  }
  asm volatile("" ::"v"(kvalid));

  // Q16 | Qb | dO tiles + the L / delta rows of the 64 queries of step qt.  Round 6: scalar base pointers + two per-lane 32-bit byte
  // offsets computed once (head-major q rows are 128 B apart, token-major dO rows H * 128 B): six LDS-DMA pieces per step with no
  // vector ALU work (the 64-bit per-lane addresses of the round-5 loop cost ~50 instructions per step).
  unsigned oqv[2], odv[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int sidx = i * 256 + tid, row = sidx >> 3, c = (sidx & 7) ^ attn_swz(row);
    oqv[i] = (unsigned)(row * 128 + c * 16);
    odv[i] = (unsigned)(row * (H * 128) + c * 16);
  }
  const unsigned m0b = __builtin_amdgcn_readfirstlane(lds_addr32(smem) + (unsigned)(tid & ~63) * 16u);
  auto issue = [&](int qt) {
    const unsigned so = (unsigned)((qt & 1) * D3_SLOT);
    unsigned q0o = oqv[0], q1o = oqv[1], d0o = odv[0], d1o = odv[1];
    if ((qt + 1) * 64 > Np) {  // last, partial tile: rows past the end re-read the last row
      const unsigned lim = (unsigned)(Np - 1 - qt * 64);
      const unsigned r0 = oqv[0] >> 7, r1 = oqv[1] >> 7;
      const unsigned c0 = r0 - min(r0, lim), c1 = r1 - min(r1, lim);
      q0o -= c0 << 7; q1o -= c1 << 7;
      d0o -= c0 * (unsigned)(H * 128); d1o -= c1 * (unsigned)(H * 128);
    }
    const u16* qs = qbase + (long)qt * 4096;
    const u16* qbs = qbbase + (long)qt * 4096;
    const u16* ds = dobase + (long)qt * 64 * (H * 64);
    glds16_sbase(q0o, qs, m0b + so);
    glds16_sbase(q1o, qs, m0b + so + 4096u);
    glds16_sbase(q0o, qbs, m0b + so + (unsigned)TILE16);
    glds16_sbase(q1o, qbs, m0b + so + (unsigned)TILE16 + 4096u);
    glds16_sbase(d0o, ds, m0b + so + 2u * TILE16);
    glds16_sbase(d1o, ds, m0b + so + 2u * TILE16 + 4096u);
    if (wave < 2) {
      char* slot = smem + (qt & 1) * D3_SLOT;
      const int n = qt * 64 + lane;
      const float* src = (wave == 0 ? lse : delta) + bh * Np + min(n, Np - 1);
      if (wave == 0 && n >= Np) src = attn_big_page;
      char* sdst = slot + 3 * TILE16 + wave * 256;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)sdst, 4, 0, 0);
    }
  };

#define VBX_BWD_RAGGED_DKDV
#include "attn_bwd_ragged.inc"
#undef VBX_BWD_RAGGED_DKDV

  unsigned ra[4], ta[2], ta8[2], sa;
  {
    const int row = lane & 31;
    const int G = lane >> 4, a16 = lane & 15;
    const int trow = 4 * (G >> 1) + (a16 >> 2);
#pragma unroll
    for (int t = 0; t < 4; t++) ra[t] = lds_addr32(smem + swz_off2(row, 2 * t + hi));
#pragma unroll
    for (int db = 0; db < 2; db++) {
      const int d = db * 32 + (G & 1) * 16 + 4 * (a16 & 3);
      ta[db] = lds_addr32(smem + swz_off2(trow, d >> 3) + (d & 7) * 2);
      ta8[db] = lds_addr32(smem + swz_off2(trow + 8, d >> 3) + (d & 7) * 2);
    }
    sa = lds_addr32(smem + 3 * TILE16 + 4 * hi * 4);
  }

  f32x16 adk[2], adv[2];
#pragma unroll
  for (int i = 0; i < 16; i++) { adk[0][i] = 0.f; adk[1][i] = 0.f; adv[0][i] = 0.f; adv[1][i] = 0.f; }

  issue(0);
  auto block = [&](auto so_c, auto qb_c) {
    constexpr int SO = decltype(so_c)::value, QB = decltype(qb_c)::value;
    constexpr int O = SO + QB * 4096;
    f32x16 s, dp;
    {
      f16x8 qfr[4];
      f32x4 l4[4];
      D3_READ128(qfr[0], ra[0], O); D3_READ128(qfr[1], ra[1], O); D3_READ128(qfr[2], ra[2], O); D3_READ128(qfr[3], ra[3], O);
      D3_READ128(l4[0], sa, SO + QB * 128); D3_READ128(l4[1], sa, SO + QB * 128 + 32);
      D3_READ128(l4[2], sa, SO + QB * 128 + 64); D3_READ128(l4[3], sa, SO + QB * 128 + 96);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      s = cat16(l4[0], l4[1], l4[2], l4[3]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int t = 0; t < 4; t++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(qfr[t], kf[t], s, 0, 0, 0);  // L - Q . K^T
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      bf16x8 dofr[4];
      f32x4 d4[4];
      D3_READ128(dofr[0], ra[0], O + 2 * TILE16); D3_READ128(dofr[1], ra[1], O + 2 * TILE16);
      D3_READ128(dofr[2], ra[2], O + 2 * TILE16); D3_READ128(dofr[3], ra[3], O + 2 * TILE16);
      D3_READ128(d4[0], sa, SO + QB * 128 + 256); D3_READ128(d4[1], sa, SO + QB * 128 + 288);
      D3_READ128(d4[2], sa, SO + QB * 128 + 320); D3_READ128(d4[3], sa, SO + QB * 128 + 352);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      dp = cat16(d4[0], d4[1], d4[2], d4[3]);
      // delta - dO . V^T, with the block's 16 exponentials (they need only s) in the gaps of the dependent chain
#pragma unroll
      for (int t = 0; t < 4; t++) {
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dofr[t], vf[t], dp, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) s[4 * t + j] = exp2_neg(s[4 * t + j]);
      }
      FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP();
      __builtin_amdgcn_sched_barrier(0);
    }
    // -dS = P * dp'.  One v_mul_f32 per element, by hand: left to the SLP vectoriser the 16 products become 12 v_pk_mul_f32 on
    // register pairs it first has to assemble with 24 v_mov / 16 v_alignbit / v_perm (the exponentials land in scattered registers).
#pragma unroll
    for (int e = 0; e < 16; e++) {
      float x = dp[e];
      asm("v_mul_f32 %0, %0, %1" : "+v"(x) : "v"(s[e]));
      dp[e] = x;
    }
    bf16x8 pf[2], dsf[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; t2++) {
      pf[t2] = pack_frag(s, t2);
      dsf[t2] = pack_frag(dp, t2);
    }
    __builtin_amdgcn_sched_barrier(0);
    s16x4 tl[4], th[4];  // transposed dO / Qb fragments of rows +0..15 (t2 = 0)
    D3_READTR(tl[0], ta[0], O + 2 * TILE16); D3_READTR(th[0], ta8[0], O + 2 * TILE16);
    D3_READTR(tl[1], ta[1], O + 2 * TILE16); D3_READTR(th[1], ta8[1], O + 2 * TILE16);
    D3_READTR(tl[2], ta[0], O + TILE16); D3_READTR(th[2], ta8[0], O + TILE16);
    D3_READTR(tl[3], ta[1], O + TILE16); D3_READTR(th[3], ta8[1], O + TILE16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 fr[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const s16x8 v8 = {tl[j][0], tl[j][1], tl[j][2], tl[j][3], th[j][0], th[j][1], th[j][2], th[j][3]};
      fr[j] = __builtin_bit_cast(bf16x8, v8);
    }
    __builtin_amdgcn_s_setprio(1);
    adv[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0], pf[0], adv[0], 0, 0, 0);
    adk[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2], dsf[0], adk[0], 0, 0, 0);
    adv[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1], pf[0], adv[1], 0, 0, 0);
    adk[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[3], dsf[0], adk[1], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    D3_READTR(tl[0], ta[0], O + 2 * TILE16 + 2048); D3_READTR(th[0], ta8[0], O + 2 * TILE16 + 2048);
    D3_READTR(tl[1], ta[1], O + 2 * TILE16 + 2048); D3_READTR(th[1], ta8[1], O + 2 * TILE16 + 2048);
    D3_READTR(tl[2], ta[0], O + TILE16 + 2048); D3_READTR(th[2], ta8[0], O + TILE16 + 2048);
    D3_READTR(tl[3], ta[1], O + TILE16 + 2048); D3_READTR(th[3], ta8[1], O + TILE16 + 2048);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const s16x8 v8 = {tl[j][0], tl[j][1], tl[j][2], tl[j][3], th[j][0], th[j][1], th[j][2], th[j][3]};
      fr[j] = __builtin_bit_cast(bf16x8, v8);
    }
    __builtin_amdgcn_s_setprio(1);
    adv[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0], pf[1], adv[0], 0, 0, 0);
    adk[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2], dsf[1], adk[0], 0, 0, 0);
    adv[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1], pf[1], adv[1], 0, 0, 0);
    adk[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[3], dsf[1], adk[1], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto step = [&](auto so_c, int qt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (qt + 1 < ntiles) issue(qt + 1);
    if (!active) return;
    block(so_c, std::integral_constant<int, 0>{});
    if (qt * 64 + 32 < kend) block(so_c, std::integral_constant<int, 1>{});
  };
  for (int qt = 0; qt < ntiles; qt += 2) {
    step(std::integral_constant<int, 0>{}, qt);
    if (qt + 1 < ntiles) step(std::integral_constant<int, D3_SLOT>{}, qt + 1);
  }
  __syncthreads();
  ATTN_TRACE_LOOP_END();

  if (active && !kvalid) {
#pragma unroll
    for (int e = 0; e < 16; e++) { adk[0][e] = 0.f; adk[1][e] = 0.f; adv[0][e] = 0.f; adv[1][e] = 0.f; }
  }
  const float nscale = -scale;  // the accumulator holds (-dS)^T . Q
  if (fk.dqkv)
    store_rows_qknorm(smem + wave * 12288, reinterpret_cast<float*>(smem + 4 * 12288), adk, nscale, fk, active, b, h, H, co.tile,
                      (Np + 127) >> 7, key0, Np, lane, wave);
  if (active) {
    char* wst = smem + wave * 12288;
    if (!fk.dqkv) store_rows_f32(wst, adk, nscale, dk + bh * Np * 64, key0, Np, lane);
    char* vst = wst + 8192;
    const int kl = lane & 31;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int d = db * 32 + 8 * g4 + 4 * hi;
        *reinterpret_cast<uint2*>(vst + kl * 128 + (((d >> 3) ^ (kl & 7)) << 4) + (d & 7) * 2) =
            make_uint2(pack_bf16x2(adv[db][4 * g4 + 0], adv[db][4 * g4 + 1]), pack_bf16x2(adv[db][4 * g4 + 2], adv[db][4 * g4 + 3]));
      }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int row = it * 8 + (lane >> 3), ch = lane & 7;
      if (key0 + row < Np)
        *reinterpret_cast<uint4*>(dv + ((long)b * Np + key0 + row) * dv_ld + h * 64 + ch * 8) =
            *reinterpret_cast<const uint4*>(vst + row * 128 + ((ch ^ (row & 7)) << 4));
    }
  }
  ATTN_TRACE_END(2);
}

// ---------------------------------------------------------------------------- dq with the folded statistics
template <bool LENS>
VBX_DEV void attn_bwd_dq_fold_body(char* smem, int wg_id, const u16* __restrict__ q16, const u16* __restrict__ k16,
                                   const u16* __restrict__ kb16, const u16* __restrict__ vv, const uint8_t* __restrict__ mask,
                                   const u16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
                                   float* __restrict__ dq, int H, int Np, float scale, int BH, int xmap, const QKBwd& fq,
                                   const int* __restrict__ key_lens) {
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5;
  const AttnCoord co = attn_coord_id(wg_id, H, Np, BH, xmap);
  if (!co.ok) return;
  ATTN_TRACE_BEGIN();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = co.h, b = co.b;
  const long bh = (long)b * H + h;
  int kend = Np;  // uniform over the workgroup
  if constexpr (LENS) {
    kend = min(max(key_lens[b], 1), Np);
    if (co.tile * 128 >= kend) {  // padding queries only (dO = 0): zero dq rows (and gamma partials), no DMA
      attn_bwd_zero_tile(dq, fq, nullptr, 0, b, h, H, co.tile, Np);
      ATTN_TRACE_END(1);
      return;
    }
  }
  const u16* kbase = k16 + bh * Np * 64;
  const u16* kbbase = kb16 + bh * Np * 64;
  const u16* vbase = vv + bh * Np * 64;
  const int q0 = co.tile * 128 + wave * 32;
  const bool active = q0 < Np;
  const int q = q0 + (lane & 31);
  const int qc = min(q, Np - 1);
  const int ntiles = (kend + 63) / 64;  // key tiles

  f16x8 qf[4];    // -Q (pre-scaled)
  bf16x8 dof[4];  // -dO
#pragma unroll
  for (int t = 0; t < 4; t++) {
    qf[t] = neg_f16x8(*reinterpret_cast<const f16x8*>(q16 + (bh * Np + qc) * 64 + 16 * t + 8 * hi));
    dof[t] = neg_bf16x8(*reinterpret_cast<const bf16x8*>(dout + ((long)b * Np + qc) * (H * 64) + h * 64 + 16 * t + 8 * hi));
  }
  const float L2 = lse[bh * Np + qc];
  const float dlt = delta[bh * Np + qc];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    asm volatile("" ::"v"(qf[t]));
    asm volatile("" ::"v"(dof[t]));
  }
  // The lane's L as a C operand (read-only for the whole key loop).  delta stays a VALU add: a second persistent 16-register tuple
  // put the body at 182 registers -- 17 spilled inside the key loop at three waves per SIMD.
  f32x16 Lc;
#pragma unroll
  for (int e = 0; e < 16; e++) Lc[e] = L2;
  asm volatile("" : "+v"(Lc));  // materialise the 16 registers here, once

  unsigned dvo[2];  // per-lane byte offsets inside a 64-row tile (round 6: scalar-base LDS-DMA, see the dk/dv body)
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int sidx = i * 256 + tid, row = sidx >> 3;
    dvo[i] = (unsigned)(row * 128 + (((sidx & 7) ^ attn_swz(row)) << 4));
  }
  const unsigned m0b = __builtin_amdgcn_readfirstlane(lds_addr32(smem) + (unsigned)(tid & ~63) * 16u);
  auto issue = [&](int kt) {
    const unsigned so = (unsigned)((kt & 1) * Q3_SLOT);
    unsigned o0 = dvo[0], o1 = dvo[1];
    if ((kt + 1) * 64 > kend) {
      const unsigned lim = (unsigned)(kend - 1 - kt * 64);
      o0 -= ((o0 >> 7) - min(o0 >> 7, lim)) << 7;
      o1 -= ((o1 >> 7) - min(o1 >> 7, lim)) << 7;
    }
    const u16* s0 = kbase + (long)kt * 4096;
    const u16* s1 = kbbase + (long)kt * 4096;
    const u16* s2 = vbase + (long)kt * 4096;
    glds16_sbase(o0, s0, m0b + so);
    glds16_sbase(o1, s0, m0b + so + 4096u);
    glds16_sbase(o0, s1, m0b + so + (unsigned)TILE16);
    glds16_sbase(o1, s1, m0b + so + (unsigned)TILE16 + 4096u);
    glds16_sbase(o0, s2, m0b + so + 2u * TILE16);
    glds16_sbase(o1, s2, m0b + so + 2u * TILE16 + 4096u);
  };
#define VBX_BWD_RAGGED_DQ
#include "attn_bwd_ragged.inc"
#undef VBX_BWD_RAGGED_DQ
  issue(0);

  unsigned ra[4], ta[2], ta8[2];
  {
    const int row = lane & 31;
    const int G = lane >> 4, a16 = lane & 15;
    const int trow = 4 * (G >> 1) + (a16 >> 2);
#pragma unroll
    for (int t = 0; t < 4; t++) ra[t] = lds_addr32(smem + swz_off2(row, 2 * t + hi));
#pragma unroll
    for (int db = 0; db < 2; db++) {
      const int d = db * 32 + (G & 1) * 16 + 4 * (a16 & 3);
      ta[db] = lds_addr32(smem + TILE16 + swz_off2(trow, d >> 3) + (d & 7) * 2);
      ta8[db] = lds_addr32(smem + TILE16 + swz_off2(trow + 8, d >> 3) + (d & 7) * 2);
    }
  }

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 16; i++) { acc[0][i] = 0.f; acc[1][i] = 0.f; }

  auto block = [&](auto so_c, auto kb_c, int k0, bool need_mask) {
    constexpr int SO = decltype(so_c)::value, KB = decltype(kb_c)::value;
    constexpr int O = SO + KB * 4096;
    f32x16 s, dp;
    {
      f16x8 kfr[4];
      D3_READ128(kfr[0], ra[0], O); D3_READ128(kfr[1], ra[1], O); D3_READ128(kfr[2], ra[2], O); D3_READ128(kfr[3], ra[3], O);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr[0], qf[0], Lc, 0, 0, 0);  // L - K . Q^T
#pragma unroll
      for (int t = 1; t < 4; t++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr[t], qf[t], s, 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
    s16x4 tl[4], th[4];
    {
      bf16x8 vfr[4];
      D3_READ128(vfr[0], ra[0], O + 2 * TILE16); D3_READ128(vfr[1], ra[1], O + 2 * TILE16);
      D3_READ128(vfr[2], ra[2], O + 2 * TILE16); D3_READ128(vfr[3], ra[3], O + 2 * TILE16);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 16; e++) dp[e] = 0.f;
#pragma unroll
      for (int t = 0; t < 4; t++) {  // -(V . dO^T)
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[t], dof[t], dp, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) s[4 * t + j] = exp2_neg(s[4 * t + j]);
      }
      FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP(); FOLD_SGB_MFMA_EXP();
      __builtin_amdgcn_sched_barrier(0);
    }
    // Kb^T fragments of keys +0..15 (into the registers the V fragments just left): they land while the VALU block runs
    D3_READTR(tl[0], ta[0], O); D3_READTR(th[0], ta8[0], O);
    D3_READTR(tl[1], ta[1], O); D3_READTR(th[1], ta8[1], O);
    D3_READTR(tl[2], ta[0], O + 2048); D3_READTR(th[2], ta8[0], O + 2048);
    D3_READTR(tl[3], ta[1], O + 2048); D3_READTR(th[3], ta8[1], O + 2048);
    __builtin_amdgcn_sched_barrier(0);
    if (need_mask) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int kg = k0 + KB * 32 + acc_row(r, hi);
        bool ok = kg < kend;
        if (ok && mask) ok = mask[(long)b * Np + kg] != 0;
        if (!ok) s[r] = 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) s[r] *= dlt + dp[r];  // -dS^T = P * (delta - dP)
    const bf16x8 ds0 = pack_frag(s, 0), ds1 = pack_frag(s, 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 fr[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const s16x8 v8 = {tl[j][0], tl[j][1], tl[j][2], tl[j][3], th[j][0], th[j][1], th[j][2], th[j][3]};
      fr[j] = __builtin_bit_cast(bf16x8, v8);
    }
    __builtin_amdgcn_s_setprio(1);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0], ds0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1], ds0, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2], ds1, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[3], ds1, acc[1], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto step = [&](auto so_c, int kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < ntiles) issue(kt + 1);
    if (!active) return;
    const int k0 = kt * 64;
    const bool need_mask = (mask != nullptr) || (k0 + 64 > kend);
    block(so_c, std::integral_constant<int, 0>{}, k0, need_mask);
    if (k0 + 32 < kend) block(so_c, std::integral_constant<int, 1>{}, k0, need_mask);
  };
  for (int kt = 0; kt < ntiles; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) step(std::integral_constant<int, Q3_SLOT>{}, kt + 1);
  }
  __syncthreads();
  ATTN_TRACE_LOOP_END();

  const float nscale = -scale;  // the accumulator holds Kb^T . (-dS^T)
  if (fq.dqkv) {
    store_rows_qknorm(smem + wave * 8192, reinterpret_cast<float*>(smem + 4 * 8192), acc, nscale, fq, active, b, h, H, co.tile,
                      (Np + 127) >> 7, q0, Np, lane, wave);
    ATTN_TRACE_END(1);
    return;
  }
  if (active) store_rows_f32(smem + wave * 8192, acc, nscale, dq + bh * Np * 64, q0, Np, lane);
  ATTN_TRACE_END(1);
}

// blockIdx -> (role, workgroup id of that role's grid).  Launch order: tails of both roles, dk/dv full tiles (the longer ones), dq full
// tiles (as attn_bwd_kernel_dma).
template <bool LENS>
VBX_DEV void attn_bwd_fold_roles(char* smem, const AttnBwdArgs& a, const int* __restrict__ key_lens) {
  int id = blockIdx.x, role;
  if (a.role) {
    role = a.role == 1;
  } else {
    const int T = attn_tail_ids(a.Np, a.BH, a.xmap), F = a.grid_one - T;
    if (a.xmap & 2) {
      if (id < 2 * F) { role = id >= F; id -= role * F; }
      else { id -= 2 * F; role = id >= T; id += F - role * T; }
    } else if (id < 2 * T) {
      role = id >= T;
      id -= role * T;
    } else {
      id -= 2 * T;
      role = id >= F;
      id += T - role * F;
    }
  }
  if (role)
    attn_bwd_dq_fold_body<LENS>(smem, id, a.q16, a.k16, a.kb16, a.vv, a.mask, a.dout, a.lse, a.delta, a.dq, a.H, a.Np, a.scale, a.BH,
                                a.xmap, a.fq, key_lens);
  else
    attn_bwd_dkdv_fold_body<LENS>(smem, id, a.q16, a.qb16, a.k16, a.vv, a.mask, a.dout, a.lse, a.delta, a.dk, a.dv, a.dv_ld, a.H, a.Np,
                                  a.scale, a.BH, a.xmap, a.fk, key_lens);
}
__global__ __launch_bounds__(256, 3) void attn_bwd_kernel_fold(const AttnBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_bwd_fold_roles<false>(smem, a, nullptr);
}
// the same two bodies with per-batch-row prefix lengths (training on ragged batches, lens=): same launch order, XCD map and tail roles.
// key_lens is a parameter of its own, behind AttnBwdArgs: no other kernel's argument block changes.
__global__ __launch_bounds__(256, 3) void attn_bwd_kernel_fold_lens(const AttnBwdArgs a, const int* __restrict__ key_lens) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_bwd_fold_roles<true>(smem, a, key_lens);
}
