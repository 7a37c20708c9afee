// Body of attn_fwd_kernel_v3 (included inside the kernel, not a header): expects the kernel parameters q16, k16, vv, mask, out,
// outb, lse, H, Np, scale2, BH, xmap and `smem`.  With VBX_FWD_DROP defined (training-time attention dropout, attend.py:131) also
// dbits (row-major keep bits R[bh][q][W2], ops.hip), W2 and rkeep: the softmax statistics (row maximum, row sum, LSE) are those
// of the UNdropped probabilities, dropped entries are zeroed in the P fragment only, and 1 / keep rides in the final 1 / l.
// With VBX_FWD_LENS defined (the sampler's prefix lengths, vbx_attn_fwd_lens) also key_lens [B]: keys at or past key_lens[b] are
// masked whatever `mask` says, so the key loop and the DMA ring stop at tile ceil(key_lens[b] / 64) -- a tile past it has maximum -inf
// and probabilities 0, it would add +0 to l and O and leave m alone -- and a query tile wholly at or past key_lens[b] (padding
// queries only) writes zeros and lse 1e30 without touching K or V.  Without the macro the text below is what it was.
// With VBX_FWD_SEGS defined (packed rows, vbx_attn_fwd_segs; include/vbx.h "packed rows") there is ONE batch row of Np = Mp rows, a
// multiple of 128, no `mask` parameter, and seg_start / seg_klen / tile_seg: the workgroup of query tile t serves segment
// s = tile_seg[t] and walks ceil(seg_klen[s] / 64) key tiles from row seg_start[s]; key indices below are LOCAL to the segment, the
// DMA never leaves its live rows (the partial tile re-reads row seg_klen[s] - 1), a query row at or past seg_klen[s] writes zeros
// and lse 1e30, and so does a whole tile with s < 0.  There is no ragged tail role: every tile has 128 rows.
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
  const AttnCoord co = attn_coord(H, Np, BH, xmap);
  if (!co.ok) return;
  ATTN_TRACE_BEGIN();
  const int h = co.h, b = co.b;
  const long bh = (long)b * H + h;
#ifdef VBX_FWD_SEGS
  const uint8_t* const mask = nullptr;
  const int seg = tile_seg[co.tile];  // uniform over the workgroup, like everything read through it
  const int sst = seg < 0 ? 0 : seg_start[seg];
  const int kend = seg < 0 ? 0 : seg_klen[seg];
  const u16* kbase = k16 + (bh * Np + sst) * 64;
  const u16* vbase = vv + (bh * Np + sst) * 64;
#define VBX_KROWS kend  // rows the K | V tile DMA may read, counted from kbase
#else
  const u16* kbase = k16 + bh * Np * 64;
  const u16* vbase = vv + bh * Np * 64;
#define VBX_KROWS Np
#endif
  const int q0 = co.tile * 128 + wave * 32;
  const bool active = q0 < Np;
  const int q = q0 + (lane & 31);
  const int qc = min(q, Np - 1);
#ifdef VBX_FWD_SEGS
  const int ntiles = (kend + 63) / 64;
  if (seg < 0) {
    for (int i = tid; i < 128 * 8; i += 256) {
      const int qq = co.tile * 128 + (i >> 3);
      const long go = (long)qq * (H * 64) + h * 64 + (i & 7) * 8;
      *reinterpret_cast<uint4*>(out + go) = make_uint4(0u, 0u, 0u, 0u);
      if (outb) *reinterpret_cast<uint4*>(outb + go) = make_uint4(0u, 0u, 0u, 0u);
      if ((i & 7) == 0) lse[bh * Np + qq] = 1e30f;
    }
    ATTN_TRACE_END(0);
    return;
  }
  const bool qdead = q - sst >= kend;  // a dead row of the segment: zeros and lse 1e30, whatever its q holds
#elif defined(VBX_FWD_LENS)
  const int kend = min(max(key_lens[b], 0), Np);  // uniform over the workgroup
  const int ntiles = (kend + 63) / 64;
  if (co.tile * 128 >= kend) {
    for (int i = tid; i < 128 * 8; i += 256) {
      const int qq = co.tile * 128 + (i >> 3);
      if (qq < Np) {
        const long go = ((long)b * Np + qq) * (H * 64) + h * 64 + (i & 7) * 8;
        *reinterpret_cast<uint4*>(out + go) = make_uint4(0u, 0u, 0u, 0u);
        if (outb) *reinterpret_cast<uint4*>(outb + go) = make_uint4(0u, 0u, 0u, 0u);
        if ((i & 7) == 0) lse[bh * Np + qq] = 1e30f;
      }
    }
    ATTN_TRACE_END(0);
    return;
  }
#else
  const int ntiles = (Np + 63) / 64;
#endif

  // K|V tile DMA (round 6): the per-lane part of the source address is a 32-bit offset inside a 64-row tile, computed ONCE; the
  // tile's base pointer and the LDS destination are scalars, so a tile costs 4 LDS-DMA instructions and no vector ALU work (the
  // round-5 loop spent ~35 vector / scalar-move instructions per tile on 64-bit addresses and v_readfirstlane -> m0).
  unsigned dvo[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int s = i * 256 + tid, row = s >> 3;
    dvo[i] = (unsigned)(row * 128 + (((s & 7) ^ attn_swz(row)) << 4));
  }
  const unsigned m0b = __builtin_amdgcn_readfirstlane(lds_addr32(smem) + (unsigned)(tid & ~63) * 16u);
  auto dma_kv = [&](unsigned slot_off, int kt) {
    unsigned o0 = dvo[0], o1 = dvo[1];
    if ((kt + 1) * 64 > VBX_KROWS) {  // the last, partial tile: rows past the end re-read the last row (masked, never stored)
      const unsigned lim = (unsigned)(VBX_KROWS - 1 - kt * 64);
      o0 -= ((o0 >> 7) - min(o0 >> 7, lim)) << 7;
      o1 -= ((o1 >> 7) - min(o1 >> 7, lim)) << 7;
    }
    const u16* kb = kbase + (long)kt * 4096;
    const u16* vb = vbase + (long)kt * 4096;
    glds16_sbase(o0, kb, m0b + slot_off);
    glds16_sbase(o1, kb, m0b + slot_off + 4096u);
    glds16_sbase(o0, vb, m0b + slot_off + (unsigned)TILE16);
    glds16_sbase(o1, vb, m0b + slot_off + (unsigned)TILE16 + 4096u);
  };
  dma_kv(0u, 0);

#if !defined(VBX_FWD_DROP) && !defined(VBX_FWD_SEGS)
  // ---- ragged tail tile (round 6): <= 16 query rows (the 16 register tokens at the benchmark's Np = 1040).  Such a workgroup used to
  // walk the key loop with one active wave of 32-query blocks: 26 us of life for 1/8 of a wave's work.  Here its four waves split
  // every 64-key tile into 16-key blocks and run 16 x 16 MFMA shapes on the 16 queries -- S^T[16 keys][16 q] = 2 x 16x16x32,
  // O^T[64 d][16 q] += V^T . P^T = 4 x 16x16x16 per wave and tile -- then merge their (m, l, O) through LDS.  (attend.py:119-137)
  if (co.tile == (Np >> 7) && (Np & 127) <= 16 && !(xmap & 4)) {  // xmap bit 2: without the ragged role (no caller sets it, attn_coord_id)
#include "attn_fwd_ragged.inc"
    ATTN_TRACE_END(0);
    return;
  }
#endif

  f16x8 qf[4];
#pragma unroll
  for (int t = 0; t < 4; t++)
    qf[t] = *reinterpret_cast<const f16x8*>(q16 + (bh * Np + qc) * 64 + 16 * t + 8 * hi);
#pragma unroll
  for (int t = 0; t < 4; t++) asm volatile("" ::"v"(qf[t]));  // retire the Q loads here (see v2)

  unsigned ka[4], va[2], va8[2];
  {
    const int row = lane & 31;
#pragma unroll
    for (int t = 0; t < 4; t++) ka[t] = lds_addr32(smem + swz_off2(row, 2 * t + hi));
    const int G = lane >> 4, a16 = lane & 15;
    const int vrow = 4 * (G >> 1) + (a16 >> 2);
#pragma unroll
    for (int db = 0; db < 2; db++) {
      const int d = db * 32 + (G & 1) * 16 + 4 * (a16 & 3);
      va[db] = lds_addr32(smem + TILE16 + swz_off2(vrow, d >> 3) + (d & 7) * 2);
      va8[db] = lds_addr32(smem + TILE16 + swz_off2(vrow + 8, d >> 3) + (d & 7) * 2);
    }
  }

  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; i++) { o[0][i] = 0.f; o[1][i] = 0.f; }
  float m_run = NEG_INF, l_run = 0.f;
#ifdef VBX_FWD_DROP
  const unsigned* brow = dbits + (bh * Np + qc) * W2;
  uint2 wkeep = *reinterpret_cast<const uint2*>(brow);  // keep bits of key tile 0; tile kt + 1 is requested during step kt
#endif

  // (Round 5 tried a HALF variant of this step for the ragged LAST key tile -- Np = 1040 leaves a 17th tile of 16 keys whose second
  //  32-key block is computed and masked away: 8 of its 16 MFMAs and half of its softmax skipped once per workgroup.  Stand-alone
  //  forward 70.5 / 71.7 us -> 71.1 / 69.8 us: nothing measurable -- and the extra instantiations pushed the kernel to 14 spilled
  //  registers, two of them the V^T fragments of an inline-asm ds_read spilled BEFORE their s_waitcnt (wrong results whenever the
  //  half tile sat in ring slot 1).  Removed.)
  auto step = [&](auto stg_c, int kt) {
    constexpr int STG = decltype(stg_c)::value;
    constexpr int SO = STG * ASTAGE;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's pieces of tile kt have landed
    __builtin_amdgcn_s_barrier();                     // tile kt visible to all; everyone is done with tile kt-1
    // The next tile's four LDS-DMA pieces are issued here, behind the barrier.  Five later placements were measured (behind the first /
    // second S chain, behind the softmax, behind the issue of the first / of both K fragment read groups): 63.1-64.4 us for every one
    // in the unstamped kernel.  Their arms, the per-step stamps and the timing ablations of this step were removed; the figures are in
    // profiles/r06_attn_fwd_steptrace.txt, profiles/r06_attn_fwd_ablation.txt and docs/history.md.
    if (kt + 1 < ntiles) dma_kv((unsigned)((STG ^ 1) * ASTAGE), kt + 1);
    if (!active) return;
    const int k0 = kt * 64;
    f32x16 s[2];
#pragma unroll
    for (int i = 0; i < 16; i++) { s[0][i] = 0.f; s[1][i] = 0.f; }
    {
      f16x8 kf[4];
      kf[0] = asm_read_b128<SO>(ka[0]); kf[1] = asm_read_b128<SO>(ka[1]);
      kf[2] = asm_read_b128<SO>(ka[2]); kf[3] = asm_read_b128<SO>(ka[3]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int t = 0; t < 4; t++) s[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[t], qf[t], s[0], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      kf[0] = asm_read_b128<SO + 4096>(ka[0]); kf[1] = asm_read_b128<SO + 4096>(ka[1]);
      kf[2] = asm_read_b128<SO + 4096>(ka[2]); kf[3] = asm_read_b128<SO + 4096>(ka[3]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int t = 0; t < 4; t++) s[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[t], qf[t], s[1], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    // V^T fragments of the first 32-key block: requested now, consumed after the softmax
    s16x4 vl[4], vh[4];
    asm_read_tr<SO>(vl[0], vh[0], va[0], va8[0]);
    asm_read_tr<SO>(vl[1], vh[1], va[1], va8[1]);
    asm_read_tr<SO + 2048>(vl[2], vh[2], va[0], va8[0]);
    asm_read_tr<SO + 2048>(vl[3], vh[3], va[1], va8[1]);
#if defined(VBX_FWD_LENS) || defined(VBX_FWD_SEGS)
    const bool need_mask = (mask != nullptr) || (k0 + 64 > kend);
#else
    const bool need_mask = (mask != nullptr) || (k0 + 64 > Np);
#endif
    if (need_mask) {
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int kg = k0 + kb * 32 + acc_row(r, hi);
#if defined(VBX_FWD_LENS) || defined(VBX_FWD_SEGS)
          bool ok = kg < kend;
#else
          bool ok = kg < Np;
#endif
          if (ok && mask) ok = mask[(long)b * Np + kg] != 0;
          if (!ok) s[kb][r] = NEG_INF;
        }
    }
    float mx = NEG_INF;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
    mx = xhalf_max(mx);  // v_permlane32_swap: no LDS round trip on the softmax's critical path
    const float m_new = fmaxf(m_run, mx * scale2);
    const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
    const float alpha = fast_exp2(m_run - m_use);
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 sc2 = {scale2, scale2}, mneg = {-m_use, -m_use};
    f2 ps2 = {0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f2 sv = {s[kb][r], s[kb][r + 1]};
        const f2 e = __builtin_elementwise_fma(sv, sc2, mneg);
        const f2 p = {fast_exp2(e.x), fast_exp2(e.y)};
        s[kb][r] = p.x;
        s[kb][r + 1] = p.y;
        ps2 += p;
      }
    l_run = l_run * alpha + (ps2.x + ps2.y);
    m_run = m_new;
#ifdef VBX_FWD_DROP
    {
      const unsigned w0 = wkeep.x >> (4 * hi), w1 = wkeep.y >> (4 * hi);  // register r <-> key 8 * (r / 4) + 4 * hi + r % 4
#pragma unroll
      for (int r = 0; r < 16; r++) {
        if (!((w0 >> (8 * (r >> 2) + (r & 3))) & 1u)) s[0][r] = 0.f;
        if (!((w1 >> (8 * (r >> 2) + (r & 3))) & 1u)) s[1][r] = 0.f;
      }
      if (kt + 1 < ntiles) wkeep = *reinterpret_cast<const uint2*>(brow + 2 * (kt + 1));
    }
#endif
    {
      const f2 a2 = {alpha, alpha};
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        f2 t0 = {o[0][i], o[0][i + 1]}, t1 = {o[1][i], o[1][i + 1]};
        t0 *= a2;
        t1 *= a2;
        o[0][i] = t0.x; o[0][i + 1] = t0.y;
        o[1][i] = t1.x; o[1][i + 1] = t1.y;
      }
    }
#define VBX_PV3(KB)                                                                                             \
    {                                                                                                           \
      const f16x8 p0 = pack_frag_f16_fast(s[KB], 0), p1 = pack_frag_f16_fast(s[KB], 1);                         \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
      f16x8 vf[4];                                                                                              \
      _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                           \
        const s16x8 t = {vl[j][0], vl[j][1], vl[j][2], vl[j][3], vh[j][0], vh[j][1], vh[j][2], vh[j][3]};       \
        vf[j] = __builtin_bit_cast(f16x8, t);                                                                   \
      }                                                                                                         \
      __builtin_amdgcn_s_setprio(1);                                                                            \
      o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0], p0, o[0], 0, 0, 0);                                  \
      o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1], p0, o[1], 0, 0, 0);                                  \
      o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[2], p1, o[0], 0, 0, 0);                                  \
      o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[3], p1, o[1], 0, 0, 0);                                  \
      __builtin_amdgcn_s_setprio(0);                                                                            \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    VBX_PV3(0)
    asm_read_tr<SO + 4096>(vl[0], vh[0], va[0], va8[0]);
    asm_read_tr<SO + 4096>(vl[1], vh[1], va[1], va8[1]);
    asm_read_tr<SO + 4096 + 2048>(vl[2], vh[2], va[0], va8[0]);
    asm_read_tr<SO + 4096 + 2048>(vl[3], vh[3], va[1], va8[1]);
    VBX_PV3(1)
#undef VBX_PV3
  };
  for (int kt = 0; kt < ntiles; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) step(std::integral_constant<int, 1>{}, kt + 1);
  }
  __syncthreads();  // every wave is done with the ring before it becomes epilogue staging space
  ATTN_TRACE_LOOP_END();

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
#ifdef VBX_FWD_DROP
  const float inv = (l_tot > 0.f) ? rkeep / l_tot : 0.f;
#else
  const float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
#endif
#ifdef VBX_FWD_SEGS
  if (hi == 0) lse[bh * Np + q] = (l_tot > 0.f && !qdead) ? (m_run + log2f(l_tot)) : 1e30f;
#else
  if (active && hi == 0 && q < Np) lse[bh * Np + q] = (l_tot > 0.f) ? (m_run + log2f(l_tot)) : 1e30f;
#endif
  char* ost = smem + wave * 8192;
  if (active) {
    const int ql = lane & 31;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int d = db * 32 + 8 * g4 + 4 * hi;
#ifdef VBX_FWD_SEGS
        const float v0 = qdead ? 0.f : o[db][4 * g4 + 0] * inv, v1 = qdead ? 0.f : o[db][4 * g4 + 1] * inv,
                    v2 = qdead ? 0.f : o[db][4 * g4 + 2] * inv, v3 = qdead ? 0.f : o[db][4 * g4 + 3] * inv;
#else
        const float v0 = o[db][4 * g4 + 0] * inv, v1 = o[db][4 * g4 + 1] * inv, v2 = o[db][4 * g4 + 2] * inv,
                    v3 = o[db][4 * g4 + 3] * inv;
#endif
        const int off = ql * 128 + ((((d >> 3) ^ (ql & 7))) << 4) + (d & 7) * 2;
        *reinterpret_cast<uint2*>(ost + off) = make_uint2(pack_f16x2(v0, v1), pack_f16x2(v2, v3));
        if (outb) *reinterpret_cast<uint2*>(ost + 4096 + off) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
      }
  }
  __builtin_amdgcn_wave_barrier();
  if (active) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int row = it * 8 + (lane >> 3), ch = lane & 7;
      const int qq = q0 + row;
      if (qq < Np) {
        const int off = row * 128 + ((ch ^ (row & 7)) << 4);
        const long go = ((long)b * Np + qq) * (H * 64) + h * 64 + ch * 8;
        *reinterpret_cast<uint4*>(out + go) = *reinterpret_cast<const uint4*>(ost + off);
        if (outb) *reinterpret_cast<uint4*>(outb + go) = *reinterpret_cast<const uint4*>(ost + 4096 + off);
      }
    }
  }
#undef VBX_KROWS
  ATTN_TRACE_END(0);
