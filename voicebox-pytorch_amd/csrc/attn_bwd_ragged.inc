// Ragged tail roles of the folded attention backward (round 6; included inside the two bodies of attn_bwd_fold.inc, after their
// `issue` lambdas): the workgroup's 128-row tile holds R <= 16 rows -- the 16 register tokens at the benchmark's Np = 1040.  Such a
// workgroup used to walk all 17 ring steps with one active wave of 32 x 32 blocks.  Here the four waves split every 64-row ring
// tile into 16-row blocks and run 16 x 16 MFMA shapes against the 16 stationary rows:
//   dq role   (stationary: the R queries; ring: K16 | Kb | V tiles; wave w owns keys 16 w .. 16 w + 15 of each tile)
//       S^T[16 k][16 q]  = K . Q^T            2 x 16x16x32 f16        dP^T = V . dO^T           2 x 16x16x32 bf16
//       dS^T = P o (dP^T - delta),  P = exp2(S^T - L)                  dq^T[64 d][16 q] += Kb^T . dS^T   4 x 16x16x16 bf16
//   dk/dv role (stationary: the R keys; ring: Q16 | Qb | dO | L | delta; wave w owns queries 16 w .. 16 w + 15 of each tile)
//       S[16 q][16 k]    = Q . K^T            dP = dO . V^T            dv^T[64 d][16 k] += dO^T . P,  dk^T += Qb^T . dS
// A lane owns the stationary row (lane & 15) and four ring rows 4 (lane >> 4) .. + 3, so the S / dP values it holds ARE the B
// fragments of the second products.  No statistics fold here (plain VALU subtracts): these workgroups are latency-bound.  The four
// waves' partial blocks are summed through LDS in the staging layout of store_rows_qknorm / store_rows_f32, whose row passes then
// run unchanged.  Reference: autograd of attend.py:121-135.  `kend` is the bodies' live-key bound (Np, or key_lens[b] in their
// length-aware instantiations, whose `ntiles` and `issue` stop there too).
#ifdef VBX_BWD_RAGGED_DQ
  if (co.tile == (Np >> 7) && (Np & 127) <= 16 && !(xmap & 4)) {
    const int qi = lane & 15, g = lane >> 4;
    const int qb0 = co.tile * 128;
    const int qrow = min(qb0 + qi, Np - 1);
    f16x8 qf2[2];
    bf16x8 dof2[2];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      qf2[ks] = *reinterpret_cast<const f16x8*>(q16 + (bh * Np + qrow) * 64 + 32 * ks + 8 * g);
      dof2[ks] = *reinterpret_cast<const bf16x8*>(dout + ((long)b * Np + qrow) * (H * 64) + h * 64 + 32 * ks + 8 * g);
    }
    const float Lq = lse[bh * Np + qrow], dlq = delta[bh * Np + qrow];
    asm volatile("" ::"v"(qf2[0]), "v"(qf2[1]), "v"(dof2[0]), "v"(dof2[1]), "v"(Lq), "v"(dlq));
    unsigned ka2[2], kta[4];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) ka2[ks] = lds_addr32(smem + swz_off2(wave * 16 + qi, 4 * ks + g));
#pragma unroll
    for (int db = 0; db < 4; db++) {
      const int d = 16 * db + 4 * (qi & 3);
      kta[db] = lds_addr32(smem + TILE16 + swz_off2(wave * 16 + 4 * g + (qi >> 2), d >> 3) + (d & 7) * 2);
    }
    f32x4 acc4[4];
#pragma unroll
    for (int db = 0; db < 4; db++) acc4[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    issue(0);
    for (int kt = 0; kt < ntiles; kt++) {
      const unsigned so = (unsigned)((kt & 1) * Q3_SLOT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 1 < ntiles) issue(kt + 1);
      f16x8 kf0, kf1;
      bf16x8 vf0, vf1;
      s16x4 ktr[4];
      D3_READ128(kf0, ka2[0] + so, 0); D3_READ128(kf1, ka2[1] + so, 0);
      D3_READ128(vf0, ka2[0] + so, 2 * TILE16); D3_READ128(vf1, ka2[1] + so, 2 * TILE16);
#pragma unroll
      for (int db = 0; db < 4; db++) D3_READTR(ktr[db], kta[db] + so, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = {0.f, 0.f, 0.f, 0.f};
      s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0, qf2[0], s4, 0, 0, 0);
      s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1, qf2[1], s4, 0, 0, 0);
      dp4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, dof2[0], dp4, 0, 0, 0);
      dp4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, dof2[1], dp4, 0, 0, 0);
      const int kg0 = kt * 64 + wave * 16 + 4 * g;
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int kg = kg0 + i;
        bool ok = kg < kend;
        if (ok && mask) ok = mask[(long)b * Np + kg] != 0;
        const float p = ok ? __builtin_amdgcn_exp2f(s4[i] - Lq) : 0.f;
        ds[i] = p * (dp4[i] - dlq);
      }
      bf16x4 dsf;
#pragma unroll
      for (int i = 0; i < 4; i++) dsf[i] = (__bf16)ds[i];
#pragma unroll
      for (int db = 0; db < 4; db++)
        acc4[db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ktr[db], __builtin_bit_cast(s16x4, dsf), acc4[db], 0, 0, 0);
    }
    __syncthreads();  // the ring becomes staging space: one [32 rows][64 fp32] block per wave, layout of store_rows_qknorm
#pragma unroll
    for (int db = 0; db < 4; db++) {
      const int c = 4 * db + g;
      *reinterpret_cast<float4*>(smem + wave * 8192 + qi * 256 + ((c ^ qi) << 4)) =
          make_float4(acc4[db][0] * scale, acc4[db][1] * scale, acc4[db][2] * scale, acc4[db][3] * scale);
    }
    __syncthreads();
    {
      const int row = tid >> 4, c = tid & 15;
      const int off = row * 256 + ((c ^ row) << 4);
      float4 t0 = *reinterpret_cast<const float4*>(smem + off);
#pragma unroll
      for (int w = 1; w < 4; w++) {
        const float4 t = *reinterpret_cast<const float4*>(smem + w * 8192 + off);
        t0.x += t.x; t0.y += t.y; t0.z += t.z; t0.w += t.w;
      }
      __syncthreads();
      *reinterpret_cast<float4*>(smem + off) = t0;
    }
    __syncthreads();
    if (fq.dqkv) {
      f32x16 dummy[2];
      store_rows_qknorm(smem, reinterpret_cast<float*>(smem + 4 * 8192), dummy, 0.f, fq, wave == 0, b, h, H, co.tile, (Np + 127) >> 7,
                        qb0, Np, lane, wave, true);
    } else if (wave == 0) {
#pragma unroll
      for (int it = 0; it < 4; it++) {
        const int row = it * 4 + (lane >> 4), ch = lane & 15;
        if (qb0 + row < Np)
          *reinterpret_cast<float4*>(dq + bh * Np * 64 + (long)(qb0 + row) * 64 + ch * 4) =
              *reinterpret_cast<const float4*>(smem + row * 256 + ((ch ^ row) << 4));
      }
    }
    ATTN_TRACE_END(1);
    return;
  }
#endif
#ifdef VBX_BWD_RAGGED_DKDV
  if (co.tile == (Np >> 7) && (Np & 127) <= 16 && !(xmap & 4)) {
    const int ki = lane & 15, g = lane >> 4;
    const int kb0 = co.tile * 128;
    const int R = Np - kb0;
    const int krow = min(kb0 + ki, Np - 1);
    bool kval = kb0 + ki < kend;
    if (kval && mask) kval = mask[(long)b * Np + kb0 + ki] != 0;
    f16x8 kf2[2];
    bf16x8 vf2[2];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      kf2[ks] = *reinterpret_cast<const f16x8*>(k16 + (bh * Np + krow) * 64 + 32 * ks + 8 * g);
      vf2[ks] = *reinterpret_cast<const bf16x8*>(vv + (bh * Np + krow) * 64 + 32 * ks + 8 * g);
    }
    asm volatile("" ::"v"(kf2[0]), "v"(kf2[1]), "v"(vf2[0]), "v"(vf2[1]), "v"(kval));
    unsigned qa[2], ta4[4];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) qa[ks] = lds_addr32(smem + swz_off2(wave * 16 + ki, 4 * ks + g));
#pragma unroll
    for (int db = 0; db < 4; db++) {
      const int d = 16 * db + 4 * (ki & 3);
      ta4[db] = lds_addr32(smem + swz_off2(wave * 16 + 4 * g + (ki >> 2), d >> 3) + (d & 7) * 2);
    }
    const unsigned la = lds_addr32(smem + 3 * TILE16 + (wave * 16 + 4 * g) * 4);
    f32x4 adv4[4], adk4[4];
#pragma unroll
    for (int db = 0; db < 4; db++) { adv4[db] = (f32x4){0.f, 0.f, 0.f, 0.f}; adk4[db] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    issue(0);
    for (int qt = 0; qt < ntiles; qt++) {
      const unsigned so = (unsigned)((qt & 1) * D3_SLOT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (qt + 1 < ntiles) issue(qt + 1);
      f16x8 qf0, qf1;
      bf16x8 df0, df1;
      f32x4 L4, D4;
      s16x4 dotr[4], qbtr[4];
      D3_READ128(qf0, qa[0] + so, 0); D3_READ128(qf1, qa[1] + so, 0);
      D3_READ128(df0, qa[0] + so, 2 * TILE16); D3_READ128(df1, qa[1] + so, 2 * TILE16);
      D3_READ128(L4, la + so, 0); D3_READ128(D4, la + so, 256);
#pragma unroll
      for (int db = 0; db < 4; db++) { D3_READTR(dotr[db], ta4[db] + so, 2 * TILE16); D3_READTR(qbtr[db], ta4[db] + so, TILE16); }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = {0.f, 0.f, 0.f, 0.f};
      s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf0, kf2[0], s4, 0, 0, 0);
      s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf1, kf2[1], s4, 0, 0, 0);
      dp4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df0, vf2[0], dp4, 0, 0, 0);
      dp4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df1, vf2[1], dp4, 0, 0, 0);
      bf16x4 pf, dsf;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float p = __builtin_amdgcn_exp2f(s4[i] - L4[i]);  // rows past Np carry L = 1e30: P = 0
        pf[i] = (__bf16)p;
        dsf[i] = (__bf16)(p * (dp4[i] - D4[i]));
      }
#pragma unroll
      for (int db = 0; db < 4; db++) {
        adv4[db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(dotr[db], __builtin_bit_cast(s16x4, pf), adv4[db], 0, 0, 0);
        adk4[db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qbtr[db], __builtin_bit_cast(s16x4, dsf), adk4[db], 0, 0, 0);
      }
    }
    __syncthreads();  // ring -> staging: per wave dk block [32 rows][64 fp32] (store_rows_qknorm layout) at +0, dv block [16][64] at +8192
    if (!kval) {
#pragma unroll
      for (int db = 0; db < 4; db++) { adv4[db] = (f32x4){0.f, 0.f, 0.f, 0.f}; adk4[db] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    }
#pragma unroll
    for (int db = 0; db < 4; db++) {
      const int c = 4 * db + g;
      *reinterpret_cast<float4*>(smem + wave * 12288 + ki * 256 + ((c ^ ki) << 4)) =
          make_float4(adk4[db][0] * scale, adk4[db][1] * scale, adk4[db][2] * scale, adk4[db][3] * scale);
      *reinterpret_cast<float4*>(smem + wave * 12288 + 8192 + ki * 256 + (c << 4)) =
          make_float4(adv4[db][0], adv4[db][1], adv4[db][2], adv4[db][3]);
    }
    __syncthreads();
    {
      const int row = tid >> 4, c = tid & 15;
      const int off = row * 256 + ((c ^ row) << 4), offv = 8192 + row * 256 + (c << 4);
      float4 t0 = *reinterpret_cast<const float4*>(smem + off), v0 = *reinterpret_cast<const float4*>(smem + offv);
#pragma unroll
      for (int w = 1; w < 4; w++) {
        const float4 t = *reinterpret_cast<const float4*>(smem + w * 12288 + off);
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 12288 + offv);
        t0.x += t.x; t0.y += t.y; t0.z += t.z; t0.w += t.w;
        v0.x += v.x; v0.y += v.y; v0.z += v.z; v0.w += v.w;
      }
      __syncthreads();
      *reinterpret_cast<float4*>(smem + off) = t0;
      if (row < R)
        *reinterpret_cast<uint2*>(dv + ((long)b * Np + kb0 + row) * dv_ld + h * 64 + c * 4) =
            make_uint2(pack_bf16x2(v0.x, v0.y), pack_bf16x2(v0.z, v0.w));
    }
    __syncthreads();
    if (fk.dqkv) {
      f32x16 dummy[2];
      store_rows_qknorm(smem, reinterpret_cast<float*>(smem + 4 * 12288), dummy, 0.f, fk, wave == 0, b, h, H, co.tile, (Np + 127) >> 7,
                        kb0, Np, lane, wave, true);
    } else if (wave == 0) {
#pragma unroll
      for (int it = 0; it < 4; it++) {
        const int row = it * 4 + (lane >> 4), ch = lane & 15;
        if (kb0 + row < Np)
          *reinterpret_cast<float4*>(dk + bh * Np * 64 + (long)(kb0 + row) * 64 + ch * 4) =
              *reinterpret_cast<const float4*>(smem + row * 256 + ((ch ^ row) << 4));
      }
    }
    ATTN_TRACE_END(2);
    return;
  }
#endif
