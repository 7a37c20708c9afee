// Ragged tail role of attn_fwd_kernel_v3 (included inside attn_fwd_v3_body.inc): the workgroup's query tile holds R <= 16 rows.
// Wave w owns the 16-key block w of every 64-key tile; a lane owns query (lane & 15) and the keys 4 * (lane >> 4) .. + 3 of the block.
//   S^T[16 keys][16 q]   = K[16 keys][64 d] . Q^T          2 x v_mfma_f32_16x16x32_f16   (A: ds_read_b128 row fragments of the K tile)
//   O^T[64 d][16 q]     += V^T[64 d][16 keys] . P^T        4 x v_mfma_f32_16x16x16_f16   (A: ds_read_b64_tr_b16 of the V tile; B = the
//                                                                                        lane's four S^T values, already in place)
// The running maximum of a query is shared by the wave's four key groups (two shuffles per tile); the row sum stays per lane until
// the end.  The four waves' (m, l, O^T) meet in LDS and 256 threads write the R output rows.  Same ring / barrier / DMA schedule as
// the full tiles.  Reference semantics: attend.py:119-137 (masked keys -> -inf).  A fully masked row
// (l = 0) is written as zeros with lse 1e30 here; the reference's softmax is uniform there, which attn_empty_batch_kernel writes after.
{
  const int qi = lane & 15, g = lane >> 4;
  const int qb0 = co.tile * 128;
  const int R = Np - qb0;
  const int qrow = min(qb0 + qi, Np - 1);
  f16x8 qf2[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) qf2[ks] = *reinterpret_cast<const f16x8*>(q16 + (bh * Np + qrow) * 64 + 32 * ks + 8 * g);
  asm volatile("" ::"v"(qf2[0]), "v"(qf2[1]));
  unsigned ka2[2], va2[4];
  {
    const int krow = wave * 16 + qi;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) ka2[ks] = lds_addr32(smem + swz_off2(krow, 4 * ks + g));
    const int vrow = wave * 16 + 4 * g + (qi >> 2);
#pragma unroll
    for (int db = 0; db < 4; db++) {
      const int d = 16 * db + 4 * (qi & 3);
      va2[db] = lds_addr32(smem + TILE16 + swz_off2(vrow, d >> 3) + (d & 7) * 2);
    }
  }
  f32x4 o2[4];
#pragma unroll
  for (int db = 0; db < 4; db++) o2[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run = NEG_INF, l_part = 0.f;
  for (int kt = 0; kt < ntiles; kt++) {
    const unsigned so = (unsigned)((kt & 1) * ASTAGE);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < ntiles) dma_kv((unsigned)(((kt + 1) & 1) * ASTAGE), kt + 1);
    const f16x8 kf0 = asm_read_b128<0>(ka2[0] + so), kf1 = asm_read_b128<0>(ka2[1] + so);
    s16x4 vt[4];
#pragma unroll
    for (int db = 0; db < 4; db++) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(vt[db]) : "v"(va2[db] + so) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
    s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0, qf2[0], s4, 0, 0, 0);
    s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1, qf2[1], s4, 0, 0, 0);
    const int kg0 = kt * 64 + wave * 16 + 4 * g;
#ifdef VBX_FWD_LENS
#define VBX_KLIM kend  // vbx_attn_fwd_lens: keys stop at key_lens[b]
#else
#define VBX_KLIM Np
#endif
    if (mask != nullptr || kt * 64 + 64 > VBX_KLIM) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int kg = kg0 + i;
        bool ok = kg < VBX_KLIM;
#undef VBX_KLIM
        if (ok && mask) ok = mask[(long)b * Np + kg] != 0;
        if (!ok) s4[i] = NEG_INF;
      }
    }
    float mx = fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx * scale2);
    const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
    const float alpha = fast_exp2(m_run - m_use);
    float p[4];
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = fast_exp2(s4[i] * scale2 - m_use);
    l_part = l_part * alpha + ((p[0] + p[1]) + (p[2] + p[3]));
    m_run = m_new;
    typedef __attribute__((ext_vector_type(2))) __fp16 h2;
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const h2 pa = __builtin_amdgcn_cvt_pkrtz(p[0], p[1]), pb = __builtin_amdgcn_cvt_pkrtz(p[2], p[3]);
    const u32x2 pw = {__builtin_bit_cast(unsigned, pa), __builtin_bit_cast(unsigned, pb)};
    const f16x4 pf = __builtin_bit_cast(f16x4, pw);
#pragma unroll
    for (int db = 0; db < 4; db++) {
      o2[db] *= alpha;
      o2[db] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, vt[db]), pf, o2[db], 0, 0, 0);
    }
  }
  __syncthreads();  // the ring becomes staging space: [wave][16 q][64 d] fp32 partial O^T, then [wave][16 q][m, l]
  float l_w = l_part + __shfl_xor(l_part, 16, 64);
  l_w += __shfl_xor(l_w, 32, 64);
  float* po = reinterpret_cast<float*>(smem);
  float* pml = po + 4 * 1024;
#pragma unroll
  for (int db = 0; db < 4; db++)
    *reinterpret_cast<float4*>(po + wave * 1024 + qi * 64 + 16 * db + 4 * g) = make_float4(o2[db][0], o2[db][1], o2[db][2], o2[db][3]);
  if (g == 0) {
    pml[(wave * 16 + qi) * 2] = m_run;
    pml[(wave * 16 + qi) * 2 + 1] = l_w;
  }
  __syncthreads();
  {
    const int qq = tid >> 4, d4 = (tid & 15) * 4;
    float mw[4], lw[4], M = NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      mw[w] = pml[(w * 16 + qq) * 2];
      lw[w] = pml[(w * 16 + qq) * 2 + 1];
      M = fmaxf(M, mw[w]);
    }
    const float M_use = (M == NEG_INF) ? 0.f : M;
    float L = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const float f = fast_exp2(mw[w] - M_use);
      const float4 t = *reinterpret_cast<const float4*>(po + w * 1024 + qq * 64 + d4);
      L += f * lw[w];
      a0 += f * t.x; a1 += f * t.y; a2 += f * t.z; a3 += f * t.w;
    }
    const float inv = (L > 0.f) ? 1.0f / L : 0.f;
    if (qq < R) {
      const long row = (long)b * Np + qb0 + qq;
      const long go = row * (H * 64) + h * 64 + d4;
      *reinterpret_cast<uint2*>(out + go) = make_uint2(pack_f16x2(a0 * inv, a1 * inv), pack_f16x2(a2 * inv, a3 * inv));
      if (outb) *reinterpret_cast<uint2*>(outb + go) = make_uint2(pack_bf16x2(a0 * inv, a1 * inv), pack_bf16x2(a2 * inv, a3 * inv));
      if ((tid & 15) == 0) lse[bh * Np + qb0 + qq] = (L > 0.f) ? (M + log2f(L)) : 1e30f;
    }
  }
}
