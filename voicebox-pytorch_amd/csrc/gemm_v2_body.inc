// Body of one gemm_kernel_v2 tile (included inside a kernel, not a header): expects the template parameters MA, MB, Epi, F16,
// BM_, the objects `p` (GemmParams), `epi`, `smem`, and the macros VBX_BX_ (block id within the GEMM), VBX_T_ (its tile count)
// and VBX_SPLIT_ (its K split).  gemm_kernel_v2 defines them as blockIdx.x / gridDim.x / blockIdx.y -- the token stream of that
// kernel is unchanged -- and gemm_kernel_v2_grouped takes them from a job table.
  constexpr int WM = BM_ / 64, NT_ = (WM == 2) ? 4 : 2;
  constexpr int DMAS = BM_ / 64 + 2;  // LDS-DMA instructions per thread per stage
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (WM == 2) ? (wave >> 1) : 0, wn = (WM == 2) ? (wave & 1) : wave;
  const int T = VBX_T_, xcd = VBX_BX_ & 7, qi = VBX_BX_ >> 3;
  const int q = T >> 3, r = T & 7;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + qi;
  const int tiles_n = T / p.tiles_m;
  const int tm = lin / tiles_n, tn = lin - tm * tiles_n;
  const int m0 = tm * BM_, n0 = tn * BN;
  const int split = VBX_SPLIT_;
  const int kbeg = split * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const int nt = (kend - kbeg + BK2 - 1) / BK2;

  DmaPlan<MA, BM_> da;
  DmaPlan<MB, 128> db;
  da.init(p.A, p.lda, m0, p.M, tid);
  db.init(p.B, p.ldb, n0, p.N, tid);
  FragPlan<MA> fa;
  FragPlan<MB> fb;
  fa.init(smem, wm * 64, lane);
  fb.init(smem, wn * NT_ * 16, lane);

  f32x4 acc[4][NT_];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < NT_; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < NST - 1; s++) {
    if (s < nt) {
      da.issue(smem + s * STAGE_BYTES, kbeg + s * BK2, kend, tid);
      db.issue(smem + s * STAGE_BYTES + OP_BYTES, kbeg + s * BK2, kend, tid);
    }
  }

  // one k-tile; STG (the ring slot of tile t) is a compile-time constant so every LDS offset is an immediate
  auto step = [&](auto stg_c, int t) {
    constexpr int STG = decltype(stg_c)::value;
    constexpr int NXT = (STG + NST - 1) % NST;  // slot of tile t-1 == slot tile t+NST-1 will use
    // this thread's DMAs of tile t have landed once at most NST-2 younger stages (DMAS instructions each) are pending
    if (nt - 1 - t >= NST - 2) {
      if (DMAS == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();  // tile t visible to all waves; everyone is done reading tile t-1
    bf16x8 af[4], bfr[4];
    s16x4 alo[4], ahi[4], blo[4], bhi[4];
    fa.template read<STG * STAGE_BYTES, 0>(af[0], alo[0], ahi[0]);
    fa.template read<STG * STAGE_BYTES, 1>(af[1], alo[1], ahi[1]);
    fa.template read<STG * STAGE_BYTES, 2>(af[2], alo[2], ahi[2]);
    fa.template read<STG * STAGE_BYTES, 3>(af[3], alo[3], ahi[3]);
    fb.template read<STG * STAGE_BYTES + OP_BYTES, 0>(bfr[0], blo[0], bhi[0]);
    fb.template read<STG * STAGE_BYTES + OP_BYTES, 1>(bfr[1], blo[1], bhi[1]);
    if (NT_ == 4) {
      fb.template read<STG * STAGE_BYTES + OP_BYTES, 2>(bfr[2], blo[2], bhi[2]);
      fb.template read<STG * STAGE_BYTES + OP_BYTES, 3>(bfr[3], blo[3], bhi[3]);
    }
    // the DMAs of tile t+NST-1 (into the slot tile t-1 used) go out BEHIND the fragment reads: the LDS round trip then runs under
    // their issue time (back to back 1-3 % faster on the model's shapes than in front of them, neutral in the train step; the arm
    // that issued them in front was removed, docs/history.md)
    if (t + NST - 1 < nt) {
      da.issue(smem + NXT * STAGE_BYTES, kbeg + (t + NST - 1) * BK2, kend, tid);
      db.issue(smem + NXT * STAGE_BYTES + OP_BYTES, kbeg + (t + NST - 1) * BK2, kend, tid);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (MA == 1) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
        s16x8 v = {alo[s][0], alo[s][1], alo[s][2], alo[s][3], ahi[s][0], ahi[s][1], ahi[s][2], ahi[s][3]};
        af[s] = __builtin_bit_cast(bf16x8, v);
      }
    }
    if (MB == 1) {
#pragma unroll
      for (int s = 0; s < NT_; s++) {
        s16x8 v = {blo[s][0], blo[s][1], blo[s][2], blo[s][3], bhi[s][0], bhi[s][1], bhi[s][2], bhi[s][3]};
        bfr[s] = __builtin_bit_cast(bf16x8, v);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < NT_; j++) acc[i][j] = mfma16<F16>(af[i], bfr[j], acc[i][j]);
  };
  static_assert(NST == 3, "the k-loop below is unrolled for a 3-slot ring");
  for (int t = 0; t < nt; t += 3) {
    step(std::integral_constant<int, 0>{}, t);
    if (t + 1 < nt) step(std::integral_constant<int, 1>{}, t + 1);
    if (t + 2 < nt) step(std::integral_constant<int, 2>{}, t + 2);
  }
  // ---- epilogue: the fp32 C tile goes through LDS in 64-row halves (keeps the footprint at 48 KiB)
#ifdef GEMM2_TRACE_MARK
  GEMM2_TRACE_MARK();
#endif
  float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int h = 0; h < WM; h++) {
    __syncthreads();  // ring (h = 0) / previous half (h = 1) no longer read
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NT_; j++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int row = i * 16 + (lane >> 4) * 4 + rr;
            const int col = wn * NT_ * 16 + j * 16 + (lane & 15);
            Cs[row * CS_LD + col] = acc[i][j][rr];
          }
    }
    __syncthreads();
    epi(Cs, m0 + h * 64, n0, tid, split, p.M, p.N, 64);
  }
