// The software-pipelined reduction loop of gemm_body (gemm.cuh), included once per k-loop body: `ex` (std::true_type / std::false_type,
// declared by the including scope) selects the exact-bf16 body or the general six-term one in lstore / compute.
#pragma unroll
  for (int u = 0; u < PF; ++u) gload(tile_of(u), u);
  lstore(0, 0, ex);
  group_sync();
  SAST_TL(1);
  int i = 0;
  SAST_TLF_DECL
  for (; i + PF <= n_it; i += PF) {   // no exits inside the unrolled body: one straight-line block per PF phases
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      gload(tile_of(i + u + PF), u);
      SAST_PHASE_FENCE();
      SAST_TLF(0);
      compute(u & 1, ex);
      SAST_TLF(1);
      SAST_TLF_WAIT_OLDER(A_PER + B_PER);      // (instrumented builds: the wait for the tile loaded a phase ago, apart from its split + store)
      lstore((u + 1) & 1, (u + 1) % PF, ex);
      SAST_TLF(2);
      group_sync();
      SAST_TLF(3);
      SAST_TLF_COUNT();
    }
  }
  SAST_TLF_FLUSH();
  if constexpr (EARLY_AUX) {
    const int jc = min(j0 + wn * 32 + (lane & 31), NJ - 1), mb = m0 + wm * T::WTM + 4 * (lane >> 5);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) eaux[reg] = ep.pre(min(mb + (reg & 3) + 8 * (reg >> 2), Meff - 1), jc);
  }
  {   // remainder (< PF phases): everything it needs is already in registers
    const int rem = n_it - i;
#pragma unroll
    for (int u = 0; u < PF - 1; ++u) {
      if (u < rem) {
        compute(u & 1, ex);
        lstore((u + 1) & 1, (u + 1) % PF, ex);
        group_sync();
      }
    }
  }
