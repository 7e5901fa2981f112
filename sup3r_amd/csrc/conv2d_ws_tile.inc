// One tile of conv2d_ws_kernel (kernels_conv2d_ws.hip), included twice:
//   WS_HAS_NEXT 1 — inside the loop over all but the last tile of the workgroup:
//                   prefetch of the next halo, taps, hand-over, epilogue;
//   WS_HAS_NEXT 0 — the last tile: taps and epilogue only.
// Two straight-line copies instead of `if (has_next)` around the prefetch and
// the hand-over, and an epilogue whose arithmetic is unconditional (only the
// stores are predicated), for the sake of the compiler's s_waitcnt placement:
// with the conditional forms it could not prove at the top of the loop that
// the previous tile's prefetch / skip registers had been consumed, and put
// vmcnt waits in front of the new prefetch — i.e. every tile first waited for
// the previous tile's output stores to drain (3 us of a 10 us tile), and a
// conv with a skip operand waited for the prefetch itself before its taps.
{
#if WS_HAS_NEXT
  if (!(g.dbg & 1)) {
    WS_FETCH(t_cur + 1);
    WS_EFETCH(t_cur + 1);
  }
#endif
  int i0, r0, c0;
  tile_org(t_cur, i0, r0, c0);
  const int im = i0 + w_img, c = c0 + frow;
  const bool pos_ok = im < g.N && c < Wo && !(g.dbg & 4);
  // (clamped twins: every address below is legal, ragged positions are masked at the store)
  const int imc = im > g.N - 1 ? g.N - 1 : im, cc = c > Wo - 1 ? Wo - 1 : c;
  const unsigned long long tbase = (unsigned long long)imc * IS + (unsigned long long)((unsigned)cc * CS);
  // this tile's skip rows (d2s == 1).  Last tile: fetched here, under the taps.
  // Other tiles: fetched AFTER the tap loop, under the hand-over — next to the
  // 44 prefetch registers and the double-buffered fragments their 32 registers
  // do not fit (4 - 10 spilled, and a spill of an in-flight load is a wait).
  uint4 rr[4][2];
#if !WS_HAS_NEXT
  if constexpr (NF == 4 && RES) {
    // (the skip tensor has the output's layout: d2s == 1, no frame)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      int r = r0 + w_row + m;
      r = r > Ho - 1 ? Ho - 1 : r;
      const unsigned long long ridx = tbase + (unsigned long long)(unsigned)r * RS;
#pragma unroll
      for (int h = 0; h < 2; ++h) rr[m][h] = *reinterpret_cast<const uint4*>(res + ridx + off_h[h]);
    }
  }
#endif

  f32x4 acc[4][NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int cb = NF == 1 ? kq * 4 : (nf >> 1) * 32 + kq * 8 + (nf & 1) * 4;
    const f32x4 b4 = {bl[cb], bl[cb + 1], bl[cb + 2], bl[cb + 3]};
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m][nf] = b4;
  }
  // (tried: (tc, k-step) outermost with the six halo rows m + tb read once
  // and shared by the three taps — 18 instead of 24 fragment reads per 48
  // MFMAs, but 32 spilled registers: 519 instead of 899 TFLOP/s at 512 x 64 x 64)
#pragma unroll 1
  for (int tb = 0; tb < ((g.dbg & 2) ? 0 : 3); ++tb) {
#pragma unroll
    for (int tc = 0; tc < 3; ++tc) {
      const int tap = tb * 3 + tc;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 wf[NF], pf[4];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          wf[nf] = *reinterpret_cast<const bf16x8*>(smem + f_addr[ks] + nf * 2048 + tap * 8192);
#pragma unroll
        for (int m = 0; m < 4; ++m)
          pf[m] = *reinterpret_cast<const bf16x8*>(smem + p_addr[tc][ks] + (m + tb) * WH_C * 128);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            acc[m][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nf], pf[m], acc[m][nf], 0, 0, 0);
      }
    }
  }

  if constexpr (EXO) {
    // the exogenous channel's taps: lane (column frow, channel groups kq 8 ..
    // and 32 + kq 8 ..) x rows m, straight into the accumulators
    const float* E = reinterpret_cast<const float*>(smem + W_EXO_OFF);
    const float* WE = reinterpret_cast<const float*>(smem + W_WE_OFF);
#pragma unroll 1
    for (int tb = 0; tb < 3; ++tb) {
#pragma unroll
      for (int tc = 0; tc < 3; ++tc) {
        const float* wt = WE + (tb * 3 + tc) * 64 + kq * 8;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt), w1 = *reinterpret_cast<const f32x4*>(wt + 4);
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(wt + 32), w3 = *reinterpret_cast<const f32x4*>(wt + 36);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float ev = E[(w_img * WH_R + w_row + m + tb) * WH_C + frow + tc];
          acc[m][0] += w0 * ev; acc[m][1 % NF] += w1 * ev;
          acc[m][2 % NF] += w2 * ev; acc[m][3 % NF] += w3 * ev;
        }
      }
    }
  }

#if WS_HAS_NEXT
  if constexpr (NF == 4 && RES) {
    // (the skip tensor has the output's layout: d2s == 1, no frame)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      int r = r0 + w_row + m;
      r = r > Ho - 1 ? Ho - 1 : r;
      const unsigned long long ridx = tbase + (unsigned long long)(unsigned)r * RS;
#pragma unroll
      for (int h = 0; h < 2; ++h) rr[m][h] = *reinterpret_cast<const uint4*>(res + ridx + off_h[h]);
    }
  }
  // ---- halo hand-over BEFORE the epilogue, behind raw barriers.  The wait for
  // the prefetched loads is a vmcnt wait and on gfx9 stores count in vmcnt too
  // (as does the vmcnt(0) inside __syncthreads()): in this order the loads have
  // had the whole tap loop to arrive and the output stores are issued after the
  // hand-over, free to drain under the next tile's taps.  Only LDS is handed
  // over: every wave's fragment reads are back (lgkmcnt) before the first
  // barrier, the ds_writes of the new halo before the second.
  // Measured (tools/dbg/ws_scaling.py, option MFMA_DBG ablations, 16 tiles per
  // CU, before the straight-line form): read-only 3.8 us per tile (5.5 TB/s),
  // write-only 3.3 us (5.0 TB/s), tap loop 3.0 us, everything 10.4 - 10.7 us —
  // the sum, because of the waits described at the top of this file.
  WG_BARRIER_LDS();
  WS_COMMIT();
  WS_ECOMMIT();
  WG_BARRIER_LDS();
#endif

  // ---- epilogue from registers: lane (position column frow, channel
  // group kq): rows m, halves h -> 8 consecutive channels, one 16-B store
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int r = r0 + w_row + m;
    const bool row_ok = pos_ok && r < Ho;
    const int rc = r > Ho - 1 ? Ho - 1 : r;
    if constexpr (NF == 1) {
      // lane (column frow, kq): channels 4 kq .. 4 kq + 3 of C_out <= 16, fp32
      float* yo = reinterpret_cast<float*>(yv) + (((size_t)imc * g.H + rc) * g.W + cc) * g.Cout;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = kq * 4 + e;
        const float v = acc[m][0][e];
        if (row_ok && co < g.Cout) yo[co] = v > 0.f ? v : slope * v;
      }
      continue;
    }
#pragma unroll
    for (int h = 0; h < (NF == 4 ? 2 : 0); ++h) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = acc[m][(2 * h) % NF][e]; v[4 + e] = acc[m][(2 * h + 1) % NF][e]; }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // max(v, slope v): identity (slope 1), ReLU (0) or LeakyReLU (0 <= alpha <= 1, checked by
        // conv2d_ws_geom_ok) — the same bits as v > 0 ? v : slope v, one instruction less per value
        // (v_max_f32 by hand: fmaxf() canonicalises its operands first)
        const float sa = slope * v[e];
        asm("v_max_f32 %0, %1, %2" : "=v"(v[e]) : "v"(v[e]), "v"(sa));
      }
      const unsigned long long dst = tbase + (unsigned long long)(unsigned)rc * RS + off_h[h];
      if constexpr (RES) {
        const uint4 q4 = rr[m][h];
        v[0] += bf_lo(q4.x); v[1] += bf_hi(q4.x); v[2] += bf_lo(q4.y); v[3] += bf_hi(q4.y);
        v[4] += bf_lo(q4.z); v[5] += bf_hi(q4.z); v[6] += bf_lo(q4.w); v[7] += bf_hi(q4.w);
      }
      if (res2) {
        // (d2s == 1; the sum of the first skip is rounded to bf16 first, as
        // the separate add of two bf16 tensors saw it)
        uint4 o1;
        o1.x = pk2(v[0], v[1]); o1.y = pk2(v[2], v[3]); o1.z = pk2(v[4], v[5]); o1.w = pk2(v[6], v[7]);
        const uint4 q4 = *reinterpret_cast<const uint4*>(res2 + dst);
        v[0] = bf_lo(o1.x) + bf_lo(q4.x); v[1] = bf_hi(o1.x) + bf_hi(q4.x);
        v[2] = bf_lo(o1.y) + bf_lo(q4.y); v[3] = bf_hi(o1.y) + bf_hi(q4.y);
        v[4] = bf_lo(o1.z) + bf_lo(q4.z); v[5] = bf_hi(o1.z) + bf_hi(q4.z);
        v[6] = bf_lo(o1.w) + bf_lo(q4.w); v[7] = bf_hi(o1.w) + bf_hi(q4.w);
      }
      uint4 o;
      o.x = pk2(v[0], v[1]); o.y = pk2(v[2], v[3]); o.z = pk2(v[4], v[5]); o.w = pk2(v[6], v[7]);
      if (row_ok && ch_ok[h]) *reinterpret_cast<uint4*>(y + dst) = o;
    }
  }
}
