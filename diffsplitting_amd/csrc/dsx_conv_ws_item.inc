// Body of one (tile, group) item of k_conv_ws's compute waves: the MFMA steps of the group and, at the end of a tile,
// the epilogue.  Included twice by dsx_conv_ws.hip: in the plain item loop (ring no deeper than a group) and in the loop
// unrolled over the ring phases of a ring that spans several groups (1 x 1 convs).  Expects `v` (item), `R0` (first
// ring slot of the item, constexpr) and DSX_WS_ITEM_NEXT (continue / return) from the including scope.  The plain
// form must stay a literal loop body: wrapped in a lambda, the two-N-block variants run into hipcc's failing spill
// path ("Illegal instruction detected: Operand has incorrect register class", ROCm 7.2).
    unsigned aaddr[MB][AD];                   // LDS byte address of the fragment rows (direct: chunks) in this item's image
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int dy = 0; dy < AD; ++dy) aaddr[mb][dy] = lds0 + ibuf * BUFB + abase[mb][dy];
    if constexpr (NBUF >= 3) lds_wait_all_ge(full_addr, v + 1, a.handoff_timeouts);   // every loader wave has finished this item's image
    f32x4_t fb[PFF + 1];                       // ring of pixel fragments: fragment k of the item lives in fb[k % (PFF + 1)]
    auto read_frag = [&](auto kc_) __attribute__((always_inline)) {
      constexpr int k = decltype(kc_)::value;
      constexpr int t = k / NF, mb = (k % NF) >> 1, ph = k & 1;
      constexpr int cg = t / TAPS, tap = t % TAPS, dy = tap / KS, dx = tap % KS;
      constexpr int imm = DIRECT ? 0 : dx * PIXB + cg * 64;   // (direct: the chunk is in the base address, ai = cg)
      constexpr int ai = DIRECT ? cg : dy;
      static_assert(imm < 65536, "ds offset field");
#ifndef DSX_ABL_L   // -DDSX_ABL_L: timing experiment, LDS operand reads off (results wrong)
      lds_read_frag<imm>(fb[k % (PFF + 1)], ph ? aaddr[mb][ai] + (unsigned)a16 : aaddr[mb][ai]);
#else
      touch_frag(fb[k % (PFF + 1)], aaddr[mb][ai]);
#endif
    };
    static_for<PFF>(read_frag);
    static_for<NPAIR>([&](auto tc_) {
      constexpr int t = decltype(tc_)::value;
      constexpr int s0 = (R0 + 2 * t) % D, s1 = (R0 + 2 * t + 1) % D;
      const WFrag w0 = bq[s0], w1 = bq[s1];
#ifndef DSX_ABL_W   // -DDSX_ABL_W: timing experiment, weight stream off (results wrong)
      bq[s0] = load_b(std::integral_constant<int, 0>{});
      bq[s1] = load_b(std::integral_constant<int, 1>{});
#endif
      static_for<NF>([&](auto fc_) __attribute__((always_inline)) {
        constexpr int f = decltype(fc_)::value, k = t * NF + f;
        constexpr int mb = f >> 1, ph = f & 1;
        if constexpr (k + PFF < FT) read_frag(std::integral_constant<int, k + PFF>{});
        constexpr int ahead = FT - 1 - k < PFF ? FT - 1 - k : PFF;   // younger reads that may stay in flight
        wait_frags<ahead>(fb[k % (PFF + 1)]);
        const f32x4_t px = fb[k % (PFF + 1)];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          // accumulator quarters of the f32x16: registers 8 ph + 4 ch + j (see mfma16_step)
          f32x4_t q0 = {acc[mb][nb][8 * ph], acc[mb][nb][8 * ph + 1], acc[mb][nb][8 * ph + 2], acc[mb][nb][8 * ph + 3]};
          f32x4_t q1 = {acc[mb][nb][8 * ph + 4], acc[mb][nb][8 * ph + 5], acc[mb][nb][8 * ph + 6], acc[mb][nb][8 * ph + 7]};
          q0 = mfma16_step<DT>(w0.v[nb], px, q0);
          q1 = mfma16_step<DT>(w1.v[nb], px, q1);
#pragma unroll
          for (int j = 0; j < 4; ++j) { acc[mb][nb][8 * ph + j] = q0[j]; acc[mb][nb][8 * ph + 4 + j] = q1[j]; }
        }
      });
    });
    DSX_STAMP_T(1 + 3 * v, tid == 0 && v < 20);
    if constexpr (NBUF == 2) ws_barrier();   // the loaders may now overwrite this image; the next one is complete
    else lds_signal(full_addr + 16, wave, v + 1);   // FREE: this wave is done with items 0 .. v (its operand reads have returned)
    if (++ibuf == NIMG) ibuf = 0;
    DSX_STAMP_T(2 + 3 * v, tid == 0 && v < 20);
    if (++g < G) DSX_WS_ITEM_NEXT;
    g = 0;

    // While the epilogue's vector work waits behind the prioritised loaders no MFMA runs on this SIMD: for the tile
    // shapes named by DSX_EPI_PRIO_COND the epilogue outranks them (the loaders get the SIMD back with the next group).
    if (DSX_EPI_PRIO_COND) __builtin_amdgcn_s_setprio(2);
    // ---- tile finished: epilogue (+ fused statistics).  Accumulator registers 8 ph + r of a lane are channels
    //      8 kq + r of the wave's 32-channel block, for the lane's pixel of the 16-pixel block ph (see mfma16_step).
    // scale/shift of tile ti+3 -> LDS slot (ti+3) % 3 == ti % 3, whose use ended with tile ti
    if (!DIRECT && a.gn_scale != nullptr && ti + 3 < ntile && tid * 4 < C) {
      float* dst = aff_base + (size_t)aslot * (AFFB / 4);
      *(float4*)(dst + tid * 4) = affv[0];
      *(float4*)(dst + C + tid * 4) = affv[1];
    }
    // conv -> + (bias | FiLM incl. bias) -> + residual.  Registers 8 ph .. 8 ph + 7 of a lane are channels
    // nbase + 32 nb .. + 7 of its pixel in the 16-pixel block ph of row block mb.
    const int rcur = PRE_RESID ? 0 : tile_pixel0(cur) * a.resid_ld;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
          float rs[8];
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            float t[CPU];
            uint4 rr = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (PRE_RESID) rr = residv[mb][nb][ph][q];
            else if (a.resid) rr = *(const uint4*)((const DT*)a.resid + (rcur + rrow[mb] + ph * r16) + 32 * nb + CPU * q);
            Unit<DT>::unpack(rr, t);
#pragma unroll
            for (int j = 0; j < CPU; ++j) rs[CPU * q + j] = t[j];
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {   // element pairs: v_pk_add_f32 (same additions in the same order as one by one)
            const float4 ta = addv[nb][j];
            const int r = 8 * ph + 4 * j;
            f32x2_t x0 = {acc[mb][nb][r + 0], acc[mb][nb][r + 1]}, x1 = {acc[mb][nb][r + 2], acc[mb][nb][r + 3]};
            const f32x2_t t0 = {ta.x, ta.y}, t1 = {ta.z, ta.w};
            const f32x2_t r0 = {rs[4 * j + 0], rs[4 * j + 1]}, r1 = {rs[4 * j + 2], rs[4 * j + 3]};
            x0 = (x0 + t0) + r0;
            x1 = (x1 + t1) + r1;
            acc[mb][nb][r + 0] = x0.x; acc[mb][nb][r + 1] = x0.y; acc[mb][nb][r + 2] = x1.x; acc[mb][nb][r + 3] = x1.y;
          }
        }
    DSX_STAMP_T(61, tid == 0 && ti == 1);
    // the operand registers are free again: fetch the next tile's (and the scale/shift of the tile three after it)
    const TilePos done = cur;
    ++ti;
    if (++aslot == 3) aslot = 0;
    cur = nxt; nxt = nn; nn = n3; tile_advance(n3);
    if (ti < ntile) prefetch_epilogue(cur, ti + 3 < ntile, n3.b);
    DSX_STAMP_T(125, tid == 0 && ti == 2);

    const int o0 = tile_pixel0(done) * a.out_ld;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float s1[8], s2[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
          float x[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) x[r] = acc[mb][nb][8 * ph + r];
          DSX_STAMP_T(114 + mb, tid == 0 && ti == 2 && nb == 0 && mb < 2 && ph == 0);
#ifndef DSX_ABL_EPI   // -DDSX_ABL_EPI: timing experiment, no output stores (results wrong)
          store8(a.out, (size_t)(o0 + orow[mb] + ph * o16 + 32 * nb), x, Kind<DT>::value);   // host: out is in the storage type
#endif
          DSX_STAMP_T(116 + mb, tid == 0 && ti == 2 && nb == 0 && mb < 2 && ph == 1);
#pragma unroll
          for (int r = 0; r < 8; r += 2) {   // v_pk_add_f32 / v_pk_fma_f32
            const f32x2_t xv = {x[r], x[r + 1]};
            f32x2_t a1 = {s1[r], s1[r + 1]}, a2 = {s2[r], s2[r + 1]};
            a1 = a1 + xv;
            a2 = xv * xv + a2;
            s1[r] = a1.x; s1[r + 1] = a1.y; s2[r] = a2.x; s2[r + 1] = a2.y;
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) acc[mb][nb][8 * ph + r] = 0.0f;
        }
      DSX_STAMP_T(126, tid == 0 && ti == 2 && nb == 0);
      if (do_stats) {
        // the 16 lanes of a DPP row (one kq) hold the same 8 channels for 16 pixel columns: lane c ends up with channel
        // row8_fold_reg(c) summed over the wave's 32 MB pixels
        const float w1 = row8_fold(s1, lane), w2 = row8_fold(s2, lane);
        const int chunk = (done.ty * a.tiles_x + done.tx) * WM + wm;
        const int nch = per_img * WM;
        const int n = nbase + 32 * nb + row8_fold_reg(c16);
        if (c16 < 8) {
          float* pp = a.stat_part + (((size_t)done.b * nch + chunk) * a.Cout + n) * 2;
          pp[0] = w1; pp[1] = w2;
        }
      }
      DSX_STAMP_T(127, tid == 0 && ti == 2 && nb == 0);
    }
    if (DSX_EPI_PRIO_COND) __builtin_amdgcn_s_setprio(0);
    DSX_STAMP_T(62, tid == 0 && ti == 2);
    DSX_STAMP_T(3 + 3 * v, tid == 0 && v < 20);
