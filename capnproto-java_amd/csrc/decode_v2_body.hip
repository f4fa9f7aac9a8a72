// decode_v2_body.hip -- the text of the record-index decoder's kernels, from
// the LUT to the last piece: included inside decode2_kernel (decode_v2.hip,
// whose header describes it) and inside decode2_at_kernel (decode_at.hip), so
// the two are one text and neither is a call into the other.  The including
// kernel declares smem, its parameters (packed, in_off, swo, n, out, status,
// ticket, avail, sd) and the constants kStream and kAt (DecPieces'), and
// defines CPK_DECODE_V2_BODY around the #include: nothing else may include it.
#ifndef CPK_DECODE_V2_BODY
#error "decode_v2_body.hip is the body of decode2_kernel and decode2_at_kernel: include it only inside them"
#endif
  uint64_t *lut = reinterpret_cast<uint64_t *>(smem);
  const int lane = lane_id(), w = wave_id();
  uint8_t *wl = smem + 2048 + w * kD2WaveLds;
  uint8_t *wbuf = wl;                                            // window bytes
  uint32_t *info = reinterpret_cast<uint32_t *>(wl + kD2WinBuf); // [kD2NI] record index
  uint32_t *bits = reinterpret_cast<uint32_t *>(wl + kD2WinBuf + kD2Info);  // record starts of a round
  VisMask *visa = reinterpret_cast<VisMask *>(info);  // [64], over the index (phases 1-3)
  if (sd.skip && __builtin_amdgcn_readfirstlane(*sd.skip)) return;
  fill_luts(lut, true);
  __syncthreads();  // the only block-wide barrier: LUT ready
  DecPieces<kStream, kAt> pc(swo, in_off, status, ticket, n, avail, sd);
  WPH_INIT

  while (pc.next()) {
    const int W = pc.W;
    const uint64_t a = pc.a;
    const uint32_t P = pc.P, glim = pc.glim;
    const uint8_t *gp = packed + a;
    uint64_t *dst = out + pc.w0;
    int st = W == 0 ? pc.empty_status() : CPK_OK;
    uint32_t e = 0;  // true tag position (piece-relative)
    int ow = 0;      // output words produced
    while (W != 0) {
      e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);  // (wave-uniform: SGPRs, scalar branches)
      ow = __builtin_amdgcn_readfirstlane(ow);
      if (e >= P) {
        if (ow < W) st = CPK_ETRUNC;  // ArrayInputStream EOF -> DecodeException
        break;
      }
      if (ow >= W) break;  // (trailing input is flagged by the record check)
      const uint32_t wend = min(e + kD2Win, P);
      WPH(0)
      const WinBytes wb = win_load<D2Geom>(wbuf, lane, gp, a, e, P);
      const uint8_t *pkw = wb.pkw;
      const uint32_t lend = wb.lend, ph = wb.ph;

      WPH(1)
      // ---- 1-4: the walks, the true chain, each lane's words and records -----
      const WinWalk ww = win_walks<!kStream, D2Geom, true>(pkw, visa, lane, e, wend DEC_PH_ARGS);
      const WinChain wc = win_chain<!kStream, D2Geom, true>(pkw, visa, lane, e, wend, ww DEC_PH_ARGS);
      const uint32_t S = ww.S, entry = wc.entry, enext = wc.enext;
      const bool on = wc.on;
      const int T = wc.T, o0 = wc.o0, NR = wc.NR, r0 = wc.r0;
      // ---- 5: the index: each true record's window position and first word ----
      // (the reference's error checks run in a window that may reach the
      // piece's end: PackedInputStream.java:53-138)
      const bool chk = (ow + T >= W) || (P - e < kD2ChkReach);
      // a window with more true records than the index holds ends at its
      // kD2NI-th record (scr: that record's position and first word)
      const bool cut = NR > (int)kD2NI;
      int err = 0x7fffffff;
      uint32_t fin = 0;  // end of the record that fills the piece (if any)
      uint32_t cutq = 0, cuto = 0;
      if (on) {
        int o = o0, rk = r0;
        for (uint32_t q = entry; q < S;) {
          const uint32_t tag = pkw[q], c1 = pkw[q + 1], c9 = pkw[q + 9];
          const uint32_t ntag = 1 + __builtin_popcount(tag);
          const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
          const int nw = 1 + (int)((zm & c1) + (fm & c9));
          const uint32_t adv = ntag + (zm & 1u) + (fm & (8u * c9 + 1u));
          if (rk >= (int)kD2NI) {
            if (rk == (int)kD2NI) {
              cutq = q;
              cuto = (uint32_t)o;
            }
            break;
          }
          const int oo = ow + o;
          if (chk && oo < W && err == 0x7fffffff) {
            // truncated tag bytes / count / literal run -> EOF DecodeException;
            // a run past the piece -> DecodeException / BufferOverflowException
            int code = 0;
            if (q + ntag > P) code = 2;
            else if (tag == 0 || tag == 0xffu) {
              if (q + (tag ? 10u : 2u) > P) code = 2;
              else if (oo + nw > W) code = 3;
              else if (q + adv > P) code = 2;
            }
            if (!kStream && !code && oo + nw == W && q + adv < P) code = 4;
            if (code) err = (int)(((q - e) << 3) | (uint32_t)code);  // window-relative
            if (oo + nw == W) fin = q + adv;
          }
          info[rk] = (q - e) | ((uint32_t)o << 12);
          ++rk;
          o += nw;
          q += adv;
        }
      }
      err = __builtin_amdgcn_readfirstlane(wave_min(err));
      if (err != 0x7fffffff) {
        st = -(err & 7);
        // (kAt: a piece full before its range ends says where -- the lane that
        // checked the filling record holds its end; written here, so nothing
        // more is live across the window loop)
        if constexpr (kAt && !kStream)
          if (st == CPK_ETRAILING) in_off[3 * (uint64_t)pc.seg + 2] = a + wave_max_u(fin);
        break;
      }
      fin = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u(fin));
      uint32_t Teff = (uint32_t)T, eff_next = enext;
      int NRe = NR;
      if (cut) {
        Teff = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u(cuto));
        eff_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u(cutq));
        NRe = (int)kD2NI;
      }
      wave_lds_order();
      WPH(5)
      // ---- 6: expansion, rounds of kD2Round words, lane = word ----
      const uint32_t Tlim = min(Teff, (uint32_t)(W - ow));
      uint64_t *dst_w = dst + ow;
      uint32_t ia = 0;  // the record covering the round's first word
      // two copies of the expansion: one for windows whose records all lie in
      // the loaded bytes (eff_next + 12 <= lend), with unchecked reads
      auto expand = [&](auto allin) __attribute__((always_inline)) {
      constexpr bool kAllIn = decltype(allin)::value;
      for (uint32_t rb = 0; rb < Tlim; rb += kD2Round) {
        const uint32_t re = min(rb + kD2Round, Tlim);
        // the round's record starts after its first word
        for (uint32_t i = (uint32_t)lane; i < kD2Bits / 16; i += 64)
          reinterpret_cast<uint4 *>(bits)[i] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_order();
        uint32_t ib = ia + 1;
        for (;;) {
          const uint32_t i = ib + (uint32_t)lane;
          const uint32_t oi = i < (uint32_t)NRe ? (info[i] >> 12) : 0xffffffffu;
          const bool in = oi < rb + kD2Round;
          if (in) atomicOr(&bits[(oi - rb) >> 5], 1u << ((oi - rb) & 31));
          const uint64_t outm = __ballot(!in);
          if (outm) {
            ib += (uint32_t)__builtin_ctzll(outm);
            break;
          }
          ib += 64;
        }
        wave_lds_order();
        // kD2Unroll groups of 64 words at a time: their LDS read chains
        // (start map -> index -> tag -> bytes) are independent and overlap
        uint32_t cum = 0;
        for (uint32_t gb = rb; gb < re; gb += 64 * kD2Unroll) {
          uint64_t bm[kD2Unroll];
#pragma unroll
          for (int u = 0; u < kD2Unroll; ++u) {
            const uint32_t g0 = gb + 64 * u;
            const uint32_t gi = (g0 - rb) >> 5;  // (even; past the round: zero bits)
            bm[u] = g0 < rb + kD2Round ? ((uint64_t)bits[gi] | ((uint64_t)bits[gi + 1] << 32)) : 0ull;
          }
          const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1);
#pragma unroll
          for (int u = 0; u < kD2Unroll; ++u) {
            const uint32_t g0 = gb + 64 * u;
            const uint32_t rec = ia + cum + (uint32_t)__builtin_popcountll(bm[u] & le);
            cum += (uint32_t)__builtin_popcountll(bm[u]);
            const uint32_t wv = g0 + (uint32_t)lane;
            const uint32_t inf = info[min(rec, kD2NI - 1)];
            const uint32_t q = e + (inf & 0xfffu);
            const uint32_t ofs = wv - (inf >> 12);
            const uint32_t tag = pkw[q];
            uint32_t x0 = 0, x1 = 0;
            // 64 words of zero runs (the mostly-zero batches this form takes)
            // have no bytes to read: the group skips the reads and the LUT
            // (round 6: config 4 decode -1.0 %)
            if (__ballot(tag != 0u)) {
              // the word's bytes: after the tag, or the literal run's ofs-th word
              const uint32_t src = q + 1 + ((tag == 0xffu && ofs) ? 1u + 8u * ofs : 0u);
              const uint64_t raw = read8<kAllIn>(pkw, src, lend, gp, glim, ph, e);
              const uint64_t sel = lut[tag];
              const uint32_t rl = (uint32_t)raw, rh = (uint32_t)(raw >> 32);
              x0 = __builtin_amdgcn_perm(rh, rl, (uint32_t)sel);
              x1 = __builtin_amdgcn_perm(rh, rl, (uint32_t)(sel >> 32));
            }
            // (nontemporal: plain stores wrote 5 % fewer bytes and took 1.7 % longer)
            if (wv < re) __builtin_nontemporal_store((uint64_t)x0 | ((uint64_t)x1 << 32), &dst_w[wv]);
          }
        }
        // the record covering the next round's first word
        const uint32_t ob = ib < (uint32_t)NRe ? (info[ib] >> 12) : 0xffffffffu;
        ia = ob == rb + kD2Round ? ib : ib - 1;
        wave_lds_order();  // bits / info reused
      }
      };
      if (eff_next + 12 <= lend) expand(std::true_type{});
      else
        expand(std::false_type{});
      WPH(6)
      if (ow + (int)Teff >= W && fin) {  // the piece is full: next piece starts at fin
        ow = W;
        e = fin;
        break;
      }
      ow += (int)Teff;
      e = eff_next;
    }
    pc.done(st, e);
  }
  WPH_FLUSH(16)
