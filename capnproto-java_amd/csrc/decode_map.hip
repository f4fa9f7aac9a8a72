// decode_map.hip -- the block-map decoder (decode_kernel and its forms).
// Included from packed_codec.hip (namespace cpk) after decode_win.hip, whose
// walks and chain (1-4 below) it shares with the record-index decoder
// (decode_v2.hip); what is the block map's own is here.
//
// Wave-per-piece decoder.  Each wave owns one piece at a time and consumes
// its packed bytes in windows of 64 chunks starting at a known tag position e:
//   1. lane l walks its chunk [e + Cl, e + Cl + C) from the chunk start,
//      speculatively treating it as a tag; visited positions form a bit mask
//      per lane, and the walk tallies its output words;
//   2. from its exit, each lane walks on until it lands on a position its
//      owner visited (the two walks coincide from there: the tag chain is a
//      function of the position);
//   3. the lanes reachable from lane 0 (whose chunk starts at the true tag e)
//      under "lane -> owner of its landing point" hold every true record
//      (pointer doubling);
//   4. on-path lanes' word counts -> wave scan; they re-walk their true
//      records to check the reference's error conditions and mark, per
//      record, the 4-word output block its first word falls in (ds_max);
//      a prefix max hands every block its covering record; all 64 lanes then
//      gather-expand the blocks (PackedInputStream.java:82-134 per word).
// No barriers: up to 28 pieces in flight per CU.
constexpr int kDecThreads = 256;               // 4 independent waves
// workgroups per CU the register budget is sized for (= the LDS limit:
// 72 VGPRs; at 8 the stream form spilled, messages decode +10 %)
#ifndef CPK_DEC_WPE
#define CPK_DEC_WPE 7
#endif
constexpr int kDecWpe = CPK_DEC_WPE;
// (kDecChunk, kDecLook and the CPK_DEC_* defaults: packed_codec.hip, before the includes)
typedef WinGeom<kDecChunk, kDecLook> DecGeom;
constexpr uint32_t kWin = DecGeom::win, kWinBuf = DecGeom::buf, kDecChkReach = DecGeom::reach;
constexpr int kRound = CPK_DEC_ROUND;  // output words expanded per round
constexpr int kBlk = CPK_DEC_BLK;  // output words per expansion block
// the visited masks (phases 1-3) and the block map (phase 5) share LDS
constexpr uint32_t kDecWaveLds = kWinBuf + (4 * (kRound / kBlk) > 64 * sizeof(VisMask)
                                                ? 4 * (kRound / kBlk)
                                                : 64 * sizeof(VisMask));
// The block map: a record marks only the block whose span ends at or after
// its first word (ds_max of an entry ordered by output position), and a
// prefix max over the blocks hands every block the last record starting at
// or before its first word: one LDS op per record, no per-block loop
constexpr int kMapPer = kRound / kBlk / 64;  // map entries per lane in the fill
static_assert((kRound / kBlk == 64 * kMapPer && kWin <= 4096 && kRound + 256 < (1 << 19)),
              "max-map entry: 12-bit window position, 19-bit output position");
// Dense windows (few, long records: 0xFF runs) are walked by one lane
// (decode_body<.., kSerial>, the form picked for dense batches): taken when
// the previous window looked dense (over 5.3 packed bytes per word); a serial
// walk passing kDecSerMax records gives the window back to the parallel
// walks, which then keep the next kDecSerCool windows.
constexpr uint32_t kDecSerMax = CPK_DEC_SER_MAX, kDecSerCool = 32;
// LUT | 4 waves' windows and block maps | 4 waves' dense-form counters
constexpr uint32_t kDecCntOff = 2048 + 4 * kDecWaveLds;
// The dense form's window counters (cpk_ctx_dense_windows): compiled into
// the diagnostics build only (libcapnp_packed_hip_diag.so, build_native.py).
// Any code in the serial path changes the dense forms' register allocation
// (spills): with the counters, config-3 message decode +2 % (round 6,
// profiles/r6f_*).
#ifndef CPK_DEC_CNT
#define CPK_DEC_CNT 0
#endif
constexpr bool kDecCnt = CPK_DEC_CNT != 0;
constexpr uint32_t kDecLds = kDecCntOff + 32;  // 22,624 at 56-byte chunks

// 8 bytes at piece position x: from the LDS window when loaded, otherwise
// (tail of a literal run reaching past the window) straight from memory
// (kAllIn: the caller knows x + 12 <= lend -- every record of the window
// lies in the loaded bytes -- so no check and no memory path)
template <bool kAllIn = false, bool kLa = true>
__device__ __forceinline__ uint64_t read8(const uint8_t *pkw, uint32_t x, uint32_t lend,
                                         const uint8_t *gpiece, uint32_t glim, uint32_t ph,
                                         uint32_t e) {
  // The LDS read is unconditional (position clamped to the window start e,
  // which has 12 buffer bytes after it whatever the window's size): with
  // both reads under one branch hipcc merged them into flat loads.
  // LDS-aligned dwords: piece position x sits at byte phase (x + ph) & 3 of
  // the 16-byte aligned window buffer.
  const bool inw = kAllIn || x + 12 <= lend;
  const uint32_t xl = inw ? x : e;
  uint32_t sh, d0, d1, d2;
  if constexpr (kLa) {
    // from the LDS byte address itself: its low bits are the phase, its
    // aligned part the first dword (add, and, and; round 5: config-3
    // messages decode -1.2 %, the dense piece form +1.8 %: not there)
    typedef __attribute__((address_space(3))) const uint8_t lds_cu8;
    typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
    const uint32_t la = (uint32_t)(uintptr_t)((lds_cu8 *)pkw) + xl;
    sh = la & 3;
    lds_cu32 *pl = (lds_cu32 *)(uintptr_t)(la & ~3u);
    d0 = pl[0], d1 = pl[1], d2 = pl[2];
  } else {
    sh = (xl + ph) & 3;
    const uint32_t *pl = reinterpret_cast<const uint32_t *>(pkw + ((int64_t)xl - sh));  // (signed: xl < sh)
    d0 = pl[0], d1 = pl[1], d2 = pl[2];
  }
  if (!kAllIn && !inw) {
    // address-aligned dwords of the packed buffer, none at or past the
    // readable limit glim (piece-relative: the piece's end rounded up to a
    // 16-byte line; bytes there are never part of a valid record)
    sh = (uint32_t)(reinterpret_cast<uintptr_t>(gpiece + x) & 3);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(gpiece + ((int64_t)x - sh));  // (stays global)
    const int64_t xa = (int64_t)x - sh;  // piece position of p[0] (>= -3: the
    d0 = xa < glim ? p[0] : 0u;           // bytes before the piece are the buffer's)
    d1 = xa + 4 < glim ? p[1] : 0u;
    d2 = (sh && xa + 8 < glim) ? p[2] : 0u;
  }
  const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
  const uint32_t hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// ---- 5: error checks, block map, expansion (rounds of kRound words) of a
// window whose true records are known: an on-path lane holds the records
// [entry, S), the first at window word o0 (myw words); T words in all, the
// window's first record at piece position e, ow piece words before it
// (decode_body; decode_piece_mw).  Returns false when a record fails (st
// set); fin: the end of the record that fills the piece, else 0.
template <bool kStream, bool kLean = true>
__device__ __forceinline__ bool win_emit(const uint8_t *pkw, const uint64_t *lut, uint32_t *blk, int lane,
                                         uint32_t e, int ow, int W, uint32_t P, int T, bool on,
                                         uint32_t entry, uint32_t S, uint64_t onmask, int o0, int myw,
                                         uint32_t enext, uint32_t lend, const uint8_t *gp, uint32_t glim,
                                         uint32_t ph, uint64_t *dst, int &st, uint32_t &fin,
                                         bool premapped DEC_PH_PARAMS) {
  bool failed = false;
  fin = 0;
  // errors and the filling record can only occur in a window reaching the
  // piece's last word or within one window plus one record of its end
  // (the window's records start before e + kWin; the longest record, a
  // 0xFF tag with its word, count and 255 words, is 2,050 bytes)
  const bool chk = (ow + T >= W) || (P - e < kDecChkReach);
  for (int rb = 0; rb < T; rb += kRound) {
    int err = 0x7fffffff;
    // (premapped: the serial walk filled round 0's map, decode_body)
    if (!(premapped && rb == 0)) {
    wave_lds_order();  // (the visited masks / last round's map reads are done)
#pragma unroll
    for (int i = 0; i < kMapPer; ++i) blk[lane * kMapPer + i] = 0u;
    wave_lds_order();
    // after the first round only the lanes whose output meets this round
    if (!(chk && rb == 0)) {
      // no record here can fail or fill the piece: the map alone
      if (rb == 0) {
        // round 0 (usually the window's only one): every record's output
        // is at or past the round's start, so it always marks a block
        if (on) {
          uint32_t ro = (uint32_t)o0;
          for (uint32_t q = entry; q < S && ro <= (uint32_t)(kRound - kBlk);) {
            uint32_t tag, c1, c9;
            rec_bytes<!kStream>(pkw, q, tag, c1, c9);
            const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
            atomicMax(&blk[(ro + kBlk - 1) / kBlk], ((ro + 256u) << 12) | (q - e));
            ro += 1u + (zm & c1) + (fm & c9);
            q += 1 + __builtin_popcount(tag) + (zm & 1u) + (fm & (8u * c9 + 1u));
          }
        }
      } else
      if (on && (rb == 0 || (o0 < rb + kRound && o0 + myw > rb))) {
        int ro = o0 - rb;  // round-relative output of the record (> -256 when live)
        // (records past the round's last block start mark nothing, nor
        // do the ones after them)
        for (uint32_t q = entry; q < S && ro <= kRound - kBlk;) {
          uint32_t tag, c1, c9;
          rec_bytes<!kStream>(pkw, q, tag, c1, c9);
          const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
          const int nw = 1 + (int)((zm & c1) + (fm & c9));
          if (ro + nw > 0)
            atomicMax(&blk[(max(ro, 0) + kBlk - 1) / kBlk], ((uint32_t)(ro + 256) << 12) | (q - e));
          ro += nw;
          q += 1 + __builtin_popcount(tag) + (zm & 1u) + (fm & (8u * c9 + 1u));
        }
      }
    } else
    {
      // round 0 of a window near the piece's end.  Only two records can
      // fail or fill the piece: the one whose words reach word W (when the
      // window gets there; the reference stops reading after it), else the
      // window's last record (the only one whose bytes can pass P: every
      // other record ends where the next begins, before wend <= P).  The
      // map walk notes them; one lane then runs the reference's checks
      // on its record (PackedInputStream.java:53-138).
      uint32_t qc = 0xffffffffu;
      int oc = 0;
      if (on) {
        const int wr = W - ow;  // words left in the piece (> 0)
        uint32_t ql = entry;
        int o = o0, ol = o0;
        for (uint32_t q = entry; q < S;) {
          const uint32_t tag = pkw[q], c1 = pkw[q + 1], c9 = pkw[q + 9];
          const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
          const int nw = 1 + (int)((zm & c1) + (fm & c9));
          const int idx = (o + kBlk - 1) / kBlk;  // (round 0: o >= 0)
          if (idx < kRound / kBlk) atomicMax(&blk[idx], ((uint32_t)(o + 256) << 12) | (q - e));
          if (o < wr && o + nw >= wr) {
            qc = q;
            oc = o;
          }
          ql = q;
          ol = o;
          o += nw;
          q += 1 + __builtin_popcount(tag) + (zm & 1u) + (fm & (8u * c9 + 1u));
        }
        if (ow + T < W && lane == 63 - __builtin_clzll(onmask)) {
          qc = ql;
          oc = ol;
        }
      }
      if (qc != 0xffffffffu) {
        const uint32_t q = qc;
        const uint32_t tag = pkw[q], c1 = pkw[q + 1], c9 = pkw[q + 9];
        const uint32_t ntag = 1 + __builtin_popcount(tag);
        const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
        const int nw = 1 + (int)((zm & c1) + (fm & c9));
        const uint32_t adv = ntag + (zm & 1u) + (fm & (8u * c9 + 1u));
        const int oo = ow + oc;
        // truncated tag bytes / count / literal run -> EOF DecodeException;
        // run past the piece -> DecodeException / BufferOverflowException
        int code = 0;
        if (q + ntag > P) code = 2;
        else if (tag == 0 || tag == 0xffu) {
          if (q + (tag ? 10u : 2u) > P) code = 2;
          else if (oo + nw > W) code = 3;
          else if (q + adv > P) code = 2;
        }
        if (!kStream && !code && oo + nw == W && q + adv < P) code = 4;
        if (code) err = (int)(((q - e) << 3) | (uint32_t)code);
        if (oo + nw == W) fin = q + adv;
      }
    }
    }
    if (rb == 0) {
      err = __builtin_amdgcn_readfirstlane(wave_min(err));
      if (err != 0x7fffffff) {
        st = -(err & 7);
        failed = true;
        break;
      }
      fin = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u(fin));
    }
    wave_lds_order();
    {
      // prefix max: lane l holds blocks [kMapPer * l, kMapPer * (l + 1))
      uint32_t m[kMapPer];
      int run = 0;
#pragma unroll
      for (int i = 0; i < kMapPer; ++i) {
        run = max(run, (int)blk[lane * kMapPer + i]);
        m[i] = (uint32_t)run;
      }
      const uint32_t pre = (uint32_t)wave_shr1(wave_incl_max(run), 0);
#pragma unroll
      for (int i = 0; i < kMapPer; ++i) blk[lane * kMapPer + i] = max(m[i], pre);
    }
    wave_lds_order();
    WPH(5)
    const int nb = (min(min(kRound, T - rb), W - ow - rb) + kBlk - 1) / kBlk;
    // two copies of the expansion: one for windows whose records all lie
    // in the loaded bytes (enext + 12 <= lend: the usual case), whose
    // reads need no bound check and no memory path
    auto expand = [&](auto allin) __attribute__((always_inline)) {
    constexpr bool kAllIn = decltype(allin)::value;
    for (int b = lane; b < nb; b += 64) {
      const uint32_t v = blk[b];
      uint32_t q = e + (v & 0xfffu);
      int ofs = kBlk * b + 256 - (int)(v >> 12);
      const int wbase = ow + rb + kBlk * b;  // piece word of the block's first word
      const int wleft = ow + T - wbase - 1;   // words of the window after the block's first
      uint64_t words[kBlk];
      // (the record's tag and count bytes are read once per record, not per
      // word: a literal run's words then need only their own reads, all in
      // flight together)
      uint32_t tag, c1, c9;
      rec_bytes<!kStream>(pkw, q, tag, c1, c9);
      if constexpr (!kStream) {
      // one path for every tag: a zero run's word reads its (unused) bytes
      // and lut[0] selects none; lut[0xff] is the identity for a literal
      // run's words (no divergent branches per word)
      uint64_t sel = lut[tag];
#pragma unroll
      for (int i = 0; i < kBlk; ++i) {
        // PackedInputStream.java:84-134 per word: zero run, 0xFF literal
        // run (tag word, then the counted words), or a tagged word
        const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
        const int nw = 1 + (int)((zm & c1) + (fm & c9));
        const uint32_t rp = (fm && ofs) ? q + 2 + 8u * (uint32_t)ofs : q + 1;
        const uint64_t raw = read8<kAllIn, kLean>(pkw, rp, lend, gp, glim, ph, e);
        const uint32_t rl = (uint32_t)raw, rh = (uint32_t)(raw >> 32);
        const uint32_t x0 = __builtin_amdgcn_perm(rh, rl, (uint32_t)sel);
        const uint32_t x1 = __builtin_amdgcn_perm(rh, rl, (uint32_t)(sel >> 32));
        words[i] = (uint64_t)x0 | ((uint64_t)x1 << 32);
        // past the window's last word: stay put (never stored)
        if (++ofs == nw && i < wleft) {
          q += 1 + __builtin_popcount(tag) + (zm & 1u) + (fm & (8u * c9 + 1u));
          ofs = 0;
          if (i + 1 < kBlk) {
            rec_bytes<!kStream>(pkw, q, tag, c1, c9);
            sel = lut[tag];
          }
        }
      }
      } else {
      // (the stream form keeps the branches: its register budget is tighter,
      // and the one-path form measured 3 % slower there, docs/tuning_log.md r5W)
#pragma unroll
      for (int i = 0; i < kBlk; ++i) {
        // PackedInputStream.java:84-134 per word: zero run, 0xFF literal
        // run (tag word, then the counted words), or a tagged word
        // (the count bytes are read with the tag: one LDS round trip)
        uint64_t x;
        int nw;
        uint32_t adv;
        if (tag == 0) {
          x = 0;
          nw = 1 + c1;
          adv = 2;
        } else if (tag == 0xffu) {
          const uint32_t rn = c9;
          nw = 1 + (int)rn;
          adv = 10 + 8 * rn;
          x = read8<kAllIn, kLean>(pkw, ofs == 0 ? q + 1 : q + 10 + 8 * (uint32_t)(ofs - 1), lend, gp, glim, ph, e);
        } else {
          const uint64_t raw = read8<kAllIn, kLean>(pkw, q + 1, lend, gp, glim, ph, e);
          const uint64_t sel = lut[tag];
          const uint32_t rl = (uint32_t)raw, rh = (uint32_t)(raw >> 32);
          const uint32_t x0 = __builtin_amdgcn_perm(rh, rl, (uint32_t)sel);
          const uint32_t x1 = __builtin_amdgcn_perm(rh, rl, (uint32_t)(sel >> 32));
          x = (uint64_t)x0 | ((uint64_t)x1 << 32);
          nw = 1;
          adv = 1 + __builtin_popcount(tag);
        }
        words[i] = x;
        // past the window's last word: stay put (never stored)
        if (++ofs == nw && i < wleft) {
          q += adv;
          ofs = 0;
          if (i + 1 < kBlk) rec_bytes<!kStream>(pkw, q, tag, c1, c9);
        }
      }
      }
      const int kw = min(kBlk, min(ow + T, W) - wbase);
      uint64_t *d = dst + wbase;
      if (kw == kBlk && ((reinterpret_cast<uintptr_t>(d) & 15) == 0)) {
#pragma unroll
        for (int i = 0; i < kBlk; i += 2) {
          uint4 v4;
          v4.x = (uint32_t)words[i];
          v4.y = (uint32_t)(words[i] >> 32);
          v4.z = (uint32_t)words[i + 1];
          v4.w = (uint32_t)(words[i + 1] >> 32);
          st_stream(v4, d + i);  // (nontemporal: plain stores cut writes 3 % and cost 1.8 % time)
        }
      }
      else if (kLean && kw == kBlk && kBlk == 4) {
        // a full block at an odd word: word 0, words 1-2 as one 16-byte
        // store, word 3 (no per-word branches; round 5: config 2 decode
        // -0.6 %, the dense piece form +2.2 %: not there)
        d[0] = words[0];  // (plain: nontemporal 8-byte stores left partial lines, +6 % HBM writes)
        uint4 v4;
        v4.x = (uint32_t)words[1];
        v4.y = (uint32_t)(words[1] >> 32);
        v4.z = (uint32_t)words[2];
        v4.w = (uint32_t)(words[2] >> 32);
        st_stream(v4, d + 1);
        d[kBlk - 1] = words[kBlk - 1];
      } else {
#pragma unroll
        for (int i = 0; i < kBlk; ++i)
          if (i < kw) d[i] = words[i];
      }
    }
    };
    if (enext + 12 <= lend) expand(std::true_type{});
    else
      expand(std::false_type{});
    wave_lds_order();  // blk reused by the next round
    WPH(6)
  }
  return !failed;
}

// (kAt: the batch form with a range per piece, in_off three words per piece
// as DecPieces<false, true> takes them -- decode_at.hip)
template <bool kStream, bool kSerial = false, bool kAt = false>
__device__ __forceinline__ void decode_body(uint8_t *smem, const uint8_t *__restrict__ packed,
                                            uint64_t *__restrict__ in_off, const uint64_t *__restrict__ swo,
                                            uint32_t n, uint64_t *__restrict__ out, int32_t *__restrict__ status,
                                            uint32_t *ticket, uint64_t avail, DecStreams sd) {
  // the expansion's lean forms (reads from LDS byte addresses, read8; odd
  // blocks' stores without branches), but in the dense piece form, where
  // they measured slower
  constexpr bool kDecLean = kStream || !kSerial;
  uint64_t *lut = reinterpret_cast<uint64_t *>(smem);
  const int lane = lane_id(), w = wave_id();
  uint8_t *wl = smem + 2048 + w * kDecWaveLds;
  uint8_t *wbuf = wl;                                            // window bytes
  uint32_t *blk = reinterpret_cast<uint32_t *>(wl + kWinBuf);    // [256]
  VisMask *visa = reinterpret_cast<VisMask *>(blk);  // [64], over the block map
  if (sd.skip && __builtin_amdgcn_readfirstlane(*sd.skip)) return;
  fill_luts(lut, true);
  if (kSerial && kDecCnt && threadIdx.x == 0)  // (the dense form's counters, below)
    reinterpret_cast<uint64_t *>(smem + kDecCntOff)[0] = 0ull;
  __syncthreads();  // the only block-wide barrier: LUT ready
  // The piece loop is DecPieces' (decode_win.hip, the comments are there),
  // written out: behind it every form but the plain one measured slower
  int xq = (kStream && sd.ns == 1) ? 0 : xcc_id(), dry = 0;
  WPH_INIT
  uint64_t scur = 0;      // stream mode: start of the next piece
  uint64_t slim = avail;  //   end of the stream's bytes
  int sfail = CPK_OK;     //   a failed piece stops the stream
  uint32_t snext = 0, sende = 0, sj = 0;  // next piece, end of the stream's pieces, stream
  bool ser = false;   // the next window is walked by one lane (the last one looked dense)
  uint32_t cool = 0;  // windows before the next serial attempt after one gave up
  int tprev = 0;      // the last window's words (a window near the piece's end stays parallel:
                      // in a stream the bytes do not say where the piece ends)
  // (dense form: windows walked serially / serial walks given back, counted
  // per workgroup at a fixed LDS address -- anything live across the window
  // loop costs the dense forms spills -- and added to ticket[1] / [2] at the
  // end: cpk_ctx_dense_windows)
  uint32_t *cnt = reinterpret_cast<uint32_t *>(smem + kDecCntOff);

  for (uint32_t sidx = 0;; ++sidx) {
    uint32_t seg = sidx;
    if (!kStream) {
      for (;;) {
        seg = take_ticket(ticket, xq);
        if (seg < n || ++dry >= 8) break;
        xq = (xq + 1) & 7;  // this counter ran dry: help the next one
      }
    } else {
      // the next stream with pieces (empty streams end where they begin)
      bool more = true;
      while (snext >= sende) {
        uint32_t j;
        for (;;) {
          j = take_ticket(ticket, xq);
          if (j < sd.ns || ++dry >= 8 || sd.ns == 1) break;
          xq = (xq + 1) & 7;
        }
        if (j >= sd.ns) {
          more = false;
          break;
        }
        if (sd.order) j = (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.order[j]);
        sj = j;
        snext = sd.sbeg ? (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.spc[j]) : 0u;
        sende = sd.sbeg ? (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.spc[j + 1]) : n;
        scur = sd.sbeg ? rfl64(sd.sbeg[j]) : 0;
        slim = sd.sbeg ? rfl64(sd.send[j]) : avail;
        sfail = CPK_OK;
        if (snext >= sende) sd.send_out[j] = scur;
      }
      if (!more) break;
      seg = snext++;
    }
    if (seg >= n) break;
    const uint64_t w0 = rfl64(swo[seg]);
    const int W = __builtin_amdgcn_readfirstlane((int)(swo[seg + 1] - w0));
    const uint64_t a = rfl64(kStream ? scur : in_off[kAt ? 3 * (uint64_t)seg : seg]);
    const uint32_t P = kStream ? (uint32_t)min(slim - scur, (uint64_t)0xffffffffu)
                               : (uint32_t)(in_off[kAt ? 3 * (uint64_t)seg + 1 : seg + 1] - a);
    if (kStream && sfail != CPK_OK) {
      status[seg] = sfail;
      if (seg + 1 == sende) sd.send_out[sj] = scur;
      continue;
    }
    const uint8_t *gp = packed + a;
    const uint32_t glim = (uint32_t)(((a + P + 15) & ~15ull) - a);  // readable bytes
    uint64_t *dst = out + w0;
    int st = CPK_OK;
    uint32_t e = 0;  // true tag position (piece-relative)
    int ow = 0;      // output words produced
    if (W == 0) st = (P == 0 || kStream) ? CPK_OK : CPK_ETRAILING;  // read() of 0 bytes
    while (W != 0) {
      // the window's start and the words so far are wave-uniform: say so
      // (the loop's exits made the compiler keep them in VGPRs and run the
      // window's uniform branches under exec masks)
      e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
      ow = __builtin_amdgcn_readfirstlane(ow);
      if (e >= P) {
        if (ow < W) st = CPK_ETRUNC;  // ArrayInputStream EOF -> DecodeException
        break;
      }
      if (ow >= W) break;  // (trailing input is flagged by the record check)
      const uint32_t wend = min(e + kWin, P);
      WPH(0)
      // (win_load's text, written out: behind the call the dense forms measured 2-5 % slower)
      // ---- window load: LDS byte x <-> packed[(a + e) & ~15 + x] ----------
      const uint32_t padw = (uint32_t)((a + e) & 15);
      const uint32_t ebase = e - padw;  // piece position of wbuf[0]
      const uint32_t need = min(e + kWin + kDecLook, P) - ebase;  // <= kWin + kDecLook + 15 bytes
      const uint32_t lines = (need + 15) >> 4;
      const uint4 *gsrc = reinterpret_cast<const uint4 *>(gp - padw + e);
      // all of a lane's lines (<= 3) in flight at once, then the LDS writes:
      // one memory latency per window instead of one per line
      {
        uint4 l[DecGeom::lines];
#pragma unroll
        for (int j = 0; j < DecGeom::lines; ++j) {
          const uint32_t L = lane + 64 * j;
          l[j] = L < lines ? gsrc[L] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < DecGeom::lines; ++j) {
          const uint32_t L = lane + 64 * j;
          if (L < lines) reinterpret_cast<uint4 *>(wbuf)[L] = l[j];
        }
      }
      const uint32_t lend = ebase + 16 * lines;  // loaded piece positions < lend
      // pkw[q] = packed byte q (signed 64-bit offset: ebase is negative when
      // the piece starts mid-line)
      const uint8_t *pkw = wbuf + (int64_t)padw - (int64_t)e;
      const uint32_t ph = (padw - e) & 3;  // LDS byte phase of piece position 0
      wave_lds_order();
      if constexpr (kSerial) {
        // ---- a dense window: its true records walked by one lane -----------
        // In a window of few, long records (the 0xFF runs of dense data) the
        // 64 speculative chunk walks mostly walk verbatim run bytes, and the
        // chain, count and map walks follow; one lane walking the true chain
        // from e visits only the ~30 true records
        // (PackedInputStream.java:82-134) and fills round 0's block map in
        // order with plain stores (a later record marking the same block is
        // the larger entry, as ds_max keeps it).  Only for windows that can
        // neither fail nor fill the piece and whose words fit one round: a
        // walk that meets the piece's last word, the round's end or
        // kDecSerMax records gives the window to the parallel path.  (The
        // decode_kernel<.., true> form, picked for dense batches: its extra
        // state costs the parallel path ~2 % on config-2 data.)
        if (ser && P - e >= kDecChkReach && W - ow > 2 * tprev) {
          wave_lds_order();
#pragma unroll
          for (int i = 0; i < kMapPer; ++i) blk[lane * kMapPer + i] = 0u;
          wave_lds_order();
          uint32_t q = e, nrec = 0;
          int o = 0, ok = 1;
          if (lane == 0) {
            const int wr = W - ow;  // words left in the piece
            while (q < wend) {
              const DecRec r = rec_at<!kStream>(pkw, q);
              if (o + (int)r.nw >= wr || o + (int)r.nw > kRound || ++nrec > kDecSerMax) {
                ok = 0;
                break;
              }
              if (o <= kRound - kBlk) blk[(o + kBlk - 1) / kBlk] = ((uint32_t)(o + 256) << 12) | (q - e);
              o += (int)r.nw;
              q += r.len;
            }
          }
          if (readlane(ok, 0)) {
            const int T = readlane(o, 0);
            const uint32_t enext = (uint32_t)readlane((int)q, 0);
            uint32_t fin = 0;
            const bool failed = !win_emit<kStream, kDecLean>(pkw, lut, blk, lane, e, ow, W, P, T, false, e, e, 0ull, 0,
                                                   0, enext, lend, gp, glim, ph, dst, st, fin, true DEC_PH_ARGS);
            if (failed) break;  // (cannot happen: no record here is checked)
            ow += T;
            e = enext;
            tprev = T;
            if (kDecCnt && lane == 0) atomicAdd(&cnt[0], 1u);
            continue;
          }
          // too many records (dense but tagged words, e.g. one zero byte per
          // word): the parallel path, and no serial walk for a while
          ser = false;
          cool = kDecSerCool;
          if (kDecCnt && lane == 0) atomicAdd(&cnt[1], 1u);
        }
      }

      WPH(1)
      // ---- 1-3: speculative walks, chain reachability ------------------------
      const WinWalk ww = win_walks<!kStream, DecGeom>(pkw, visa, lane, e, wend DEC_PH_ARGS);
      // ---- the hand-over along the true chain; 4: each lane's output words --
      const WinChain wc = win_chain<!kStream, DecGeom>(pkw, visa, lane, e, wend, ww DEC_PH_ARGS);
      const uint32_t S = ww.S, enext = wc.enext;
      const int T = wc.T;
      // ---- 5: error checks, block map, expansion ------------------------------
      uint32_t fin = 0;  // end of the record that fills the piece (if any)
      const bool failed = !win_emit<kStream, kDecLean>(pkw, lut, blk, lane, e, ow, W, P, T, wc.on, wc.entry, S,
                                                       wc.onmask, wc.o0, wc.myw, enext, lend, gp, glim, ph, dst, st,
                                                       fin, false DEC_PH_ARGS);
      if (failed) {
        // (kAt: a piece full before its range ends says where -- the lane that
        // checked the filling record holds its end; written here, so nothing
        // more is live across the window loop)
        if constexpr (kAt && !kStream)
          if (st == CPK_ETRAILING) in_off[3 * (uint64_t)seg + 2] = a + wave_max_u(fin);
        break;
      }
      if (ow + T >= W && fin) {  // the piece is full: next piece starts at fin
        ow = W;
        e = fin;
        break;
      }
      if constexpr (kSerial) {
        // dense data: ~8 packed bytes per word (0xFF runs); config-2-like
        // windows take ~3.8 (their ~550 records would be a long serial walk)
        // (wave-uniform values: kept in scalar registers)
        if (cool) --cool;
        else ser = __builtin_amdgcn_readfirstlane((int)(16u * (uint32_t)T < 3u * (enext - e))) != 0;
        tprev = __builtin_amdgcn_readfirstlane(T);
      }
      ow += T;
      e = enext;
    }
    status[seg] = st;  // every lane the same value: no lane-dependent branch
    if (kStream) {
      in_off[seg] = a;
      scur = a + e;
      sfail = st;
      if (seg + 1 == sende) sd.send_out[sj] = scur;
    }
  }
  if constexpr (kSerial && kDecCnt) {
    // (each wave hands on what the workgroup has counted so far, its own
    // counts included: every count is taken by its own wave's exchange)
    if (lane == 0) {
      const uint32_t a = atomicExch(&cnt[0], 0u), b = atomicExch(&cnt[1], 0u);
      if (a) atomicAdd(&ticket[1], a);
      if (b) atomicAdd(&ticket[2], b);
    }
  }
  WPH_FLUSH(16)
}
template <bool kStream, bool kSerial = false>
__global__ __launch_bounds__(kDecThreads, kDecWpe) void decode_kernel(
    const uint8_t *__restrict__ packed, uint64_t *__restrict__ in_off,
    const uint64_t *__restrict__ swo, uint32_t n, uint64_t *__restrict__ out,
    int32_t *__restrict__ status, uint32_t *ticket, uint64_t avail, DecStreams sd) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  decode_body<kStream, kSerial>(smem, packed, in_off, swo, n, out, status, ticket, avail, sd);
}
