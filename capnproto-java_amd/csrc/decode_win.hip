// decode_win.hip -- what every wave-per-window decoder does before it knows
// what to write: the pieces a wave takes one after another (DecPieces), a
// window's bytes into LDS (win_load), the speculative chunk walks with their
// pointer-doubling reachability (win_walks) and the hand-over along the true
// chain with each lane's output words (win_chain).  Included from
// packed_codec.hip (namespace cpk) before the decoders: decode_v2.hip
// (decode2_kernel) uses all of it, decode_map.hip (decode_body) the walks and
// the chain -- its piece loop and window load are the same text written out,
// faster so in its dense and stream forms --, decode_mw.hip (mw_window) the
// load and the walks.  decode_map.hip's header describes the phases.

// A decoder's window geometry: lane chunks of `chunk` bytes, kLook bytes
// loaded past the window's 64 chunks (a literal run reaching past them is
// read from memory).
template <uint32_t kChunk, uint32_t kLook>
struct WinGeom {
  static constexpr uint32_t chunk = kChunk;
  static constexpr uint32_t win = 64 * kChunk;  // packed bytes resolved per window
  static constexpr uint32_t look = kLook;
  static constexpr uint32_t buf = (win + 15 + look + 16 + 15) & ~15u;  // + pad, look-ahead, slack
  static constexpr int lines = (int)((win + 15 + look + 15) / 16 + 63) / 64;  // 16-byte lines per lane
  // errors and the record that fills the piece can only occur in a window
  // reaching the piece's last word or starting within `reach` of its end
  // (the window's records start before e + win; the longest record, a 0xFF
  // tag with its word, count and 255 words, is 2,050 bytes)
  static constexpr uint32_t reach = win + 2064;
  static_assert(reach >= win + 2050, "a window's last record must fall inside the checked reach");
  static_assert(chunk <= 64, "visited mask bits");
};

// a lane's visited positions: one bit per chunk byte (bit q mod 64 for
// position q: the walks index it by the position itself, so it is 64 bits
// whatever the chunk size)
typedef uint64_t VisMask;
static_assert(sizeof(VisMask) == 8, "visited bits are set at position mod 64");

// The tag at piece position q and both possible count bytes (c1 after a
// 0x00 tag, c9 after 0xFF), read together: one LDS round trip per record on
// the walks.  (Round 5: reading a count byte only for the tags that have one
// cut the decoder's LDS cycles 22 % and made it 6 % slower -- the dependent
// second read and its exec-mask branches, docs/tuning_log.md.)
template <bool k32 = true>
__device__ __forceinline__ void rec_bytes(const uint8_t *pkw, uint32_t q, uint32_t &tag, uint32_t &c1, uint32_t &c9) {
  tag = pkw[q];
  c1 = pkw[q + 1];
  c9 = pkw[q + 9];
  // k32: the tag kept a 32-bit value (hipcc otherwise narrows it to 16-bit
  // ops: a mask and a separate +1 around every popcount; round 5: config 2
  // decode -1.0 %, the stream forms +5 %: not there)
  if constexpr (k32) asm("" : "+v"(tag));
}

// The record whose tag is at piece position q: its byte length and output
// words (PackedInputStream.java:82-134).
struct DecRec {
  uint32_t len, nw;
};
template <bool k32 = true>
__device__ __forceinline__ DecRec rec_at(const uint8_t *pkw, uint32_t q) {
  uint32_t tag, c1, c9;
  rec_bytes<k32>(pkw, q, tag, c1, c9);
  // masks, not nested selects (hipcc turns those into exec-mask branches)
  const uint32_t zm = 0u - (uint32_t)(tag == 0), fm = 0u - (uint32_t)(tag == 0xffu);
  DecRec r;
  r.len = 1u + __builtin_popcount(tag) + (zm & 1u) + (fm & (8u * c9 + 1u));
  r.nw = 1u + (zm & c1) + (fm & c9);
  return r;
}

// ---- the pieces ------------------------------------------------------------
// kStream = false: piece i's packed bytes are [in_off[i], in_off[i+1]) and a
//   piece that fills before its range ends is CPK_ETRAILING.
// kStream = true: packed streams, each a wave's: the pieces of stream j,
//   [spc[j], spc[j+1]), are decoded back to back from its bytes
//   [sbeg[j], send[j]); each read() fills its piece and leaves the rest of
//   the stream to the next (PackedInputStream.java:35-140 as Serialize.read
//   calls it, Serialize.java:165-175).  in_off[piece] is written with the
//   piece's start and send_out[j] with the stream's end.  sbeg == nullptr:
//   one stream, pieces 0..n-1, bytes [0, avail).
struct DecStreams {
  const uint64_t *sbeg, *send, *spc;
  uint32_t ns;
  uint64_t *send_out;
  const uint32_t *skip;   // (batch form: nonzero = the other decoder took the batch)
  const uint32_t *order;  // (stream form: ticket -> stream, largest first; null: in order)
  // the forms the host passes: the batch form (skip: its gate word, or null)
  static DecStreams batch(const uint32_t *skip = nullptr) {
    return {nullptr, nullptr, nullptr, 0, nullptr, skip, nullptr};
  }
  // one stream, pieces 0..n-1, bytes [0, avail): its end to *end_out
  static DecStreams one(uint64_t *end_out) { return {nullptr, nullptr, nullptr, 1, end_out, nullptr, nullptr}; }
  // one stream from a device descriptor: desc[0] its begin, [1] its end, [2..3] its pieces
  static DecStreams one_desc(const uint64_t *desc, uint64_t *end_out) {
    return {desc, desc + 1, desc + 2, 1, end_out, nullptr, nullptr};
  }
  // ns streams, a wave each, in `order`; their ends to end_out[0..ns)
  static DecStreams many(const uint64_t *sbeg, const uint64_t *send, const uint64_t *spc, uint32_t ns,
                         uint64_t *end_out, const uint32_t *order) {
    return {sbeg, send, spc, ns, end_out, nullptr, order};
  }
};

// One wave's pieces: next() takes the next one (false: none is left) and
// done() writes what it came to.  Batch pieces come from the per-XCD ticket
// counters, a stream's pieces one after another from the stream a ticket
// gave the wave.  Every value here is wave-uniform.
// kAt (the batch form of cpk_decode_batch_at, decode_at.hip): in_off holds three
//   words per piece -- its first packed byte, the end of its range (a range
//   of its own), and, written by the decoder for a piece full before its
//   range ends (CPK_ETRAILING), where the piece ended.  One array, so the
//   form keeps no pointer the batch form does not.
template <bool kStream, bool kAt = false>
struct DecPieces {
  const uint64_t *swo;
  uint64_t *in_off;
  int32_t *status;
  uint32_t *ticket;
  uint32_t n;
  uint64_t avail;
  const DecStreams &sd;
  int xq, dry = 0;
  uint64_t scur = 0;      // stream mode: start of the next piece
  uint64_t slim;          //   end of the stream's bytes
  int sfail = CPK_OK;     //   a failed piece stops the stream
  uint32_t snext = 0, sende = 0, sj = 0;  // next piece, end of the stream's pieces, stream
  // the piece: its index, first output word and words, its first packed byte,
  // its packed bytes (a stream's: all that are left) and the readable ones
  uint32_t seg;
  uint64_t w0, a;
  int W;
  uint32_t P, glim;

  // (one stream: its one ticket is item 0 of counter 0 -- start there, and
  // a wave that does not get it leaves at once instead of trying the other
  // seven counters one dependent atomic after another)
  __device__ __forceinline__ DecPieces(const uint64_t *swo, uint64_t *in_off, int32_t *status, uint32_t *ticket,
                                       uint32_t n, uint64_t avail, const DecStreams &sd)
      : swo(swo), in_off(in_off), status(status), ticket(ticket), n(n), avail(avail), sd(sd),
        xq((kStream && sd.ns == 1) ? 0 : xcc_id()), slim(avail) {}

  __device__ __forceinline__ bool next() {
    for (;;) {
      // every branch below is on wave-uniform (SGPR) values: the compiler
      // must not turn the piece / window loops into divergent loops
      // All 64 lanes add 1 (hipcc folds it into one +64 atomic): no lane-0-only
      // branch at the loop head, which hipcc otherwise structurised into a
      // divergent loop re-running piece 0.  Tickets count in units of 64.
      // The counter's index is said to be wave-uniform (readfirstlane): the
      // fold needs a uniform address, and without it the stream forms' 64
      // lanes added 1 each -- two waves' lanes interleave, lane 0 no longer
      // reads a multiple of 64 and a ticket is taken twice, another never.
      if (!kStream) {
        for (;;) {
          seg = take_ticket(ticket, __builtin_amdgcn_readfirstlane(xq));
          if (seg < n || ++dry >= 8) break;
          xq = (xq + 1) & 7;  // this counter ran dry: help the next one
        }
      } else {
        // the next stream with pieces (empty streams end where they begin)
        while (snext >= sende) {
          uint32_t j;
          for (;;) {
            j = take_ticket(ticket, __builtin_amdgcn_readfirstlane(xq));
            if (j < sd.ns || ++dry >= 8 || sd.ns == 1) break;
            xq = (xq + 1) & 7;
          }
          if (j >= sd.ns) return false;
          // (the stream's values are wave-uniform: kept in scalar registers,
          // which leaves the stream form's VGPRs to the windows)
          if (sd.order) j = (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.order[j]);
          sj = j;
          snext = sd.sbeg ? (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.spc[j]) : 0u;
          sende = sd.sbeg ? (uint32_t)__builtin_amdgcn_readfirstlane((int)sd.spc[j + 1]) : n;
          scur = sd.sbeg ? rfl64(sd.sbeg[j]) : 0;
          slim = sd.sbeg ? rfl64(sd.send[j]) : avail;
          sfail = CPK_OK;
          if (snext >= sende) sd.send_out[j] = scur;
        }
        seg = snext++;
      }
      if (seg >= n) return false;
      w0 = rfl64(swo[seg]);
      W = __builtin_amdgcn_readfirstlane((int)(swo[seg + 1] - w0));
      a = rfl64(kStream ? scur : in_off[kAt ? 3 * (uint64_t)seg : seg]);
      P = kStream ? (uint32_t)min(slim - scur, (uint64_t)0xffffffffu)
                  : (uint32_t)(in_off[kAt ? 3 * (uint64_t)seg + 1 : seg + 1] - a);
      if (kStream && sfail != CPK_OK) {
        status[seg] = sfail;
        if (seg + 1 == sende) sd.send_out[sj] = scur;
        continue;
      }
      glim = (uint32_t)(((a + P + 15) & ~15ull) - a);  // readable bytes
      return true;
    }
  }
  // the status of a piece of no words: a read() of 0 bytes
  __device__ __forceinline__ int empty_status() const { return (P == 0 || kStream) ? CPK_OK : CPK_ETRAILING; }
  // the piece came to st; a stream's next piece starts at piece position e
  __device__ __forceinline__ void done(int st, uint32_t e) {
    status[seg] = st;  // every lane the same value: no lane-dependent branch
    if (kStream) {
      in_off[seg] = a;
      scur = a + e;
      sfail = st;
      if (seg + 1 == sende) sd.send_out[sj] = scur;
    }
  }
};

// ---- window load: LDS byte x <-> packed[(a + e) & ~15 + x] -------------------
// The window at piece position e of the piece at packed offset a (gp = packed
// + a, P bytes): its bytes and G::look more, whole 16-byte lines, into wbuf.
// lend: loaded piece positions < lend; pkw[q] = packed byte q; ph: the LDS
// byte phase of piece position 0.
struct WinBytes {
  const uint8_t *pkw;
  uint32_t lend, ph;
};
template <class G>
__device__ __forceinline__ WinBytes win_load(uint8_t *wbuf, int lane, const uint8_t *gp, uint64_t a, uint32_t e,
                                             uint32_t P) {
  const uint32_t padw = (uint32_t)((a + e) & 15);
  const uint32_t ebase = e - padw;  // piece position of wbuf[0]
  const uint32_t need = min(e + G::win + G::look, P) - ebase;  // <= win + look + 15 bytes
  const uint32_t lines = (need + 15) >> 4;
  const uint4 *gsrc = reinterpret_cast<const uint4 *>(gp - padw + e);
  // all of a lane's lines (<= 3) in flight at once, then the LDS writes:
  // one memory latency per window instead of one per line
  {
    uint4 l[G::lines];
#pragma unroll
    for (int j = 0; j < G::lines; ++j) {
      const uint32_t L = lane + 64 * j;
      l[j] = L < lines ? gsrc[L] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < G::lines; ++j) {
      const uint32_t L = lane + 64 * j;
      if (L < lines) reinterpret_cast<uint4 *>(wbuf)[L] = l[j];
    }
  }
  WinBytes wb;
  wb.lend = ebase + 16 * lines;
  // (signed 64-bit offset: ebase is negative when the piece starts mid-line)
  wb.pkw = wbuf + (int64_t)padw - (int64_t)e;
  wb.ph = (padw - e) & 3;
  wave_lds_order();
  return wb;
}

// (stats build: the window phases' clock sums live in the caller)
#ifdef CPK_PHASE_STATS
#define DEC_PH_PARAMS , unsigned long long &wph_last, unsigned long long *wph_acc
#define DEC_PH_ARGS , wph_last, wph_acc
#else
#define DEC_PH_PARAMS
#define DEC_PH_ARGS
#endif
// ---- 1-3 of a window [e, wend): lane l walks its chunk [cb, cb + G::chunk)
// from cb as if a tag stood there (the visited positions into visa[l], its
// words wt, its exit X), then on until it lands on a position some lane
// visited -- from there the two walks coincide, the chain being a function of
// the position -- (S, its words lw); R: the lanes reachable from l under
// "lane -> owner of its landing point" (always a later lane), by pointer
// doubling (6 rounds cover a chain of 64).  Nothing here depends on where the
// window's true records start.  kCountRecs (the record index): the records of
// the two walks too (nr, lr).
struct WinWalk {
  uint32_t cb, S, wt, lw;
  uint64_t R;
  uint32_t nr, lr;
};
template <bool k32, class G, bool kCountRecs = false>
__device__ __forceinline__ WinWalk win_walks(const uint8_t *pkw, VisMask *visa, int lane, uint32_t e,
                                             uint32_t wend DEC_PH_PARAMS) {
  // ---- 1: speculative chunk walks --------------------------------------
  const uint32_t cb = e + G::chunk * lane;
  const uint32_t ce = min(cb + G::chunk, wend);
  VisMask vis = 0;
  uint32_t X = cb, wt = 0;  // wt: output words of the walk
  if (cb < wend) {
    uint32_t pos = cb;
    while (pos < ce) {
      // (the bit of piece position pos mod 64 -- a rotation of the chunk
      // offsets, distinct for a chunk of 64 bytes or fewer: the shift takes
      // pos itself, no subtraction per record; round 5: config 2 decode
      // -0.5 %)
      vis |= (VisMask)1 << (pos & 63u);
      const DecRec r = rec_at<k32>(pkw, pos);
      wt += r.nw;
      pos += r.len;
    }
    X = pos;
  }
  visa[lane] = vis;
  wave_lds_order();
  // ---- 2: walk on until landing on a visited position -------------------
  uint32_t S = X, lw = 0, lr = 0;  // lw / lr: output words / records of the landing walk
  if (cb < wend) {
    while (S < wend) {
      const uint32_t r = S - e;
      const uint32_t ow_ = chunk_div<G::chunk>(r);
      if ((visa[ow_] >> (S & 63u)) & 1) break;  // (bit S mod 64, as above)
      const DecRec rr = rec_at<k32>(pkw, S);
      lw += rr.nw;
      if constexpr (kCountRecs) ++lr;
      S += rr.len;
    }
  }
  WPH(2)
  // ---- 3: reachability over lanes --------------------------------------
  int nx = (cb < wend && S < wend) ? (int)chunk_div<G::chunk>(S - e) : 64;
  uint64_t R = 1ull << lane;
  {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int src = (nx & 63) << 2;
    const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)R);
    const uint32_t rhi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(R >> 32));
    const int nn = __builtin_amdgcn_ds_bpermute(src, nx);
    if (nx < 64) {
      R |= ((uint64_t)rhi << 32) | rlo;
      nx = nn;
    }
  }
  }
  WinWalk ww;
  ww.cb = cb;
  ww.S = S;
  ww.wt = wt;
  ww.lw = lw;
  ww.R = R;
  ww.nr = kCountRecs ? (uint32_t)__builtin_popcountll(vis) : 0u;
  ww.lr = lr;
  return ww;
}

// ---- the hand-over and 4 of a window whose walks started at its first true
// record e: the true records are on the lanes reachable from lane 0
// (onmask); each of them (on) holds the records [entry, S), entry handed to
// it by its predecessor through visa, the last one's S being the next
// window's start (enext); myw: their output words, o0: the window word of the
// first, T: the window's words.  kCountRecs: the same for the records (myr,
// r0, NR).
struct WinChain {
  uint64_t onmask;
  uint32_t enext, entry;
  bool on;
  int myw, T, o0;
  int myr, NR, r0;
};
template <bool k32, class G, bool kCountRecs = false>
__device__ __forceinline__ WinChain win_chain(const uint8_t *pkw, VisMask *visa, int lane, uint32_t e, uint32_t wend,
                                              const WinWalk &ww DEC_PH_PARAMS) {
  WinChain c;
  c.onmask = readlane64(ww.R, 0);
  c.enext = (uint32_t)__builtin_amdgcn_readlane((int)ww.S, 63 - __builtin_clzll(c.onmask));
  // each on-path lane hands its landing point to its successor
  wave_lds_order();  // (phase 2's reads of visa are done)
  if (((c.onmask >> lane) & 1) && ww.S < wend) visa[chunk_div<G::chunk>(ww.S - e)] = (VisMask)ww.S;
  wave_lds_order();
  c.entry = lane == 0 ? e : (uint32_t)visa[lane];
  c.on = (c.onmask >> lane) & 1;
  WPH(3)
  // ---- 4: output words of each lane's true records ----------------------
  // [entry, S) = the walk's records from entry (a position the walk
  // visited) plus the landing walk: the walk's words (records) minus those
  // before entry (usually one or two records of a false start)
  c.myw = 0, c.myr = 0;
  if (c.on) {
    uint32_t pre = 0, prer = 0;
    for (uint32_t q = ww.cb; q < c.entry;) {
      const DecRec r = rec_at<k32>(pkw, q);
      pre += r.nw;
      if constexpr (kCountRecs) ++prer;
      q += r.len;
    }
    c.myw = (int)(ww.wt - pre + ww.lw);
    c.myr = (int)(ww.nr - prer + ww.lr);
  }
  const int inc = wave_incl_add(c.myw);
  c.T = readlane(inc, 63);
  c.o0 = inc - c.myw;  // window-relative output of this lane's first record
  c.NR = c.r0 = 0;
  if constexpr (kCountRecs) {
    const int incr = wave_incl_add(c.myr);
    c.NR = readlane(incr, 63);  // true records in the window
    c.r0 = incr - c.myr;        // rank of this lane's first record
  }
  WPH(4)
  return c;
}
