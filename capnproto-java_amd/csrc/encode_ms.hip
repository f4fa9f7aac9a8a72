// encode_ms.hip -- a stream of unpacked messages whose boundaries are not
// known, packed in one call (cpk_encode_message_stream): a loop of
// Serialize.read(ReadableByteChannel) over the words (Serialize.java:119-178),
// each message written with SerializePacked.write (SerializePacked.java:
// 101-134, Serialize.java:256-288).  Included by packed_codec.hip after
// stream_split.hip, whose wave helpers (ss_rl64, ss_scan_add) it uses.
//
// The input is what cpk_decode_message_stream writes: every message's table
// words followed by its segments.  Its pieces -- the table's words as they
// stand, then each segment -- tile the words of the complete messages, so
// once their word offsets are known the stream is an ordinary batch:
//   ems_chain  one wave follows the messages through the words, as ms_chain
//              does on the decode side: a message's first 64 words a lane
//              each (the first table word and up to 127 sizes in one round
//              trip), larger tables 64 sizes a round, the sizes checked in
//              Serialize.read's order and scanned into the pieces' places.
//              It writes the piece word offsets, each message's first piece
//              and the result row, and stops at the end of the words or at
//              the first message that fails;
// the host reads the row back (the piece count sizes the encoders' launches)
// and the pieces go to the batch encoder (cpk_encode_batch_cap's path).
//
// The table rounds restate ms_chain_kernel's (a lambda inside that kernel):
// they are copied here, not shared, so that kernel compiles to what it did.
// Unlike it this chain tells the failures apart, because here no later
// kernel reads the message again: the tail status is made in this wave.

// the result row
constexpr int kEmsMsgs = 0, kEmsPieces = 1, kEmsWords = 2, kEmsTail = 3, kEmsMax = 4, kEmsRow = 8;

// piece_lim / msg_lim: the last entry piece_off / msg_piece holds (-1 with no
// array).  Entries past them are not stored; the counting goes on.
__global__ __launch_bounds__(64) void ems_chain_kernel(const uint64_t *__restrict__ in, uint64_t W, uint64_t limit,
                                                       uint64_t *__restrict__ piece_off, int64_t piece_lim,
                                                       uint64_t *__restrict__ msg_piece, int64_t msg_lim,
                                                       uint64_t *__restrict__ row) {
  const int lane = (int)threadIdx.x;
  uint64_t x = 0, m = 0, pb = 0;
  uint64_t lmax = 0;  // (per lane: the largest piece it has seen in a complete message)
  int st = CPK_OK;
  // the message's first 64 words, a lane each
  uint64_t head = W ? in[min(x + (uint64_t)lane, W - 1)] : 0;
  for (;;) {
    // (the entry of the message that ends the loop closes both arrays)
    if (lane == 0) {
      if ((int64_t)pb <= piece_lim) piece_off[pb] = x;
      if ((int64_t)m <= msg_lim) msg_piece[m] = pb;
    }
    if (x >= W) break;
    const uint64_t first = ss_rl64(head, 0);
    const uint32_t raw = (uint32_t)first;
    // Serialize.java:128-139: the count, then segment 0's size, before the
    // rest of the table is read
    if (raw > 511u || (int32_t)(uint32_t)(first >> 32) < 0) {
      st = CPK_EFRAME;
      break;
    }
    const uint32_t count = raw + 1, rest = (count & ~1u) / 2;
    if (x + 1 + rest > W) {  // :146-148, the words end inside the table
      st = CPK_ETRUNC;
      break;
    }
    const uint64_t s0w = x + 1 + rest;
    // segment i's size is u32 i + 1 of the table; table words under 64 are in `head`
    auto round = [&](uint32_t base, uint64_t before, uint32_t &sz, uint64_t &beg) {
      const uint32_t i = base + (uint32_t)lane, u = i + 1, wi = u / 2;
      const uint64_t hv = __shfl(head, (int)(wi & 63u), 64);
      const uint64_t wv = wi < 64u ? hv : (i < count ? in[x + wi] : 0);
      sz = i < count ? (uint32_t)(wv >> (32 * (u & 1))) : 0u;
      const uint64_t inc = ss_scan_add(sz, lane);
      beg = s0w + before + inc - sz;
      return ss_rl64(inc, 63);
    };
    uint64_t total = 0, beg0 = 0, bigbeg = 0, mmax = lane == 0 ? 1u + rest : 0u;
    uint32_t sz0 = 0;
    bool neg = false, big = false;
    for (uint32_t base = 0; base < count; base += 64) {
      uint32_t sz;
      uint64_t beg;
      const uint64_t sum = round(base, total, sz, beg);
      neg |= __ballot((int32_t)sz < 0) != 0;
      const uint64_t bm = __ballot(sz > (uint32_t)kMaxSegmentWords);
      if (bm && !big) {  // the first segment that cannot be allocated, and where it would start
        big = true;
        bigbeg = ss_rl64(beg, (int)__builtin_ctzll(bm));
      }
      mmax = max(mmax, (uint64_t)sz);
      if (base == 0) {
        sz0 = sz;
        beg0 = beg;
      }
      total += sum;
    }
    // :150-162 a negative size, the traversal limit; then the segments in
    // order (:165-175): one over 2^28 - 1 words throws where it would be
    // allocated (:45-53), unless the words end in a segment before it
    if (neg || total > limit) st = CPK_EFRAME;
    else if (big) st = bigbeg <= W ? CPK_EFRAME : CPK_ETRUNC;
    else if (s0w + total > W) st = CPK_ETRUNC;
    if (st != CPK_OK) break;
    // the next message's first words on their way before this one's stores
    const uint64_t xn = s0w + total;
    const uint64_t nhead = xn < W ? in[min(xn + (uint64_t)lane, W - 1)] : 0;
    uint64_t before = 0;
    for (uint32_t base = 0; base < count; base += 64) {
      uint32_t sz = sz0;
      uint64_t beg = beg0;
      if (base) before += round(base, before, sz, beg);
      else before = ss_rl64(beg0 + sz0, 63) - s0w;
      const uint64_t j = pb + 1 + base + (uint32_t)lane;
      if (base + (uint32_t)lane < count && (int64_t)j <= piece_lim) piece_off[j] = beg;
    }
    head = nhead;
    lmax = max(lmax, mmax);
    x = xn;
    pb += 1 + count;
    ++m;
  }
  for (int d = 32; d; d >>= 1) lmax = max(lmax, (uint64_t)__shfl_xor(lmax, d, 64));
  if (lane == 0) {
    row[kEmsMsgs] = m;
    row[kEmsPieces] = pb;
    row[kEmsWords] = x;
    row[kEmsTail] = (uint64_t)(int64_t)st;
    row[kEmsMax] = lmax;
  }
}
