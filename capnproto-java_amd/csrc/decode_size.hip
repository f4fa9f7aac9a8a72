// decode_size.hip -- unpacked sizes of packed pieces without decoding
// (cpk_unpacked_size_batch): how many words each piece's packed byte range
// unpacks to, read as PackedInputStream.java:82-134 reads records, with no
// word written.  Included from packed_codec.hip (namespace cpk) after
// decode_win.hip, the decoders and stream_split.hip.  Two forms:
//   us_wave_kernel  a wave per piece: decode_win.hip's window load, walks and
//                   chain over the piece, the windows' words summed -- no
//                   block map, no record index, no expansion.
//   us_end_kernel   a few large pieces: stream_split.hip's block map
//                   (ss_scan / ss_group / ss_top / ss_cut) over one piece's
//                   bytes alone, as cpk_decode_message_stream runs it, then
//                   this kernel walks the last whole records to the piece's
//                   end.  A piece whose map is irregular or which ends inside
//                   a record is left to the wave form.
//
// The end of a piece.  A window's walks stop at wend = min(e + win, P), so
// the chain's last record starts before P and enext is where it ends: the
// piece is CPK_OK when that is P exactly and CPK_ETRUNC when it is past P.
// The loaded 16-byte lines reach up to 15 bytes past P, and a record that
// starts before P may take its count byte from those garbage bytes -- never
// with a wrong verdict, because every record whose count byte lies at or past
// P has a length whose lower bound already passes P:
//   * a 0x00 tag at q has its count at q + 1 >= P only for q = P - 1: its
//     length is 2 whatever the count says, q + 2 = P + 1 > P;
//   * a 0xFF tag at q has its count at q + 9 >= P only for q >= P - 9: its
//     length is 10 + 8 * count >= 10, q + 10 > P;
//   * any other tag's length, 1 + popcount(tag), depends on no other byte.
// The garbage changes by how much enext passes P and the words of that last
// record, never whether it passes; a piece that is not CPK_OK reports 0 words.
// A record whose count byte lies before P is read from the piece's own bytes,
// and its length is exact: enext > P then means a tag without all its bytes
// or a literal run cut short.

// The map decoder's chunk and look-ahead (the one geometry measured); with no
// expansion table the wave's LDS is the window buffer and the visited masks
constexpr uint32_t kUsChunk = 56;
constexpr uint32_t kUsLook = 240;
typedef WinGeom<kUsChunk, kUsLook> UsGeom;
constexpr int kUsThreads = 256;  // 4 independent waves
// 8 workgroups of 4 waves per CU: 8 waves per SIMD, the hardware's limit
// (4,368 B of LDS per wave, 139,776 B per CU; at most 64 VGPRs)
constexpr int kUsWpe = 8;
constexpr uint32_t kUsWaveLds = UsGeom::buf + 64 * sizeof(VisMask);
constexpr uint32_t kUsLds = (kUsThreads / 64) * kUsWaveLds;
static_assert(kUsWaveLds % 16 == 0, "each wave's window buffer on a 16-byte line");
static_assert(kUsWpe * kUsLds <= 160 * 1024, "kUsWpe workgroups per CU by LDS");

// One wave's pieces off the per-XCD ticket counters (DecPieces' batch form
// without the word offsets): every value is wave-uniform.
struct UsPieces {
  uint32_t *ticket;
  uint32_t n;
  int xq, dry = 0;
  __device__ __forceinline__ UsPieces(uint32_t *ticket, uint32_t n) : ticket(ticket), n(n), xq(xcc_id()) {}
  // the next piece, or n when none is left (all 64 lanes call it: one folded
  // +64 atomic per wave, the counter's index said to be wave-uniform)
  __device__ __forceinline__ uint32_t next() {
    uint32_t seg;
    for (;;) {
      seg = take_ticket(ticket, __builtin_amdgcn_readfirstlane(xq));
      if (seg < n || ++dry >= 8) break;
      xq = (xq + 1) & 7;  // this counter ran dry: help the next one
    }
    return seg < n ? seg : n;
  }
};

// (us_wave_at_kernel, decode_at.hip, is this kernel's loop written out again
// over a begin and an end array -- with the loop shared through an inlined
// function this kernel's scalar registers moved: a change here goes there too)
// words[i], status[i] of every piece i (todo: only of those with todo[i]
// nonzero -- the pieces the block form left over)
__global__ __launch_bounds__(kUsThreads, kUsWpe) void us_wave_kernel(const uint8_t *__restrict__ packed,
                                                                     const uint64_t *__restrict__ in_off, uint32_t n,
                                                                     uint64_t *__restrict__ words,
                                                                     int32_t *__restrict__ status, uint32_t *ticket,
                                                                     const uint32_t *__restrict__ todo) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  uint8_t *wbuf = smem + wave_id() * kUsWaveLds;
  VisMask *visa = reinterpret_cast<VisMask *>(wbuf + UsGeom::buf);
  UsPieces pc(ticket, n);
  for (;;) {
    const uint32_t seg = pc.next();
    if (seg >= n) break;
    if (todo && __builtin_amdgcn_readfirstlane((int)todo[seg]) == 0) continue;
    const uint64_t a = rfl64(in_off[seg]);
    // (a piece's length modulo 2^32, as the batch decoders take it)
    const uint32_t P = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(in_off[seg + 1] - a));
    const uint8_t *gp = packed + a;
    uint32_t e = 0;
    uint64_t w = 0;
    while (e < P) {
      const uint32_t wend = min(e + UsGeom::win, P);
      const WinBytes wb = win_load<UsGeom>(wbuf, lane, gp, a, e, P);
      const WinWalk ww = win_walks<true, UsGeom>(wb.pkw, visa, lane, e, wend);
      const WinChain wc = win_chain<true, UsGeom>(wb.pkw, visa, lane, e, wend, ww);
      w += (uint64_t)(uint32_t)wc.T;
      e = (uint32_t)__builtin_amdgcn_readfirstlane((int)wc.enext);
      wave_lds_order();  // (the next window's load overwrites wbuf and visa)
    }
    const bool ok = e == P;  // e > P: the last record runs past the range
    if (lane == 0) {
      words[seg] = ok ? w : 0;
      status[seg] = ok ? CPK_OK : CPK_ETRUNC;
    }
  }
}

// The block form's end for one piece of R bytes whose map B holds (nbmax
// blocks): from the last block that starts at a true record the whole records
// are walked to where they end; the piece is CPK_OK iff that is R and the map
// was regular.  Otherwise todo stays set and the wave form sizes the piece.
__global__ void us_end_kernel(const uint8_t *__restrict__ pk, uint64_t nbmax, SsBufs B, uint64_t *__restrict__ words,
                              int32_t *__restrict__ status, uint32_t *__restrict__ todo) {
  if (threadIdx.x || blockIdx.x) return;
  const uint64_t R = B.lim[0], nb = ss_nb(B, nbmax), W = B.WO[nb];
  const uint64_t lo = ms_block(B, nb, kSsInf);
  uint64_t p = B.E[lo], w = B.WO[lo];
  while (p < R && ss_step(SsGlobal{pk, R}, R, p, w)) {
  }
  const bool ok = p == R && w == W && B.flag[0] == 0;
  if (ok) {
    *words = w;
    *status = CPK_OK;
  }
  *todo = ok ? 0u : 1u;
}
