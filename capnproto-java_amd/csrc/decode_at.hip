// decode_at.hip -- the decoders with every group's packed range given by the
// caller (cpk_decode_batch_at, cpk_unpacked_size_batch_at): what reads back
// what cpk_encode_batch_at (encode_at.hip) placed.  Included from
// packed_codec.hip (namespace cpk) after the decoders and decode_size.hip: it
// runs their text -- decode_body, the record-index kernel's body
// (decode_v2_body.hip) with DecPieces, decode_size.hip's pieces and window
// loop, the windows, walks, block map and expansion behind them -- with the
// piece's end taken from an array of its own (kAt), and leaves every existing
// instantiation as it compiled before.
//
// Group g's packed bytes are [src_off[g], src_off[g] + src_len[g]) of the
// packed buffer, any alignment, any order, gaps and overlaps allowed: the
// buffer is only read.  New against cpk_decode_batch is where a piece's first
// byte and length come from, and what refuses a range before a byte of it is
// read:
//   dat_prep_kernel   a thread per group: the range held against in_cap and
//                     2^32-1 bytes, the pieces' word counts against 2^31; the
//                     group's begin and end as the decoders take them (a
//                     refused range: empty, so nothing of it is read and no
//                     word written), the batch's packed bytes summed.
//   dat_gate_kernel   dec_gate_kernel's rule over that sum.
//   the decoders      no groups given: the batch forms on a range per piece
//                     (kAt: decode_at_kernel, decode2_at_kernel), per-XCD
//                     tickets, CPK_ETRAILING found by the record check, each
//                     piece's end written out.  Groups given: the stream forms
//                     as they stand (decode_kernel<true, ..>,
//                     decode2_kernel<true>), a wave per group, the groups
//                     largest first -- DecStreams with the gate's skip word.
//   dat_final_kernel  a thread per group: its status and the bytes consumed.
//
// The window loads read whole 16-byte lines around a piece (win_load, glim):
// with placed ranges those hold the gap's or a neighbour's bytes, as in a tiled
// batch they hold the next piece's.  Nothing parsed depends on them: the walks
// stop at wend <= P, and the one record that may take a count byte from at or
// past P is the window's last, which the record check holds against P before
// its count is believed (win_emit; decode_size.hip's header has the argument
// byte by byte).  With the buffer 16-byte aligned and every range below in_cap
// the lines stay below round_up(in_cap, 16).

// What the caller gives and the scratch the kernels share
struct DatArgs {
  const uint64_t *src_off, *src_len;  // [ng]
  const uint64_t *grp;                // [ng + 1] the groups' pieces; null: piece g is group g
  const uint64_t *swo;                // [n + 1] the pieces' words; null: the size query
  uint32_t n, ng;
  uint64_t in_cap;
  // group g's entries are at index g * gs: gs = 1, three arrays (the stream
  // forms and the size query), or gs = 3, one array of begin | end | out per
  // piece (the batch forms, DecPieces<false, true>)
  uint64_t *gbeg, *gend;              // written: the group's range as decoded (refused: empty)
  uint64_t *gout;                     // where the group's pieces ended (preset to its begin); null: the size query
  uint32_t gs;
  int32_t *gstatus;                   // [ng] written: CPK_OK or why the range is refused
};

// the pieces of group g, clamped to n for dat_prep_kernel and
// dat_final_kernel: in these two kernels offsets that are not what the contract
// asks for give wrong statuses, never an index out of range.  (The stream
// decoders read the same array unclamped, as sd.spc; there the piece loop's
// own seg >= n check keeps status and swo in range.)
__device__ __forceinline__ void dat_pieces(const DatArgs &A, uint32_t g, uint64_t &p0, uint64_t &p1) {
  p0 = g, p1 = (uint64_t)g + 1;
  if (A.grp) {
    p0 = A.grp[g] < A.n ? A.grp[g] : A.n;
    p1 = A.grp[g + 1] < A.n ? A.grp[g + 1] : A.n;
    if (p1 < p0) p1 = p0;
  }
}

constexpr int kDatThreads = 256;
// One thread per group.  psum: the accepted ranges' bytes summed (a sum per
// workgroup, one atomic each); glen: their lengths, for the largest-first
// order (null: not wanted); the size query's rows: words 0, the status, todo
// (1: us_wave_body sizes the piece).
__global__ __launch_bounds__(kDatThreads) void dat_prep_kernel(DatArgs A, unsigned long long *psum,
                                                               uint64_t *__restrict__ glen,
                                                               uint64_t *__restrict__ words,
                                                               uint32_t *__restrict__ todo) {
  __shared__ unsigned long long part[kDatThreads / 64];
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t len = 0;
  if (g < A.ng) {
    const uint64_t off = A.src_off[g];
    len = A.src_len[g];
    int st = CPK_OK;
    // (the sum saturating: off + len > in_cap without computing it)
    if (len > 0xffffffffull) st = CPK_EUNSUPPORTED;
    else if (off > A.in_cap || len > A.in_cap - off) st = CPK_EINVAL;
    if (A.swo) {
      uint64_t p0, p1;
      dat_pieces(A, g, p0, p1);
      for (uint64_t p = p0; p < p1; ++p)
        if (A.swo[p + 1] - A.swo[p] >= (1ull << 31) && st == CPK_OK) st = CPK_EINVAL;
    }
    if (st != CPK_OK) len = 0;
    const uint64_t gi = (uint64_t)g * A.gs;
    A.gbeg[gi] = st == CPK_OK ? off : 0;
    A.gend[gi] = st == CPK_OK ? off + len : 0;
    if (A.gout) A.gout[gi] = st == CPK_OK ? off : 0;
    A.gstatus[g] = st;
    if (glen) glen[g] = len;
    if (words) words[g] = 0;
    if (todo) todo[g] = st == CPK_OK ? 1u : 0u;
  }
  if (!psum) return;
  unsigned long long v = len;
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < kDatThreads / 64; ++i) t += part[i];
    if (t) atomicAdd(psum, t);
  }
}

// dec_gate_kernel's rule between the block map, the record index and the
// dense form, the packed bytes being the ranges' sum: skip[k] nonzero = form
// k returns at once.
__global__ void dat_gate_kernel(const unsigned long long *__restrict__ psum, const uint64_t *__restrict__ swo,
                                uint32_t n, uint32_t *skip) {
  if (threadIdx.x == 0) {
    const uint64_t P = *psum, U = 8 * (swo[n] - swo[0]);
    const bool v2 = 100 * P < 15 * U, dense = 100 * P >= 80 * U;
    skip[0] = (v2 || dense) ? 1u : 0u;
    skip[1] = v2 ? 0u : 1u;
    skip[2] = dense ? 0u : 1u;
  }
}

// The batch forms on a range per piece: piece i is [in_off[3 i], in_off[3 i + 1]),
// the end of a piece that is CPK_ETRAILING goes to in_off[3 i + 2].  Launch bounds, LDS and arguments are those
// of the forms they mirror.
template <bool kSerial>
__global__ __launch_bounds__(kDecThreads, kDecWpe) void decode_at_kernel(
    const uint8_t *__restrict__ packed, uint64_t *__restrict__ in_off, const uint64_t *__restrict__ swo, uint32_t n,
    uint64_t *__restrict__ out, int32_t *__restrict__ status, uint32_t *ticket, uint64_t avail, DecStreams sd) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  decode_body<false, kSerial, true>(smem, packed, in_off, swo, n, out, status, ticket, avail, sd);
}
__global__ __launch_bounds__(kD2Threads, kD2Wpe) void decode2_at_kernel(
    const uint8_t *__restrict__ packed, uint64_t *__restrict__ in_off, const uint64_t *__restrict__ swo, uint32_t n,
    uint64_t *__restrict__ out, int32_t *__restrict__ status, uint32_t *ticket, uint64_t avail, DecStreams sd) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr bool kStream = false, kAt = true;
#define CPK_DECODE_V2_BODY
#include "decode_v2_body.hip"
#undef CPK_DECODE_V2_BODY
}

// One thread per group, after the decoders.  A refused range: its status to
// the group and every piece of it.  Otherwise the group's status is its last
// piece's (a failed piece stops the group: the later ones carry its status),
// or CPK_ETRAILING when the pieces ended (gout) before the range did -- for a
// group of one piece also in the piece's status, as the batch form has it.
// used: the bytes consumed, 0 for a group that failed otherwise.
__global__ void dat_final_kernel(DatArgs A, int32_t *__restrict__ status, uint64_t *__restrict__ used) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= A.ng) return;
  uint64_t p0, p1;
  dat_pieces(A, g, p0, p1);
  int st = A.gstatus[g];
  if (st != CPK_OK) {
    for (uint64_t p = p0; p < p1; ++p) status[p] = st;
    used[g] = 0;
    return;
  }
  st = p1 > p0 ? status[p1 - 1] : CPK_OK;
  // (the batch forms, gs = 3, write a piece's end only when it is
  // CPK_ETRAILING: a CPK_OK piece ended where its range does)
  const uint64_t u = (A.gs == 3 && st == CPK_OK) ? A.src_len[g]
                                                 : A.gout[(uint64_t)g * A.gs] - A.gbeg[(uint64_t)g * A.gs];
  if (st == CPK_OK && u < A.src_len[g]) {
    st = CPK_ETRAILING;
    if (p1 - p0 == 1) status[p0] = st;
  }
  A.gstatus[g] = st;
  used[g] = (st == CPK_OK || st == CPK_ETRAILING) ? u : 0;
}

// The size query's wave-per-piece form on a range per piece: us_wave_kernel's
// loop (decode_size.hip, whose header has the end-of-piece argument) over
// [beg[i], end[i]); todo: the accepted ranges, the others keep
// dat_prep_kernel's rows.
__global__ __launch_bounds__(kUsThreads, kUsWpe) void us_wave_at_kernel(
    const uint8_t *__restrict__ packed, const uint64_t *__restrict__ beg, const uint64_t *__restrict__ end, uint32_t n,
    uint64_t *__restrict__ words, int32_t *__restrict__ status, uint32_t *ticket, const uint32_t *__restrict__ todo) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  uint8_t *wbuf = smem + wave_id() * kUsWaveLds;
  VisMask *visa = reinterpret_cast<VisMask *>(wbuf + UsGeom::buf);
  UsPieces pc(ticket, n);
  for (;;) {
    const uint32_t seg = pc.next();
    if (seg >= n) break;
    if (__builtin_amdgcn_readfirstlane((int)todo[seg]) == 0) continue;
    const uint64_t a = rfl64(beg[seg]);
    const uint32_t P = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(end[seg] - a));  // (<= 2^32-1)
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
