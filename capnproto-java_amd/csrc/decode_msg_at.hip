// decode_msg_at.hip -- packed messages decoded from the byte ranges the caller
// names (cpk_decode_messages_at): cpk_decode_messages' framing on
// cpk_decode_batch_at's ranges, with the capacity verdict made on the device,
// so the call never returns to the host between the table pass and the
// decode.  Included from packed_codec.hip (namespace cpk) after decode_at.hip.
// Nothing of the framing or the decoders is restated: the tables are read by
// read_table, the segments by the stream forms as they stand
// (decode_kernel<true, ..>, decode2_kernel<true>), a wave per message, the
// messages largest first.
//
//   mat_table_kernel  a thread per message: dat_prep_kernel's range rule, then
//                     read_table over the range; the message's words, segment
//                     count, first segment byte, range end and status.  A
//                     message whose range and table are good is accepted.
//   two scans         over the accepted messages' words and segment counts.
//   mat_fit_kernel    a thread per message: it fits iff its own inclusive sums
//                     end at or below the capacities (the sums are monotone:
//                     the test is local and the fitting messages a prefix of
//                     the accepted ones); the first message that does not
//                     (one atomicMin per workgroup), the fitting messages
//                     counted and their ranges' bytes summed (an atomic each
//                     per workgroup) -- the sum the gate needs is that of the
//                     messages that are decoded, so it is taken here and not
//                     in the table pass.
//   mat_place_kernel  a thread per message: F, the segments' end of the last
//                     fitting message; d_totals; the decoders' piece ranges
//                     (the scanned counts clamped at F: a message that is
//                     refused, failed or does not fit has no pieces and an
//                     empty stream); CPK_ENOMEM; the fitting messages' tables
//                     read again for the segments' word offsets, as
//                     msg_swo_kernel reads them.
//   dat_gate_kernel   as it stands, over the fitting messages' bytes and words.
//   the decoders      DecStreams{first segment byte, range end, piece ranges};
//                     n = seg_cap for the piece loop's own seg >= n check.
//   mat_final_kernel  a thread per message: the status by precedence and the
//                     bytes consumed.
//
// The reads stay below round_up(in_cap, 16) as decode_at.hip's header argues:
// read_table reads bytes of the range only, the windows whole 16-byte lines
// around it.

constexpr int kMatThreads = 256;
// the fit pass's words: the first message that does not fit (preset to all
// ones), the messages that fit, their ranges' bytes; the gate's two word
// offsets (0, the fitting messages' words)
constexpr int kMatNoFit = 0, kMatCount = 1, kMatBytes = 2, kMatGate = 3, kMatWords = 5;

__global__ __launch_bounds__(kMatThreads) void mat_table_kernel(
    const uint8_t *__restrict__ packed, const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
    uint32_t nm, uint64_t in_cap, uint64_t limit, uint64_t *__restrict__ mwords, uint64_t *__restrict__ mcount,
    uint64_t *__restrict__ mbeg, uint64_t *__restrict__ mend, int32_t *__restrict__ mstatus) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const uint64_t off = src_off[m], len = src_len[m];
  int st = CPK_OK;
  // (dat_prep_kernel's rule, the sum saturating: off + len > in_cap without computing it)
  if (len > 0xffffffffull) st = CPK_EUNSUPPORTED;
  else if (off > in_cap || len > in_cap - off) st = CPK_EINVAL;
  uint64_t ip = 0, total = 0;
  uint32_t count = 0;
  if (st == CPK_OK) st = read_table(packed + off, len, limit, ip, count, total, [](uint32_t, uint32_t) {});
  const bool ok = st == CPK_OK;
  mstatus[m] = st;
  mwords[m] = ok ? total : 0;
  mcount[m] = ok ? count : 0;
  mbeg[m] = ok ? off + ip : 0;
  mend[m] = ok ? off + len : 0;
}

// mwoff, msoff: the scans of the accepted messages' words and segment counts
__global__ __launch_bounds__(kMatThreads) void mat_fit_kernel(
    uint32_t nm, const uint64_t *__restrict__ mwoff, const uint64_t *__restrict__ msoff,
    const uint64_t *__restrict__ src_len, const int32_t *__restrict__ mstatus, uint64_t out_cap, uint64_t seg_cap,
    unsigned long long *fit) {
  __shared__ unsigned long long part[3][kMatThreads / 64];
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long first = ~0ull, cnt = 0, bytes = 0;
  if (m < nm) {
    // (the first message whose sums pass a capacity is an accepted one: a
    // message that is not adds nothing to them)
    const bool fits = mwoff[m + 1] <= out_cap && msoff[m + 1] <= seg_cap;
    if (!fits) first = m;
    if (fits && mstatus[m] == CPK_OK) cnt = 1, bytes = src_len[m];
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(first, d, 64);
    first = o < first ? o : first;
    cnt += __shfl_xor(cnt, d, 64);
    bytes += __shfl_xor(bytes, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = first;
    part[1][threadIdx.x >> 6] = cnt;
    part[2][threadIdx.x >> 6] = bytes;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    first = ~0ull, cnt = 0, bytes = 0;
    for (int i = 0; i < kMatThreads / 64; ++i) {
      first = part[0][i] < first ? part[0][i] : first;
      cnt += part[1][i];
      bytes += part[2][i];
    }
    if (first != ~0ull) atomicMin(&fit[kMatNoFit], first);
    if (cnt) atomicAdd(&fit[kMatCount], cnt);
    if (bytes) atomicAdd(&fit[kMatBytes], bytes);
  }
}

// Threads 0 .. nm: thread nm writes the call's totals and the arrays' ends.
// swo, sin: d_seg_word_off and d_seg_in_off (null with seg_cap 0: then no
// message fits and neither is touched).
__global__ __launch_bounds__(kMatThreads) void mat_place_kernel(
    const uint8_t *__restrict__ packed, const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
    uint32_t nm, uint64_t limit, const uint64_t *__restrict__ mwoff, const uint64_t *__restrict__ msoff,
    uint64_t *__restrict__ fit, uint64_t *__restrict__ mbeg, uint64_t *__restrict__ mend,
    uint64_t *__restrict__ spc, int32_t *__restrict__ mstatus, uint64_t *__restrict__ swo,
    uint64_t *__restrict__ sin, uint64_t *__restrict__ totals) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m > nm) return;
  const uint64_t x = fit[kMatNoFit] < nm ? fit[kMatNoFit] : nm;  // the fitting messages are those accepted below x
  const uint64_t F = msoff[x];
  spc[m] = msoff[m] < F ? msoff[m] : F;
  if (m == nm) {
    totals[0] = mwoff[nm];
    totals[1] = msoff[nm];
    totals[2] = fit[kMatCount];
    fit[kMatGate] = 0;
    fit[kMatGate + 1] = mwoff[x];
    if (swo) swo[F] = mwoff[x];
    return;
  }
  if (mstatus[m] != CPK_OK) return;
  if (m >= x) {
    mstatus[m] = CPK_ENOMEM;
    mbeg[m] = mend[m] = 0;
    return;
  }
  const uint64_t a = src_off[m], s0 = msoff[m];
  uint64_t ip = 0, total = 0, acc = mwoff[m];
  uint32_t count = 0;
  read_table(packed + a, src_len[m], limit, ip, count, total, [&](uint32_t i, uint32_t sz) {
    swo[s0 + i] = acc;
    sin[s0 + i] = 0;  // (the decoders write a segment's start when they reach it)
    acc += sz;
  });
}

// The precedence: the range's status, the table's, CPK_ENOMEM (all three in
// mstatus by now), the first failed segment's (a failure stops the stream: the
// message's last segment carries it), CPK_ETRAILING when the segments ended
// (mout) before the range did, CPK_OK.  used: the bytes consumed, table and
// segments, 0 for a message that failed otherwise.
__global__ __launch_bounds__(kMatThreads) void mat_final_kernel(
    uint32_t nm, const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
    const uint64_t *__restrict__ spc, const uint64_t *__restrict__ mout, const int32_t *__restrict__ seg_status,
    int32_t *__restrict__ mstatus, uint64_t *__restrict__ used) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  uint64_t u = 0;
  if (mstatus[m] == CPK_OK) {  // (a fitting message: it has a segment at least)
    int st = seg_status[spc[m + 1] - 1];
    u = mout[m] - src_off[m];
    if (st == CPK_OK && u < src_len[m]) st = CPK_ETRAILING;
    if (st != CPK_OK && st != CPK_ETRAILING) u = 0;
    mstatus[m] = st;
  }
  used[m] = u;
}
