// encode_size.hip -- the exact packed size of every piece of a batch without
// encoding it (cpk_packed_size_batch / cpk_packed_size_messages).  Included
// from packed_codec.hip (namespace cpk) after encode_v4.hip, sp_chunk.hip and
// encode_sp.hip: it uses their device helpers and leaves their kernels as
// they are.
//
// A read-only pass: device traffic is the unpacked words plus the offsets.
// Two forms, chosen on the device from the piece sizes (sz_gate_kernel; no
// density sample: nothing is emitted, so no ring can overflow):
//   wave per piece   e4_size_kernel<false> (encode_v4.hip): the two-pass
//                    encoder's size walk without its boundary rows.  Small
//                    and mixed pieces, and the segments of message batches.
//   chunk parallel   sz_chunk_kernel below: a workgroup per 8192-word unit
//                    from the in-order ticket runs the chunk algebra and the
//                    hand-over of sp_chunk.hip and nothing of B: no rings, no
//                    look-back for offsets, no word, tag or run end kept.
//                    Batches with a piece of over one chunk that is far
//                    larger than the rest (or few pieces): a wave would walk
//                    it alone.
// A unit's bytes are added to its piece's size (integer atomics on a u64:
// exact in any order); e4_scan_* turns the sizes into offsets.

constexpr int kSzWpe = 8;  // workgroups per CU (4 waves each: 8 waves per SIMD, <= 64 VGPRs)
// A1's load policy (sp_a1_reload): nontemporal loads (U is not read again),
// no tags kept
struct SzForm {
  static constexpr int kA1G = 8;  // steps in flight per group (as e4_size_kernel's PF)
  static constexpr bool kA1Stream = true;
  static constexpr bool kA1Tags = false;
};

// Units as sp_encode_kernel's: utab[u] = piece << 32 | chunk, *nunits of them
// (utab == nullptr: every piece is one chunk, unit = piece); ustate[u]: the
// run state unit u leaves for unit u + 1 of the same piece.  sizes[] is
// zeroed by the host; a piece the form cannot take (2^31 words or more, over
// the hint) is reported and sized 0, as the encoder sizes it.
__global__ __launch_bounds__(kSpThreads, kSzWpe) void sz_chunk_kernel(
    const uint64_t *__restrict__ in, const uint64_t *__restrict__ swo, uint32_t n,
    unsigned long long *__restrict__ sizes, uint32_t *ticket, const uint64_t *__restrict__ utab,
    const uint64_t *__restrict__ nunits, uint64_t *ustate, uint32_t ep, uint64_t hint, uint32_t *err) {
  __shared__ uint64_t msk[3 * kSpCS];  // the chunk's masks, u64[kSpCS][3]
  __shared__ uint64_t scr[2];          // [0] ticket, [1] the state entering the chunk
  const int lane0 = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  SpStash R;
  R.zl = R.zh = R.dll = R.dlh = R.dl_ = R.dh_ = 0;
  R.oml = R.omh = R.ohl = R.ohh = R.oel = R.oeh = 0;
  const uint32_t nu = utab ? (uint32_t)*nunits : n;
  for (;;) {
    if (threadIdx.x == 0) scr[0] = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t t = (uint32_t)sp_ld(&scr[0]);
    __syncthreads();  // (scr[0] and the last unit's masks read by all before the next ticket)
    if (t >= nu) break;
    const uint64_t ud = utab ? utab[t] : (uint64_t)t << 32;
    const uint32_t p = (uint32_t)(ud >> 32), c = (uint32_t)ud;
    int lane = lane0;
    asm volatile("" : "+v"(lane));  // (nothing lane-dependent hoisted out of the unit loop)
    const uint64_t w0 = swo[p], W64 = swo[p + 1] - w0;
    // (with a unit table, a piece over the hint is one empty unit:
    // sp_units_count_kernel)
    const bool bad = W64 >= (1ull << 31) || (!utab && W64 > 64ull * kSpCS) || (utab && hint && W64 > hint);
    if ((bad || (hint && W64 > hint)) && threadIdx.x == 0 && c == 0) atomicOr(err, kErrHint);
    const uint32_t W = bad ? 0u : (uint32_t)W64;
    const uint64_t *pw = in + w0;
    const SpGeom g = sp_geom(W, c, w);
    SpHandover h = {c ? ustate + (t - 1) : nullptr, g.lastc ? nullptr : ustate + t, ep, err};
    uint32_t acc = 0;
    if (g.cnt) {
      acc = g.full() ? sp_a1_reload<SzForm, true>(R, pw + g.wfirst, g.wrem, g.cnt, lane)
                     : sp_a1_reload<SzForm, false>(R, pw + g.wfirst, g.wrem, g.cnt, lane);
      sp_put_masks(R, msk, g.sa, g.cnt, lane);
    }
    __syncthreads();  // the chunk's masks in LDS
    h.publish_early(msk, g, lane);
    SpSt cst = {0u, 0u, 0u};
    if (h.prev) cst = h.wait<false>(0, &scr[1]);
    if (g.cnt) {
      bool dep_ = false;
      const SpSt st = sp_state_at(msk, g.sa, cst, dep_);
      // (no run ends for an emit pass: the step after the wave's last is not looked at)
      const uint32_t bytes = sp_a2(R, g.cnt, g.wrem, st, 0u, 0u, lane) +
                             (uint32_t)__builtin_amdgcn_readlane(wave_incl_add((int)acc), 63);
      if (lane == 0 && bytes) atomicAdd(&sizes[p], (unsigned long long)bytes);
    }
    h.publish_late(msk, g, cst, lane);
  }
}

// Which form sizes the batch, from the min / max piece words
// (e4_minmax_kernel without its sample: tickets[kTkGate + kGateMin], [kTkGate + kGateMax]):
// the chunk-parallel form for batches with a piece of over one 8192-word unit
// and at least 1/2048 of the batch's words (a wave would walk it alone long
// after the rest is done: the encode gate's rule for one dominant piece,
// e4_gate_kernel), the wave per piece otherwise.  Like-sized pieces of one
// chunk stay with the wave walk: measured on 64 KiB pieces (1 Mi pieces,
// configs 2 / 3 / 4) the chunk form takes 14.87 / 14.85 / 14.88 ms against
// the walk's 11.39 / 11.00 / 11.19 -- its barriers and ordered ticket buy
// nothing when every wave has a piece of its own.
// The form not picked returns at once: the wave walk reads
// tickets[kTkGate + kGatePick], the chunk form finds its ordered ticket exhausted.
// can_chunk: the chunk form was enqueued at all; force: 1 chunk form, 2 wave
// per piece (CPK_SIZE_FORM).
__global__ void sz_gate_kernel(uint32_t *tickets, const uint64_t *swo, uint32_t n, uint32_t can_chunk,
                               uint32_t force) {
  const uint32_t hi = tickets[kTkGate + kGateMax];
  const uint64_t total = swo[n] - swo[0];
  const bool big = hi > 8192u && (uint64_t)hi * 2048u >= total;
  const bool chunk = can_chunk && (force ? force == 1u : big);
  if (threadIdx.x == 0) {
    tickets[kTkGate + kGatePick] = chunk ? 1u : 0u;
    tickets[kTkPlan] = chunk ? 0u : 0x7fffffffu;
  }
}
