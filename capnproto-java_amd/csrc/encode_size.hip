// encode_size.hip -- the exact packed size of every piece of a batch without
// encoding it (cpk_packed_size_batch / cpk_packed_size_messages).  Included
// from packed_codec.hip (namespace cpk) after encode_v4.hip and encode_sp.hip:
// it uses their device helpers and the role algebra of sp_roles.hip, and
// leaves their kernels as they are.
//
// A read-only pass: device traffic is the unpacked words plus the offsets.
// Two forms, chosen on the device from the piece sizes (sz_gate_kernel; no
// density sample: nothing is emitted, so no ring can overflow):
//   wave per piece   e4_size_kernel<false> (encode_v4.hip): the two-pass
//                    encoder's size walk without its boundary rows.  Small
//                    and mixed pieces, and the segments of message batches.
//   chunk parallel   sz_chunk_kernel below: a workgroup per 8192-word unit
//                    from the in-order ticket runs the single pass's A1
//                    (loads, tags, Z / DL / D ballots, masks to LDS) and A2
//                    (sp_a2p / sp_a2_seq: sp_roles and the popcounts) and
//                    nothing of B: no rings, no look-back for offsets, no
//                    word kept after its ballots.  Batches with a piece of
//                    over one chunk that is far larger than the rest (or
//                    few pieces): a wave would walk it alone.
// The run state crossing a chunk boundary inside a piece is handed over as
// sp_chunk (encode_sp.hip) hands it: the state a chunk leaves is published in
// the unit's epoch-tagged status word -- early, before the chunk waits, when
// it does not depend on the state entering the chunk -- and a chunk that
// continues a piece waits for its predecessor unit's word (an earlier ticket:
// resident and running), in a bounded spin that sets the context's error bit.
// A unit's bytes are added to its piece's size (integer atomics on a u64:
// exact in any order); e4_scan_* turns the sizes into offsets.

constexpr int kSzWpe = 8;  // workgroups per CU (4 waves each: 8 waves per SIMD, <= 64 VGPRs)
constexpr int kSzA1G = 8;  // steps whose loads A1 keeps in flight per group (as e4_size_kernel's PF)
static_assert(kSpWS % kSzA1G == 0, "A1 groups");

// A1 without the words or their tags kept: the wave's cnt steps at src (wrem
// piece words from src on), their Z / DL / D ballots stashed lane = step;
// returns this lane's nonzero-byte count.  kFull: kSpWS whole steps.
// (sp_a1's reload form with nontemporal loads: U is not read again)
template <bool kFull>
__device__ __forceinline__ uint32_t sz_a1(SpStash &R, const uint64_t *__restrict__ src, uint32_t wrem, int cnt,
                                          int lane) {
  constexpr int G = kSzA1G;
  uint64_t v[2][G];
  // loads clamped to the piece, not predicated (sp_a1)
  auto ld = [&](int j) __attribute__((always_inline)) -> uint64_t {
    return ld_stream(&(src + j * 64)[kFull ? (uint32_t)lane : min((uint32_t)lane, min(wrem - 1 - 64u * j, 63u))]);
  };
#pragma unroll
  for (int i = 0; i < G; ++i)
    if (kFull || i < cnt) v[0][i] = ld(i);
  uint32_t acc = 0;
#pragma unroll
  for (int g = 0; g < kSpWS / G; ++g) {
    if (g + 1 < kSpWS / G) {
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const int j = (g + 1) * G + i;
        if (kFull || j < cnt) v[(g + 1) & 1][i] = ld(j);
      }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int j = g * G + i;
      if (kFull || j < cnt) {
        const bool valid = kFull || (uint32_t)lane < wrem - 64u * j;
        const uint32_t m = valid ? e4_tag(v[g & 1][i]) : 0u;
        const uint32_t pc = (uint32_t)__builtin_popcount(m);
        acc += pc;
        const uint64_t Z = __ballot(valid && m == 0), DL = __ballot(pc >= 7), D = __ballot(m == 0xffu);
        R.zl = sp_wl(R.zl, (uint32_t)Z, j);
        R.zh = sp_wl(R.zh, (uint32_t)(Z >> 32), j);
        R.dll = sp_wl(R.dll, (uint32_t)DL, j);
        R.dlh = sp_wl(R.dlh, (uint32_t)(DL >> 32), j);
        R.dl_ = sp_wl(R.dl_, (uint32_t)D, j);
        R.dh_ = sp_wl(R.dh_, (uint32_t)(D >> 32), j);
      }
    }
    CPK_SP_STEP_FENCE();
  }
  return acc;
}

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
    const uint32_t ns = (W + 63) >> 6;
    const uint32_t nch = max((ns + kSpCS - 1) / kSpCS, 1u);
    const uint32_t cs0 = c * kSpCS;
    const int cs = c < nch ? (int)min((uint32_t)kSpCS, ns - cs0) : 0;  // steps in this chunk
    uint64_t *prev = c ? ustate + (t - 1) : nullptr;
    uint64_t *next = c + 1 >= nch ? nullptr : ustate + t;
    // the chunk's steps spread over the waves (sp_chunk)
    const int per = min(kSpWS, ((cs + kSpWaves - 1) / kSpWaves + 1) & ~1);
    const int sa = w * per;
    const int cnt = max(0, min(per, cs - sa));
    const uint32_t wfirst = (cs0 + (uint32_t)sa) * 64;  // the wave's first word
    const uint32_t wrem = cnt ? W - wfirst : 0;
    uint32_t acc = 0;
    if (cnt) {
      if (cnt == kSpWS && wrem >= 64u * kSpWS) acc = sz_a1<true>(R, pw + wfirst, wrem, cnt, lane);
      else
        acc = sz_a1<false>(R, pw + wfirst, wrem, cnt, lane);
      sp_put_masks(R, msk, sa, cnt, lane);
    }
    __syncthreads();  // the chunk's masks in LDS
    SpSt cst = {0u, 0u, 0u};
    const bool last = cnt && sa + cnt == cs;  // this wave holds the chunk's last step
    // the state leaving the chunk, published before this chunk waits for its
    // own entering state unless it depends on that (a zero run or D/L stretch
    // over the whole chunk): the chunks of a piece do not wait in a chain
    bool early = false;
    if (next && last) {
      bool dep = false;
      const SpSt ex = sp_state_at(msk, cs, cst, dep);
      if (!dep) {
        early = true;
        if (lane == 0) st_status(next, sp_word(ep, 2u, sp_pack_state(ex)));
      }
    }
    if (prev) {
      // the predecessor chunk holds an earlier ticket, so it is resident and
      // running, and publishes after its own masks are in LDS
      if (threadIdx.x == 0) {
        uint32_t spins = 0;
        uint64_t v;
        while (sp_flag(v = ld_status(prev), ep) != 2u) {
          if (++spins > (1u << 24)) {  // cannot happen: see above
            atomicOr(err, kErrWait);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        scr[1] = v & kSpValMask;
      }
      __syncthreads();
      cst = sp_unpack_state(sp_ld(&scr[1]));
    }
    if (cnt) {
      bool dep_ = false;
      const SpSt st = sp_state_at(msk, sa, cst, dep_);
      // (no run ends for an emit pass: the step after the wave's last is not looked at)
      uint32_t rb = 0;
      if (!sp_a2p(R, cnt, wrem, st, 0u, 0u, lane, rb)) rb = sp_a2_seq(R, cnt, wrem, st, 0u, 0u);
      const uint32_t bytes = rb + (uint32_t)__builtin_amdgcn_readlane(wave_incl_add((int)acc), 63);
      if (lane == 0 && bytes) atomicAdd(&sizes[p], (unsigned long long)bytes);
    }
    if (last && next && !early) {
      bool dep_ = false;
      const SpSt ex = sp_state_at(msk, cs, cst, dep_);
      if (lane == 0) st_status(next, sp_word(ep, 2u, sp_pack_state(ex)));
    }
  }
}

// Which form sizes the batch, from the min / max piece words
// (e4_minmax_kernel without its sample: tickets[kTkGate], [kTkGate + 1]):
// the chunk-parallel form for batches with a piece of over one 8192-word unit
// and at least 1/2048 of the batch's words (a wave would walk it alone long
// after the rest is done: the encode gate's rule for one dominant piece,
// e4_gate_kernel), the wave per piece otherwise.  Like-sized pieces of one
// chunk stay with the wave walk: measured on 64 KiB pieces (1 Mi pieces,
// configs 2 / 3 / 4) the chunk form takes 14.87 / 14.85 / 14.88 ms against
// the walk's 11.39 / 11.00 / 11.19 -- its barriers and ordered ticket buy
// nothing when every wave has a piece of its own.
// The form not picked returns at once: the wave walk reads
// tickets[kTkGate + 2], the chunk form finds its ordered ticket exhausted.
// can_chunk: the chunk form was enqueued at all; force: 1 chunk form, 2 wave
// per piece (CPK_SIZE_FORM).
__global__ void sz_gate_kernel(uint32_t *tickets, const uint64_t *swo, uint32_t n, uint32_t can_chunk,
                               uint32_t force) {
  const uint32_t hi = tickets[kTkGate + 1];
  const uint64_t total = swo[n] - swo[0];
  const bool big = hi > 8192u && (uint64_t)hi * 2048u >= total;
  const bool chunk = can_chunk && (force ? force == 1u : big);
  if (threadIdx.x == 0) {
    tickets[kTkGate + 2] = chunk ? 1u : 0u;
    tickets[kTkPlan] = chunk ? 0u : 0x7fffffffu;
  }
}
