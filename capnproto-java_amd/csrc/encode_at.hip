// encode_at.hip -- the single pass with the output placed by the caller
// (cpk_encode_batch_at).  Included from packed_codec.hip (namespace cpk) after
// sp_chunk.hip and encode_sp.hip: it runs their shared text -- the unit
// tickets and unit table, SpGeom, sp_a1_*, sp_put_masks, SpHandover, sp_a2,
// sp_wave_bytes, sp_b with its rings, sp_lookback -- and changes none of it.
//
// Pieces come in groups (a message: its table piece, then its segments); a
// group's pieces are packed back to back from the byte the caller names,
// d_out + dst_off[g], into a slot of dst_cap[g] bytes.  What is new against
// sp_encode_kernel is where a unit's base comes from: the group's offset plus
// the bytes of the group's units before this one, found by a look-back over
// the status words that stops at the group's first unit.  That unit knows its
// base from the start (sp_b's `known`): a group of one piece of at most one
// chunk does no look-back and none of its waves waits for an offset.
//
// The slot's end, min(dst_off + dst_cap, out_cap), is sp_b's ocap: no line or
// byte at or past it is stored, and sp_b stores a wave's own bytes only (whole
// 16-byte lines of them at any alignment, the last partial line by bytes), so
// nothing outside a group's packed bytes is written -- not the gap between
// two slots, not the rest of a 16-byte line the group starts or ends in.

// A1's load policy for the form whose B reads the words again
// (sp_a1_reload): as sp_encode_kernel's, plain loads (B finds the lines in
// L2), the tags kept
template <class F>
struct AtA1 {
  static constexpr int kA1G = F::kA1G;
  static constexpr bool kA1Stream = false;
  static constexpr bool kA1Tags = true;
};

// the wave's words into registers (the form that keeps them for B), every
// load in flight at once; clamped to the piece, not predicated
template <bool kFull>
__device__ __forceinline__ void at_load(uint64_t (&V)[kSpWS], const uint64_t *__restrict__ src, uint32_t wrem,
                                        int cnt, int lane) {
  __builtin_amdgcn_s_setprio(1);  // (the loads out first)
#pragma unroll
  for (int j = 0; j < kSpWS; ++j)
    if (kFull || j < cnt)
      V[j] = ld_stream(&(src + j * 64)[kFull ? (uint32_t)lane : min((uint32_t)lane, min(wrem - 1 - 64u * j, 63u))]);
  __builtin_amdgcn_s_setprio(0);
}

// A of one unit (all waves; two barriers, three when the chunk continues a
// piece): sp_chunk.hip's sequence.  Returns the chunk's packed bytes;
// wbefore / wmine: bytes of the waves before this one / of this one.
template <class F>
__device__ __forceinline__ uint64_t at_chunk(SpRegs<F> &R, const uint64_t *__restrict__ pw, uint32_t W,
                                             const SpGeom &g, uint64_t *msk, uint64_t *scr, SpHandover h, int w,
                                             int lane, uint64_t &wbefore, uint64_t &wmine) {
  uint32_t acc = 0;
  if (g.cnt) {
    const uint64_t *src = pw + g.wfirst;
    if constexpr (F::kReload) {
      acc = g.full() ? sp_a1_reload<AtA1<F>, true>(R, src, g.wrem, g.cnt, lane)
                     : sp_a1_reload<AtA1<F>, false>(R, src, g.wrem, g.cnt, lane);
    } else {
      if (g.full()) {
        at_load<true>(R.v, src, g.wrem, g.cnt, lane);
        acc = sp_a1_regs<true>(R, R.v, g.wrem, g.cnt, lane);
      } else {
        at_load<false>(R.v, src, g.wrem, g.cnt, lane);
        acc = sp_a1_regs<false>(R, R.v, g.wrem, g.cnt, lane);
      }
    }
    sp_put_masks(R, msk, g.sa, g.cnt, lane);
  }
  __syncthreads();  // the chunk's masks in LDS
  h.publish_early(msk, g, lane);
  SpSt cst = {0u, 0u, 0u};
  if (h.prev) cst = h.wait<false>(0, &scr[12]);
  uint32_t bytes = 0;
  if (g.cnt) {
    bool dep_ = false;
    const SpSt st = sp_state_at(msk, g.sa, cst, dep_);
    uint32_t nz0, ndl0, Xlast;
    const uint64_t *la = pw + g.wend();
    auto la_word = [&](int j) __attribute__((always_inline)) { return (la + 64 * j)[lane]; };
    sp_next_step(R, msk, g, W, lane, la_word, nz0, ndl0, Xlast);
    const uint32_t rb = sp_a2(R, g.cnt, g.wrem, st, nz0, ndl0, lane);
    sp_xs(R, g.cnt, Xlast, lane);
    bytes = rb + (uint32_t)__builtin_amdgcn_readlane(wave_incl_add((int)acc), 63);
  }
  h.publish_late(msk, g, cst, lane);
  return sp_wave_bytes(scr, bytes, w, lane, wbefore, wmine);
}

// What the caller places, as the kernels take it
static_assert((CPK_EINVAL | CPK_ENOMEM) == CPK_EINVAL && CPK_OK == 0, "statuses OR-ed into d_status");
struct AtArgs {
  const uint64_t *in, *swo;  // the pieces: words [swo[p], swo[p + 1]) of in
  uint32_t n, ng;
  uint8_t *out;
  uint64_t out_cap;
  const uint64_t *dst_off;   // [ng] the group's first byte in out
  const uint64_t *dst_cap;   // [ng] its slot's bytes; null: to out_cap
  const uint32_t *pgrp;      // [n] the piece's group (at_prep_kernel); null: piece p is group p
  const uint64_t *gfirst;    // [ng + 1] the group's first unit; null: group g is unit g
  uint64_t *piece_off;       // [n] written: the piece's first byte in out
  uint64_t *grp_len;         // [ng] written: the group's packed bytes
  int32_t *gstatus;          // [ng] written
};

// the slot's end: no byte of the group at or past it
__device__ __forceinline__ uint64_t at_slot_end(const AtArgs &A, uint32_t g, uint64_t d0) {
  if (!A.dst_cap) return A.out_cap;
  const uint64_t cap = A.dst_cap[g];
  const uint64_t e = cap > ~d0 ? ~(uint64_t)0 : d0 + cap;  // (saturating)
  return e < A.out_cap ? e : A.out_cap;
}

// One thread per group: each piece's group and the group's first unit (when
// the caller gave groups: grp[ng + 1], ustart the pieces' first units or null:
// unit = piece), the group's status -- CPK_ENOMEM at once for a slot that
// passes out_cap (the kernel ORs its findings in) -- and the length of a group without pieces (the others' is
// written by their last unit).  Piece indices are clamped to n: offsets that
// are not what the contract asks for give wrong bytes, never an index out of
// range (pgrp is preset to ~0: a piece of no group is skipped).
__global__ void at_prep_kernel(AtArgs A, const uint64_t *__restrict__ grp, const uint64_t *__restrict__ ustart,
                               uint32_t *__restrict__ pgrp, uint64_t *__restrict__ gfirst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= A.ng) return;
  uint64_t a = g, b = (uint64_t)g + 1;
  if (grp) {
    a = grp[g] < A.n ? grp[g] : A.n;
    b = grp[g + 1] < A.n ? grp[g + 1] : A.n;
    for (uint64_t p = a; p < b; ++p) pgrp[p] = g;
    if (gfirst) {  // (null: a call without pieces)
      gfirst[g] = ustart ? ustart[a] : a;
      if (g + 1 == A.ng) gfirst[A.ng] = ustart ? ustart[b] : b;
    }
  }
  const uint64_t d0 = A.dst_off[g];
  const bool passes = d0 > A.out_cap || (A.dst_cap && A.dst_cap[g] > A.out_cap - d0);
  A.gstatus[g] = passes ? CPK_ENOMEM : CPK_OK;
  if (a >= b) A.grp_len[g] = 0;
}

// Which form places the batch: the sparse one for batches whose sampled words
// are >= 85 % zero (e4_gate_kernel's rule, from e4_minmax_kernel's sample:
// tickets[kTkGate + kGateZero]); force: 1 dense, 2 sparse (CPK_AT_FORM).  The
// ordered ticket starts at 0; the form not picked returns at once.
__global__ void at_gate_kernel(uint32_t *tickets, uint32_t samples, uint32_t force) {
  const bool sparse = force ? force == 2u : (uint64_t)tickets[kTkGate + kGateZero] * 100u >= (uint64_t)samples * 85u;
  if (threadIdx.x == 0) {
    tickets[kTkGate + kGateSparse] = sparse ? 1u : 0u;
    tickets[kTkPlan] = 0u;
  }
}

// Units and tickets as sp_encode_kernel's (utab[u] = piece << 32 | chunk,
// *nunits of them; utab == nullptr: unit = piece), the status words and run
// states of the same plan (sp_plan).  Unit t of group g, whose units are
// [gfirst[g], gfirst[g + 1]): its base is dst_off[g] + the bytes of units
// [gfirst[g], t), from sp_lookback over status + gfirst[g]; the group's first
// unit publishes inclusive at once and has its base from the start.
// LDS and scratch words as sp_encode_kernel's.
template <class F>
__global__ __launch_bounds__(kSpThreads, F::kWpe) void sp_place_kernel(
    AtArgs A, uint64_t *status, uint32_t ep, uint32_t *ticket, const uint64_t *__restrict__ utab,
    const uint64_t *__restrict__ nunits, uint64_t *ustate, uint64_t hint, uint32_t *err, const uint32_t *pick,
    uint32_t mine) {
  using L = SpLay<F>;
  // (pick: the device gate's choice between this form and the other one)
  if ((uint32_t)__builtin_amdgcn_readfirstlane((int)*pick) != mine) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint64_t *lut = reinterpret_cast<uint64_t *>(smem + kSpoLut);
  uint64_t *msk = reinterpret_cast<uint64_t *>(smem + kSpoMsk);
  uint64_t *scr = reinterpret_cast<uint64_t *>(smem + L::kScr);
  const int lane0 = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  uint32_t *ring = reinterpret_cast<uint32_t *>(smem + kSpoRing + w * L::kRingStride);
  fill_luts(lut, false);
  for (uint32_t i = lane0; i < L::kRingStride / 16; i += 64)
    reinterpret_cast<uint4 *>(ring)[i] = make_uint4(0u, 0u, 0u, 0u);
  SpRegs<F> R;
  R.zl = R.zh = R.dll = R.dlh = R.dl_ = R.dh_ = 0;
  R.oml = R.omh = R.ohl = R.ohh = R.oel = R.oeh = 0;
  if (threadIdx.x == 0) scr[11] = 0;  // (LDS holds whatever the last kernel left)
  const uint32_t nu = utab ? (uint32_t)*nunits : A.n;
  for (;;) {
    if (threadIdx.x == 0) scr[0] = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t t = (uint32_t)sp_ld(&scr[0]);
    __syncthreads();  // (scr[0] read by all before the next ticket)
    if (t >= nu) break;
    const uint64_t ud = utab ? utab[t] : (uint64_t)t << 32;
    const uint32_t p = (uint32_t)(ud >> 32), c = (uint32_t)ud;
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(A.pgrp ? A.pgrp[p] : p));
    if (g >= A.ng) continue;  // (a piece of no group: offsets the contract excludes)
    int lane = lane0;
    asm volatile("" : "+v"(lane));  // (nothing lane-dependent hoisted out of the unit loop)
    const uint32_t u0 = A.gfirst ? (uint32_t)A.gfirst[g] : g;
    const uint32_t u1 = A.gfirst ? (uint32_t)A.gfirst[g + 1] : g + 1;
    const uint64_t d0 = sp_uni(A.dst_off[g]);
    const uint64_t send = sp_uni(at_slot_end(A, g, d0));
    const uint64_t sb = d0 < send ? d0 : send;  // (a slot that starts past out_cap: nothing of it is stored)
    const uint64_t w0 = A.swo[p], W64 = A.swo[p + 1] - w0;
    // a piece the kernel cannot take, or over the caller's bound: sized 0,
    // the group CPK_EINVAL (with a unit table it is one empty unit:
    // sp_units_count_kernel)
    const bool bad = W64 >= (1ull << 31) || (!utab && W64 > 64ull * kSpCS) || (hint && W64 > hint);
    // (the statuses are OR-ed in: CPK_EINVAL = -1 covers CPK_ENOMEM = -5)
    if (bad && threadIdx.x == 0 && c == 0) atomicOr(&A.gstatus[g], (int32_t)CPK_EINVAL);
    const uint32_t W = bad ? 0u : (uint32_t)W64;
    const uint64_t *pw = A.in + w0;
    const SpGeom gm = sp_geom(W, c, w);
    uint64_t wbefore = 0, wmine = 0;
    const uint64_t ct = at_chunk<F>(R, pw, W, gm, msk, scr,
                                    SpHandover{c ? ustate + (t - 1) : nullptr, gm.lastc ? nullptr : ustate + t, ep, err},
                                    w, lane, wbefore, wmine);
    const bool first = t == u0;  // the group's first unit: its base is the slot's
    // the unit's size, published before its strings are laid out, for the
    // group's later units (a group of one unit has none)
    if (w == 0 && lane == 0 && u1 - u0 > 1u) st_status(&status[t], sp_word(ep, first ? 2u : 1u, ct));
    // (one lane) what the unit reports once `excl`, the group's bytes before
    // it, is known: a slot too small (its lines past the slot's end are not
    // stored, ArrayOutputStream.java:40-42), the piece's offset, the group's
    // length
    auto report = [&](uint64_t excl) __attribute__((always_inline)) {
      if (excl + ct > send - sb) atomicOr(&A.gstatus[g], (int32_t)CPK_ENOMEM);
      if (c == 0) A.piece_off[p] = d0 + excl;
      if (t + 1 == u1) A.grp_len[g] = excl + ct;
    };
    // (wave 0) the look-back inside the group
    auto getoff = [&]() {
      const uint64_t excl = sp_lookback(status + u0, t - u0, ct, ep, err, lane);
      if (lane == 0) {
        report(excl);
        scr[5] = sb + excl;
        __builtin_amdgcn_s_waitcnt(0xc07f);  // (the offset before the flag)
        scr[11] = (uint64_t)t + 1;
      }
      return sb + excl;
    };
    if (first && w == 0 && lane == 0) report(0);
    if (gm.cnt) {
      auto getbase = [&]() -> uint64_t {
        if (w == 0) return getoff() + wbefore;
        while ((uint32_t)sp_ld(&scr[11]) != t + 1) __builtin_amdgcn_s_sleep(1);
        return sp_ld(&scr[5]) + wbefore;
      };
      sp_b<F>(R, gm.cnt, lut, ring, A.out, first, wmine + 16 <= F::kRing, sb + wbefore, lane, send,
              pw + gm.wfirst, gm.wrem, getbase);
    } else if (w == 0 && !first) {
      getoff();  // wave 0 runs the look-back even without steps (an empty piece)
    }
    // (no wave takes the next ticket before the unit's offset is out: scr[5])
    if (!first)
      while ((uint32_t)sp_ld(&scr[11]) != t + 1) __builtin_amdgcn_s_sleep(1);
  }
}
