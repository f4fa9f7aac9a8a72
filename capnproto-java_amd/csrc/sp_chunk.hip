// sp_chunk.hip -- one 8192-word chunk of a piece, up to its packed size: what
// the single pass (sp_encode_kernel, encode_sp.hip), the one-workgroup kernel
// (sp_small_kernel, encode_sp3.hip) and the size query (sz_chunk_kernel,
// encode_size.hip) all run per unit.  The latter two call it; the single pass
// keeps its own written-out text of A1, the look-ahead and the chunk sequence
// (encode_sp.hip says why) on top of the shared state, masks and A2.
// Included from packed_codec.hip (namespace cpk) after encode_v4.hip (e4_tag;
// SpSt and sp_roles of sp_roles.hip) and before the three.
//
// A chunk is kSpCS steps of 64 words, spread over the workgroup's waves
// (SpGeom), lane = word.  Per chunk:
//   A1  per word the nonzero-byte tag m (PackedOutputStream.java:64-117); per
//       step the Z / DL / D ballots (zero word, <= 1 zero byte, tag 0xff),
//       stashed lane-per-step (sp_a1_step) and copied to LDS for the other
//       waves (sp_put_masks).  Where the words come from is the caller's
//       load policy: sp_a1_reload reads them in groups and drops them,
//       sp_a1_regs takes them from registers;
//   hand-over  the run state crossing a chunk boundary inside a piece
//       (SpHandover): published for the next chunk, taken from the one before;
//   A2  each wave recomputes the state entering its first step from the
//       earlier steps' masks (sp_state_at), then the roles
//       PackedOutputStream.write gives each word, from mask arithmetic
//       (sp_a2: lane-parallel, or step by step on the scalar ALU).  The packed
//       bytes of the wave follow from popcounts (sp_wave_bytes).  An encoder
//       also needs the run ends for its heads' counts: the step after the
//       wave's last (sp_next_step, sp_lookahead past the chunk) and sp_xs.
// tools/step_model.py is this algebra and the hand-over in Python, checked
// against the oracle (tests/test_step_model.py, test_packed_size_model.py).

#ifndef CPK_SP_WAVES
#define CPK_SP_WAVES 4
#endif
constexpr int kSpWaves = CPK_SP_WAVES;
constexpr int kSpThreads = 64 * kSpWaves;
constexpr int kSpWS = 128 / kSpWaves;          // steps per wave
constexpr int kSpCS = kSpWaves * kSpWS;        // steps per chunk (8192 words)
static_assert(kSpWaves <= 16 && kSpWS >= 4 && kSpWS <= 32 && kSpWS % 4 == 0, "wave count");

// Steps are scheduled one at a time: hoisting later steps' LUT reads and
// lane reads ahead would keep them all live at once (VGPR spills).
#define CPK_SP_STEP_FENCE() __builtin_amdgcn_sched_barrier(0)

// status word per piece: [63:62] flag (1 aggregate, 2 inclusive prefix),
// [61:46] launch epoch, [45:0] value (a relaxed 8-byte agent-scope granule:
// the data is the flag, cdna_hip_programming.md Guideline 16 form R2)
constexpr uint64_t kSpValMask = (1ull << 46) - 1;
__device__ __forceinline__ uint64_t sp_word(uint32_t ep, uint32_t flag, uint64_t v) {
  return ((uint64_t)flag << 62) | ((uint64_t)(ep & 0xffffu) << 46) | (v & kSpValMask);
}
__device__ __forceinline__ uint32_t sp_flag(uint64_t w, uint32_t ep) {
  return (uint32_t)((w >> 46) & 0xffffu) == (ep & 0xffffu) ? (uint32_t)(w >> 62) : 0u;
}
// run state <-> a status word's value (zl < 2^31, dlo, hd <= 256: 41 bits)
__device__ __forceinline__ uint64_t sp_pack_state(SpSt s) {
  return (uint64_t)s.zl | ((uint64_t)s.dlo << 31) | ((uint64_t)s.hd << 32);
}
__device__ __forceinline__ SpSt sp_unpack_state(uint64_t v) {
  SpSt s = {(uint32_t)v & 0x7fffffffu, (uint32_t)(v >> 31) & 1u, (uint32_t)(v >> 32) & 0x1ffu};
  return s;
}

__device__ __forceinline__ uint64_t sp_ld(const uint64_t *p) { return sp_uni(*p); }

// ---- the chunk's steps over the waves ---------------------------------------------
// Chunk c of a piece of W words as wave w sees it.  A chunk's steps are spread
// over all waves (a short piece keeps every wave busy, not wave 0 alone): per
// wave ceil(cs / waves), rounded up to a pair.
struct SpGeom {
  uint32_t nch;     // the piece's chunks (>= 1)
  bool lastc;       // c is the piece's last chunk
  int cs;           // steps in this chunk
  int sa, cnt;      // this wave's steps [sa, sa + cnt) of the chunk
  uint32_t wfirst;  // the wave's first word (piece-relative)
  uint32_t wrem;    // piece words from wfirst on (0: no steps)
  bool last;        // this wave holds the chunk's last step
  // kSpWS whole steps (A1's straight-line form)
  __device__ __forceinline__ bool full() const { return cnt == kSpWS && wrem >= 64u * kSpWS; }
  // the first word past the wave's steps
  __device__ __forceinline__ uint32_t wend() const { return wfirst + 64u * cnt; }
};
// c may be a chunk the piece does not have (no steps then: the ns > cs0
// guard).  The single pass's written-out copy goes without the guard: its
// unit table never names such a chunk.
__device__ __forceinline__ SpGeom sp_geom(uint32_t W, uint32_t c, int w) {
  SpGeom g;
  const uint32_t ns = (W + 63) >> 6;
  g.nch = max((ns + kSpCS - 1) / kSpCS, 1u);
  g.lastc = c + 1 >= g.nch;
  const uint32_t cs0 = c * kSpCS;
  g.cs = ns > cs0 ? (int)min((uint32_t)kSpCS, ns - cs0) : 0;
  const int per = min(kSpWS, ((g.cs + kSpWaves - 1) / kSpWaves + 1) & ~1);
  g.sa = w * per;
  g.cnt = max(0, min(per, g.cs - g.sa));
  g.wfirst = (cs0 + (uint32_t)g.sa) * 64;
  g.wrem = g.cnt ? W - g.wfirst : 0;
  g.last = g.cnt && g.sa + g.cnt == g.cs;
  return g;
}

// ---- masks in LDS: the state entering a step ---------------------------------------
// first D word at chunk position >= x and < lim, else lim
__device__ int sp_first_d(const uint64_t *msk, int x, int lim) {
  if (x >= lim) return lim;
  int q = x >> 6;
  uint64_t m = sp_ld(&msk[3 * q + 2]) & (~0ull << (x & 63));
  while (!m) {
    ++q;
    if (q * 64 >= lim) return lim;
    m = sp_ld(&msk[3 * q + 2]);
  }
  return min(q * 64 + __builtin_ctzll(m), lim);
}

// State entering chunk step s0 from the masks of the steps before it and
// the chunk's entering state (tools/step_model.py: state_at); dep is set
// when the result used the entering state (a zero run or D/L stretch over
// every step before s0)
__device__ SpSt sp_state_at(const uint64_t *msk, int s0, SpSt cst, bool &dep) {
  if (s0 == 0) {
    dep = true;
    return cst;
  }
  SpSt st = {0u, 0u, 0u};
  const uint64_t Zp = sp_ld(&msk[3 * (s0 - 1)]), DLp = sp_ld(&msk[3 * (s0 - 1) + 1]);
  if (Zp >> 63) {
    int q = s0 - 1;
    uint32_t zl = 0;
    uint64_t z = Zp;
    while (z == ~0ull) {
      zl += 64;
      if (--q < 0) break;
      z = sp_ld(&msk[3 * q]);
    }
    st.zl = zl + (q >= 0 ? (uint32_t)__builtin_clzll(~z) : cst.zl);
    dep |= q < 0;
  }
  if (!(DLp >> 63)) return st;
  st.dlo = 1;
  int q = s0 - 1;
  uint64_t d = DLp;
  while (d == ~0ull) {
    if (--q < 0) break;
    d = sp_ld(&msk[3 * q + 1]);
  }
  const int P = 64 * s0;
  int h;
  if (q >= 0 || !cst.dlo || !cst.hd) {
    const int start = q >= 0 ? 64 * q + 64 - __builtin_clzll(~d) : 0;
    h = sp_first_d(msk, start, P);
    if (h >= P) return st;
  } else {
    h = -(int)cst.hd;
  }
  dep |= q < 0;
  for (;;) {
    const int h2 = sp_first_d(msk, max(h + 256, 0), P);
    if (h2 >= P) break;
    h = h2;
  }
  st.hd = (uint32_t)min(P - h, 256);
  return st;
}

// words of class cls (0: Z, 1: DL) from chunk step s on (<= 256); la: the
// count continuing past the chunk's end
__device__ uint32_t sp_cont(const uint64_t *msk, int s, int cs, int cls, uint32_t la) {
  uint32_t r = 0;
  for (int q = s; r < 256; ++q) {
    if (q >= cs) {
      r += la;
      break;
    }
    const uint64_t m = sp_ld(&msk[3 * q + cls]);
    if (m != ~0ull) {
      r += (uint32_t)__builtin_ctzll(~m);
      break;
    }
    r += 64;
  }
  return min(r, 256u);
}

// ---- A1 ---------------------------------------------------------------------------
// What a wave keeps of its steps from A1 to B, whatever the form
struct SpStash {
  uint32_t mp[kSpWS / 4];  // tags, four per register
  uint32_t zl, zh, dll, dlh, dl_, dh_;                 // A1 stash: Z, DL, D (lane = step)
  uint32_t oml, omh, ohl, ohh, oel, oeh;               // A2 stash: Mem, HC, E
  uint32_t ox;                                         //   X: words past the step to the next run end
};

// Step j of the wave from this lane's word of it (valid: the word is inside
// the piece): the tag (kTags: kept in R.mp for B), the step's ballots stashed
// at lane j; returns the word's nonzero bytes
template <bool kTags>
__device__ __forceinline__ uint32_t sp_a1_step(SpStash &R, uint64_t word, bool valid, int j) {
  const uint32_t m = valid ? e4_tag(word) : 0u;
  if constexpr (kTags) {
    if (j & 3) R.mp[j >> 2] |= m << (8 * (j & 3));
    else R.mp[j >> 2] = m;
  }
  const uint32_t pc = (uint32_t)__builtin_popcount(m);
  const uint64_t Z = __ballot(valid && m == 0), DL = __ballot(pc >= 7), D = __ballot(m == 0xffu);
  R.zl = sp_wl(R.zl, (uint32_t)Z, j);
  R.zh = sp_wl(R.zh, (uint32_t)(Z >> 32), j);
  R.dll = sp_wl(R.dll, (uint32_t)DL, j);
  R.dlh = sp_wl(R.dlh, (uint32_t)(DL >> 32), j);
  R.dl_ = sp_wl(R.dl_, (uint32_t)D, j);
  R.dh_ = sp_wl(R.dh_, (uint32_t)(D >> 32), j);
  return pc;
}

// A1 of the wave's cnt steps (wrem piece words from its first on); returns
// this lane's nonzero-byte count.
// kFull: the wave holds kSpWS whole steps -- straight-line code, so each
// step waits only for its own load (vmcnt(kSpWS - 1 - j)); with the per-step
// branches of the general form the compiler waits for all of them at the
// first step.
// The words already in registers (step j in V[j]), their loads in flight:
template <bool kFull>
__device__ __forceinline__ uint32_t sp_a1_regs(SpStash &R, const uint64_t (&V)[kSpWS], uint32_t wrem, int cnt,
                                               int lane) {
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < kSpWS; ++j) {
    // (lane vs a scalar bound: no per-step lane constants kept in registers)
    if (kFull || j < cnt) acc += sp_a1_step<true>(R, V[j], kFull || (uint32_t)lane < wrem - 64u * j, j);
    CPK_SP_STEP_FENCE();
  }
  return acc;
}
// The words at src, not kept: loads in groups of F::kA1G steps, the next
// group's in flight while a group's tags are taken; clamped to the piece, not
// predicated: step j's lanes read min(lane, last valid lane of the step).
// F::kA1Stream: nontemporal loads (the words are not read again);
// F::kA1Tags: the tags kept.
template <class F, bool kFull>
__device__ __forceinline__ uint32_t sp_a1_reload(SpStash &R, const uint64_t *__restrict__ src, uint32_t wrem,
                                                 int cnt, int lane) {
  constexpr int G = F::kA1G;
  static_assert(kSpWS % G == 0, "A1 groups");
  uint64_t v[2][G];
  auto ld = [&](int j) __attribute__((always_inline)) -> uint64_t {
    const uint64_t *p = &(src + j * 64)[kFull ? (uint32_t)lane : min((uint32_t)lane, min(wrem - 1 - 64u * j, 63u))];
    if constexpr (F::kA1Stream) return ld_stream(p);
    else return *p;
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
      if (kFull || j < cnt)
        acc += sp_a1_step<F::kA1Tags>(R, v[g & 1][i], kFull || (uint32_t)lane < wrem - 64u * j, j);
    }
    CPK_SP_STEP_FENCE();
  }
  return acc;
}

// the wave's masks to LDS (lane j = step sa + j)
__device__ __forceinline__ void sp_put_masks(const SpStash &R, uint64_t *msk, int sa, int cnt, int lane) {
  if (lane < cnt) {
    uint64_t *m = msk + 3 * (sa + lane);
    m[0] = (uint64_t)R.zl | ((uint64_t)R.zh << 32);
    m[1] = (uint64_t)R.dll | ((uint64_t)R.dlh << 32);
    m[2] = (uint64_t)R.dl_ | ((uint64_t)R.dh_ << 32);
  }
}

// ---- the run state from chunk to chunk ---------------------------------------------
// A chunk that continues a piece enters with the run state its predecessor
// left, and leaves its own for the next: one epoch-tagged status word per
// chunk (flag 2), `prev` the predecessor's and `next` this chunk's (null:
// the piece's first / last chunk).  In order, once the chunk's masks are in
// LDS (a barrier): publish_early, wait (if prev), A2, publish_late.
// The state leaving a chunk depends on the one entering it only when a zero
// run or D/L stretch covers the whole chunk (sp_state_at's dep); otherwise it
// is published before this chunk waits for its own entering state, so the
// chunks of a piece do not wait on one another in a chain.
// The wait cannot hang: chunks are taken in order (the in-order ticket; the
// small kernel's loop), so the predecessor holds an earlier ticket, is
// resident and running, and publishes at the latest after its own A2 -- for
// which it waits only on chunks earlier still.  The spin is bounded all the
// same and reports kErrWait.
struct SpHandover {
  uint64_t *prev, *next;
  uint32_t ep;    // the launch epoch tagging the words
  uint32_t *err;  // error bits
  bool early = false;  // (internal) the leaving state went out before the wait

  __device__ __forceinline__ void publish(SpSt s, int lane) const {
    if (lane == 0) st_status(next, sp_word(ep, 2u, sp_pack_state(s)));
  }
  // (the chunk's last wave)
  __device__ __forceinline__ void publish_early(const uint64_t *msk, const SpGeom &g, int lane) {
    early = false;
    if (next && g.last) {
      bool dep = false;
      const SpSt ex = sp_state_at(msk, g.cs, SpSt{0u, 0u, 0u}, dep);
      if (!dep) {
        early = true;
        publish(ex, lane);
      }
    }
  }
  // All threads (a barrier); the value lands in the LDS word `slot`.
  // kProbed: thread 0 passes a read of *prev it issued earlier as `first`.
  template <bool kProbed>
  __device__ __forceinline__ SpSt wait(uint64_t first, uint64_t *slot) const {
    if (threadIdx.x == 0) {
      uint32_t spins = 0;
      uint64_t v = kProbed ? first : ld_status(prev);
      while (sp_flag(v, ep) != 2u) {
        if (++spins > (1u << 24)) {  // cannot happen: see above
          atomicOr(err, kErrWait);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        v = ld_status(prev);
      }
      *slot = v & kSpValMask;
    }
    __syncthreads();
    return sp_unpack_state(sp_ld(slot));
  }
  // cst: the state that entered the chunk
  __device__ __forceinline__ void publish_late(const uint64_t *msk, const SpGeom &g, SpSt cst, int lane) const {
    if (g.last && next && !early) {
      bool dep_ = false;
      publish(sp_state_at(msk, g.cs, cst, dep_), lane);
    }
  }
};

// ---- A2 ---------------------------------------------------------------------------
// A2, sequential form (scalar ALU, one step at a time): the roles of the
// wave's steps from the state entering its first step; stashes Mem
// (literal-run members), HC (heads with a count byte) and E (run ends) at
// lane = step (B needs no mask of the words without output: they are the
// zero words that are no head); returns the steps' packed bytes beyond
// their nonzero bytes.  nz0 / ndl0: bit 0 of the step after the wave's last.
// Used when a D/L stretch longer than 192 words enters a step (a literal run
// may end inside it); sp_a2p otherwise.
__device__ __forceinline__ uint32_t sp_a2_seq(SpStash &R, int cnt, uint32_t wrem, SpSt st, uint32_t nz0, uint32_t ndl0) {
  uint32_t bytes = 0;
  for (int j = 0; j < cnt; ++j) {
    const uint64_t Z = sp_rl(R.zl, R.zh, j), DL = sp_rl(R.dll, R.dlh, j), D = sp_rl(R.dl_, R.dh_, j);
    const uint32_t vr = wrem - 64u * j;
    const uint64_t V = vr >= 64 ? ~0ull : ((1ull << vr) - 1);
    uint64_t Zh, Mem;
    sp_roles(Z, DL, D, st, Zh, Mem);
    const uint64_t HC = Zh | (D & ~Mem), ZO = (Z & ~Zh) | ~V;
    bytes += (uint32_t)(__builtin_popcountll(~ZO & ~Mem) + __builtin_popcountll(Mem & ~D) +
                        __builtin_popcountll(HC));
    uint64_t z0 = nz0, d0 = ndl0;
    if (j + 1 < cnt) {
      z0 = (uint32_t)__builtin_amdgcn_readlane((int)R.zl, j + 1) & 1u;
      d0 = (uint32_t)__builtin_amdgcn_readlane((int)R.dll, j + 1) & 1u;
    }
    const uint64_t E = (Z & ~((Z >> 1) | (z0 << 63))) | (DL & ~((DL >> 1) | (d0 << 63)));
    R.oml = sp_wl(R.oml, (uint32_t)Mem, j);
    R.omh = sp_wl(R.omh, (uint32_t)(Mem >> 32), j);
    R.ohl = sp_wl(R.ohl, (uint32_t)HC, j);
    R.ohh = sp_wl(R.ohh, (uint32_t)(HC >> 32), j);
    R.oel = sp_wl(R.oel, (uint32_t)E, j);
    R.oeh = sp_wl(R.oeh, (uint32_t)(E >> 32), j);
  }
  return bytes;
}

// value of v at lane src
__device__ __forceinline__ uint32_t sp_from(uint32_t v, int src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
}

// A2, lane-parallel form: lane j computes step j's roles with 64-bit vector
// ops; what carries from step to step (the zero run's length, whether the
// D/L stretch entering a step already has its 0xFF head) comes from ballots
// over the steps.  Exact while every literal run that enters a step covers
// it to its end, i.e. no D/L stretch longer than 192 words enters a step:
// returns false (nothing written) when one does.  Same stash as sp_a2_seq.
__device__ __forceinline__ bool sp_a2p(SpStash &R, int cnt, uint32_t wrem, SpSt st, uint32_t nz0,
                                       uint32_t ndl0, int lane, uint32_t &bytes) {
  const bool act = lane < cnt;
  const uint64_t Z = act ? ((uint64_t)R.zl | ((uint64_t)R.zh << 32)) : 0ull;
  const uint64_t DL = act ? ((uint64_t)R.dll | ((uint64_t)R.dlh << 32)) : 0ull;
  const uint64_t D = act ? ((uint64_t)R.dl_ | ((uint64_t)R.dh_ << 32)) : 0ull;
  const uint64_t below = (1ull << lane) - 1;  // steps before this one
  // ---- D/L stretch entering the step: its length (bounds the distance to
  // its last head) and whether it has a head yet
  const uint32_t dlo = (uint32_t)wave_shr1((int)(uint32_t)(DL >> 63), (int)st.dlo);
  const uint32_t topdl = DL == ~0ull ? 64u : (uint32_t)__builtin_clzll(~DL);
  const uint64_t notall = __ballot(!act || DL != ~0ull);
  const uint64_t kdm = notall & below;
  const int kd = kdm ? 63 - __builtin_clzll(kdm) : -1;  // last step before with a non-D/L word
  const uint32_t topdl_k = sp_from(topdl, kd < 0 ? 0 : kd);
  const uint32_t len = kd >= 0 ? topdl_k + 64u * (uint32_t)(lane - 1 - kd)
                               : (st.dlo ? st.hd : 0u) + 64u * (uint32_t)lane;
  const bool cont = act && dlo && (DL & 1);
  if (__ballot(cont && len > 192)) return false;
  const uint64_t anyD = __ballot(act && D != 0);
  const bool topd = topdl > 0 && (D >> (64 - topdl)) != 0;
  const uint64_t TD = __ballot(act && topd);
  const uint64_t btw = anyD & below & (kd >= 0 ? (~0ull << kd) << 1 : ~0ull);
  const bool head = btw != 0 || (kd >= 0 ? ((TD >> kd) & 1) != 0 : (st.dlo && st.hd));
  const uint64_t cin = (cont && head) ? 1ull : 0ull;
  const uint64_t A = ((D << 1) | cin) & DL;
  const uint64_t C = (DL + A) ^ DL ^ A;
  const uint64_t Mem = DL & (A | C);
  // ---- zero runs: heads at run starts and every 256 words
  const uint32_t zc = (uint32_t)wave_shr1((int)(uint32_t)(Z >> 63), st.zl ? 1 : 0);
  uint64_t Zh = Z & ~((Z << 1) | zc);
  {
    const uint32_t topz = Z == ~0ull ? 64u : (uint32_t)__builtin_clzll(~Z);
    const uint64_t kzm = __ballot(!act || Z != ~0ull) & below;
    const int kz = kzm ? 63 - __builtin_clzll(kzm) : -1;
    const uint32_t topz_k = sp_from(topz, kz < 0 ? 0 : kz);
    const uint32_t zl = kz >= 0 ? topz_k + 64u * (uint32_t)(lane - 1 - kz) : st.zl + 64u * (uint32_t)lane;
    const uint32_t j0 = (256u - (zl & 255u)) & 255u;
    if (__ballot(act && zc && (Z & 1) && j0 < 64)) {
      const uint64_t pre = j0 >= 63 ? ~0ull : ((2ull << j0) - 1);
      if (act && zc && (Z & 1) && j0 < 64 && (Z & pre) == pre) Zh |= 1ull << j0;
    }
  }
  // ---- per step: output masks, run ends, bytes
  const uint32_t vr = act ? wrem - 64u * (uint32_t)lane : 0u;
  const uint64_t V = vr >= 64 ? ~0ull : ((1ull << vr) - 1);
  const uint64_t HC = Zh | (D & ~Mem), ZO = (Z & ~Zh) | ~V;
  // bit 0 of the next step (lane + 1; the wave's last step: nz0 / ndl0)
  uint32_t zn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)Z, 0x130, 0xf, 0xf, false) & 1u;
  uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)DL, 0x130, 0xf, 0xf, false) & 1u;
  if (lane == cnt - 1) {
    zn = nz0;
    dn = ndl0;
  }
  const uint64_t E = (Z & ~((Z >> 1) | ((uint64_t)zn << 63))) | (DL & ~((DL >> 1) | ((uint64_t)dn << 63)));
  uint32_t b = act ? (uint32_t)(__builtin_popcountll(~ZO & ~Mem) + __builtin_popcountll(Mem & ~D) +
                                __builtin_popcountll(HC))
                   : 0u;
  bytes = (uint32_t)__builtin_amdgcn_readlane(wave_incl_add((int)b), 63);
  R.oml = (uint32_t)Mem;
  R.omh = (uint32_t)(Mem >> 32);
  R.ohl = (uint32_t)HC;
  R.ohh = (uint32_t)(HC >> 32);
  R.oel = (uint32_t)E;
  R.oeh = (uint32_t)(E >> 32);
  return true;
}

// A2 in whichever form is exact
__device__ __forceinline__ uint32_t sp_a2(SpStash &R, int cnt, uint32_t wrem, SpSt st, uint32_t nz0, uint32_t ndl0,
                                          int lane) {
  uint32_t rb = 0;
  if (!sp_a2p(R, cnt, wrem, st, nz0, ndl0, lane, rb)) rb = sp_a2_seq(R, cnt, wrem, st, nz0, ndl0);
  return rb;
}

// X per step (lane = step): words past the step's end to the first run end
// after it (a head's count reaches that far), from the next step with a run
// end; past the wave's last step, Xlast.  At most 256.
__device__ __forceinline__ void sp_xs(SpStash &R, int cnt, uint32_t Xlast, int lane) {
  const bool act = lane < cnt;
  const uint64_t E = (uint64_t)R.oel | ((uint64_t)R.oeh << 32);
  const uint64_t en = __ballot(act && E != 0);
  const uint64_t km = lane == 63 ? 0ull : (en & (~0ull << (lane + 1)));
  const int k = km ? __builtin_ctzll(km) : 64;
  const uint32_t ce = E ? (uint32_t)__builtin_ctzll(E) : 64u;
  const uint32_t ce_k = sp_from(ce, k & 63);
  uint32_t X = k < cnt ? 64u * (uint32_t)(k - lane - 1) + ce_k : 64u * (uint32_t)(cnt - 1 - lane) + Xlast;
  R.ox = min(X, 256u);
}

// Look-ahead past a chunk: the zero run / D/L stretch continuing from the
// chunk's end (<= 256 words each), from the next 4 steps' words; word(j):
// this lane's word of step j past the chunk (asked for only inside the piece:
// avail words are left).
template <class Word>
__device__ __forceinline__ void sp_lookahead(uint32_t avail, int lane, Word word, uint32_t &laz, uint32_t &ladl) {
  uint32_t rz = 0, rd = 0;
  bool oz = true, od = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool valid = (uint32_t)lane < (avail > 64u * j ? avail - 64u * j : 0u);
    const uint64_t x = valid ? word(j) : 0ull;
    const uint32_t m = valid ? e4_tag(x) : 0u;
    const uint64_t Z = __ballot(valid && m == 0), DL = __ballot(__builtin_popcount(m) >= 7);
    if (oz) {
      if (Z == ~0ull) rz += 64;
      else { rz += (uint32_t)__builtin_ctzll(~Z); oz = false; }
    }
    if (od) {
      if (DL == ~0ull) rd += 64;
      else { rd += (uint32_t)__builtin_ctzll(~DL); od = false; }
    }
  }
  laz = rz;
  ladl = rd;
}

// The step after the wave's last, in the chunk or past it (look-ahead, by
// the chunk's last wave when the piece goes on: W words, word(j) as
// sp_lookahead's): bit 0 of its Z and DL masks, and Xlast, the words past the
// wave's last step to the next run end.
template <class Word>
__device__ __forceinline__ void sp_next_step(const SpStash &R, const uint64_t *msk, const SpGeom &g, uint32_t W,
                                             int lane, Word word, uint32_t &nz0, uint32_t &ndl0, uint32_t &Xlast) {
  const int cnt = g.cnt, send = g.sa + g.cnt;
  Xlast = 0;
  uint32_t laz = 0, ladl = 0;
  if (g.last && g.wend() < W) sp_lookahead(W - g.wend(), lane, word, laz, ladl);
  if (send < g.cs) {
    nz0 = (uint32_t)sp_ld(&msk[3 * send]) & 1u;
    ndl0 = (uint32_t)sp_ld(&msk[3 * send + 1]) & 1u;
  } else {
    nz0 = laz ? 1u : 0u;
    ndl0 = ladl ? 1u : 0u;
  }
  const uint64_t Zl = sp_rl(R.zl, R.zh, cnt - 1), DLl = sp_rl(R.dll, R.dlh, cnt - 1);
  const int cls = (Zl >> 63) ? 0 : ((DLl >> 63) ? 1 : -1);
  if (cls >= 0) {
    const uint32_t r = sp_cont(msk, send, g.cs, cls, cls ? ladl : laz);
    Xlast = r ? r - 1 : 0;
  }
}

// The waves' packed bytes through scr[16 + wave] (all waves; a barrier):
// returns the chunk's; wbefore: of the waves before this one; wmine: this one's
__device__ __forceinline__ uint64_t sp_wave_bytes(uint64_t *scr, uint32_t bytes, int w, int lane, uint64_t &wbefore,
                                                  uint64_t &wmine) {
  if (lane == 0) scr[16 + w] = bytes;
  __syncthreads();  // wave bytes in LDS
  uint64_t tot = 0;
  wbefore = 0;
  wmine = 0;
#pragma unroll
  for (int q = 0; q < kSpWaves; ++q) {
    const uint64_t b = sp_ld(&scr[16 + q]);
    if (q < w) wbefore += b;
    if (q == w) wmine = b;
    tot += b;
  }
  return tot;
}
