// packed_codec.hip -- MI355X (gfx950, CDNA4) batched codec for Cap'n Proto's
// packed stream encoding: the kernels.  The host layer and the C ABI
// (include/capnp_packed.h) are in host_api.hip, included last.
//
// Reference semantics: runtime/src/main/java/org/capnproto/
//   PackedOutputStream.java:35-205 (encoder), PackedInputStream.java:35-140
//   (decoder).  One "piece" = one write()/read() call; pieces are independent
//   (PackedOutputStream.java:36-43 re-initialises all run state per call).
//
// Design (DESIGN.md has the full derivation and the rooflines):
//   encoders       encode_sp.hip (single pass, the default for like-sized
//                  pieces of 4 Ki words or more and small message batches):
//                  a workgroup per 8192-word chunk, the chunk in VGPRs, roles
//                  by mask algebra, a decoupled look-back for the offsets,
//                  strings (tag + v_perm-compacted bytes + count) OR-ed into
//                  an LDS ring, 16-byte line stores; its sparse form
//                  (SpSparse: words re-read in B, twice the workgroups per
//                  CU) for batches whose sampled words are >= 85 %
//                  zero; encode_v4.hip (two passes, mixed-size and small-
//                  piece batches): one wave per piece, a size pass, a scan,
//                  an emit pass.  The device chooses (e4_gate_kernel).
//   decoders       decode_map.hip, decode_kernel: one wave per piece, packed bytes staged in
//                  LDS window by window, the tag chain found by speculative
//                  per-lane walks with pointer-doubling validation, then a
//                  gather-expand of every 4-word output block from its
//                  covering record; decode_v2.hip (sparse batches): a record
//                  index per window instead of the block map;
//                  decode_win.hip: the piece loop, window load, walks and
//                  chain the two share;
//                  stream_split.hip: one long stream cut into blocks.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

#include "../../include/capnp_packed.h"
#include <initializer_list>

namespace cpk {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// ---- ticket counters ------------------------------------------------------
// One counter word saturates near 88 returning atomics per microsecond
// (MI355X_MICROARCH.md, row "dequeue").  Work with no order dependence (the
// decoder) is sharded per XCD: the k-th ticket taken from counter x is item
// 8k + x, every item is taken exactly once, and a wave whose counter runs
// dry moves on to the next counter, so coverage never depends on where the
// waves were placed (the XCD id only picks the first counter).  Work whose
// items depend on their predecessors (the encoders' look-back) keeps one
// ordered counter.
constexpr int32_t kMaxSegmentWords = (1 << 28) - 1;  // Serialize.java:45
constexpr int kTkStride = 32;          // u32 words between counters (128 B)
constexpr int kTkEnc = 0;              // encoder counters [8]
constexpr int kTkDec = 8 * kTkStride;  // decoder counters [8]
constexpr int kTkPlan = 16 * kTkStride;
constexpr int kTkErr = 17 * kTkStride;
// bits of the error word (cpk_ctx_take_error): a piece over its size hint, a
// timed-out cross-workgroup wait, packed bytes past the caller's capacity
constexpr uint32_t kErrHint = 1u, kErrWait = 4u, kErrCap = 8u;
// the gates' block (e4_minmax_kernel, e4_gate_kernel, sz_gate_kernel,
// dec_gate_kernel) and its words
constexpr int kTkGate = 17 * kTkStride + 8;
constexpr int kGateMin = 0, kGateMax = 1;  // min, max piece words of the batch
constexpr int kGatePick = 2;     // encoder / size form choice (nonzero: the single pass / the chunk form took it)
constexpr int kGateZero = 3;     // sampled zero words
constexpr int kGateSparse = 6;   // the single pass's form (1: sparse)
constexpr int kGateBytes = 7;    // the sampled words' packed bytes
constexpr int kGateDecSkip = 8;  // [3] decoder choice: nonzero = skip the block map, the record index, the dense
                                 // block map
constexpr int kTkWords = 18 * kTkStride;
__device__ __forceinline__ int xcc_id() {
  int x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 7;
}
// all 64 lanes call it (one folded +64 atomic per wave); the wave's item.
// The fold is the compiler's and the tickets depend on it: it needs x proved
// wave-uniform.  Unfolded, the lanes of two waves interleave on the counter
// and lane 0 reads no multiple of 64: one item taken twice, one never.  A
// caller whose x the compiler may lose track of passes readfirstlane(x)
// (DecPieces, decode_win.hip); after a change, look for s_bcnt1 in front of
// the global_atomic_add in the caller's assembly.
__device__ __forceinline__ uint32_t take_ticket(uint32_t *ctr, int x) {
  const uint32_t t = atomicAdd(&ctr[x * kTkStride], 1u);
  return (((uint32_t)__builtin_amdgcn_readlane((int)t, 0) >> 6) << 3) | (uint32_t)x;
}
// ordered single-counter form
__device__ __forceinline__ uint32_t take_ordered(uint32_t *ctr) {
  const uint32_t t = atomicAdd(ctr, 1u);
  return (uint32_t)__builtin_amdgcn_readlane((int)t, 0) >> 6;
}
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// a wave-uniform 64-bit value into scalar registers
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// ------------------------------------------------------------ wave scans
// DPP forms (gfx9 row_shr / row_bcast): no lane-compare masks, no LDS.
template <int kCtrl, int kRowMask = 0xf>
__device__ __forceinline__ int dpp(int old, int src) {
  return __builtin_amdgcn_update_dpp(old, src, kCtrl, kRowMask, 0xf, false);
}
#define CPK_WAVE_SCAN(NAME, OP, ID)                         \
  __device__ __forceinline__ int NAME(int v) {              \
    v = OP(v, dpp<0x111>(ID, v));                           \
    v = OP(v, dpp<0x112>(ID, v));                           \
    v = OP(v, dpp<0x114>(ID, v));                           \
    v = OP(v, dpp<0x118>(ID, v));                           \
    v = OP(v, dpp<0x142, 0xa>(ID, v));                      \
    v = OP(v, dpp<0x143, 0xc>(ID, v));                      \
    return v;                                               \
  }
__device__ __forceinline__ int op_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int op_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int op_add(int a, int b) { return a + b; }
CPK_WAVE_SCAN(wave_incl_max, op_max, -1)
CPK_WAVE_SCAN(wave_incl_add, op_add, 0)
CPK_WAVE_SCAN(wave_incl_min_fwd, op_min, 0x3fffffff)
// value of lane-1 (lane 0 gets `id`)
__device__ __forceinline__ int wave_shr1(int v, int id) { return dpp<0x138>(id, v); }
// suffix (right-to-left) inclusive min via lane reversal
__device__ __forceinline__ int wave_sufx_min(int v) {
  const int rl = 63 - (int)(threadIdx.x & 63);
  int r = __shfl(v, rl, 64);
  r = wave_incl_min_fwd(r);
  return __shfl(r, rl, 64);
}
__device__ __forceinline__ int readlane(int v, int l) {
  return __builtin_amdgcn_readlane(v, l);
}
// (the decoders' 64-bit form; encode_v4.hip keeps its own rl64)
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
}

// ---- diagnostic phase timing (built only with -DCPK_PHASE_STATS) ----------
// Thread 0 of each workgroup accumulates s_memtime deltas per phase in LDS
// (scr[96..127] as u64[16]) and adds them to g_phase at exit.  Shares of the
// total, not absolute times, are what a stats build is good for.
#ifdef CPK_PHASE_STATS
__device__ unsigned long long g_phase[64];
#define PH_INIT(scr)                                                         \
  unsigned long long ph_last = 0;                                            \
  unsigned long long *ph_acc = reinterpret_cast<unsigned long long *>(&(scr)[96]); \
  if (threadIdx.x < 16) ph_acc[threadIdx.x] = 0;                            \
  if (threadIdx.x == 0) ph_last = __builtin_amdgcn_s_memtime();
#define PH(i)                                                                \
  if (threadIdx.x == 0) {                                                    \
    unsigned long long t_ = __builtin_amdgcn_s_memtime();                    \
    ph_acc[i] += t_ - ph_last;                                               \
    ph_last = t_;                                                            \
  }
#define PH_ADD(i, v) if (threadIdx.x == 0) ph_acc[i] += (v);
#define PH_FLUSH(base)                                                       \
  __syncthreads();                                                           \
  if (threadIdx.x < 16) atomicAdd(&g_phase[(base) + threadIdx.x], ph_acc[threadIdx.x]);
// wave-level form (barrier-free kernels): per-wave sums, lane 0 flushes
#define WPH_INIT                                                             \
  unsigned long long wph_last = __builtin_amdgcn_s_memtime(), wph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define WPH(i)                                                               \
  {                                                                          \
    unsigned long long t_ = __builtin_amdgcn_s_memtime();                    \
    wph_acc[i] += t_ - wph_last;                                             \
    wph_last = t_;                                                           \
  }
#define WPH_FLUSH(base)                                                      \
  if ((threadIdx.x & 63) == 0)                                               \
    for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_phase[(base) + i_], wph_acc[i_]);
#else
#define PH_INIT(scr)
#define PH(i)
#define PH_ADD(i, v)
#define PH_FLUSH(base)
#define WPH_INIT
#define WPH(i)
#define WPH_FLUSH(base)
#endif

// floor(r / C) for window positions (r < 2^13) by a full-rate 24-bit
// multiply and a shift (the compiler's division by a constant is a
// quarter-rate v_mul_hi_u32 + v_mad_u64_u32 pair, in the landing walk's loop)
template <uint32_t C>
__device__ __forceinline__ uint32_t chunk_div(uint32_t r) {
  constexpr uint32_t kM = ((1u << 20) + C - 1) / C;
  static_assert((kM * C - (1u << 20)) * (1u << 13) < (1u << 20), "exact for r < 2^13");
  return __umul24(r, kM) >> 20;
}

// LUT entries.  compact: byte j = index of the j-th set bit of m (else 0x0C
// = zero byte for v_perm).  expand: byte i = popcount(m & ((1<<i)-1)) if bit
// i is set, else 0x0C.
__device__ void fill_luts(uint64_t *lut, bool expand) {
  int m = threadIdx.x;
  if (m < 256) {
    uint64_t v = 0;
    if (expand) {
      int c = 0;
      for (int i = 0; i < 8; ++i) {
        uint64_t s = (m >> i) & 1 ? (uint64_t)(c++) : 0x0cull;
        v |= s << (8 * i);
      }
    } else {
      int j = 0;
      for (int i = 0; i < 8; ++i)
        if ((m >> i) & 1) v |= (uint64_t)i << (8 * j++);
      for (; j < 8; ++j) v |= 0x0cull << (8 * j);
    }
    lut[m] = v;
  }
}

// Orders this wave's LDS accesses without waiting for them: DS instructions
// of one wave execute in issue order, so a later read sees earlier writes
// and atomics of every lane; only the compiler must not reorder across.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void wave_lds_sync() {
  // DS ops of one wave complete in order; this only stops the compiler
  // moving LDS accesses across the point and drains this lane's queue.
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");  // re-read LDS after this point (no forwarding)
}

// ------------------------------------------------------------ streaming hints
// nontemporal (streaming) loads and stores: data read or written once
typedef unsigned int cpk_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint64_t ld_stream(const uint64_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ uint4 ld_stream16(const uint4 *p) {
  const cpk_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const cpk_u32x4 *>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(uint4 w, void *p) {
  cpk_u32x4 v = {w.x, w.y, w.z, w.w};
  __builtin_nontemporal_store(v, reinterpret_cast<cpk_u32x4 *>(p));
}

// ------------------------------------------------------------ look-back
// One 8-byte relaxed agent-scope granule per status word: the data is the
// flag (cdna_hip_programming.md Guideline 16, form R2); the single-pass
// encoder's words (encode_sp.hip: sp_word) carry flag, epoch and value.
__device__ __forceinline__ void st_status(uint64_t *p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_status(uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}

// ---- the block-map decoder's geometry (decode_map.hip): declared here, where
// the seam tests read them (tests/_packed_records.py), so the sweeps move
// with them
// Lane chunks C of 56 bytes (3.5 KiB windows, 7 workgroups per CU by LDS):
// measured against 40 / 48 / 60 / 64 at 131,072 pieces with the max-map
// block map, 56 is fastest on configs 2-4 (against 48: 4.29 -> 4.13 ms,
// 6.80 -> 6.51, 2.84 -> 2.80)
constexpr uint32_t kDecChunk = 56;
// bytes loaded past the window (a literal run reaching past them is read from memory;
// 240: config 3 decode -4.5 % against 32, config 2 neutral; 368 costs occupancy)
constexpr uint32_t kDecLook = 240;
// output words expanded per round
// (8 workgroups per CU with 48-byte chunks; larger rounds cost occupancy)
#ifndef CPK_DEC_ROUND
#define CPK_DEC_ROUND 1280
#endif
// output words per expansion block
// (4: 64 lanes cover a window's blocks in fewer, fuller passes; measured faster than 8)
#ifndef CPK_DEC_BLK
#define CPK_DEC_BLK 4
#endif
// records a dense window's serial walk may pass (decode_body<.., kSerial>)
#ifndef CPK_DEC_SER_MAX
#define CPK_DEC_SER_MAX 128
#endif
#include "decode_win.hip"
#include "decode_map.hip"

// ------------------------------------------------------------ messages
// Serialize.read over PackedInputStream for a batch of packed messages whose
// byte ranges are known (Serialize.java:119-178): a thread per message reads
// the segment table (two read() calls: the first word, then 4 * (count & ~1)
// bytes), validates it, and the segments are then decoded as one packed
// stream per message by decode_kernel<true>.

// one read() of `words` words, byte-serial (tables are at most 257 words):
// PackedInputStream.java:35-140 as the oracle restates it
// (oracle/packed_oracle.c:cpko_unpack); f(word index, word) per word
template <class F>
__device__ int serial_read(const uint8_t *p, uint64_t n, uint64_t &ip, uint32_t words, F f) {
  if (words == 0) return CPK_OK;
  uint32_t wi = 0;
  for (;;) {
    if (ip >= n) return CPK_ETRUNC;
    const uint32_t tag = p[ip++];
    uint64_t w = 0;
    for (int i = 0; i < 8; ++i)
      if ((tag >> i) & 1) {
        if (ip >= n) return CPK_ETRUNC;
        w |= (uint64_t)p[ip++] << (8 * i);
      }
    f(wi++, w);
    if (tag == 0 || tag == 0xffu) {
      if (ip >= n) return CPK_ETRUNC;
      const uint32_t run = p[ip++];
      if (run > words - wi) return CPK_EOVERRUN;
      if (tag == 0) {
        for (uint32_t k = 0; k < run; ++k) f(wi++, 0ull);
      } else {
        if (n - ip < 8ull * run) return CPK_ETRUNC;
        for (uint32_t k = 0; k < run; ++k) {
          uint64_t v = 0;
          for (int i = 0; i < 8; ++i) v |= (uint64_t)p[ip + i] << (8 * i);
          ip += 8;
          f(wi++, v);
        }
      }
    }
    if (wi == words) return CPK_OK;
  }
}

// the table of message m: status, segment count, total words; on OK the
// packed position after the table.  emit(i, size) per segment.
struct NoWords {
  __device__ void operator()(uint32_t, uint64_t) const {}
};
// A valid table with a segment over 2^28 - 1 words: Serialize.read allocates
// and reads the segments in order (:165-175) and makeByteBufferForWords
// (:45-53) throws only when it reaches that segment, so a segment before it
// that fails wins.  The table at tp is read again, each earlier segment
// walked from sp[ip..sn) as its own read(), nothing stored.  -> the first
// failure among them, else CPK_EFRAME.  (Malformed messages only.)
__device__ int oversized_status(const uint8_t *tp, uint64_t tn, const uint8_t *sp, uint64_t sn, uint64_t ip,
                                uint32_t count) {
  int st = CPK_OK;
  bool hit = false;
  auto seg = [&](uint32_t sz) {
    if (hit || st != CPK_OK) return;
    if (sz > (uint32_t)kMaxSegmentWords)
      hit = true;
    else
      st = serial_read(sp, sn, ip, sz, NoWords());
  };
  uint64_t tip = 0;
  serial_read(tp, tn, tip, 1, [&](uint32_t, uint64_t w) { seg((uint32_t)(w >> 32)); });
  if (count > 1) {
    const uint32_t c = count;
    serial_read(tp, tn, tip, (count & ~1u) / 2, [&](uint32_t i, uint64_t w) {
      for (uint32_t h = 0; h < 2; ++h)
        if (2 * i + h + 1 < c) seg((uint32_t)(w >> (32 * h)));
    });
  }
  return st != CPK_OK ? st : CPK_EFRAME;
}

// (word(i, w): the table's words as read, i = 0 the first)
// (sp, sn: the bytes the segments are walked in when one is oversized, the
// table's end at the same offset as in p; null: p itself holds them)
template <class F, class G = NoWords>
__device__ int read_table(const uint8_t *p, uint64_t n, uint64_t limit, uint64_t &ip,
                          uint32_t &count, uint64_t &total, F emit, G word = G(),
                          const uint8_t *sp = nullptr, uint64_t sn = 0) {
  uint64_t first = 0;
  int st = serial_read(p, n, ip, 1, [&](uint32_t, uint64_t w) {
    first = w;
    word(0u, w);
  });
  if (st) return st;
  const int32_t raw = (int32_t)(uint32_t)first;
  if (raw < 0 || raw > 511) return CPK_EFRAME;  // Serialize.java:128-131
  count = (uint32_t)raw + 1;
  const int32_t s0 = (int32_t)(uint32_t)(first >> 32);
  if (s0 < 0) return CPK_EFRAME;  // :135-137
  total = (uint64_t)s0;
  bool neg = false, big = s0 > kMaxSegmentWords;
  emit(0u, (uint32_t)s0);
  if (count > 1) {  // :144-157
    const uint32_t c = count;
    st = serial_read(p, n, ip, (count & ~1u) / 2, [&](uint32_t i, uint64_t w) {
      word(1u + i, w);
      for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t k = 2 * i + h;  // moreSizes[k] = segment k + 1
        if (k + 1 < c) {
          const int32_t v = (int32_t)(uint32_t)(w >> (32 * h));
          neg |= v < 0;
          big |= v > kMaxSegmentWords;
          total += (uint64_t)(uint32_t)v;
          emit(k + 1, (uint32_t)v);
        }
      }
    });
    if (st) return st;
    if (neg) return CPK_EFRAME;  // :150-153 (the first negative size throws)
  }
  if (total > limit) return CPK_EFRAME;  // :160-162
  // makeByteBufferForWords (:45-53) throws for a segment over 2^28 - 1 words
  // when that segment is allocated, in segment order: the message fails
  // either way, with an earlier segment's failure if one fails
  if (big) return oversized_status(p, n, sp ? sp : p, sp ? sn : n, ip, count);
  return CPK_OK;
}

// ---- stream tickets, largest first --------------------------------------
// A wave decodes a message's stream whole, so a large message taken last
// leaves the other waves idle while it finishes (config 3: 1 MiB messages
// among 16 KiB ones; taken largest first the decode is 3.8 % shorter).  A
// counting sort by the bit length of the word count: order[t] = the t-th
// message to take, larger classes first (within a class in any order -- the
// output does not depend on it).  (The two-pass encoder's segments taken
// the same way: 51.3 -> 57.0 ms on config 3 -- the passes stream the words
// in memory order, and lose that locality.)
constexpr int kOrdClasses = 64;
__device__ __forceinline__ uint32_t ord_class(uint64_t w) {
  return (uint32_t)(kOrdClasses - 1) - (w ? 64u - (uint32_t)__builtin_clzll(w) : 0u);
}
// (item i's words: words[i], or swo[i + 1] - swo[i] when swo is given)
__device__ __forceinline__ uint64_t ord_words(const uint64_t *words, const uint64_t *swo, uint32_t i) {
  return swo ? swo[i + 1] - swo[i] : words[i];
}
__global__ void ord_hist_kernel(const uint64_t *__restrict__ words, uint32_t n, uint32_t *hist,
                                const uint64_t *__restrict__ swo) {
  __shared__ uint32_t h[kOrdClasses];
  if (threadIdx.x < kOrdClasses) h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&h[ord_class(ord_words(words, swo, i))], 1u);
  __syncthreads();
  if (threadIdx.x < kOrdClasses && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
__global__ void ord_scan_kernel(uint32_t *hist) {
  if (threadIdx.x != 0) return;
  uint32_t run = 0;
  for (int c = 0; c < kOrdClasses; ++c) {
    const uint32_t k = hist[c];
    hist[c] = run;
    run += k;
  }
}
// (a block reserves its range in each class with one global atomic: with a
// few classes and 256 Ki messages, one atomic per message took 1.5 ms)
__global__ void ord_scatter_kernel(const uint64_t *__restrict__ words, uint32_t n, uint32_t *cursor,
                                   uint32_t *__restrict__ order, const uint64_t *__restrict__ swo) {
  __shared__ uint32_t cnt[kOrdClasses], base[kOrdClasses];
  if (threadIdx.x < kOrdClasses) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t c = i < n ? ord_class(ord_words(words, swo, i)) : 0u;
  const uint32_t r = i < n ? atomicAdd(&cnt[c], 1u) : 0u;
  __syncthreads();
  if (threadIdx.x < kOrdClasses && cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (i < n) order[base[c] + r] = i;
}

// pass 1: per message its table's status, segment count, words and the
// packed position of segment 0
__global__ void msg_table_kernel(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ moff,
                                 uint32_t nm, uint64_t limit, uint64_t *__restrict__ mwords,
                                 uint64_t *__restrict__ mcount, uint64_t *__restrict__ mbeg,
                                 int32_t *__restrict__ mstatus) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const uint64_t a = moff[m];
  uint64_t ip = 0, total = 0;
  uint32_t count = 0;
  const int st = read_table(packed + a, moff[m + 1] - a, limit, ip, count, total,
                            [](uint32_t, uint32_t) {});
  mstatus[m] = st;
  mwords[m] = st ? 0 : total;
  mcount[m] = st ? 0 : count;
  mbeg[m] = a + ip;
}

// pass 2: the segments' word offsets (segment table read again)
__global__ void msg_swo_kernel(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ moff,
                               uint32_t nm, uint64_t limit, const uint64_t *__restrict__ mwoff,
                               const uint64_t *__restrict__ mseg, const int32_t *__restrict__ mstatus,
                               uint64_t *__restrict__ swo) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  if (m == nm - 1) swo[mseg[nm]] = mwoff[nm];
  if (mstatus[m] != CPK_OK) return;
  const uint64_t a = moff[m], s0 = mseg[m];
  uint64_t ip = 0, total = 0, acc = mwoff[m];
  uint32_t count = 0;
  read_table(packed + a, moff[m + 1] - a, limit, ip, count, total, [&](uint32_t i, uint32_t sz) {
    swo[s0 + i] = acc;
    acc += sz;
  });
}

// pass 4: a message's status: its table's, else its first failed segment's
// (a failure stops the stream: the last segment carries it), else
// CPK_ETRAILING when the segments end before the message's bytes do
__global__ void msg_final_kernel(const uint64_t *__restrict__ moff, uint32_t nm,
                                 const uint64_t *__restrict__ mseg, const uint64_t *__restrict__ mend,
                                 const int32_t *__restrict__ seg_status, int32_t *__restrict__ mstatus) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm || mstatus[m] != CPK_OK) return;
  const int32_t st = seg_status[mseg[m + 1] - 1];
  mstatus[m] = st != CPK_OK ? st : (mend[m] != moff[m + 1] ? CPK_ETRAILING : CPK_OK);
}

// The one-launch small paths' completion flag: once every wave's writes
// (pinned host memory included) are complete at system scope, seq goes to
// *flag -- host memory the caller spins on instead of a stream
// synchronisation (small_wait)
__device__ __forceinline__ void small_done(uint64_t *flag, uint64_t seq) {
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ... and its start: with no stream synchronisation between two calls the
// launch's own acquire may stop at device scope, so lines of the pinned
// input an earlier call read could still sit in L2: dropped here
__device__ __forceinline__ void small_begin() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, ""); }

// ---- one message from the front of a stream (cpk_read_message) -------------
// Serialize.read over PackedInputStream (Serialize.java:119-178) when the
// message's packed length is unknown: the table is read here, laid out as the
// stream's pieces -- [first word] [rest of the table] [segment 0] ... -- and
// padded with empty pieces (a read() of nothing consumes nothing,
// PackedInputStream.java:38) to kRmPieces, so the stream decoder's launch
// needs nothing from the host.  A failed table (or segments over the
// caller's capacity) leaves every piece empty: nothing is decoded.
constexpr uint32_t kRmHead = 257;              // table words at most (512 segments)
constexpr uint32_t kRmPieces = 2 + 512;        // first word, rest of the table, segments
constexpr uint32_t kRmInfo = 4 + 513;          // status, consumed, count, words, offsets

// sdesc: the one-wave decoder's stream descriptor (DecStreams with one
// stream): [0] its first byte, [1] its end, [2..3] its pieces (the table's
// two and the segments only: the padding is the parallel path's); [5] the
// parallel path's piece count
// (dec_tk: the batch decoder's ticket counters, zeroed here for the one-wave
// decode launched next -- one command fewer than a memset)
// (out, when set -- the one-launch path: the parse's own table words are
// written there and the stream descriptor starts at the first segment, so
// the decoder walks the segments only; otherwise the swo of the padding
// pieces is filled by all threads)
constexpr uint32_t kRmTableBytes = 2576;  // a table's packed bytes at most (257 words: 2,570)
struct RmScratch {
  uint32_t size[512];  // the segments' sizes as the parse reads them
  uint64_t fill[2];    // swo padding: first index, value
};
static_assert(kRmTableBytes % 16 == 0 && kRmTableBytes + sizeof(RmScratch) <= kDecLds, "rm_small_kernel LDS");
__device__ void rm_table_parse(const uint8_t *tb, uint64_t nt, const uint8_t *packed, uint64_t avail, uint64_t limit,
                               uint64_t cap_words, uint64_t *__restrict__ swo, uint64_t *__restrict__ info,
                               uint64_t *__restrict__ sdesc, uint64_t *__restrict__ out, RmScratch &rs);
__device__ __forceinline__ void rm_table_body(const uint8_t *__restrict__ packed, uint64_t avail, uint64_t limit,
                                              uint64_t cap_words, uint64_t *__restrict__ swo,
                                              uint64_t *__restrict__ info, uint64_t *__restrict__ sdesc,
                                              uint32_t *__restrict__ dec_tk, uint8_t *tb, RmScratch &rs,
                                              uint64_t *__restrict__ out) {
  if (dec_tk)
    for (uint32_t i = threadIdx.x; i < 8 * kTkStride; i += blockDim.x) dec_tk[i] = 0;
  // the bytes a table can reach staged in LDS (tb) by whole 16-byte lines
  // (readable up to round_up(avail, 16)), so the byte-serial parse below
  // makes no dependent memory round trips -- the packed bytes may be pinned
  // host memory
  const uint64_t nt = min(avail, (uint64_t)kRmTableBytes);
  for (uint32_t i = threadIdx.x; i < (uint32_t)((nt + 15) / 16); i += blockDim.x)
    reinterpret_cast<uint4 *>(tb)[i] = reinterpret_cast<const uint4 *>(packed)[i];
  __syncthreads();
  if (threadIdx.x == 0) rm_table_parse(tb, nt, packed, avail, limit, cap_words, swo, info, sdesc, out, rs);
  if (out) return;
  __syncthreads();
  const uint32_t f0 = (uint32_t)rs.fill[0];
  const uint64_t fv = rs.fill[1];
  for (uint32_t i = f0 + threadIdx.x; i <= kRmPieces; i += blockDim.x) swo[i] = fv;
}
__global__ void rm_table_kernel(const uint8_t *__restrict__ packed, uint64_t avail, uint64_t limit,
                                uint64_t cap_words, uint64_t *__restrict__ swo, uint64_t *__restrict__ info,
                                uint64_t *__restrict__ sdesc, uint32_t *__restrict__ dec_tk) {
  __shared__ __attribute__((aligned(16))) uint8_t tb[kRmTableBytes];
  __shared__ RmScratch rs;
  rm_table_body(packed, avail, limit, cap_words, swo, info, sdesc, dec_tk, tb, rs, nullptr);
}
// (one thread) the table read and checked as doRead does, the message laid
// out as the stream's pieces
__device__ void rm_table_parse(const uint8_t *tb, uint64_t nt, const uint8_t *packed, uint64_t avail, uint64_t limit,
                               uint64_t cap_words, uint64_t *__restrict__ swo, uint64_t *__restrict__ info,
                               uint64_t *__restrict__ sdesc, uint64_t *__restrict__ out, RmScratch &rs) {
  uint64_t ip = 0, total = 0;
  uint32_t count = 0;
  // (an oversized segment: the segments before it are walked in the bytes the
  // call may read, 10 per word of the caller's capacity, ss_reach)
  const uint64_t room = cap_words > (~0ull - 16) / 10 - kRmHead ? ~0ull : 10 * (cap_words + kRmHead) + 16;
  const uint64_t sn = min(avail, room);
  int st = read_table(
      tb, nt, limit, ip, count, total, [&](uint32_t i, uint32_t sz) { rs.size[i] = sz; },
      [&](uint32_t i, uint64_t w) {
        if (out) out[i] = w;
      },
      packed, sn);
  if (st == CPK_OK && total > cap_words) st = CPK_ENOMEM;
  // (a table always ends within kRmTableBytes < room, so with room's bytes
  // at hand only that walk can come up short: the segments before the
  // oversized one exceed the capacity, and where they end is not known --
  // the table's own verdict stands)
  if (st == CPK_ETRUNC && sn == room) st = CPK_EFRAME;
  info[0] = (uint64_t)(int64_t)st;
  info[1] = 0;
  info[2] = st == CPK_OK || st == CPK_ENOMEM ? count : 0;
  info[3] = st == CPK_OK || st == CPK_ENOMEM ? total : 0;
  uint64_t w = 0;
  swo[0] = 0;
  if (st == CPK_OK) {
    swo[1] = w = 1;
    swo[2] = w += (count & ~1u) / 2;
    for (uint32_t i = 0; i < count; ++i) {
      info[4 + i] = w;
      swo[3 + i] = w += rs.size[i];
    }
    info[4 + count] = w;
  } else {
    swo[1] = swo[2] = 0;
  }
  rs.fill[0] = (st == CPK_OK ? count : 0) + 3;
  rs.fill[1] = w;
  const bool go = st == CPK_OK;
  // (out: the segments' stream starts where the table's bytes end)
  sdesc[0] = out && go ? ip : 0;
  sdesc[1] = avail;
  sdesc[2] = out && go ? 2 : 0;
  sdesc[3] = go ? count + 2 : 0;
  sdesc[5] = kRmPieces;  // (the parallel path decodes every piece)
}

// the message's status: its table's, else the stream's (a failed piece
// stops the stream: the last piece carries it); the bytes consumed
// (end: where the stream's pieces ended; npieces: how many were decoded)
// (mirror: a host-visible copy of the finished row, or null)
__device__ __forceinline__ void rm_final_body(const uint64_t *__restrict__ end, const int32_t *__restrict__ pstatus,
                                              const uint64_t *__restrict__ npieces, uint64_t *__restrict__ info,
                                              uint64_t *__restrict__ mirror);
__global__ void rm_final_kernel(const uint64_t *__restrict__ end, const int32_t *__restrict__ pstatus,
                                const uint64_t *__restrict__ npieces, uint64_t *__restrict__ info,
                                uint64_t *__restrict__ mirror) {
  rm_final_body(end, pstatus, npieces, info, mirror);
}
__device__ __forceinline__ void rm_final_body(const uint64_t *__restrict__ end, const int32_t *__restrict__ pstatus,
                                              const uint64_t *__restrict__ npieces, uint64_t *__restrict__ info,
                                              uint64_t *__restrict__ mirror) {
  if (threadIdx.x == 0 && (int64_t)info[0] == CPK_OK) {
    const int32_t st = pstatus[*npieces - 1];
    info[0] = (uint64_t)(int64_t)st;
    info[1] = st == CPK_OK ? *end : 0;
  }
  if (!mirror) return;
  __syncthreads();
  const uint32_t rows = 4 + (uint32_t)min(info[2], (uint64_t)512) + 1;  // (status, consumed, count, words, offsets)
  for (uint32_t i = threadIdx.x; i < rows; i += blockDim.x) mirror[i] = info[i];
}

// cpk_read_message whole in ONE launch when the one-wave decoder takes the
// message: the table (rm_table_body, which also writes the table's words),
// the stream of its segments from where the table's bytes end
// (decode_body<true>: one of the four waves finds the stream's ticket) and
// the info row (rm_final_body), separated by workgroup barriers -- three
// launches' dispatch latency saved on the small-message path
// (dcopy, when set: the packed bytes -- pinned host memory -- are first
// copied there by all threads at once, one PCIe round trip instead of one
// per window of the one-wave walk; round_up(avail, 16) + 64 bytes)
__global__ __launch_bounds__(kDecThreads, 1) void rm_small_kernel(
    const uint8_t *__restrict__ packed, uint64_t avail, uint64_t limit, uint64_t cap_words,
    uint64_t *__restrict__ swo, uint64_t *__restrict__ info, uint64_t *__restrict__ sdesc, uint32_t *tk,
    uint64_t *__restrict__ out, uint64_t *__restrict__ in_off, int32_t *__restrict__ pst,
    uint64_t *__restrict__ send_out, uint64_t *__restrict__ mirror, uint8_t *__restrict__ dcopy, uint64_t seq) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (mirror) small_begin();
  if (dcopy) {
    const uint32_t lines = (uint32_t)((avail + 15) / 16) + 4;
    for (uint32_t i = threadIdx.x; i < lines; i += blockDim.x)
      reinterpret_cast<uint4 *>(dcopy)[i] = reinterpret_cast<const uint4 *>(packed)[i];
    __syncthreads();
    packed = dcopy;
  }
  rm_table_body(packed, avail, limit, cap_words, swo, info, sdesc, tk, smem,
                *reinterpret_cast<RmScratch *>(smem + kRmTableBytes), out);
  __syncthreads();  // (the layout and the zeroed tickets before the decode)
  decode_body<true>(smem, packed, in_off, swo, kRmPieces, out, pst, tk, avail,
                    DecStreams{sdesc, sdesc + 1, sdesc + 2, 1, send_out, nullptr});
  __syncthreads();  // (the stream's end and statuses before the fold)
  rm_final_body(send_out, pst, sdesc + 3, info, mirror);
  if (mirror) small_done(mirror + kRmInfo, seq);
}

#include "decode_mw.hip"

// ---- message write: Serialize.write = table piece + segment pieces --------
// PackedOutputStream.write (:35-205) byte-serial over a word source, as the
// oracle restates it (oracle/packed_oracle.c:cpko_pack); for the segment
// tables (a thread per message).  word(i) -> word i; emit(byte).
template <class Wf, class Ef>
__device__ void serial_pack(uint32_t nwords, Wf word, Ef emit) {
  uint32_t i = 0;
  while (i < nwords) {
    const uint64_t w = word(i++);
    uint32_t tag = 0;
    for (int b = 0; b < 8; ++b) tag |= ((w >> (8 * b)) & 0xffu) ? (1u << b) : 0u;
    emit(tag);
    for (int b = 0; b < 8; ++b)
      if ((tag >> b) & 1) emit((uint32_t)(w >> (8 * b)) & 0xffu);
    if (tag == 0) {  // :119-131
      uint32_t run = 0;
      while (i < nwords && run < 255 && word(i) == 0) {
        ++run;
        ++i;
      }
      emit(run);
    } else if (tag == 0xffu) {  // :133-193: stop before a word with >= 2 zero bytes
      uint32_t run = 0;
      while (i < nwords && run < 255) {
        const uint64_t x = word(i);
        int z = 0;
        for (int b = 0; b < 8; ++b) z += ((x >> (8 * b)) & 0xffu) == 0;
        if (z >= 2) break;
        ++run;
        ++i;
      }
      emit(run);
      for (uint32_t k = i - run; k < i; ++k) {
        const uint64_t x = word(k);
        for (int b = 0; b < 8; ++b) emit((uint32_t)(x >> (8 * b)) & 0xffu);
      }
    }
  }
}

// word k of message m's segment table (Serialize.java:256-273): ints
// [count - 1, size_0 .. size_{count-1}, 0 pad], (count + 2) & ~1 of them
__device__ __forceinline__ uint64_t table_word(const uint64_t *swo, uint64_t s0, uint32_t count,
                                               uint32_t k) {
  uint32_t v[2];
  for (int h = 0; h < 2; ++h) {
    const uint32_t j = 2 * k + h;
    v[h] = j == 0 ? count - 1 : (j <= count ? (uint32_t)(swo[s0 + j] - swo[s0 + j - 1]) : 0u);
  }
  return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
}
__device__ __forceinline__ uint32_t table_words(uint32_t count) { return ((count + 2) & ~1u) / 2; }

// packed size of every message's table
__global__ void msg_table_size_kernel(const uint64_t *__restrict__ swo,
                                      const uint64_t *__restrict__ mseg, uint32_t nm,
                                      uint64_t *__restrict__ tsize) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const uint64_t s0 = mseg[m];
  const uint32_t count = (uint32_t)(mseg[m + 1] - s0);
  uint64_t nb = 0;
  serial_pack(table_words(count), [&](uint32_t k) { return table_word(swo, s0, count, k); },
              [&](uint32_t) { ++nb; });
  tsize[m] = nb;
}

// piece sizes in message order: table, then its segments
__global__ void msg_interleave_kernel(const uint64_t *__restrict__ mseg, uint32_t nm,
                                      const uint64_t *__restrict__ tsize,
                                      const uint64_t *__restrict__ ssize, uint64_t *__restrict__ comb) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const uint64_t s0 = mseg[m], s1 = mseg[m + 1];
  uint64_t *c = comb + s0 + m;
  c[0] = tsize[m];
  for (uint64_t s = s0; s < s1; ++s) c[1 + s - s0] = ssize[s];
}

// each segment's packed offset (from the message-order offsets), and the
// tables' packed bytes
__global__ void msg_table_emit_kernel(const uint64_t *__restrict__ swo,
                                      const uint64_t *__restrict__ mseg, uint32_t nm,
                                      const uint64_t *__restrict__ poff, uint64_t *__restrict__ soff,
                                      uint8_t *__restrict__ out, const uint64_t *__restrict__ tsize,
                                      uint64_t ocap, uint32_t *err) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const uint64_t s0 = mseg[m], s1 = mseg[m + 1];
  const uint64_t *c = poff + s0 + m;
  for (uint64_t s = s0; s < s1; ++s) soff[s] = c[1 + s - s0];
  // (the caller's output capacity: a table that would pass it is not
  // written, ArrayOutputStream.java:40-42)
  if (c[0] + tsize[m] > ocap) {
    atomicOr(err, kErrCap);
    return;
  }
  uint8_t *o = out + c[0];
  const uint32_t count = (uint32_t)(s1 - s0);
  serial_pack(table_words(count), [&](uint32_t k) { return table_word(swo, s0, count, k); },
              [&](uint32_t b) { *o++ = (uint8_t)b; });
}

// ------------------------------------------------------------ bench support
struct FastRand {
  int32_t x, y, z, w;
};
// benchmark/src/main/java/org/capnproto/benchmark/Common.java:31-38
__device__ __forceinline__ uint32_t fr_next(FastRand &r) {
  uint32_t ux = (uint32_t)r.x;
  uint32_t tmp = ux ^ (ux << 11);
  r.x = r.y;
  r.y = r.z;
  r.z = r.w;
  uint32_t w = (uint32_t)r.w;
  w = w ^ (uint32_t)(r.w >> 19) ^ tmp ^ (uint32_t)((int32_t)tmp >> 8);
  r.w = (int32_t)w;
  return w;
}
__device__ __forceinline__ uint64_t splitmix64(uint64_t &s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void generate_kernel(cpk_gen_params p, const uint64_t *__restrict__ swo, uint32_t n,
                                uint64_t *__restrict__ out) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    uint64_t sd = 0x1d2acd47ull ^ ((uint64_t)p.cfg << 40) ^ ((uint64_t)s * 0xD1B54A32D192ED03ull);
    uint64_t a = splitmix64(sd), b = splitmix64(sd);
    FastRand r{(int32_t)(uint32_t)a, (int32_t)(uint32_t)(a >> 32), (int32_t)(uint32_t)b,
               (int32_t)(uint32_t)(b >> 32)};
    if ((r.x | r.y | r.z | r.w) == 0) r.w = 1;
    uint64_t w0 = swo[s], w1 = swo[s + 1];
    bool zero = (uint64_t)fr_next(r) < p.t_zero0;
    for (uint64_t k = 0; k < w1 - w0; ++k) {
      if (k) {
        uint32_t t = fr_next(r);
        zero = zero ? !((uint64_t)t < p.t_z2n) : ((uint64_t)t < p.t_n2z);
      }
      uint64_t v = 0;
      if (!zero) {
        for (int bb = 0; bb < 8; ++bb) {
          uint32_t t = fr_next(r);
          uint64_t byte = ((uint64_t)t < p.t_qbyte) ? 0 : (uint64_t)(1 + (t >> 8) % 255);
          v |= byte << (8 * bb);
        }
      }
      out[w0 + k] = v;
    }
  }
}

__global__ void mismatch_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                uint64_t words, unsigned long long *cnt) {
  unsigned long long c = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words;
       i += (uint64_t)gridDim.x * blockDim.x)
    c += a[i] != b[i];
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt, c);
}

// up to 8 device words gathered into pinned host memory, for the host's
// read-backs of a few sizes (read_words): one launch and one sync instead
// of a copy into pageable memory per word (~15-20 us each)
struct Gather8 {
  const uint64_t *p[8];
};
__global__ void gather8_kernel(Gather8 g, uint32_t k, uint64_t *out) {
  if (threadIdx.x < k) out[threadIdx.x] = *g.p[threadIdx.x];
}

#include "encode_v4.hip"
#include "sp_chunk.hip"
#include "encode_sp.hip"
#include "encode_sp3.hip"
#include "encode_size.hip"
#include "encode_at.hip"
#include "encode_msg_at.hip"
#include "decode_v2.hip"
#include "stream_split.hip"
#include "decode_size.hip"
#include "decode_at.hip"
#include "decode_msg_at.hip"
#include "encode_ms.hip"

}  // namespace cpk

#include "host_api.hip"
