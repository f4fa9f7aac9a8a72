// decode_v2.hip -- the decoder with a record index (the default).  Included
// from packed_codec.hip (namespace cpk): the pieces, the window load, the
// speculative chunk walks and the pointer-doubling chain resolution are
// decode_win.hip's, shared with decode_kernel (decode_map.hip); what follows
// differs.
//
// decode_kernel maps every 4-word output block to its covering record by
// walking each true record once per expansion round and writing one map entry
// per block it covers (a 256-word zero run: 64 entries by one lane while the
// others wait), then expands block by block with a branch per word kind.
// Here each true record is written once, as one 32-bit index entry (its
// window position and first output word), by the lane that holds it; the
// expansion then takes 64 consecutive output words per wave instruction,
// lane = word:
//   * the record covering word w is the index entry at rank (records started
//     at or before w): a 2048-bit map of record starts per expansion round
//     and a popcount below the lane give it;
//   * every word is one 8-byte read at the record's bytes and one v_perm
//     through LUT[tag]: a tagged word expands (PackedInputStream.java:84-90),
//     LUT[0] is all zero bytes (a zero run, :92-105), LUT[0xff] the identity
//     (the 0xFF word and its literal run, :106-134, read at tag + 2 + 8 ofs).
// No per-word branches, and the cost of a run is its words, not its length
// in loop trips of one lane.
// A window with more than kD2NI true records (at most kD2Win / 2) is cut at
// its kD2NI-th record; the next window starts there.

constexpr int kD2Threads = 256;  // 4 independent waves
// workgroups per CU the register budget is sized for (LDS allows 5)
constexpr int kD2Wpe = 5;
constexpr uint32_t kD2Chunk = 48;
constexpr uint32_t kD2Look = 32;  // bytes loaded past the window
typedef WinGeom<kD2Chunk, kD2Look> D2Geom;
constexpr uint32_t kD2Win = D2Geom::win, kD2WinBuf = D2Geom::buf, kD2ChkReach = D2Geom::reach;
constexpr uint32_t kD2NI = 1024;  // records indexed per window
constexpr uint32_t kD2Round = 2048;  // output words per expansion round
constexpr int kD2Unroll = 4;  // 64-word groups expanded together
constexpr uint32_t kD2Info = kD2NI * 4;
static_assert(kD2Info >= 64 * sizeof(VisMask) + 8, "visited masks live over the index");
// record starts of a round: a bit per output word, set with atomics
constexpr uint32_t kD2Bits = kD2Round / 8;
constexpr uint32_t kD2WaveLds = kD2WinBuf + kD2Info + kD2Bits;
constexpr uint32_t kD2Lds = 2048 + 4 * kD2WaveLds;
static_assert(kD2Win <= 4095, "record positions are 12-bit");

template <bool kStream>
__global__ __launch_bounds__(kD2Threads, kD2Wpe) void decode2_kernel(
    const uint8_t *__restrict__ packed, uint64_t *__restrict__ in_off,
    const uint64_t *__restrict__ swo, uint32_t n, uint64_t *__restrict__ out,
    int32_t *__restrict__ status, uint32_t *ticket, uint64_t avail, DecStreams sd) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // (the kernel's text, shared with decode2_at_kernel of decode_at.hip, where
  // kAt is true: a range per piece)
  constexpr bool kAt = false;
#define CPK_DECODE_V2_BODY
#include "decode_v2_body.hip"
#undef CPK_DECODE_V2_BODY
}

// ---- decoder choice on the device (cpk_decode_batch, no host sync) --------
// Sparse batches (packed bytes under 15 % of the words' bytes: long zero
// runs) go to the record-index decoder, which measured 2.75 against 3.46 ms
// per 131,072 config-4 pieces; the others to the block-map decoder (4.5
// against 6.2 ms at config 2).  skip[0]: the block-map decoder's flag,
// skip[1]: the record-index decoder's.
// After a few large pieces were decoded as one stream (cpk_decode_batch):
// when every piece ended exactly at its packed range's end and decoded, the
// batch decoders are told to skip (both flags); else they run and give each
// piece its batch-form status.  One block; n <= 32.
__global__ void dec_stream_check_kernel(const uint64_t *__restrict__ found, const uint64_t *__restrict__ in_off,
                                        const int32_t *__restrict__ st, uint32_t n, uint32_t *skip) {
  const uint32_t i = threadIdx.x;
  const bool ok = i > n || (found[i] == in_off[i] - in_off[0] && (i == n || st[i] == CPK_OK));
  if (__syncthreads_and(ok) && i == 0) {
    skip[0] = 1u;
    skip[1] = 1u;
    skip[2] = 1u;
  }
}

__global__ void dec_gate_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ swo, uint32_t n,
                                uint32_t *skip) {
  if (threadIdx.x == 0) {
    const uint64_t P = in_off[n] - in_off[0], U = 8 * (swo[n] - swo[0]);
    // skip[0]: the block-map decoder, [1] the record-index one (sparse
    // batches), [2] the block-map decoder's dense form (serial walks of
    // windows of few long records: packed bytes >= 80 % of the words')
    const bool v2 = 100 * P < 15 * U, dense = 100 * P >= 80 * U;
    skip[0] = (v2 || dense) ? 1u : 0u;
    skip[1] = v2 ? 0u : 1u;
    skip[2] = dense ? 0u : 1u;
  }
}
