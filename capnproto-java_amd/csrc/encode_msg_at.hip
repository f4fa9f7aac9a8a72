// encode_msg_at.hip -- messages packed to slots the caller names
// (cpk_encode_messages_at).  Included from packed_codec.hip (namespace cpk)
// after encode_v4.hip and encode_at.hip.  It restates neither encoder: the
// segments are packed by the two passes (e4_size_kernel, e4_emit_kernel with
// an end per piece) or by the placed single pass (sp_place_kernel, the
// messages' segments as its groups), and the tables are built and packed as
// cpk_encode_messages builds them (table_word, table_words, serial_pack).
// What is here is the message's side of both: a thread per message that
// judges the slot, stores the table and tells the form that runs where the
// segments go.
//
//   wave form    size pass -> mat_slot_kernel (the message's length from the
//                sizes, its status, every piece's offset; the table; each
//                segment's placed offset and slot end, 0 for a message that
//                is refused) -> e4_emit_kernel<true>
//   placed form  mat_slot_kernel (the table; the segments' base and capacity
//                behind it) -> sp_place_kernel over private arrays ->
//                mat_finish_kernel (table bytes added, statuses merged)
// Both are enqueued where both can run; mat_pick_kernel leaves the choice in
// tickets[kTkGate + kGatePick] (nonzero: the placed form).

// The form, after e4_gate_kernel (cpk_encode_batch's rule over the segments as
// pieces, in kGatePick) and at_gate_kernel (dense or sparse, in kGateSparse):
// a form the host did not enqueue is never picked, and when the wave form
// runs neither placed kernel does (kGateSparse = 2 is neither's).
__global__ void mat_pick_kernel(uint32_t *tickets, uint32_t can_wave, uint32_t can_place) {
  if (threadIdx.x) return;
  const bool place = !can_wave || (can_place && tickets[kTkGate + kGatePick] != 0u);
  tickets[kTkGate + kGatePick] = place ? 1u : 0u;
  if (!place) tickets[kTkGate + kGateSparse] = 2u;
}

struct MatArgs {
  const uint64_t *mseg;    // [nm + 1] the messages' first segments
  const uint64_t *tsize;   // [nm] the tables' packed bytes (msg_table_size_kernel)
  const uint64_t *ssize;   // [nseg] the segments' packed bytes (the size pass; wave form)
  uint64_t hint;           // max_seg_words
  uint64_t *soff, *send;   // [nseg] wave form, written: the segment's first byte, its slot's end
  uint64_t *base, *cap;    // [nm] placed form, written: the segments' first byte and room behind the table
  const uint64_t *glen;    // [nm] placed form: the segments' packed bytes (sp_place_kernel)
  const int32_t *gst;      // [nm]   their status
  const uint64_t *spoff;   // [nseg]   their first bytes
  const uint32_t *pick;    // nonzero: the placed form runs
};

// message m's segments, clamped to the batch: with offsets that are not what
// the contract asks for, these kernels' own indices stay in range (as
// at_prep_kernel's; msg_table_size_kernel reads d_msg_seg_off as it stands,
// here as in cpk_encode_messages)
__device__ __forceinline__ void mat_segs(const AtArgs &U, const MatArgs &M, uint32_t m, uint64_t &s0, uint64_t &s1) {
  s0 = M.mseg[m] < U.n ? M.mseg[m] : U.n;
  s1 = M.mseg[m + 1] < U.n ? M.mseg[m + 1] : U.n;
  if (s1 < s0) s1 = s0;
}

// One thread per message.  U: the caller's placement (ng = nm messages over
// n = nseg segments; piece_off / grp_len / gstatus the caller's d_piece_off /
// d_msg_len / d_status).
__global__ void mat_slot_kernel(AtArgs U, MatArgs M) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= U.ng) return;
  uint64_t s0, s1;
  mat_segs(U, M, m, s0, s1);
  const uint32_t count = (uint32_t)(s1 - s0);
  const uint64_t d0 = U.dst_off[m], end = at_slot_end(U, m, d0);
  const bool passes = d0 > U.out_cap || (U.dst_cap && U.dst_cap[m] > U.out_cap - d0);
  const uint64_t room = d0 < end ? end - d0 : 0;
  const uint64_t tb = M.tsize[m];
  uint64_t *poff = U.piece_off + s0 + m;  // (message order: the table, then the segments)
  poff[0] = d0;
  bool table;
  if (*M.pick) {
    // the placed form sizes the segments as it stores them: the table goes
    // out when it fits alone, the rest of the slot is the segments'
    table = !passes && tb <= room;
    U.gstatus[m] = table ? CPK_OK : CPK_ENOMEM;
    M.base[m] = tb > ~d0 ? ~(uint64_t)0 : d0 + tb;  // (saturating)
    M.cap[m] = table ? room - tb : 0;
  } else {
    uint64_t len = tb;
    bool inval = false;
    for (uint64_t s = s0; s < s1; ++s) {
      const uint64_t W = U.swo[s + 1] - U.swo[s];
      inval |= W > M.hint || W >= (1ull << 31);
      poff[1 + s - s0] = M.soff[s] = d0 + len;
      len += M.ssize[s];
    }
    table = !inval && !passes && len <= room;
    // (a refused message's segments: offset 0 against the end 0, so that no
    // d_dst_off, however large, wraps the emit pass's offset + size past it)
    for (uint64_t s = s0; s < s1; ++s) {
      M.send[s] = table ? end : 0;
      if (!table) M.soff[s] = 0;
    }
    U.grp_len[m] = len;
    U.gstatus[m] = inval ? CPK_EINVAL : table ? CPK_OK : CPK_ENOMEM;
  }
  if (!table) return;
  uint8_t *o = U.out + d0;
  serial_pack(table_words(count), [&](uint32_t k) { return table_word(U.swo, s0, count, k); },
              [&](uint32_t b) { *o++ = (uint8_t)b; });
}

// The placed form's results in the caller's arrays: the message's length is
// its table's bytes and its segments', its status the table's OR the
// segments' (CPK_EINVAL covers CPK_ENOMEM: encode_at.hip's static_assert).
__global__ void mat_finish_kernel(AtArgs U, MatArgs M) {
  if (!*M.pick) return;
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= U.ng) return;
  uint64_t s0, s1;
  mat_segs(U, M, m, s0, s1);
  U.grp_len[m] = M.tsize[m] + M.glen[m];
  U.gstatus[m] |= M.gst[m];
  for (uint64_t s = s0; s < s1; ++s) U.piece_off[s + m + 1] = M.spoff[s];
}
