/*
 * capnp_packed.h -- C ABI of the MI355X (gfx950) packed-stream codec.
 *
 * Drop-in boundary for capnproto-java's packed encoding
 * (runtime/src/main/java/org/capnproto/PackedOutputStream.java:35-205,
 * PackedInputStream.java:35-140).  Plain pointers and sizes only; the JNI
 * glue in capnproto-java_amd/java/ binds exactly these entry points
 * (INTEGRATION.md).
 *
 * A "piece" is what one PackedOutputStream.write() / PackedInputStream.read()
 * call handles.  Serialize.write issues one write() per segment and one for
 * the segment table (Serialize.java:256-288), and each call starts from fresh
 * run state (PackedOutputStream.java:36-43), so a batch of pieces is encoded
 * and decoded independently, bit-exact with the reference.
 *
 * Threading: reentrant; a context may be used from one host thread at a time,
 * different contexts concurrently.  All *_batch calls are asynchronous on the
 * given stream (hipStream_t passed as void*; NULL = the device's null stream).
 * Calls on one context share its device workspace (counters, piece sizes,
 * step boundaries): issue them on one stream, or order the streams, so that
 * they do not run at the same time.
 *
 * Graph capture: a device entry point that makes no host synchronisation may
 * be called on a stream that is being captured (hipStreamBeginCapture) and
 * the graph replayed with other data in the same buffers: cpk_encode_batch,
 * cpk_encode_batch_cap, cpk_encode_messages[_cap], cpk_packed_size_batch and
 * cpk_encode_batch_at with max_seg_words != 0, cpk_packed_size_messages,
 * cpk_encode_messages_at, cpk_decode_batch and cpk_unpacked_size_batch
 * (their read-back for n <= 32 is skipped while capturing),
 * cpk_decode_batch_at, cpk_unpacked_size_batch_at, cpk_decode_messages_at,
 * cpk_read_message,
 * cpk_generate, cpk_count_mismatch, and cpk_decode_stream below 384 KiB of
 * `avail` (from there on it reads its word total back).  The call must have
 * run once uncaptured on the same context with the same n, counts, bounds and
 * capacities: the context's buffers grow on demand, and growth allocates,
 * which a capture does not allow.  Not to be captured: the calls documented
 * to synchronise (cpk_decode_messages, the *_message_stream calls,
 * cpk_ctx_take_error, cpk_ctx_dense_windows, every host form) and
 * max_seg_words == 0.  tests/test_gpu_graph_replay.py replays each of them
 * (cpk_encode_messages_at: tests/test_gpu_encode_messages_at_replay.py).
 */
#ifndef CAPNP_PACKED_H
#define CAPNP_PACKED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPK_ABI_VERSION 1

/* Status codes.  Decode errors are the reference's exceptions:
 *   CPK_EINVAL    piece length not a multiple of 8 -> DecodeException
 *                 ("PackedInputStream reads must be word-aligned",
 *                 PackedInputStream.java:40-42); bad arguments.
 *   CPK_ETRUNC    packed input ended before the piece was filled ->
 *                 DecodeException (ArrayInputStream.java:53-58,
 *                 PackedInputStream.java:93-95).  Also a literal run cut
 *                 short by end of input, which the reference may accept
 *                 silently through ArrayInputStream (documented divergence,
 *                 DESIGN.md).
 *   CPK_EOVERRUN  a 0x00/0xFF run runs past the end of the piece ->
 *                 DecodeException / BufferOverflowException
 *                 (PackedInputStream.java:99-105, :110-114).
 *   CPK_ETRAILING batch form only: the piece was filled before the end of
 *                 its packed byte range (the reference would leave the
 *                 bytes to the next read()).
 *   CPK_EFRAME    segment table invalid: count over 512, a negative size, a
 *                 message over the traversal limit or a segment over 2^28-1
 *                 words -> DecodeException (Serialize.java:45-53, :125-163).
 *                 The last is thrown in segment order, when the read reaches
 *                 that segment (:165-175): a segment before it that fails
 *                 gives the message its own status (CPK_ETRUNC,
 *                 CPK_EOVERRUN) instead.  Such a message reports its status
 *                 at any capacity, never CPK_ENOMEM; cpk_read_message walks
 *                 the earlier segments in the bytes it may read and reports
 *                 CPK_EFRAME when they end beyond those.
 *   CPK_ENOMEM, CPK_EDEVICE  allocation / HIP runtime failure (-> IOException).
 *   CPK_EUNSUPPORTED  a piece outside what this build handles.
 */
#define CPK_OK 0
#define CPK_EINVAL (-1)
#define CPK_ETRUNC (-2)
#define CPK_EOVERRUN (-3)
#define CPK_ETRAILING (-4)
#define CPK_ENOMEM (-5)
#define CPK_EDEVICE (-6)
#define CPK_EFRAME (-7)
#define CPK_EUNSUPPORTED (-8)

typedef struct cpk_ctx_s *cpk_ctx;

int cpk_abi_version(void);
const char *cpk_status_string(int status);

/* Worst-case packed size of one piece of `words` words: 8w + 2*ceil(w/2).
 * (An isolated all-nonzero word costs 10 bytes) */
uint64_t cpk_packed_bound(uint64_t words);

/* Capacity, in bytes, the caller must allocate for the packed output of a
 * batch whose pieces have the given word counts: sum of the bounds plus 16
 * bytes of read slack (the decoder reads whole 16-byte lines). */
uint64_t cpk_batch_packed_capacity(const uint64_t *h_seg_word_off, uint32_t n);

/* Context bound to one HIP device.  Holds the look-back workspace. */
int cpk_ctx_create(int device, cpk_ctx *out);
void cpk_ctx_destroy(cpk_ctx ctx);
int cpk_ctx_device(cpk_ctx ctx);
/* Times a one-launch host path (small messages) found its kernel's pinned
 * completion flag unset even after the stream synchronisation it falls back
 * to when the flag has not turned within 5 ms (a late launch on a busy GPU
 * only takes that fallback and is not counted).  Zero in normal operation: a
 * count that grows means a lost completion flag (a device-side bug). */
uint64_t cpk_ctx_small_fallbacks(cpk_ctx ctx);
/* Diagnostics of the last batch / message decode on this context (synchronises
 * `stream`): windows the dense block-map form walked with one lane along the
 * true chain, and serial walks it gave back to the parallel walks (too many
 * records); both 0 when another decoder form took the batch.  Counted only by
 * the diagnostics build (libcapnp_packed_hip_diag.so: the counters cost the
 * dense forms ~2 %); the product library returns CPK_EUNSUPPORTED. */
int cpk_ctx_dense_windows(cpk_ctx ctx, void *stream, uint64_t *serial, uint64_t *given_back);

/* Batch encode of n pieces, device-resident (replaces n calls of
 * PackedOutputStream.write, PackedOutputStream.java:35-205).  Pieces of any
 * size.  The encoder is chosen on the device from the piece sizes (no host
 * sync): like-sized pieces of 4 Ki words or more (the largest at most twice
 * the smallest) take the single-pass encoder (read the words once, write the
 * packed bytes once, work ticketed per 8192-word chunk, offsets by a decoupled
 * look-back over the chunks; pieces over one chunk need max_seg_words), in
 * its sparse form (twice the workgroups per CU) when >= 85 % of a sample of
 * the words are zero; other batches the two-pass one (a size pass, a scan of
 * the sizes, an emit pass).
 *   d_in            : 8-byte aligned words; piece i is words
 *                     [d_seg_word_off[i], d_seg_word_off[i+1]).
 *   d_seg_word_off  : uint64[n+1], device.
 *   max_seg_words   : host bound on every piece's size in words, 0 = unknown
 *                     (the call then reads d_seg_word_off[0], [n] back,
 *                     synchronising `stream`).  A piece larger than a nonzero
 *                     bound is reported by cpk_ctx_take_error (output
 *                     undefined for that piece).
 *   d_out           : 16-byte aligned, capacity cpk_batch_packed_capacity().
 *   d_out_off       : uint64[n+1], device, written: piece i's packed bytes
 *                     are d_out[d_out_off[i] .. d_out_off[i+1]), contiguous
 *                     and in order, i.e. exactly the bytes the reference
 *                     writes for pieces 0..n-1 through one sink.
 * Returns CPK_OK or an error; asynchronous on `stream`. */
int cpk_encode_batch(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                     uint32_t n, uint64_t max_seg_words, void *d_out,
                     uint64_t *d_out_off, void *stream);

/* Batch of messages (Serialize.write through PackedOutputStream for each,
 * SerializePacked.write, Serialize.java:256-288): message m's segments are
 * pieces [d_msg_seg_off[m], d_msg_seg_off[m+1]) of d_in / d_seg_word_off
 * (nseg pieces in message order, d_msg_seg_off[0] = 0, [nm] = nseg); its segment table (count - 1, the sizes in
 * words, zero pad; :256-273) is built and packed on the device, so the
 * output holds, per message, packed(table) || packed(seg 0) || ... -- the
 * bytes SerializePacked.write produces, messages back to back.
 *   max_seg_words   : host bound on every segment's words (required, > 0;
 *                     a segment over it is reported by cpk_ctx_take_error).
 *   d_out           : 16-byte aligned, capacity cpk_batch_packed_capacity()
 *                     of the segments + 10 * ((count + 2) / 2 + 1) bytes per
 *                     message of `count` segments.
 *   d_out_off       : uint64[nm + nseg + 1], written: piece offsets in
 *                     message order (table, segments; next message); message
 *                     m starts at d_out_off[d_msg_seg_off[m] + m] and the
 *                     last entry is the total.
 * Asynchronous on `stream`. */
int cpk_encode_messages(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                        uint32_t nseg, const uint64_t *d_msg_seg_off, uint32_t nm,
                        uint64_t max_seg_words, void *d_out, uint64_t *d_out_off, void *stream);

/* The same two calls with the byte capacity of d_out (the reference's sink
 * refuses a write that does not fit: ArrayOutputStream.write throws
 * IOException, ArrayOutputStream.java:36-44).  A piece whose packed bytes
 * would pass out_cap is reported -- cpk_ctx_take_error returns CPK_ENOMEM --
 * and no byte at or past d_out + out_cap is ever stored; pieces wholly below
 * it are written as usual (the bytes of the piece that crosses it are
 * undefined).  cpk_encode_batch / cpk_encode_messages are these calls with
 * out_cap = UINT64_MAX: they trust the documented capacity. */
int cpk_encode_batch_cap(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                         uint32_t n, uint64_t max_seg_words, void *d_out, uint64_t out_cap,
                         uint64_t *d_out_off, void *stream);
int cpk_encode_messages_cap(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                            uint32_t nseg, const uint64_t *d_msg_seg_off, uint32_t nm,
                            uint64_t max_seg_words, void *d_out, uint64_t out_cap,
                            uint64_t *d_out_off, void *stream);

/* Synchronises `stream` and returns the first problem an encode issued since
 * the last call met (and clears it): CPK_ENOMEM if packed bytes would have
 * passed an out_cap (the *_cap forms), CPK_EINVAL if a piece was larger than
 * its max_seg_words bound, else CPK_OK.  The host forms below check it
 * themselves. */
int cpk_ctx_take_error(cpk_ctx ctx, void *stream);

/* Exact packed sizes without encoding: what cpk_encode_batch /
 * cpk_encode_messages would write to d_out_off for the same arguments, with
 * no packed byte produced and no output buffer taken -- to allocate exactly
 * instead of cpk_batch_packed_capacity() (about 1.25 x the unpacked bytes), to
 * write a length prefix ahead of the packed bytes, or to see whether packing
 * pays.  (The unpacked half of the question is the reference's
 * Serialize.computeSerializedSizeInWords, Serialize.java:229.)  Device
 * traffic is the unpacked words, read once, plus the offset array.  The form
 * is chosen on the device from the piece sizes: a workgroup per 8192-word
 * chunk for a batch with a piece of over one chunk and at least 1/2048 of the
 * batch's words (one piece far larger than the rest, or few large pieces), a
 * wave per piece otherwise; CPK_ENCODER has no say.
 *   cpk_packed_size_batch: d_out_off is uint64[n+1], device, written: [0] = 0,
 *     [i+1] - [i] = piece i's packed bytes, [n] = the total.
 *   cpk_packed_size_messages: d_out_off is uint64[nm + nseg + 1], laid out as
 *     cpk_encode_messages lays it out: per message the table piece, then its
 *     segments.  The tables are built and sized on the device as the encoder
 *     builds them; none is stored to caller memory.
 *   max_seg_words: as for cpk_encode_batch.  Nonzero: no host
 *     synchronisation; a piece larger than the bound is reported by
 *     cpk_ctx_take_error as CPK_EINVAL (its size is then undefined).  0 =
 *     unknown: cpk_packed_size_batch reads d_seg_word_off[0], [n] back,
 *     synchronising `stream`, as cpk_encode_batch does
 *     (cpk_packed_size_messages needs no bound and takes 0 without a sync).
 * Both are asynchronous on `stream` and never set CPK_ENOMEM in
 * cpk_ctx_take_error.  n == 0 (nm == 0) is valid: d_out_off[0] = 0.  A piece
 * of 0 words sizes to 0.  d_in is only read. */
int cpk_packed_size_batch(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                          uint32_t n, uint64_t max_seg_words, uint64_t *d_out_off, void *stream);
int cpk_packed_size_messages(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off,
                             uint32_t nseg, const uint64_t *d_msg_seg_off, uint32_t nm,
                             uint64_t max_seg_words, uint64_t *d_out_off, void *stream);
/* The same from host memory; synchronous.  The words are staged through the
 * context's pinned chunk pipeline as cpk_encode_host stages them (host to
 * device only, in chunks of whole pieces or messages of CPK_HOST_CHUNK_MB, one
 * large piece in its sub-chunks); only the offsets are copied back. */
int cpk_packed_size_host(cpk_ctx ctx, const void *h_in, const uint64_t *h_seg_word_off,
                         uint32_t n, uint64_t *h_out_off);
int cpk_packed_size_messages_host(cpk_ctx ctx, const void *h_in, const uint64_t *h_seg_word_off,
                                  uint32_t nseg, const uint64_t *h_msg_seg_off, uint32_t nm,
                                  uint64_t *h_out_off);

/* Encode to caller-given offsets: the pieces of cpk_encode_batch, packed to
 * where the caller says -- into an allocation of exactly the size
 * cpk_packed_size_batch reported, behind a length prefix or record header the
 * caller writes itself, or each message into a slot of its own (a ring-buffer
 * entry, a send buffer per peer) in any order.  A slot that is too small is
 * refused as the reference's sink refuses a write that does not fit
 * (ArrayOutputStream.write, ArrayOutputStream.java:36-44).
 *   Pieces: d_in, d_seg_word_off[n+1], max_seg_words as for cpk_encode_batch
 *     (0 = unknown: d_seg_word_off[0], [n] are read back, synchronising
 *     `stream`; so is a bound so loose that n pieces of it would make more than
 *     2^25 chunks of 8192 words).
 *   Groups: group g is the pieces [d_grp_piece_off[g], d_grp_piece_off[g+1]),
 *     uint64[ng+1], device, [0] = 0 and [ng] = n.  The pieces of a group are
 *     packed back to back, each from fresh run state (bit-exact with the
 *     reference's write() per piece), as cpk_encode_batch packs a whole batch.
 *     d_grp_piece_off == NULL: ng must equal n, every piece is its own group.
 *     A message is a group whose first piece is its table words; this call
 *     builds no tables.
 *   Placement: group g's first byte is d_out + d_dst_off[g] (uint64[ng], any
 *     byte alignment, slots in any order) and its slot is d_dst_cap[g] bytes
 *     (uint64[ng]).  d_dst_cap == NULL: every slot runs to out_cap -- d_dst_off
 *     may then be the first n entries of what cpk_packed_size_batch wrote, as
 *     they stand.  d_out is 16-byte aligned, out_cap its bytes.  Slots of
 *     different groups must not overlap (overlapping slots leave their bytes
 *     undefined; nothing outside [0, out_cap) is stored even then).
 *   Written: d_piece_off[n], the absolute byte offset in d_out of every
 *     piece's first packed byte; d_grp_len[ng], the group's exact packed bytes,
 *     also when it did not fit; d_status[ng], int32, every entry:
 *       CPK_OK;
 *       CPK_ENOMEM when d_grp_len[g] > d_dst_cap[g] or the slot passes out_cap
 *         (no byte outside the group's own slot is stored, the bytes inside it
 *         are undefined);
 *       CPK_EINVAL when a piece of the group is larger than a nonzero
 *         max_seg_words (or 2^31 words and more): it is sized 0, the group's
 *         bytes and length are undefined.
 *   Bytes of d_out that belong to no group's packed bytes are never written:
 *     not the gaps between slots, not the unused tail of a slot, not the bytes
 *     that share a 16-byte line with the start or end of a group.
 * Asynchronous on `stream`, no host synchronisation when max_seg_words != 0;
 * cpk_ctx_take_error is not involved.  n == 0 or ng == 0 is valid.  Missing or
 * misaligned pointers, or d_grp_piece_off == NULL with ng != n: CPK_EINVAL.
 * The kernel is the single pass (a workgroup per 8192-word chunk) with each
 * group's base given: a group of one piece of at most one chunk waits for no
 * other; the chunks of a larger group look back over that group only.  Its
 * dense or sparse form is chosen on the device from a sample of the words
 * (CPK_AT_FORM=dense|sparse, read at context creation, forces one).  There is
 * no host form: the host encoders' packed bytes already pass through pinned
 * staging, from where the caller's own memcpy places them. */
int cpk_encode_batch_at(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off, uint32_t n,
                        uint64_t max_seg_words,
                        const uint64_t *d_grp_piece_off, uint32_t ng,
                        void *d_out, uint64_t out_cap,
                        const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                        uint64_t *d_piece_off, uint64_t *d_grp_len, int32_t *d_status,
                        void *stream);

/* Encode messages to caller-given slots: SerializePacked.write of message m
 * into the slot d_out + [d_dst_off[m], d_dst_off[m] + d_dst_cap[m]) -- one
 * packed message per ring-buffer entry or per-peer send buffer, the segment
 * tables built on the device.  The sender's side of cpk_decode_messages_at.
 *   Messages: d_in, d_seg_word_off[nseg+1], d_msg_seg_off[nm+1] and
 *     max_seg_words as for cpk_encode_messages; max_seg_words is required
 *     (> 0).  Message m's table is built exactly as cpk_encode_messages builds
 *     it, no table word comes from caller memory, and the message's bytes and
 *     length are what cpk_encode_messages writes for it: packed(table) ||
 *     packed(segment 0) || ..., each piece from fresh run state.
 *   Placement: as cpk_encode_batch_at.  d_dst_off[nm], any byte alignment and
 *     any order; d_dst_cap[nm], or NULL: every slot runs to out_cap; d_out is
 *     16-byte aligned, out_cap its bytes; slots must not overlap.
 *   Written: d_piece_off[nm + nseg], the absolute byte offset in d_out of
 *     every piece's first packed byte in message order (table, then segments,
 *     then the next message: the indexing of cpk_encode_messages' d_out_off,
 *     message m's table is entry d_msg_seg_off[m] + m); d_msg_len[nm], the
 *     message's exact packed bytes, also when it did not fit; d_status[nm],
 *     int32, every entry:
 *       CPK_OK;
 *       CPK_ENOMEM when d_msg_len[m] > d_dst_cap[m] or the slot passes out_cap
 *         (no byte outside the message's own slot is stored, the bytes inside
 *         it are undefined; a table that does not fit is not stored at all);
 *       CPK_EINVAL when a segment of the message is larger than max_seg_words
 *         (or 2^31 words and more): the message's length and bytes are
 *         undefined, nothing outside its slot is stored.
 *   Bytes of d_out that belong to no message's packed bytes are never written:
 *     not the gaps between slots, not the unused tail of a slot, not the bytes
 *     that share a 16-byte line with a message's first or last byte or with
 *     the seam between a table and its first segment.
 * Asynchronous on `stream`, no host synchronisation and no read-back at any
 * nm; cpk_ctx_take_error is not involved, and neither a refused slot nor a
 * segment over max_seg_words sets the context's error bits.  nm == 0 is
 * valid.  Missing or misaligned pointers, max_seg_words == 0: CPK_EINVAL with
 * nothing written.  CPK_EUNSUPPORTED when max_seg_words is so loose that nseg
 * segments of it pass both forms' workspace bounds (4 GiB of the size pass's
 * rows, 24 bytes per 64 words, and 2^25 chunks of 8192 words).
 * Round trip: d_dst_off and d_msg_len are cpk_decode_messages_at's d_src_off
 * and d_src_len; the lengths are the per-message differences of what
 * cpk_packed_size_messages reports.
 * Two forms, both enqueued, one picked on the device by the rule
 * cpk_encode_batch applies to the same segments as pieces: the two passes (a
 * wave per segment, each segment emitted against its own slot's end; nothing
 * of a refused message is stored), or, for like-sized segments of 4 Ki words
 * and more or one dominant segment, the placed single pass of
 * cpk_encode_batch_at over the segments behind each table (dense or sparse
 * as there, CPK_AT_FORM).  CPK_MSG_AT_FORM=wave|place, read at context
 * creation, forces a form.  There is no host form. */
int cpk_encode_messages_at(cpk_ctx ctx, const void *d_in, const uint64_t *d_seg_word_off, uint32_t nseg,
                           const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t max_seg_words,
                           void *d_out, uint64_t out_cap,
                           const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                           uint64_t *d_piece_off, uint64_t *d_msg_len, int32_t *d_status,
                           void *stream);

/* Batch decode of n pieces, device-resident (replaces n calls of
 * PackedInputStream.read, PackedInputStream.java:35-140).
 *   d_packed        : packed bytes, readable up to round_up(d_in_off[n], 16).
 *   d_in_off        : uint64[n+1], device; piece i's packed bytes.
 *   d_seg_word_off  : uint64[n+1], device; piece i's unpacked words.
 *   d_out           : 8-byte aligned; piece i -> words d_seg_word_off[i]...
 *   d_status        : int32[n], device, written per piece (CPK_* codes).
 * Returns CPK_OK if launched; per-piece results are in d_status.  A batch of
 * at most 32 pieces reads its extent back (one sync of `stream`): with
 * >= 8 MiB of words (1 Mi words) per piece on average it is decoded as one
 * stream, 256-byte blocks in parallel, the batch decoders running after it
 * only when some piece did not end exactly at its packed range's end.
 * Confinement (the packed bytes may come from outside): whatever a piece's
 * status, no word outside [d_seg_word_off[0], d_seg_word_off[n]) is written
 * and no entry outside d_status[0..n); d_packed, d_in_off and d_seg_word_off
 * are only read.  A piece whose packed range is empty and whose word count is
 * not 0 is CPK_ETRUNC and no word is written for it.  The words of any other
 * piece that is not CPK_OK are undefined; the words of a CPK_OK piece are the
 * reference's, whatever its neighbours' statuses.  One exception: a batch
 * that takes the one-stream path above (at most 32 pieces, 1 Mi words each on
 * average) reads on across piece boundaries before the batch decoders set
 * the statuses, so there words may be written for a failed piece with an
 * empty range too (the bounds of the first sentence are cpk_decode_stream's
 * there, which are the same). */
int cpk_decode_batch(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off,
                     const uint64_t *d_seg_word_off, uint32_t n, void *d_out,
                     int32_t *d_status, void *stream);

/* Unpacked sizes without decoding: how many words each piece's packed bytes
 * unpack to -- the d_seg_word_off every decode entry point must be given --
 * for a caller that knows byte ranges and nothing else (length-prefixed packed
 * blobs, pieces of cpk_encode_batch kept with d_out_off alone, packed bytes
 * taken from outside, to be sized before anything is allocated for them: one
 * 00 ff pair expands 2 bytes to 2 KiB).  The mirror image of
 * cpk_packed_size_batch; upstream Cap'n Proto's C++ library has it as
 * computeUnpackedSizeInWords.  Device traffic is the packed bytes, read once,
 * plus 12 bytes per piece.
 *   Piece i is the packed bytes [d_in_off[i], d_in_off[i+1]), parsed from
 *     fresh state as PackedInputStream.java:82-134 reads records.
 *   d_packed        : 16-byte aligned, readable up to round_up(d_in_off[n], 16)
 *                     as for cpk_decode_batch.  It is only read.
 *   d_in_off        : uint64[n+1], device.
 *   d_seg_word_off  : uint64[n+1], device, written: [0] = 0, [i+1] - [i] =
 *                     piece i's words, [n] = the total.  It can be handed to
 *                     cpk_decode_batch as it stands.
 *   d_status        : int32[n], device, written: CPK_OK when the range ends
 *                     exactly at a record's end (an empty range is CPK_OK with
 *                     0 words); CPK_ETRUNC when it ends inside a record: a tag
 *                     without all its bytes, 00 without its count, ff without
 *                     its word and count, a literal run cut short.  No other
 *                     status can occur: CPK_EOVERRUN and CPK_ETRAILING need a
 *                     word count to be measured against.
 * A piece that is not CPK_OK sizes to 0 words: cpk_decode_batch given these
 * offsets then reports CPK_ETRAILING for that piece and writes nothing for it
 * (its behaviour for 0 words and a nonempty range), and the good pieces
 * decode.  For a CPK_OK piece the size is the one and only word count for
 * which cpk_decode_batch returns CPK_OK on that range.
 * The device form is asynchronous on `stream` and returns CPK_OK once
 * launched; CPK_EINVAL for missing or misaligned pointers.  n == 0 is valid:
 * [0] = 0.  cpk_ctx_take_error is not involved.  As cpk_decode_batch does, a
 * batch of at most 32 pieces reads its extent back (one sync of `stream`; not
 * while the stream is being captured): a piece of n * 64 KiB or more is then
 * sized by the 256-byte block map over its own bytes (a piece that starts off
 * a 16-byte line, or whose map is irregular, by one wave like the others).
 * A piece of more than 2^32-1 packed bytes is handled as cpk_decode_batch
 * handles it: the wave-per-piece form, like the batch decoders, takes the
 * range's length modulo 2^32 (the result is then that of the shorter range,
 * not an error), and only the block-map path of a batch of at most 32 pieces
 * measures in 64 bits, as that call's stream path does.
 * The host form is synchronous: the packed bytes go up through the context's
 * pinned chunk pipeline in chunks of whole pieces (CPK_HOST_CHUNK_MB), only
 * the offsets and statuses come back.  It returns CPK_OK iff every piece is
 * CPK_OK, otherwise the first failed piece's status, as cpk_decode_host. */
int cpk_unpacked_size_batch(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off,
                            uint32_t n, uint64_t *d_seg_word_off, int32_t *d_status, void *stream);
int cpk_unpacked_size_host(cpk_ctx ctx, const void *h_packed, const uint64_t *h_in_off,
                           uint32_t n, uint64_t *h_seg_word_off, int32_t *h_status);

/* Decode from caller-given ranges: the pieces of cpk_decode_batch, each group
 * of them read from the byte range the caller names -- the receiver's side of
 * cpk_encode_batch_at: length-prefixed blobs, ring-buffer entries, a send
 * buffer per peer, slots in any order, decoded where they lie with no
 * compaction first.
 *   Ranges: group g's packed bytes are d_packed + [d_src_off[g], d_src_off[g] +
 *     d_src_len[g]), uint64[ng] each, device.  Any byte alignment, any order,
 *     gaps between them; ranges may overlap or coincide: the input is only
 *     read.  d_packed is 16-byte aligned and readable up to
 *     round_up(in_cap, 16); no byte at or past that is read, and d_packed is
 *     never written.
 *   Groups: group g is the pieces [d_grp_piece_off[g], d_grp_piece_off[g+1]),
 *     uint64[ng+1], device, [0] = 0 and [ng] = n.  The pieces of a group are
 *     decoded back to back from the group's range, each read() from fresh
 *     state; a piece that fills leaves the rest of the range to the next (the
 *     stream rule of cpk_decode_stream, per group).  d_grp_piece_off == NULL:
 *     ng must equal n, every piece is its own group.  No segment table is read
 *     here: the caller gives every piece's word count
 *     (cpk_decode_messages_at reads the tables from the slots).
 *   Output: piece i goes to words [d_seg_word_off[i], d_seg_word_off[i+1]) of
 *     d_out (8-byte aligned), tiled as in cpk_decode_batch -- so the offsets
 *     cpk_unpacked_size_batch_at writes can be handed over as they stand.
 *     There is no output scatter per piece.
 *   Written: d_status[n], int32, one entry per piece; d_grp_status[ng], int32;
 *     d_grp_used[ng], uint64: the bytes the group's pieces consumed.  The
 *     group's status is
 *       CPK_OK;
 *       the first failed piece's status (CPK_ETRUNC, CPK_EOVERRUN): that piece
 *         and every later piece of the group carry it, d_grp_used[g] is 0;
 *       CPK_ETRAILING when all pieces filled before the range ended:
 *         d_grp_used[g] < d_src_len[g] says by how much.  For a group of one
 *         piece this is the batch form's CPK_ETRAILING, also in d_status;
 *       CPK_EUNSUPPORTED when d_src_len[g] > 2^32-1: reported, not taken
 *         modulo 2^32 as the batch form takes it (checked first: such a range
 *         need not lie below in_cap to be told so);
 *       CPK_EINVAL when the range passes in_cap (the sum computed
 *         saturating), or for a piece of 2^31 words or more.
 *     A group refused with the last two has nothing of its range read and
 *     none of its words written; all its pieces carry its status and
 *     d_grp_used[g] is 0.
 *   Confinement, as for cpk_decode_batch: no word outside [d_seg_word_off[0],
 *     d_seg_word_off[n]) is written.  A CPK_OK piece's words are the
 *     reference's, whatever the other groups' statuses; a group's failure
 *     touches no other group.  A piece with words and an empty range is
 *     CPK_ETRUNC and no word is written for it.
 * Round trip: the arrays of a cpk_encode_batch_at call decode what that call
 * wrote -- d_dst_off as d_src_off, d_grp_len as d_src_len, the same
 * d_grp_piece_off and d_seg_word_off.
 * Asynchronous on `stream`, no host synchronisation at any n;
 * cpk_ctx_take_error is not involved.  n == 0 or ng == 0 is valid.  Missing or
 * misaligned pointers, or d_grp_piece_off == NULL with ng != n: CPK_EINVAL; a
 * call that returns anything but CPK_OK writes nothing.  The decoder is chosen
 * on the device as for cpk_decode_batch, from the ranges' summed bytes
 * (CPK_DECODER forces one).
 * Limit: a piece is decoded by one wave, whatever its size.  The "few large
 * pieces as one stream" path of cpk_decode_batch needs a read-back and is not
 * taken here: for one large range use cpk_decode_stream on it.  There is no
 * host form. */
int cpk_decode_batch_at(cpk_ctx ctx,
                        const void *d_packed, uint64_t in_cap,
                        const uint64_t *d_src_off, const uint64_t *d_src_len,
                        const uint64_t *d_grp_piece_off, uint32_t ng,
                        const uint64_t *d_seg_word_off, uint32_t n,
                        void *d_out,
                        int32_t *d_status, int32_t *d_grp_status, uint64_t *d_grp_used,
                        void *stream);

/* cpk_unpacked_size_batch over n ranges: piece i is the packed bytes d_packed +
 * [d_src_off[i], d_src_off[i] + d_src_len[i]), placed as for
 * cpk_decode_batch_at (any alignment and order, gaps, overlaps; d_packed
 * 16-byte aligned, readable up to round_up(in_cap, 16), only read).
 *   d_seg_word_off  : uint64[n+1], device, written: [0] = 0, [i+1] - [i] =
 *                     piece i's words, [n] = the total; it can be handed to
 *                     cpk_decode_batch_at as it stands.
 *   d_status        : int32[n], device, written: CPK_OK, or CPK_ETRUNC with
 *                     the piece sized 0, as cpk_unpacked_size_batch; and the
 *                     two range statuses of cpk_decode_batch_at, the piece
 *                     sized 0 and nothing of it read: CPK_EUNSUPPORTED for
 *                     d_src_len[i] > 2^32-1, CPK_EINVAL for a range that
 *                     passes in_cap.
 * A piece sized 0 for a nonempty range is CPK_ETRAILING to cpk_decode_batch_at
 * with nothing written, and the good pieces decode (a refused range stays
 * refused there).  Asynchronous on `stream` with no host synchronisation: the
 * wave-per-piece form only, no read-back and no block-map path.  n == 0 is
 * valid: [0] = 0.  CPK_EINVAL for missing or misaligned pointers. */
int cpk_unpacked_size_batch_at(cpk_ctx ctx,
                               const void *d_packed, uint64_t in_cap,
                               const uint64_t *d_src_off, const uint64_t *d_src_len, uint32_t n,
                               uint64_t *d_seg_word_off, int32_t *d_status, void *stream);

/* Stream decode (Serialize.read over PackedInputStream, Serialize.java:
 * 165-175): pieces 0..n-1 are decoded back to back from one packed stream of
 * `avail` bytes; each piece's read() stops when the piece is full and leaves
 * the rest to the next (PackedInputStream.java:35-140), so no packed offsets
 * are needed.  d_in_off[n+1] is written with the piece boundaries found
 * (d_in_off[n] = bytes consumed).  A failed piece stops the stream: it and
 * every later piece get its status.  Asynchronous on `stream`.
 * Confinement, as for cpk_decode_batch: whatever the statuses, no word outside
 * [d_seg_word_off[0], d_seg_word_off[n]) is written and no entry outside
 * d_status[0..n) and d_in_off[0..n]; d_packed and d_seg_word_off are only
 * read.  The words of the pieces before the first failed one are the
 * reference's and their boundaries exact; the words and boundaries of the
 * failed piece and of every later one are undefined. */
int cpk_decode_stream(cpk_ctx ctx, const void *d_packed, uint64_t avail,
                      const uint64_t *d_seg_word_off, uint32_t n, void *d_out,
                      uint64_t *d_in_off, int32_t *d_status, void *stream);

/* Batch of packed messages (Serialize.read over PackedInputStream for each,
 * SerializePacked.read, Serialize.java:119-178): message m is the packed
 * bytes [d_msg_off[m], d_msg_off[m+1]) -- its segment table (two read()
 * calls: the first word, then 4 * (count & ~1) bytes), validated, then its
 * segments back to back.  Segments of all messages are written contiguously
 * in message order:
 *   d_msg_seg_off   : uint64[nm+1], written: message m's segments are
 *                     [d_msg_seg_off[m], d_msg_seg_off[m+1]) (none when its
 *                     table failed).
 *   d_seg_word_off  : uint64[segments+1], written: segment words in d_out.
 *   d_seg_in_off    : uint64[segments], written: segment packed starts.
 *   d_seg_status    : int32[segments], written (a failed segment stops its
 *                     message: later segments carry its status).
 *   d_msg_status    : int32[nm], written: CPK_OK, the table's error
 *                     (CPK_EFRAME, CPK_ETRUNC, ...), the first failed
 *                     segment's, or CPK_ETRAILING if the message's bytes
 *                     outlast its segments.
 *   traversal_limit_words: ReaderOptions.traversalLimitInWords (reference
 *                     default 8 Mi words).
 *   h_totals[2]     : host, written: total words, total segments.
 * The call synchronises `stream` once (to read the totals) and returns
 * CPK_ENOMEM, without decoding, if they exceed out_cap_words / seg_cap.
 * d_packed readable up to round_up(d_msg_off[nm], 16). */
int cpk_decode_messages(cpk_ctx ctx, const void *d_packed, const uint64_t *d_msg_off, uint32_t nm,
                        uint64_t traversal_limit_words, void *d_out, uint64_t out_cap_words,
                        uint64_t *d_seg_word_off, uint64_t *d_seg_in_off, int32_t *d_seg_status,
                        uint32_t seg_cap, uint64_t *d_msg_seg_off, int32_t *d_msg_status,
                        uint64_t *h_totals, void *stream);

/* Decode messages from caller-given ranges: cpk_decode_messages' framing on
 * cpk_decode_batch_at's ranges -- what a receiver of packed messages holds:
 * ring-buffer entries, length-prefixed records, a send buffer per peer.  The
 * segment tables are read from the slots where they lie, so the caller gives
 * byte ranges and no word counts, and the capacity verdict is made on the
 * device: the call never returns to the host between the tables and the
 * decode.  Semantics: SerializePacked.read on each range (Serialize.read over
 * PackedInputStream, Serialize.java:119-178).
 *   Ranges: message m is the packed bytes d_packed + [d_src_off[m],
 *     d_src_off[m] + d_src_len[m]), uint64[nm] each, device.  Any byte
 *     alignment, any order, gaps; ranges may overlap or coincide: the input is
 *     only read.  d_packed is 16-byte aligned and readable up to
 *     round_up(in_cap, 16); no byte at or past that is read.  A range is
 *     refused before a byte of it is read, as cpk_decode_batch_at refuses it:
 *     CPK_EUNSUPPORTED for d_src_len[m] > 2^32-1 (checked first), CPK_EINVAL
 *     for a range that passes in_cap (the sum computed saturating).
 *   Table: read from the front of the range as cpk_decode_messages reads it
 *     (the first word, then 4 * (count & ~1) bytes) with the same checks in
 *     the same order: count <= 512, sizes >= 0, total <=
 *     traversal_limit_words, segments <= 2^28-1 words.  A failed table gives
 *     the message its status (CPK_EFRAME, CPK_ETRUNC, CPK_EOVERRUN), no
 *     segments and no words.
 *   Capacity: a message whose range and table are good is accepted.
 *     d_totals[CPK_MAT_TOTALS], uint64, device, written whatever the
 *     capacities: [0] the words and [1] the segments of all accepted
 *     messages, [2] the accepted messages that fit.  Message m fits iff, over
 *     the accepted messages in index order, its words end at or below
 *     out_cap_words and its segments at or below seg_cap: the fitting
 *     messages are a prefix of the accepted ones.  An accepted message that
 *     does not fit is CPK_ENOMEM: nothing past its table is read, and no
 *     word, segment entry or segment status is written for it.  d_out and the
 *     three segment arrays may be NULL with capacities 0: every accepted
 *     message is then CPK_ENOMEM and d_totals says what to allocate -- one
 *     preliminary call sizes everything.
 *   d_msg_seg_off : uint64[nm+1], written in full: [0] = 0, [m+1] - [m] the
 *     table's count for an accepted message, fitting or not, 0 otherwise;
 *     [nm] = d_totals[1] (values may exceed seg_cap).
 *   For the fitting messages the segments are tiled in message order in d_out
 *     (8-byte aligned) as cpk_decode_messages tiles them: d_seg_word_off[j]
 *     and [j+1] bound segment j's words, d_seg_in_off[j] is the absolute byte
 *     offset in d_packed of its first packed byte, d_seg_status[j] its status
 *     (a failed segment stops its message: the later segments of that message
 *     carry its status, and their d_seg_in_off is 0).  With F the segments'
 *     end of the last fitting message, d_seg_word_off is written for [0, F],
 *     d_seg_in_off and d_seg_status for [0, F), nothing beyond.  There is no
 *     output scatter per message.
 *   d_msg_status  : int32[nm], written, in this precedence: the range's
 *     status; the table's; CPK_ENOMEM; the first failed segment's;
 *     CPK_ETRAILING when the segments end before the range does; CPK_OK.
 *   d_msg_used    : uint64[nm], written: the bytes consumed, table plus
 *     segments, when the status is CPK_OK or CPK_ETRAILING -- where a ring
 *     reader finds the next record --, otherwise 0.
 *   Confinement: no word outside [0, out_cap_words) of d_out is written, no
 *     entry past seg_cap (seg_cap + 1 for d_seg_word_off) or nm (nm + 1 for
 *     d_msg_seg_off).  A CPK_OK message's words are the reference's, whatever
 *     its neighbours' statuses; a failed message touches no other message.
 * Round trip: groups encoded by cpk_encode_batch_at whose first piece is the
 * table's words are messages; d_dst_off and d_grp_len of that call serve as
 * d_src_off and d_src_len.
 * Asynchronous on `stream`, no host synchronisation and no read-back at any
 * nm; cpk_ctx_take_error is not involved.  nm == 0 is valid:
 * d_msg_seg_off[0] = 0, d_totals = {0, 0, 0}.  Missing or misaligned pointers
 * (the checks of cpk_decode_batch_at; an array may be NULL only where its
 * capacity or nm is 0): CPK_EINVAL, and nothing is written.  The decoder is
 * chosen on the device from the fitting messages' bytes and words
 * (CPK_DECODER forces one).
 * Limits: a message is decoded by one wave, as in cpk_decode_messages.  There
 * is no host form. */
#define CPK_MAT_TOTALS 3
int cpk_decode_messages_at(cpk_ctx ctx,
                           const void *d_packed, uint64_t in_cap,
                           const uint64_t *d_src_off, const uint64_t *d_src_len, uint32_t nm,
                           uint64_t traversal_limit_words,
                           void *d_out, uint64_t out_cap_words,
                           uint64_t *d_seg_word_off, uint64_t *d_seg_in_off, int32_t *d_seg_status,
                           uint32_t seg_cap,
                           uint64_t *d_msg_seg_off, int32_t *d_msg_status, uint64_t *d_msg_used,
                           uint64_t *d_totals, void *stream);

/* One message from the front of a packed byte stream whose length is not
 * known in advance (SerializePacked.read / readFromUnbuffered: Serialize.read
 * over PackedInputStream, Serialize.java:119-178), in one enqueue with no
 * host sync.  The device reads the segment table as the reference does (the
 * first word, then 4 * (count & ~1) bytes), validates it (count <= 512,
 * sizes >= 0, total <= traversal_limit_words, segments <= 2^28-1 words,
 * Serialize.java:45-53, :125-163) and decodes every segment back to back
 * from where the table ends.  Bytes after the message are left alone.
 *   d_packed : the stream's first `avail` bytes, 16-byte aligned, readable
 *              up to round_up(avail, 16).
 *   d_out    : 8-byte aligned, out_cap_words + CPK_MSG_HEAD_WORDS words: the
 *              table's words land first, segment i is words
 *              [d_info[4 + i], d_info[5 + i]).
 *   d_info   : uint64[CPK_MSG_INFO_WORDS], device, written: [0] status (as
 *              int64), [1] bytes consumed, [2] segment count, [3] total
 *              segment words, [4 .. 4 + count] segment word offsets.
 * Status: CPK_OK; CPK_ETRUNC when the bytes end inside the message (a
 * channel reader takes more and calls again); CPK_EFRAME / CPK_EOVERRUN as
 * Serialize.read would throw; CPK_ENOMEM when the segments exceed
 * out_cap_words (nothing decoded; [2] and [3] say how many).  Only
 * min(avail, 10 * (out_cap_words + CPK_MSG_HEAD_WORDS) + 16) bytes are read. */
#define CPK_MSG_HEAD_WORDS 257
#define CPK_MSG_INFO_WORDS 517
int cpk_read_message(cpk_ctx ctx, const void *d_packed, uint64_t avail, uint64_t traversal_limit_words,
                     void *d_out, uint64_t out_cap_words, uint64_t *d_info, void *stream);

/* A whole stream of packed messages whose boundaries are not known: a log
 * file, a pipe or a socket buffer that SerializePacked.write was called on
 * message after message.  The semantics are those of a loop of
 * SerializePacked.read (SerializePacked.java:51-66, Serialize.java:119-178)
 * over the first `avail` bytes, until the bytes are used up or a message
 * fails; the device finds the messages itself, in one call.
 *   d_packed : 16-byte aligned, readable up to round_up(avail, 16).
 *   d_out    : 8-byte aligned, out_cap_words words; receives the flat
 *              unpacked stream: every message's table words followed by its
 *              segments, in stream order.  The segments are addressed in place:
 *   d_seg_begin, d_seg_words : uint64[seg_cap], written: segment j's first
 *              word in d_out and its length, segments numbered over all
 *              messages in order.
 *   d_msg_seg_off : uint64[msg_cap + 1], written: message m's segments are
 *              [d_msg_seg_off[m], d_msg_seg_off[m + 1]).
 *   d_msg_off : uint64[msg_cap + 1], written: message m's first packed byte;
 *              d_msg_off[nm] = the bytes consumed.
 *   h_info   : host, uint64[CPK_MS_INFO_WORDS], written after one
 *              synchronisation of `stream` (a second only for a stream of
 *              more than a message per 64 bytes): [0] complete messages nm,
 *              [1] their segments, [2] their words in d_out, [3] bytes
 *              consumed (the packed end of the last complete message), [4]
 *              tail status as int64: CPK_OK iff [3] == avail, else what the
 *              reference's next read would throw on the bytes from [3] on:
 *              CPK_ETRUNC, CPK_EFRAME, or CPK_EOVERRUN (a run across a piece
 *              boundary: first table word / rest of the table / segment /
 *              next message).
 * Messages before the first failing one are decoded and reported, nothing
 * for the failing one or the bytes after it (d_out beyond [2] words and the
 * arrays beyond the counts are undefined).  Each message is held against
 * traversal_limit_words on its own.
 * Returns CPK_OK whenever the call ran (the tail status is in h_info[4]);
 * CPK_ENOMEM, with nothing guaranteed in the output arrays, when
 * out_cap_words, msg_cap or seg_cap is too small: h_info[2] is then the
 * words d_out must hold (the whole stream's), and h_info[0], [1] the
 * messages and segments, exact whenever out_cap_words was enough -- so two
 * preliminary calls at most size everything (the arrays may be NULL with a
 * capacity of 0).  CPK_EINVAL for misaligned or missing pointers.  avail ==
 * 0: no messages, tail CPK_OK. */
#define CPK_MS_INFO_WORDS 5
int cpk_decode_message_stream(cpk_ctx ctx, const void *d_packed, uint64_t avail,
                              uint64_t traversal_limit_words,
                              void *d_out, uint64_t out_cap_words,
                              uint64_t *d_msg_off, uint64_t *d_msg_seg_off, uint32_t msg_cap,
                              uint64_t *d_seg_begin, uint64_t *d_seg_words, uint32_t seg_cap,
                              uint64_t *h_info, void *stream);
/* The same with every pointer in host memory; synchronous (the bytes staged
 * through the context's pinned slot, the words and the four arrays copied
 * back; the same CPK_ENOMEM sizing protocol). */
int cpk_decode_message_stream_host(cpk_ctx ctx, const void *h_packed, uint64_t avail,
                                   uint64_t traversal_limit_words,
                                   void *h_out, uint64_t out_cap_words,
                                   uint64_t *h_msg_off, uint64_t *h_msg_seg_off, uint32_t msg_cap,
                                   uint64_t *h_seg_begin, uint64_t *h_seg_words, uint32_t seg_cap,
                                   uint64_t *h_info);

/* The other direction: a whole stream of UNPACKED messages whose boundaries
 * are not known -- a file or a socket buffer that Serialize.write was called
 * on message after message (Serialize.java:256-288), or the flat output of
 * cpk_decode_message_stream, data words edited in place -- packed in one
 * call.  The semantics are those of a loop of
 * Serialize.read(ReadableByteChannel) (Serialize.java:119-178) over the first
 * `avail_words` words, each message read then written with
 * SerializePacked.write (SerializePacked.java:101-134): one piece for the
 * message's segment table, all of its words in one write(), and one per
 * segment (a segment of 0 words packs to 0 bytes), every piece from fresh run
 * state, packed back to back in stream order.  The pieces of the complete
 * messages tile the input words exactly.  The device finds the messages
 * itself (one wave follows the tables), so the host never learns a boundary.
 *   d_in     : 8-byte aligned, avail_words words.
 *   d_out    : 16-byte aligned, out_cap bytes; as in the *_cap forms no byte
 *              at or past d_out + out_cap is ever stored.
 *   d_out_off : uint64[piece_cap + 1], written: packed piece offsets in
 *              stream order (table, segments; next message); the last entry
 *              is the total.
 *   d_msg_piece : uint64[msg_cap + 1], written: message m's pieces are
 *              [d_msg_piece[m], d_msg_piece[m + 1]), so its packed bytes
 *              start at d_out_off[d_msg_piece[m]].
 *   h_info   : host, uint64[CPK_EMS_INFO_WORDS], written: [0] complete
 *              messages, [1] their pieces (messages + segments), [2] words
 *              consumed (the end of the last complete message), [3] packed
 *              bytes: the exact total, also when out_cap was too small, [4]
 *              tail status as int64, [5] the largest piece in words.
 * Tail status: CPK_OK iff every word was consumed; CPK_ETRUNC when the words
 * end inside a message (after the first table word when the rest of the
 * table is due, inside the rest of the table, inside a segment); CPK_EFRAME
 * for a table Serialize.read refuses, the checks in its order: a count over
 * 512, a negative size, a total over traversal_limit_words, a segment over
 * 2^28-1 words.  Each message is held against the limit on its own.
 * Messages before the first failing one are packed and reported, nothing for
 * the failing one or the words after it.
 * Divergence from the reference: the table is packed as its words stand in
 * the input.  Serialize.write zeroes the pad half-word of an even-count
 * table and Serialize.read ignores it, so the output equals the reference's
 * read followed by write exactly when the pad is zero -- every stream a
 * conforming writer made.  A nonzero pad is kept: the call is lossless,
 * decoding its output gives the input words back.
 * Returns CPK_OK whenever the call ran (the tail status is in h_info[4]);
 * CPK_ENOMEM, with nothing guaranteed in the outputs, when piece_cap, msg_cap
 * or out_cap is too small: h_info[0] and [1] are then exact and say what the
 * arrays need, and [3] is exact whenever the arrays were large enough.  The
 * arrays and d_out may be NULL with a capacity of 0, so two preliminary
 * calls at most size everything: the first with everything NULL / 0 gives
 * [0] and [1]; the second with the arrays and out_cap 0 gives [3].
 * CPK_EINVAL for misaligned or missing pointers.  avail_words == 0: no
 * messages, tail CPK_OK, d_out_off[0] = 0.
 * The call synchronises `stream` twice: once after the chain (the piece
 * count sizes the encoders' launches; a call whose arrays are too small
 * returns here) and once after the encoders, for [3] and the capacity
 * verdict.  A capacity overrun is reported by the return value and leaves
 * nothing behind for cpk_ctx_take_error. */
#define CPK_EMS_INFO_WORDS 6
int cpk_encode_message_stream(cpk_ctx ctx, const void *d_in, uint64_t avail_words,
                              uint64_t traversal_limit_words,
                              void *d_out, uint64_t out_cap,
                              uint64_t *d_out_off, uint32_t piece_cap,
                              uint64_t *d_msg_piece, uint32_t msg_cap,
                              uint64_t *h_info, void *stream);
/* The same with every pointer in host memory; synchronous (the words staged
 * whole through the context's pinned slot, the packed bytes and the two
 * arrays copied back; the same CPK_ENOMEM sizing protocol).  It does not
 * pipeline the stream in chunks: copy in, pack, copy out, one after the
 * other. */
int cpk_encode_message_stream_host(cpk_ctx ctx, const void *h_in, uint64_t avail_words,
                                   uint64_t traversal_limit_words,
                                   void *h_out, uint64_t out_cap,
                                   uint64_t *h_out_off, uint32_t piece_cap,
                                   uint64_t *h_msg_piece, uint32_t msg_cap,
                                   uint64_t *h_info);

/* Host-memory convenience forms (the socket/file ByteBuffer path,
 * SerializePacked.java:75-96, :119-134).  Synchronous.  encode_host and
 * decode_host pipeline the batch in chunks of whole pieces through pinned
 * staging kept in the context (CPK_HOST_CHUNK_MB, default 256;
 * CPK_HOST_THREADS copy threads, default 8); decode_stream_host and
 * read_message_host stage only the bytes the pieces can reach (10 per word
 * at most), the rest of `avail` may be later messages.
 *   cpk_read_message_host: cpk_read_message over host memory; h_out gets the
 *                    segments only, back to back (out_cap_words words), and
 *                    h_info[4 + i] their word offsets from 0.  Two syncs (the
 *                    info row, then the words).
 *   cpk_encode_host: h_out capacity >= cpk_batch_packed_capacity();
 *                    h_out_off[n+1] written.
 *   cpk_decode_host: h_status[n] written; returns CPK_OK iff all pieces OK. */
int cpk_encode_host(cpk_ctx ctx, const void *h_in, const uint64_t *h_seg_word_off,
                    uint32_t n, void *h_out, uint64_t h_out_cap, uint64_t *h_out_off);
/* Gather form of cpk_encode_host (builder segments in
 * their own direct ByteBuffers, DefaultAllocator.java:56-62, packed without a
 * host-side concatenation): piece i is the h_swo[i+1] - h_swo[i] words at
 * h_pieces[i] (any host pointer, no alignment needed; NULL only for an empty
 * piece); h_swo is read only for the sizes.  Output as cpk_encode_host. */
int cpk_encode_host_gather(cpk_ctx ctx, const void *const *h_pieces, const uint64_t *h_swo,
                           uint32_t n, void *h_out, uint64_t h_out_cap, uint64_t *h_out_off);
int cpk_decode_host(cpk_ctx ctx, const void *h_packed, const uint64_t *h_in_off,
                    const uint64_t *h_seg_word_off, uint32_t n, void *h_out,
                    int32_t *h_status);
int cpk_decode_stream_host(cpk_ctx ctx, const void *h_packed, uint64_t avail,
                           const uint64_t *h_seg_word_off, uint32_t n, void *h_out,
                           uint64_t *h_in_off, int32_t *h_status);
int cpk_read_message_host(cpk_ctx ctx, const void *h_packed, uint64_t avail, uint64_t traversal_limit_words,
                          void *h_out, uint64_t out_cap_words, uint64_t *h_info);

/* Host-memory forms of the message batches (staged whole through device
 * memory; synchronous).
 *   cpk_encode_messages_host: h_msg_seg_off[0] = 0, [nm] = nseg; h_out
 *     capacity as cpk_encode_messages; h_out_off[nm + nseg + 1] written.
 *   cpk_decode_messages_host: h_msg_seg_off[nm+1], h_msg_status[nm],
 *     h_seg_word_off[segments+1] (segment words in h_out) and h_totals[2]
 *     written; CPK_ENOMEM (with the totals) if out_cap_words / seg_cap are
 *     too small -- call with 0 / NULL first to size them; otherwise returns
 *     the first failed message's status or CPK_OK. */
int cpk_encode_messages_host(cpk_ctx ctx, const void *h_in, const uint64_t *h_seg_word_off,
                             uint32_t nseg, const uint64_t *h_msg_seg_off, uint32_t nm,
                             void *h_out, uint64_t h_out_cap, uint64_t *h_out_off);
/* Gather form of cpk_encode_messages_host: segment i is the
 * h_swo[i+1] - h_swo[i] words at h_segs[i] (any host pointer; NULL only for
 * an empty segment), e.g. each MessageBuilder's own segment buffers
 * (BuilderArena.getSegmentsForOutput, BuilderArena.java:143-154).  Output as
 * cpk_encode_messages_host. */
int cpk_encode_messages_host_gather(cpk_ctx ctx, const void *const *h_segs, const uint64_t *h_swo,
                                    uint32_t nseg, const uint64_t *h_msg_seg_off, uint32_t nm,
                                    void *h_out, uint64_t h_out_cap, uint64_t *h_out_off);
int cpk_decode_messages_host(cpk_ctx ctx, const void *h_packed, const uint64_t *h_msg_off,
                             uint32_t nm, uint64_t traversal_limit_words, void *h_out,
                             uint64_t out_cap_words, uint64_t *h_seg_word_off, uint32_t seg_cap,
                             uint64_t *h_msg_seg_off, int32_t *h_msg_status, uint64_t *h_totals);

/* ---- benchmark support (synthetic device-resident workloads) ---- */

/* Device generator of the synthetic segments described in SURVEY.md 8d:
 * a 2-state Markov chain over words (thresholds out of 2^31: FastRand draws
 * are never negative), seeded per
 * segment from (cfg, segment index).  Identical stream to the host copy in
 * oracle/packed_oracle.c:cpko_generate. */
typedef struct {
  uint64_t t_zero0, t_z2n, t_n2z, t_qbyte;
  uint32_t cfg, pad;
} cpk_gen_params;

int cpk_generate(cpk_ctx ctx, const cpk_gen_params *params, const uint64_t *d_seg_word_off,
                 uint32_t n, void *d_out, void *stream);

/* Counts 8-byte words that differ between two device buffers into
 * *d_mismatch (uint64, device, accumulated; zero it first). */
int cpk_count_mismatch(cpk_ctx ctx, const void *d_a, const void *d_b, uint64_t words,
                       uint64_t *d_mismatch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
