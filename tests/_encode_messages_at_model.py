"""What cpk_encode_messages_at must leave behind, in pure Python on the oracle
(oracle.pack per piece, checked against oracle.write_message per message):
the buffer image, the bytes of it that are defined, d_piece_off, d_msg_len and
d_status.  The rules are the header's:

  * message m's slot is [off, off + cap) with off + cap saturating at 2^64 - 1
    and cut at out_cap; cap None: the slot runs to out_cap;
  * CPK_EINVAL when a segment is over max_seg_words (length, offsets and the
    slot's bytes undefined);
  * CPK_ENOMEM when the slot passes out_cap (off > out_cap, or cap > out_cap -
    off) or the packed message is longer than the slot: the bytes inside the
    slot are undefined, unless the slot lies within out_cap and the table
    alone does not fit -- then nothing of the message is stored;
  * CPK_OK: exactly the message's packed bytes at off;
  * every other byte keeps what it held (the sentinel).

tests/test_encode_messages_at_model.py pins these rules on hand-written cases;
the GPU tests compare the device's results with this model."""
import numpy as np

OK, EINVAL, ENOMEM = 0, -1, -5
U64 = (1 << 64) - 1


def table_bytes(msg):
    """The segment table of a message as Serialize.write lays it out
    (Serialize.java:256-273): count - 1, the sizes, a pad to a whole word."""
    tb = ((len(msg) - 1) & 0xffffffff).to_bytes(4, "little") + b"".join((len(s) // 8).to_bytes(4, "little") for s in msg)
    return tb + b"\0" * (-len(tb) % 8)


_PACKS = {}


def pack(oracle, piece):
    """oracle.pack(piece), computed once per piece and left unchanged."""
    if piece not in _PACKS:
        _PACKS[piece] = oracle.pack(piece)
    return _PACKS[piece]


_MSGS = {}


def packed_pieces(oracle, msg):
    """[packed table, packed segment 0, ...]; their concatenation is checked
    against oracle.write_message once per message."""
    key = tuple(msg)
    if key not in _MSGS:
        packs = [pack(oracle, table_bytes(msg))] + [pack(oracle, s) for s in msg]
        assert b"".join(packs) == oracle.write_message(list(msg)), "the pieces are not SerializePacked.write's bytes"
        _MSGS[key] = packs
    return _MSGS[key]


def slot(off, cap, out_cap):
    """-> (passes, end): whether the slot passes out_cap, and the first byte
    past what may be stored of it."""
    if cap is None:
        return off > out_cap, out_cap
    end = min(min(off + cap, U64), out_cap)
    return off > out_cap or cap > out_cap - off, end


class Expected:
    def __init__(self, image, care, piece_off, msg_len, status, defined):
        self.image = image          # uint8[size]: the sentinel but for the CPK_OK messages' bytes
        self.care = care            # bool[size]: False inside a refused message's slot
        self.piece_off = piece_off  # per piece in message order (table, segments); None where undefined
        self.msg_len = msg_len      # per message; None where undefined
        self.status = status        # per message
        self.defined = defined      # per message: length and offsets are defined (not CPK_EINVAL)


def expected(oracle, msgs, dst_off, dst_cap, out_cap, max_seg_words, size, sentinel):
    """The model of one call over a buffer of `size` bytes (>= out_cap) filled
    with `sentinel`."""
    image = np.full(size, sentinel, np.uint8)
    care = np.ones(size, bool)
    piece_off, msg_len, status, defined = [], [], [], []
    for m, msg in enumerate(msgs):
        off = int(dst_off[m])
        cap = None if dst_cap is None else int(dst_cap[m])
        passes, end = slot(off, cap, out_cap)
        room = max(end - off, 0)
        inval = any(len(s) // 8 > max_seg_words or len(s) // 8 >= 1 << 31 for s in msg)
        if inval:
            status.append(EINVAL)
            msg_len.append(None)
            piece_off += [off] + [None] * len(msg)
            defined.append(False)
            care[min(off, out_cap):end] = False
            continue
        packs = packed_pieces(oracle, msg)
        n = sum(len(p) for p in packs)
        msg_len.append(n)
        defined.append(True)
        o = off
        for p in packs:
            piece_off.append(o & U64)
            o += len(p)
        if passes or n > room:
            status.append(ENOMEM)
            if passes or len(packs[0]) <= room:  # (a table that does not fit is not stored at all)
                care[min(off, out_cap):end] = False
            continue
        status.append(OK)
        image[off:off + n] = np.frombuffer(b"".join(packs), np.uint8)
    return Expected(image, care, piece_off, msg_len, status, defined)
