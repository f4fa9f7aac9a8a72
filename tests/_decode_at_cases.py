"""Placed layouts for cpk_decode_batch_at / cpk_unpacked_size_batch_at and a
model of what they must report.

place() puts packed byte strings (pieces, or groups of pieces back to back)
into slots of one buffer: the slots in a given order, a gap before each, and
every byte that belongs to no slot taken from a filler that would be dangerous
if it were read as records:
  ff      0xFF tags: each claims 8 literal bytes, a count and a literal run
  00ff    zero runs of 255 words, 2 KiB of output per pair
  ff8ff   a 0xFF tag, eight bytes, then 0xFF as the count: 255 literal words
The model is the oracle's: oracle.unpack_batch on the compacted batch for
pieces of their own, the oracle's read() piece after piece for a group (the
stream rule), plus the range rules of the header."""
import numpy as np

OK, EINVAL, ETRUNC, EOVERRUN, ETRAILING, EUNSUPPORTED = 0, -1, -2, -3, -4, -8

FILLERS = {"ff": b"\xff", "00ff": b"\x00\xff", "ff8ff": b"\xff" + bytes(range(1, 9)) + b"\xff"}
ORDERS = ("forward", "reversed", "shuffled")


def slot_order(n, order):
    """order[k] = the item that lies in the k-th slot of the buffer."""
    if order == "forward":
        return list(range(n))
    if order == "reversed":
        return list(range(n - 1, -1, -1))
    assert order == "shuffled"
    return [int(i) for i in np.random.default_rng(20251).permutation(n)]


def default_gap(k):
    """Bytes before the k-th slot: every alignment of a slot's start occurs."""
    return (7 * k + 3) % 23


def place(items, order="forward", gap=default_gap, filler="ff", tail=5):
    """-> (src_off uint64[n], src_len uint64[n], in_cap, buffer uint8[in_cap])
    for the byte strings `items`; in_cap is `tail` bytes past the last slot."""
    n = len(items)
    off = np.zeros(n, np.uint64)
    cur = 0
    for k, i in enumerate(slot_order(n, order)):
        cur += gap(k)
        off[i] = cur
        cur += len(items[i])
    in_cap = cur + tail
    pat = FILLERS[filler]
    buf = np.frombuffer((pat * (in_cap // len(pat) + 1))[:in_cap], np.uint8).copy()
    for i, b in enumerate(items):
        buf[int(off[i]):int(off[i]) + len(b)] = np.frombuffer(b, np.uint8)
    return off, np.array([len(b) for b in items], np.uint64), in_cap, buf


def extract(buf, src_off, src_len):
    """The slots' bytes, in item order."""
    return [buf[int(o):int(o) + int(l)].tobytes() for o, l in zip(src_off, src_len)]


def range_status(off, length, in_cap):
    """What the call says of a range before it reads a byte of it."""
    if length > 0xFFFFFFFF:
        return EUNSUPPORTED
    if off > in_cap or length > in_cap - off:
        return EINVAL
    return OK


def group_model(oracle, stream: bytes, words):
    """One group: its pieces of `words` words each read back to back from
    `stream`.  -> (piece statuses, piece bytes or None, group status, used)"""
    st, out, pos, fail = [], [], 0, OK
    for w in words:
        if fail != OK:
            st.append(fail)
            out.append(None)
        elif w == 0:
            st.append(OK)
            out.append(b"")
        else:
            s, data, used = oracle.unpack(stream[pos:pos + 10 * w + 16], 8 * w)
            st.append(s)
            out.append(data if s == OK else None)
            if s == OK:
                pos += used
            else:
                fail = s
    if fail != OK:
        return st, out, fail, 0
    if pos < len(stream):
        if len(words) == 1:
            st[0], out[0] = ETRAILING, None
        return st, out, ETRAILING, pos
    return st, out, OK, pos


def batch_model(oracle, streams, groups):
    """Every group of a call: groups[g] the word counts of group g's pieces,
    streams[g] its bytes.  -> (piece statuses int32[n], piece bytes list,
    group statuses int32[ng], used uint64[ng])"""
    pst, pout, gst, used = [], [], [], []
    for s, ws in zip(streams, groups):
        a, b, c, d = group_model(oracle, s, ws)
        pst += a
        pout += b
        gst.append(c)
        used.append(d)
    return np.array(pst, np.int32), pout, np.array(gst, np.int32), np.array(used, np.uint64)
