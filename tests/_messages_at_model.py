"""A model of cpk_decode_messages_at's contract (include/capnp_packed.h), built
from three things only: oracle.read_message for every verdict on a message's
bytes, _decode_at_cases.range_status for a range, and the fit rule.  No GPU, no
pytest; tests/test_messages_at_model.py checks it against the framing corpus.

The oracle's reader answers CPK_EINVAL exactly when a table has passed every
check of Serialize.read and declares more words than the output holds.  With no
output at all that tells a good table (with words) from a failed one without a
second restatement of the framing; the sizes are then taken from the table's
words as the oracle unpacks them.  A good table with an oversized segment is
not accepted: makeByteBufferForWords throws, and the oracle's status for the
whole message (an earlier segment's failure, else CPK_EFRAME) is the table's,
as csrc/packed_codec.hip:read_table has it.
"""
from __future__ import annotations

import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _decode_at_cases as D

OK, EINVAL, ETRUNC, EOVERRUN, ETRAILING, ENOMEM, EFRAME, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -7, -8
MAX_SEGMENT_WORDS = (1 << 28) - 1

# One message's bytes read with room for everything: accepted (range aside),
# the table's sizes (accepted only), the status with CPK_ETRAILING folded in,
# the segments' bytes (CPK_OK / CPK_ETRAILING only), the bytes consumed
Facts = namedtuple("Facts", "accepted sizes status segs used")


@lru_cache(maxsize=None)
def facts(data: bytes, limit: int) -> Facts:
    import oracle
    st, segs, used = oracle.read_message(data, limit, out_cap=0)
    if st == OK:  # (a good table of empty segments)
        sizes = tuple(0 for _ in segs)
    elif st != EINVAL:
        return Facts(False, (), st, None, 0)
    else:
        s1, first, u1 = oracle.unpack(data, 8)
        assert s1 == OK
        count = struct.unpack("<I", first[:4])[0] + 1
        sizes = [struct.unpack("<I", first[4:])[0]]
        if count > 1:
            s2, rest, _ = oracle.unpack(data[u1:], 4 * (count & ~1))
            assert s2 == OK
            sizes += list(struct.unpack(f"<{count & ~1}I", rest))[:count - 1]
        sizes = tuple(sizes)
        st, segs, used = oracle.read_message(data, limit, out_cap=8 * sum(sizes))
        assert st != EINVAL
        if max(sizes) > MAX_SEGMENT_WORDS:
            return Facts(False, (), st, None, 0)
    if st == OK and used < len(data):
        st = ETRAILING
    if st not in (OK, ETRAILING):
        return Facts(True, sizes, st, None, 0)
    return Facts(True, sizes, st, tuple(segs), used)


Model = namedtuple("Model", "status used mseg totals fits sizes segs swo F")


def fit(words, counts, out_cap_words, seg_cap):
    """The fit rule over the accepted messages in index order: words[m] and
    counts[m] are 0 for a message that is not accepted.  -> (the inclusive
    sums' verdict per message, words' scan, counts' scan)"""
    w = np.concatenate([[0], np.cumsum(np.asarray(words, dtype=object))])
    c = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=object))])
    return [w[m + 1] <= out_cap_words and c[m + 1] <= seg_cap for m in range(len(words))], w, c


def batch(buf, src_off, src_len, in_cap, limit, out_cap_words, seg_cap) -> Model:
    """What one call must report.  buf: the packed buffer's bytes (a range
    that is refused is never looked up in it)."""
    nm = len(src_off)
    fs, rs = [], []
    for o, l in zip(src_off, src_len):
        o, l = int(o), int(l)
        r = D.range_status(o, l, in_cap)
        rs.append(r)
        fs.append(facts(bytes(buf[o:o + l]), limit) if r == OK else Facts(False, (), r, None, 0))
    acc = [f.accepted for f in fs]
    words = [sum(f.sizes) for f in fs]
    counts = [len(f.sizes) for f in fs]
    ok, w, c = fit(words, counts, out_cap_words, seg_cap)
    fits = [a and k for a, k in zip(acc, ok)]
    # (monotone sums: the fitting messages are a prefix of the accepted ones)
    seen_nofit = False
    for a, f in zip(acc, fits):
        assert not (f and seen_nofit)
        seen_nofit |= a and not f
    status = [ENOMEM if a and not k else f.status for f, a, k in zip(fs, acc, fits)]
    used = [f.used if a and k else 0 for f, a, k in zip(fs, acc, fits)]
    F = max([int(c[m + 1]) for m in range(nm) if fits[m]], default=0)
    swo = [0] * (F + 1)
    for m in range(nm):
        if fits[m]:
            a = int(w[m])
            for i, s in enumerate(fs[m].sizes):
                swo[int(c[m]) + i] = a
                a += s
            swo[int(c[m + 1])] = a
    return Model(np.array(status, np.int32), np.array(used, np.uint64), [int(v) for v in c],
                 (int(w[nm]), int(c[nm]), sum(fits)), fits, [f.sizes for f in fs],
                 [f.segs if k else None for f, k in zip(fs, fits)], swo, F)
