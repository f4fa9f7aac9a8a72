"""Single packed messages that sit on every edge of message framing, for the
framing tests (no GPU, no pytest; tests/test_message_frames.py pins this file
against the oracle, tests/test_gpu_message_frames.py feeds it to every device
reader).

Framing is Serialize.read (Serialize.java:119-178) over PackedInputStream:
three kinds of read() in order -- the first table word, the rest of the table
(4 * (count & ~1) bytes), each segment -- with the table's checks between
them.  Six device readers restate it; the cases here are the inputs on which a
restatement goes wrong:

  count   1-4 (odd / even padding); 127|128|129 (the chains hold the first word
          and 63 table words in their 64-word head); 191|192|193, 255|256|257
          (their 64 sizes a round); 511, 512; refused counts
  pad     a nonzero pad half-word on an even count (ignored on read)
  neg     bit 31 in the size of segment 0, 1, 63, 64, 65, 126, 127, 128, 511,
          and the cases that pin the ORDER of the reference's checks
  limit   total = limit, limit + 1 (limit 20 and the default), a sum that
          needs more than 32 bits
  big     a segment of 2^28 words (makeByteBufferForWords throws when the
          read REACHES it, so a failing segment before it wins), at index 0,
          1, 64, 511; 2^28 - 1 words with no data
  run     a 0x00 / 0xFF run across each piece boundary (CPK_EOVERRUN)
  trunc   a six-segment message cut after every byte of its table and at
          every segment's start
  zero    `00 00`, once and 300 times

A case's `packed` is built piece by piece with oracle.pack, so a piece
boundary falls exactly where the case wants it; `words` is the same message
unpacked (table words, then segments) where that form exists and has the same
status; `status` and `nseg` are literals, what the case was built to produce.
Segment k's word j is (k + 1) | (j + 1) << 16: every word names its place, so
a size taken from a neighbouring lane shows in the contents.  No case holds
more than a few KiB of real words: a huge size is declared, not supplied.
"""
from __future__ import annotations

import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np

OK, ETRUNC, EOVERRUN, EFRAME = 0, -2, -3, -7
LIMIT = 8 * 1024 * 1024          # ReaderOptions.DEFAULT_TRAVERSAL_LIMIT_IN_WORDS
BIG_LIMIT = 1 << 40
MAX_SEGMENT_WORDS = (1 << 28) - 1  # Serialize.java:45
# the oracle's output capacity: its CPK_EINVAL for a short buffer would hide
# the real status (the zero pages are never touched beyond the words read)
SMALL_CAP = 64 * 1024
HUGE_CAP = (1 << 31) + 4096

# the piece boundaries a run can cross (include/capnp_packed.h, CPK_EOVERRUN)
BOUNDARIES = ("first-word", "table/segment-0:zero", "table/segment-0:literal", "segment/segment:first",
              "segment/segment:last", "next-message")

Case = namedtuple("Case", "name packed words limit status nseg boundary declared tseg")


def seg(k: int, n: int) -> bytes:
    """Segment k's n words."""
    return struct.pack(f"<{n}Q", *[(k + 1) | (j + 1) << 16 for j in range(n)])


def table(sizes, pad=0, count_field=None) -> bytes:
    """The segment table's words (Serialize.java:256-273) as bytes."""
    n = len(sizes)
    t = [n - 1 if count_field is None else count_field] + list(sizes)
    if n % 2 == 0:
        t.append(pad)
    return struct.pack(f"<{len(t)}I", *t)


def sizes_for(count: int):
    """0..3 words, every neighbour different."""
    return [(i + 1) % 4 for i in range(count)]


def pieces(oracle, t: bytes, segs) -> bytes:
    """SerializePacked.write piece by piece: first table word, rest, segments."""
    out = oracle.pack(t[:8])
    if len(t) > 8:
        out += oracle.pack(t[8:])
    return out + b"".join(oracle.pack(s) for s in segs)


@lru_cache(maxsize=None)
def corpus():
    """name -> Case, in a fixed order."""
    import oracle
    cases = {}

    def add(name, packed, words, status, nseg, limit=LIMIT, boundary=None, declared=0, tseg=None):
        """(declared: the words the table declares when the oracle needs room for them; tseg: the segments
        of a table that passes every check and has no oversized segment -- what a batch reader counts for
        the message -- when the message is not read whole)"""
        assert name not in cases, name
        cases[name] = Case(name, bytes(packed), None if words is None else bytes(words), limit, status, nseg,
                           boundary, declared, nseg if tseg is None else tseg)

    def good(name, sizes, pad=0):
        t = table(sizes, pad)
        segs = [seg(k, s) for k, s in enumerate(sizes)]
        add(name, pieces(oracle, t, segs), t + b"".join(segs), OK, len(sizes))

    # ---- counts
    for c in (1, 2, 3, 4, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512):
        good(f"count/{c}", sizes_for(c))
    good("count/512-all-empty", [0] * 512)
    good("count/3-last-empty", [2, 1, 0])
    for raw, tag in ((512, "513"), (0x80000000, "0x80000000"), (0xFFFFFFFF, "0xffffffff")):
        # thrown before the rest of the table is read: nothing need follow
        t = struct.pack("<II", raw, 1)
        add(f"count/refused-{tag}/alone", oracle.pack(t), t, EFRAME, 0)
    t = struct.pack("<II", 512, 1) + struct.pack("<512I", *([1] * 512))
    add("count/refused-513/with-rest", oracle.pack(t[:8]) + oracle.pack(t[8:]) + oracle.pack(seg(0, 1)), t + seg(0, 1),
        EFRAME, 0)

    # ---- padding
    good("pad/2-nonzero", sizes_for(2), pad=0xDEADBEEF)
    good("pad/512-nonzero", sizes_for(512), pad=0x00010000)

    # ---- negative sizes
    for i in (0, 1, 63, 64, 65, 126, 127, 128, 511):
        sizes = sizes_for(min(i + 2, 512))
        sizes[i] |= 0x80000000
        t = table(sizes)
        add(f"neg/segment-{i}", pieces(oracle, t, []), t, EFRAME, 0)
    t = table([0x80000003, 1, 2])
    add("neg/segment-0/alone", oracle.pack(t[:8]), t[:8], EFRAME, 0)  # (:135-137, before the rest is read)
    t = table([1, 2, 3, 0x80000001, 2])
    add("neg/segment-3/rest-cut", oracle.pack(t[:8]) + oracle.pack(t[8:])[:-1], t[:-8], ETRUNC, 0)  # (read, then checked)
    t = table([LIMIT, 1, 2, 3])
    add("limit/over/rest-cut", oracle.pack(t[:8]) + oracle.pack(t[8:])[:-1], t[:-8], ETRUNC, 0)

    # ---- traversal limit
    for name, sizes, status in (("limit/20-equal", [7, 6, 7], OK), ("limit/20-plus-1", [7, 7, 7], EFRAME)):
        t = table(sizes)
        segs = [seg(k, s) for k, s in enumerate(sizes)]
        add(name, pieces(oracle, t, segs), t + b"".join(segs), status, 3 if status == OK else 0, limit=20)
    t = table([LIMIT - 5, 2, 3])  # (passes the check; its words are not there)
    add("limit/default-equal-no-data", pieces(oracle, t, []), t, ETRUNC, 0, declared=LIMIT, tseg=3)
    t = table([LIMIT - 5, 3, 3])
    add("limit/default-plus-1", pieces(oracle, t, []), t, EFRAME, 0)
    t = table([MAX_SEGMENT_WORDS] * 20)  # (5 * 2^30 - 20 words: a 32-bit sum would pass 2^31)
    add("limit/sum-over-32-bits", pieces(oracle, t, []), t, EFRAME, 0, limit=1 << 31)

    # ---- oversized segment
    big = MAX_SEGMENT_WORDS + 1
    t = table([big])
    add("big/at-0", pieces(oracle, t, []), t, EFRAME, 0, limit=BIG_LIMIT, declared=big)
    for at in (1, 64, 511):
        # (the chains look for the first oversized lane: at 64 and 511 that search crosses a round)
        sizes = ([3] if at == 1 else [1] * at) + [big]
        t = table(sizes)
        segs = [seg(k, s) for k, s in enumerate(sizes[:-1])]
        head = oracle.pack(t[:8]) + oracle.pack(t[8:]) + b"".join(oracle.pack(s) for s in segs[:-1])
        kw = dict(limit=BIG_LIMIT, declared=big + sum(sizes[:-1]))
        add(f"big/at-{at}/earlier-complete", head + oracle.pack(segs[-1]), t + b"".join(segs), EFRAME, 0, **kw)
        short = segs[-1][:-8]  # (the last earlier segment a word short)
        add(f"big/at-{at}/earlier-truncated", head + oracle.pack(short), t + b"".join(segs[:-1]) + short, ETRUNC, 0,
            **kw)
        add(f"big/at-{at}/earlier-overrun", head + b"\x00\x05", None, EOVERRUN, 0, **kw)
    t = table([MAX_SEGMENT_WORDS])
    add("big/minus-1-no-data", pieces(oracle, t, []), t, ETRUNC, 0, limit=BIG_LIMIT, declared=MAX_SEGMENT_WORDS,
        tseg=1)

    # ---- runs across every piece boundary
    add("run/first-word", b"\x00\x01", None, EOVERRUN, 0, boundary="first-word")
    # (the rest of the table ends in a zero word; segment 0 leads with one)
    t = table([2, 1, 0, 0])
    s0 = bytes(8) + seg(0, 2)[8:]
    add("run/table-into-segment-0/zero", oracle.pack(t[:8]) + oracle.pack(t[8:] + s0) + oracle.pack(seg(1, 1)), None,
        EOVERRUN, 0, boundary="table/segment-0:zero")
    # (the rest of the table all nonzero bytes, and segment 0's first word too)
    t = table([0x01010101] * 4, pad=0x01010101)
    add("run/table-into-segment-0/literal", oracle.pack(t[:8]) + oracle.pack(t[8:] + b"\x07" * 8), None, EOVERRUN, 0,
        limit=BIG_LIMIT, boundary="table/segment-0:literal", declared=4 * 0x01010101)
    for k, which in ((0, "first"), (2, "last")):  # (k = 0 and k = count - 2 of four segments)
        sizes = [2, 2, 2, 2]
        t = table(sizes)
        segs = [seg(i, 2) for i in range(4)]
        segs[k] = segs[k][:8] + bytes(8)
        segs[k + 1] = bytes(8) + segs[k + 1][8:]
        body = b"".join(oracle.pack(s) for s in segs[:k]) + oracle.pack(segs[k] + segs[k + 1]) + \
            b"".join(oracle.pack(s) for s in segs[k + 2:])
        add(f"run/segment-{k}-into-{k + 1}", oracle.pack(t[:8]) + oracle.pack(t[8:]) + body, None, EOVERRUN, 0,
            boundary=f"segment/segment:{which}", tseg=4)
    # (the next message's first word is an all-zero table: one empty segment)
    t = table([2, 2])
    last = seg(1, 2)[:8] + bytes(8)
    add("run/into-next-message", oracle.pack(t[:8]) + oracle.pack(t[8:]) + oracle.pack(seg(0, 2)) +
        oracle.pack(last + bytes(8)), None, EOVERRUN, 0, boundary="next-message", tseg=2)

    # ---- truncation: six segments, a table of four words
    sizes = [1, 2, 3, 1, 2, 3]
    t = table(sizes)
    segs = [seg(k, s) for k, s in enumerate(sizes)]
    tp = oracle.pack(t[:8]) + oracle.pack(t[8:])
    whole = tp + b"".join(oracle.pack(s) for s in segs)
    for cut in range(1, len(tp)):
        add(f"trunc/table@{cut}", whole[:cut], None, ETRUNC, 0)
    pos = len(tp)
    for k, s in enumerate(segs):
        add(f"trunc/segment-{k}@start", whole[:pos], t + b"".join(segs[:k]), ETRUNC, 0, tseg=6)
        add(f"trunc/segment-{k}@first-byte", whole[:pos + 1], None, ETRUNC, 0, tseg=6)
        pos += len(oracle.pack(s))
    assert pos == len(whole)

    # ---- the smallest streams
    add("zero/one", b"\x00\x00", bytes(8), OK, 1)
    add("zero/300", b"\x00\x00" * 300, bytes(8 * 300), OK, 1)  # (one message read; 299 behind it)
    return cases


NAMES = tuple(corpus())


def oracle_cap(case) -> int:
    """The output capacity the oracle needs to reach this case's real status."""
    return HUGE_CAP if case.declared > SMALL_CAP // 8 else SMALL_CAP


def _dense(rng, n):
    return rng.integers(1, 256, size=8 * n, dtype=np.uint8).tobytes()


@lru_cache(maxsize=None)
def tails():
    """(tail_small, its messages, tail_large, its messages): valid messages to
    put behind a case -- about 100 bytes, and over 128 KiB of a few hundred
    small messages (their words without a zero byte: 8 packed bytes each)."""
    import oracle
    rng = np.random.default_rng(20261020)
    small = [[_dense(rng, 3), b""], [_dense(rng, 4)], [seg(0, 2), seg(1, 1), _dense(rng, 2)]]
    large = [[_dense(rng, 18 + i % 5), _dense(rng, 20 + i % 3)] + ([b""] if i % 7 == 0 else []) for i in range(420)]
    return (b"".join(oracle.write_message(m) for m in small), small,
            b"".join(oracle.write_message(m) for m in large), large)
