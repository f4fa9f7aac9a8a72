"""Layouts that put a batch's word or byte offsets above and across 2^32 bytes
(no GPU, no pytest; tests/test_high_offsets_cases.py pins this file,
tests/test_gpu_high_offsets.py hands the layouts to every device entry point).

Every device entry point takes 64-bit offsets next to deliberately 32-bit
quantities.  A batch of a few hundred KiB whose offsets are large shows a
truncated base as well as a batch of gigabytes does: the pointer passed is the
base of an arena of a little over 4 GiB of which only the batch's own bytes and
a guard window on either side are touched, so a truncated offset still lands
inside the arena and shows as wrong bytes against the oracle.

A batch is given by relative offsets (rel[0] = 0); a layout moves it so that
LINE = 2^32 bytes falls

  above     below the whole batch: the first offset is LINE + 129 words for
            word arrays, LINE + 48 + r bytes (r = 0, 5, 15) for byte ranges
  edge      exactly on a piece boundary, pieces with content on both sides
  straddle  strictly inside a piece, off the 64-word (16-byte) grid counted
            from the piece's start
  middle    like-sized batches: inside the middle piece, 4097 words from its
            start (one word past half an 8192-word chunk)
"""
from __future__ import annotations

import numpy as np

LINE = 1 << 32                    # bytes
GUARD = 64 * 1024                 # bytes of guard window on either side of a batch
WORD_ARENA = (1 << 29) + (1 << 20)   # int64 words
BYTE_ARENA = (1 << 32) + (1 << 23)   # bytes
LEAD_WORDS = 129
BYTE_PHASES = (0, 5, 15)
WORD_WHERE = ("above", "edge", "straddle")
LIKE_WHERE = WORD_WHERE + ("middle",)
BYTE_WHERE = ("above0", "above5", "above15", "edge", "straddle")
# the word position that goes with a byte position when both sides of a call are high
WORD_OF_BYTE = {"above0": "above", "above5": "above", "above15": "above", "edge": "edge", "straddle": "straddle"}

MIXED = [0, 1, 17, 63, 64, 65, 300, 2000, 4095, 4096, 8191, 8192, 8193, 20000]
LIKE = [8192] * 24
BIG = [300, 3 * 8192 + 5, 65]
MORE = [3 * 8192 + 5, 12000, 16384, 777, 5000]  # pieces of several decoder windows


def rel_off(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


class Layout:
    """A batch at an absolute position.  unit: 8 for word offsets, 1 for byte
    offsets; off: the absolute offsets, uint64[n+1]; piece: the piece that
    holds LINE (straddle, middle) or whose start is LINE (edge), None for
    above; rem: LINE's distance from that piece's start, in units."""

    def __init__(self, where, unit, off, piece, rem):
        self.where, self.unit, self.off, self.piece, self.rem = where, unit, off, piece, rem

    @property
    def lo(self):
        """First byte of the batch in its arena."""
        return int(self.off[0]) * self.unit

    @property
    def hi(self):
        return int(self.off[-1]) * self.unit

    def fits(self, arena_bytes):
        """The batch, its guard windows and the 16-byte line a reader may
        finish lie inside the arena."""
        return self.lo - GUARD >= 0 and (self.hi + 15) // 16 * 16 + GUARD <= arena_bytes

    def check(self):
        """What the layout promises; raises AssertionError."""
        off, u = self.off.astype(object), self.unit
        assert off[0] >= 0 and all(a <= b for a, b in zip(off, off[1:]))
        if self.where.startswith("above"):
            assert off[0] * u >= LINE and self.piece is None
            if u == 8:
                assert off[0] * u == LINE + 8 * LEAD_WORDS
            else:
                assert off[0] == LINE + 48 + int(self.where[5:]) and int(self.where[5:]) in BYTE_PHASES
            return
        k = self.piece
        if self.where == "edge":
            assert off[k] * u == LINE and self.rem == 0
            assert off[0] < off[k] < off[-1], "content on both sides of the line"
            return
        assert off[k] * u < LINE < off[k + 1] * u
        assert off[k] * u + self.rem * u == LINE
        grid = 64 if u == 8 else 16
        assert self.rem % grid != 0
        if self.where == "middle":
            assert self.rem == 4097 and k == (len(off) - 1) // 2


def _shift(where, unit, rel, k, rem):
    assert int(rel[0]) == 0 and LINE % unit == 0
    base = LINE // unit - int(rel[k]) - rem
    assert base >= 0
    return Layout(where, unit, (rel.astype(object) + base).astype(np.uint64), k, rem)


def _edge_piece(rel):
    """A boundary near the middle with content on both sides."""
    n = len(rel) - 1
    for k in sorted(range(1, n), key=lambda i: abs(i - n // 2)):
        if rel[0] < rel[k] < rel[n]:
            return k
    raise AssertionError("no inner boundary with content on both sides")


def _straddle(rel, grid):
    """(piece, rem): the longest piece but the last (so that pieces start
    above LINE too), LINE near its middle and off the grid."""
    ln = np.diff(rel.astype(np.int64))
    k = int(np.argmax(ln[:-1] if len(ln) > 1 else ln))
    n = int(ln[k])
    assert n >= 2, "no piece LINE can fall strictly inside"
    rem = n // 2 // grid * grid + grid // 2 + 1
    if rem >= n:
        rem = 1
    return k, rem


def place(rel, unit, where):
    """The batch `rel` (relative offsets in units of `unit` bytes) at `where`."""
    rel = np.asarray(rel, dtype=np.uint64)
    if where.startswith("above"):
        first = LINE // 8 + LEAD_WORDS if unit == 8 else LINE + 48 + int(where[5:])
        return Layout(where, unit, (rel.astype(object) + first).astype(np.uint64), None, None)
    if where == "edge":
        return _shift(where, unit, rel, _edge_piece(rel), 0)
    if where == "straddle":
        return _shift(where, unit, rel, *_straddle(rel, 64 if unit == 8 else 16))
    assert where == "middle" and unit == 8
    return _shift(where, unit, rel, (len(rel) - 1) // 2, 4097)


def place_words(sizes, where):
    return place(rel_off(sizes), 8, where)


def place_bytes(lengths, where):
    return place(rel_off(lengths), 1, where)


# ---- the batches ---------------------------------------------------------------
MIXES = {"uniform": [.25, .25, .25, .25], "dense": [.01, .7, .285, .005],
         "sparse": [.85, .05, .05, .05], "lonely_ff": [.45, .05, .05, .45]}  # (test_gpu_parity.py's class mixes)


def random_words(rng, n, probs):
    """test_gpu_parity.py's _random_words: zero words, words with one zero
    byte, with several, and all-nonzero words by the given shares."""
    kind = rng.choice(4, size=n, p=probs)
    w = rng.integers(1, 256, size=(n, 8), dtype=np.uint8)
    w[kind == 0] = 0
    one = np.where(kind == 1)[0]
    w[one, rng.integers(0, 8, size=one.size)] = 0
    for i in np.where(kind == 2)[0]:
        w[i, rng.choice(8, size=int(rng.integers(2, 8)), replace=False)] = 0
    return w.reshape(-1)


def word_batch(oracle, name):
    """-> (sizes, data as uint8): mixed (ragged sizes, the class mixes in
    turn: under the gate the two passes), like2 / like4 (24 x 8192 words of
    generator config 2 / 4: the single pass, dense and sparse), big (one
    piece of three chunks and five words between two small ones)."""
    if name == "mixed":
        rng = np.random.default_rng(2032)
        mixes = list(MIXES.values())
        return MIXED, np.concatenate([random_words(rng, s, mixes[i % 4]) for i, s in enumerate(MIXED)])
    sizes = {"like2": LIKE, "like4": LIKE, "big": BIG}[name]
    cfg = 4 if name == "like4" else 2
    return sizes, oracle.generate(oracle.preset(cfg), rel_off(sizes))


WORD_BATCHES = {"mixed": WORD_WHERE, "like2": LIKE_WHERE, "like4": LIKE_WHERE, "big": WORD_WHERE}
WORD_CASES = [(b, w) for b, ws in WORD_BATCHES.items() for w in ws]


def messages(nmsg):
    """nmsg messages of 1, 2, 3 and 9 segments in turn, the segments' sizes
    taken from MIXED (from its sizes up to 300 words when there are many
    messages, every fifteenth message from all of them), the bytes by the
    recipe of test_gpu_capacity.py::test_encode_messages_capacity."""
    rng = np.random.default_rng(77 + nmsg)
    small = [s for s in MIXED if s <= 300]
    msgs = []
    for i in range(nmsg):
        nseg = (1, 2, 3, 9)[i % 4]
        pool = MIXED if nmsg <= 60 or i % 15 == 7 else small
        sizes = [int(rng.choice(pool)) for _ in range(nseg)]
        msgs.append([(rng.integers(0, 256, size=8 * s, dtype=np.uint8)
                      * (rng.random(8 * s) < 0.6)).astype(np.uint8).tobytes() for s in sizes])
    return msgs


MESSAGE_COUNTS = (12, 300)  # 12: at most 1,024 pieces; 300: over 1,024 (the two-pass message path)


def table_bytes(msg):
    """The segment table of a message as Serialize.write lays it out (Serialize.java:256-273)."""
    tb = ((len(msg) - 1) & 0xffffffff).to_bytes(4, "little") + b"".join((len(s) // 8).to_bytes(4, "little") for s in msg)
    return tb + b"\0" * (-len(tb) % 8)


def message_piece_offsets(oracle, msgs):
    """Packed piece offsets in message order (table, segments) from oracle.pack."""
    woff, o = [0], 0
    for m in msgs:
        for piece in [table_bytes(m)] + list(m):
            o += len(oracle.pack(piece))
            woff.append(o)
    return np.asarray(woff, dtype=np.uint64)


# ---- packed batches for the decoders ---------------------------------------------
DECODE_N = (14, 40)
DECODE_CFG = {"sparse": 4, "dense": 3}
BAD = 6  # the piece of a decode batch that is replaced by a truncated one


def truncated_piece(style):
    """A first-window seam piece of tests/_packed_records.py (an F29 probe
    whose tag is the last byte of the block map's first window) cut in the
    middle of its literals, as first_window_cuts cuts it; the word count stays
    the whole piece's."""
    import _packed_records as R
    p = R.kWin - 1
    b = R.filled(p, style) + R.probe("F29") + R.filled(40, style, 1)
    return R.Case(f"win{R.kWin}/F29/tag@-1/{style}/cut@lits", R.Built(b.packed, b.words), style, p, "F29",
                  packed=b.packed[:p + 10 + 4 * 29], expect="ETRUNC")


def decode_batch(oracle, density, n):
    """A packed batch for the decoders -> (packed pieces as a list of bytes,
    word counts, the words as bytes or None per piece).  Sizes: MIXED, for
    n = 40 also MORE five times over and one piece more; generator config 4
    (sparse: the record index under the gate) or 3 (dense: the dense block
    map); piece BAD is a truncated piece of _packed_records.py."""
    assert n in DECODE_N
    sizes = list(MIXED) if n == 14 else list(MIXED) + MORE * 5 + [2049]
    assert len(sizes) == n
    swo = rel_off(sizes)
    data = oracle.generate(oracle.preset(DECODE_CFG[density]), swo)
    pk, off = oracle.pack_batch(data, swo)
    pk, data = pk.tobytes(), data.tobytes()
    pieces = [pk[int(off[i]):int(off[i + 1])] for i in range(n)]
    words = [data[8 * int(swo[i]):8 * int(swo[i + 1])] for i in range(n)]
    bad = truncated_piece("sparse" if density == "sparse" else "dense")
    pieces[BAD], sizes[BAD], words[BAD] = bad.packed, bad.nwords, None
    return pieces, sizes, words


def gate_of(pieces, sizes):
    """dec_gate_kernel's choice (decode_v2.hip) for the batch, as _packed_records.gate_of."""
    P, U = sum(len(p) for p in pieces), 8 * sum(sizes)
    return "index" if 100 * P < 15 * U else "dense" if 100 * P >= 80 * U else "map"


# (byte position of the packed side, word position of the output side; None: that side is low)
DECODE_PLACEMENTS = [(b, None) for b in BYTE_WHERE] + [(None, w) for w in WORD_WHERE] + \
    [(b, WORD_OF_BYTE[b]) for b in BYTE_WHERE]


def placement_id(p):
    return f"bytes-{p[0] or 'low'}+words-{p[1] or 'low'}"


# ---- streams ------------------------------------------------------------------------
# name -> (sizes, generator config): a stream for the one-wave reader, one for
# the one-workgroup reader (6-384 KiB) and one for the parallel blocks
STREAMS = {"small": ([17, 300, 0, 64], 2), "mid": (MIXED, 2), "large": (LIKE, 2)}
STREAM_BYTES = {"small": (0, 6 << 10), "mid": (6 << 10, 384 << 10), "large": (384 << 10, 1 << 40)}


def stream_position(length, where):
    """The 16-aligned byte position of a stream of `length` bytes: above the
    line, ending on it (the 16-byte line the reader finishes is the first
    above), or with the line inside."""
    if where == "above":
        return LINE + 48
    if where == "edge":
        return (LINE - length) // 16 * 16
    assert where == "straddle"
    return (LINE - length // 2) // 16 * 16 - 16


# ---- placed encode, high destinations ---------------------------------------------------
AT_GROUPS = [[300], [2000, 17], [64, 0, 4095, 65, 1], [8192], [8193, 63], [4096], [17, 300, 2000, 1, 64], [20000]]
AT_SHORT = 5  # the group whose slot is one byte short
AT_WHERE = ("cross", "abut")


def at_slots(group_bytes, where):
    """Slots for the groups' packed bytes, given in descending address order:
    the last group lowest.  cross: the lowest slot starts below LINE and its
    bytes cross it; abut: the lowest slot ends exactly at LINE and the next
    starts there.  Every other slot lies above LINE at some byte alignment,
    with gaps of 1..19 bytes; slot AT_SHORT is one byte short of its group.
    -> (dst_off, dst_cap), per group."""
    ng = len(group_bytes)
    cap = [b - 1 if g == AT_SHORT else b + (3 * g) % 8 for g, b in enumerate(group_bytes)]
    off = [0] * ng
    order = list(range(ng))[::-1]
    low = order[0]
    assert group_bytes[low] >= 2 and low != AT_SHORT and order[1] != AT_SHORT
    if where == "cross":
        off[low] = LINE - group_bytes[low] // 2 - 3
        cur = off[low] + cap[low] + 7
        assert cur > LINE
    else:
        assert where == "abut"
        cap[low] = group_bytes[low]
        off[low] = LINE - cap[low]
        cur = LINE
    for i, g in enumerate(order[1:]):
        off[g] = cur
        cur += cap[g] + 1 + (7 * i) % 19
    return off, cap


# ---- the packed output that itself passes 4 GiB ---------------------------------------------
PART3_CYCLE = [8192, 3000, 8191, 12000, 17, 4096]
PART3_BYTES = 4710 << 20  # about 4.6 GiB of words (config 3, P/U 0.967: about 4.45 GiB packed)


def part3_sizes():
    per = sum(PART3_CYCLE)
    return PART3_CYCLE * (PART3_BYTES // (8 * per) + 1)


def part3_sample(out_off, seed=5):
    """The pieces whose bytes are compared with the oracle: the piece that
    holds byte LINE, three on each side, the first, the last, 32 seeded
    random ones."""
    n = len(out_off) - 1
    k = int(np.searchsorted(out_off, LINE, side="right")) - 1
    assert 3 <= k < n - 3 and int(out_off[k]) <= LINE < int(out_off[k + 1])
    pick = set(range(k - 3, k + 4)) | {0, n - 1}
    pick |= {int(i) for i in np.random.default_rng(seed).integers(0, n, size=32)}
    return k, sorted(pick)
