"""Packed pieces built from records, for the decoder seam tests (no GPU, no
pytest; tests/test_packed_records.py pins this file against the oracle,
tests/test_gpu_decoder_seams.py feeds the corpora to every decoder form,
tests/test_gpu_decoder_confinement.py checks that nothing is written outside
the pieces).

A piece is a list of records, so the builder knows every record's packed byte
position and first output word (PackedInputStream.java:82-134 reads exactly
these three record kinds):

  Z(k)            00 k                      k + 1 zero words
  T(mask, bytes)  mask, popcount(mask) B    one word (mask not 00 / ff)
  F(k, ...)       ff, 8 B, k, 8k B          1 + k words, the 8k bytes verbatim

The decoders' geometry is parsed from the kernel sources, so a change of a
window, chunk or round size moves every sweep with it.  The window placement
rule (window_starts) is only used to put a probe somewhere; what a decoder
must produce is always the oracle's answer.
"""
from __future__ import annotations

import re
import zlib
from functools import lru_cache
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parents[1] / "capnproto-java_amd" / "csrc"

# name -> source file.  A constant is read from its declaration: a plain
# literal, or a simple integer expression of constants parsed before it
# (constexpr uint32_t kX = 64 * kY;).  Anything else fails loudly, so the
# sweeps never run on a value the kernels no longer use: the next author
# extends this table or the parser on purpose.
_CONSTANTS = {
    "kDecChunk": "packed_codec.hip",
    "kDecLook": "packed_codec.hip",
    "CPK_DEC_ROUND": "packed_codec.hip",
    "CPK_DEC_BLK": "packed_codec.hip",
    "CPK_DEC_SER_MAX": "packed_codec.hip",
    "kD2Chunk": "decode_v2.hip",
    "kD2NI": "decode_v2.hip",
    "kD2Round": "decode_v2.hip",
    "kSsBlock": "stream_split.hip",
    "kSsGroup": "stream_split.hip",
    "kMwWaves": "decode_mw.hip",
}


def parse_constant(text: str, name: str, known: dict) -> int:
    """The value of `name` as declared in `text`: after `constexpr TYPE` (as
    the first or a later declarator of the line) or `#define`."""
    m = re.search(r"^[ \t]*constexpr\s+\w+\s+(?:[^;\n]*,\s*)?" + name + r"\s*=\s*([^;,\n]*)[;,]", text, re.M) or \
        re.search(r"^[ \t]*#\s*define\s+" + name + r"[ \t]+([^\n]*?)[ \t]*(?://.*|/\*.*)?$", text, re.M)
    if m is None:
        raise AssertionError(f"{name}: no declaration found")
    expr = re.sub(r"\b(\d+)[uU]?[lL]{0,2}\b", r"\1", m.group(1))
    expr = re.sub(r"[A-Za-z_]\w*", lambda w: str(known[w.group(0)]) if w.group(0) in known else w.group(0), expr)
    if not re.fullmatch(r"[\d\s+\-*/()]+", expr):
        raise AssertionError(f"{name} = {m.group(1).strip()!r}: not an integer expression of parsed constants")
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def parse_constants() -> dict:
    """{name: value}; raises if a name is not found or cannot be evaluated."""
    out = {}
    for name, src in _CONSTANTS.items():
        out[name] = parse_constant((CSRC / src).read_text(), name, out)
    return out


CONST = parse_constants()
kDecChunk, kDecLook = CONST["kDecChunk"], CONST["kDecLook"]
kRound, kBlk, kDecSerMax = CONST["CPK_DEC_ROUND"], CONST["CPK_DEC_BLK"], CONST["CPK_DEC_SER_MAX"]
kD2Chunk, kD2NI, kD2Round = CONST["kD2Chunk"], CONST["kD2NI"], CONST["kD2Round"]
kSsBlock, kSsGroup, kMwWaves = CONST["kSsBlock"], CONST["kSsGroup"], CONST["kMwWaves"]
kWin = 64 * kDecChunk          # block-map window, packed bytes
kD2Win = 64 * kD2Chunk         # record-index window
kDecChkReach = kWin + 2064     # windows this close to the piece's end are checked
LONGEST = 1 + 8 + 1 + 8 * 255  # an F(255) record

STATUS = {0: "OK", -1: "EINVAL", -2: "ETRUNC", -3: "EOVERRUN", -4: "ETRAILING", -7: "EFRAME"}


# ---- records -------------------------------------------------------------
class Rec:
    """One record: kind ("Z3", "T1", "F29"), its packed bytes, its words."""
    __slots__ = ("kind", "packed", "words", "first_zeros")

    def __init__(self, kind, packed, words):
        self.kind, self.packed, self.words = kind, packed, words
        self.first_zeros = words[:8].count(0)  # zero bytes of the first word

    @property
    def nwords(self):
        return len(self.words) // 8


def Z(k: int) -> Rec:
    assert 0 <= k <= 255
    return Rec(f"Z{k}", bytes([0, k]), bytes(8 * (k + 1)))


def T(mask: int, data: bytes) -> Rec:
    assert 0 < mask < 255 and len(data) == bin(mask).count("1") and 0 not in data
    it = iter(data)
    word = bytes(next(it) if mask >> i & 1 else 0 for i in range(8))
    return Rec(f"T{len(data)}", bytes([mask]) + bytes(data), word)


def F(k: int, head: bytes, lits: bytes) -> Rec:
    assert 0 <= k <= 255 and len(head) == 8 and 0 not in head and len(lits) == 8 * k
    return Rec(f"F{k}", b"\xff" + bytes(head) + bytes([k]) + bytes(lits), bytes(head) + bytes(lits))


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _new_T(rng, nbytes: int) -> Rec:
    mask = 0
    for b in rng.choice(8, size=nbytes, replace=False):
        mask |= 1 << int(b)
    return T(mask, bytes(rng.integers(1, 256, size=nbytes, dtype=np.uint8)))


kPool = 64


@lru_cache(maxsize=None)
def _pool(kind: str, zero_lits: bool = False):
    """kPool fixed records of one kind: the corpora hold millions of
    records, drawn from these instead of made one by one."""
    rng = _rng("pool", kind, zero_lits)
    n = int(kind[1:])
    return [_new_T(rng, n) if kind[0] == "T" else rand_F(rng, n, zero_lits) for _ in range(kPool)]


def rand_T(rng, nbytes: int) -> Rec:
    """A tagged word with nbytes (1..7) nonzero bytes at random places."""
    return _pool(f"T{nbytes}")[int(rng.integers(kPool))]


def rand_Ts(rng, nbytes: int, count: int):
    pool = _pool(f"T{nbytes}")
    return [pool[i] for i in rng.integers(kPool, size=count)]


def rand_F(rng, k: int, zero_lits: bool = False) -> Rec:
    """An 0xFF record.  Its literal words keep at most one zero byte each
    (about a quarter of them have one), which is what the encoder's run
    accepts (PackedOutputStream.java:149-161); zero_lits: all-zero literal
    words, which only a decoder ever sees."""
    head = bytes(rng.integers(1, 256, size=8, dtype=np.uint8))
    if zero_lits:
        return F(k, head, bytes(8 * k))
    lits = rng.integers(1, 256, size=(k, 8), dtype=np.uint8)
    z = np.where(rng.random(k) < 0.25)[0]
    lits[z, rng.integers(0, 8, size=z.size)] = 0
    return F(k, head, lits.tobytes())


# ---- built pieces ----------------------------------------------------------
def canonical_pair(a: Rec, b: Rec) -> bool:
    """Would the encoder emit record b right after record a?  A zero run
    under its cap is never followed by a zero word; a literal run under its
    cap is followed by a word with two zero bytes or more
    (PackedOutputStream.java:119-161)."""
    if a.kind[0] == "Z" and a.kind != "Z255" and b.kind[0] == "Z":
        return False
    if a.kind[0] == "F" and a.kind != "F255" and b.first_zeros < 2:
        return False
    return True


def canonical_rec(r: Rec) -> bool:
    """Literal words of an 0xFF record with two zero bytes or more end the
    encoder's run."""
    if r.kind[0] != "F":
        return True
    w = np.frombuffer(r.words[8:], np.uint8).reshape(-1, 8)
    return bool(((w == 0).sum(axis=1) < 2).all())


class Built:
    """Records laid out: packed bytes, words, and whether the encoder would
    have written exactly these bytes for these words.  Built + Built joins
    two of them (the junction is checked for canonicity)."""
    __slots__ = ("packed", "words", "nrec", "first", "last", "canonical")

    def __init__(self, packed=b"", words=b"", nrec=0, first=None, last=None, canonical=True):
        self.packed, self.words, self.nrec = packed, words, nrec
        self.first, self.last, self.canonical = first, last, canonical

    @property
    def nwords(self):
        return len(self.words) // 8

    def __add__(self, o: "Built") -> "Built":
        if o.nrec == 0:
            return self
        if self.nrec == 0:
            return o
        return Built(self.packed + o.packed, self.words + o.words, self.nrec + o.nrec, self.first, o.last,
                     self.canonical and o.canonical and canonical_pair(self.last, o.first))


def built(records) -> Built:
    records = list(records)
    if not records:
        return Built()
    ok = all(canonical_rec(r) for r in records) and \
        all(canonical_pair(a, b) for a, b in zip(records, records[1:]))
    return Built(b"".join(r.packed for r in records), b"".join(r.words for r in records), len(records),
                 records[0], records[-1], ok)


def build(records):
    """-> (packed bytes, word count, [(byte_pos, first_word, kind)])."""
    index, pos, w = [], 0, 0
    for r in records:
        index.append((pos, w, r.kind))
        pos += len(r.packed)
        w += r.nwords
    return b"".join(r.packed for r in records), w, index


def parse_records(packed: bytes):
    """The record index of well-formed packed bytes, read back from the bytes
    alone (PackedInputStream.java:82-134): [(byte_pos, first_word, kind)]."""
    index, q, w = [], 0, 0
    while q < len(packed):
        tag = packed[q]
        if tag == 0:
            k = packed[q + 1]
            index.append((q, w, f"Z{k}"))
            q, w = q + 2, w + 1 + k
        elif tag == 255:
            k = packed[q + 9]
            index.append((q, w, f"F{k}"))
            q, w = q + 10 + 8 * k, w + 1 + k
        else:
            n = bin(tag).count("1")
            index.append((q, w, f"T{n}"))
            q, w = q + 1 + n, w + 1
    assert q == len(packed)
    return index


def window_starts(index, P: int, win: int, cap: int | None = None):
    """The decoders' window starts over one piece: the next window starts at
    the end of the last record whose tag lies in [e, min(e + win, P)); the
    record index additionally cuts a window at its cap-th record."""
    pos = [p for p, _, _ in index] + [P]
    starts, i = [], 0
    while i < len(index):
        starts.append(pos[i])
        j = i
        while j < len(index) and pos[j] < min(pos[i] + win, P):
            j += 1
        if cap is not None and j - i > cap:
            j = i + cap
        i = j
    return starts


# ---- fill ------------------------------------------------------------------
STYLES = ("sparse", "mid", "dense", "z0pair")


def fill(nbytes: int, style: str, seed=0):
    """Records totalling exactly nbytes packed bytes (0, or any nbytes >= 2;
    odd lengths get one three-byte T).

    sparse  Z(2), T pairs: 4 bytes per 4 words, 12.5 % of the words' bytes
            (dec_gate_kernel sends a batch under 15 % to the record index)
    mid     two-byte T records, 2 bytes per word: the block map; a 3072-byte
            window of them holds 1536 records, over the record index's cap
    dense   F(k), k in 16..64, each followed by a two-byte T (the encoder
            ends a literal run at such a word), the rest in 8-byte T: over
            80 % of the words' bytes, few records per window
    z0pair  Z(0) back to back (valid, never written by the encoder): two
            bytes per word like mid, every tag zero
    """
    assert nbytes == 0 or nbytes >= 2, nbytes
    rng = _rng("fill", nbytes, style, seed)
    recs = []
    left = nbytes
    if left % 2:
        recs.append(rand_T(rng, 2))
        left -= 3
    if style == "z0pair":
        return recs + [Z(0)] * (left // 2)
    if style == "mid":
        return recs + rand_Ts(rng, 1, left // 2)
    if style == "sparse":
        if left % 4:
            recs.append(rand_T(rng, 1))
            left -= 2
        z2 = Z(2)
        for t in rand_Ts(rng, 1, left // 4):
            recs += [z2, t]
        return recs
    assert style == "dense", style
    while left >= 12 + 8 * 16:
        k = int(rng.integers(16, 65))
        k = min(k, (left - 12) // 8)
        recs += [rand_F(rng, k), rand_T(rng, 1)]
        left -= 12 + 8 * k
    while left >= 16 or left == 8:
        recs.append(rand_T(rng, 7))
        left -= 8
    if left > 8:        # 10, 12, 14: an 8-byte T and the rest
        recs.append(rand_T(rng, 7))
        left -= 8
    if left:            # 2, 4, 6
        recs.append(rand_T(rng, left - 1))
    return recs


@lru_cache(maxsize=None)
def filled(nbytes: int, style: str, seed=0) -> Built:
    b = built(fill(nbytes, style, seed))
    assert len(b.packed) == nbytes
    return b


def fill_words(nwords: int, style: str, seed=0):
    """Records totalling exactly nwords words that stay inside one window of
    either decoder (about 1000 records and 2 KiB at the most): whole Z(255) records
    first, then the style's records (sparse: Z(2), T; mid: T)."""
    rng = _rng("fill_words", nwords, style, seed)
    per = 1000
    nz = max(0, -(-(nwords - per) // 256))
    recs = [Z(255)] * nz
    left = nwords - 256 * nz
    assert left >= 0
    if style == "sparse":
        z2 = Z(2)
        for t in rand_Ts(rng, 1, left // 4):
            recs += [z2, t]
        left %= 4
    return recs + rand_Ts(rng, 1, left)


# ---- probes ----------------------------------------------------------------
PROBES = ("Z0", "Z1", "Z255", "T1", "T7", "F0", "F1", "F29", "F30", "F255")
WORD_PROBES = ("Z0", "Z1", "Z2", "Z3", "Z4", "Z255", "F0", "F3", "F255", "T3")


@lru_cache(maxsize=None)
def probe(kind: str, seed=0) -> Built:
    rng = _rng("probe", kind, seed)
    n = int(kind[1:])
    r = Z(n) if kind[0] == "Z" else rand_T(rng, n) if kind[0] == "T" else rand_F(rng, n)
    return built([r])


class Case:
    """(name, packed bytes, word count) and what the builder knows of it:
    words (None for a malformed case), canonical, expect (the status name the
    builder predicts; the oracle's answer is the authority), tag (the probe's
    byte position), style; where the builder placed a probe with a tail behind
    it, word (the probe's first output word) and tail (the bytes behind it)."""
    __slots__ = ("name", "packed", "nwords", "words", "canonical", "expect", "tag", "kind", "style", "word", "tail")

    def __init__(self, name, b: Built, style, tag=None, kind=None, packed=None, nwords=None, expect="OK",
                 word=None, tail=None):
        self.name, self.style, self.tag, self.kind, self.expect = name, style, tag, kind, expect
        self.word, self.tail = word, tail
        self.packed = b.packed if packed is None else packed
        self.nwords = b.nwords if nwords is None else nwords
        valid = expect == "OK"
        self.words = b.words if valid else None
        self.canonical = b.canonical if valid else False


TAILS = (0, 40, kDecChkReach - 8, 2 * kWin)


def first_window_seams(style: str):
    """Packed-byte seams of the first window: each probe kind's tag at every
    byte of [S - kDecChunk - 4, S + 18] for S = 3072 and 3584 (and 2 * kD2NI,
    the record-cap cut, for the two-byte styles), then a tail of 0, 40,
    kDecChkReach - 8 or 2 * kWin bytes, cycling."""
    seams = [kD2Win, kWin] + ([2 * kD2NI] if style in ("mid", "z0pair") else [])
    cases, n = [], 0
    for S in seams:
        for kind in PROBES:
            for p in range(S - kDecChunk - 4, S + 19):
                tail = TAILS[n % 4]
                n += 1
                b = filled(p, style) + probe(kind) + filled(tail, style, 1)
                cases.append(Case(f"win{S}/{kind}/tag@{p - S:+d}/{style}/tail{tail}", b, style, tag=p, kind=kind,
                                  word=filled(p, style).nwords, tail=tail))
    return cases


def _place_at_window_edge(style, w, off, kind, win, tail_bytes):
    """A piece whose probe's tag lies off bytes past the end of window w
    (windows by the placement rule; their starts are unaligned)."""
    base = fill((w + 1) * win + 700, style, seed=w)
    _, _, idx = build(base)
    ew = window_starts(idx, 1 << 30, win)[w]
    target = ew + win + off
    keep = [r for r, (p, _, _) in zip(base, idx) if p + len(r.packed) <= target - 150]
    head = built(keep)
    gap = target - len(head.packed)
    head = head + filled(gap, style, 2)
    b = head + probe(kind) + filled(tail_bytes, style, 3)
    return b, target, head.nwords


def later_window_seams():
    """Dense pieces of at least four windows, the probe at the end of window
    1 and 2 (the windows the dense form may walk serially; window 0 is always
    parallel), tag offsets -2..+2."""
    cases = []
    for w in (1, 2):
        for kind in PROBES:
            for off in range(-2, 3):
                tail = 2 * kWin + 300
                b, tag, word = _place_at_window_edge("dense", w, off, kind, kWin, tail)
                cases.append(Case(f"winedge{w}|{w + 1}/{kind}/tag@{off:+d}/dense", b, "dense", tag=tag, kind=kind,
                                  word=word, tail=tail))
    return cases


def wave_wrap_seams():
    """Pieces of 18 windows, the probe at the edge between windows 15|16 and
    16|17: where decode_mw.hip's kMwWaves waves wrap."""
    cases = []
    for w in (kMwWaves - 1, kMwWaves):
        for kind in PROBES:
            for off in range(-2, 3):
                tail = (kMwWaves + 1 - w) * kWin + 300
                b, tag, word = _place_at_window_edge("dense", w, off, kind, kWin, tail)
                cases.append(Case(f"wrap{w}|{w + 1}/{kind}/tag@{off:+d}/dense", b, "dense", tag=tag, kind=kind,
                                  word=word, tail=tail))
    return cases


WORD_SEAMS = sorted({kRound, 2 * kRound, kD2Round, 2 * kD2Round})
WORD_OFFS = tuple(range(8, -2, -1))  # the probe's first word at R - d


def output_word_seams(style: str):
    """Inside one window: the probe's first word at R - d, d in 8..-1, for
    the rounds of both decoders and their second round edge (every phase of
    the kBlk-word block)."""
    cases = []
    for R in WORD_SEAMS:
        for kind in WORD_PROBES:
            for d in WORD_OFFS:
                head = built(fill_words(R - d, style))
                assert len(head.packed) < 2100 and head.nrec < kD2NI - 8 and head.nwords == R - d
                b = head + probe(kind) + filled(40, style, 1)
                cases.append(Case(f"round{R}/{kind}/word@{-d:+d}/{style}", b, style, tag=len(head.packed), kind=kind,
                                  word=R - d, tail=40))
    return cases


def many_round_pieces():
    """One window that expands through hundreds of rounds: kWin / 2 records
    Z(255) (458,752 words from 3,584 bytes), and the same with a T after
    every seventh."""
    n = kWin // 2
    rng = _rng("many")
    mixed = []
    for i in range(n):
        mixed.append(Z(255))
        if i % 7 == 6:
            mixed.append(rand_T(rng, 3))
    return [Case(f"rounds/Z255x{n}/sparse", built([Z(255)] * n), "sparse"),
            Case(f"rounds/Z255x{n}+T/sparse", built(mixed), "sparse")]


def record_count_edges():
    """mid: a window of exactly kD2NI - 1, kD2NI, kD2NI + 1 two-byte records
    before a Z(255) / F(255) probe (the record index's cap).  dense: after a
    first window, a window of exactly kDecSerMax - 1, kDecSerMax, kDecSerMax
    + 1 records -- F(2) records and a last F(255) that reaches past the
    window -- which the serial walk keeps (<= kDecSerMax) or gives back."""
    mid, dense = [], []
    for n in (kD2NI - 1, kD2NI, kD2NI + 1):
        for kind in ("Z255", "F255"):
            rng = _rng("cnt", n, kind)
            b = built(rand_Ts(rng, 1, n)) + probe(kind) + filled(40, "mid", 1)
            mid.append(Case(f"reccap{kD2NI}/{kind}/records{n}/mid", b, "mid", tag=2 * n, kind=kind))
    base = fill(kWin + 700, "dense", seed=9)
    _, _, idx = build(base)
    e1 = window_starts(idx, 1 << 30, kWin)[1]
    head = built([r for r, (p, _, _) in zip(base, idx) if p < e1])
    assert len(head.packed) == e1
    for n in (kDecSerMax - 1, kDecSerMax, kDecSerMax + 1):
        for rep in range(4):  # (several per count: the counters add up over a batch)
            rng = _rng("ser", n, rep)
            assert 26 * (n - 1) < kWin < 26 * (n - 1) + LONGEST
            body = built([rand_F(rng, 2) for _ in range(n - 1)] + [rand_F(rng, 255)])
            b = head + body + filled(2 * kWin + 300, "dense", 4 + rep)
            dense.append(Case(f"sermax{kDecSerMax}/F2/records{n}/dense/{rep}", b, "dense", tag=e1, kind="F2"))
    return mid, dense


def noncanonical_streams():
    """Well-formed bytes the encoder never writes (PackedInputStream.read
    accepts any sequence of records): back-to-back Z(0) and F(0), Z(k) right
    after Z(255), all-zero literal words, T then Z(0), and 200 random record
    sequences of 1..6000 records."""
    cases = []
    rng = _rng("nc")
    for n in (2, 3, kD2NI, kWin // 2, kWin // 2 + 1, 4000):
        cases.append(Case(f"noncanon/Z0x{n}", built([Z(0)] * n), "mid"))
    for n in (2, 3, kWin // 10, kWin // 10 + 1, 800):
        cases.append(Case(f"noncanon/F0x{n}", built([rand_F(rng, 0) for _ in range(n)]), "dense"))
    for k in (0, 1, 2, 254, 255):
        cases.append(Case(f"noncanon/Z255,Z{k}", built([rand_T(rng, 1), Z(255), Z(k), rand_T(rng, 2)]), "sparse"))
        cases.append(Case(f"noncanon/Z{k},Z{k}x300", built([Z(k), Z(k)] * 300), "sparse"))
    for k in (1, 3, 29, 30, 255):
        cases.append(Case(f"noncanon/F{k}zero", built([rand_F(rng, k, True), rand_T(rng, 1)] * 5), "dense"))
    for n in (1, 7, 896, 897, 2000):
        cases.append(Case(f"noncanon/T,Z0x{n}", built([x for _ in range(n) for x in (rand_T(rng, 1), Z(0))]), "mid"))
    zs = {k: Z(k) for k in (0, 1, 2, 3, 29, 30, 64, 255)}

    def counts(n):  # mostly short runs; the long ones rare, so the corpus stays small
        u = rng.random(n)
        k = np.array([0, 0, 0, 0, 1, 1, 2, 3])[rng.integers(8, size=n)]
        k = np.where(u < 0.012, np.array([29, 30, 64])[rng.integers(3, size=n)], k)
        return np.where(u < 0.004, 255, k)
    for i in range(200):
        n = int(rng.integers(1, 6001)) if i % 4 else int(rng.integers(1, 40))
        kinds, ks, us = rng.integers(0, 3, size=n), counts(n), rng.random(n)
        tn, pi = rng.integers(1, 8, size=n), rng.integers(kPool, size=n)
        recs = [zs[k] if kd == 0 else _pool(f"T{t}")[p] if kd == 1 else _pool(f"F{k}", u < 0.1)[p]
                for kd, k, u, t, p in zip(kinds.tolist(), ks.tolist(), us.tolist(), tn.tolist(), pi.tolist())]
        cases.append(Case(f"noncanon/random{i}/records{n}", built(recs), "mid"))
    return cases


END_OFFS = tuple(range(-17, 18))


def end_of_piece_edges(style: str):
    """Pieces whose length P puts window 1 on either side of the check reach:
    P - e1 = kDecChkReach + d, d in -17..17, e1 the start of window 1 (the
    last window but one whenever the last record's tag lies past it), the
    last record of each probe kind.  Each also cut short by one byte, and
    with one word fewer and one more than it holds.  -> (valid, malformed)."""
    base = fill(kWin + 700, style, seed=5)
    _, _, idx = build(base)
    e1 = window_starts(idx, 1 << 30, kWin)[1]
    head = built([r for r, (p, _, _) in zip(base, idx) if p < e1])
    assert len(head.packed) == e1
    good, bad = [], []
    for kind in PROBES:
        pr = probe(kind, 1)
        for d in END_OFFS:
            P = e1 + kDecChkReach + d
            b = head + filled(P - e1 - len(pr.packed), style, 6) + pr
            assert len(b.packed) == P
            name = f"end/{kind}/reach{d:+d}/{style}"
            tag = P - len(pr.packed)
            good.append(Case(name, b, style, tag=tag, kind=kind))
            bad.append(Case(name + "/cut1", b, style, tag, kind, packed=b.packed[:-1], expect="ETRUNC"))
            one = kind in ("Z0", "T1", "T7", "F0")  # a one-word last record is left unread
            bad.append(Case(name + "/words-1", b, style, tag, kind, nwords=b.nwords - 1,
                            expect="ETRAILING" if one else "EOVERRUN"))
            bad.append(Case(name + "/words+1", b, style, tag, kind, nwords=b.nwords + 1, expect="ETRUNC"))
    return good, bad


def first_window_cuts(cases):
    """Every first-window S = kWin case with tag offset -2..+2, cut after
    the tag, before the count byte, in the middle of the literals and one
    byte before its end (the word count stays the whole piece's)."""
    out = []
    for c in first_window_edge_cases(cases):
        k = int(c.kind[1:])
        cuts = {"tag": c.tag + 1, "end-1": len(c.packed) - 1}
        if c.kind[0] == "F":
            cuts["count"] = c.tag + 9
            if k:
                cuts["lits"] = c.tag + 10 + 4 * k
        assert all(c.tag < v < len(c.packed) for v in cuts.values())
        for what, at in sorted(set(cuts.items()), key=lambda kv: kv[1]):
            out.append(Case(f"{c.name}/cut@{what}", Built(c.packed, c.words), c.style, c.tag, c.kind,
                            packed=c.packed[:at], expect="ETRUNC"))
    return out


FULL_VARIANTS = ("full@probe", "full+1", "full@end-1", "full@end")


def full_variants(c: Case):
    """The word counts at which the piece of valid case c is full at or
    inside its probe (first word o, nw words, t bytes behind it), while its
    packed bytes go on: [(variant, nwords, expect)].

      full@probe  o           the record before the probe fills the piece
      full+1      o + 1       the probe's run overruns after its first word
      full@end-1  o + nw - 1  ... one word before its end
      full@end    o + nw      the probe fills the piece, the tail is left
    """
    o, nw, t = c.word, probe(c.kind).nwords, c.tail
    out = []
    if o > 0:
        out.append(("full@probe", o, "ETRAILING"))
    if nw > 1:
        out.append(("full+1", o + 1, "EOVERRUN"))
    if nw > 2:
        out.append(("full@end-1", o + nw - 1, "EOVERRUN"))
    if t > 0:
        out.append(("full@end", o + nw, "ETRAILING"))
    return out


def full_before_the_end(cases):
    """Every variant of full_variants for each valid case: the case's bytes,
    only the word count changed, so the piece is full with its tail (and, but
    for full@end, the rest of the probe) unread.  With a tail of two bytes or
    more also as /tailcut: the last packed byte dropped, so the bytes end
    inside a record windows behind the full point.  The reference stops at
    the full point: the status stays what it was."""
    out = []
    for c in cases:
        assert c.expect == "OK" and c.word is not None and c.tail is not None and c.kind in PROBES + WORD_PROBES
        b = Built(c.packed, c.words)
        for v, nwords, expect in full_variants(c):
            assert 0 < nwords < c.nwords
            out.append(Case(f"{c.name}/{v}", b, c.style, c.tag, c.kind, nwords=nwords, expect=expect,
                            word=c.word, tail=c.tail))
            if c.tail >= 2:
                out.append(Case(f"{c.name}/{v}/tailcut", b, c.style, c.tag, c.kind, packed=c.packed[:-1],
                                nwords=nwords, expect=expect, word=c.word, tail=c.tail - 1))
    return out


FULL_LONG_TAIL = 2 * kWin
FULL_LONG_KINDS = ("Z255", "F255")


def output_word_seams_long_tail(style: str):
    """output_word_seams' pieces for the probe at word R exactly, with two
    windows of bytes behind the probe instead of 40 bytes (valid cases, used
    only as sources of full_before_the_end: a full point on a round edge
    whose tail ends windows later)."""
    cases = []
    for R in WORD_SEAMS:
        for kind in FULL_LONG_KINDS:
            head = built(fill_words(R, style))
            b = head + probe(kind) + filled(FULL_LONG_TAIL, style, 1)
            cases.append(Case(f"round{R}/{kind}/word@+0/{style}/tail{FULL_LONG_TAIL}", b, style,
                              tag=len(head.packed), kind=kind, word=R, tail=FULL_LONG_TAIL))
    return cases


def first_window_edge_cases(cases):
    """The first-window S = kWin cases with tag offset -2..+2 (what
    first_window_cuts cuts)."""
    return [c for c in cases if c.name.startswith(f"win{kWin}/") and -2 <= c.tag - kWin <= 2]


FULL_WRAP_KINDS = ("Z255", "F255", "F1", "T1")
# source corpora of each full/* corpus (full_sources picks from them)
FULL_SOURCES = {"full/words-sparse": ("words/sparse",), "full/words-mid": ("words/mid",),
                "full/first": tuple(f"first/{s}" for s in STYLES), "full/later": ("later/dense",),
                "full/wrap": ("wrap/dense",)}


def full_sources(c: dict, name: str):
    """The valid cases a full/* corpus is derived from."""
    src = [x for s in FULL_SOURCES[name] for x in c[s]]
    if name.startswith("full/words-"):
        return src + output_word_seams_long_tail(name.split("-")[1])
    if name == "full/first":
        return first_window_edge_cases(src)
    if name == "full/wrap":
        return [x for x in src if "/tag@+0/" in x.name and x.kind in FULL_WRAP_KINDS]
    return src


# ---- batches and streams -----------------------------------------------------
def filler_piece(nbytes: int, serial) -> Case:
    return Case(f"filler{serial}/{nbytes}", filled(nbytes, "mid", 7), "mid")


def batch_with_all_phases(cases):
    """The cases in order as one batch.  Where a piece would start at an
    in_off % 16 that an earlier piece already had, while some value is
    still missing, an odd filler piece (3..15 bytes) is put in front of it
    that moves it to a missing one (the window load's padw depends on
    in_off % 16).  -> list of cases."""
    out, pos, seen = [], 0, set()
    for c in cases:
        if pos % 16 in seen and len(seen) < 16:
            nb = next((nb for nb in range(3, 16, 2) if (pos + nb) % 16 not in seen), 0)
            if nb:
                out.append(filler_piece(nb, len(out)))
                pos += nb
        seen.add(pos % 16)
        out.append(c)
        pos += len(c.packed)
    return out


def in_off_phases(cases):
    """The in_off % 16 of the batch's pieces, fillers not counted."""
    pos, seen = 0, set()
    for c in cases:
        if not c.name.startswith("filler"):
            seen.add(pos % 16)
        pos += len(c.packed)
    return seen


STREAM_RESIDUES = tuple(r % kSsBlock for r in range(kSsBlock - 12, kSsBlock + 3))


def stream_coverage(cases, shift=0):
    """-> ({probe kind: residues of its tag mod kSsBlock}, F255 probes whose
    tag lies in the last block of a kSsGroup-block group)."""
    res, last, pos = {}, 0, shift
    for c in cases:
        if c.tag is not None and c.kind in PROBES:
            t = pos + c.tag
            res.setdefault(c.kind, set()).add(t % kSsBlock)
            if c.kind == "F255" and (t // kSsBlock) % kSsGroup == kSsGroup - 1:
                last += 1
        pos += len(c.packed)
    return res, last


def stream_covers(cases, shift=0):
    res, last = stream_coverage(cases, shift)
    return last > 0 and all(set(STREAM_RESIDUES) <= res.get(k, set()) for k in PROBES)


def stream_of(cases):
    """The valid cases as pieces of one stream, its head shifted by filler
    pieces until each probe kind's tag position mod kSsBlock covers
    [kSsBlock - 12, kSsBlock + 2] and an F255 probe starts in the last block
    of a group.  -> list of cases (fillers first)."""
    for shift in [0] + list(range(2, 4 * kSsBlock * kSsGroup, 251)):
        if stream_covers(cases, shift):
            head, left = [], shift
            while left:
                nb = left if left <= 60003 else 60000  # (never leaves a last filler under 2 bytes)
                head.append(filler_piece(nb, f"-head{len(head)}"))
                left -= nb
            return head + list(cases)
    raise AssertionError("no head shift gives the stream its block-edge coverage")


@lru_cache(maxsize=None)
def corpora() -> dict:
    """Every corpus, built once: {name: [Case]}."""
    c = {}
    for style in STYLES:
        c[f"first/{style}"] = batch_with_all_phases(first_window_seams(style))
    c["later/dense"] = later_window_seams()
    c["wrap/dense"] = wave_wrap_seams()
    for style in ("sparse", "mid"):
        c[f"words/{style}"] = output_word_seams(style)
    c["rounds/sparse"] = many_round_pieces()
    c["count/mid"], c["count/dense"] = record_count_edges()
    c["noncanon"] = noncanonical_streams()
    for style in ("dense", "mid"):
        c[f"end/{style}"], c[f"endbad/{style}"] = end_of_piece_edges(style)
    c["cuts"] = first_window_cuts([x for s in STYLES for x in c[f"first/{s}"]])
    for name in FULL_SOURCES:
        c[name] = full_before_the_end(full_sources(c, name))
    return c


def release():
    """Drop the built corpora (several hundred MiB of bytes); the test
    modules call it when they are done."""
    corpora.cache_clear()
    filled.cache_clear()


VALID = ("first/sparse", "first/mid", "first/dense", "first/z0pair", "later/dense", "wrap/dense", "words/sparse",
         "words/mid", "rounds/sparse", "count/mid", "count/dense", "noncanon", "end/dense", "end/mid")
MALFORMED = ("endbad/dense", "endbad/mid", "cuts") + tuple(FULL_SOURCES)
# what dec_gate_kernel does with each batch when the decoder is not forced
GATE = {"first/sparse": "index", "words/sparse": "index", "rounds/sparse": "index",
        "first/mid": "map", "first/z0pair": "map", "count/mid": "map", "end/mid": "map",
        "first/dense": "dense", "later/dense": "dense", "wrap/dense": "dense", "count/dense": "dense",
        "end/dense": "dense"}


def gate_of(cases) -> str:
    """dec_gate_kernel's choice (decode_v2.hip) for the cases as one batch."""
    P = sum(len(c.packed) for c in cases)
    U = 8 * sum(c.nwords for c in cases)
    return "index" if 100 * P < 15 * U else "dense" if 100 * P >= 80 * U else "map"


def batch_arrays(cases):
    """-> (packed uint8 array, in_off uint64[n+1], seg_word_off uint64[n+1])."""
    packed = np.frombuffer(b"".join(c.packed for c in cases), np.uint8)
    in_off = np.concatenate([[0], np.cumsum([len(c.packed) for c in cases], dtype=np.uint64)]).astype(np.uint64)
    swo = np.concatenate([[0], np.cumsum([c.nwords for c in cases], dtype=np.uint64)]).astype(np.uint64)
    return packed, in_off, swo
