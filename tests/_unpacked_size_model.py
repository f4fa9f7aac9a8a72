"""The contract of cpk_unpacked_size_batch as a record walk over bytes (no GPU,
no library; tests/test_unpacked_size_model.py pins it against the oracle): a
packed range is CPK_OK with the words of its records when it ends exactly at
a record's end, CPK_ETRUNC with 0 words when it ends inside one
(PackedInputStream.java:82-134)."""
from _packed_records import CSRC, F, Z, _rng, parse_constant, rand_F, rand_T

OK, ETRUNC = 0, -2
kUsChunk = parse_constant((CSRC / "decode_size.hip").read_text(), "kUsChunk", {})
kUsWin = 64 * kUsChunk


def record_at(b: bytes, q: int):
    """The record whose tag is b[q] -> (its byte length, its words), either
    None while the count byte that decides it lies past the end of b."""
    tag = b[q]
    if tag == 0:
        return (2, 1 + b[q + 1]) if q + 1 < len(b) else (2, None)
    if tag == 255:
        return (10 + 8 * b[q + 9], 1 + b[q + 9]) if q + 9 < len(b) else (None, None)
    return 1 + bin(tag).count("1"), 1


def walk(b: bytes):
    """-> (bytes of the complete records, their words, the cut record or None)."""
    q = w = 0
    while q < len(b):
        ln, nw = record_at(b, q)
        if ln is None or q + ln > len(b):
            return q, w, (ln, nw)
        q, w = q + ln, w + nw
    return q, w, None


def unpacked_size(b: bytes):
    """-> (status, words) of the packed range b."""
    _, w, cut = walk(b)
    return (OK, w) if cut is None else (ETRUNC, 0)


def hand_built():
    """Three pieces with Z, T and F records -- two of about 300 bytes, the
    third with an F(255), 2,070 bytes; every prefix of each is a case."""
    rng = _rng("usize-hand")
    lits = bytes(range(1, 9))
    a = [Z(0), rand_T(rng, 1), Z(255), rand_T(rng, 7), rand_F(rng, 0), Z(3), rand_F(rng, 29), rand_T(rng, 3), Z(1),
         rand_T(rng, 2)]
    b = [rand_F(rng, 1), rand_F(rng, 30), Z(0), Z(0), rand_T(rng, 4), F(2, lits, bytes(16)), rand_T(rng, 6), Z(64)]
    c = [rand_T(rng, 5), rand_F(rng, 255), Z(7), rand_T(rng, 1)]
    return [b"".join(r.packed for r in p) for p in (a, b, c)]


def prefixes(piece: bytes):
    return [piece[:k] for k in range(len(piece) + 1)]
