"""Pins tests/_high_offsets.py (no GPU): every layout that
tests/test_gpu_high_offsets.py hands to the library really lies above or across
2^32 bytes, names the piece that holds the line and its remainder, and fits
into its arena with a guard window on either side -- so a layout can never
silently degrade to a low offset."""
import numpy as np
import pytest

import _high_offsets as H

LINE = H.LINE
WORD_BYTES, BYTE_BYTES = 8 * H.WORD_ARENA, H.BYTE_ARENA


def _holds_line(lay):
    """(piece, rem) of LINE by a search of the offsets, not by the layout's own word."""
    off = lay.off.astype(object) * lay.unit
    inside = [k for k in range(len(off) - 1) if off[k] < LINE < off[k + 1]]
    starts = [k for k in range(len(off) - 1) if off[k] == LINE and off[k + 1] > LINE]
    return inside, starts


def _check(lay, arena_bytes):
    lay.check()
    assert lay.fits(arena_bytes), (lay.where, lay.lo, lay.hi)
    inside, starts = _holds_line(lay)
    if lay.where.startswith("above"):
        assert not inside and int(lay.off[0]) * lay.unit >= LINE
    elif lay.where == "edge":
        assert not inside and starts and int(lay.off[lay.piece]) * lay.unit == LINE
        assert lay.lo < LINE < lay.hi
    else:
        assert inside == [lay.piece]
        assert (LINE - int(lay.off[lay.piece]) * lay.unit) == lay.rem * lay.unit
        assert lay.rem % (64 if lay.unit == 8 else 16) != 0
    assert lay.hi >= LINE  # never a low batch


def test_arenas():
    assert WORD_BYTES == LINE + (1 << 23) and BYTE_BYTES == LINE + (1 << 23)
    assert H.GUARD == 64 * 1024
    # the file's peak: both arenas (Part 3 frees them first and stays under 16 GiB by itself)
    words = sum(H.part3_sizes())
    assert 8 * words >= H.PART3_BYTES and 8 * words < H.PART3_BYTES + (1 << 20)
    assert 8 * words + 9 * words + 16 + 8 * words < 15 << 30
    assert 0.96 * 8 * words > LINE  # (config 3 packs to 0.967 of the words' bytes: d_out_off[n] passes the line)


@pytest.mark.parametrize("batch,where", H.WORD_CASES)
def test_word_layouts(oracle, batch, where):
    sizes, data = H.word_batch(oracle, batch)
    assert data.size == 8 * sum(sizes)
    lay = H.place_words(sizes, where)
    _check(lay, WORD_BYTES)
    assert np.array_equal(np.diff(lay.off.astype(np.int64)), np.asarray(sizes))
    if where == "above":
        assert int(lay.off[0]) == (LINE >> 3) + 129
    if where == "middle":
        assert lay.piece == len(sizes) // 2 and lay.rem == 4097
    if where == "straddle":
        assert sizes[lay.piece] == max(sizes[:-1]) and lay.piece < len(sizes) - 1
        assert int(lay.off[-2]) * 8 > LINE  # (a piece starts above the line too)


def test_word_batches_reach_their_encoders():
    """mixed stays under the single pass's gate (pieces under 4 Ki words, the
    largest over twice the smallest); the like-sized ones are one chunk each;
    big has a piece of over three chunks."""
    assert min(H.MIXED) < 4096 and max(H.MIXED) > 2 * 8192 and len(H.MIXED) == 14
    assert set(H.LIKE) == {8192} and len(H.LIKE) == 24
    assert max(H.BIG) == 3 * 8192 + 5 and H.BIG.index(max(H.BIG)) == 1
    assert {w for _, w in H.WORD_CASES} == set(H.LIKE_WHERE)
    assert ("like2", "middle") in H.WORD_CASES and ("like4", "middle") in H.WORD_CASES


@pytest.mark.parametrize("nmsg", H.MESSAGE_COUNTS)
@pytest.mark.parametrize("where", H.WORD_WHERE)
def test_message_layouts(nmsg, where):
    msgs = H.messages(nmsg)
    assert {len(m) for m in msgs} == {1, 2, 3, 9}
    sizes = [len(s) // 8 for m in msgs for s in m]
    assert set(sizes) <= set(H.MIXED)
    pieces = len(msgs) + len(sizes)
    assert (pieces > 1024) == (nmsg == 300)
    _check(H.place_words(sizes, where), WORD_BYTES)


@pytest.mark.parametrize("n", H.DECODE_N)
@pytest.mark.parametrize("density", list(H.DECODE_CFG))
def test_decode_layouts(oracle, density, n):
    pieces, sizes, words = H.decode_batch(oracle, density, n)
    assert len(pieces) == n and (n <= 32) == (n == 14)
    assert H.gate_of(pieces, sizes) == {"sparse": "index", "dense": "dense"}[density]
    # the truncated piece is refused by the oracle, its neighbours are not
    for i in (H.BAD - 1, H.BAD, H.BAD + 1):
        st, out, used = oracle.unpack(pieces[i], 8 * sizes[i])
        if i == H.BAD:
            assert st == oracle.ETRUNC and words[i] is None
        else:
            assert st == oracle.OK and used == len(pieces[i]) and out == words[i]
    import _packed_records as R
    assert max(len(p) for p in pieces) > 2 * R.kWin  # pieces of several windows
    assert {b for b, _ in H.DECODE_PLACEMENTS} == set(H.BYTE_WHERE) | {None}
    assert {w for _, w in H.DECODE_PLACEMENTS} == set(H.WORD_WHERE) | {None}
    assert all(b or w for b, w in H.DECODE_PLACEMENTS)
    for where in H.BYTE_WHERE:
        lay = H.place_bytes([len(p) for p in pieces], where)
        _check(lay, BYTE_BYTES)
        if where.startswith("above"):
            assert int(lay.off[0]) % 16 == int(where[5:]) % 16
    assert {int(w[5:]) for w in H.BYTE_WHERE if w.startswith("above")} == {0, 5, 15}
    for where in H.WORD_WHERE:
        _check(H.place_words(sizes, where), WORD_BYTES)


@pytest.mark.parametrize("name", list(H.STREAMS))
def test_stream_layouts(oracle, name):
    sizes, cfg = H.STREAMS[name]
    swo = H.rel_off(sizes)
    pk, _ = oracle.pack_batch(oracle.generate(oracle.preset(cfg), swo), swo)
    lo, hi = H.STREAM_BYTES[name]
    assert lo <= len(pk) < hi
    for where in H.WORD_WHERE:
        _check(H.place_words(sizes, where), WORD_BYTES)
        pos = H.stream_position(len(pk), where)
        assert pos % 16 == 0 and pos - H.GUARD >= 0 and pos + len(pk) + 16 + H.GUARD <= BYTE_BYTES
        if where == "above":
            assert pos >= LINE
        elif where == "edge":
            assert pos + len(pk) <= LINE < pos + len(pk) + 16
        else:
            assert pos < LINE < pos + len(pk)


def test_message_byte_layouts(oracle):
    msgs = H.messages(20)
    lens = [len(oracle.write_message(m)) for m in msgs]
    for where in H.BYTE_WHERE:
        _check(H.place_bytes(lens, where), BYTE_BYTES)


@pytest.mark.parametrize("where", H.AT_WHERE)
def test_placed_slots(where):
    # (any byte counts of the right order: the GPU test takes the oracle's)
    gb = [8 * sum(g) // 2 + 1 for g in H.AT_GROUPS]
    off, cap = H.at_slots(gb, where)
    assert {len(g) for g in H.AT_GROUPS} == {1, 2, 5}
    assert all(a > b for a, b in zip(off, off[1:])), "descending order"
    spans = sorted((o, o + c) for o, c in zip(off, cap))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "slots overlap"
    low = len(gb) - 1
    if where == "cross":
        assert off[low] < LINE < off[low] + gb[low] and cap[low] >= gb[low]
    else:
        assert off[low] + cap[low] == LINE and cap[low] == gb[low] and LINE in off
    assert all(o >= LINE for g, o in enumerate(off) if g != low)
    assert len({o % 16 for o in off}) >= 4, "arbitrary byte alignments"
    assert cap[H.AT_SHORT] == gb[H.AT_SHORT] - 1
    assert all(c >= b for g, (c, b) in enumerate(zip(cap, gb)) if g != H.AT_SHORT)
    assert min(off) - H.GUARD >= 0 and max(o + c for o, c in zip(off, cap)) + H.GUARD <= BYTE_BYTES


def test_part3_sample():
    sizes = H.part3_sizes()
    assert sizes[:6] == H.PART3_CYCLE
    # offsets as a dense batch would have them: 0.967 of the words' bytes
    off = np.concatenate([[0], np.cumsum([int(7.736 * s) for s in sizes])]).astype(np.uint64)
    assert int(off[-1]) > LINE
    k, pick = H.part3_sample(off)
    assert int(off[k]) <= LINE < int(off[k + 1])
    assert {k - 3, k - 2, k - 1, k, k + 1, k + 2, k + 3, 0, len(sizes) - 1} <= set(pick)
    assert len(pick) >= 35 and pick == sorted(set(pick))
