"""Decoder confinement: whatever a piece's status, the batch and stream
decoders write no word outside [d_seg_word_off[0], d_seg_word_off[n]), no
entry outside d_status[0..n) / d_in_off[0..n], and nothing into a piece whose
packed range is empty (include/capnp_packed.h at cpk_decode_batch and
cpk_decode_stream).

Every corpus of tests/_packed_records.py, malformed ones included, goes through
cpk_decode_batch with a guard piece behind every case: an empty packed range
and G words, which the reference fails with ETRUNC and for which no word may be
written.  in_off does not move at a guard, so every case keeps its load phase;
the output starts at word 3, so pieces start off the 16- and 32-byte grids.
The output, the statuses and the boundaries are filled with sentinels that no
builder writes, and every sentinel outside what the call may write is checked.
A stray word from a failed piece's zero run or literal run lands in the guard
behind it, where no other wave writes.
"""
import numpy as np
import pytest

import _packed_records as R
import test_gpu_decoder_seams as S

pytestmark = pytest.mark.gpu

LEAD, GUARD = 3, 8
SENT, ST_SENT = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A
G = 2 * R.kBlk + 1  # a guard piece's words: two expansion blocks and a word
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    S._cache.clear()  # (the streams built through S._stream)
    R.release()


def _sentinels(n, dtype=np.uint64):
    return np.full(n, SENT if dtype == np.uint64 else ST_SENT, dtype)


def _dev(a):
    import torch
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def _dev_packed(packed):
    """The packed bytes on the device, zeros behind them over the 16-byte
    lines the decoders may read, and a copy to compare with afterwards."""
    buf = np.zeros((len(packed) + 64 + 15) // 16 * 16, np.uint8)
    buf[:len(packed)] = packed
    d = _dev(buf)
    return d, d.clone()


def _guard_piece(g):
    return R.Case(f"guard{g}", R.Built(), "mid", packed=b"", nwords=g, expect="ETRUNC")


def _guarded(oracle, name):
    """A corpus with a guard piece after every case, as batch arrays whose
    first word offset is LEAD, and the oracle's answer; once per corpus."""
    if name not in _cache:
        cases = R.corpora()[name]
        g = G
        if name in R.GATE and R.gate_of([x for c in cases for x in (c, _guard_piece(g))]) != R.GATE[name]:
            g = R.kBlk + 1
        guard = _guard_piece(g)
        batch = [x for c in cases for x in (c, guard)]
        packed, in_off, swo = R.batch_arrays(batch)
        swo = swo + np.uint64(LEAD)
        want, ost = oracle.unpack_batch(packed, in_off, swo, threads=8)
        _cache[name] = (batch, packed, in_off, swo, want.view(np.uint64), ost)
    return _cache[name]


def _names(bad):
    return len(bad), bad[:8]


def _check_words(batch, swo, got, want, ost):
    """got / want: uint64 words from word 0 of the output.  The words of
    every piece the oracle accepts are the oracle's; every word of a piece
    with an empty packed range and every word outside [swo[0], swo[n]) is
    still the sentinel."""
    n = len(batch)
    total = int(swo[-1])
    counts = np.diff(swo.astype(np.int64))
    piece = np.repeat(np.arange(n), counts)  # piece of output word LEAD + i
    body, ref = got[LEAD:total], want[LEAD:total]
    assert not (ref == SENT).any(), "the sentinel is a word of the corpus"
    ok = (ost == 0)[piece]
    wrong = np.unique(piece[ok & (body != ref)])
    assert wrong.size == 0, _names([batch[i].name for i in wrong])
    empty = np.array([len(c.packed) == 0 for c in batch])[piece]
    hit = np.nonzero(empty & (body != SENT))[0]
    if hit.size:
        first = {}
        for i in hit:
            first.setdefault(int(piece[i]), int(i))
        bad = [f"after {batch[p - 1].name}: guard word {i + LEAD - int(swo[p])} (output word {i + LEAD}) = "
               f"{int(body[i]):#018x}" for p, i in list(first.items())[:8]]
        raise AssertionError(f"{len(first)} guard pieces written: {bad}")
    for what, part, at in (("lead", got[:LEAD], 0), ("trailing", got[total:], total)):
        hit = np.nonzero(part != SENT)[0]
        assert hit.size == 0, [f"{what} word {at + int(i)} = {int(part[i]):#018x}" for i in hit[:8]]
    assert got.size == total + GUARD


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_batch_decode_is_confined(ctx, oracle, name):
    """One cpk_decode_batch per corpus with guards: statuses and accepted
    words are the oracle's, the guards, the lead and trailing words and the
    status sentinels are untouched, the packed bytes unchanged; and the guards
    leave the batch with the decoder form its corpus is meant for."""
    import torch
    batch, packed, in_off, swo, want, ost = _guarded(oracle, name)
    n = len(batch)
    if name in R.GATE:
        assert R.gate_of(batch) == R.GATE[name]
    # (never the few-large-pieces stream path of cpk_decode_batch: at most 32 pieces of 1 Mi words on average)
    assert n > 32 or int(swo[-1] - swo[0]) < n << 20
    guards = np.arange(n) % 2 == 1
    assert (ost[guards] == -2).all() and all(len(c.packed) == 0 for c in batch[1::2])
    d_pk, before = _dev_packed(packed)
    d_off, d_swo = _dev(in_off), _dev(swo)
    d_out = _dev(_sentinels(int(swo[-1]) + GUARD))
    d_st = _dev(_sentinels(n + GUARD, np.uint32))
    ctx.decode_batch(d_pk, d_off, d_swo, d_out, d_st[:n])
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    assert (st[n:] == ST_SENT).all(), "written past d_status[n - 1]"
    bad = [f"{c.name}: status {R.STATUS.get(int(s), int(s))}, expected {R.STATUS[int(o)]}"
           for c, s, o in zip(batch, st[:n], ost) if s != o]
    assert not bad, _names(bad)
    _check_words(batch, swo, d_out.cpu().numpy().view(np.uint64), want, ost)
    assert torch.equal(d_pk, before), "the packed bytes were written"
    assert torch.equal(d_off, _dev(in_off)) and torch.equal(d_swo, _dev(swo))


HOST = R.MALFORMED + ("words/sparse", "later/dense", "first/mid")


@pytest.mark.parametrize("name", HOST)
def test_batch_decode_host_is_confined(ctx, oracle, name):
    """cpk_decode_host into a caller's buffer 64 bytes longer than
    8 * swo[n]: the extra bytes survive (guard pieces are not asserted here:
    the pipeline copies whole ranges back)."""
    packed, in_off, swo, want, ost = S._expected(oracle, name)
    size = 8 * int(swo[-1])
    buf = _sentinels(size // 8 + 8).view(np.uint8)
    src = packed.copy()
    got, st = ctx.decode_host(src, in_off, swo, out=buf)
    assert np.array_equal(src, packed), "the packed bytes were written"
    assert (buf[size:].view(np.uint64) == SENT).all(), "written past 8 * seg_word_off[n]"
    S._compare(R.corpora()[name], swo, got, st, want, ost)


# ---- stream forms ------------------------------------------------------------
def _device_stream(ctx, stream, swo):
    """One device cpk_decode_stream with sentinels around all three output
    arrays -> (words from swo[0] as bytes, boundaries, statuses)."""
    import torch
    n = len(swo) - 1
    lead = swo + np.uint64(LEAD)
    d_pk, before = _dev_packed(np.frombuffer(stream, np.uint8))
    d_swo = _dev(lead)
    d_out = _dev(_sentinels(int(lead[-1]) + GUARD))
    d_io = _dev(_sentinels(n + 1 + GUARD))
    d_st = _dev(_sentinels(n + GUARD, np.uint32))
    ctx.decode_stream(d_pk, len(stream), d_swo, d_out, d_io[:n + 1], d_st[:n])
    torch.cuda.synchronize()
    out, io, st = d_out.cpu().numpy().view(np.uint64), d_io.cpu().numpy().view(np.uint64), d_st.cpu().numpy()
    assert (out[:LEAD] == SENT).all(), "written before d_seg_word_off[0]"
    hit = np.nonzero(out[int(lead[-1]):] != SENT)[0]
    assert hit.size == 0, [f"word {int(lead[-1]) + int(i)} = {int(out[int(lead[-1]) + i]):#018x}" for i in hit[:8]]
    assert (io[n + 1:] == SENT).all(), "written past d_in_off[n]"
    assert (st[n:] == ST_SENT).all(), "written past d_status[n - 1]"
    assert torch.equal(d_pk, before), "the packed bytes were written"
    assert torch.equal(d_swo, _dev(lead))
    return out[LEAD:int(lead[-1])].view(np.uint8), io[:n + 1], st[:n]


@pytest.mark.parametrize("splice", [None, "first", "middle", "last"])
def test_stream_decode_is_confined(ctx, oracle, splice):
    """The seam tests' stream of first-window and non-canonical pieces, whole
    and with a failing piece spliced in first, in the middle and last,
    through device cpk_decode_stream and through cpk_decode_stream_host into
    a caller's buffer: the pieces before the failing one are exact, the
    boundaries and statuses are the oracle's, and nothing is written outside
    the ranges of the three output arrays."""
    stream, swo, cases, walk = S._stream(oracle, splice)
    assert (walk[0] != 0).any() == (splice is not None)
    got, bounds, st = _device_stream(ctx, stream, swo)
    S._compare_stream(cases, swo, got, bounds, st, walk)
    size = 8 * int(swo[-1])
    buf = _sentinels(size // 8 + 8).view(np.uint8)
    got, bounds, st = ctx.decode_stream_host(np.frombuffer(stream, np.uint8), swo, out=buf)
    assert (buf[size:].view(np.uint64) == SENT).all(), "written past 8 * seg_word_off[n]"
    S._compare_stream(cases, swo, got, bounds, st, walk)


@pytest.mark.parametrize("name", ["later/dense", "wrap/dense", "full/later", "full/wrap"])
def test_workgroup_reader_piece_full_early(ctx, oracle, name):
    """Each later-window and wave-wrap piece (100 each) as a device stream of
    its own with junk behind it, which the one-workgroup reader takes
    (decode_mw.hip), with one word fewer than it holds; and each of their
    full-before-the-end variants (uncut) with the variant's word count, which
    is full at the window edge itself, windows before the bytes end.  The
    window hand-over then meets a filled piece.  The status, the boundary
    and, where it accepts the piece, the words are the oracle's read of the
    same stream (a stream has no trailing bytes: a piece that is full at a
    record's end is read, and the next read starts there)."""
    from test_gpu_stream import _oracle_stream
    cases = [c for c in R.corpora()[name] if not c.name.endswith("/tailcut")]
    assert len(cases) == {"later/dense": 100, "wrap/dense": 100, "full/later": 300, "full/wrap": 26}[name]
    junk = bytes(np.random.default_rng(6).integers(0, 256, size=500, dtype=np.uint8))
    bad, seen = [], set()
    for c in cases:
        assert 6 * 1024 <= len(c.packed) < 384 * 1024
        stream = c.packed + junk
        swo = np.array([0, c.nwords - (c.expect == "OK")], np.uint64)
        ost, obounds, oout = _oracle_stream(oracle, stream, swo)
        seen.add(int(ost[0]))
        got, bounds, st = _device_stream(ctx, stream, swo)
        if st[0] != ost[0]:
            bad.append(f"{c.name}: status {R.STATUS.get(int(st[0]), int(st[0]))}, expected {R.STATUS[int(ost[0])]}")
        elif ost[0] == 0 and (int(bounds[0]), int(bounds[1])) != (0, obounds[1]):
            bad.append(f"{c.name}: ends at {int(bounds[1])}, expected {obounds[1]}")
        elif ost[0] == 0 and got.tobytes() != oout[0]:
            bad.append(f"{c.name}: words")
    assert not bad, _names(bad)
    assert 0 in seen  # (a one-word last record is left for the next read; a longer one overruns)
    if name.startswith("full/"):
        assert seen == {0, -3}
