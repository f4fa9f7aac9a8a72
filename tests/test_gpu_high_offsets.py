"""Offsets above and across 4 GiB in every device entry point.

The library always gets the base pointer of an arena of a little over 4 GiB
(2^29 + 2^20 words, 2^32 + 2^23 bytes); only the offsets carry the position, so
a base truncated to 32 bits still lands inside the arena and shows as wrong
bytes against the oracle, not as a fault.  A case touches its batch and a 64 KiB
guard window on either side (all-ones on an input side, a sentinel on an output
side) and reads back no more than that; the layouts are those of
tests/_high_offsets.py, pinned on the CPU by tests/test_high_offsets_cases.py.
What is expected always comes from the oracle (oracle.pack, pack_batch,
unpack_batch, write_message, read_message, generate); Part 3's whole-array
checks are made against the size kernel and the device mismatch count as well
as an oracle sample.  Every test asserts before the call, on the arrays the
device holds, that its offsets lie above or across 2^32 bytes.

  Part 1  input words high: cpk_encode_batch, cpk_packed_size_batch,
          cpk_encode_messages, cpk_packed_size_messages, cpk_encode_batch_at
  Part 2  packed bytes and output words high: cpk_decode_batch,
          cpk_decode_stream, cpk_unpacked_size_batch, cpk_decode_messages,
          cpk_encode_batch_at's destinations
  Part 3  cpk_encode_batch whose own d_out_off passes 2^32 (about 4.6 GiB of
          dense words), decoded back
"""
import os
import time

import numpy as np
import pytest

import _high_offsets as H

pytestmark = pytest.mark.gpu

LINE = H.LINE
OK, ETRUNC, ENOMEM = 0, -2, -5
SENT = 0xA5                       # output bytes
SENT_W = -0x5A5A5A5A5A5A5A5B      # 0xA5A5A5A5A5A5A5A5 as int64: output words, offsets
ST_SENT = 0x5A5A5A5A
TAIL = 8                          # sentinel entries behind every small output array
PAD = 4096                        # sentinel bytes behind a low packed output
GW = H.GUARD // 8
PEAK_LIMIT = 16 << 30
ENV_KEYS = ("CPK_ENCODER", "CPK_DECODER", "CPK_SP_FORM", "CPK_SIZE_FORM", "CPK_USIZE_FORM", "CPK_AT_FORM",
            "CPK_E4_ORDER")


# ---- arenas ------------------------------------------------------------------------
def _alloc(n, dtype):
    import torch
    try:
        return torch.empty(n, dtype=dtype, device="cuda")
    except RuntimeError:  # (torch.cuda.OutOfMemoryError is one)
        free, total = torch.cuda.mem_get_info()
        size = n * torch.empty(0, dtype=dtype).element_size()
        pytest.skip(f"{size >> 20} MiB of device memory cannot be allocated: {free >> 20} of {total >> 20} MiB free")


class Arenas:
    """The word arena and the byte arena, allocated when first asked for and
    again after release() (Part 3 frees them for its own gigabytes)."""

    def __init__(self):
        self._words = self._bytes = None

    def words(self):
        import torch
        if self._words is None:
            self._words = _alloc(H.WORD_ARENA, torch.int64)
        return self._words

    def bytes(self):
        import torch
        if self._bytes is None:
            self._bytes = _alloc(H.BYTE_ARENA, torch.uint8)
        return self._bytes

    def release(self):
        import torch
        self._words = self._bytes = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arenas():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    a = Arenas()
    yield a
    a.release()
    del a
    torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_allocated()
    print(f"\nhigh offsets: peak device memory of the file {peak / 2**30:.2f} GiB")
    assert peak <= PEAK_LIMIT


def _make_ctx(**env):
    """A context created under `env` alone of ENV_KEYS (read at creation)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return cp.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _form_fixture(name, key, values):
    @pytest.fixture(scope="module", name=name, params=values, ids=[f"{key[4:].lower()}-{v or 'auto'}" for v in values])
    def fx(request):
        c = _make_ctx(**({key: request.param} if request.param else {}))
        yield c
        c.close()
    return fx


size_ctx = _form_fixture("size_ctx", "CPK_SIZE_FORM", ["chunk", "wave"])
at_ctx = _form_fixture("at_ctx", "CPK_AT_FORM", ["dense", "sparse"])
usize_wave_ctx = _form_fixture("usize_wave_ctx", "CPK_USIZE_FORM", [None, "2"])
usize_map_ctx = _form_fixture("usize_map_ctx", "CPK_USIZE_FORM", [None, "1"])


# ---- device helpers ---------------------------------------------------------------
def _dev64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64).copy()).cuda()


def _dev8(b):
    import torch
    a = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8)
    return torch.from_numpy(a.copy()).cuda()


def _full(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device="cuda")


def _low(rel, unit):
    """A batch at a low position in a buffer of its own, laid out like an
    arena's: a guard window below and above it."""
    import torch
    off = np.asarray(rel, dtype=np.uint64) + np.uint64(H.GUARD // unit)
    lay = H.Layout("low", unit, off, None, None)
    nbytes = (lay.hi + 15) // 16 * 16 + H.GUARD
    return lay, torch.empty(nbytes // unit, dtype=torch.int64 if unit == 8 else torch.uint8, device="cuda")


def _span(lay):
    """[a, b) in units of the layout: the batch, the line a reader may finish, the guards."""
    return (lay.lo - H.GUARD) // lay.unit, ((lay.hi + 15) // 16 * 16 + H.GUARD) // lay.unit


def _put(buf, lay, data):
    """An input side: all-ones guards, the data between them.  -> a copy of
    the window, to compare with afterwards (inputs are only read)."""
    a, b = _span(lay)
    buf[a:b] = -1 if lay.unit == 8 else 0xFF
    if lay.hi > lay.lo:
        d = _dev8(data)
        assert d.numel() == lay.hi - lay.lo
        buf[lay.lo // lay.unit:lay.hi // lay.unit] = d.view(buf.dtype)
    return buf[a:b].clone()


def _unchanged(buf, lay, before):
    import torch
    a, b = _span(lay)
    return bool(torch.equal(buf[a:b], before))


def _sentinels(buf, lay):
    a, b = _span(lay)
    buf[a:b] = SENT_W if lay.unit == 8 else SENT


def _window(buf, lay):
    """The window read back -> (guard below, body, guard above) as uint8."""
    a, b = _span(lay)
    w = buf[a:b].cpu().numpy().view(np.uint8)
    n = lay.hi - lay.lo
    return w[:H.GUARD], w[H.GUARD:H.GUARD + n], w[H.GUARD + n:]


def _pre(d_off, lay):
    """The precondition, on what the device holds: the offsets are the
    layout's and lie above / across LINE as its name says."""
    off = [int(x) * lay.unit for x in d_off.cpu().numpy().astype(np.uint64)]
    assert off == [int(x) * lay.unit for x in lay.off]
    if lay.where == "low":
        return
    if lay.where.startswith("above"):
        assert off[0] >= LINE
    elif lay.where == "edge":
        assert off[lay.piece] == LINE and off[0] < LINE < off[-1]
    else:
        assert off[lay.piece] < LINE < off[lay.piece + 1]
        assert (LINE - off[lay.piece]) % (512 if lay.unit == 8 else 16) != 0


def _guards_intact(below, above, what):
    for name, g in (("below", below), ("above", above)):
        hit = np.nonzero(g != SENT)[0]
        assert hit.size == 0, f"{what}: guard {name} the batch written at byte {int(hit[0])} of it ({hit.size} bytes)"


_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@pytest.fixture(scope="module", autouse=True)
def _release_memo():
    yield
    _memo.clear()
    import _packed_records as R
    R.release()


# ---- Part 1: input words above and across the line -------------------------------------
def _word_batch(oracle, name):
    def make():
        sizes, data = H.word_batch(oracle, name)
        want, woff = oracle.pack_batch(data, H.rel_off(sizes), threads=8)
        return sizes, data, want.tobytes(), np.asarray(woff, dtype=np.uint64)
    return _once(("words", name), make)


ENCODE_CASES = [(b, w, "exact") for b, w in H.WORD_CASES] + [("mixed", w, "hint-0") for w in H.WORD_WHERE]


@pytest.mark.parametrize("batch,where,hint", ENCODE_CASES, ids=["-".join(c) for c in ENCODE_CASES])
def test_encode_batch(ctx, oracle, arenas, batch, where, hint):
    """cpk_encode_batch through every encoder of the `ctx` fixture, the bound
    exact; mixed also without a bound (the two passes then pack their rows by
    word offset, counted from d_seg_word_off[0])."""
    import capnp_packed as cp
    sizes, data, want, woff = _word_batch(oracle, batch)
    n = len(sizes)
    lay = H.place_words(sizes, where)
    A = arenas.words()
    before = _put(A, lay, data)
    d_swo = _dev64(lay.off)
    cap = (cp.batch_capacity(lay.off) + 15) // 16 * 16
    d_pk = _full(cap + PAD, SENT, _u8())
    d_off = _full(n + 1 + TAIL, SENT_W, A.dtype)
    _pre(d_swo, lay)
    ctx.encode_batch(A, d_swo, max(sizes) if hint == "exact" else 0, d_pk, d_off)
    assert ctx.take_error() == cp.OK
    off = d_off.cpu().numpy()
    assert (off[n + 1:] == SENT_W).all(), "written past d_out_off[n]"
    assert np.array_equal(off[:n + 1].astype(np.uint64), woff), "piece offsets differ"
    got = d_pk.cpu().numpy()
    assert got[:len(want)].tobytes() == want, "packed bytes differ"
    assert (got[cap:] == SENT).all(), "bytes stored past the capacity"
    assert _unchanged(A, lay, before), "the input words or their guards were written"


def _u8():
    import torch
    return torch.uint8


@pytest.mark.parametrize("batch,where,hint", ENCODE_CASES, ids=["-".join(c) for c in ENCODE_CASES])
def test_packed_size_batch(size_ctx, oracle, arenas, batch, where, hint):
    """cpk_packed_size_batch in its chunk-parallel and its wave-per-piece form."""
    import capnp_packed as cp
    sizes, data, _, woff = _word_batch(oracle, batch)
    n = len(sizes)
    lay = H.place_words(sizes, where)
    A = arenas.words()
    before = _put(A, lay, data)
    d_swo = _dev64(lay.off)
    d_off = _full(n + 1 + TAIL, SENT_W, A.dtype)
    _pre(d_swo, lay)
    size_ctx.packed_size_batch(A, d_swo, max(sizes) if hint == "exact" else 0, d_off)
    assert size_ctx.take_error() == cp.OK
    off = d_off.cpu().numpy()
    assert (off[n + 1:] == SENT_W).all(), "written past d_out_off[n]"
    assert np.array_equal(off[:n + 1].astype(np.uint64), woff)
    assert _unchanged(A, lay, before), "the input words or their guards were written"


def _message_batch(oracle, nmsg):
    def make():
        msgs = H.messages(nmsg)
        want = b"".join(oracle.write_message(m) for m in msgs)
        woff = H.message_piece_offsets(oracle, msgs)
        assert int(woff[-1]) == len(want)
        return msgs, want, woff
    return _once(("messages", nmsg), make)


@pytest.mark.parametrize("where", H.WORD_WHERE)
@pytest.mark.parametrize("nmsg", H.MESSAGE_COUNTS)
def test_messages(ctx, oracle, arenas, nmsg, where):
    """cpk_packed_size_messages and cpk_encode_messages: the segment tables
    are built on the device from word offsets above LINE; 12 messages (the
    single pass with the tables' descriptors) and 300 (over 1,024 pieces: the
    two passes)."""
    import capnp_packed as cp
    msgs, want, woff = _message_batch(oracle, nmsg)
    segs = [s for m in msgs for s in m]
    sizes = [len(s) // 8 for s in segs]
    lay = H.place_words(sizes, where)
    A = arenas.words()
    before = _put(A, lay, b"".join(segs))
    d_swo = _dev64(lay.off)
    d_mseg = _dev64(H.rel_off([len(m) for m in msgs]))
    np_ = len(msgs) + len(segs)
    cap = cp.batch_capacity(lay.off) + sum(10 * ((len(m) + 2) // 2 + 1) for m in msgs)
    cap = (cap + 15) // 16 * 16
    _pre(d_swo, lay)
    d_soff = _full(np_ + 1 + TAIL, SENT_W, A.dtype)
    ctx.packed_size_messages(A, d_swo, d_mseg, max(sizes), d_soff)
    assert ctx.take_error() == cp.OK
    soff = d_soff.cpu().numpy()
    assert (soff[np_ + 1:] == SENT_W).all()
    assert np.array_equal(soff[:np_ + 1].astype(np.uint64), woff), "cpk_packed_size_messages"
    d_pk = _full(cap + PAD, SENT, _u8())
    d_off = _full(np_ + 1 + TAIL, SENT_W, A.dtype)
    ctx.encode_messages(A, d_swo, d_mseg, max(sizes), d_pk, d_off)
    assert ctx.take_error() == cp.OK
    off = d_off.cpu().numpy()
    assert (off[np_ + 1:] == SENT_W).all()
    assert np.array_equal(off[:np_ + 1].astype(np.uint64), woff), "cpk_encode_messages: piece offsets"
    got = d_pk.cpu().numpy()
    assert got[:len(want)].tobytes() == want
    assert (got[cap:] == SENT).all()
    assert _unchanged(A, lay, before), "the input words or their guards were written"


def _piece_packs(oracle, sizes, data):
    swo = H.rel_off(sizes).astype(np.int64)
    b = np.ascontiguousarray(data, np.uint8).tobytes()
    return [oracle.pack(b[8 * swo[i]:8 * swo[i + 1]]) for i in range(len(sizes))]


@pytest.mark.parametrize("batch,where", H.WORD_CASES, ids=["-".join(c) for c in H.WORD_CASES])
def test_encode_batch_at_low_destinations(at_ctx, oracle, arenas, batch, where):
    """cpk_encode_batch_at, dense and sparse form: the words high, every piece
    a group of its own in a low slot of a small buffer."""
    sizes, data, _, _ = _word_batch(oracle, batch)
    packs = _once(("packs", batch), lambda: _piece_packs(oracle, sizes, data))
    n = len(sizes)
    lay = H.place_words(sizes, where)
    A = arenas.words()
    before = _put(A, lay, data)
    d_swo = _dev64(lay.off)
    dst, cap, cur = [], [], 5
    for g, p in enumerate(packs):
        dst.append(cur)
        cap.append(len(p) + (g % 3) * 7)
        cur += cap[-1] + (5 * g + 3) % 16
    out_cap = cur + 3
    buf = _full(out_cap + PAD + 16, SENT, _u8())
    d_poff = _full(n + TAIL, SENT_W, A.dtype)
    d_glen = _full(n + TAIL, SENT_W, A.dtype)
    d_st = _full(n + TAIL, ST_SENT, _i32())
    _pre(d_swo, lay)
    at_ctx.encode_batch_at(A, d_swo, max(sizes), None, buf, out_cap, _dev64(dst), _dev64(cap), d_poff, d_glen, d_st,
                           ng=n)
    got, poff, glen, st = buf.cpu().numpy(), d_poff.cpu().numpy(), d_glen.cpu().numpy(), d_st.cpu().numpy()
    assert (poff[n:] == SENT_W).all() and (glen[n:] == SENT_W).all() and (st[n:] == ST_SENT).all()
    assert (st[:n] == OK).all(), st[:n]
    assert glen[:n].tolist() == [len(p) for p in packs]
    assert poff[:n].tolist() == dst
    want = np.full(got.size, SENT, np.uint8)
    for o, p in zip(dst, packs):
        want[o:o + len(p)] = np.frombuffer(p, np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} wrong bytes, the first at {bad[0]}"
    assert _unchanged(A, lay, before), "the input words or their guards were written"


def _i32():
    import torch
    return torch.int32


# ---- Part 2: packed bytes and output words above and across the line ---------------------
def _decode_batch(oracle, density, n):
    def make():
        pieces, sizes, words = H.decode_batch(oracle, density, n)
        packed = np.frombuffer(b"".join(pieces), np.uint8)
        _, ost = oracle.unpack_batch(packed, H.rel_off([len(p) for p in pieces]), H.rel_off(sizes), threads=8)
        assert ost[H.BAD] == ETRUNC and (np.delete(ost, H.BAD) == OK).all()
        return pieces, sizes, words, packed, ost
    return _once(("decode", density, n), make)


@pytest.mark.parametrize("place", H.DECODE_PLACEMENTS, ids=H.placement_id)
@pytest.mark.parametrize("n", H.DECODE_N)
@pytest.mark.parametrize("density", list(H.DECODE_CFG))
def test_decode_batch(ctx, oracle, arenas, density, n, place):
    """cpk_decode_batch through every decoder of the `ctx` fixture: a sparse
    and a dense batch, 14 pieces (the extent read-back path) and 40, one of
    them truncated; the packed bytes high, the words high, both."""
    pieces, sizes, words, packed, ost = _decode_batch(oracle, density, n)
    lens = [len(p) for p in pieces]
    if place[0]:
        blay, P = H.place_bytes(lens, place[0]), arenas.bytes()
    else:
        blay, P = _low(H.rel_off(lens), 1)
    if place[1]:
        wlay, W = H.place_words(sizes, place[1]), arenas.words()
    else:
        wlay, W = _low(H.rel_off(sizes), 8)
    before = _put(P, blay, packed)
    _sentinels(W, wlay)
    d_in_off, d_swo = _dev64(blay.off), _dev64(wlay.off)
    d_st = _full(n + TAIL, ST_SENT, _i32())
    _pre(d_in_off, blay)
    _pre(d_swo, wlay)
    ctx.decode_batch(P, d_in_off, d_swo, W, d_st[:n])
    st = d_st.cpu().numpy()
    assert (st[n:] == ST_SENT).all(), "written past d_status[n - 1]"
    assert st[:n].tolist() == ost.tolist()
    below, body, above = _window(W, wlay)
    _guards_intact(below, above, "output words")
    o = 0
    for i, w in enumerate(words):
        if w is not None:
            assert body[o:o + len(w)].tobytes() == w, f"piece {i} ({sizes[i]} words)"
        o += 8 * sizes[i]
    assert _unchanged(P, blay, before), "the packed bytes or their guards were written"


def _stream(oracle, name):
    def make():
        sizes, cfg = H.STREAMS[name]
        swo = H.rel_off(sizes)
        data = oracle.generate(oracle.preset(cfg), swo)
        pk, off = oracle.pack_batch(data, swo, threads=8)
        return sizes, data.tobytes(), pk.tobytes(), np.asarray(off, dtype=np.uint64)
    return _once(("stream", name), make)


@pytest.mark.parametrize("where", H.WORD_WHERE)
@pytest.mark.parametrize("name", list(H.STREAMS))
def test_decode_stream(ctx, oracle, arenas, name, where):
    """cpk_decode_stream's output placement: d_seg_word_off above and across
    LINE; the packed pointer is the byte arena's base plus a 16-aligned
    position above, at and across it.  One stream for each reader (one wave,
    one workgroup, parallel blocks)."""
    sizes, data, pk, off = _stream(oracle, name)
    n = len(sizes)
    wlay = H.place_words(sizes, where)
    pos = H.stream_position(len(pk), where)
    play = H.Layout("low", 1, np.array([pos, pos + len(pk)], np.uint64), None, None)
    P, W = arenas.bytes(), arenas.words()
    before = _put(P, play, pk)
    _sentinels(W, wlay)
    d_swo = _dev64(wlay.off)
    d_io = _full(n + 1 + TAIL, SENT_W, W.dtype)
    d_st = _full(n + TAIL, ST_SENT, _i32())
    _pre(d_swo, wlay)
    assert pos % 16 == 0 and (pos >= LINE if where == "above" else pos < LINE <= pos + len(pk) + 15)
    ctx.decode_stream(P[pos:], len(pk), d_swo, W, d_io[:n + 1], d_st[:n])
    st, io = d_st.cpu().numpy(), d_io.cpu().numpy()
    assert (st[n:] == ST_SENT).all() and (io[n + 1:] == SENT_W).all()
    assert (st[:n] == OK).all(), st[:n]
    assert np.array_equal(io[:n + 1].astype(np.uint64), off), "d_in_off"
    below, body, above = _window(W, wlay)
    _guards_intact(below, above, "output words")
    assert body.tobytes() == data
    assert _unchanged(P, play, before), "the packed bytes or their guards were written"


@pytest.mark.parametrize("where", H.BYTE_WHERE)
@pytest.mark.parametrize("n", H.DECODE_N)
@pytest.mark.parametrize("density", list(H.DECODE_CFG))
def test_unpacked_size_wave_form(usize_wave_ctx, oracle, arenas, density, n, where):
    """cpk_unpacked_size_batch, a wave per piece (the default choice for these
    batches, and forced): the decode batches with d_in_off high."""
    import _unpacked_size_model as M
    pieces, sizes, words, packed, ost = _decode_batch(oracle, density, n)
    assert M.unpacked_size(pieces[H.BAD]) == (ETRUNC, 0)
    counts = [0 if i == H.BAD else s for i, s in enumerate(sizes)]
    blay = H.place_bytes([len(p) for p in pieces], where)
    P = arenas.bytes()
    before = _put(P, blay, packed)
    d_in_off = _dev64(blay.off)
    d_swo = _full(n + 1 + TAIL, SENT_W, arenas.words().dtype)
    d_st = _full(n + TAIL, ST_SENT, _i32())
    _pre(d_in_off, blay)
    usize_wave_ctx.unpacked_size_batch(P, d_in_off, d_swo[:n + 1], d_st)
    swo, st = d_swo.cpu().numpy(), d_st.cpu().numpy()
    assert (swo[n + 1:] == SENT_W).all() and (st[n:] == ST_SENT).all()
    assert st[:n].tolist() == ost.tolist()
    assert np.array_equal(swo[:n + 1].astype(np.uint64), H.rel_off(counts))
    assert _unchanged(P, blay, before), "the packed bytes or their guards were written"


@pytest.mark.parametrize("cut", [0, 3])
def test_unpacked_size_block_map_form(usize_map_ctx, oracle, arenas, cut):
    """cpk_unpacked_size_batch of one piece of about 80 KiB that starts on a
    16-byte line 40 KiB below LINE: sized by the block map over its own bytes
    (include/capnp_packed.h: 'only the block-map path of a batch of at most 32
    pieces measures in 64 bits'), whole and cut inside its last record."""
    import _unpacked_size_model as M
    words = 10500
    piece = _once("usize-piece", lambda: oracle.pack(oracle.generate(oracle.preset(3), H.rel_off([words]))))
    assert 76 << 10 <= len(piece) <= 84 << 10
    piece = piece[:len(piece) - cut]
    want = _once(("usize-want", cut), lambda: M.unpacked_size(piece))
    assert want == ((OK, words) if cut == 0 else (ETRUNC, 0))
    pos = LINE - (40 << 10)
    lay = H.Layout("straddle", 1, np.array([pos, pos + len(piece)], np.uint64), 0, 40 << 10)
    P = arenas.bytes()
    before = _put(P, lay, piece)
    d_in_off = _dev64(lay.off)
    d_swo = _full(2 + TAIL, SENT_W, arenas.words().dtype)
    d_st = _full(1 + TAIL, ST_SENT, _i32())
    off = [int(x) for x in d_in_off.cpu().numpy()]
    assert off[0] % 16 == 0 and off[0] < LINE < off[1] and off[1] - off[0] >= 64 << 10
    usize_map_ctx.unpacked_size_batch(P, d_in_off, d_swo[:2], d_st)
    swo, st = d_swo.cpu().numpy(), d_st.cpu().numpy()
    assert (swo[2:] == SENT_W).all() and (st[1:] == ST_SENT).all()
    assert (int(st[0]), swo[:2].tolist()) == (want[0], [0, want[1]])
    assert _unchanged(P, lay, before), "the packed bytes or their guards were written"


def _packed_messages(oracle):
    def make():
        msgs = H.messages(20)
        packed = [oracle.write_message(m) for m in msgs]
        for m, p in zip(msgs, packed):
            assert oracle.read_message(p) == (OK, m, len(p))
        # each segment's packed start, from the message's first byte
        starts = []
        for m in msgs:
            o = len(oracle.pack(H.table_bytes(m)))
            for s in m:
                starts.append(o)
                o += len(oracle.pack(s))
        return msgs, packed, starts
    return _once("packed-messages", make)


@pytest.mark.parametrize("where", H.BYTE_WHERE)
def test_decode_messages(ctx, oracle, arenas, where):
    """cpk_decode_messages of 20 packed messages with d_msg_off above, at the
    edge and straddling; d_seg_in_off holds absolute positions above LINE."""
    msgs, packed, starts = _packed_messages(oracle)
    nm = len(msgs)
    segs = [s for m in msgs for s in m]
    S, Wt = len(segs), sum(len(s) // 8 for s in segs)
    lay = H.place_bytes([len(p) for p in packed], where)
    P = arenas.bytes()
    before = _put(P, lay, b"".join(packed))
    d_moff = _dev64(lay.off)
    i64 = arenas.words().dtype
    d_out = _full(Wt + TAIL, SENT_W, i64)
    d_swo = _full(S + 1 + TAIL, SENT_W, i64)
    d_sin = _full(S + TAIL, SENT_W, i64)
    d_sst = _full(S + TAIL, ST_SENT, _i32())
    d_mseg = _full(nm + 1 + TAIL, SENT_W, i64)
    d_mst = _full(nm + TAIL, ST_SENT, _i32())
    _pre(d_moff, lay)
    rc, W2, S2 = ctx.decode_messages(P, d_moff, d_out[:Wt], d_swo[:S + 1], d_sin[:S], d_sst[:S], d_mseg, d_mst)
    out, swo, sin = d_out.cpu().numpy(), d_swo.cpu().numpy(), d_sin.cpu().numpy()
    sst, mseg, mst = d_sst.cpu().numpy(), d_mseg.cpu().numpy(), d_mst.cpu().numpy()
    assert rc == OK and (W2, S2) == (Wt, S)
    for a, k, sent in ((out, Wt, SENT_W), (swo, S + 1, SENT_W), (sin, S, SENT_W), (sst, S, ST_SENT),
                       (mseg, nm + 1, SENT_W), (mst, nm, ST_SENT)):
        assert (a[k:] == sent).all(), "written past an output array's end"
    assert (mst[:nm] == OK).all() and (sst[:S] == OK).all()
    assert np.array_equal(mseg[:nm + 1].astype(np.uint64), H.rel_off([len(m) for m in msgs]))
    assert np.array_equal(swo[:S + 1].astype(np.uint64), H.rel_off([len(s) // 8 for s in segs]))
    want_in = [int(lay.off[m]) + starts[j] for m in range(nm) for j in range(int(mseg[m]), int(mseg[m + 1]))]
    assert sin[:S].tolist() == want_in, "d_seg_in_off"
    assert max(want_in) > LINE
    assert out[:Wt].tobytes() == b"".join(segs)
    assert _unchanged(P, lay, before), "the packed bytes or their guards were written"


@pytest.mark.parametrize("where", H.AT_WHERE)
def test_encode_batch_at_high_destinations(at_ctx, oracle, arenas, where):
    """cpk_encode_batch_at with d_dst_off above LINE at arbitrary alignments,
    in descending order: groups of 1, 2 and 5 pieces; one slot's bytes cross
    LINE (cross), or one slot ends exactly at LINE and the next starts there
    (abut); one slot is a byte short.  Nothing but the CPK_OK groups' bytes is
    written in the slots' range and the guard windows around it."""
    sizes = [w for g in H.AT_GROUPS for w in g]
    data = _once("at-data", lambda: oracle.generate(oracle.preset(2), H.rel_off(sizes)))
    packs = _once("at-packs", lambda: _piece_packs(oracle, sizes, data))
    n, ng = len(sizes), len(H.AT_GROUPS)
    grp = H.rel_off([len(g) for g in H.AT_GROUPS]).astype(np.int64)
    bodies = [b"".join(packs[grp[g]:grp[g + 1]]) for g in range(ng)]
    dst, cap = H.at_slots([len(b) for b in bodies], where)
    lo, hi = min(dst), max(o + c for o, c in zip(dst, cap))
    P = arenas.bytes()
    a, b = lo - H.GUARD, hi + H.GUARD
    P[a:b] = SENT
    i64 = arenas.words().dtype
    d_in = _dev8(np.concatenate([data, np.zeros(8, np.uint8)])).view(i64)
    d_swo, d_grp, d_dst, d_cap = _dev64(H.rel_off(sizes)), _dev64(grp), _dev64(dst), _dev64(cap)
    d_poff = _full(n + TAIL, SENT_W, i64)
    d_glen = _full(ng + TAIL, SENT_W, i64)
    d_st = _full(ng + TAIL, ST_SENT, _i32())
    # the precondition, on the device's arrays
    h_dst, h_cap = [int(x) for x in d_dst.cpu().numpy()], [int(x) for x in d_cap.cpu().numpy()]
    assert all(x > y for x, y in zip(h_dst, h_dst[1:])) and all(o >= LINE for o in h_dst[:-1])
    if where == "cross":
        assert h_dst[-1] < LINE < h_dst[-1] + len(bodies[-1])
    else:
        assert h_dst[-1] + h_cap[-1] == LINE == h_dst[-2] and len(bodies[-1]) == h_cap[-1]
    at_ctx.encode_batch_at(d_in, d_swo, max(sizes), d_grp, P, H.BYTE_ARENA, d_dst, d_cap, d_poff, d_glen, d_st)
    got = P[a:b].cpu().numpy()
    poff, glen, st = d_poff.cpu().numpy(), d_glen.cpu().numpy(), d_st.cpu().numpy()
    assert (poff[n:] == SENT_W).all() and (glen[ng:] == SENT_W).all() and (st[ng:] == ST_SENT).all()
    assert st[:ng].tolist() == [ENOMEM if g == H.AT_SHORT else OK for g in range(ng)]
    assert glen[:ng].tolist() == [len(x) for x in bodies]
    want_poff = []
    for g in range(ng):
        o = dst[g]
        for p in packs[grp[g]:grp[g + 1]]:
            want_poff.append(o)
            o += len(p)
    assert poff[:n].tolist() == want_poff and min(want_poff[:-1]) >= LINE
    want = np.full(got.size, SENT, np.uint8)
    care = np.ones(got.size, bool)
    for g in range(ng):
        if g == H.AT_SHORT:  # (the bytes inside a refused group's own slot are undefined)
            care[dst[g] - a:dst[g] - a + cap[g]] = False
        else:
            want[dst[g] - a:dst[g] - a + len(bodies[g])] = np.frombuffer(bodies[g], np.uint8)
    bad = np.nonzero((got != want) & care)[0]
    assert bad.size == 0, f"{bad.size} wrong bytes, the first at arena byte {a + int(bad[0])}"


# ---- Part 3: packed output that itself passes 4 GiB ------------------------------------------
def test_packed_output_passes_the_line(ctx, oracle, arenas):
    """About 4.6 GiB of dense pieces (generator config 3, sizes cycling through
    8192, 3000, 8191, 12000, 17, 4096 words) through cpk_encode_batch:
    d_out_off passes 2^32.  The offsets equal cpk_packed_size_batch's (another
    kernel); the pieces around byte 2^32, the first, the last and 32 random
    ones have exactly the oracle's bytes; cpk_decode_batch of the result is
    CPK_OK throughout and gives the input back."""
    import torch
    import capnp_packed as cp
    arenas.release()
    t0 = time.perf_counter()
    sizes = H.part3_sizes()
    n = len(sizes)
    swo = H.rel_off(sizes)
    total, maxw = int(swo[-1]), max(sizes)
    cap = (cp.batch_capacity(swo) + 15) // 16 * 16
    d_in = _alloc(total, torch.int64)
    d_pk = _alloc(cap, torch.uint8)
    d_out = _alloc(total, torch.int64)
    d_swo = _dev64(swo)
    ctx.generate(cp.preset(3), d_swo, d_in)
    d_off = _full(n + 1, SENT_W, torch.int64)
    d_soff = _full(n + 1, SENT_W, torch.int64)
    ctx.encode_batch(d_in, d_swo, maxw, d_pk, d_off)
    assert ctx.take_error() == cp.OK
    off = d_off.cpu().numpy().astype(np.uint64)
    assert int(off[n]) > LINE, "the packed output does not pass 2^32 bytes"
    ctx.packed_size_batch(d_in, d_swo, maxw, d_soff)
    assert ctx.take_error() == cp.OK
    assert torch.equal(d_off, d_soff), "cpk_encode_batch's offsets differ from cpk_packed_size_batch's"
    k, pick = H.part3_sample(off)
    assert int(off[k]) <= LINE < int(off[k + 1])
    op = oracle.preset(3)
    for i in pick:
        want = oracle.pack(oracle.generate(op, swo, first=i, count=1))
        a, b = int(off[i]), int(off[i + 1])
        assert b - a == len(want), f"piece {i}: {b - a} packed bytes, oracle {len(want)}"
        assert d_pk[a:b].cpu().numpy().tobytes() == want, f"piece {i} at byte {a}"
    d_st = _full(n, ST_SENT, torch.int32)
    ctx.decode_batch(d_pk, d_off, d_swo, d_out, d_st)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.count_mismatch(d_in, d_out, total, cnt)
    assert int((d_st != OK).sum().item()) == 0
    assert int(cnt.item()) == 0
    free, dev_total = torch.cuda.mem_get_info()
    peak = torch.cuda.max_memory_allocated()
    print(f"\npart 3: {time.perf_counter() - t0:.2f} s for {n} pieces, {total * 8 / 2**30:.2f} GiB of words, "
          f"{int(off[n]) / 2**30:.2f} GiB packed; peak {peak / 2**30:.2f} GiB in tensors, "
          f"{(dev_total - free) / 2**30:.2f} GiB of the device in use")
    assert peak <= PEAK_LIMIT
    del d_in, d_pk, d_out
    torch.cuda.empty_cache()
