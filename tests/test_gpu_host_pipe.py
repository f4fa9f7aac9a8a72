"""The host staging's edges (csrc/host_pipe.hip): the chunk pipeline's
prologue and epilogue at one to four chunks and with empty chunks, an output
capacity that runs out in the middle of the pipeline, and one context taken
through every host form, small, large and small again, so that the pinned
slots regrow under single-slot and two-slot forms in turn.  Every expected
byte, offset and status is the oracle's."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, ENOMEM = 0, -5
MIX = [.4, .3, .2, .1]


def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _random_words(rng, n, probs=MIX):
    """n words as bytes: all-zero words, one zero byte, several, none."""
    kind = rng.choice(4, size=n, p=probs)
    w = rng.integers(1, 256, size=(n, 8), dtype=np.uint8)
    w[kind == 0] = 0
    one = np.where(kind == 1)[0]
    w[one, rng.integers(0, 8, size=one.size)] = 0
    for i in np.where(kind == 2)[0]:
        w[i, rng.choice(8, size=int(rng.integers(2, 8)), replace=False)] = 0
    return w.reshape(-1)


def _table(sizes):
    """The segment table's words (Serialize.java:256-273) as bytes."""
    t = np.zeros((len(sizes) + 2) & ~1, np.uint32)
    t[0] = len(sizes) - 1
    t[1:1 + len(sizes)] = sizes
    return t.tobytes()


@functools.lru_cache(maxsize=None)
def _case(sizes, seed, per_msg=1):
    """Pieces of the given sizes, and the same pieces as messages of per_msg
    segments, with everything the oracle says about them."""
    import oracle
    rng = np.random.default_rng(seed)
    parts = [_random_words(rng, s) for s in sizes]
    swo = _swo(sizes)
    data = np.concatenate(parts + [np.zeros(0, np.uint8)])
    pk, off = oracle.pack_batch(data, swo, threads=8)
    back, st = oracle.unpack_batch(pk, off, swo, threads=8)
    assert np.array_equal(back, data) and (st == 0).all()
    msgs = [[p.tobytes() for p in parts[i:i + per_msg]] for i in range(0, len(parts), per_msg)]
    mpk = [oracle.write_message(m) for m in msgs]
    return dict(parts=parts, swo=swo, data=data, pk=pk, off=off, msgs=msgs, mpk=b"".join(mpk),
                moff=_swo([len(m) for m in mpk]))


def _check_piece_forms(ctx, c):
    pk, off = ctx.encode_host(c["data"], c["swo"])
    assert np.array_equal(off, c["off"]) and np.array_equal(pk, c["pk"])
    pk, off = ctx.encode_host_gather([p.view(np.uint64) for p in c["parts"]])
    assert np.array_equal(off, c["off"]) and np.array_equal(pk, c["pk"])
    dec, st = ctx.decode_host(c["pk"], c["off"], c["swo"])
    assert (st == 0).all() and np.array_equal(dec, c["data"])


def _piece_offsets(c):
    """The oracle's packed offset of every piece of the message batch, in
    message order: a message's table, then its segments."""
    import oracle
    o, offs = 0, [0]
    for m in c["msgs"]:
        for piece in [_table([len(s) // 8 for s in m])] + m:
            o += len(oracle.pack(piece))
            offs.append(o)
    return np.array(offs, np.uint64)


def _check_message_forms(ctx, c):
    want_off = _piece_offsets(c)
    for enc in (ctx.encode_messages_host, ctx.encode_messages_host_gather):
        pk, off = enc(c["msgs"])
        assert pk == c["mpk"] and np.array_equal(off, want_off)
    st, got = ctx.decode_messages_host(c["mpk"], c["moff"])
    assert (st == 0).all() and got == c["msgs"]


# one chunk per piece of 8,192 words at CPK_HOST_CHUNK_KB=64; an all-empty
# batch is one chunk without input; a last chunk that is one empty piece
# follows a piece larger than a chunk
CHUNK_COUNTS = {"1": (8192,), "2": (8192,) * 2, "3": (8192,) * 3, "4": (8192,) * 4,
                "all-empty": (0,) * 5, "empty-last": (8192, 9000, 0)}


@pytest.mark.parametrize("name", list(CHUNK_COUNTS))
def test_chunk_counts(ctx, oracle, name, monkeypatch):
    """K = 1..4 chunks, so that the loop's first and last two rounds (no
    chunk to send, none to land) meet every K; chunks without bytes."""
    monkeypatch.setenv("CPK_HOST_CHUNK_KB", "64")
    c = _case(CHUNK_COUNTS[name], 7)
    _check_piece_forms(ctx, c)
    _check_message_forms(ctx, c)  # (single-segment messages: a table and a segment each)


def _encode_host_raw(ctx, c, cap):
    out = np.zeros(max(cap, 1), np.uint8)
    off = np.zeros(len(c["swo"]), np.uint64)
    rc = ctx._lib.cpk_encode_host(ctx.handle, c["data"].ctypes.data, c["swo"].ctypes.data, len(c["swo"]) - 1,
                                  out.ctypes.data, cap, off.ctypes.data)
    return rc, out[:cap], off


def _encode_messages_host_raw(ctx, c, cap):
    segs = [s for m in c["msgs"] for s in m]
    mso = _swo([len(m) for m in c["msgs"]])
    out = np.zeros(max(cap, 1), np.uint8)
    off = np.zeros(len(c["msgs"]) + len(segs) + 1, np.uint64)
    rc = ctx._lib.cpk_encode_messages_host(ctx.handle, c["data"].ctypes.data, c["swo"].ctypes.data, len(segs),
                                           mso.ctypes.data, len(c["msgs"]), out.ctypes.data, cap,
                                           off.ctypes.data)
    return rc, out[:cap], off


def test_output_capacity_mid_pipeline(ctx, oracle, monkeypatch):
    """The caller's `out` at exactly the packed size is enough; a byte less,
    or half, is refused with CPK_ENOMEM while later chunks are in flight, and
    the same context then encodes the batch again with nothing left over."""
    monkeypatch.setenv("CPK_HOST_CHUNK_KB", "1")
    rng = np.random.default_rng(23)
    sizes = tuple(int(s) for s in rng.integers(200, 2501, size=20))  # (each piece over 1 KiB: a chunk each)
    c = _case(sizes, 23, per_msg=2)
    assert len(c["data"]) >= 6 << 10
    for raw, want in ((_encode_host_raw, c["pk"].tobytes()), (_encode_messages_host_raw, c["mpk"])):
        for cap in (len(want) - 1, len(want) // 2, len(want)):
            rc, out, _ = raw(ctx, c, cap)
            if cap < len(want):
                assert rc == ENOMEM, (raw.__name__, cap, rc)
                rc, out, _ = raw(ctx, c, len(want))
            assert rc == OK and out.tobytes() == want, (raw.__name__, cap, rc)
            assert ctx.take_error() == OK


def _shape(small):
    """20 messages of 3 segments: a few hundred words, or a few hundred
    thousand with a first message of 150,000 (over the one-launch read)."""
    rng = np.random.default_rng(5 if small else 6)
    sizes = rng.integers(0, 11, size=60) if small else rng.integers(0, 8001, size=60)
    if not small:
        sizes[:3] = 50000
    return _case(tuple(int(s) for s in sizes), 11 + small, per_msg=3)


def _host_forms(ctx, c):
    """name -> a check of one host entry point against the oracle; the
    two-slot forms and the single-slot ones take turns."""
    import oracle

    def encode_host():
        pk, off = ctx.encode_host(c["data"], c["swo"])
        assert np.array_equal(off, c["off"]) and np.array_equal(pk, c["pk"])

    def decode_stream_host():
        dec, io, st = ctx.decode_stream_host(c["pk"], c["swo"])
        assert (st == 0).all() and np.array_equal(io, c["off"]) and np.array_equal(dec, c["data"])

    def encode_host_gather():
        pk, off = ctx.encode_host_gather([p.view(np.uint64) for p in c["parts"]])
        assert np.array_equal(off, c["off"]) and np.array_equal(pk, c["pk"])

    def read_message_host():
        first = c["mpk"][: int(c["moff"][1])]
        ost, segs, used = oracle.read_message(first, out_cap=sum(len(s) for s in c["msgs"][0]) + 4096)
        st, got, consumed, _ = ctx.read_message_host(c["mpk"])  # (the later messages lie behind it)
        assert (st, got, consumed) == (ost, segs, used) == (OK, c["msgs"][0], len(first))

    def decode_host():
        dec, st = ctx.decode_host(c["pk"], c["off"], c["swo"])
        assert (st == 0).all() and np.array_equal(dec, c["data"])

    def decode_message_stream_host():
        tail, got, consumed = ctx.decode_message_stream_host(c["mpk"])
        assert (tail, consumed) == (OK, len(c["mpk"])) and got == c["msgs"]

    def encode_messages_host():
        pk, off = ctx.encode_messages_host(c["msgs"])
        assert pk == c["mpk"] and np.array_equal(off, _piece_offsets(c))

    def encode_message_stream_host():
        stream = b"".join(_table([len(s) // 8 for s in m]) + b"".join(m) for m in c["msgs"])
        tail, pk, off, mp, consumed = ctx.encode_message_stream_host(stream)
        assert (tail, consumed) == (OK, len(stream) // 8) and pk == c["mpk"]
        assert np.array_equal(off, _piece_offsets(c))
        assert [int(v) for v in mp] == [4 * m for m in range(len(c["msgs"]) + 1)]

    def encode_messages_host_gather():
        pk, off = ctx.encode_messages_host_gather(c["msgs"])
        assert pk == c["mpk"] and np.array_equal(off, _piece_offsets(c))

    def decode_messages_host():
        st, got = ctx.decode_messages_host(c["mpk"], c["moff"])
        assert (st == 0).all() and got == c["msgs"]

    return [encode_host, decode_stream_host, encode_host_gather, read_message_host, decode_host,
            decode_message_stream_host, encode_messages_host, encode_message_stream_host,
            encode_messages_host_gather, decode_messages_host]


@pytest.mark.parametrize("chunk_kb", [None, "4"])
def test_one_context_every_host_form(ctx, oracle, chunk_kb, monkeypatch):
    """Small, large, small again on one context through all ten host entry
    points: the slots are grown by whichever form first needs more (a
    single-slot form grows slot 0 alone, the next two-slot form then slot 1)
    and serve the small shapes afterwards.  Each pass starts at another form."""
    if chunk_kb:
        monkeypatch.setenv("CPK_HOST_CHUNK_KB", chunk_kb)
    for turn, small in enumerate((True, False, True)):
        forms = _host_forms(ctx, _shape(small))
        assert len(forms) == 10
        for f in forms[turn:] + forms[:turn]:
            f()
