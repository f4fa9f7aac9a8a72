"""cpk_encode_messages_at: messages packed to the slots the caller names, the
segment tables built on the device (encode_msg_at.hip: the wave form over the
two passes, the placed form over sp_place_kernel dense and sparse).  Expected
bytes, lengths, offsets and statuses come from tests/_encode_messages_at_model.py,
which is built on the oracle (oracle.pack, oracle.write_message) -- never from
another GPU call, except in the tests where equality with another call is the
thing asserted.  The output buffer is filled with a sentinel and carries a
sentinel pad after out_cap: every test asserts that every byte outside the
CPK_OK messages' packed bytes is still the sentinel, and for a refused message
that every byte outside its slot is.  Each context is created here with
CPK_MSG_AT_FORM unset, wave and place, the last with CPK_AT_FORM dense and
sparse."""
import os

import numpy as np
import pytest

import _encode_messages_at_model as M
import _high_offsets as H

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 4096  # sentinel bytes after out_cap
OK, EINVAL, ENOMEM = M.OK, M.EINVAL, M.ENOMEM
CHUNK = 8192
# test_gpu_encode_at.py's list: the step edge, one wave's 32 steps against the
# spread over four waves, the unit table, the chunk hand-over, the look-back
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 16385, 3 * CHUNK + 1]
MAXW = 3 * CHUNK + 1
KINDS = [2, 3, 4, "nz", "zero"]
FORMS = [(None, None), ("wave", None), ("place", "dense"), ("place", "sparse")]


def _context(forms):
    """A context under a CPK_MSG_AT_FORM / CPK_AT_FORM pair (read at context creation)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    want = dict(zip(("CPK_MSG_AT_FORM", "CPK_AT_FORM"), forms))
    saved = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        c = cp.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield c
    finally:
        c.close()


@pytest.fixture(scope="module", params=FORMS, ids=["form-auto", "form-wave", "form-place-dense", "form-place-sparse"])
def mctx(request):
    yield from _context(request.param)


@pytest.fixture(scope="module", params=[("wave", None), ("place", None)], ids=["form-wave", "form-place"])
def lctx(request):
    """One wave and one placed context, for the test whose input is large."""
    yield from _context(request.param)


# ---- data -------------------------------------------------------------------------
_DATA = {}


def _segments(oracle, kind, sizes):
    """Segments of `sizes` words: kind 2 / 3 / 4 the generator's presets, "nz"
    all-nonzero words, "zero" all-zero words.  Built once per (kind, sizes)."""
    key = (kind, tuple(sizes))
    if key not in _DATA:
        swo = H.rel_off(sizes).astype(np.int64)
        if kind == "zero":
            data = np.zeros(8 * sum(sizes), np.uint8)
        elif kind == "nz":
            data = np.random.default_rng(11).integers(1, 256, size=8 * sum(sizes), dtype=np.uint8)
        else:
            data = oracle.generate(oracle.preset(kind), swo.astype(np.uint64))
        b = np.ascontiguousarray(data, np.uint8).tobytes()
        _DATA[key] = [b[8 * swo[i]:8 * swo[i + 1]] for i in range(len(sizes))]
    return _DATA[key]


def _messages(oracle, kind, shapes):
    """Messages of the given segment sizes (a list of lists)."""
    segs = _segments(oracle, kind, [w for s in shapes for w in s])
    out, p = [], 0
    for s in shapes:
        out.append(segs[p:p + len(s)])
        p += len(s)
    return out


def _len(oracle, msg):
    return sum(len(p) for p in M.packed_pieces(oracle, msg))


def _layout(oracle, msgs, gap=lambda g: (5 * g + 3) % 16, room=lambda g: 0, start=5):
    """Slots in message order: each its packed bytes + room(g), gap(g) bytes
    between them -- every line phase at both ends and at the table seam.
    -> (dst_off, dst_cap, out_cap)"""
    off, cap, cur = [], [], start
    for g, m in enumerate(msgs):
        n = _len(oracle, m)
        off.append(cur)
        cap.append(n + room(g))
        cur += n + room(g) + gap(g)
    return off, cap, cur + 3


def _dev64(v):
    import torch
    return torch.from_numpy(np.asarray(list(v) + [0], dtype=np.uint64).view(np.int64).copy()).cuda()


# ---- one call ---------------------------------------------------------------------
class Call:
    """The device arrays of one cpk_encode_messages_at call; launched by the
    constructor, read back (after a sync) by results()."""

    def __init__(self, ctx, msgs, dst_off, dst_cap, out_cap, maxw, misalign=0, drop=None):
        import torch
        segs = [s for m in msgs for s in m]
        self.nm, self.np = len(msgs), len(msgs) + len(segs)
        data = np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8)
        self.d_in = torch.from_numpy(data.view(np.int64).copy()).cuda()
        self.d_swo = _dev64(H.rel_off([len(s) // 8 for s in segs]))[:len(segs) + 1]
        self.d_mseg = _dev64(H.rel_off([len(m) for m in msgs]))[:len(msgs) + 1]
        self.d_off = _dev64(dst_off)
        self.d_cap = None if dst_cap is None else _dev64(dst_cap)
        self.buf = torch.full((out_cap + PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.d_poff = torch.full((self.np + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_len = torch.full((self.nm + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((self.nm + 1,), 77, dtype=torch.int32, device="cuda")
        a = dict(d_in=self.d_in, d_seg_word_off=self.d_swo, d_msg_seg_off=self.d_mseg, max_seg_words=maxw,
                 d_out=self.buf[misalign:], out_cap=out_cap, d_dst_off=self.d_off, d_dst_cap=self.d_cap,
                 d_piece_off=self.d_poff, d_msg_len=self.d_len, d_status=self.d_st)
        if drop:
            a[drop] = None
        ctx.encode_messages_at(nm=self.nm, nseg=len(segs), **a)

    def results(self):
        import torch
        torch.cuda.synchronize()
        poff, ln, st = self.d_poff.cpu().numpy(), self.d_len.cpu().numpy(), self.d_st.cpu().numpy()
        assert poff[self.np] == -1 and ln[self.nm] == -1 and st[self.nm] == 77, "written past an output array's end"
        return self.buf.cpu().numpy(), poff[:self.np], ln[:self.nm], st[:self.nm]


def _compare(exp, buf, poff, ln, st, msgs, out_cap):
    assert st.tolist() == exp.status, f"d_status {st.tolist()}, the model's {exp.status}"
    p = 0
    for m, msg in enumerate(msgs):
        if exp.defined[m]:
            assert int(ln[m]) == exp.msg_len[m], f"message {m}: d_msg_len {ln[m]}, the model's {exp.msg_len[m]}"
            got = [int(x) & M.U64 for x in poff[p:p + 1 + len(msg)]]
            assert got == exp.piece_off[p:p + 1 + len(msg)], f"message {m}: d_piece_off"
        p += 1 + len(msg)
    bad = np.nonzero((buf != exp.image) & exp.care)[0]
    assert bad.size == 0, (f"{bad.size} wrong bytes, the first at {bad[0]} (out_cap {out_cap}): "
                           f"{buf[bad[0]]:#x}, expected {exp.image[bad[0]]:#x}")


def _verify(call, oracle, msgs, dst_off, dst_cap, out_cap, maxw):
    """Statuses, lengths, piece offsets and every byte of the buffer against the model."""
    buf, poff, ln, st = call.results()
    _compare(M.expected(oracle, msgs, dst_off, dst_cap, out_cap, maxw, buf.size, SENTINEL), buf, poff, ln, st, msgs,
             out_cap)
    return st


def _run(ctx, oracle, msgs, dst_off, dst_cap, out_cap, maxw=MAXW):
    return _verify(Call(ctx, msgs, dst_off, dst_cap, out_cap, maxw), oracle, msgs, dst_off, dst_cap, out_cap, maxw)


# ---- 1. segment counts and sizes --------------------------------------------------
def _count_shapes():
    """Messages of 1, 2, 3 and 4 segments that between them hold every size of
    SIZES (odd / even count: with and without the table's pad half-word), one
    of empty segments only, and messages of 511 and 512 segments (a 256- and a
    257-word table) of small sizes with a few large ones among them."""
    shapes, k = [], 0
    for count in (1, 2, 3, 4, 1, 2, 3, 4):
        shapes.append([SIZES[5 * (k + j) % len(SIZES)] for j in range(count)])  # (5 and 14 are coprime)
        k += count
    shapes.insert(3, [0, 0, 0])
    small = [0, 1, 63, 64, 65]
    for count in (511, 512):
        s = [small[(3 * j + count) % len(small)] for j in range(count)]
        s[7], s[count // 2], s[count - 1] = 2049, CHUNK + 1, 2047
        shapes.append(s)
    assert {w for s in shapes for w in s} >= set(SIZES)
    return shapes


@pytest.mark.parametrize("kind", KINDS)
def test_segment_counts_and_sizes(mctx, oracle, kind):
    msgs = _messages(oracle, kind, _count_shapes())
    off, cap, out_cap = _layout(oracle, msgs)
    st = _run(mctx, oracle, msgs, off, cap, out_cap)  # exact capacities
    assert (st == OK).all()


def test_lookback_inside_a_message(mctx, oracle):
    """A 3-chunk segment in a message between one-word messages, and one with
    segments before and after it: the placed form's look-back stops at the
    message's first unit, and the wave form's offsets sum over the message."""
    msgs = _messages(oracle, 2, [[1], [3 * CHUNK + 1], [1], [65, 3 * CHUNK + 1, 300], [1]])
    off, cap, out_cap = _layout(oracle, msgs, room=lambda g: 3 * (g % 2))
    assert (_run(mctx, oracle, msgs, off, cap, out_cap) == OK).all()


def test_table_of_literal_words(lctx, oracle):
    """A 512-segment message whose sizes are all 0x01010101 words: every table
    word after the first has eight nonzero bytes, so serial_pack takes its
    literal-run path (257 words: a run of 254 behind the second, up to the
    last word with its pad).  Sizes of 2^24 words and more are what that
    takes, so the input is 512 x 128.5 MiB: about 69 GB of device memory,
    which is why this test runs in one wave and one placed context only.  The
    segments exist on the device only: zero words, but for a 1 in the last
    word of every 8192 (a zero run that crossed every chunk edge would make
    the placed form's chunks wait for each other one by one); one segment is
    packed by the oracle and stands for all 512."""
    import torch
    w, count = 0x01010101, 512
    host = np.zeros(w, np.int64)
    host[:w // CHUNK * CHUNK].reshape(-1, CHUNK)[:, CHUNK - 1] = 1
    seg = host.tobytes()
    msg = [seg] * count
    table = M.pack(oracle, M.table_bytes(msg))
    assert table[7] == 0xff and table[16] == 254  # (the first word's tag and 6 bytes; then 0xff, 8 bytes, the count)
    one = M.pack(oracle, seg)
    n = len(table) + count * len(one)
    off, out_cap = 11, 11 + n + 5
    d_in = torch.zeros(count * w + 8, dtype=torch.int64, device="cuda")
    d_in[:count * w].view(count, w)[:, :w // CHUNK * CHUNK].view(count, -1, CHUNK)[:, :, CHUNK - 1] = 1
    d_swo = _dev64([w * i for i in range(count + 1)])
    d_mseg, d_off, d_cap = _dev64([0, count]), _dev64([off]), _dev64([n])
    buf = torch.full((out_cap + PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_poff = torch.full((count + 2,), -1, dtype=torch.int64, device="cuda")
    d_len = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    lctx.encode_messages_at(d_in, d_swo, d_mseg, w, buf, out_cap, d_off, d_cap, d_poff, d_len, d_st, nm=1, nseg=count)
    torch.cuda.synchronize()
    del d_in
    assert d_st.cpu().tolist() == [OK, 77] and d_len.cpu().tolist() == [n, -1]
    want_poff = [off] + [off + len(table) + i * len(one) for i in range(count)] + [-1]
    assert d_poff.cpu().tolist() == want_poff
    got = buf.cpu().numpy()
    assert got[off:off + len(table)].tobytes() == table
    body = got[off + len(table):off + n].reshape(count, len(one))
    assert (body == np.frombuffer(one, np.uint8)).all()
    assert (got[:off] == SENTINEL).all() and (got[off + n:] == SENTINEL).all()


# ---- 2. slots ------------------------------------------------------------------------
MIXED_SHAPES = [[300], [2049, 17], [64, 0, 4095, 65, 1], [8192], [8193, 63], [0], [17, 300, 2000, 1, 64], [16385]]


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_slot_order(mctx, oracle, order):
    msgs = _messages(oracle, 2, MIXED_SHAPES)
    sizes = [_len(oracle, m) for m in msgs]
    idx = list(range(len(msgs)))[::-1] if order == "descending" else \
        [int(i) for i in np.random.default_rng(5).permutation(len(msgs))]
    slots, cur = {}, 9
    for j in idx:
        slots[j] = cur
        cur += sizes[j] + 5
    assert (_run(mctx, oracle, msgs, [slots[j] for j in range(len(msgs))], sizes, cur) == OK).all()


@pytest.mark.parametrize("cfg", [2, 3])
def test_without_capacities(mctx, oracle, cfg):
    """d_dst_cap == NULL: every slot runs to out_cap; the last message ends
    exactly there, and one placed a byte further on would not fit."""
    msgs = _messages(oracle, cfg, MIXED_SHAPES)
    off, cap, _ = _layout(oracle, msgs)
    out_cap = off[-1] + cap[-1]
    assert (_run(mctx, oracle, msgs, off, None, out_cap) == OK).all()
    off[-1] += 1
    st = _run(mctx, oracle, msgs, off, None, out_cap)
    assert st.tolist() == [OK] * (len(msgs) - 1) + [ENOMEM]


def test_roomy_slots(mctx, oracle):
    msgs = _messages(oracle, 3, MIXED_SHAPES)
    off, cap, out_cap = _layout(oracle, msgs, room=lambda g: 7 * (g % 3))
    assert (_run(mctx, oracle, msgs, off, cap, out_cap) == OK).all()


# ---- 3. refusals -----------------------------------------------------------------------
def test_refusals(mctx, oracle):
    """One byte short, capacity 0, a capacity smaller than the table, d_dst_off
    past out_cap, a slot that passes out_cap and a segment over max_seg_words,
    each between CPK_OK neighbours that must still be exact; and the context's
    error word stays clear."""
    import capnp_packed as cp
    shapes = [[300], [2049, 17], [65], [64, 1], [17], [8193, 63], [1], [100, 200, 300], [63], [64, 65], [2], [300, 8194],
              [5]]
    msgs = _messages(oracle, 2, shapes)
    off, cap, out_cap = _layout(oracle, msgs, room=lambda g: g % 2)
    out_cap += 64
    cap[1] = _len(oracle, msgs[1]) - 1                      # one byte short
    cap[3] = 0                                              # capacity 0
    cap[5] = len(M.packed_pieces(oracle, msgs[5])[0]) - 1   # smaller than the table
    off[7] = out_cap + 9                                    # past out_cap
    off[9], cap[9] = out_cap - 40, 41                       # passes out_cap by a byte (the message is 1 KiB)
    st = _run(mctx, oracle, msgs, off, cap, out_cap, maxw=8193)  # (message 11 has a segment of 8194 words)
    assert st.tolist() == [OK, ENOMEM, OK, ENOMEM, OK, ENOMEM, OK, ENOMEM, OK, ENOMEM, OK, EINVAL, OK]
    assert mctx.take_error() == cp.OK
    # the same refusals with the table fitting and the segments not, a slot
    # that would hold the message but passes out_cap, and off + cap wrapping
    msgs = _messages(oracle, 3, shapes)
    off, cap, out_cap = _layout(oracle, msgs)
    cap[1] = len(M.packed_pieces(oracle, msgs[1])[0])        # the table alone
    cap[5] = len(M.packed_pieces(oracle, msgs[5])[0]) + 100  # ... and some of the first segment
    cap[9] = M.U64 - 7                                       # off + cap wraps
    last = len(msgs) - 1
    cap[last] = out_cap - off[last] + 1                      # holds the message, ends a byte past out_cap
    st = _run(mctx, oracle, msgs, off, cap, out_cap, maxw=MAXW)
    assert st.tolist() == [OK, ENOMEM, OK, OK, OK, ENOMEM, OK, OK, OK, ENOMEM, OK, OK, ENOMEM]
    assert mctx.take_error() == cp.OK


# ---- 4. many small messages ----------------------------------------------------------------
def test_many_small_messages(mctx, oracle):
    """4,096 one-segment messages of 8 words: the ticket paths of both forms."""
    msgs = _messages(oracle, 2, [[8]] * 4096)
    off, cap, out_cap = _layout(oracle, msgs)
    assert (_run(mctx, oracle, msgs, off, cap, out_cap, maxw=8) == OK).all()


# ---- 5. edge cases ---------------------------------------------------------------------------
def test_no_messages(mctx, oracle):
    _run(mctx, oracle, [], [], [], 64)
    _run(mctx, oracle, [], [], None, 64)


def test_invalid_arguments(mctx, oracle):
    import capnp_packed as cp
    msgs = _messages(oracle, 2, [[64], [65, 1]])
    off, cap, out_cap = _layout(oracle, msgs)
    bad = [dict(misalign=1), dict(maxw=0)] + \
        [dict(drop=k) for k in ("d_msg_seg_off", "d_seg_word_off", "d_out", "d_dst_off", "d_piece_off", "d_msg_len",
                                "d_status")]
    for kw in bad:
        kw.setdefault("maxw", 65)
        with pytest.raises(cp.CodecError) as e:
            Call(mctx, msgs, off, cap, out_cap, **kw)
        assert e.value.status == cp.EINVAL, kw
    assert (_run(mctx, oracle, msgs, off, cap, out_cap, maxw=65) == OK).all()  # (the context is as good as before)


# ---- 6. equalities with the other calls --------------------------------------------------------
@pytest.mark.parametrize("cfg", [2, 4])
def test_agrees_with_the_other_message_calls(mctx, oracle, cfg):
    """The lengths are the per-message differences of cpk_packed_size_messages,
    the placed bytes are cpk_encode_messages' per message, and
    cpk_decode_messages_at over d_dst_off / d_msg_len gives the words back with
    every status CPK_OK."""
    import torch
    import capnp_packed as cp
    msgs = _messages(oracle, cfg, MIXED_SHAPES + _count_shapes()[:5])
    nm = len(msgs)
    segs = [s for m in msgs for s in m]
    S, Wt = len(segs), sum(len(s) // 8 for s in segs)
    off, cap, out_cap = _layout(oracle, msgs)
    call = Call(mctx, msgs, off, cap, out_cap, MAXW)
    st = _verify(call, oracle, msgs, off, cap, out_cap, MAXW)
    assert (st == OK).all()
    mseg = call.d_mseg.cpu().numpy()
    # sizes
    d_soff = torch.full((nm + S + 1,), -1, dtype=torch.int64, device="cuda")
    mctx.packed_size_messages(call.d_in, call.d_swo, call.d_mseg, MAXW, d_soff)
    # the tiled encode
    ref = torch.full((out_cap + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_roff = torch.full((nm + S + 1,), -1, dtype=torch.int64, device="cuda")
    mctx.encode_messages(call.d_in, call.d_swo, call.d_mseg, MAXW, ref, d_roff)
    torch.cuda.synchronize()
    soff, roff, ln = d_soff.cpu().numpy(), d_roff.cpu().numpy(), call.d_len.cpu().numpy()[:nm]
    starts = [int(mseg[m]) + m for m in range(nm)] + [nm + S]
    assert [int(soff[starts[m + 1]] - soff[starts[m]]) for m in range(nm)] == ln.tolist()
    got, tiled = call.buf.cpu().numpy(), ref.cpu().numpy()
    for m in range(nm):
        a = int(roff[starts[m]])
        assert got[off[m]:off[m] + ln[m]].tobytes() == tiled[a:a + ln[m]].tobytes(), f"message {m}"
    # the round trip
    d_out = torch.full((Wt + 8,), -1, dtype=torch.int64, device="cuda")
    d_swo2 = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    d_sin = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    d_sst = torch.full((S,), 77, dtype=torch.int32, device="cuda")
    d_mseg2 = torch.full((nm + 1,), -1, dtype=torch.int64, device="cuda")
    d_mst = torch.full((nm,), 77, dtype=torch.int32, device="cuda")
    d_used = torch.full((nm,), -1, dtype=torch.int64, device="cuda")
    d_tot = torch.full((cp.MAT_TOTALS,), -1, dtype=torch.int64, device="cuda")
    mctx.decode_messages_at(call.buf, out_cap, call.d_off, call.d_len, d_out, d_swo2, d_sin, d_sst, d_mseg2, d_mst,
                            d_used, d_tot, nm=nm, out_cap_words=Wt)
    torch.cuda.synchronize()
    assert (d_mst.cpu().numpy() == OK).all() and (d_sst.cpu().numpy() == OK).all()
    assert d_used.cpu().numpy().tolist() == ln.tolist()
    assert np.array_equal(d_mseg2.cpu().numpy(), mseg)
    assert d_out.cpu().numpy()[:Wt].tobytes() == b"".join(segs)


# ---- 7. offsets above 4 GiB ------------------------------------------------------------------------
def test_slots_around_4_gib(mctx, oracle):
    """A buffer of a little over 4 GiB: one slot ends just below byte 2^32, one
    crosses it, one starts just above, one far above is a byte short.  The
    windows around the slots are compared, not the whole buffer."""
    import torch
    msgs = _messages(oracle, 2, [[300, 17], [2049], [64, 0, 65], [8193, 63]])
    n = [_len(oracle, m) for m in msgs]
    off = [H.LINE - n[0] - n[1] // 2 - 5, H.LINE - n[1] // 2, H.LINE + n[1] + 3, H.LINE + (1 << 22) + 7]
    cap = [n[0], n[1], n[2] + 4, n[3] - 1]
    out_cap = H.BYTE_ARENA
    assert off[0] + n[0] < H.LINE and off[1] < H.LINE < off[1] + n[1] and off[2] > H.LINE
    P = torch.empty(H.BYTE_ARENA + 16, dtype=torch.uint8, device="cuda")
    windows = [(off[0] - H.GUARD, off[2] + cap[2] + H.GUARD), (off[3] - H.GUARD, off[3] + cap[3] + H.GUARD)]
    for a, b in windows:
        P[a:b] = SENTINEL
    segs = [s for m in msgs for s in m]
    d_in = torch.from_numpy(np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8).view(np.int64).copy()).cuda()
    d_swo = _dev64(H.rel_off([len(s) // 8 for s in segs]))
    d_mseg, d_off, d_cap = _dev64(H.rel_off([len(m) for m in msgs])), _dev64(off), _dev64(cap)
    np_ = len(msgs) + len(segs)
    d_poff = torch.full((np_,), -1, dtype=torch.int64, device="cuda")
    d_len = torch.full((len(msgs),), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(msgs),), 77, dtype=torch.int32, device="cuda")
    mctx.encode_messages_at(d_in, d_swo, d_mseg, MAXW, P, out_cap, d_off, d_cap, d_poff, d_len, d_st,
                            nm=len(msgs), nseg=len(segs))
    torch.cuda.synchronize()
    for a, b in windows:
        got = P[a:b].cpu().numpy()
        rel = [o - a for o in off]  # (slots outside the window fall outside the image)
        inside = [m for m in range(len(msgs)) if a <= off[m] < b]
        exp = M.expected(oracle, [msgs[m] for m in inside], [rel[m] for m in inside], [cap[m] for m in inside],
                         b - a, MAXW, b - a, SENTINEL)
        bad = np.nonzero((got != exp.image) & exp.care)[0]
        assert bad.size == 0, f"{bad.size} wrong bytes, the first at buffer byte {a + int(bad[0])}"
    del P
    assert d_st.cpu().tolist() == [OK, OK, OK, ENOMEM]
    assert d_len.cpu().tolist() == n
    want = []
    for m, msg in enumerate(msgs):
        o = off[m]
        for p in M.packed_pieces(oracle, msg):
            want.append(o)
            o += len(p)
    assert d_poff.cpu().tolist() == want and max(want) > H.LINE
