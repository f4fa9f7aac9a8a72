"""cpk_encode_batch_at: pieces packed to where the caller says (encode_at.hip,
sp_place_kernel in both forms).  The expected bytes always come from the
oracle (oracle.pack per piece, oracle.pack_batch, oracle.write_message), never
from another GPU call -- except in the size round trip, where equality with
cpk_encode_batch_cap is the thing asserted.  The output buffer is filled with a
sentinel and carries a sentinel pad after out_cap: every test asserts that
every byte outside the CPK_OK groups' packed bytes is still the sentinel, and
for a refused group that every byte outside its slot is.  Each context is
created here with CPK_AT_FORM unset, dense and sparse."""
import os

import numpy as np
import pytest

import _encoder_seams as es

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 4096  # sentinel bytes after out_cap
OK, EINVAL, ENOMEM = 0, -1, -5
CHUNK = 8192
# the step edge, one wave's 32 steps against the spread over four waves; the
# unit table, the chunk hand-over and the in-piece look-back at depths 1, 2, 3
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 16385, 3 * CHUNK + 1]
RAGGED = [8192] * 40 + [8191, 17, 4096, 0, 8192]  # test_gpu_capacity.py's ragged batch


@pytest.fixture(scope="module", params=[None, "dense", "sparse"], ids=["form-auto", "form-dense", "form-sparse"])
def actx(request):
    """A context per CPK_AT_FORM value (read at context creation)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = os.environ.get("CPK_AT_FORM")
    if request.param is None:
        os.environ.pop("CPK_AT_FORM", None)
    else:
        os.environ["CPK_AT_FORM"] = request.param
    try:
        c = cp.Context(0)
    finally:
        if saved is None:
            os.environ.pop("CPK_AT_FORM", None)
        else:
            os.environ["CPK_AT_FORM"] = saved
    try:
        yield c
    finally:
        c.close()


# ---- data -------------------------------------------------------------------------
def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _split(data, sizes):
    swo = _swo(sizes).astype(np.int64)
    b = np.ascontiguousarray(data, np.uint8).tobytes()
    return [b[8 * swo[i]:8 * swo[i + 1]] for i in range(len(sizes))]


_DATA = {}


def _pieces(oracle, kind, sizes):
    """Pieces of `sizes` words: kind 2 / 3 / 4 the generator's presets, "nz"
    all-nonzero words, "zero" all-zero words.  Built once per (kind, sizes)."""
    key = (kind, tuple(sizes))
    if key not in _DATA:
        if kind == "zero":
            data = np.zeros(8 * sum(sizes), np.uint8)
        elif kind == "nz":
            data = np.random.default_rng(11).integers(1, 256, size=8 * sum(sizes), dtype=np.uint8)
        else:
            data = oracle.generate(oracle.preset(kind), _swo(sizes))
        _DATA[key] = _split(data, sizes)
    return _DATA[key]


_PACKS = {}


def _pack(oracle, piece):
    """oracle.pack(piece), computed once per piece and left unchanged."""
    if piece not in _PACKS:
        _PACKS[piece] = oracle.pack(piece)
    return _PACKS[piece]


def _layout(oracle, pieces, groups, gap=lambda g: (5 * g + 3) % 16, room=lambda g: 0, start=5):
    """Slots in group order: each its packed bytes + room(g), gap(g) bytes
    between them.  -> (dst_off, dst_cap, out_cap)"""
    gs = groups if groups is not None else [1] * len(pieces)
    off, cap, cur, p = [], [], start, 0
    for g, k in enumerate(gs):
        n = sum(len(_pack(oracle, pieces[p + i])) for i in range(k))
        off.append(cur)
        cap.append(n + room(g))
        cur += n + room(g) + gap(g)
        p += k
    return off, cap, cur + 3


# ---- one call ---------------------------------------------------------------------
class Call:
    """The device arrays of one cpk_encode_batch_at call; launched by the
    constructor, read back (after a sync) by results()."""

    def __init__(self, ctx, pieces, groups, dst_off, dst_cap, out_cap, maxw, ng=None, misalign=0):
        import torch
        n = len(pieces)
        swo = _swo([len(p) // 8 for p in pieces])
        data = np.frombuffer(b"".join(pieces) + b"\0" * 8, np.uint8)
        self.d_in = torch.from_numpy(data.view(np.int64).copy()).cuda()
        self.d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
        self.d_grp = None if groups is None else torch.from_numpy(_swo(groups).astype(np.int64)).cuda()
        k = len(groups) if groups is not None else n
        dev64 = lambda v: torch.from_numpy(np.asarray(list(v) + [0], dtype=np.int64)).cuda()
        self.d_off = dev64(dst_off)
        self.d_cap = None if dst_cap is None else dev64(dst_cap)
        self.buf = torch.full((out_cap + PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.d_poff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_glen = torch.full((k + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((k + 1,), 77, dtype=torch.int32, device="cuda")
        self.n, self.k = n, k
        ctx.encode_batch_at(self.d_in, self.d_swo, maxw, self.d_grp, self.buf[misalign:], out_cap, self.d_off,
                            self.d_cap, self.d_poff, self.d_glen, self.d_st, ng=ng)

    def results(self):
        import torch
        torch.cuda.synchronize()
        return (self.buf.cpu().numpy(), self.d_poff.cpu().numpy()[:self.n], self.d_glen.cpu().numpy()[:self.k],
                self.d_st.cpu().numpy()[:self.k])


def _verify(call, oracle, pieces, groups, dst_off, dst_cap, out_cap, maxw):
    """Statuses, lengths, piece offsets and every byte of the buffer against
    the oracle."""
    buf, poff, glen, st = call.results()
    gs = groups if groups is not None else [1] * len(pieces)
    want = np.full(buf.size, SENTINEL, np.uint8)
    care = np.ones(buf.size, bool)
    p = 0
    for g, k in enumerate(gs):
        packs = [_pack(oracle, pieces[p + i]) for i in range(k)]
        body = b"".join(packs)
        d0 = dst_off[g]
        cap = dst_cap[g] if dst_cap is not None else out_cap - d0
        inval = bool(maxw) and any(len(pieces[p + i]) // 8 > maxw for i in range(k))
        refused = d0 > out_cap or d0 + cap > out_cap or len(body) > cap
        exp = EINVAL if inval else ENOMEM if refused else OK
        assert st[g] == exp, f"group {g}: status {st[g]}, expected {exp}"
        if not inval:
            assert glen[g] == len(body), f"group {g}: d_grp_len {glen[g]}, oracle {len(body)}"
            o = d0
            for i in range(k):
                assert poff[p + i] == o, f"piece {p + i} of group {g}: d_piece_off {poff[p + i]}, oracle {o}"
                o += len(packs[i])
        if exp == OK:
            want[d0:d0 + len(body)] = np.frombuffer(body, np.uint8)
        else:  # (the bytes inside a refused group's own slot are undefined)
            care[min(d0, out_cap):min(d0 + max(cap, 0), out_cap)] = False
        p += k
    assert p == len(pieces)
    bad = np.nonzero((buf != want) & care)[0]
    assert bad.size == 0, (f"{bad.size} wrong bytes, the first at {bad[0]} (out_cap {out_cap}): "
                           f"{buf[bad[0]]:#x}, expected {want[bad[0]]:#x}")


def _run(ctx, oracle, pieces, groups, dst_off, dst_cap, out_cap, maxw):
    _verify(Call(ctx, pieces, groups, dst_off, dst_cap, out_cap, maxw), oracle, pieces, groups, dst_off, dst_cap,
            out_cap, maxw)


# ---- 1. piece sizes ---------------------------------------------------------------
@pytest.mark.parametrize("kind", [2, 3, 4, "nz", "zero"])
def test_piece_sizes(actx, oracle, kind):
    """Every size, each piece its own group in a slot of its own: all-nonzero
    words overflow both rings (the drain path with the base known from the
    start)."""
    pieces = _pieces(oracle, kind, SIZES)
    off, cap, out_cap = _layout(oracle, pieces, None, room=lambda g: (g % 3) * 7)
    _run(actx, oracle, pieces, None, off, cap, out_cap, 3 * CHUNK + 1)
    # ... and back to back in one group: the look-back over every unit before
    off, cap, out_cap = _layout(oracle, pieces, [len(pieces)])
    _run(actx, oracle, pieces, [len(pieces)], off, cap, out_cap, 3 * CHUNK + 1)


# ---- 2. seams ---------------------------------------------------------------------
def _seam_pieces():
    """2-chunk pieces with a zero run or a literal run crossing word 8192."""
    out = []
    for kind in ("zero", "dense", "dense+L"):
        for before in (1, 128, 255, 256):
            for ln in (254, 255, 256, 257, 513):
                if ln <= before:
                    continue
                w = es.bg(2 * CHUNK)
                w[CHUNK - before:CHUNK - before + ln] = es.run_words(kind, ln, es._rng("at", kind, before, ln))
                out.append(np.ascontiguousarray(w, np.uint8).tobytes())
    return out


def test_seams_across_the_chunk_edge(actx, oracle):
    pieces = _seam_pieces()
    off, cap, out_cap = _layout(oracle, pieces, None, gap=lambda g: 3)
    _run(actx, oracle, pieces, None, off, cap, out_cap, 2 * CHUNK)


# ---- 3. alignment and neighbours --------------------------------------------------
def test_every_alignment(actx, oracle):
    piece = _pieces(oracle, 2, [65] * 16)
    off = [1024 * a + a for a in range(16)]
    cap = [len(_pack(oracle, p)) for p in piece]
    _run(actx, oracle, piece, None, off, cap, 16 * 1024, 65)


@pytest.mark.parametrize("gap", [0, 1, 15])
def test_neighbours_in_one_line(actx, oracle, gap):
    """Two groups whose bytes lie `gap` bytes apart, the first ending one byte
    into a 16-byte line: a line stored whole by either would cover the other's
    bytes or the sentinel between them."""
    a, b = _pieces(oracle, 3, [65, 2049])
    la = len(_pack(oracle, a))
    d0 = 32 + (1 - la) % 16
    for pieces, off in (([a, b], [d0, d0 + la + gap]), ([b, a], [d0 + la + gap, d0])):
        out_cap = d0 + la + gap + len(_pack(oracle, b)) + 7
        _run(actx, oracle, pieces, None, off, None if gap else [len(_pack(oracle, p)) for p in pieces], out_cap, 2049)


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_slot_order(actx, oracle, order):
    pieces = _pieces(oracle, 2, [300, 8192, 17, 0, 16385, 2048, 65, 1])
    off, cap, out_cap = _layout(oracle, pieces, None)
    idx = list(range(len(pieces)))[::-1] if order == "descending" else \
        list(np.random.default_rng(5).permutation(len(pieces)))
    # (piece i takes the slot laid out for piece idx[i]: the slots are sized anew)
    sizes = [len(_pack(oracle, p)) for p in pieces]
    slots, cur = {}, 9
    for j in idx:
        slots[j] = cur
        cur += sizes[j] + 5
    _run(actx, oracle, pieces, None, [slots[j] for j in range(len(pieces))], sizes, cur, 3 * CHUNK)


# ---- 4. groups ----------------------------------------------------------------------
GROUPS = [[], [65], [100, 2049], [0, 64, 0, 65, 0], [2048, 3 * CHUNK + 1, 63], [300, 17, 4096], []]


@pytest.mark.parametrize("cfg", [2, 3])
def test_groups(actx, oracle, cfg):
    """Groups of 0, 1, 2, 3 and 5 pieces, empty pieces at the front, middle
    and end, a 3-chunk piece in the middle, and one whole message (its table
    words first) against oracle.write_message."""
    sizes = [w for g in GROUPS for w in g]
    pieces = list(_pieces(oracle, cfg, sizes))
    groups = [len(g) for g in GROUPS]
    segs = list(_pieces(oracle, cfg, [17, CHUNK + 1, 0]))
    table = np.array([len(segs) - 1] + [len(s) // 8 for s in segs], dtype="<u4").tobytes()
    table += b"\0" * (-len(table) % 8)
    msg = [table] + segs
    assert b"".join(_pack(oracle, p) for p in msg) == oracle.write_message(segs)
    pieces[len(GROUPS[0]) + len(GROUPS[1]):len(GROUPS[0]) + len(GROUPS[1])] = msg  # (the message: group 2)
    groups.insert(2, len(msg))
    off, cap, out_cap = _layout(oracle, pieces, groups, room=lambda g: 11 * (g % 2))
    _run(actx, oracle, pieces, groups, off, cap, out_cap, 3 * CHUNK + 1)


# ---- 5. round trip of the size query ----------------------------------------------
@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_size_query_round_trip(actx, oracle, cfg):
    """size -> allocate exactly -> placed encode: cpk_packed_size_batch's
    offsets handed over as they stand, no d_dst_cap, out_cap the exact total;
    the buffer is cpk_encode_batch_cap's byte for byte, and the oracle's."""
    import torch
    import capnp_packed as cp
    swo = _swo(RAGGED)
    n = len(RAGGED)
    data = oracle.generate(oracle.preset(cfg), swo)
    want, woff = oracle.pack_batch(data, swo, threads=8)
    total = int(woff[-1])
    d_in = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)]).view(np.int64).copy()).cuda()
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    actx.packed_size_batch(d_in, d_swo, CHUNK, d_off)
    buf = torch.full((total + PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_poff = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_glen = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    actx.encode_batch_at(d_in, d_swo, CHUNK, None, buf, total, d_off, None, d_poff, d_glen, d_st)
    ref = torch.full((cp.batch_capacity(swo) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_off2 = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    actx.encode_batch_cap(d_in, d_swo, CHUNK, ref, total, d_off2)
    assert actx.take_error() == cp.OK
    got = buf.cpu().numpy()
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), woff)
    assert (d_st.cpu().numpy() == OK).all()
    assert np.array_equal(d_poff.cpu().numpy().astype(np.uint64), woff[:-1])
    assert np.array_equal(d_glen.cpu().numpy().astype(np.uint64), np.diff(woff))
    assert got[:total].tobytes() == np.asarray(want).tobytes()
    assert got[:total].tobytes() == ref.cpu().numpy()[:total].tobytes()
    assert (got[total:] == SENTINEL).all()


# ---- 6. capacity ----------------------------------------------------------------------
def test_capacity(actx, oracle):
    """An exact slot, a slot one byte short, half a slot for a 3-chunk piece
    (its later chunks store nothing past it), a roomy slot that ends one byte
    past out_cap; the other groups of the same call are the oracle's bytes."""
    pieces = _pieces(oracle, 2, [8192, 8192, 3 * CHUNK + 1, 65, 2049, 300])
    n = [len(_pack(oracle, p)) for p in pieces]
    cap = [n[0], n[1] - 1, n[2] // 2, n[3], n[4], n[5] + 100]
    off, cur = [], 7
    for c in cap:
        off.append(cur)
        cur += c + 9
    out_cap = off[5] + cap[5] - 1  # (the last slot ends one byte past it)
    _run(actx, oracle, pieces, None, off, cap, out_cap, 3 * CHUNK + 1)
    # a group of several units refused as a whole: the look-back's base + bytes
    groups = [2, 1, 3]
    cap = [n[0] + n[1] - 1, n[2], n[3] + n[4] + n[5]]
    off = [3, 3 + cap[0] + 16, 3 + cap[0] + 16 + cap[1] + 1]
    _run(actx, oracle, pieces, groups, off, cap, off[2] + cap[2], 3 * CHUNK + 1)


# ---- 7. argument checks -----------------------------------------------------------------
def test_piece_over_the_bound(actx, oracle):
    pieces = _pieces(oracle, 2, [64, 200, 100, 17])
    off, cap, out_cap = _layout(oracle, pieces, None)
    _run(actx, oracle, pieces, None, off, cap, out_cap, 100)
    groups = [1, 2, 1]  # (the group with the piece over the bound, and its neighbours)
    off, cap, out_cap = _layout(oracle, pieces, groups)
    _run(actx, oracle, pieces, groups, off, cap, out_cap, 100)


def test_no_bound_reads_the_extent_back(actx, oracle):
    pieces = _pieces(oracle, 3, [65, 9000, 0, 64])
    off, cap, out_cap = _layout(oracle, pieces, [1, 3])
    _run(actx, oracle, pieces, [1, 3], off, cap, out_cap, 0)


def test_empty_calls(actx, oracle):
    _run(actx, oracle, [], None, [], [], 64, 8192)     # n == 0 (and ng == 0)
    _run(actx, oracle, [], [], [], [], 64, 8192)       # ng == 0
    _run(actx, oracle, [], [0, 0], [3, 80], [0, 5], 64, 8192)  # groups without pieces: statuses and lengths written


def test_invalid_arguments(actx, oracle):
    import capnp_packed as cp
    pieces = _pieces(oracle, 2, [64, 65])
    off, cap, out_cap = _layout(oracle, pieces, None)
    with pytest.raises(cp.CodecError) as e:  # no groups given: ng must be n
        Call(actx, pieces, None, off + [0], cap + [0], out_cap, 65, ng=3)
    assert e.value.status == cp.EINVAL
    with pytest.raises(cp.CodecError) as e:  # d_out off its 16-byte line
        Call(actx, pieces, None, off, cap, out_cap, 65, misalign=1)
    assert e.value.status == cp.EINVAL
    _run(actx, oracle, pieces, None, off, cap, out_cap, 65)  # (the context is as good as before)


# ---- 8. two calls back to back ------------------------------------------------------------
def test_two_calls_back_to_back(actx, oracle):
    """One context, one stream, no sync between: the second call's look-back
    must not take the first call's status words for its own (the epoch)."""
    pieces = _pieces(oracle, 2, [8192] * 6 + [16385, 100, 3 * CHUNK + 1])
    calls = []
    for groups in ([3, 3, 1, 2], [1, 5, 3], [9]):
        off, cap, out_cap = _layout(oracle, pieces, groups)
        calls.append((Call(actx, pieces, groups, off, cap, out_cap, 3 * CHUNK + 1), groups, off, cap, out_cap))
    for call, groups, off, cap, out_cap in calls:
        _verify(call, oracle, pieces, groups, off, cap, out_cap, 3 * CHUNK + 1)
