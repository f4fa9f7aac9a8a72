"""cpk_decode_batch_at and cpk_unpacked_size_batch_at: pieces decoded from the
byte ranges the caller names (decode_at.hip).  The expected side is always the
oracle's (tests/_decode_at_cases.py: oracle.unpack per piece, the stream rule
per group, the range rules) -- except in the round trip, where equality with
the words given to cpk_encode_batch_at is the thing asserted.  Every call runs
on sentinel-filled outputs with a sentinel pad before word d_seg_word_off[0]
(word 3) and after the last, and on a packed buffer of exactly
round_up(in_cap, 16) bytes that is compared with a clone afterwards.  Each
context is created here with CPK_DECODER unset (the device's gate), 1 (block
map) and 2 (record index)."""
import os

import numpy as np
import pytest

import _decode_at_cases as D
import _high_offsets as H
import _packed_records as R
import _unpacked_size_model as M
from test_gpu_encode_at import RAGGED, SIZES, _pieces, _swo

pytestmark = pytest.mark.gpu

LEAD = 3           # d_seg_word_off[0]
PAD = 64           # sentinel words / entries after what a call may write
WORD_SENT = 0x5A5A5A5A5A5A5A5A
ST_SENT, USED_SENT = 77, -1
OK, EINVAL, ETRUNC, ETRAILING, EUNSUPPORTED = D.OK, D.EINVAL, D.ETRUNC, D.ETRAILING, D.EUNSUPPORTED


@pytest.fixture(scope="module", params=[None, "1", "2"], ids=["dec-auto", "dec-block-map", "dec-index"])
def dctx(request):
    """A context per CPK_DECODER value (read at context creation)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = os.environ.get("CPK_DECODER")
    if request.param is None:
        os.environ.pop("CPK_DECODER", None)
    else:
        os.environ["CPK_DECODER"] = request.param
    try:
        c = cp.Context(0)
    finally:
        if saved is None:
            os.environ.pop("CPK_DECODER", None)
        else:
            os.environ["CPK_DECODER"] = saved
    try:
        yield c
    finally:
        c.close()


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    _sizes.clear()
    R.release()


def _dev64(v):
    import torch
    return torch.from_numpy(np.asarray(list(v) + [0], dtype=np.uint64).view(np.int64).copy()).cuda()


def _packed_dev(buf, in_cap):
    """The packed buffer on the device: exactly round_up(in_cap, 16) bytes."""
    import torch
    size = (in_cap + 15) // 16 * 16
    host = np.full(max(size, 16), 0xFF, np.uint8)
    host[:len(buf)] = buf[:size]
    return torch.from_numpy(host).cuda()


class Call:
    """One cpk_decode_batch_at call on sentinel-filled outputs; results() syncs,
    checks every sentinel outside what the call may write and that d_packed is
    unchanged, and returns (words uint8, piece statuses, group statuses, used)."""

    def __init__(self, ctx, buf, in_cap, src_off, src_len, words, groups=None, d_pk=None):
        import torch
        self.n, self.total = len(words), int(sum(words))
        self.ng = len(groups) if groups is not None else self.n
        self.d_pk = _packed_dev(buf, in_cap) if d_pk is None else d_pk
        self.clone = self.d_pk.clone() if d_pk is None else None
        swo = LEAD + _swo(words)
        self.d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
        self.d_grp = None if groups is None else torch.from_numpy(_swo(groups).astype(np.int64)).cuda()
        self.d_off, self.d_len = _dev64(src_off), _dev64(src_len)
        self.d_out = torch.full((LEAD + self.total + PAD,), WORD_SENT, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((self.n + PAD,), ST_SENT, dtype=torch.int32, device="cuda")
        self.d_gst = torch.full((self.ng + PAD,), ST_SENT, dtype=torch.int32, device="cuda")
        self.d_used = torch.full((self.ng + PAD,), USED_SENT, dtype=torch.int64, device="cuda")
        ctx.decode_batch_at(self.d_pk, in_cap, self.d_off, self.d_len, self.d_grp, self.d_swo, self.d_out, self.d_st,
                            self.d_gst, self.d_used, ng=self.ng)

    def results(self):
        import torch
        torch.cuda.synchronize()
        out, st = self.d_out.cpu().numpy(), self.d_st.cpu().numpy()
        gst, used = self.d_gst.cpu().numpy(), self.d_used.cpu().numpy()
        assert (out[:LEAD] == WORD_SENT).all() and (out[LEAD + self.total:] == WORD_SENT).all()
        assert (st[self.n:] == ST_SENT).all() and (gst[self.ng:] == ST_SENT).all()
        assert (used[self.ng:] == USED_SENT).all()
        if self.clone is not None:
            assert torch.equal(self.d_pk, self.clone), "d_packed was written"
        return (out[LEAD:LEAD + self.total].view(np.uint8), st[:self.n], gst[:self.ng],
                used[:self.ng].view(np.uint64))


def _check(res, words, names, pst, pout, gst, used):
    """Statuses, group statuses and consumed bytes equal to the model's, and
    the words of every piece it accepts."""
    got, st, g, u = res
    bad = [f"{nm}: status {int(s)}, expected {int(o)}" for nm, s, o in zip(names, st, pst) if s != o]
    assert not bad, (len(bad), bad[:8])
    assert np.array_equal(g, gst), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(g, gst)) if a != b][:8]
    assert np.array_equal(u, used), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(u, used)) if a != b][:8]
    swo = _swo(words).astype(np.int64)
    for i, nm in enumerate(names):
        if pst[i] == OK and got[8 * swo[i]:8 * swo[i + 1]].tobytes() != pout[i]:
            bad.append(nm)
    assert not bad, (len(bad), bad[:8])


def _sentinel_words(res, words, which):
    got = res[0].view(np.uint64)
    swo = _swo(words).astype(np.int64)
    for i in which:
        assert (got[swo[i]:swo[i + 1]] == WORD_SENT).all(), f"piece {i}: words written"


def _corpus_model(oracle, name):
    if name not in _cache:
        cases = R.corpora()[name]
        _cache[name] = D.batch_model(oracle, [c.packed for c in cases], [[c.nwords] for c in cases])
    return _cache[name]


# ---- pieces of their own ------------------------------------------------------------
@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_corpora_placed(dctx, oracle, name):
    """Every corpus -- the window, round, block and serial-walk edges, the
    malformed cases -- forward, reversed and shuffled, in each filler."""
    cases = R.corpora()[name]
    items, words, names = [c.packed for c in cases], [c.nwords for c in cases], [c.name for c in cases]
    model = _corpus_model(oracle, name)
    calls = []
    for order in D.ORDERS:
        for filler in D.FILLERS:
            off, ln, in_cap, buf = D.place(items, order, filler=filler)
            calls.append(Call(dctx, buf, in_cap, off, ln, words))
    for c in calls:
        _check(c.results(), words, names, *model)


def test_alignment_sweep(dctx, oracle):
    """A piece of about kWin + LONGEST bytes and one of 1 byte (a zero run cut
    to its tag), the start at every byte of a 16-byte line and the end at
    every byte of one, 0xFF on both sides: P limits the parse at every phase."""
    big = R.filled(R.kWin + R.LONGEST, "mid", seed=3).packed
    cut = R.built([R.Z(3)]).packed[:1]
    ends = [q for q in _record_ends(big) if q >= R.kWin]
    items, words, phases = [], [], []
    for s in range(16):
        # start phase s; the end phases a permutation of the 16 (this filling's
        # records all have even lengths, so the end keeps the start's parity)
        e = next(q for q in ends if q % 16 == 2 * ((5 * s + 1) % 8))
        items += [big[:e], cut]
        words += [M.unpacked_size(big[:e])[1], 4]
        phases += [s, (s + 9) % 16]
    gaps = _phase_gaps(items, phases)
    off, ln, in_cap, buf = D.place(items, "forward", gap=lambda k: gaps[k], filler="ff")
    assert [int(o) % 16 for o in off[0::2]] == list(range(16))
    assert {int(o + l) % 16 for o, l in zip(off[0::2], ln[0::2])} == set(range(16))
    model = D.batch_model(oracle, items, [[w] for w in words])
    assert list(model[0][0::2]) == [OK] * 16 and list(model[0][1::2]) == [ETRUNC] * 16
    res = Call(dctx, buf, in_cap, off, ln, words).results()
    _check(res, words, [f"piece{i}" for i in range(len(items))], *model)
    _sentinel_words(res, words, range(1, len(items), 2))


def _record_ends(packed):
    out, q = [], 0
    while q < len(packed):
        n, _ = M.record_at(packed, q)
        q += n
        out.append(q)
    return out


def _phase_gaps(items, phases):
    """Gaps (>= 1 byte of filler) that start item k at phase phases[k] of a 16-byte line."""
    gaps, cur = [], 0
    for b, p in zip(items, phases):
        g = (p - cur - 1) % 16 + 1
        gaps.append(g)
        cur += g + len(b)
    return gaps


# ---- groups --------------------------------------------------------------------------
def _group_case(oracle):
    """Groups of 1, 2 and 5 pieces with empty pieces first, in the middle and
    last; trailing bytes of 1 byte and of a whole window; a failing second
    piece followed by a good group; an empty group."""
    sizes = [300, 0, 17, 2000, 64, 0, 4095, 65, 0, 1000, 0, 8, 500, 600, 700, 33, 129]
    pcs = _pieces(oracle, 2, sizes)
    pk = [oracle.pack(p) for p in pcs]
    groups = [[0], [1, 2], [3, 4, 5, 6, 7], [8, 9, 10], [11], [12, 13, 14], [], [15], [16]]
    streams = [b"".join(pk[i] for i in g) for g in groups]
    streams[3] += b"\x00"                                  # 1 byte outlasts the pieces
    streams[4] += R.filled(R.kWin, "mid", seed=9).packed   # a whole window does
    cutat = len(pk[12]) + len(pk[13]) // 2                 # the second piece of group 5 fails
    streams[5] = streams[5][:cutat]
    words = [[sizes[i] for i in g] for g in groups]
    return streams, words, pcs, groups


@pytest.mark.parametrize("order", D.ORDERS)
def test_group_rules(dctx, oracle, order):
    streams, gw, pcs, groups = _group_case(oracle)
    pst, pout, gst, used = D.batch_model(oracle, streams, gw)
    assert list(gst) == [OK, OK, OK, ETRAILING, ETRAILING, ETRUNC, OK, OK, OK]
    assert int(used[3]) == len(streams[3]) - 1 and int(used[4]) == len(streams[4]) - R.kWin and used[6] == 0
    flat = [w for g in gw for w in g]
    assert list(pst[12:15]) == [OK, ETRUNC, ETRUNC] and pst[11] == ETRAILING
    off, ln, in_cap, buf = D.place(streams, order, filler="00ff")
    c = Call(dctx, buf, in_cap, off, ln, flat, groups=[len(g) for g in gw])
    _check(c.results(), flat, [f"piece{i}" for i in range(len(flat))], pst, pout, gst, used)


@pytest.mark.parametrize("kind", [2, 4, "zero", "nz"])
@pytest.mark.parametrize("shape", ["sizes", "ragged"])
@pytest.mark.parametrize("grouped", [False, True], ids=["pieces", "groups"])
def test_round_trip(dctx, oracle, kind, shape, grouped):
    """cpk_encode_batch_at into reversed slots with gaps, then
    cpk_decode_batch_at with the arrays that call wrote: the words come back
    and every status is CPK_OK."""
    import torch
    sizes = SIZES if shape == "sizes" else RAGGED
    pcs = _pieces(oracle, kind, sizes)
    n = len(pcs)
    groups = None
    if grouped:
        groups, left = [], n
        while left:
            groups.append(min(left, (1, 2, 5)[len(groups) % 3]))
            left -= groups[-1]
    ng = len(groups) if grouped else n
    gsz = np.add.reduceat(np.array([10 * s + 16 for s in sizes]), _swo(groups)[:-1].astype(np.int64)) if grouped \
        else np.array([10 * s + 16 for s in sizes])
    # reversed slots, a gap of 4 to 19 bytes before each
    dst, cur = np.zeros(ng, np.uint64), 0
    for g in range(ng - 1, -1, -1):
        cur += 4 + (5 * g) % 16
        dst[g] = cur
        cur += int(gsz[g])
    out_cap = cur + 7
    data = np.frombuffer(b"".join(pcs) + b"\0" * 8, np.uint8)
    d_in = torch.from_numpy(data.view(np.int64).copy()).cuda()
    d_swo = torch.from_numpy(_swo(sizes).astype(np.int64)).cuda()
    d_grp = None if not grouped else torch.from_numpy(_swo(groups).astype(np.int64)).cuda()
    d_dst, d_cap = _dev64(dst), _dev64(gsz)
    d_buf = torch.full(((out_cap + 15) // 16 * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_glen = torch.zeros(ng + 1, dtype=torch.int64, device="cuda")
    d_est = torch.full((ng + 1,), ST_SENT, dtype=torch.int32, device="cuda")
    dctx.encode_batch_at(d_in, d_swo, max(sizes), d_grp, d_buf, out_cap, d_dst, d_cap, d_poff, d_glen, d_est, ng=ng)
    d_out = torch.full((sum(sizes) + PAD,), WORD_SENT, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), ST_SENT, dtype=torch.int32, device="cuda")
    d_gst = torch.full((ng,), ST_SENT, dtype=torch.int32, device="cuda")
    d_used = torch.full((ng,), USED_SENT, dtype=torch.int64, device="cuda")
    dctx.decode_batch_at(d_buf, out_cap, d_dst, d_glen, d_grp, d_swo, d_out, d_st, d_gst, d_used, ng=ng)
    torch.cuda.synchronize()
    assert (d_est[:ng] == OK).all()
    assert (d_st == OK).all() and (d_gst == OK).all()
    assert torch.equal(d_used, d_glen[:ng])
    assert torch.equal(d_out[:sum(sizes)], d_in[:sum(sizes)])
    assert (d_out[sum(sizes):] == WORD_SENT).all()


# ---- ranges --------------------------------------------------------------------------
def test_ranges(dctx, oracle):
    """Ranges at and past in_cap, overflowing sums, a length of 2^32, empty
    ranges with and without words, two pieces over one range."""
    a = bytes(range(1, 41))
    pa = oracle.pack(a)
    filler = b"\xff" * 7
    buf = np.frombuffer(filler + pa, np.uint8)  # the last range ends at in_cap, in_cap % 16 != 0
    in_cap = len(buf)
    assert in_cap % 16 != 0
    s = len(filler)
    off = [s, s + 1, 2**64 - 8, 0, 3, 3, s, s, in_cap + 1, in_cap]
    ln = [len(pa), len(pa), 16, 2**32, 0, 0, len(pa), len(pa), 0, 0]
    words = [5, 5, 5, 5, 0, 5, 5, 5, 0, 0]
    want = [OK, EINVAL, EINVAL, EUNSUPPORTED, OK, ETRUNC, OK, OK, EINVAL, OK]
    assert [D.range_status(o, l, in_cap) for o, l in zip(off, ln)] == \
        [OK, EINVAL, EINVAL, EUNSUPPORTED, OK, OK, OK, OK, EINVAL, OK]
    c = Call(dctx, buf, in_cap, off, ln, words)
    res = c.results()
    got, st, gst, used = res
    assert list(st) == want and list(gst) == want
    assert list(used) == [len(pa), 0, 0, 0, 0, 0, len(pa), len(pa), 0, 0]
    swo = _swo(words).astype(np.int64)
    for i in (0, 6, 7):
        assert got[8 * swo[i]:8 * swo[i + 1]].tobytes() == a
    _sentinel_words(res, words, [1, 2, 3, 5])


def test_calling_rules(dctx, oracle):
    import torch
    pa = oracle.pack(bytes(range(1, 41)))
    buf = np.frombuffer(pa, np.uint8)
    # n == 0 and ng == 0
    dctx.decode_batch_at(None, 0, None, None, None, None, None, None, None, None)
    c = Call(dctx, buf, len(pa), [0, 0], [len(pa), 0], [], groups=[0, 0])
    got, st, gst, used = c.results()
    assert list(gst) == [ETRAILING, OK] and list(used) == [0, 0]
    import capnp_packed as cp
    good = Call(dctx, buf, len(pa), [0], [len(pa)], [5])
    assert list(good.results()[1]) == [OK]
    # ng != n without groups
    with pytest.raises(cp.CodecError) as e:
        dctx.decode_batch_at(good.d_pk, len(pa), good.d_off, good.d_len, None, good.d_swo, good.d_out, good.d_st,
                             good.d_gst, good.d_used, ng=2)
    assert e.value.status == EINVAL
    # misaligned d_packed / d_out
    for bad_pk, bad_out in ((True, False), (False, True)):
        d_out = torch.full((16,), WORD_SENT, dtype=torch.int64, device="cuda")
        with pytest.raises(cp.CodecError) as e:
            # (the binding passes data_ptr(): offset by hand)
            rc = dctx._lib.cpk_decode_batch_at(
                dctx.handle, good.d_pk.data_ptr() + (1 if bad_pk else 0), len(pa), good.d_off.data_ptr(),
                good.d_len.data_ptr(), None, 1, good.d_swo.data_ptr(), 1, d_out.data_ptr() + (4 if bad_out else 0),
                good.d_st.data_ptr(), good.d_gst.data_ptr(), good.d_used.data_ptr(), None)
            cp._check(rc, "cpk_decode_batch_at")
        assert e.value.status == EINVAL
        torch.cuda.synchronize()
        assert (d_out == WORD_SENT).all()


# ---- the size query ------------------------------------------------------------------
_sizes = {}


def _corpus_sizes(name):
    """(statuses, words) of a corpus's pieces from tests/_unpacked_size_model.py, once."""
    if name not in _sizes:
        sized = [M.unpacked_size(c.packed) for c in R.corpora()[name]]
        _sizes[name] = ([int(s) for s, _ in sized], [int(w) for _, w in sized])
    return _sizes[name]


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_size_query_then_decode(dctx, oracle, name):
    """cpk_unpacked_size_batch_at against the model on every placed corpus
    (plus a refused range of each kind), forward, reversed and shuffled, each
    with a filler of its own; its offsets handed straight on: good pieces
    CPK_OK, the others CPK_ETRAILING with nothing written."""
    import torch
    cases = R.corpora()[name]
    items = [c.packed for c in cases]
    n = len(items) + 2
    mst, mwords = _corpus_sizes(name)
    wst, wwords = mst + [EINVAL, EUNSUPPORTED], mwords + [0, 0]
    pout = None
    for order, filler in zip(D.ORDERS, D.FILLERS):
        off, ln, in_cap, buf = D.place(items, order, filler=filler)
        off = np.concatenate([off, np.array([in_cap - 2, 0], np.uint64)])
        ln = np.concatenate([ln, np.array([3, 2**32], np.uint64)])
        d_pk = _packed_dev(buf, in_cap)
        clone = d_pk.clone()
        d_off, d_len = _dev64(off), _dev64(ln)
        d_swo = torch.full((n + 1 + PAD,), USED_SENT, dtype=torch.int64, device="cuda")
        d_st = torch.full((n + PAD,), ST_SENT, dtype=torch.int32, device="cuda")
        dctx.unpacked_size_batch_at(d_pk, in_cap, d_off, d_len, d_swo[:n + 1], d_st)
        torch.cuda.synchronize()
        swo, st = d_swo.cpu().numpy(), d_st.cpu().numpy()
        bad = [f"{c.name}: status {int(s)}, expected {o}" for c, s, o in zip(cases, st, wst) if s != o]
        assert not bad, (order, len(bad), bad[:8])
        assert list(st[:n]) == wst
        assert list(np.diff(swo[:n + 1])) == wwords and swo[0] == 0
        assert (swo[n + 1:] == USED_SENT).all() and (st[n:] == ST_SENT).all()
        total = int(swo[n])
        d_out = torch.full((total + PAD,), WORD_SENT, dtype=torch.int64, device="cuda")
        d_dst = torch.full((n,), ST_SENT, dtype=torch.int32, device="cuda")
        d_gst = torch.full((n,), ST_SENT, dtype=torch.int32, device="cuda")
        d_used = torch.full((n,), USED_SENT, dtype=torch.int64, device="cuda")
        dctx.decode_batch_at(d_pk, in_cap, d_off, d_len, None, d_swo[:n + 1], d_out, d_dst, d_gst, d_used)
        torch.cuda.synchronize()
        assert torch.equal(d_pk, clone)
        # (an empty range that sized to 0 words is CPK_OK)
        want = [s if s in (OK, EINVAL, EUNSUPPORTED) else (OK if int(l) == 0 else ETRAILING)
                for s, l in zip(wst, ln)]
        assert list(d_dst.cpu().numpy()) == want and list(d_gst.cpu().numpy()) == want
        got = d_out.cpu().numpy()
        assert (got[total:] == WORD_SENT).all()
        if pout is None:
            pout = D.batch_model(oracle, items, [[w] for w in mwords])[1]
        for i, c in enumerate(cases):
            if want[i] == OK:
                assert got[int(swo[i]):int(swo[i + 1])].tobytes() == pout[i], (order, c.name)


# ---- offsets above and across 4 GiB --------------------------------------------------
@pytest.mark.parametrize("where", ["above5", "straddle"])
def test_high_offsets(dctx, oracle, where):
    import torch
    sizes = H.MORE
    pcs = _pieces(oracle, 2, sizes)
    pk = [oracle.pack(p) for p in pcs]
    lay = H.place_bytes([len(b) for b in pk], where)
    lay.check()
    in_cap = lay.hi + 3
    try:
        d_pk = torch.empty((in_cap + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    except RuntimeError:
        free, total = torch.cuda.mem_get_info()
        pytest.skip(f"{in_cap >> 20} MiB of device memory cannot be allocated: {free >> 20} of {total >> 20} MiB free")
    lo = lay.lo - 64
    d_pk[lo:] = 0xFF
    for o, b in zip(lay.off[:-1], pk):
        d_pk[int(o):int(o) + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    edge = d_pk[lo:].clone()
    c = Call(dctx, None, in_cap, [int(o) for o in lay.off[:-1]], [len(b) for b in pk], sizes, d_pk=d_pk)
    got, st, gst, used = c.results()
    assert list(st) == [OK] * len(pk) and list(gst) == [OK] * len(pk)
    assert list(used) == [len(b) for b in pk]
    assert got.tobytes() == b"".join(pcs)
    assert torch.equal(d_pk[lo:], edge)
    del d_pk, c, edge
    torch.cuda.empty_cache()
