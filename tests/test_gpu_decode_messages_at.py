"""cpk_decode_messages_at: packed messages decoded from the byte ranges the
caller names, tables read and capacities judged on the device
(csrc/decode_msg_at.hip).  The expected side is tests/_messages_at_model.py --
oracle.read_message on each slot's bytes, the range rules, the fit rule --
except in the parity test, where cpk_decode_messages on the same messages
tiled is the reference, and the round trip, where equality with the words
given to cpk_encode_batch_at is the thing asserted.  Every call runs on
sentinel-filled outputs with sentinels before and after what the call may
write, and on a packed buffer of exactly round_up(in_cap, 16) bytes that is
compared with a clone afterwards."""
import os

import numpy as np
import pytest

import _decode_at_cases as D
import _message_frames as mf
import _messages_at_model as M

pytestmark = pytest.mark.gpu

PAD = 64           # sentinel words / entries on each side of what a call may write
WORD_SENT = 0x5A5A5A5A5A5A5A5A
ST_SENT = 77
OK, EINVAL, ETRUNC, ETRAILING, ENOMEM, EFRAME, EUNSUPPORTED = M.OK, M.EINVAL, M.ETRUNC, M.ETRAILING, M.ENOMEM, \
    M.EFRAME, M.EUNSUPPORTED


def _new_context(decoder=None):
    """A context created with CPK_DECODER unset (the device's gate), "1"
    (block map) or "2" (record index); the variable is read at creation."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = os.environ.get("CPK_DECODER")
    if decoder is None:
        os.environ.pop("CPK_DECODER", None)
    else:
        os.environ["CPK_DECODER"] = decoder
    try:
        return cp.Context(0)
    finally:
        if saved is None:
            os.environ.pop("CPK_DECODER", None)
        else:
            os.environ["CPK_DECODER"] = saved


@pytest.fixture(scope="module")
def mctx():
    c = _new_context()
    try:
        yield c
    finally:
        c.close()


def _dev64(v):
    import torch
    return torch.from_numpy(np.asarray(list(v) + [0], dtype=np.uint64).view(np.int64).copy()).cuda()


def _packed_dev(buf, in_cap):
    """The packed buffer on the device: exactly round_up(in_cap, 16) bytes."""
    import torch
    size = (in_cap + 15) // 16 * 16
    host = np.full(max(size, 16), 0xFF, np.uint8)
    host[:min(len(buf), size)] = buf[:size]
    return torch.from_numpy(host).cuda()


def _guard64(n):
    import torch
    base = torch.full((PAD + n + PAD,), WORD_SENT, dtype=torch.int64, device="cuda")
    return base, base[PAD:PAD + n]


def _guard32(n):
    import torch
    base = torch.full((PAD + n + PAD,), ST_SENT, dtype=torch.int32, device="cuda")
    return base, base[PAD:PAD + n]


def _clean(base, lo, hi=None):
    """The sentinels of a guarded tensor outside [lo, hi) of its inner part (checked on the device)."""
    sent = WORD_SENT if base.element_size() == 8 else ST_SENT
    inner_end = base.numel() - PAD if hi is None else PAD + hi
    return bool((base[:PAD + lo] == sent).all()) and bool((base[inner_end:] == sent).all())


class Call:
    """One cpk_decode_messages_at call.  sizing: d_out and the segment arrays
    NULL, capacities 0.  Otherwise out_cap words and seg_cap entries exactly,
    guarded on both sides."""

    def __init__(self, ctx, buf, in_cap, off, ln, limit=mf.LIMIT, out_cap=0, seg_cap=0, sizing=False, d_pk=None):
        self.nm, self.out_cap, self.seg_cap, self.sizing = len(off), out_cap, seg_cap, sizing
        self.d_pk = _packed_dev(buf, in_cap) if d_pk is None else d_pk
        self.clone = self.d_pk.clone()
        self.d_off, self.d_len = _dev64(off), _dev64(ln)
        self.b_mseg, self.d_mseg = _guard64(self.nm + 1)
        self.b_used, self.d_used = _guard64(self.nm)
        self.b_tot, self.d_tot = _guard64(3)
        self.b_mst, self.d_mst = _guard32(self.nm)
        if sizing:
            self.d_out = self.d_swo = self.d_sin = self.d_sst = None
        else:
            self.b_out, self.d_out = _guard64(out_cap)
            self.b_swo, self.d_swo = _guard64(seg_cap + 1)
            self.b_sin, self.d_sin = _guard64(seg_cap)
            self.b_sst, self.d_sst = _guard32(seg_cap)
        ctx.decode_messages_at(self.d_pk, in_cap, self.d_off, self.d_len, self.d_out, self.d_swo, self.d_sin,
                               self.d_sst, self.d_mseg, self.d_mst, self.d_used, self.d_tot,
                               traversal_limit_words=limit, nm=self.nm, out_cap_words=out_cap, seg_cap=seg_cap)

    def results(self):
        """Syncs; the sentinels around every array and d_packed unchanged.
        -> (msg status, used, msg_seg_off, totals)"""
        import torch
        torch.cuda.synchronize()
        for b in (self.b_mseg, self.b_used, self.b_tot, self.b_mst):
            assert _clean(b, 0)
        assert torch.equal(self.d_pk, self.clone), "d_packed was written"
        self.mst, self.used = self.d_mst.cpu().numpy(), self.d_used.cpu().numpy().view(np.uint64)
        self.mseg, self.tot = [int(v) for v in self.d_mseg.cpu().numpy()], tuple(int(v) for v in self.d_tot.cpu().numpy())
        return self.mst, self.used, self.mseg, self.tot

    def check(self, model, buf, names=None, unpack_segments=True):
        """Everything the model says, and that nothing beyond F and the fitting words is written."""
        import oracle
        mst, used, mseg, tot = self.results()
        names = names or [f"message{i}" for i in range(self.nm)]
        bad = [f"{n}: status {int(s)}, expected {int(o)}" for n, s, o in zip(names, mst, model.status) if s != o]
        assert not bad, (len(bad), bad[:8])
        assert np.array_equal(used, model.used), [(names[i], int(a), int(b)) for i, (a, b) in
                                                  enumerate(zip(used, model.used)) if a != b][:8]
        assert mseg == model.mseg and tot == model.totals and mseg[self.nm] == tot[1]
        if self.sizing:
            assert model.F == 0
            return
        F, fw = model.F, model.swo[model.F]
        assert F <= self.seg_cap and fw <= self.out_cap
        assert _clean(self.b_swo, 0, F + 1) and _clean(self.b_sin, 0, F) and _clean(self.b_sst, 0, F)
        assert _clean(self.b_out, 0, fw), "words past the fitting messages' were written"
        swo, sin, sst = (t.cpu().numpy() for t in (self.d_swo[:F + 1], self.d_sin[:F], self.d_sst[:F]))
        assert [int(v) for v in swo] == model.swo
        off, ln = self.d_off.cpu().numpy().view(np.uint64), self.d_len.cpu().numpy().view(np.uint64)
        for i, name in enumerate(names):
            if not model.fits[i]:
                continue
            a, b = mseg[i], mseg[i + 1]
            if model.status[i] not in (OK, ETRAILING):
                # (a failed segment stops its message: the last one carries its status)
                assert sst[b - 1] == model.status[i], name
                continue
            assert (sst[a:b] == OK).all(), name
            w0, w1 = int(swo[a]), int(swo[b])
            out = self.d_out[w0:w1].cpu().numpy().view(np.uint8) if w1 > w0 else np.zeros(0, np.uint8)
            got = [out[8 * (int(swo[j]) - w0):8 * (int(swo[j + 1]) - w0)].tobytes() for j in range(a, b)]
            assert got == list(model.segs[i]), name
            # d_seg_in_off: absolute, in order, inside the bytes consumed; the segment unpacks from there
            lo, hi = int(off[i]), int(off[i]) + int(used[i])
            pos = [int(v) for v in sin[a:b]]
            assert pos == sorted(pos) and lo < pos[0] and pos[-1] <= hi, name
            if unpack_segments:
                for j, p in zip(range(a, b), pos):
                    n = 8 * (int(swo[j + 1]) - int(swo[j]))
                    if n:
                        assert oracle.unpack(bytes(buf[p:hi]), n)[:2] == (OK, model.segs[i][j - a]), (name, j - a)


def _sized(ctx, buf, in_cap, off, ln, limit=mf.LIMIT, names=None, **kw):
    """A sizing call with NULL arrays, then the real call with what it said."""
    s = Call(ctx, buf, in_cap, off, ln, limit, sizing=True)
    s.check(M.batch(buf, off, ln, in_cap, limit, 0, 0), buf, names)
    W, S, fitting = s.tot
    assert fitting == 0
    c = Call(ctx, buf, in_cap, off, ln, limit, out_cap=W, seg_cap=S, d_pk=s.d_pk)
    model = M.batch(buf, off, ln, in_cap, limit, W, S)
    assert model.totals[2] == sum(model.fits) == sum(1 for z in model.sizes if z)  # (everything accepted fits)
    c.check(model, buf, names, **kw)
    return c, model


# ---- 1: the framing corpus, placed ---------------------------------------------------
def _by_limit():
    groups = {}
    for n in mf.NAMES:
        groups.setdefault(mf.corpus()[n].limit, []).append(n)
    return groups


@pytest.mark.parametrize("order,filler", [(o, "ff") for o in D.ORDERS] + [("forward", "00ff"), ("forward", "ff8ff")])
def test_framing_corpus_placed(mctx, oracle, order, filler):
    for limit, names in _by_limit().items():
        cases = [mf.corpus()[n] for n in names]
        off, ln, in_cap, buf = D.place([c.packed for c in cases], order, filler=filler)
        c, model = _sized(mctx, buf, in_cap, off, ln, limit, names)
        for i, case in enumerate(cases):
            assert c.mseg[i + 1] - c.mseg[i] == case.tseg, case.name
            st, segs, used = oracle.read_message(case.packed, limit, out_cap=mf.oracle_cap(case))
            want = ETRAILING if st == OK and used != len(case.packed) else st
            assert c.mst[i] == want, (case.name, int(c.mst[i]), want)
            assert c.used[i] == (used if want in (OK, ETRAILING) else 0), case.name
        del c
        import torch
        torch.cuda.empty_cache()


# ---- 2: range refusals among good messages ---------------------------------------------
def _good_messages(oracle, n, seed=5):
    """n good messages of 1-5 segments of 0-40 words (generator preset 2)."""
    rng = np.random.default_rng(seed)
    counts = [1 + int(rng.integers(0, 5)) for _ in range(n)]
    sizes = [int(rng.integers(0, 41)) for _ in range(sum(counts))]
    data = oracle.generate(oracle.preset(2), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)).tobytes()
    msgs, s, w = [], 0, 0
    for c in counts:
        segs = []
        for z in sizes[s:s + c]:
            segs.append(data[8 * w:8 * (w + z)])
            w += z
        s += c
        msgs.append(segs)
    return msgs


def test_range_refusals(mctx, oracle):
    msgs = _good_messages(oracle, 6)
    off, ln, in_cap, buf = D.place([oracle.write_message(m) for m in msgs], "shuffled")
    bad_off = [in_cap + 1, in_cap - 1, 2**64 - 1, 0]
    bad_len = [0, 2, 2, 2**32]
    # the refused ranges between the good ones
    o2, l2, where = [], [], []
    for i in range(6):
        o2.append(int(off[i]))
        l2.append(int(ln[i]))
        if i < 4:
            where.append(len(o2))
            o2.append(bad_off[i])
            l2.append(bad_len[i])
    c, model = _sized(mctx, buf, in_cap, o2, l2)
    assert [int(c.mst[w]) for w in where] == [EINVAL, EINVAL, EINVAL, EUNSUPPORTED]
    for w in where:
        assert c.mseg[w + 1] == c.mseg[w] and c.used[w] == 0
    good = [i for i in range(len(o2)) if i not in where]
    assert [int(c.mst[i]) for i in good] == [OK] * 6 and c.tot[2] == 6
    assert [list(model.segs[i]) for i in good] == msgs


# ---- 3: capacity ----------------------------------------------------------------------
def test_capacity(mctx, oracle):
    msgs = _good_messages(oracle, 20, seed=8)
    items = [oracle.write_message(m) for m in msgs]
    items[9] = mf.corpus()["neg/segment-1"].packed  # a failed table in the middle
    off, ln, in_cap, buf = D.place(items, "reversed", filler="00ff")
    d_pk = _packed_dev(buf, in_cap)
    full = M.batch(buf, off, ln, in_cap, mf.LIMIT, 1 << 62, 1 << 62)
    W, S, A = full.totals
    assert A == 19 and full.status[9] == EFRAME and full.mseg[10] == full.mseg[9]
    acc = [i for i in range(20) if i != 9]
    mid = acc[10]
    cuts = {"exact": (W, S, 19), "a word short": (W - 1, S, 18), "a segment short": (W, S - 1, 18),
            "words cut in the middle": (full.swo[full.mseg[mid + 1]] - 1, S, 10),
            "segments cut in the middle": (W, full.mseg[mid + 1] - 1, 10),
            "no words": (0, S, None), "one segment": (W, 1, None)}
    assert all(sum(len(s) for s in msgs[i]) > 0 for i in (19, mid))  # (the messages cut off need words)
    for what, (ow, sc, fitting) in cuts.items():
        c = Call(mctx, buf, in_cap, off, ln, out_cap=ow, seg_cap=sc, d_pk=d_pk)
        model = M.batch(buf, off, ln, in_cap, mf.LIMIT, ow, sc)
        c.check(model, buf)
        assert c.tot[:2] == (W, S) and c.mseg[20] == S, what
        if fitting is not None:
            assert c.tot[2] == fitting, what
            assert [int(s) for s in c.mst] == [EFRAME if i == 9 else (OK if i in acc[:fitting] else ENOMEM)
                                               for i in range(20)], what


# ---- 4: trailing bytes -----------------------------------------------------------------
def test_trailing_bytes(mctx, oracle):
    msgs = _good_messages(oracle, 5, seed=13)
    items = [oracle.write_message(m) for m in msgs]
    extra = [1, 15, 16, 17, 0]
    slots = [b + b"\xff" * e for b, e in zip(items, extra)]
    off, ln, in_cap, buf = D.place(slots, "forward")
    c, model = _sized(mctx, buf, in_cap, off, ln)
    assert [int(s) for s in c.mst] == [ETRAILING] * 4 + [OK]
    assert [int(u) for u in c.used] == [len(b) for b in items]
    assert [list(model.segs[i]) for i in range(5)] == msgs


# ---- 5: coinciding and overlapping ranges ----------------------------------------------
def test_coinciding_and_overlapping(mctx, oracle):
    msgs = _good_messages(oracle, 3, seed=21)
    items = [oracle.write_message(m) for m in msgs]
    off, ln, in_cap, buf = D.place([items[0], items[1] + items[2]], "forward")
    o = [int(off[0])] * 3 + [int(off[1]), int(off[1]) + len(items[1])]
    l = [len(items[0])] * 3 + [len(items[1]) + len(items[2]), len(items[2])]
    c, model = _sized(mctx, buf, in_cap, o, l)
    assert [int(s) for s in c.mst] == [OK, OK, OK, ETRAILING, OK]
    assert int(c.used[3]) == len(items[1])
    assert [list(s) for s in model.segs] == [msgs[0]] * 3 + [msgs[1], msgs[2]]


# ---- 6: parity with cpk_decode_messages ---------------------------------------------------
_PARITY = {}


def _parity_messages(oracle, preset):
    """About 300 messages of 1-4 segments of 0-3000 words, packed once per preset."""
    if preset not in _PARITY:
        rng = np.random.default_rng(100 + preset)
        counts = [1 + int(rng.integers(0, 4)) for _ in range(300)]
        sizes = [int(rng.integers(0, 3001)) for _ in range(sum(counts))]
        data = oracle.generate(oracle.preset(preset), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)).tobytes()
        items, s, w = [], 0, 0
        for c in counts:
            segs = []
            for z in sizes[s:s + c]:
                segs.append(data[8 * w:8 * (w + z)])
                w += z
            s += c
            items.append(oracle.write_message(segs))
        _PARITY[preset] = (items, sum(sizes), sum(counts), data)
    return _PARITY[preset]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _PARITY.clear()
    M.facts.cache_clear()


@pytest.mark.parametrize("decoder", [None, "1", "2"], ids=["dec-auto", "dec-block-map", "dec-index"])
def test_parity_with_decode_messages(oracle, decoder):
    import torch
    ctx = _new_context(decoder)
    try:
        for preset in (2, 3, 4):
            items, W, S, data = _parity_messages(oracle, preset)
            nm = len(items)
            # tiled, through cpk_decode_messages
            moff = np.concatenate([[0], np.cumsum([len(b) for b in items])]).astype(np.int64)
            tiled = np.frombuffer(b"".join(items), np.uint8)
            t_pk = _packed_dev(tiled, len(tiled))
            t_out = torch.full((W,), WORD_SENT, dtype=torch.int64, device="cuda")
            t_swo = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
            t_sin = torch.zeros(S, dtype=torch.int64, device="cuda")
            t_sst = torch.full((S,), ST_SENT, dtype=torch.int32, device="cuda")
            t_mseg = torch.zeros(nm + 1, dtype=torch.int64, device="cuda")
            t_mst = torch.full((nm,), ST_SENT, dtype=torch.int32, device="cuda")
            rc, w, s = ctx.decode_messages(t_pk, torch.from_numpy(moff).cuda(), t_out, t_swo, t_sin, t_sst, t_mseg, t_mst)
            assert (rc, w, s) == (OK, W, S)
            # placed with gaps, through cpk_decode_messages_at
            off, ln, in_cap, buf = D.place(items, "shuffled", filler="ff8ff")
            c = Call(ctx, buf, in_cap, off, ln, out_cap=W, seg_cap=S)
            mst, used, mseg, tot = c.results()
            assert tot == (W, S, nm) and (mst == OK).all() and [int(u) for u in used] == [len(b) for b in items]
            assert _clean(c.b_out, 0, W) and _clean(c.b_swo, 0, S + 1) and _clean(c.b_sin, 0, S) and _clean(c.b_sst, 0, S)
            assert torch.equal(c.d_out, t_out) and torch.equal(c.d_swo, t_swo) and torch.equal(c.d_sst, t_sst)
            assert torch.equal(c.d_mseg, t_mseg) and torch.equal(c.d_mst, t_mst)
            assert c.d_out.cpu().numpy().tobytes() == data  # (and both are the generator's words)
            # each segment's start, shifted by its slot's displacement
            shift = np.repeat(off.astype(np.int64) - moff[:-1], np.diff(t_mseg.cpu().numpy()))
            assert np.array_equal(c.d_sin.cpu().numpy(), t_sin.cpu().numpy() + shift)
            del c
    finally:
        ctx.close()


# ---- 7: round trip with cpk_encode_batch_at --------------------------------------------
def test_round_trip_with_encode_batch_at(mctx, oracle):
    """Groups whose first piece is the table's words, encoded into shuffled
    slots; the arrays that call took and wrote name the messages."""
    import torch
    rng = np.random.default_rng(77)
    counts = [1 + int(rng.integers(0, 4)) for _ in range(40)]
    pieces, groups, seg_words = [], [], []
    for m, cnt in enumerate(counts):
        sizes = [1 + int(rng.integers(0, 2500)) for _ in range(cnt)]
        t = mf.table(sizes)
        pieces.append(len(t) // 8)
        pieces += sizes
        groups.append(1 + cnt)
        seg_words += sizes
    swo = np.concatenate([[0], np.cumsum(pieces)]).astype(np.uint64)
    words = oracle.generate(oracle.preset(2), swo).view(np.uint64).copy()
    p = 0
    for cnt in counts:  # the table pieces' words
        sizes = pieces[p + 1:p + 1 + cnt]
        words[int(swo[p]):int(swo[p + 1])] = np.frombuffer(mf.table(sizes), np.uint64)
        p += 1 + cnt
    ng, n = len(groups), len(pieces)
    gpo = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
    gsz = np.array([sum(10 * w + 16 for w in pieces[gpo[g]:gpo[g + 1]]) for g in range(ng)])
    dst, cur = np.zeros(ng, np.uint64), 0
    for k, g in enumerate(D.slot_order(ng, "shuffled")):
        cur += 4 + (5 * k) % 16
        dst[g] = cur
        cur += int(gsz[g])
    out_cap = cur + 7
    d_in = torch.from_numpy(np.concatenate([words, np.zeros(1, np.uint64)]).view(np.int64).copy()).cuda()
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_grp = torch.from_numpy(gpo).cuda()
    d_dst, d_cap = _dev64(dst), _dev64(gsz)
    d_buf = torch.full(((out_cap + 15) // 16 * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_glen = torch.zeros(ng + 1, dtype=torch.int64, device="cuda")
    d_est = torch.full((ng + 1,), ST_SENT, dtype=torch.int32, device="cuda")
    mctx.encode_batch_at(d_in, d_swo, max(pieces), d_grp, d_buf, out_cap, d_dst, d_cap, d_poff, d_glen, d_est, ng=ng)
    W, S = sum(seg_words), len(seg_words)
    b_out, d_out = _guard64(W)
    b_swo, d_sw = _guard64(S + 1)
    d_sin = torch.zeros(S, dtype=torch.int64, device="cuda")
    d_sst = torch.full((S,), ST_SENT, dtype=torch.int32, device="cuda")
    d_mseg = torch.zeros(ng + 1, dtype=torch.int64, device="cuda")
    d_mst = torch.full((ng,), ST_SENT, dtype=torch.int32, device="cuda")
    d_used = torch.zeros(ng, dtype=torch.int64, device="cuda")
    d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
    mctx.decode_messages_at(d_buf, out_cap, d_dst, d_glen, d_out, d_sw, d_sin, d_sst, d_mseg, d_mst, d_used, d_tot,
                            nm=ng)
    torch.cuda.synchronize()
    assert (d_est[:ng] == OK).all()
    assert [int(v) for v in d_tot.cpu()] == [W, S, ng]
    assert (d_mst == OK).all() and (d_sst == OK).all() and torch.equal(d_used, d_glen[:ng])
    assert _clean(b_out, 0, W) and _clean(b_swo, 0, S + 1)
    assert [int(v) for v in d_mseg.cpu()] == [0] + list(np.cumsum(counts))
    assert [int(v) for v in d_sw.cpu()] == [0] + list(np.cumsum(seg_words))
    seg_piece = np.array([i for g in range(ng) for i in range(gpo[g] + 1, gpo[g + 1])])
    want = np.concatenate([words[int(swo[i]):int(swo[i + 1])] for i in seg_piece])
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)


# ---- 8: alignment sweep ------------------------------------------------------------------
def test_alignment_sweep(mctx, oracle):
    """One message whose first segment spans several decoder windows, its
    start at every byte of a 16-byte line; the message's last byte is the
    buffer's: in_cap exactly, no tail."""
    dense = np.random.default_rng(31).integers(1, 256, size=8 * 5000, dtype=np.uint8).tobytes()
    sparse = oracle.generate(oracle.preset(2), np.array([0, 700], np.uint64)).tobytes()
    segs = [dense, sparse, b""]
    msg = oracle.write_message(segs)
    assert len(msg) > 10 * 3584
    calls = []
    for s in range(16):
        buf = np.frombuffer(b"\xff" * s + msg, np.uint8)
        in_cap = len(buf)
        calls.append((Call(mctx, buf, in_cap, [s], [len(msg)], out_cap=5700, seg_cap=3), buf, in_cap, s))
    for c, buf, in_cap, s in calls:
        model = M.batch(buf, [s], [len(msg)], in_cap, mf.LIMIT, 5700, 3)
        assert list(model.status) == [OK] and list(model.segs[0]) == segs
        c.check(model, buf)


# ---- 9: empty and tiny; the calling rules ------------------------------------------------
def test_empty_and_tiny(mctx, oracle):
    import torch
    # nm == 0
    b_mseg, d_mseg = _guard64(1)
    b_tot, d_tot = _guard64(3)
    mctx.decode_messages_at(None, 0, None, None, None, None, None, None, d_mseg, None, None, d_tot, nm=0)
    torch.cuda.synchronize()
    assert _clean(b_mseg, 0) and _clean(b_tot, 0)
    assert int(d_mseg[0]) == 0 and [int(v) for v in d_tot.cpu()] == [0, 0, 0]
    # one message of one empty segment; an empty range; both again without room
    buf = np.frombuffer(b"\xff\xff\xff\x00\x00\xff", np.uint8)
    c, model = _sized(mctx, buf, 6, [3, 5], [2, 0])
    assert [int(s) for s in c.mst] == [OK, ETRUNC] and c.tot == (0, 1, 1) and [int(u) for u in c.used] == [2, 0]
    assert c.mseg == [0, 1, 1]


def test_calling_rules(mctx, oracle):
    import torch
    msg = oracle.write_message([mf.seg(0, 3)])
    buf = np.frombuffer(msg, np.uint8)
    good = Call(mctx, buf, len(msg), [0], [len(msg)], out_cap=3, seg_cap=1)
    assert list(good.results()[0]) == [OK]
    args = [good.d_pk.data_ptr(), len(msg), good.d_off.data_ptr(), good.d_len.data_ptr(), 1, mf.LIMIT,
            good.d_out.data_ptr(), 3, good.d_swo.data_ptr(), good.d_sin.data_ptr(), good.d_sst.data_ptr(), 1,
            good.d_mseg.data_ptr(), good.d_mst.data_ptr(), good.d_used.data_ptr(), good.d_tot.data_ptr(), None]
    # (index into args, what becomes of it)
    cases = [(0, args[0] + 1), (6, args[6] + 4), (2, args[2] + 4), (8, args[8] + 4), (10, args[10] + 2),
             (13, args[13] + 2), (15, args[15] + 4), (12, None), (15, None), (2, None), (13, None), (14, None),
             (8, None), (6, None)]
    before = [t.clone() for t in (good.b_out, good.b_swo, good.b_sin, good.b_sst, good.b_mseg, good.b_mst,
                                  good.b_used, good.b_tot)]
    for at, value in cases:
        a = list(args)
        a[at] = value
        assert mctx._lib.cpk_decode_messages_at(mctx.handle, *a) == EINVAL, (at, value)
    torch.cuda.synchronize()
    after = (good.b_out, good.b_swo, good.b_sin, good.b_sst, good.b_mseg, good.b_mst, good.b_used, good.b_tot)
    assert all(torch.equal(x, y) for x, y in zip(before, after))  # (a refused call writes nothing)
