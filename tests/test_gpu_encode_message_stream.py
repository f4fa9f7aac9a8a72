"""cpk_encode_message_stream: a whole stream of unpacked messages whose
boundaries are not known, packed in one call (a loop of Serialize.read,
Serialize.java:119-178, each message written with SerializePacked.write).

Expected values never come from the code under test: the counts, the piece
boundaries and the tail status from a plain restatement of the unpacked
Serialize.read loop (_read_loop below), the packed bytes from the oracle
(cpko_pack per piece, through oracle.pack_batch; oracle.write_message per
message for the streams whose table pads are zero).

Streams are a few KiB unless a case says otherwise; each is the smallest in
which one part of the device path can go wrong."""
import functools

import numpy as np
import pytest

LIMIT = 8 * 1024 * 1024
MAX_SEGMENT_WORDS = (1 << 28) - 1
OK, ETRUNC, ENOMEM, EFRAME = 0, -2, -5, -7
GUARD = 0xA5A5A5A5A5A5A5A5 - (1 << 64)  # sentinel words around every output array (as int64)
GUARD_BYTE = 0xA5


# ---- streams ---------------------------------------------------------------

def _table(sizes, pad=0, count_field=None):
    """The segment table's words (Serialize.java:256-273) as bytes; `pad`: the
    half-word after an even count of sizes."""
    n = len(sizes)
    t = np.zeros((n + 2) & ~1, np.uint32)
    t[0] = n - 1 if count_field is None else count_field
    t[1:1 + n] = sizes
    if n % 2 == 0:
        t[-1] = pad
    return t.tobytes()


def _message(segs, pad=0):
    return _table([len(s) // 8 for s in segs], pad) + b"".join(segs)


def _words(b):
    return np.frombuffer(b, np.uint64).copy() if b else np.zeros(0, np.uint64)


def _cfg_words(cfg, n, seed=0):
    """n words of the synthetic workload `cfg` (the oracle's generator)."""
    import oracle
    swo = np.zeros(seed + 2, np.uint64)  # (the generator is seeded per segment: segment `seed`)
    swo[-1] = n
    return oracle.generate(oracle.preset(cfg), swo, first=seed, count=1).tobytes()


def _cut(data, sizes):
    """data cut into segments of the given word counts."""
    out, o = [], 0
    for s in sizes:
        out.append(data[8 * o: 8 * (o + s)])
        o += s
    return out


def _read_loop(words, limit=LIMIT):
    """The loop of Serialize.read(ReadableByteChannel) over unpacked words
    (Serialize.java:119-178), restated: -> (piece word offsets [pieces + 1] of
    the complete messages, msg_piece [messages + 1], words consumed, tail
    status, largest piece in words)."""
    W = len(words)
    u = words.view(np.uint32)
    x, off, mp, largest, st = 0, [0], [0], 0, OK
    while x < W:
        raw = int(np.int32(u[2 * x]))
        if raw < 0 or raw > 511:  # :128-131
            st = EFRAME
            break
        count = raw + 1
        if int(np.int32(u[2 * x + 1])) < 0:  # :135-139
            st = EFRAME
            break
        rest = (count & ~1) // 2
        if x + 1 + rest > W:  # :146-148 fillBuffer: premature EOF
            st = ETRUNC
            break
        sizes = [int(v) for v in u[2 * x + 1: 2 * x + 1 + count].view(np.int32)]
        if any(s < 0 for s in sizes):  # :150-153
            st = EFRAME
            break
        if sum(sizes) > limit:  # :160-162
            st = EFRAME
            break
        pos, ends = x + 1 + rest, []
        for s in sizes:  # :165-175, makeByteBufferForWords :45-53
            if s > MAX_SEGMENT_WORDS:
                st = EFRAME
                break
            if pos + s > W:
                st = ETRUNC
                break
            pos += s
            ends.append(pos)
        if st != OK:
            break
        off += [x + 1 + rest] + ends
        largest = max([largest, 1 + rest] + sizes)
        x = pos
        mp.append(len(off) - 1)
    return off, mp, x, st, largest


def _expected(oracle, words, limit=LIMIT):
    off, mp, x, st, largest = _read_loop(words, limit)
    pk, poff = oracle.pack_batch(words.view(np.uint8), np.array(off, np.uint64))
    return dict(bytes=pk.tobytes(), off=[int(v) for v in poff], mp=mp, consumed=x, tail=st, largest=largest,
                pieces=len(off) - 1, word_off=off)


COUNTS = (1, 2, 3, 127, 128, 129, 512)


@functools.lru_cache(maxsize=None)
def _counts_stream(cfg):
    """Messages of 1, 2, 3, 127, 128, 129 and 512 segments of 0..3 words in
    one stream, small ones between them (tables of one 64-lane round, of
    exactly two, of more; even and odd counts; empty segments)."""
    rng = np.random.default_rng(100 + cfg)
    msgs = []
    for i, c in enumerate(COUNTS):
        sizes = [int(v) for v in rng.integers(0, 4, size=c)]
        sizes[-1] = 0 if i % 2 else 3  # (an empty last segment: it sits at the next message's first word)
        msgs.append(_cut(_cfg_words(cfg, sum(sizes), seed=i), sizes))
        msgs.append(_cut(_cfg_words(cfg, 7, seed=50 + i), [7]))
    return b"".join(_message(m) for m in msgs), msgs


@functools.lru_cache(maxsize=None)
def _ten():
    """Ten small messages; message 4 has three segments (a table of two words)."""
    msgs = []
    for i in range(10):
        sizes = [5, 9, 4] if i == 4 else [3 + i] * (1 + i % 2)
        msgs.append(_cut(_cfg_words(2, sum(sizes), seed=200 + i), sizes))
    return msgs


def _starts(msgs):
    s = [0]
    for m in msgs:
        s.append(s[-1] + len(_message(m)) // 8)
    return s


def test_restated_read_loop_agrees_with_the_oracle(oracle):
    """Pins _read_loop and the fixtures: on a zero-pad stream its pieces,
    packed by the oracle, are the oracle's SerializePacked.write of each
    message, and reading those bytes back (oracle.read_message) gives the
    messages the stream was built from."""
    data, msgs = _counts_stream(2)
    assert len(data) < 32 * 1024
    e = _expected(oracle, _words(data))
    assert (e["tail"], e["consumed"]) == (OK, len(data) // 8)
    assert e["mp"][-1] == e["pieces"] == sum(1 + len(m) for m in msgs)
    assert e["bytes"] == b"".join(oracle.write_message(m) for m in msgs)
    pos = 0
    for m in msgs:
        st, segs, used = oracle.read_message(e["bytes"][pos:], LIMIT, out_cap=1 << 16)
        assert st == oracle.OK and segs == m
        pos += used
    assert pos == len(e["bytes"])


# ---- the device call --------------------------------------------------------

@pytest.fixture()
def plain_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    c = cp.Context(0)
    try:
        yield c
    finally:
        c.close()


def _guarded(n):
    """A tensor of n words with two sentinel words on each side."""
    import torch
    base = torch.full((n + 4,), GUARD, dtype=torch.int64, device="cuda")
    return base, base[2:2 + n]


def _guarded_bytes(n, after=64):
    """n bytes at a 16-byte aligned address, 64 sentinel bytes before and `after` behind."""
    import torch
    base = torch.full((64 + n + after,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    return base, base[64:64 + n]


def _untouched(base, inner=None):
    b = base.cpu().numpy()
    if b.dtype == np.uint8:
        return bool((b[:64] == GUARD_BYTE).all() and (b[64 + inner:] == GUARD_BYTE).all())
    return bool((b[:2] == GUARD).all() and (b[-2:] == GUARD).all())


def _device_words(words):
    import torch
    d = torch.zeros(max(len(words), 1), dtype=torch.int64, device="cuda")
    if len(words):
        d[:len(words)] = torch.from_numpy(words.view(np.int64).copy())
    return d


def _encode(ctx, words, limit=LIMIT, avail=None):
    """Sizes the outputs by the CPK_ENOMEM protocol (the arrays, then the
    bytes), packs, checks the sentinels.  -> (info, packed bytes, out_off,
    msg_piece)."""
    d_in = _device_words(words)
    avail = len(words) if avail is None else avail
    cap = npieces = nm = -1
    for _ in range(3):
        bo, d_out = _guarded_bytes(max(cap, 0))
        bf, d_off = _guarded(npieces + 1)
        bm, d_mp = _guarded(nm + 1)
        rc, info = ctx.encode_message_stream(d_in, avail, d_out if cap > 0 else None,
                                             d_off if npieces >= 0 else None, d_mp if nm >= 0 else None, limit)
        assert _untouched(bo, max(cap, 0)) and _untouched(bf) and _untouched(bm)
        if rc != ENOMEM:
            break
        if npieces < 0:
            npieces, nm = info[1], info[0]
        else:
            cap = info[3]
    assert rc == OK, (rc, info)
    out = d_out.cpu().numpy()[:info[3]].tobytes()
    off = [int(v) for v in d_off.cpu().numpy()[:info[1] + 1]]
    mp = [int(v) for v in d_mp.cpu().numpy()[:info[0] + 1]]
    return info, out, off, mp


def _compare(ctx, oracle, words, limit=LIMIT):
    e = _expected(oracle, words, limit)
    info, out, off, mp = _encode(ctx, words, limit)
    print("info", info, "expected", len(e["mp"]) - 1, e["pieces"], e["consumed"], len(e["bytes"]), e["tail"],
          e["largest"])
    assert info[:4] == [len(e["mp"]) - 1, e["pieces"], e["consumed"], len(e["bytes"])]
    assert info[4] == e["tail"] and info[5] == e["largest"]
    assert (info[4] == OK) == (info[2] == len(words))
    assert mp == e["mp"]
    assert off == e["off"]
    assert out == e["bytes"]
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_segment_counts(ctx, oracle, cfg):
    """Through each encoder choice (the `ctx` fixture: by piece size, the
    single pass forced, the two passes forced)."""
    data, msgs = _counts_stream(cfg)
    e = _compare(ctx, oracle, _words(data))
    assert e["tail"] == OK and len(e["mp"]) - 1 == len(msgs)
    assert e["bytes"] == b"".join(oracle.write_message(m) for m in msgs)  # (zero pads)


@pytest.mark.gpu
def test_large_piece(ctx, oracle):
    """A 20,000-word segment: a piece over one 8192-word chunk of the single pass."""
    msgs = [_cut(_cfg_words(2, 12, seed=1), [12]), _cut(_cfg_words(2, 20009, seed=2), [20000, 9]),
            _cut(_cfg_words(2, 5, seed=3), [5])]
    e = _compare(ctx, oracle, _words(b"".join(_message(m) for m in msgs)))
    assert e["tail"] == OK and e["largest"] == 20000
    assert e["bytes"] == b"".join(oracle.write_message(m) for m in msgs)


@pytest.mark.gpu
def test_one_word_tables_in_a_literal_run(ctx, oracle):
    """2,000 single-segment messages of 5 words: 4,000 pieces, each 1-word
    table (count - 1 = 0, size 5) packed on its own from fresh run state."""
    body = _cfg_words(2, 5 * 2000, seed=9)
    msgs = [[body[40 * i: 40 * (i + 1)]] for i in range(2000)]
    e = _compare(ctx, oracle, _words(b"".join(_message(m) for m in msgs)))
    assert (e["tail"], len(e["mp"]) - 1, e["pieces"]) == (OK, 2000, 4000)
    assert e["bytes"][:2] == bytes([0x10, 5])  # the table word 0x0000000500000000: one nonzero byte


@pytest.mark.gpu
def test_empty_and_tiny_streams(plain_ctx, oracle):
    import torch
    # no words: no messages, d_out_off[0] = 0
    bf, d_off = _guarded(1)
    bm, d_mp = _guarded(1)
    rc, info = plain_ctx.encode_message_stream(_device_words(np.zeros(0, np.uint64)), 0, None, d_off, d_mp)
    assert rc == OK and info == [0, 0, 0, 0, OK, 0]
    assert int(d_off[0]) == 0 and int(d_mp[0]) == 0 and _untouched(bf) and _untouched(bm)
    torch.cuda.synchronize()
    # one empty single-segment message: the one-word table and a piece of no words
    e = _compare(plain_ctx, oracle, _words(_message([b""])))
    assert (e["tail"], e["pieces"], e["off"], e["bytes"]) == (OK, 2, [0, 2, 2], oracle.write_message([b""]))


def _three_segment_stream():
    """_ten(): message 4 has three segments -> (words, first word of each message)."""
    msgs = _ten()
    assert len(msgs[4]) == 3
    return _words(b"".join(_message(m) for m in msgs)), _starts(msgs)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first-table-word", "mid-table", "after-table", "mid-segment"])
def test_truncated_tail(plain_ctx, oracle, where):
    words, starts = _three_segment_stream()
    x = starts[4]  # table: 2 words; segments of 5, 9 and 4 words
    cut = {"first-table-word": x + 1, "mid-table": x + 1, "after-table": x + 2, "mid-segment": x + 2 + 5 + 4}[where]
    if where == "mid-table":
        # a table of 4 words (6 segments) cut after its second
        six = _cut(_cfg_words(2, 21, seed=77), [1, 2, 3, 4, 5, 6])
        words = np.concatenate([words[:x], _words(_message(six))])
        cut = x + 2
    e = _compare(plain_ctx, oracle, words[:cut])
    assert (e["tail"], e["consumed"], len(e["mp"]) - 1) == (ETRUNC, x, 4)
    # the messages before the cut are packed as the whole stream's are
    assert e["bytes"] == b"".join(oracle.write_message(m) for m in _ten()[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["count-513", "size-bit-31", "first-size-bit-31", "over-limit", "at-limit"])
def test_table_refused(plain_ctx, oracle, what):
    msgs = _ten()
    good = b"".join(_message(m) for m in msgs)
    x = _starts(msgs)[3]
    limit = LIMIT
    if what == "count-513":
        bad = _table([1] * 513) + bytes(8 * 513)  # (the words a 513-segment message would have)
    elif what == "size-bit-31":
        bad = _table([2, 0x80000000]) + bytes(8 * 2)
    elif what == "first-size-bit-31":
        bad = _table([0x80000001]) + bytes(8)
    else:
        # 64 words in two segments against a limit of 64, or one more; every other message is under it
        limit = 64
        n = 65 if what == "over-limit" else 64
        bad = _message(_cut(_cfg_words(3, n, seed=5), [40, n - 40]))
    words = _words(good[:8 * x] + bad + good[8 * x:])
    e = _compare(plain_ctx, oracle, words, limit)
    if what == "at-limit":
        assert (e["tail"], len(e["mp"]) - 1, e["consumed"]) == (OK, 11, len(words))
    else:
        assert (e["tail"], len(e["mp"]) - 1, e["consumed"]) == (EFRAME, 3, x)


@pytest.mark.gpu
def test_nonzero_pad_is_kept(plain_ctx, oracle):
    """Serialize.write zeroes the pad of an even-count table; this call packs
    the table's words as they stand, so the packed stream decodes back to the
    input words, pad included (the documented divergence)."""
    msgs = _ten()
    two = _cut(_cfg_words(2, 11, seed=31), [4, 7])
    data = _message(msgs[0]) + _message(two, pad=0xDEADBEEF) + _message(msgs[1])
    words = _words(data)
    e = _compare(plain_ctx, oracle, words)
    assert e["tail"] == OK
    assert e["bytes"] != b"".join(oracle.write_message(m) for m in (msgs[0], two, msgs[1]))
    # decoded piece by piece by the oracle: the input words
    back, st = oracle.unpack_batch(np.frombuffer(e["bytes"], np.uint8), np.array(e["off"], np.uint64),
                                   np.array(e["word_off"], np.uint64))
    assert (st == 0).all() and back.tobytes() == data
    # and by the device's stream reader: the same flat words
    info, flat, _ = _decode_stream(plain_ctx, e["bytes"])
    assert info[4] == OK and flat.tobytes() == data


@pytest.mark.gpu
def test_sizing_protocol(ctx, oracle):
    """Through each encoder choice: the total is exact whatever the capacity."""
    data, msgs = _counts_stream(2)
    words = _words(data)
    e = _expected(oracle, words)
    d_in = _device_words(words)
    total = len(e["bytes"])
    # everything NULL / 0: the arrays' sizes
    rc, info = ctx.encode_message_stream(d_in, len(words), None, None, None)
    assert rc == ENOMEM and info[:2] == [len(msgs), e["pieces"]]
    # one piece short
    bf, d_off = _guarded(info[1])
    bm, d_mp = _guarded(info[0] + 1)
    rc, info = ctx.encode_message_stream(d_in, len(words), None, d_off, d_mp)
    assert rc == ENOMEM and info[:2] == [len(msgs), e["pieces"]] and _untouched(bf) and _untouched(bm)
    # the arrays, no bytes: the packed total
    bf, d_off = _guarded(info[1] + 1)
    rc, info = ctx.encode_message_stream(d_in, len(words), None, d_off, d_mp)
    assert rc == ENOMEM and info[:4] == [len(msgs), e["pieces"], len(words), total]
    assert _untouched(bf) and _untouched(bm)
    assert ctx.take_error() == OK  # (reported by the return value, nothing left behind)
    # exactly the total, 64 sentinel bytes behind
    bo, d_out = _guarded_bytes(total)
    rc, info = ctx.encode_message_stream(d_in, len(words), d_out, d_off, d_mp)
    assert rc == OK and info == [len(msgs), e["pieces"], len(words), total, OK, e["largest"]]
    assert d_out.cpu().numpy().tobytes() == e["bytes"]
    assert [int(v) for v in d_off.cpu().numpy()] == e["off"] and [int(v) for v in d_mp.cpu().numpy()] == e["mp"]
    assert _untouched(bo, total) and _untouched(bf) and _untouched(bm)
    # one byte short: refused, nothing stored at or past the capacity
    bo, d_out = _guarded_bytes(total - 1, after=65)
    rc, info = ctx.encode_message_stream(d_in, len(words), d_out, d_off, d_mp)
    assert rc == ENOMEM and info[3] == total
    assert _untouched(bo, total - 1)
    assert ctx.take_error() == OK
    # misaligned words / bytes
    import capnp_packed as cp
    import torch
    with pytest.raises(cp.CodecError):
        ctx.encode_message_stream(d_in.view(torch.uint8)[4:], len(words) - 1, d_out, d_off, d_mp)
    with pytest.raises(cp.CodecError):
        ctx.encode_message_stream(d_in, len(words), bo[72:], d_off, d_mp)


def _decode_stream(ctx, packed, limit=LIMIT):
    """cpk_decode_message_stream, sized by its own protocol.  -> (info, flat
    words as uint64, (msg_seg_off, seg_begin, seg_words))."""
    import torch
    d_pk = torch.zeros(max((len(packed) + 15) // 16 * 16, 16), dtype=torch.uint8, device="cuda")
    if packed:
        d_pk[:len(packed)] = torch.from_numpy(np.frombuffer(packed, np.uint8).copy())
    words = nm = ns = 0
    for _ in range(3):
        d_out = torch.zeros(max(words, 1), dtype=torch.int64, device="cuda")
        d_mo = torch.zeros(nm + 1, dtype=torch.int64, device="cuda")
        d_mso = torch.zeros(nm + 1, dtype=torch.int64, device="cuda")
        d_sb = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda")
        d_sw = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda")
        rc, info = ctx.decode_message_stream(d_pk, len(packed), d_out if words else None, d_mo, d_mso,
                                             d_sb if ns else None, d_sw if ns else None, limit)
        if rc != ENOMEM:
            break
        words, nm, ns = max(words, info[2]), max(nm, info[0]), max(ns, info[1])
    assert rc == OK, (rc, info)
    flat = d_out.cpu().numpy().view(np.uint64)[:info[2]]
    lay = ([int(v) for v in d_mso.cpu().numpy()[:info[0] + 1]], [int(v) for v in d_sb.cpu().numpy()[:info[1]]],
           [int(v) for v in d_sw.cpu().numpy()[:info[1]]])
    return info, flat, lay


@pytest.mark.gpu
def test_round_trip_unpacked_packed_unpacked(plain_ctx, oracle):
    """decode_message_stream(encode_message_stream(x)) gives x's words and the
    segment layout the restated read loop finds in x."""
    data, msgs = _counts_stream(3)
    words = _words(data)
    info, packed, off, mp = _encode(plain_ctx, words)
    dinfo, flat, (mso, sb, sw) = _decode_stream(plain_ctx, packed)
    assert dinfo[4] == OK and dinfo[3] == len(packed)
    assert flat.tobytes() == data
    poff, pmp, _, _, _ = _read_loop(words)
    want_sb, want_sw, want_mso = [], [], [0]
    for m in range(len(pmp) - 1):
        for p in range(pmp[m] + 1, pmp[m + 1]):  # (a message's first piece is its table)
            want_sb.append(poff[p])
            want_sw.append(poff[p + 1] - poff[p])
        want_mso.append(len(want_sb))
    assert (mso, sb, sw) == (want_mso, want_sb, want_sw)
    assert dinfo[:2] == [len(msgs), len(want_sb)]


@pytest.mark.gpu
def test_round_trip_packed_unpacked_packed(plain_ctx, oracle):
    """encode_message_stream of the flat output of decode_message_stream(p)
    gives p back, for p made by encode_messages."""
    import torch
    data, msgs = _counts_stream(4)
    segs = [s for m in msgs for s in m]
    swo = np.concatenate([[0], np.cumsum([len(s) // 8 for s in segs])]).astype(np.int64)
    mso = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.int64)
    body = b"".join(segs)
    d_in = _device_words(_words(body))
    d_swo, d_mso = torch.from_numpy(swo).cuda(), torch.from_numpy(mso).cuda()
    cap = 10 * (len(body) // 8) + 16 + sum(10 * ((len(m) + 2) // 2 + 1) for m in msgs)
    d_p = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_poff = torch.zeros(len(msgs) + len(segs) + 1, dtype=torch.int64, device="cuda")
    plain_ctx.encode_messages(d_in, d_swo, d_mso, 8, d_p, d_poff)
    poff = [int(v) for v in d_poff.cpu().numpy()]
    p = d_p.cpu().numpy()[:poff[-1]].tobytes()
    assert p == b"".join(oracle.write_message(m) for m in msgs)
    dinfo, flat, _ = _decode_stream(plain_ctx, p)
    assert dinfo[4] == OK and flat.tobytes() == data
    info, packed, off, mp = _encode(plain_ctx, flat)
    assert info[4] == OK and packed == p and off == poff
    assert mp == [int(mso[m]) + m for m in range(len(msgs) + 1)]


@pytest.mark.gpu
def test_host_form(plain_ctx, oracle):
    msgs = _ten()
    x = _starts(msgs)[4]
    good = _words(b"".join(_message(m) for m in msgs))
    refused = _words(_message(msgs[0]) + _table([1] * 513) + bytes(8 * 513))
    for name, words, limit in (("counts", _words(_counts_stream(2)[0]), LIMIT),
                               ("mid-segment", good[:x + 2 + 5 + 4], LIMIT),
                               ("count-513", refused, LIMIT),
                               ("empty", np.zeros(0, np.uint64), LIMIT)):
        e = _expected(oracle, words, limit)
        tail, packed, off, mp, consumed = plain_ctx.encode_message_stream_host(words, limit)
        assert (tail, consumed) == (e["tail"], e["consumed"]), name
        assert packed == e["bytes"] and [int(v) for v in off] == e["off"] and [int(v) for v in mp] == e["mp"], name
    # bytes as well as words
    tail, packed, _, _, consumed = plain_ctx.encode_message_stream_host(good.tobytes())
    assert (tail, consumed, packed) == (OK, len(good), _expected(oracle, good)["bytes"])
