"""cpk_decode_message_stream: a whole stream of packed messages whose
boundaries are not known, decoded in one call (a loop of SerializePacked.read,
SerializePacked.java:51-66).  Expected results come from the oracle only: a
loop of oracle.read_message over the remaining bytes.

Every stream is at most 1 MiB packed; each is the smallest case in which one
part of the device path can go wrong (see the builders)."""
import functools
import os

import numpy as np
import pytest

LIMIT = 8 * 1024 * 1024
GUARD = 0xA5A5A5A5A5A5A5A5 - (1 << 64)  # sentinel words around every output tensor (as int64)


# ---- streams ---------------------------------------------------------------

def _rand_words(rng, n, zero=0.5):
    """n words, about `zero` of them zero (in runs), the others with some zero bytes."""
    b = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    b[rng.random((n, 8)) < 0.25] = 0
    z = np.repeat(rng.random(n // 4 + 1) < zero, 4)[:n]
    b[z] = 0
    return b.reshape(-1).tobytes()


def _dense_words(rng, n):
    """n words without a zero byte: 8 packed bytes each inside a literal run."""
    return rng.integers(1, 256, size=8 * n, dtype=np.uint8).tobytes()


def _table(sizes):
    """The segment table's words (Serialize.java:256-273) as bytes."""
    t = np.zeros((len(sizes) + 2) & ~1, np.uint32)
    t[0] = len(sizes) - 1
    t[1:1 + len(sizes)] = sizes
    return t.tobytes()


def _write_pieces(oracle, msg, first_word=None):
    """SerializePacked.write piece by piece (first table word, rest, segments),
    the first table word replaced when given."""
    t = _table([len(s) // 8 for s in msg])
    out = oracle.pack(first_word if first_word is not None else t[:8])
    if len(t) > 8:
        out += oracle.pack(t[8:])
    return out + b"".join(oracle.pack(s) for s in msg)


def _oracle_loop(oracle, data, limit=LIMIT, out_cap=2 * 1024 * 1024):
    """while (...) SerializePacked.read(in) -> (messages, their first bytes + the end, tail status).
    (out_cap: the oracle's output bytes per message; more for a stream that declares a huge segment)"""
    msgs, offs, pos, st = [], [0], 0, oracle.OK
    while pos < len(data):
        st, segs, used = oracle.read_message(data[pos:], limit, out_cap=out_cap)
        if st != oracle.OK:
            break
        msgs.append(segs)
        pos += used
        offs.append(pos)
    return msgs, offs, st


def _ten(rng):
    """Ten small messages; the 7th has six segments (a table of four words)."""
    msgs = [[_rand_words(rng, int(rng.integers(1, 30))) for _ in range(int(rng.integers(1, 4)))] for _ in range(10)]
    msgs[6] = [_rand_words(rng, k + 1) for k in range(6)]
    msgs[9] = [_rand_words(rng, 40, zero=0.3), _dense_words(rng, 6)]
    return msgs


@functools.lru_cache(maxsize=None)
def _good():
    """name -> (stream bytes, the messages it was built from)."""
    import oracle
    rng = np.random.default_rng(20240611)
    fx = {}

    def add(name, msgs):
        fx[name] = (b"".join(oracle.write_message(m) for m in msgs), msgs)

    # the chain is per message: more messages than two rounds of 64 lanes, one-word tables
    add("130-small", [[_rand_words(rng, 1 + (7 * i) % 40)] for i in range(130)])
    # even / odd table padding, size loads of several rounds, empty segments
    add("many-segments", [[_rand_words(rng, int(k)) for k in rng.integers(0, 4, size=c)] for c in (2, 3, 4, 511, 512)])
    # more than 4 groups of 256 blocks, messages across group borders
    cfg2 = oracle.generate(oracle.preset(2), np.array([0, 5 * 16000], np.uint64)).tobytes()
    add("300k-five", [[cfg2[8 * 16000 * i: 8 * 16000 * (i + 1)]] for i in range(5)])
    # the second message starts exactly on a 256-byte block boundary
    for k in range(1, 300):
        m0 = [_dense_words(rng, 20) + b"\1\0\0\0\0\0\0\0" * k]
        if len(oracle.write_message(m0)) % 256 == 0:
            break
    add("block-boundary", [m0, [_rand_words(rng, 50)], [_rand_words(rng, 9), b""]])
    # a block that holds tens of thousands of words
    add("zero-tail", [[_rand_words(rng, 10), bytes(8 * 40000)], [_rand_words(rng, 33)]])
    # 1, 2 and 3 blocks: a message of one segment of w dense words packs to 4 + 8 w bytes, an empty one to 2
    for total, ws in ((100, (5, 6)), (300, (5, 10, 8, 12)), (700, (20, 9, 30, 1, 14, 10))):
        add(f"{total}-bytes", [[_dense_words(rng, w)] for w in ws] + [[b""], [b""]])
    add("empty", [])
    add("ten", _ten(np.random.default_rng(7)))
    return fx


@functools.lru_cache(maxsize=None)
def _bad():
    """name -> (stream bytes, limit, complete messages, tail status)."""
    import oracle
    ten = _ten(np.random.default_rng(7))
    good = b"".join(oracle.write_message(m) for m in ten)
    offs = _oracle_loop(oracle, good)[1]
    fx = {"one-short": (good[:-1], LIMIT, 9, oracle.ETRUNC),
          "mid-table": (good[:offs[6] + 5], LIMIT, 6, oracle.ETRUNC)}
    # 16 consecutive ends around a record of the last message (its last
    # segment is a literal run: the ends fall in its words)
    for i in range(16):
        fx[f"cut-{i}"] = (good[:len(good) - 20 + i], LIMIT, 9, oracle.ETRUNC)
    w = np.frombuffer(_table([len(s) // 8 for s in ten[2]])[:8], np.uint32).copy()
    w[0] = 512  # count 513
    fx["count-513"] = (good[:offs[2]] + _write_pieces(oracle, ten[2], w.tobytes()) + good[offs[3]:], LIMIT, 2,
                       oracle.EFRAME)
    # message 3 has 21 words, over a limit of 20; the others are under it
    small = [[_rand_words(np.random.default_rng(i), 3 + i)] for i in range(6)]
    small[3] = [_rand_words(np.random.default_rng(99), 12), _rand_words(np.random.default_rng(98), 9)]
    fx["over-limit"] = (b"".join(oracle.write_message(m) for m in small), 20, 3, oracle.EFRAME)
    # message 4's last segment ends in zero words and message 5 (one empty
    # segment: its table is one zero word) is packed with it as one piece, so
    # one zero run crosses the message boundary
    rng = np.random.default_rng(5)
    k = [_rand_words(rng, 7), _dense_words(rng, 3) + bytes(8 * 5)]
    t = _table([len(s) // 8 for s in k])
    joined = oracle.pack(t[:8]) + oracle.pack(t[8:]) + oracle.pack(k[0]) + oracle.pack(k[1] + bytes(8))
    fx["run-across"] = (good[:offs[4]] + joined + good[offs[5]:], LIMIT, 4, oracle.EOVERRUN)
    return fx


def _flat_words(msgs):
    return sum(1 + (len(m) & ~1) // 2 + sum(len(s) // 8 for s in m) for m in msgs)


def test_fixture_streams_read_back_by_the_oracle(oracle):
    """Pins the fixtures: the oracle loop yields the messages each good stream
    was built from, and the stated status at the stated message of each
    malformed one."""
    for name, (data, msgs) in _good().items():
        assert len(data) <= 1 << 20, name
        got, offs, st = _oracle_loop(oracle, data)
        assert st == oracle.OK and got == msgs and offs[-1] == len(data), name
    assert len(_good()["300k-five"][0]) > 4 * 256 * 256
    for total in (100, 300, 700):
        assert len(_good()[f"{total}-bytes"][0]) == total
    data, msgs = _good()["block-boundary"]
    assert len(oracle.write_message(msgs[0])) % 256 == 0
    for name, (data, limit, nm, status) in _bad().items():
        got, offs, st = _oracle_loop(oracle, data, limit)
        assert (len(got), st) == (nm, status), name
        assert offs[-1] < len(data), name


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


def _untouched(base):
    b = base.cpu().numpy()
    return (b[:2] == GUARD).all() and (b[-2:] == GUARD).all()


def _device_bytes(data):
    import torch
    d = torch.zeros(max((len(data) + 15) // 16 * 16, 16), dtype=torch.uint8, device="cuda")
    if data:
        d[:len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy())
    return d


def _decode(ctx, data, limit=LIMIT):
    """Sizes the outputs by the CPK_ENOMEM protocol, decodes, checks the
    sentinels.  -> (info, messages as [[bytes]], msg_off list)."""
    import capnp_packed as cp
    d_pk = _device_bytes(data)
    words = nm = ns = 0
    for _ in range(3):
        bo, d_out = _guarded(words)
        bm, d_mo = _guarded(nm + 1)
        bs, d_mso = _guarded(nm + 1)
        bb, d_sb = _guarded(ns)
        bw, d_sw = _guarded(ns)
        rc, info = ctx.decode_message_stream(d_pk, len(data), d_out if words else None, d_mo, d_mso,
                                             d_sb if ns else None, d_sw if ns else None, limit)
        assert all(_untouched(b) for b in (bo, bm, bs, bb, bw))
        if rc != cp.ENOMEM:
            break
        words, nm, ns = max(words, info[2]), max(nm, info[0]), max(ns, info[1])
    assert rc == cp.OK, (rc, info)
    out = d_out.cpu().numpy().view(np.uint8)
    mo, mso = d_mo.cpu().numpy(), d_mso.cpu().numpy()
    sb, sw = d_sb.cpu().numpy(), d_sw.cpu().numpy()
    assert mso[0] == 0 and mso[info[0]] == info[1] and mo[info[0]] == info[3]
    msgs = [[out[8 * int(sb[j]): 8 * int(sb[j] + sw[j])].tobytes() for j in range(int(mso[m]), int(mso[m + 1]))]
            for m in range(info[0])]
    return info, msgs, [int(v) for v in mo[:info[0] + 1]]


def _compare(ctx, oracle, data, limit=LIMIT, out_cap=2 * 1024 * 1024):
    import capnp_packed as cp
    want, offs, st = _oracle_loop(oracle, data, limit, out_cap)
    info, msgs, mo = _decode(ctx, data, limit)
    print("info", info, "oracle", len(want), sum(len(m) for m in want), offs[-1], st)
    assert info[4] != cp.EUNSUPPORTED
    assert info[0] == len(want) and info[1] == sum(len(m) for m in want)
    assert info[2] == _flat_words(want)
    assert info[3] == offs[-1] and info[4] == st
    assert (info[4] == cp.OK) == (info[3] == len(data))
    assert mo == offs
    assert msgs == want


GOOD = ["130-small", "many-segments", "300k-five", "block-boundary", "zero-tail", "100-bytes", "300-bytes",
        "700-bytes", "empty", "ten"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOOD)
def test_well_formed_stream(plain_ctx, oracle, name):
    data, msgs = _good()[name]
    if name.endswith("-bytes"):  # 1, 2 and 3 blocks of 256 bytes
        assert -(-len(data) // 256) == {"100-bytes": 1, "300-bytes": 2, "700-bytes": 3}[name]
    _compare(plain_ctx, oracle, data)


@pytest.mark.gpu
def test_parallel_path_alone(oracle):
    """With CPK_STREAM_NO_FALLBACK=1 around context creation and use no
    status may read CPK_EUNSUPPORTED: the block path itself made the result."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    os.environ["CPK_STREAM_NO_FALLBACK"] = "1"
    c = None
    try:
        c = cp.Context(0)
        for name in ("300k-five", "many-segments"):
            _compare(c, oracle, _good()[name][0])
        _compare(c, oracle, _bad()["one-short"][0])
    finally:
        os.environ.pop("CPK_STREAM_NO_FALLBACK", None)
        if c is not None:
            c.close()


BAD = ["one-short", "mid-table", "count-513", "over-limit", "run-across"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAD)
def test_malformed_tail(plain_ctx, oracle, name):
    data, limit, nm, status = _bad()[name]
    _compare(plain_ctx, oracle, data, limit)


@pytest.mark.gpu
def test_cut_at_16_consecutive_bytes(plain_ctx, oracle):
    for i in range(16):
        data, limit, nm, status = _bad()[f"cut-{i}"]
        _compare(plain_ctx, oracle, data, limit)


@pytest.mark.gpu
def test_sizing_protocol(plain_ctx, oracle):
    import capnp_packed as cp
    data, msgs = _good()["many-segments"]
    d_pk = _device_bytes(data)
    # zero capacities: the words needed
    rc, info = plain_ctx.decode_message_stream(d_pk, len(data), None, None, None, None, None)
    assert rc == cp.ENOMEM and info[2] == _flat_words(msgs)
    # room for the words only: the messages and segments needed
    bo, d_out = _guarded(info[2])
    bm, d_mo = _guarded(1)
    bs, d_mso = _guarded(1)
    rc, info = plain_ctx.decode_message_stream(d_pk, len(data), d_out, d_mo, d_mso, None, None)
    assert rc == cp.ENOMEM
    assert info[0] == len(msgs) and info[1] == sum(len(m) for m in msgs) and info[2] == _flat_words(msgs)
    assert all(_untouched(b) for b in (bo, bm, bs))
    # one segment short
    bb, d_sb = _guarded(info[1] - 1)
    bw, d_sw = _guarded(info[1] - 1)
    bm, d_mo = _guarded(info[0] + 1)
    bs, d_mso = _guarded(info[0] + 1)
    rc, info = plain_ctx.decode_message_stream(d_pk, len(data), d_out, d_mo, d_mso, d_sb, d_sw)
    assert rc == cp.ENOMEM and info[1] == sum(len(m) for m in msgs)
    assert all(_untouched(b) for b in (bo, bm, bs, bb, bw))
    # misaligned packed bytes
    with pytest.raises(cp.CodecError):
        plain_ctx.decode_message_stream(d_pk[8:], len(data) - 8, d_out, d_mo, d_mso, d_sb, d_sw)


@pytest.mark.gpu
def test_host_form(plain_ctx, oracle):
    import capnp_packed as cp
    for name in GOOD:
        data, msgs = _good()[name]
        tail, got, consumed = plain_ctx.decode_message_stream_host(data)
        assert (tail, consumed) == (cp.OK, len(data)), name
        assert got == msgs, name
    for name in BAD:
        data, limit, nm, status = _bad()[name]
        want, offs, st = _oracle_loop(oracle, data, limit)
        tail, got, consumed = plain_ctx.decode_message_stream_host(data, limit)
        assert (tail, consumed) == (st, offs[-1]) and got == want, name
