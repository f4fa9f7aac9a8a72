"""The context's scratch buffers across growth (csrc/host_api.hip: DevBuf,
reserve): every buffer is allocated by the first call that needs it, freed
and allocated anew when a later call needs more, and used again afterwards.

Each case runs, on one context, a small shape (the buffer at its floor), one
large enough to pass the floor and force a regrow, and the small shape again.
All three results are compared byte for byte with the oracle, statuses
included.  The module-scoped `ctx` fixture gives this module a fresh context
per encoder / decoder pair; where a shape cannot reach a buffer under one of
the pairs the case still runs there and only exercises less.

Which buffer each shape reaches (the floors and needs are host_api.hip's):
  batches          `status` past its floor of 1,024 entries (two passes);
                   `sp_status` past 8,192 (single pass: two words per piece);
                   `sp_units` for pieces over one 8,192-word chunk
  message batches  `sp_desc` (single pass: forced, or at most 1,024 pieces);
                   `status` and `e4_bv` (two passes)
  streams          `ss_buf` from 384 KiB packed (kSsMin)
  message streams  `ms_buf`: more messages than a message per 64 bytes + 1,024
  unpacked message streams  `ems_buf` past 1,024 piece offsets"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMIT = 8 * 1024 * 1024
OK, ENOMEM = 0, -5


def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _dev(a, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).cuda()


def _dev_bytes(b):
    """The bytes on the device at a 16-byte aligned address, 64 zero bytes of read slack behind."""
    import torch
    d = torch.zeros((len(b) + 64 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    if len(b):
        d[:len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy())
    return d


def _cfg2(words, seed=0):
    """`words` words of the synthetic workload 2 (about half of them zero)."""
    import oracle
    swo = np.zeros(seed + 2, np.uint64)  # (the generator is seeded per segment: segment `seed`)
    swo[-1] = words
    return oracle.generate(oracle.preset(2), swo, first=seed, count=1)


def _table(sizes):
    """The segment table's words (Serialize.java:256-273) as bytes."""
    t = np.zeros((len(sizes) + 2) & ~1, np.uint32)
    t[0] = len(sizes) - 1
    t[1:1 + len(sizes)] = sizes
    return t.tobytes()


def _messages(nm, seed):
    """nm messages of 3 segments of 0..40 words."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 41, size=(nm, 3))
    data = _cfg2(int(sizes.sum()), seed).tobytes()
    msgs, o = [], 0
    for row in sizes:
        m = []
        for s in row:
            m.append(data[8 * o: 8 * (o + int(s))])
            o += int(s)
        msgs.append(m)
    return msgs


def _in_turn(check, small, large):
    """small, large, small again: the same context before, across and after a regrow."""
    for shape in (small, large, small):
        check(shape)


# ---- cpk_encode_batch / cpk_decode_batch ----------------------------------

@functools.lru_cache(maxsize=None)
def _batch(n, words, seed):
    """n pieces of `words` words -> (swo, data, oracle's packed bytes, offsets, statuses of its decode)."""
    import oracle
    swo = _swo([words] * n)
    data = _cfg2(n * words, seed)
    pk, off = oracle.pack_batch(data, swo, threads=8)
    back, st = oracle.unpack_batch(pk, off, swo, threads=8)
    assert np.array_equal(back, data)
    return swo, data, pk, off, st


def _check_batch(ctx, shape):
    import torch
    import capnp_packed as cp
    swo, data, pk, off, st = _batch(*shape)
    words = shape[1]
    d_in, d_swo = _dev(np.append(data, np.zeros(8, np.uint8))), _dev(swo)
    d_pk = torch.zeros((cp.batch_capacity(swo) + 63) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_off = torch.full((len(swo),), -1, dtype=torch.int64, device="cuda")
    ctx.encode_batch(d_in, d_swo, words, d_pk, d_off)
    assert ctx.take_error() == OK
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), off), shape
    assert np.array_equal(d_pk[:len(pk)].cpu().numpy(), pk), shape
    d_out = torch.zeros(int(swo[-1]) + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(swo) - 1,), 99, dtype=torch.int32, device="cuda")
    ctx.decode_batch(d_pk, d_off, d_swo, d_out, d_st)
    torch.cuda.synchronize()
    assert np.array_equal(d_st.cpu().numpy(), st), shape
    assert np.array_equal(d_out.cpu().numpy().view(np.uint8)[:data.size], data), shape


def test_batches(ctx, oracle):
    """16 pieces of 64 words, then 6,000 (past `status`' floor; under the
    forced single pass 12,000 look-back words, past `sp_status`' 8,192); 3
    pieces of 20,000 words with the hint given (`sp_units` allocated), then
    40 of them (regrown)."""
    _in_turn(lambda s: _check_batch(ctx, s), (16, 64, 1), (6000, 64, 2))
    _in_turn(lambda s: _check_batch(ctx, s), (3, 20000, 3), (40, 20000, 4))


# ---- cpk_encode_messages / cpk_decode_messages -----------------------------

@functools.lru_cache(maxsize=None)
def _message_batch(nm, seed):
    """-> (messages, oracle's packed stream, piece offsets, message offsets)."""
    import oracle
    msgs = _messages(nm, seed)
    pieces = [p for m in msgs for p in [_table([len(s) // 8 for s in m])] + m]
    pk, off = oracle.pack_batch(np.frombuffer(b"".join(pieces) + bytes(8), np.uint8),
                                _swo([len(p) // 8 for p in pieces]), threads=8)
    assert pk.tobytes() == b"".join(oracle.write_message(m) for m in msgs)
    for i in (0, nm // 2, nm - 1):  # (Serialize.read gives the segments back)
        st, segs, used = oracle.read_message(pk[int(off[4 * i]): int(off[4 * i + 4])].tobytes(), LIMIT, out_cap=1 << 12)
        assert (st, segs, used) == (oracle.OK, msgs[i], int(off[4 * i + 4] - off[4 * i]))
    return msgs, pk, off, off[::4]


def _check_message_batch(ctx, shape):
    import torch
    import capnp_packed as cp
    msgs, pk, off, moff = _message_batch(*shape)
    nm = len(msgs)
    segs = [s for m in msgs for s in m]
    swo, mseg = _swo([len(s) // 8 for s in segs]), _swo([3] * nm)
    d_in = _dev(np.frombuffer(b"".join(segs) + bytes(8), np.uint8))
    cap = cp.batch_capacity(swo) + 20 * nm
    d_pk = torch.zeros((cap + 63) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_off = torch.full((nm + len(segs) + 1,), -1, dtype=torch.int64, device="cuda")
    ctx.encode_messages(d_in, _dev(swo), _dev(mseg), 40, d_pk, d_off)
    assert ctx.take_error() == OK
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), off), shape
    assert np.array_equal(d_pk[:len(pk)].cpu().numpy(), pk), shape
    # and back (the message ranges: the table pieces' offsets)
    d_mso = torch.full((nm + 1,), -1, dtype=torch.int64, device="cuda")
    d_mst = torch.full((nm,), 99, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(int(swo[-1]) + 1, dtype=torch.int64, device="cuda")
    d_sw = torch.full((len(segs) + 1,), -1, dtype=torch.int64, device="cuda")
    d_si = torch.zeros(len(segs) + 1, dtype=torch.int64, device="cuda")
    d_ss = torch.full((len(segs),), 99, dtype=torch.int32, device="cuda")
    rc, W, S = ctx.decode_messages(d_pk, _dev(moff), d_out, d_sw, d_si, d_ss, d_mso, d_mst)
    torch.cuda.synchronize()
    assert (rc, W, S) == (OK, int(swo[-1]), len(segs)), shape
    assert not d_mst.cpu().numpy().any() and not d_ss.cpu().numpy().any(), shape
    assert np.array_equal(d_mso.cpu().numpy().view(np.uint64), mseg), shape
    assert np.array_equal(d_sw.cpu().numpy().view(np.uint64), swo), shape
    assert d_out.cpu().numpy().view(np.uint8)[:8 * W].tobytes() == b"".join(segs), shape


def test_message_batches(ctx, oracle):
    """4 messages of 3 segments (16 pieces), then 1,500 (6,000 pieces: past
    `sp_desc` under the forced single pass, past `status` and `e4_bv` under
    the two passes, which a batch over 1,024 pieces takes by default)."""
    _in_turn(lambda s: _check_message_batch(ctx, s), (4, 11), (1500, 12))


# ---- cpk_decode_stream ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stream(chunks, seed):
    """`chunks` pieces of 8,192 words and three odd ones, back to back -> (swo, data, stream, piece boundaries)."""
    import oracle
    swo = _swo([8192] * chunks + [0, 5, 777])
    data = _cfg2(int(swo[-1]), seed)
    pk, off = oracle.pack_batch(data, swo, threads=8)
    back, st = oracle.unpack_batch(pk, off, swo, threads=8)
    assert np.array_equal(back, data) and not st.any()
    return swo, data, pk.tobytes(), off


def _check_stream(ctx, shape):
    import torch
    swo, data, stream, off = _stream(*shape)
    assert len(stream) >= 384 * 1024  # (kSsMin: cut into blocks, the map in `ss_buf`)
    d_pk, d_swo = _dev_bytes(stream), _dev(swo)
    d_out = torch.zeros(int(swo[-1]) + 1, dtype=torch.int64, device="cuda")
    d_io = torch.full((len(swo),), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(swo) - 1,), 99, dtype=torch.int32, device="cuda")
    ctx.decode_stream(d_pk, len(stream), d_swo, d_out, d_io, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any(), shape
    assert np.array_equal(d_io.cpu().numpy().view(np.uint64), off), shape
    assert np.array_equal(d_out.cpu().numpy().view(np.uint8)[:data.size], data), shape


def test_streams(ctx, oracle):
    """One stream of a little over 400 KiB packed, then one of about 1.6 MiB."""
    small, large = (14, 21), (56, 22)
    assert 400 * 1024 <= len(_stream(*small)[2]) < 512 * 1024 and len(_stream(*large)[2]) >= 3 * 512 * 1024
    _in_turn(lambda s: _check_stream(ctx, s), small, large)


# ---- cpk_decode_message_stream ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _packed_message_stream(nm, seed):
    """nm messages of one segment, empty but for one in 64 (an empty one packs
    to 2 bytes) -> (stream, messages, their first bytes + the end) by a loop
    of the oracle's SerializePacked.read."""
    import oracle
    words = _cfg2(9 * (nm // 64 + 1), seed).tobytes()
    built = [[words[72 * (i // 64): 72 * (i // 64 + 1)] if i % 64 == 3 else b""] for i in range(nm)]
    data = b"".join(oracle.write_message(m) for m in built)
    msgs, offs, pos = [], [0], 0
    while pos < len(data):
        st, segs, used = oracle.read_message(data[pos:pos + 4096], LIMIT, out_cap=1 << 12)
        assert st == oracle.OK
        msgs.append(segs)
        pos += used
        offs.append(pos)
    assert msgs == built
    return data, msgs, offs


def _check_packed_message_stream(ctx, shape):
    import torch
    data, msgs, offs = _packed_message_stream(*shape)
    d_pk = _dev_bytes(data)
    words = nm = ns = 0
    for _ in range(3):  # (sized by the CPK_ENOMEM protocol)
        d_out = torch.zeros(max(words, 1), dtype=torch.int64, device="cuda")
        d_mo = torch.full((nm + 1,), -1, dtype=torch.int64, device="cuda")
        d_mso = torch.full((nm + 1,), -1, dtype=torch.int64, device="cuda")
        d_sb = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda")
        d_sw = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda")
        rc, info = ctx.decode_message_stream(d_pk, len(data), d_out if words else None, d_mo, d_mso,
                                             d_sb if ns else None, d_sw if ns else None, LIMIT)
        if rc != ENOMEM:
            break
        words, nm, ns = max(words, info[2]), max(nm, info[0]), max(ns, info[1])
    assert rc == OK, (rc, info)
    flat = sum(1 + len(m[0]) // 8 for m in msgs)  # (a one-word table before each segment)
    assert info == [len(msgs), len(msgs), flat, len(data), OK], shape
    assert [int(v) for v in d_mo.cpu().numpy()] == offs, shape
    assert [int(v) for v in d_mso.cpu().numpy()] == list(range(len(msgs) + 1)), shape
    out = d_out.cpu().numpy().view(np.uint8)
    sb, sw = d_sb.cpu().numpy(), d_sw.cpu().numpy()
    assert [[out[8 * int(b): 8 * int(b + w)].tobytes()] for b, w in zip(sb, sw)] == msgs, shape


def test_packed_message_streams(ctx, oracle):
    """A stream of 5 messages, then 6,000 in about 15 KiB: more than a message
    per 64 packed bytes + 1,024, so the chain runs short of entries and the
    call regrows `ms_buf` to the count it found and runs the chain again."""
    data, msgs, _ = _packed_message_stream(6000, 32)
    assert len(msgs) > len(data) // 64 + 1024 + (len(data) // 64 + 1024) // 4
    _in_turn(lambda s: _check_packed_message_stream(ctx, s), (5, 31), (6000, 32))


# ---- cpk_encode_message_stream ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _unpacked_message_stream(nm, seed):
    """nm messages of 3 segments as Serialize.write lays them out -> (words,
    oracle's packed bytes, piece offsets, each message's first piece, largest
    piece in words)."""
    import oracle
    msgs = _messages(nm, seed)
    pieces = [p for m in msgs for p in [_table([len(s) // 8 for s in m])] + m]
    words = np.frombuffer(b"".join(pieces), np.uint64).copy()
    pk, off = oracle.pack_batch(words.view(np.uint8), _swo([len(p) // 8 for p in pieces]), threads=8)
    assert pk.tobytes() == b"".join(oracle.write_message(m) for m in msgs)
    return words, pk.tobytes(), [int(v) for v in off], list(range(0, 4 * nm + 1, 4)), max(len(p) // 8 for p in pieces)


def _check_unpacked_message_stream(ctx, shape):
    import torch
    words, pk, off, mp, largest = _unpacked_message_stream(*shape)
    d_in = _dev(words)
    cap = npieces = nm = -1
    for _ in range(3):  # (sized by the CPK_ENOMEM protocol: the arrays, then the bytes)
        d_out = torch.zeros(max(cap, 16), dtype=torch.uint8, device="cuda")
        d_off = torch.full((npieces + 1,), -1, dtype=torch.int64, device="cuda")
        d_mp = torch.full((nm + 1,), -1, dtype=torch.int64, device="cuda")
        rc, info = ctx.encode_message_stream(d_in, len(words), d_out if cap > 0 else None,
                                             d_off if npieces >= 0 else None, d_mp if nm >= 0 else None, LIMIT)
        if rc != ENOMEM:
            break
        if npieces < 0:
            npieces, nm = info[1], info[0]
        else:
            cap = info[3]
    assert rc == OK, (rc, info)
    assert info == [len(mp) - 1, len(off) - 1, len(words), len(pk), OK, largest], shape
    assert ctx.take_error() == OK
    assert [int(v) for v in d_mp.cpu().numpy()] == mp, shape
    assert [int(v) for v in d_off.cpu().numpy()] == off, shape
    assert d_out.cpu().numpy()[:len(pk)].tobytes() == pk, shape


def test_unpacked_message_streams(ctx, oracle):
    """4 messages (16 pieces), then 400 (1,600 pieces: past `ems_buf`'s floor of 1,024 offsets)."""
    _in_turn(lambda s: _check_unpacked_message_stream(ctx, s), (4, 41), (400, 42))
