"""Exact packed sizes without encoding (cpk_packed_size_batch /
cpk_packed_size_messages and their host forms): d_out_off is what the encoder
would write, checked against the oracle (oracle.pack, oracle.pack_batch,
oracle.write_message) and the reference's known-answer vectors, never against
the library alone.  The size query ignores CPK_ENCODER: every context of the
`ctx` fixture must give the same answer.  Both size forms run: the wave per
piece walk (ragged and small batches, messages) and the chunk-parallel form
(like-sized pieces of 4 Ki words or more, one piece far larger than the
rest), with its run state handed across 8192-word chunk boundaries."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from _packed_size_cases import boundary_pieces, PIECE_WORDS

pytestmark = pytest.mark.gpu

GOLD = json.loads((Path(__file__).parent / "golden" / "reference_kats.json").read_text())
SENTINEL = 0xA5
PAD = 4096  # sentinel bytes after the capacity
RAGGED = [8192] * 40 + [8191, 17, 4096, 0, 8192]


def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _dev(data, swo):
    import torch
    d = np.frombuffer(bytes(data) + b"\0" * 8, np.uint8) if not isinstance(data, np.ndarray) else \
        np.concatenate([data.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)])
    return torch.from_numpy(d.view(np.int64).copy()).cuda(), torch.from_numpy(swo.astype(np.int64)).cuda()


def _size(ctx, d_in, d_swo, maxw):
    """One size call -> (offsets, take_error(), the input unchanged)."""
    import torch
    before = d_in.clone()
    d_off = torch.full((d_swo.numel(),), -1, dtype=torch.int64, device="cuda")
    ctx.packed_size_batch(d_in, d_swo, maxw, d_off)
    rc = ctx.take_error()
    return d_off.cpu().numpy().astype(np.uint64), rc, bool(torch.equal(before, d_in))


def _piece_offsets(oracle, pieces):
    return np.concatenate([[0], np.cumsum([len(oracle.pack(p)) for p in pieces])]).astype(np.uint64)


@pytest.fixture(scope="module")
def ragged(oracle):
    """cfg -> (data, swo, oracle offsets) of the ragged batch, computed once."""
    out = {}
    swo = _swo(RAGGED)
    for cfg in (2, 3, 4):
        data = oracle.generate(oracle.preset(cfg), swo)
        _, woff = oracle.pack_batch(data, swo, threads=8)
        out[cfg] = (data, swo, np.asarray(woff, dtype=np.uint64))
    return out


@pytest.fixture(scope="module")
def boundary(oracle):
    """The hand-built chunk-boundary pieces as one batch, and their oracle sizes."""
    pcs = boundary_pieces()
    data = np.concatenate([p for _, p in pcs])
    swo = _swo([PIECE_WORDS] * len(pcs))
    want = np.array([len(oracle.pack(p)) for _, p in pcs], dtype=np.uint64)
    return [n for n, _ in pcs], data, swo, want


def _messages(nmsg):
    """The 60- and 300-message generators of test_gpu_capacity.py::test_encode_messages_capacity."""
    rng = np.random.default_rng(77 + nmsg)
    msgs = []
    for i in range(nmsg):
        nseg = int(rng.choice([1, 2, 3, 4, 9]))
        sizes = [int(rng.choice([0, 1, 17, 300, 2000, 9000])) for _ in range(nseg)]
        msgs.append([(rng.integers(0, 256, size=8 * s, dtype=np.uint8)
                      * (rng.random(8 * s) < 0.6)).astype(np.uint8).tobytes() for s in sizes])
    return msgs


def _message_offsets(oracle, msgs):
    """Piece offsets in message order (table, segments) from oracle.pack."""
    woff, o = [0], 0
    for m in msgs:
        tb = ((len(m) - 1) & 0xffffffff).to_bytes(4, "little") + b"".join(
            (len(s) // 8).to_bytes(4, "little") for s in m)
        tb += b"\0" * (-len(tb) % 8)
        for piece in [tb] + m:
            o += len(oracle.pack(piece))
            woff.append(o)
    return np.asarray(woff, dtype=np.uint64)


@pytest.fixture(scope="module", params=[60, 300])
def messages(request, oracle):
    msgs = _messages(request.param)
    woff = _message_offsets(oracle, msgs)
    assert int(woff[-1]) == len(b"".join(oracle.write_message(m) for m in msgs))
    return msgs, woff


# ---- 1. known-answer vectors -------------------------------------------------
def test_known_answer_vectors(ctx):
    import capnp_packed as cp
    kats = GOLD["kats"]
    pieces = [bytes.fromhex(k["unpacked"]) for k in kats]
    swo = _swo([len(p) // 8 for p in pieces])
    d_in, d_swo = _dev(b"".join(pieces), swo)
    off, rc, same = _size(ctx, d_in, d_swo, max(1, int(np.diff(swo.astype(np.int64)).max())))
    assert rc == cp.OK and same
    assert off[0] == 0
    assert [int(x) for x in np.diff(off.astype(np.int64))] == [len(bytes.fromhex(k["packed"])) for k in kats]


# ---- 2. generated ragged batch -------------------------------------------------
@pytest.mark.parametrize("maxw", [8192, 0])
@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_ragged_batch(ctx, ragged, cfg, maxw):
    import torch
    import capnp_packed as cp
    data, swo, woff = ragged[cfg]
    d_in, d_swo = _dev(data, swo)
    off, rc, same = _size(ctx, d_in, d_swo, maxw)
    assert rc == cp.OK and same
    assert np.array_equal(off, woff)
    # ... and what cpk_encode_batch writes on the same context
    d_pk = torch.zeros(cp.batch_capacity(swo), dtype=torch.uint8, device="cuda")
    d_eoff = torch.zeros(len(swo), dtype=torch.int64, device="cuda")
    ctx.encode_batch(d_in, d_swo, maxw, d_pk, d_eoff)
    assert ctx.take_error() == cp.OK
    assert np.array_equal(d_eoff.cpu().numpy().astype(np.uint64), off)


# ---- 3. chunk boundaries ---------------------------------------------------------
def test_chunk_boundaries(ctx, boundary):
    import capnp_packed as cp
    names, data, swo, want = boundary
    d_in, d_swo = _dev(data, swo)
    off, rc, same = _size(ctx, d_in, d_swo, PIECE_WORDS)
    assert rc == cp.OK and same
    got = np.diff(off.astype(np.int64)).astype(np.uint64)
    bad = [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
    assert not bad, bad[:8]
    assert off[0] == 0 and int(off[-1]) == int(want.sum())


# ---- 4. gate edges -----------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[200000, 3, 17], [4095, 4096, 4097, 8193, 16384, 1, 0], "3000-small"],
                         ids=["one-large", "thresholds", "3000-small"])
@pytest.mark.parametrize("hinted", [True, False])
def test_gate_edges(ctx, oracle, sizes, hinted):
    import capnp_packed as cp
    if sizes == "3000-small":
        sizes = [int(x) for x in np.random.default_rng(5).integers(0, 41, size=3000)]
    swo = _swo(sizes)
    data = oracle.generate(oracle.preset(2), swo)
    _, woff = oracle.pack_batch(data, swo, threads=8)
    d_in, d_swo = _dev(data, swo)
    off, rc, same = _size(ctx, d_in, d_swo, max(sizes) if hinted else 0)
    assert rc == cp.OK and same
    assert np.array_equal(off, np.asarray(woff, dtype=np.uint64))


# ---- 5. messages -----------------------------------------------------------------------
def test_messages(ctx, messages):
    import torch
    import capnp_packed as cp
    msgs, woff = messages
    segs = [s for m in msgs for s in m]
    swo = _swo([len(s) // 8 for s in segs])
    mseg = _swo([len(m) for m in msgs])
    d_in, d_swo = _dev(b"".join(segs), swo)
    d_mseg = torch.from_numpy(mseg.astype(np.int64)).cuda()
    before = d_in.clone()
    d_off = torch.full((len(woff),), -1, dtype=torch.int64, device="cuda")
    ctx.packed_size_messages(d_in, d_swo, d_mseg, 9000, d_off)
    assert ctx.take_error() == cp.OK
    assert torch.equal(before, d_in)
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), woff)


# ---- 6. use: allocate exactly ---------------------------------------------------------------
@pytest.mark.parametrize("cfg", [2, 4])
def test_exact_allocation(ctx, oracle, ragged, cfg):
    import torch
    import capnp_packed as cp
    data, swo, woff = ragged[cfg]
    want, _ = oracle.pack_batch(data, swo, threads=8)
    d_in, d_swo = _dev(data, swo)
    off, rc, _ = _size(ctx, d_in, d_swo, 8192)
    assert rc == cp.OK
    total = int(off[-1])
    assert total == int(woff[-1])
    for cap, status in ((total, cp.OK), (total - 1, cp.ENOMEM)):
        d_pk = torch.full((total + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_eoff = torch.zeros(len(swo), dtype=torch.int64, device="cuda")
        ctx.encode_batch_cap(d_in, d_swo, 8192, d_pk, cap, d_eoff)
        assert ctx.take_error() == status
        got = d_pk.cpu().numpy()
        assert (got[cap:] == SENTINEL).all()
        if status == cp.OK:
            assert got[:total].tobytes() == want.tobytes()


# ---- 7. contract --------------------------------------------------------------------------------
def test_piece_over_the_bound_is_reported(ctx, ragged):
    import capnp_packed as cp
    data, swo, woff = ragged[2]
    d_in, d_swo = _dev(data, swo)
    _, rc, same = _size(ctx, d_in, d_swo, 8191)
    assert rc == cp.EINVAL and same
    off, rc, _ = _size(ctx, d_in, d_swo, 8192)  # cleared: the next call is clean
    assert rc == cp.OK and np.array_equal(off, woff)


def test_empty_batch(ctx):
    import torch
    import capnp_packed as cp
    d_in = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_swo = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ctx.packed_size_batch(d_in, d_swo, 8192, d_off)
    assert ctx.take_error() == cp.OK and int(d_off.cpu()[0]) == 0
    d_off.fill_(-1)
    ctx.packed_size_messages(d_in, d_swo, d_swo, 8192, d_off)
    assert ctx.take_error() == cp.OK and int(d_off.cpu()[0]) == 0


# ---- 8. host forms ----------------------------------------------------------------------------------
def test_host_forms(ctx, ragged, messages):
    import torch
    data, swo, woff = ragged[3]
    d_in, d_swo = _dev(data, swo)
    off, _, _ = _size(ctx, d_in, d_swo, 8192)
    assert np.array_equal(ctx.packed_size_host(data, swo), off)
    assert np.array_equal(off, woff)
    msgs, mwoff = messages
    segs = [s for m in msgs for s in m]
    mswo = _swo([len(s) // 8 for s in segs])
    d_min, d_mswo = _dev(b"".join(segs), mswo)
    d_mseg = torch.from_numpy(_swo([len(m) for m in msgs]).astype(np.int64)).cuda()
    d_off = torch.zeros(len(mwoff), dtype=torch.int64, device="cuda")
    ctx.packed_size_messages(d_min, d_mswo, d_mseg, 9000, d_off)
    dev = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(ctx.packed_size_messages_host(msgs), dev)
    assert np.array_equal(dev, mwoff)


def test_host_forms_cross_chunks(oracle, ragged, messages):
    """CPK_HOST_CHUNK_MB=1 on a fresh context: the ~3 MiB batches cross the
    pinned pipeline's chunk boundaries."""
    import capnp_packed as cp
    saved = os.environ.get("CPK_HOST_CHUNK_MB")
    os.environ["CPK_HOST_CHUNK_MB"] = "1"
    c = cp.Context(0)
    try:
        data, swo, woff = ragged[2]
        assert int(swo[-1]) * 8 > 2 * (1 << 20)
        assert np.array_equal(c.packed_size_host(data, swo), woff)
        msgs, mwoff = messages
        assert np.array_equal(c.packed_size_messages_host(msgs), mwoff)
    finally:
        c.close()
        if saved is None:
            os.environ.pop("CPK_HOST_CHUNK_MB")
        else:
            os.environ["CPK_HOST_CHUNK_MB"] = saved
