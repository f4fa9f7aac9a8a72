"""cpk_unpacked_size_batch / _host on the GPU: the words each packed range
unpacks to, without decoding.  What is expected never comes from the library:
the reference vectors' lengths, the record builder's word counts
(tests/_packed_records.py) and the record walk of tests/_unpacked_size_model.py,
which tests/test_unpacked_size_model.py pins to the oracle.  Every call checks
that the packed bytes are unchanged and that nothing is written past
d_seg_word_off[n] and d_status[n - 1].  The packed bytes are followed by 0xFF
up to the 16-byte line the call may read: a tag and a count of 255 wherever a
record is read past its range."""
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _packed_records as R
import _unpacked_size_model as M

pytestmark = pytest.mark.gpu

GOLD = json.loads((Path(__file__).parent / "golden" / "reference_kats.json").read_text())
# pieces of this many bytes and more take the block form (host_api.hip)
kUsBlockMin = R.parse_constant((R.CSRC / "host_api.hip").read_text(), "kUsBlockMin", {})
GUARD = 8  # sentinel entries behind each output array
RAGGED = [8192] * 40 + [8191, 17, 4096, 0, 8192]  # (tests/test_gpu_packed_size.py's batch)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    R.release()
    _model.cache_clear()


def _in_off(pieces):
    return np.concatenate([[0], np.cumsum([len(p) for p in pieces], dtype=np.uint64)]).astype(np.uint64)


def _device_bytes(packed: np.ndarray):
    """The packed bytes on the device, 0xFF behind them to the end of their last 16-byte line."""
    import torch
    buf = np.full((len(packed) + 15) // 16 * 16 + 16, 0xFF, np.uint8)
    buf[:len(packed)] = packed
    return torch.from_numpy(buf).cuda()


def _size(ctx, packed, in_off, d_packed=None):
    """One device call -> (seg_word_off uint64[n+1], status int32[n], d_packed, d_in_off, d_swo)."""
    import torch
    packed = np.frombuffer(packed, np.uint8) if isinstance(packed, (bytes, bytearray)) else packed
    n = len(in_off) - 1
    if d_packed is None:
        d_packed = _device_bytes(packed)
    before = d_packed.clone()
    d_in_off = torch.from_numpy(in_off.astype(np.int64)).cuda()
    d_swo = torch.full((n + 1 + GUARD,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    d_st = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.unpacked_size_batch(d_packed, d_in_off, d_swo[:n + 1], d_st)
    torch.cuda.synchronize()
    assert torch.equal(before, d_packed), "the packed bytes were written"
    swo, st = d_swo.cpu().numpy(), d_st.cpu().numpy()
    assert (swo[n + 1:] == -0x5A5A5A5A5A5A5A5B).all(), "written past d_seg_word_off[n]"
    assert (st[n:] == 0x5A5A5A5A).all(), "written past d_status[n - 1]"
    return swo[:n + 1].astype(np.uint64), st[:n].copy(), d_packed, d_in_off, d_swo


def _host(ctx, packed, in_off):
    """cpk_unpacked_size_host -> (return value, seg_word_off, status)."""
    packed = np.ascontiguousarray(np.frombuffer(packed, np.uint8) if isinstance(packed, (bytes, bytearray)) else packed)
    io = np.ascontiguousarray(in_off, dtype=np.uint64)
    n = len(io) - 1
    swo = np.full(n + 1 + GUARD, 0xA5A5A5A5A5A5A5A5, np.uint64)
    st = np.full(n + GUARD, 0x5A5A5A5A, np.int32)
    rc = ctx._lib.cpk_unpacked_size_host(ctx.handle, packed.ctypes.data if packed.size else None, io.ctypes.data, n,
                                         swo.ctypes.data, st.ctypes.data)
    assert (swo[n + 1:] == 0xA5A5A5A5A5A5A5A5).all() and (st[n:] == 0x5A5A5A5A).all()
    return rc, swo[:n + 1], st[:n]


def _expect(pieces):
    """The model's (seg_word_off, status) for the pieces as one batch."""
    res = [M.unpacked_size(p) for p in pieces]
    swo = np.concatenate([[0], np.cumsum([w for _, w in res], dtype=np.uint64)]).astype(np.uint64)
    return swo, np.array([s for s, _ in res], np.int32)


@lru_cache(maxsize=None)
def _model(name):
    """The model over a malformed corpus, once for all contexts (pieces that share their bytes walked once)."""
    seen = {}
    res = []
    for c in R.corpora()[name]:
        if c.packed not in seen:
            seen[c.packed] = M.unpacked_size(c.packed)
        res.append(seen[c.packed])
    swo = np.concatenate([[0], np.cumsum([w for _, w in res], dtype=np.uint64)]).astype(np.uint64)
    return swo, np.array([s for s, _ in res], np.int32)


@lru_cache(maxsize=None)
def _prefix_batch():
    pieces = [pre for p in M.hand_built() for pre in M.prefixes(p)]
    return pieces, _in_off(pieces), _expect(pieces)


@lru_cache(maxsize=None)
def _ragged(cfg):
    import oracle
    swo = np.concatenate([[0], np.cumsum(np.asarray(RAGGED, dtype=np.uint64))]).astype(np.uint64)
    data = oracle.generate(oracle.preset(cfg), swo)
    pk, off = oracle.pack_batch(data, swo, threads=8)
    return data, swo, np.asarray(pk), np.asarray(off, dtype=np.uint64)


def _forced(monkeypatch, form):
    import capnp_packed as cp
    monkeypatch.setenv("CPK_USIZE_FORM", form)
    return cp.Context(0)


# ---- 1. known-answer vectors -------------------------------------------------
def test_known_answer_vectors(ctx):
    kats = GOLD["kats"]
    pieces = [bytes.fromhex(k["packed"]) for k in kats]
    swo, st, *_ = _size(ctx, b"".join(pieces), _in_off(pieces))
    assert (st == 0).all()
    assert swo[0] == 0
    assert [int(x) for x in np.diff(swo.astype(np.int64))] == [len(bytes.fromhex(k["unpacked"])) // 8 for k in kats]


# ---- 2. the decoder seam corpora ---------------------------------------------
def test_geometry_needs_no_sweep_of_its_own():
    # (records are swept across the 3584- and 3072-byte window edges by the corpora)
    assert M.kUsWin in (R.kWin, R.kD2Win)


@pytest.mark.parametrize("name", R.VALID)
def test_valid_corpora(ctx, name):
    cases = R.corpora()[name]
    packed, in_off, want = R.batch_arrays(cases)
    if name.startswith("first/"):
        assert R.in_off_phases(cases) == set(range(16))
    swo, st, *_ = _size(ctx, packed, in_off)
    bad = np.nonzero(st != 0)[0]
    assert bad.size == 0, [(cases[i].name, int(st[i])) for i in bad[:5]]
    diff = np.nonzero(np.diff(swo.astype(np.int64)) != np.diff(want.astype(np.int64)))[0]
    assert diff.size == 0, [cases[i].name for i in diff[:5]]
    assert np.array_equal(swo, want)


@pytest.mark.parametrize("name", R.MALFORMED)
def test_malformed_corpora(ctx, name):
    cases = R.corpora()[name]
    packed, in_off, _ = R.batch_arrays(cases)
    want_swo, want_st = _model(name)
    assert (want_st == M.ETRUNC).any()  # (the words-1 / words+1 cases of endbad are whole ranges: OK here)
    swo, st, *_ = _size(ctx, packed, in_off)
    diff = np.nonzero(st != want_st)[0]
    assert diff.size == 0, [(cases[i].name, int(st[i]), int(want_st[i])) for i in diff[:5]]
    assert np.array_equal(swo, want_swo)


# ---- 3. every prefix: the end-of-piece rule against the bytes behind the range ----
def test_every_prefix(ctx):
    pieces, in_off, (want_swo, want_st) = _prefix_batch()
    assert len(pieces) > 900
    swo, st, *_ = _size(ctx, b"".join(pieces), in_off)
    diff = np.nonzero(st != want_st)[0]
    assert diff.size == 0, [(int(i), len(pieces[i]), int(st[i]), int(want_st[i])) for i in diff[:8]]
    assert np.array_equal(swo, want_swo)


# ---- 4. edges ----------------------------------------------------------------------
def test_empty_pieces_among_full_ones(ctx):
    full = [bytes.fromhex(k["packed"]) for k in GOLD["kats"] if k["packed"]][:3]
    pieces = [b"", full[0], b"", b"", full[1], full[2], b""]
    want_swo, want_st = _expect(pieces)
    swo, st, *_ = _size(ctx, b"".join(pieces), _in_off(pieces))
    assert (st == 0).all() and (want_st == 0).all()
    assert np.array_equal(swo, want_swo)


def test_no_pieces(ctx):
    swo, st, *_ = _size(ctx, b"", np.zeros(1, np.uint64))
    assert swo.tolist() == [0] and st.size == 0


def test_one_byte(ctx):
    swo, st, *_ = _size(ctx, b"\x00", np.array([0, 1], np.uint64))
    assert swo.tolist() == [0, 0] and st.tolist() == [M.ETRUNC]


@pytest.mark.parametrize("count", [1, 40])
def test_whole_windows_of_literal_runs(ctx, count):
    rng = R._rng("usize-f255", count)
    piece = b"".join(R.rand_F(rng, 255).packed for _ in range(count))
    swo, st, *_ = _size(ctx, piece, np.array([0, len(piece)], np.uint64))
    assert st.tolist() == [0] and swo.tolist() == [0, 256 * count]
    swo, st, *_ = _size(ctx, piece[:-3], np.array([0, len(piece) - 3], np.uint64))
    assert st.tolist() == [M.ETRUNC] and swo.tolist() == [0, 0]


# ---- 5. size -> decode, with no synchronisation in between --------------------------
@pytest.mark.parametrize("cfg", [2, 4])
def test_round_trip(ctx, cfg):
    import torch
    data, swo, pk, off = _ragged(cfg)
    n = len(swo) - 1
    d_packed = _device_bytes(pk)
    before = d_packed.clone()
    d_in_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_swo = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    d_st = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(int(swo[-1]) + 8, dtype=torch.int64, device="cuda")
    d_st2 = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.unpacked_size_batch(d_packed, d_in_off, d_swo[:n + 1], d_st)
    ctx.decode_batch(d_packed, d_in_off, d_swo[:n + 1], d_out, d_st2)  # (the device's offsets, not read back)
    torch.cuda.synchronize()
    assert torch.equal(before, d_packed)
    assert (d_swo[n + 1:] == -7).all() and (d_st[n:] == 0x5A5A5A5A).all()
    assert np.array_equal(d_swo[:n + 1].cpu().numpy().astype(np.uint64), swo)
    assert (d_st[:n] == 0).all() and (d_st2 == 0).all()
    assert d_out[:int(swo[-1])].cpu().numpy().tobytes() == bytes(data)


# ---- 6. the block form ----------------------------------------------------------------
@lru_cache(maxsize=None)
def _block_pieces():
    """Four large pieces, each starting on a 16-byte line (small filler
    pieces in between): three groups of blocks; the same with an F(255)
    astride each group edge; the first cut inside its last record; just over
    64 groups (ss_top's second round)."""
    g = R.kSsBlock * R.kSsGroup
    a = R.filled(2 * g + 300, "dense").packed
    f = R.probe("F255").packed
    b = R.filled(g - 1000, "dense", 1).packed + f
    b += R.filled(2 * g - 1000 - len(b), "dense", 2).packed + f + R.filled(300, "dense", 3).packed
    assert len(b) > 2 * g and b[g - 1000] == 0xFF and b[2 * g - 1000] == 0xFF
    c = a[:-1]
    d = R.filled(64 * g + 300, "dense", 4).packed
    pieces, large = [], []
    for p in (a, b, c, d):
        pos = sum(len(x) for x in pieces)
        if pos % 16:
            pad = 16 - pos % 16
            pieces.append(R.filled(pad if pad >= 2 else 17, "mid", 5).packed)
        assert sum(len(x) for x in pieces) % 16 == 0
        large.append(len(pieces))
        pieces.append(p)
    assert len(pieces) <= 32
    return pieces, large, _in_off(pieces), _expect(pieces)


def test_block_form_and_wave_form_agree(monkeypatch):
    pieces, large, in_off, (want_swo, want_st) = _block_pieces()
    assert [int(want_st[i]) for i in large] == [0, 0, M.ETRUNC, 0]
    packed = np.frombuffer(b"".join(pieces), np.uint8)
    got = {}
    for form in ("1", "2"):
        c = _forced(monkeypatch, form)
        try:
            swo, st, *_ = _size(c, packed, in_off)
        finally:
            c.close()
        assert st.tolist() == want_st.tolist(), form
        assert np.array_equal(swo, want_swo), form
        got[form] = (swo, st)
    assert np.array_equal(got["1"][0], got["2"][0]) and np.array_equal(got["1"][1], got["2"][1])


# ---- 7. the host form ------------------------------------------------------------------
def _host_batches():
    pieces, in_off, _ = _prefix_batch()
    _, _, pk, off = _ragged(2)
    return [("prefixes", np.frombuffer(b"".join(pieces), np.uint8), in_off), ("ragged", pk, off)]


def test_host_form(ctx, monkeypatch):
    import capnp_packed as cp
    for name, packed, in_off in _host_batches():
        swo, st, *_ = _size(ctx, packed, in_off)
        first = next((int(s) for s in st if s != 0), 0)
        rc, hswo, hst = _host(ctx, packed, in_off)
        assert rc == first, name
        assert np.array_equal(hswo, swo) and np.array_equal(hst, st), name
        with monkeypatch.context() as mp:
            mp.setenv("CPK_HOST_CHUNK_MB", "1")  # (pieces over several chunks, offsets rebased per chunk)
            assert int(in_off[-1]) > 1 << 20
            c = cp.Context(0)
            try:
                rc, hswo, hst = _host(c, packed, in_off)
            finally:
                c.close()
        assert rc == first, name
        assert np.array_equal(hswo, swo) and np.array_equal(hst, st), name


def test_host_form_takes_a_large_piece_by_the_block_map(ctx):
    """A piece over the block form's threshold at the front of its chunk, and the same cut short."""
    unit = R.filled(3 * R.kSsBlock * R.kSsGroup + 300, "dense", 7).packed
    piece = unit * (kUsBlockMin // len(unit) + 1)
    for p in (piece, piece[:-1]):
        want_swo, want_st = _expect([p])
        rc, swo, st = _host(ctx, p, np.array([0, len(p)], np.uint64))
        assert rc == int(want_st[0])
        assert np.array_equal(swo, want_swo) and st.tolist() == want_st.tolist()
