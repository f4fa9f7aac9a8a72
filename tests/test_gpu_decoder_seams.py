"""Decoder seam parity: records placed on purpose at every edge of the
decoders' own geometry, through every decoder form, against the oracle bit
for bit (tests/_packed_records.py builds the corpora; tests/
test_packed_records.py pins them on the CPU and checks their coverage).

  block map / dense   decode_map.hip     windows of kWin packed bytes, lane
                                         chunks, the kDecLook look-ahead, rounds
                                         of kRound words, kBlk-word blocks, the
                                         check reach, the serial walk's cap
  record index        decode_v2.hip      windows of kD2Win bytes cut at kD2NI
                                         records, rounds of kD2Round words
  workgroup reader    decode_mw.hip      the windows over kMwWaves waves
  parallel stream     stream_split.hip   kSsBlock-byte blocks in groups of
                                         kSsGroup

A case is named seam/record kind/offset/fill style, e.g.
win3584/F255/tag@-1/mid/tail40, and a failure lists the first names.  The
expected words, statuses and consumed bytes are the oracle's alone
(PackedInputStream.java:82-134 accepts any sequence of records, so the
streams the encoder never writes -- 00 00 00 00, back-to-back ff .. 00,
all-zero literal words -- are decoded like any other).
"""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import _packed_records as R
from test_gpu_stream import _oracle_stream

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
# What several tests reuse (every entry serves all three ctx parametrisations):
# each corpus as batch arrays with the oracle's answer, and the streams with
# the oracle's walk.  Dropped, with the corpora, when the module is done.
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    _cache.clear()
    R.release()


def _corpus(name):
    return R.corpora()[name]


def _expected(oracle, name):
    """(words, statuses) of a corpus as one batch, from the oracle, once."""
    if name not in _cache:
        packed, in_off, swo = R.batch_arrays(_corpus(name))
        out, st = oracle.unpack_batch(packed, in_off, swo, threads=8)
        _cache[name] = (packed, in_off, swo, out, st)
    return _cache[name]


def _compare(cases, swo, got, st, want, ost):
    """Statuses equal to the oracle's, and the words of every piece it
    accepts; the message names the first failing cases."""
    bad = [f"{c.name}: status {R.STATUS.get(int(s), int(s))}, expected {R.STATUS[int(o)]}"
           for c, s, o in zip(cases, st, ost) if s != o]
    assert not bad, (len(bad), bad[:8])
    if (ost == 0).all():
        if np.array_equal(got, want):
            return
    for i, c in enumerate(cases):
        a, b = 8 * int(swo[i]), 8 * int(swo[i + 1])
        if ost[i] == 0 and not np.array_equal(got[a:b], want[a:b]):
            bad.append(f"{c.name}: word {int(np.argmax(got[a:b] != want[a:b])) // 8} of {c.nwords}")
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_batch_decode_host(ctx, oracle, name):
    """Each corpus as one cpk_decode_host batch, through the default decoder
    choice, the record index forced and the block map forced."""
    packed, in_off, swo, want, ost = _expected(oracle, name)
    got, st = ctx.decode_host(packed, in_off, swo)
    _compare(_corpus(name), swo, got, st, want, ost)


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_batch_decode_device(ctx, oracle, name):
    """Each corpus through device-resident cpk_decode_batch (dec_gate_kernel
    picks the form when none is forced; the corpora of a few pieces also
    try the one-stream decode of few-piece batches first)."""
    import torch
    packed, in_off, swo, want, ost = _expected(oracle, name)
    n = len(swo) - 1
    d_pk = torch.zeros((len(packed) + 64 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_pk[: len(packed)] = torch.from_numpy(packed.copy())
    d_off = torch.from_numpy(in_off.astype(np.int64)).cuda()
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_out = torch.zeros(int(swo[-1]) + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    ctx.decode_batch(d_pk, d_off, d_swo, d_out, d_st)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()[: int(swo[-1])].view(np.uint8)
    _compare(_corpus(name), swo, got, d_st.cpu().numpy(), want, ost)


def _dense_counters(oracle, cases):
    """(windows walked serially, walks given back) by the dense form over the
    cases as one device batch, from the diagnostics library in a child
    process (tests/_dense_windows_probe.py, which also checks the words)."""
    packed, in_off, swo = R.batch_arrays(cases)
    assert R.gate_of(cases) == "dense"
    data, st = oracle.unpack_batch(packed, in_off, swo, threads=8)
    assert (st == 0).all()
    diag = REPO / "capnproto-java_amd" / "lib" / "libcapnp_packed_hip_diag.so"
    assert diag.exists(), "diagnostics library not built (build_native.build_diag)"
    with tempfile.TemporaryDirectory() as td:
        for k, v in (("pk", packed), ("off", in_off), ("swo", swo), ("data", data)):
            np.save(Path(td) / f"{k}.npy", v)
        env = {k: v for k, v in os.environ.items() if k not in ("CPK_DECODER", "CPK_ENCODER")}
        r = subprocess.run([sys.executable, str(REPO / "tests" / "_dense_windows_probe.py"), td],
                           capture_output=True, text=True, timeout=120, env=dict(env, CPK_LIB=str(diag)))
    assert r.returncode == 0, r.stdout + r.stderr
    ser, back = (int(x) for x in r.stdout.split("dense_windows")[1].split())
    return ser, back


def test_dense_form_walks_and_gives_back(oracle):
    """The dense corpora really take the serial walk (decode_body<.., kSerial>):
    the later-window pieces and the windows of kDecSerMax - 1 and kDecSerMax
    records are walked by one lane; every window of kDecSerMax + 1 records
    is given back to the parallel path (++nrec > kDecSerMax)."""
    cnt = _corpus("count/dense")
    keep = [c for c in cnt if f"records{R.kDecSerMax + 1}/" not in c.name]
    over = [c for c in cnt if f"records{R.kDecSerMax + 1}/" in c.name]
    assert len(keep) == 8 and len(over) == 4
    ser, back = _dense_counters(oracle, _corpus("later/dense") + keep)
    assert ser >= len(_corpus("later/dense")) + len(keep), (ser, back)
    ser, back = _dense_counters(oracle, over)
    assert back >= len(over), (ser, back)


# ---- stream forms ------------------------------------------------------------
def _stream(oracle, splice=None):
    """The valid first-window and non-canonical pieces as one stream with
    3000 random bytes behind it (and optionally one malformed case spliced
    in as piece number splice) -> (bytes, swo, cases, oracle's walk)."""
    key = ("stream", splice)
    if key not in _cache:
        cases = R.stream_of([c for s in R.STYLES for c in _corpus(f"first/{s}")] + _corpus("noncanon"))
        if splice is not None:
            bad = next(c for c in _corpus("endbad/dense") if c.name == "end/F255/reach+0/dense/words-1")
            at = {"first": 0, "middle": len(cases) // 2, "last": len(cases)}[splice]
            cases = cases[:at] + [bad] + cases[at:]
        tail = bytes(np.random.default_rng(5).integers(0, 256, size=3000, dtype=np.uint8))
        stream = b"".join(c.packed for c in cases) + tail
        swo = R.batch_arrays(cases)[2]
        if splice is not None:  # (only one spliced stream is kept; each ctx run rebuilds it)
            for k in [k for k in _cache if k[0] == "stream" and k[1] not in (None, splice)]:
                del _cache[k]
        _cache[key] = (stream, swo, cases, _oracle_stream(oracle, stream, swo))
    return _cache[key]


def _compare_stream(cases, swo, got, bounds, st, walk):
    ost, obounds, oout = walk
    bad = [f"{c.name}: status {R.STATUS.get(int(s), int(s))}, expected {R.STATUS[int(o)]}"
           for c, s, o in zip(cases, st, ost) if s != o]
    assert not bad, (len(bad), bad[:8])
    good = int(np.argmax(ost != 0)) if (ost != 0).any() else len(ost)
    assert good == len(obounds) - 1
    bad = [f"{cases[i].name}: ends at {int(bounds[i + 1])}, expected {obounds[i + 1]}"
           for i in range(good) if int(bounds[i + 1]) != obounds[i + 1]]
    assert not bad and int(bounds[0]) == 0, (len(bad), bad[:8])
    want = np.frombuffer(b"".join(oout), np.uint8)
    n = 8 * int(swo[good])
    if not np.array_equal(got[:n], want[:n]):
        for i in range(good):
            a, b = 8 * int(swo[i]), 8 * int(swo[i + 1])
            if not np.array_equal(got[a:b], want[a:b]):
                bad.append(cases[i].name)
        assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("way", ["parallel", "one-wave", "device"])
def test_stream_forms(ctx, oracle, way):
    """The pieces back to back, boundaries unknown: the parallel block path
    on its own (CPK_STREAM_NO_FALLBACK), the one-wave decoder, and
    device-resident cpk_decode_stream find the oracle's boundaries, statuses
    and words."""
    stream, swo, cases, walk = _stream(oracle)
    assert (walk[0] == 0).all() and walk[1][-1] == len(stream) - 3000
    arr = np.frombuffer(stream, np.uint8)
    if way == "device":
        import torch
        d_pk = torch.zeros((len(stream) + 64 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_pk[: len(stream)] = torch.from_numpy(arr.copy())
        d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
        d_out = torch.zeros(int(swo[-1]) + 1, dtype=torch.int64, device="cuda")
        d_io = torch.zeros(len(swo), dtype=torch.int64, device="cuda")
        d_st = torch.full((len(swo) - 1,), 99, dtype=torch.int32, device="cuda")
        ctx.decode_stream(d_pk, len(stream), d_swo, d_out, d_io, d_st)
        torch.cuda.synchronize()
        got, bounds, st = d_out.cpu().numpy().view(np.uint8), d_io.cpu().numpy(), d_st.cpu().numpy()
    else:
        var = "CPK_STREAM_NO_FALLBACK" if way == "parallel" else "CPK_STREAM_ONE_WAVE"
        os.environ[var] = "1"
        try:
            got, bounds, st = ctx.decode_stream_host(arr, swo)
        finally:
            os.environ.pop(var)
    _compare_stream(cases, swo, got, bounds, st, walk)


@pytest.mark.parametrize("splice", ["first", "middle", "last"])
def test_stream_with_a_failing_piece(ctx, oracle, splice):
    """The same stream with one piece whose last literal run overruns it,
    as piece 0, in the middle and last: it and every later piece carry the
    oracle's status, everything before it is decoded.  Through the default
    cpk_decode_stream_host: the parallel block path gives up on such a
    stream and hands it to the one-wave decoder enqueued behind it, so the
    statuses compared are the one-wave decoder's after that hand-over."""
    stream, swo, cases, walk = _stream(oracle, splice)
    assert (walk[0] != 0).any()
    got, bounds, st = ctx.decode_stream_host(np.frombuffer(stream, np.uint8), swo)
    _compare_stream(cases, swo, got, bounds, st, walk)


# ---- the workgroup reader ------------------------------------------------------
def _table(nwords_per_segment):
    """Serialize.java:256-288: segment count - 1, the sizes, padded to a word."""
    n = len(nwords_per_segment)
    tb = (n - 1).to_bytes(4, "little") + b"".join(int(w).to_bytes(4, "little") for w in nwords_per_segment)
    return tb + b"\0" * (-len(tb) % 8)


@pytest.mark.parametrize("name", ["wrap/dense", "later/dense"])
def test_workgroup_reader_window_edges(ctx, oracle, name):
    """Every wave-wrap piece (18 windows, the probe where the kMwWaves waves
    wrap) and every later-window piece, 100 pieces each, as a stream of its
    own, 6..384 KiB, which the one-workgroup reader takes (decode_mw.hip):
    through cpk_decode_stream_host, and framed as a one-segment message
    through cpk_read_message_host and the device cpk_read_message.  (The
    reader does not depend on the decoder choice; with the record index
    forced the read_message forms take the one-wave decoder instead.)"""
    import torch
    import capnp_packed as cp
    cases = _corpus(name)
    assert len(cases) == 100
    f0 = ctx.small_fallbacks()
    junk = bytes(np.random.default_rng(6).integers(0, 256, size=500, dtype=np.uint8))
    bad = []
    for c in cases:
        assert 6 * 1024 <= len(c.packed) < 384 * 1024
        ost, want, used = oracle.unpack(c.packed + junk, 8 * c.nwords)
        assert ost == 0 and used == len(c.packed)
        swo = np.array([0, c.nwords], np.uint64)
        got, bounds, st = ctx.decode_stream_host(np.frombuffer(c.packed + junk, np.uint8), swo)
        if st[0] != 0 or int(bounds[1]) != used or got.tobytes() != want:
            bad.append(c.name + " (stream)")
        msg = oracle.pack(_table([c.nwords])) + c.packed
        mst, msegs, mused = oracle.read_message(msg + junk)
        assert mst == 0 and msegs == [want] and mused == len(msg)
        rst, rsegs, rused, _ = ctx.read_message_host(np.frombuffer(msg + junk, np.uint8))
        if rst != 0 or rsegs != msegs or rused != mused:
            bad.append(c.name + " (read_message_host)")
        data = np.frombuffer(msg + junk, np.uint8)
        d_pk = torch.zeros((len(data) + 64 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_pk[: len(data)] = torch.from_numpy(data.copy())
        d_out = torch.zeros(c.nwords + cp.MSG_HEAD_WORDS, dtype=torch.int64, device="cuda")
        d_info = torch.zeros(cp.MSG_INFO_WORDS, dtype=torch.int64, device="cuda")
        ctx.read_message(d_pk, len(data), d_out, d_info)
        torch.cuda.synchronize()
        info = d_info.cpu().numpy()
        out = d_out.cpu().numpy().view(np.uint8)
        if [int(x) for x in info[:4]] != [0, mused, 1, c.nwords] or \
                out[8 * int(info[4]): 8 * int(info[5])].tobytes() != want:
            bad.append(c.name + " (read_message)")
    assert not bad, (len(bad), bad[:8])
    assert ctx.small_fallbacks() == f0


# ---- messages ----------------------------------------------------------------
def test_messages_of_window_edge_segments(ctx, oracle):
    """64 first-window pieces with the probe within two bytes of byte kWin,
    as the segments of 16 messages: through cpk_decode_messages_host (known
    message ranges) and cpk_decode_message_stream_host (whose flat block
    decode has kSsBlock-byte edges again), against the oracle's
    Serialize.read."""
    pick = [c for s in R.STYLES for c in _corpus(f"first/{s}")
            if c.name.startswith(f"win{R.kWin}/") and abs(c.tag - R.kWin) <= 2]
    pick = pick[:: len(pick) // 64][:64]
    assert len(pick) == 64 and len({c.kind for c in pick}) == len(R.PROBES)
    msgs, want = [], []
    for m in range(16):
        segs = pick[4 * m: 4 * m + 4]
        msg = oracle.pack(_table([c.nwords for c in segs])) + b"".join(c.packed for c in segs)
        ost, osegs, used = oracle.read_message(msg)
        assert ost == 0 and used == len(msg)
        msgs.append(msg)
        want.append(osegs)
    blob = b"".join(msgs)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    st, got = ctx.decode_messages_host(blob, moff)
    bad = [f"message {m} ({pick[4 * m + j].name})" for m in range(16) for j in range(4)
           if st[m] != 0 or got[m][j] != want[m][j]]
    assert not bad, bad[:8]
    tail_st, sgot, used = ctx.decode_message_stream_host(blob)
    assert used == len(blob) and len(sgot) == 16, (tail_st, used, len(sgot))
    bad = [f"message {m} ({pick[4 * m + j].name})" for m in range(16) for j in range(4) if sgot[m][j] != want[m][j]]
    assert not bad, bad[:8]
