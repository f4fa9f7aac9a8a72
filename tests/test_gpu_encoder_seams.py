"""Encoder seam parity: runs planted on purpose at every edge of the two-pass
encoder's own geometry (csrc/encode_v4.hip: 64-word steps, groups of 64
steps, the 192-word limit of the lane-parallel roles, the zero-run cap
phase, four rows of look-ahead for a head's count, the 2 KiB output ring and
its overhang line, the loads' prefetch batches), through every encoder form,
against the oracle bit for bit (tests/_encoder_seams.py builds the corpora;
tests/test_encoder_seams_corpus.py pins them on the CPU).

  1  two passes, device-resident   encode_batch, CPK_ENCODER=4: the stride row
                                   layout (hint = largest piece), rows packed
                                   by word offset (hint 0), and hint 0 with
                                   seg_word_off[0] = 129
  2  two passes from host memory   encode_host, CPK_ENCODER=4, CPK_NO_SMALL
                                   (without it small_ok(), host_pipe.hip:232,
                                   hands every small host batch to
                                   sp_small_kernel whatever CPK_ENCODER says)
  3  the default choice            device-resident and host: the gate decides
  4  message batches               encode_messages, four segments a message,
                                   the segments largest first (order[])
  5  size query, wave form         e4_size_kernel<false>, CPK_SIZE_FORM=wave
  6  the one-workgroup kernel and the forced single pass

A case is named seam/kind/position/length, e.g.
grp4096/dense+L/enter193@+0/len600; a failure lists the first names with the
byte offset inside the piece.  The device output buffer is filled with 0xA5
first and every byte past the last piece must still be 0xA5.  Every encode
is decoded back by the default decoder.
"""
import os

import numpy as np
import pytest

import _encoder_seams as S

pytestmark = pytest.mark.gpu

# per corpus: the batch arrays and the oracle's answer, computed once
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    _cache.clear()
    S.release()


def _expected(oracle, name):
    """(cases, data, swo, packed, offsets) of a corpus as one batch."""
    if name not in _cache:
        cases = S.corpora()[name]
        data, swo = S.batch_arrays(cases)
        opk, ooff = oracle.pack_batch(data, swo, threads=8)
        _cache[name] = (cases, data, swo, opk, ooff)
    return _cache[name]


def _make_ctx(**env):
    """A context created under the given variables (CPK_ENCODER and
    CPK_SIZE_FORM are read at creation), the others of them unset."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    keys = ("CPK_ENCODER", "CPK_SP_FORM", "CPK_SIZE_FORM", "CPK_E4_ORDER")
    saved = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return cp.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def two_pass_ctx():
    c = _make_ctx(CPK_ENCODER="4")
    yield c
    c.close()


@pytest.fixture(scope="module")
def single_pass_ctx():
    c = _make_ctx(CPK_ENCODER="0")
    yield c
    c.close()


@pytest.fixture(scope="module")
def default_ctx():
    c = _make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def wave_size_ctx():
    c = _make_ctx(CPK_SIZE_FORM="wave")
    yield c
    c.close()


@pytest.fixture
def pipeline(monkeypatch):
    """Host calls stay off the one-workgroup kernel, on the default chunks."""
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    monkeypatch.delenv("CPK_HOST_CHUNK_KB", raising=False)
    monkeypatch.delenv("CPK_HOST_CHUNK_MB", raising=False)


def _diff_report(cases, ooff, pk, opk, off):
    """The first eight pieces that differ, by name, with the byte offset
    inside the piece (or the sizes, where those differ)."""
    bad = []
    if not np.array_equal(off, ooff):
        sz, osz = np.diff(off.astype(np.int64)), np.diff(ooff.astype(np.int64))
        bad = [f"{cases[i].name}: {int(sz[i])} bytes, expected {int(osz[i])}" for i in np.nonzero(sz != osz)[0][:8]]
        return f"piece sizes differ: {bad}" if bad else f"offsets differ from {int(off[0])} / {int(ooff[0])}"
    m = min(len(pk), len(opk))
    at = np.nonzero(pk[:m] != opk[:m])[0]
    if at.size == 0:
        return f"lengths {len(pk)} / {len(opk)}"
    pc = np.searchsorted(ooff, at, side="right") - 1
    seen = []
    for b, p in zip(at, pc):
        if p not in [q for q, _ in seen]:
            seen.append((int(p), int(b)))
        if len(seen) == 8:
            break
    first = [f"{cases[p].name} +{b - int(ooff[p])}: got {bytes(pk[b:b + 12]).hex()} want {bytes(opk[b:b + 12]).hex()}"
             for p, b in seen]
    return f"{at.size} bytes differ in {len(set(pc.tolist()))} pieces; first: {first}"


def _compare(cases, ooff, opk, pk, off):
    off = np.asarray(off).astype(np.uint64)
    assert np.array_equal(off, ooff) and np.array_equal(pk, opk), _diff_report(cases, ooff, pk, opk, off)


def _decode_back(dec_ctx, cases, pk, off, swo, data):
    """The default decoder reads the encoder's bytes back to the words."""
    dec, st = dec_ctx.decode_host(pk, off, swo)
    bad = [c.name for c, s in zip(cases, st) if s != 0]
    assert not bad, (len(bad), bad[:8])
    if not np.array_equal(dec, data):
        bad = [c.name for i, c in enumerate(cases)
               if not np.array_equal(dec[8 * int(swo[i]):8 * int(swo[i + 1])], c.words)]
        assert not bad, (len(bad), bad[:8])


FILL = 0xA5


def _device_batch(data, swo, lead=0):
    """The words on the device, preceded by `lead` unused words (all ones),
    seg_word_off moved with them, and an output buffer of 0xA5."""
    import torch
    import capnp_packed as cp
    w = np.full(lead + data.size // 8 + 1, -1, np.int64)
    w[lead:lead + data.size // 8] = data.view(np.int64)
    d_in = torch.from_numpy(w).cuda()
    d_swo = torch.from_numpy((swo + np.uint64(lead)).astype(np.int64)).cuda()
    cap = (cp.batch_capacity(swo) + 15) // 16 * 16
    d_pk = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(len(swo), dtype=torch.int64, device="cuda")
    return d_in, d_swo, d_pk, d_off


def _encode_device(c, data, swo, hint, lead=0):
    """-> (packed bytes, offsets); asserts the buffer past them untouched."""
    import capnp_packed as cp
    d_in, d_swo, d_pk, d_off = _device_batch(data, swo, lead)
    c.encode_batch(d_in, d_swo, hint, d_pk, d_off)
    assert c.take_error() == cp.OK
    off = d_off.cpu().numpy().astype(np.uint64)
    out = d_pk.cpu().numpy()
    end = int(off[-1])
    assert end <= out.size and (out[end:] == FILL).all(), \
        f"{int((out[end:] != FILL).sum())} bytes written past the last piece, first at +{int(np.argmax(out[end:] != FILL))}"
    return out[:end], off


def _encode_host(c, data, swo):
    import capnp_packed as cp
    out = np.full(cp.batch_capacity(swo), FILL, np.uint8)
    pk, off = c.encode_host(data, swo, out=out)
    assert (out[int(off[-1]):] == FILL).all(), "bytes written past the last piece"
    return pk, off


def _hint(swo):
    return max(int(np.diff(swo.astype(np.int64)).max()), 1)


# ---- 1: the two passes, device-resident ----------------------------------------
@pytest.mark.parametrize("rows", ["stride", "by-word-offset", "by-word-offset+129"])
@pytest.mark.parametrize("name", S.CORPORA)
def test_two_pass_device(two_pass_ctx, default_ctx, oracle, name, rows):
    """e4_size_kernel<true> + e4_emit_kernel on each corpus as one batch: the
    size pass's rows `stride` per piece (hint = the largest piece), packed by
    (w0 - swo[0]) / 64 + seg (hint 0), and the latter with 129 unused words
    before the first piece."""
    cases, data, swo, opk, ooff = _expected(oracle, name)
    hint = _hint(swo) if rows == "stride" else 0
    pk, off = _encode_device(two_pass_ctx, data, swo, hint, lead=129 if rows.endswith("+129") else 0)
    _compare(cases, ooff, opk, pk, off)
    if rows == "stride":
        _decode_back(default_ctx, cases, pk, off, swo, data)


# ---- 2: the two passes from host memory ------------------------------------------
@pytest.mark.parametrize("name", S.CORPORA)
def test_two_pass_host(two_pass_ctx, default_ctx, oracle, name, pipeline):
    cases, data, swo, opk, ooff = _expected(oracle, name)
    f0 = two_pass_ctx.small_fallbacks()
    pk, off = _encode_host(two_pass_ctx, data, swo)
    _compare(cases, ooff, opk, pk, off)
    assert two_pass_ctx.small_fallbacks() == f0
    _decode_back(default_ctx, cases, pk, off, swo, data)


# ---- 3: the default choice ---------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", S.CORPORA)
def test_default_encoder(default_ctx, oracle, name, where, pipeline):
    """No encoder forced: e4_gate_kernel decides (mixed sizes and pieces
    under 4096 words: the two passes; the dense like-sized ones as well)."""
    cases, data, swo, opk, ooff = _expected(oracle, name)
    if where == "device":
        pk, off = _encode_device(default_ctx, data, swo, _hint(swo))
    else:
        pk, off = _encode_host(default_ctx, data, swo)
    _compare(cases, ooff, opk, pk, off)
    _decode_back(default_ctx, cases, pk, off, swo, data)


# ---- 4: message batches ----------------------------------------------------------------
def _messages(oracle, name):
    """The corpus four segments to a message -> (cases, messages, the
    oracle's SerializePacked.write of each)."""
    key = ("msg", name)
    if key not in _cache:
        cases = S.corpora()[name]
        msgs = [[c.words.tobytes() for c in cases[i:i + 4]] for i in range(0, len(cases), 4)]
        _cache[key] = (cases, msgs, [oracle.write_message(m) for m in msgs])
    return _cache[key]


@pytest.mark.parametrize("enc", ["two-pass", "default"])
@pytest.mark.parametrize("name", S.MESSAGE_CORPORA)
def test_message_batches(two_pass_ctx, default_ctx, oracle, name, enc):
    """encode_messages with CPK_ENCODER=4, and with the default encoder for a
    batch of over 1,024 pieces (which takes the two passes): both walk the
    segments largest first.  Expected: the oracle's SerializePacked.write."""
    import torch
    import capnp_packed as cp
    cases, msgs, want = _messages(oracle, name)
    if enc == "default":
        # (the ring corpus is 130 segments: repeated until the batch is over 1,024 pieces)
        rep = -(-1025 // (len(msgs) + len(cases)))
        msgs, want, cases = msgs * rep, want * rep, cases * rep
        assert len(msgs) + len(cases) > 1024
    c = two_pass_ctx if enc == "two-pass" else default_ctx
    segs = [s for m in msgs for s in m]
    swo = np.concatenate([[0], np.cumsum([len(s) // 8 for s in segs])]).astype(np.uint64)
    mseg = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    data = np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8)
    d_in = torch.from_numpy(data.view(np.int64).copy()).cuda()
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_mseg = torch.from_numpy(mseg.astype(np.int64)).cuda()
    cap = cp.batch_capacity(swo) + sum(10 * ((len(m) + 2) // 2 + 1) for m in msgs)
    d_pk = torch.full(((cap + 15) // 16 * 16,), FILL, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(len(msgs) + len(segs) + 1, dtype=torch.int64, device="cuda")
    c.encode_messages(d_in, d_swo, d_mseg, _hint(swo), d_pk, d_off)
    assert c.take_error() == cp.OK
    off = d_off.cpu().numpy().astype(np.int64)
    out = d_pk.cpu().numpy()
    moff = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    got_moff = np.append(off[(mseg[:-1] + np.arange(len(msgs), dtype=np.uint64)).astype(np.int64)], off[-1])
    bad = []
    for m in range(len(msgs)):
        a, b = int(got_moff[m]), int(got_moff[m + 1])
        if b - a != len(want[m]) or out[a:b].tobytes() != want[m]:
            w = np.frombuffer(want[m], np.uint8)
            g = out[a:a + len(w)]
            at = int(np.argmax(g != w)) if len(g) == len(w) and (g != w).any() else -1
            bad.append(f"message {m} ({', '.join(x.name for x in cases[4 * m:4 * m + 4])}): "
                       f"{b - a} bytes, expected {len(w)}, first difference at +{at}")
    assert not bad, (len(bad), bad[:8])
    assert np.array_equal(got_moff, moff) and (out[int(off[-1]):] == FILL).all()
    st, got = default_ctx.decode_messages_host(out[: int(off[-1])].tobytes(), moff.astype(np.uint64),
                                               traversal_limit_words=1 << 26)
    bad = [f"message {m}" for m in range(len(msgs)) if st[m] != 0 or got[m] != msgs[m]]
    assert not bad, (len(bad), bad[:8])


# ---- 5: the size query's wave form ---------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", S.CORPORA)
def test_size_query_wave_form(wave_size_ctx, oracle, name, where, pipeline):
    """packed_size_batch / packed_size_host with CPK_SIZE_FORM=wave:
    e4_size_kernel<false>, the sizes alone, equal the oracle's offsets."""
    import capnp_packed as cp
    cases, data, swo, _, ooff = _expected(oracle, name)
    if where == "device":
        d_in, d_swo, _, d_off = _device_batch(data, swo)
        wave_size_ctx.packed_size_batch(d_in, d_swo, _hint(swo), d_off)
        assert wave_size_ctx.take_error() == cp.OK
        off = d_off.cpu().numpy().astype(np.uint64)
    else:
        off = wave_size_ctx.packed_size_host(data, swo)
    assert np.array_equal(off, ooff), _diff_report(cases, ooff, ooff[:0], ooff[:0], off)


# ---- 6: the one-workgroup kernel and the forced single pass ------------------------------------
def _small_batches(cases):
    """The cases in order, cut into batches of at most kSpSmallPieces pieces
    and kSpSmallWords words."""
    out, cur, words = [], [], 0
    for c in cases:
        assert c.nwords <= S.kSpSmallWords
        if cur and (len(cur) == S.kSpSmallPieces or words + c.nwords > S.kSpSmallWords):
            out.append(cur)
            cur, words = [], 0
        cur.append(c)
        words += c.nwords
    return out + [cur]


@pytest.mark.parametrize("name", S.CORPORA)
def test_small_kernel(default_ctx, oracle, name, monkeypatch):
    """encode_host without CPK_NO_SMALL: sp_small_kernel takes each batch of
    at most 512 pieces and kSpSmallWords words."""
    for v in ("CPK_NO_SMALL", "CPK_HOST_CHUNK_KB", "CPK_HOST_CHUNK_MB"):
        monkeypatch.delenv(v, raising=False)
    cases, data, swo, opk, ooff = _expected(oracle, name)
    f0 = default_ctx.small_fallbacks()
    i = 0
    for batch in _small_batches(cases):
        j = i + len(batch)
        a, b = int(swo[i]), int(swo[j])
        pk, off = _encode_host(default_ctx, data[8 * a:8 * b], swo[i:j + 1] - swo[i])
        _compare(batch, ooff[i:j + 1] - ooff[i], opk[int(ooff[i]):int(ooff[j])], pk, off)
        i = j
    assert i == len(cases) and default_ctx.small_fallbacks() == f0


@pytest.mark.parametrize("name", S.CORPORA)
def test_forced_single_pass(single_pass_ctx, default_ctx, oracle, name):
    """CPK_ENCODER=0, device-resident: sp_encode_kernel for every batch (the
    step2048 cases sit on its wave edges)."""
    cases, data, swo, opk, ooff = _expected(oracle, name)
    pk, off = _encode_device(single_pass_ctx, data, swo, _hint(swo))
    _compare(cases, ooff, opk, pk, off)
    _decode_back(default_ctx, cases, pk, off, swo, data)
