"""Ring pressure on the single-pass encoder (encode_sp.hip), both forms.

A wave of the single pass lays the strings of its steps (64 words each) into
a per-wave LDS ring -- 4,096 bytes in the sparse form, 11,264 in the dense
one -- and streams complete 16-byte lines out once the unit's offset is
known.  A wave whose output does not fit its ring depends on the flush
keeping pace with the layout: what is laid out and not yet stored must never
span more than the ring.  Mostly-zero pieces with one dense stretch are the
inputs that put a wave under that pressure inside a batch the device gate
sends to the small ring, so they are the inputs here: every piece is all zero
words except one stretch, swept over the words that fall inside one wave
(2,048 words: 32 steps; four waves per 8,192-word unit), over the stretch's
place relative to the wave and unit boundaries, and over five kinds of
stretch, each at a known packed-bytes-per-word rate (asserted from the
oracle, so the input is known to press as hard as meant).

Every case is the parity check of test_gpu_parity.py: encode, compare the
offsets and the packed bytes with the oracle bit for bit, decode back.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT = 8192   # words per unit (a workgroup's chunk)
WAVE = 2048   # words per wave of a whole unit
KINDS = ["ff", "rand_d", "d_x", "l_only", "dl_run"]
# just under and over the point where a sparse wave's output passes 4,096
# bytes (at 8 B/word: 512 words), a whole wave, and (1,408 / 1,472) the
# dense form's 11,264 bytes
LENGTHS = [320, 384, 448, 512, 513, 576, 1024, 1408, 1472, 2047, 2048]


def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _stretch(kind, n, rng):
    """n words of one kind, as an (n, 8) byte array."""
    if kind == "ff":            # every byte 0xFF
        return np.full((n, 8), 0xFF, np.uint8)
    w = rng.integers(1, 256, size=(n, 8), dtype=np.uint8)
    if kind == "rand_d":        # all-nonzero words: a lost or OR-ed byte shows as a wrong value
        return w
    if kind == "d_x":           # all-nonzero word, word with exactly two zero bytes, ...
        for i in range(1, n, 2):
            w[i, rng.choice(8, size=2, replace=False)] = 0
        return w
    if kind == "l_only":        # exactly one zero byte in every word, no 0xFF head anywhere
        w[np.arange(n), rng.integers(0, 8, size=n)] = 0
        return w
    assert kind == "dl_run"     # a literal run: a 0xFF head, ~30 % one-zero-byte members
    one = np.where(rng.random(n) < 0.3)[0]
    one = one[one > 0]
    w[one, rng.integers(0, 8, size=one.size)] = 0
    return w


def _check_rate(oracle, kind, words):
    """The packed bytes of the stretch alone (PackedOutputStream.java:64-193),
    from the format: an all-nonzero word that heads a run is tag + 8 bytes +
    count (10), a run member its 8 bytes, at most 255 members per head; a
    word with k zero bytes outside a run is tag + (8 - k)."""
    n = len(words)
    got = len(oracle.pack(words.reshape(-1)))
    heads = -(-n // 256)
    if kind in ("ff", "rand_d"):
        assert got == 8 * n + 2 * heads, (kind, n, got)             # 2,050 per 256 words
    elif kind == "d_x":
        assert got == 10 * ((n + 1) // 2) + 7 * (n // 2), (kind, n, got)  # 8.5 per word
    elif kind == "l_only":
        assert got == 8 * n, (kind, n, got)                           # tag + 7, a string per word
    else:
        # a head per run; after a 255-member cap the next all-nonzero word heads a new run
        assert 8 * n + 2 <= got <= 8 * n + 2 * heads, (kind, n, got)
        if n >= 640:
            assert got >= 8 * n + 4, (kind, n, got)                   # a cap inside the stretch


def _piece(oracle, kind, words, start, n, rng):
    """A piece of `words` zero words but for n words of `kind` from `start`."""
    assert 0 <= start and start + n <= words, (words, start, n)
    s = _stretch(kind, n, rng)
    _check_rate(oracle, kind, s)
    p = np.zeros((words, 8), np.uint8)
    p[start:start + n] = s
    return p.reshape(-1)


def _starts(words, n):
    """Eight places for a stretch of n words in a piece of `words` words: at
    a wave's start, mid-wave, ending at a wave's last word, across the wave
    boundary at word 2,048 (both neighbours overflow) and, for two-unit
    pieces, at / across the unit boundary at word 8,192 and inside the short
    second unit (4,096 words: 16 steps per wave)."""
    s = [0,                          # the piece's (and a wave's) first word
         WAVE,                       # a wave's first word
         2 * WAVE + 333,             # mid-wave (a long stretch runs on into the next wave)
         2 * WAVE - n,               # ends exactly at a wave's last word
         WAVE - n // 2,              # across the wave boundary at word 2,048
         3 * WAVE - n // 3]          # across another, off centre
    if words == UNIT:
        s += [UNIT - n,              # ends at the piece's last word
              WAVE + 1]              # one word into a wave
    else:
        s += [UNIT - n // 2,         # across the unit boundary (run state handed over)
              min(UNIT + 1024 + 7, words - n)]  # in the second unit
    assert len(s) == 8
    return s


def _diff_report(pk, opk, off):
    """Where the packed bytes differ: count, the first offsets by piece."""
    m = min(len(pk), len(opk))
    bad = np.nonzero(pk[:m] != opk[:m])[0]
    if bad.size == 0:
        return f"lengths {len(pk)} / {len(opk)}"
    pc = np.searchsorted(off, bad, side="right") - 1
    first = [f"piece {int(p)} +{int(b - off[p])}" for b, p in zip(bad[:6], pc[:6])]
    i = int(bad[0])
    return (f"{bad.size} bytes differ in pieces {sorted(set(int(p) for p in pc))}; first at "
            f"{', '.join(first)}; got {bytes(pk[i:i + 16]).hex()} want {bytes(opk[i:i + 16]).hex()}")


def _check_batch(c, oracle, data, swo):
    """Encode on the GPU, compare with the oracle byte for byte, decode back."""
    pk, off = c.encode_host(data, swo)
    opk, ooff = oracle.pack_batch(data, swo, threads=8)
    assert np.array_equal(off, ooff), "piece offsets differ"
    assert np.array_equal(pk, opk), "packed bytes differ: " + _diff_report(pk, opk, ooff)
    dec, st = c.decode_host(pk, off, swo)
    assert (st == 0).all(), st[st != 0][:8]
    assert np.array_equal(dec, data)


@pytest.fixture(scope="module", params=["d", "s"], ids=["form-dense", "form-sparse"])
def form_ctx(request):
    """(context, form): the default encoder with the single pass's form
    forced (CPK_SP_FORM is read at context creation), so the gate sends every
    like-sized batch to that form whatever its density."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = {k: os.environ.get(k) for k in ("CPK_ENCODER", "CPK_SP_FORM")}
    os.environ.pop("CPK_ENCODER", None)
    os.environ["CPK_SP_FORM"] = request.param
    try:
        c = cp.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c, request.param
    c.close()


def _seed(*key):
    return [int.from_bytes(str(k).encode(), "little") % (1 << 32) for k in key]


@pytest.mark.parametrize("words", [UNIT, UNIT + UNIT // 2])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_dense_stretch(form_ctx, oracle, kind, n, words, monkeypatch):
    """Eight like-sized pieces, each zero but for one stretch of n words of
    one kind, the stretch at eight places (_starts).  (CPK_NO_SMALL keeps the
    batch off the one-workgroup path for small batches.)"""
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    rng = np.random.default_rng(_seed(kind, n, words))
    pieces = [_piece(oracle, kind, words, s, n, rng) for s in _starts(words, n)]
    _check_batch(form_ctx[0], oracle, np.concatenate(pieces), _swo([words] * 8))


@pytest.mark.parametrize("words", [UNIT, UNIT + UNIT // 2])
@pytest.mark.parametrize("kind", KINDS)
def test_whole_pieces_dense(form_ctx, oracle, kind, words, monkeypatch):
    """Eight pieces that are one stretch from end to end: every wave of
    every unit overflows its ring (in the sparse form; in the dense one every
    wave of a whole unit), the worst sustained case."""
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    rng = np.random.default_rng(_seed(kind, words, "whole"))
    pieces = [_piece(oracle, kind, words, 0, words, rng) for _ in range(8)]
    _check_batch(form_ctx[0], oracle, np.concatenate(pieces), _swo([words] * 8))


@pytest.mark.parametrize("words", [UNIT, UNIT + UNIT // 2])
def test_overflowing_next_to_fitting_pieces(form_ctx, oracle, words, monkeypatch):
    """Pieces whose waves overflow the ring between pieces whose waves fit
    it (all zero, config-4 data, a stretch of 320 words): a workgroup takes
    one after the other, so a ring line left uncleared or a flush position
    left over from an overflowing unit would show in the next."""
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    rng = np.random.default_rng(_seed(words, "mixed"))
    c4 = oracle.generate(oracle.preset(4), _swo([words] * 2))
    pieces = [_piece(oracle, "rand_d", words, 0, words, rng),
              np.zeros(8 * words, np.uint8),
              _piece(oracle, "d_x", words, 0, words, rng),
              c4[: 8 * words],
              _piece(oracle, "ff", words, 100, words - 100, rng),
              _piece(oracle, "l_only", words, WAVE + 5, 320, rng),
              _piece(oracle, "dl_run", words, 0, words, rng),
              c4[8 * words:]]
    _check_batch(form_ctx[0], oracle, np.concatenate(pieces), _swo([words] * 8))


def test_mostly_zero_batch_with_dense_pieces_default_gate(ctx, oracle, monkeypatch):
    """The batch a user could submit: 24 like-sized pieces of 8,192 words,
    over 90 % zero words overall, one piece in twelve all-nonzero random
    bytes, through the default encoder choice (and the other pairs of the ctx
    fixture).  The device gate samples the words, finds them >= 85 % zero and
    is expected to pick the sparse form, whose 4 KiB rings the two dense
    pieces overflow in every wave; which form ran cannot be observed from
    outside, so what is asserted is parity alone."""
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    rng = np.random.default_rng(2412)
    pieces = []
    for i in range(24):
        if i % 12 == 5:
            pieces.append(_piece(oracle, "rand_d", UNIT, 0, UNIT, rng))
        else:
            p = np.zeros((UNIT, 8), np.uint8)
            some = rng.choice(UNIT, size=UNIT // 100, replace=False)  # 1 % of the words
            p[some] = rng.integers(0, 256, size=(some.size, 8), dtype=np.uint8)
            pieces.append(p.reshape(-1))
    data = np.concatenate(pieces)
    zero_words = int((data.view(np.uint64) == 0).sum())
    assert zero_words >= 0.9 * 24 * UNIT, zero_words
    _check_batch(ctx, oracle, data, _swo([UNIT] * 24))
