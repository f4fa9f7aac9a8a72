"""The run state handed from chunk to chunk of a piece, through every encoder
that hands it (csrc/sp_chunk.hip: early publish, wait, late publish).

The pieces are the hand-built chunk-boundary pieces of
tests/_packed_size_cases.py: 3 x 8192 + 1 words each, a run's start, its
255 / 256 caps and its end on either side of the boundary at word 8192, so a
chunk's leaving state is both published early and waited for.
tests/test_gpu_packed_size.py checks their sizes; here their packed bytes and
offsets are compared with the oracle bit for bit, through
  - the single pass (sp_encode_kernel), dense and sparse form forced, a piece
    per call and all 51 in one batch (units of different pieces interleaved
    in ticket order);
  - the one-workgroup kernel (sp_small_kernel), a piece per call.
"""
import os

import numpy as np
import pytest

from _packed_size_cases import boundary_pieces, PIECE_WORDS

pytestmark = pytest.mark.gpu


def _swo(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


@pytest.fixture(scope="module")
def cases(oracle):
    """[(name, piece, packed bytes by the oracle)], computed once."""
    return [(name, p, oracle.pack(p)) for name, p in boundary_pieces()]


@pytest.fixture(scope="module", params=["d", "s"], ids=["form-dense", "form-sparse"])
def form_ctx(request):
    """The default encoder with the single pass's form forced (CPK_SP_FORM is
    read at context creation): like-sized pieces of over one chunk go to the
    single pass in that form, with a unit table."""
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
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    c = cp.Context(0)
    yield c
    c.close()


def _check_each(c, cases):
    one = _swo([PIECE_WORDS])
    for name, piece, want in cases:
        pk, off = c.encode_host(piece, one)
        assert off.tolist() == [0, len(want)], name
        assert pk.tobytes() == bytes(want), name


def test_single_pass_piece_per_call(form_ctx, cases, monkeypatch):
    monkeypatch.setenv("CPK_NO_SMALL", "1")  # (off the one-workgroup path)
    monkeypatch.delenv("CPK_HOST_CHUNK_KB", raising=False)  # (the host pipe's default chunks)
    _check_each(form_ctx, cases)


def test_single_pass_all_pieces_one_batch(form_ctx, cases, monkeypatch):
    monkeypatch.setenv("CPK_NO_SMALL", "1")
    monkeypatch.delenv("CPK_HOST_CHUNK_KB", raising=False)
    data = np.concatenate([p for _, p, _ in cases])
    pk, off = form_ctx.encode_host(data, _swo([PIECE_WORDS] * len(cases)))
    want_off = _swo([len(w) for _, _, w in cases])
    assert np.array_equal(off, want_off), [n for (n, _, _), a, b in zip(cases, np.diff(off), np.diff(want_off)) if a != b]
    for (name, _, want), a, b in zip(cases, want_off[:-1], want_off[1:]):
        assert pk[int(a):int(b)].tobytes() == bytes(want), name


def test_small_kernel_piece_per_call(plain_ctx, cases, monkeypatch):
    """3 x 8192 + 1 words are under kSpSmallWords: one workgroup takes the
    piece's four chunks in order, the state through two LDS words."""
    monkeypatch.delenv("CPK_NO_SMALL", raising=False)
    monkeypatch.delenv("CPK_HOST_CHUNK_KB", raising=False)
    f0 = plain_ctx.small_fallbacks()
    _check_each(plain_ctx, cases)
    assert plain_ctx.small_fallbacks() == f0
