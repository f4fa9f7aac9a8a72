"""The device launch layer's branches that no other file forces (host_api.hip:
the single pass's plan with a unit table, from the hint and from the word
total read back; the size query's two forms; the two passes' rows packed by
word offset; the message front half under every CPK_E4_ORDER; one context's
look-back words across encodes of different unit counts and a size call that
shares them).  Every result is compared with the oracle (oracle.pack_batch,
oracle.write_message), never with the library alone.

The batch is five pieces of 8192, 8193, 1, 0 and 20000 words of config-2
data: one unit exactly, one word over a chunk, a tiny piece, an empty one and
three units -- the smallest sizes at which the unit table and the plan can go
wrong.  The messages are test_gpu_packed_size.py's 60."""
import os

import numpy as np
import pytest

from test_gpu_packed_size import _dev, _message_offsets, _messages, _swo

pytestmark = pytest.mark.gpu

SIZES = [8192, 8193, 1, 0, 20000]
KEYS = ("CPK_ENCODER", "CPK_SIZE_FORM", "CPK_E4_ORDER")


def _context(**env):
    """A context created under `env` alone of KEYS (they are read at
    creation); the environment is restored at once."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
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


def _batch(oracle, sizes):
    swo = _swo(sizes)
    data = oracle.generate(oracle.preset(2), swo)
    want, woff = oracle.pack_batch(data, swo)
    return data, swo, want.tobytes(), np.asarray(woff, dtype=np.uint64)


@pytest.fixture(scope="module")
def large(oracle):
    """(data, swo, oracle bytes, oracle offsets) of the five pieces, computed once."""
    return _batch(oracle, SIZES)


@pytest.fixture(scope="module")
def small(oracle):
    return _batch(oracle, [100] * 5)


@pytest.fixture(scope="module")
def messages(oracle):
    """(messages, oracle bytes, oracle piece offsets in message order)."""
    msgs = _messages(60)
    want = b"".join(oracle.write_message(m) for m in msgs)
    woff = _message_offsets(oracle, msgs)
    assert int(woff[-1]) == len(want)
    return msgs, want, woff


def _encode(c, batch, maxw):
    """One encode_batch -> (bytes, offsets); take_error() must be OK."""
    import torch
    import capnp_packed as cp
    data, swo, _, _ = batch
    d_in, d_swo = _dev(data, swo)
    d_pk = torch.zeros(cp.batch_capacity(swo), dtype=torch.uint8, device="cuda")
    d_off = torch.full((len(swo),), -1, dtype=torch.int64, device="cuda")
    c.encode_batch(d_in, d_swo, maxw, d_pk, d_off)
    assert c.take_error() == cp.OK
    off = d_off.cpu().numpy().astype(np.uint64)
    return d_pk.cpu().numpy()[: int(off[-1])].tobytes(), off


def _size(c, batch, maxw):
    """One packed_size_batch -> offsets; take_error() OK and the input unchanged."""
    import torch
    import capnp_packed as cp
    data, swo, _, _ = batch
    d_in, d_swo = _dev(data, swo)
    before = d_in.clone()
    d_off = torch.full((len(swo),), -1, dtype=torch.int64, device="cuda")
    c.packed_size_batch(d_in, d_swo, maxw, d_off)
    assert c.take_error() == cp.OK
    assert torch.equal(before, d_in)
    return d_off.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("hinted", [True, False], ids=["hint", "hint-0"])
@pytest.mark.parametrize("form", ["chunk", "wave"])
def test_size_forms(large, form, hinted):
    """Both size forms forced; without a hint the unit bound comes from the
    batch's word total, read back."""
    c = _context(CPK_SIZE_FORM=form)
    try:
        assert np.array_equal(_size(c, large, max(SIZES) if hinted else 0), large[3])
    finally:
        c.close()


@pytest.mark.parametrize("encoder", ["0", "4"], ids=["single-pass", "two-pass"])
def test_encode_without_hint(large, encoder):
    """Hint 0: the single pass forced takes its unit bound (several units)
    from the word total read back; the two passes pack their rows by word
    offset."""
    c = _context(CPK_ENCODER=encoder)
    try:
        pk, off = _encode(c, large, 0)
        assert np.array_equal(off, large[3])
        assert pk == large[2]
    finally:
        c.close()


@pytest.mark.parametrize("order", ["0", "1", "2"])
def test_message_front_half(messages, order):
    """The two passes over a message batch and the size call's front half of
    them, segments in order (0), largest first in both passes (1), in the
    emit pass only (2)."""
    import torch
    import capnp_packed as cp
    msgs, want, woff = messages
    segs = [s for m in msgs for s in m]
    swo = _swo([len(s) // 8 for s in segs])
    d_in, d_swo = _dev(b"".join(segs), swo)
    d_mseg = torch.from_numpy(_swo([len(m) for m in msgs]).astype(np.int64)).cuda()
    before = d_in.clone()
    c = _context(CPK_ENCODER="4", CPK_E4_ORDER=order)
    try:
        d_pk = torch.zeros(cp.batch_capacity(swo) + 16 * len(msgs) * 10, dtype=torch.uint8, device="cuda")
        d_eoff = torch.full((len(woff),), -1, dtype=torch.int64, device="cuda")
        c.encode_messages(d_in, d_swo, d_mseg, 9000, d_pk, d_eoff)
        assert c.take_error() == cp.OK
        d_soff = torch.full((len(woff),), -1, dtype=torch.int64, device="cuda")
        c.packed_size_messages(d_in, d_swo, d_mseg, 9000, d_soff)
        assert c.take_error() == cp.OK
        assert torch.equal(before, d_in)
    finally:
        c.close()
    eoff = d_eoff.cpu().numpy().astype(np.uint64)
    soff = d_soff.cpu().numpy().astype(np.uint64)
    assert np.array_equal(eoff, woff)
    assert np.array_equal(soff, eoff)
    assert d_pk.cpu().numpy()[: len(want)].tobytes() == want


def test_one_context_small_large_small_size(small, large):
    """One context, the single pass forced: a small batch, the large one (a
    unit table, more of the look-back words used), the small one again (words
    tagged by the large batch's epoch must not be taken for its own), then
    the size call on the large batch: the shared plan after an encode.  The
    look-back array has a floor of 8192 entries and these batches need 30 at
    most, so it is allocated (and cleared) once and never grows here: what
    this checks is the epoch tagging and the unit table across calls."""
    c = _context(CPK_ENCODER="0")
    try:
        for batch, maxw in ((small, 100), (large, max(SIZES)), (small, 100)):
            pk, off = _encode(c, batch, maxw)
            assert np.array_equal(off, batch[3])
            assert pk == batch[2]
        assert np.array_equal(_size(c, large, max(SIZES)), large[3])
    finally:
        c.close()
