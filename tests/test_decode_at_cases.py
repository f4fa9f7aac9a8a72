"""The placed layouts and the model behind tests/test_gpu_decode_at.py, held
against the oracle on the CPU: extracting the slots of a layout gives the
compacted batch back whatever the order, gaps and filler, and the model's
statuses for pieces of their own equal oracle.unpack_batch's on every corpus of
tests/_packed_records.py."""
import numpy as np
import pytest

import _decode_at_cases as D
import _packed_records as R


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    R.release()


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_slots_give_back_the_batch(name):
    cases = R.corpora()[name]
    items = [c.packed for c in cases]
    for k, (order, filler) in enumerate(zip(D.ORDERS, D.FILLERS)):
        off, ln, in_cap, buf = D.place(items, order, filler=filler)
        assert D.extract(buf, off, ln) == items
        assert len(buf) == in_cap and int((off + ln).max()) + 5 == in_cap
        # slots are disjoint, and every byte outside them is the filler's
        mask = np.zeros(in_cap, bool)
        for o, l in zip(off, ln):
            assert not mask[int(o):int(o) + int(l)].any()
            mask[int(o):int(o) + int(l)] = True
        pat = np.frombuffer(D.FILLERS[filler], np.uint8)
        want = np.resize(pat, in_cap)
        assert np.array_equal(buf[~mask], want[~mask])
        assert all(D.range_status(int(o), int(l), in_cap) == D.OK for o, l in zip(off, ln))


def test_orders_and_gaps():
    assert D.slot_order(5, "forward") == [0, 1, 2, 3, 4]
    assert D.slot_order(5, "reversed") == [4, 3, 2, 1, 0]
    assert sorted(D.slot_order(50, "shuffled")) == list(range(50))
    assert D.slot_order(50, "shuffled") != list(range(50))
    off, ln, _, _ = D.place([b"x" * 40] * 64)
    assert {int(o) % 16 for o in off} == set(range(16))


def test_range_rules():
    assert D.range_status(0, 0, 0) == D.OK
    assert D.range_status(10, 6, 16) == D.OK
    assert D.range_status(10, 7, 16) == D.EINVAL
    assert D.range_status(17, 0, 16) == D.EINVAL
    assert D.range_status(2**64 - 8, 16, 1 << 20) == D.EINVAL
    assert D.range_status(0, 1 << 32, 1 << 20) == D.EUNSUPPORTED
    assert D.range_status(0, (1 << 32) - 1, 1 << 32) == D.OK


@pytest.mark.parametrize("name", R.VALID + R.MALFORMED)
def test_model_statuses_equal_the_oracles(oracle, name):
    cases = R.corpora()[name]
    packed, in_off, swo = R.batch_arrays(cases)
    want, ost = oracle.unpack_batch(packed, in_off, swo, threads=8)
    pst, pout, gst, used = D.batch_model(oracle, [c.packed for c in cases], [[c.nwords] for c in cases])
    bad = [f"{c.name}: model {int(s)}, oracle {int(o)}" for c, s, o in zip(cases, pst, ost) if s != o]
    assert not bad, (len(bad), bad[:8])
    assert np.array_equal(gst, pst)
    for i, c in enumerate(cases):
        if ost[i] == D.OK:
            assert int(used[i]) == len(c.packed)
            assert pout[i] == want[8 * int(swo[i]):8 * int(swo[i + 1])].tobytes(), c.name


def test_group_model_rules(oracle):
    a, b = bytes(range(1, 17)), bytes(8) + b"\x01" * 8
    pa, pb = oracle.pack(a), oracle.pack(b)
    st, out, g, used = D.group_model(oracle, pa + pb, [2, 0, 2])
    assert (st, out, g, used) == ([0, 0, 0], [a, b"", b], D.OK, len(pa) + len(pb))
    st, out, g, used = D.group_model(oracle, pa + pb + b"\x00", [2, 2])
    assert (st, g, used) == ([0, 0], D.ETRAILING, len(pa) + len(pb))
    st, out, g, used = D.group_model(oracle, pa, [2, 2, 0])
    assert (st, g, used) == ([0, D.ETRUNC, D.ETRUNC], D.ETRUNC, 0)
    st, out, g, used = D.group_model(oracle, pa + b"\x00", [2])
    assert (st, g, used) == ([D.ETRAILING], D.ETRAILING, len(pa))
    assert D.group_model(oracle, b"", []) == ([], [], D.OK, 0)
    assert D.group_model(oracle, b"\xff", [])[2:] == (D.ETRAILING, 0)
