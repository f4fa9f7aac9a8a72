"""tests/_messages_at_model.py held against the framing corpus
(tests/_message_frames.py, whose statuses and segment counts are literals) and
against itself: the fit rule, the range rules, what a message that is not
accepted leaves behind.  No GPU."""
import numpy as np
import pytest

import _decode_at_cases as D
import _message_frames as mf
import _messages_at_model as M

OK, EINVAL, ETRUNC, ETRAILING, ENOMEM, EFRAME, EUNSUPPORTED = M.OK, M.EINVAL, M.ETRUNC, M.ETRAILING, M.ENOMEM, \
    M.EFRAME, M.EUNSUPPORTED
BIG = 1 << 62


@pytest.mark.parametrize("name", mf.NAMES)
def test_facts_on_the_corpus(oracle, name):
    """Accepted iff the case counts segments for a batch reader (tseg); the
    status the oracle's, CPK_ETRAILING where the bytes outlast the message."""
    c = mf.corpus()[name]
    f = M.facts(c.packed, c.limit)
    assert f.accepted == (c.tseg > 0) and len(f.sizes) == c.tseg
    st, segs, used = oracle.read_message(c.packed, c.limit, out_cap=mf.oracle_cap(c))
    assert st == c.status
    want = ETRAILING if st == OK and used != len(c.packed) else st
    assert f.status == want
    if want in (OK, ETRAILING):
        assert list(f.segs) == segs and f.used == used and [len(s) // 8 for s in segs] == list(f.sizes)
    else:
        assert f.segs is None and f.used == 0
    if c.declared and f.accepted:
        assert sum(f.sizes) == c.declared


def _small_batch(oracle):
    """Good messages of 1-5 segments with a failed table, a truncated message
    and refused ranges among them."""
    msgs = [[mf.seg(k, (3 * m + k) % 7) for k in range(1 + m % 5)] for m in range(9)]
    items = [oracle.write_message(s) for s in msgs]
    items[3] = mf.corpus()["count/refused-513/alone"].packed   # a failed table
    items[6] = items[6][:-1]                                    # accepted, fails in its last segment
    items[7] += b"\x00"                                         # a byte outlasts it
    off, ln, in_cap, buf = D.place(items, "shuffled")
    return msgs, items, off, ln, in_cap, buf


def test_batch_rules(oracle):
    msgs, items, off, ln, in_cap, buf = _small_batch(oracle)
    nm = len(items)
    m = M.batch(buf, off, ln, in_cap, mf.LIMIT, BIG, BIG)
    assert list(m.status) == [OK, OK, OK, EFRAME, OK, OK, ETRUNC, ETRAILING, OK]
    assert m.mseg[0] == 0 and m.mseg[nm] == m.totals[1] and m.mseg[4] == m.mseg[3]  # (no room for the failed table)
    assert m.totals == (sum(len(s) // 8 for i, x in enumerate(msgs) if i != 3 for s in x),
                        sum(len(x) for i, x in enumerate(msgs) if i != 3), nm - 1)
    assert int(m.used[7]) == len(items[7]) - 1 and m.used[6] == 0 and m.used[3] == 0
    assert m.F == m.totals[1] and m.swo[m.F] == m.totals[0] and m.swo == sorted(m.swo)
    for i in (0, 1, 2, 4, 5, 7, 8):
        assert list(m.segs[i]) == msgs[i]
    # the sizing call: nothing fits, the totals stand
    z = M.batch(buf, off, ln, in_cap, mf.LIMIT, 0, 0)
    assert z.totals[:2] == m.totals[:2] and z.mseg == m.mseg and z.F == 0 and z.swo == [0]
    assert [int(s) for s in z.status] == [ENOMEM if f else int(s) for f, s in zip(m.fits, m.status)]
    assert z.totals[2] == 0 and not z.used.any()  # (every accepted message has a segment)


@pytest.mark.parametrize("short", ["words", "segments"])
def test_fit_is_a_prefix(oracle, short):
    """Each capacity from nothing to everything: the fitting messages are a
    prefix of the accepted ones, the rest CPK_ENOMEM, the others unchanged."""
    msgs, items, off, ln, in_cap, buf = _small_batch(oracle)
    full = M.batch(buf, off, ln, in_cap, mf.LIMIT, BIG, BIG)
    total = full.totals[0 if short == "words" else 1]
    seen = set()
    for cap in range(total + 1):
        m = M.batch(buf, off, ln, in_cap, mf.LIMIT, cap if short == "words" else BIG, cap if short == "segments" else BIG)
        assert m.totals[:2] == full.totals[:2] and m.mseg == full.mseg
        acc = [i for i in range(len(items)) if full.fits[i]]
        k = m.totals[2]
        assert [i for i in acc if m.fits[i]] == acc[:k]
        for i in range(len(items)):
            if i in acc[k:]:
                assert m.status[i] == ENOMEM and m.used[i] == 0 and m.segs[i] is None
            else:
                assert m.status[i] == full.status[i] and m.used[i] == full.used[i]
        assert m.F == (full.mseg[acc[k - 1] + 1] if k else 0) and m.swo == full.swo[:m.F + 1]
        seen.add(k)
    assert max(seen) == len(acc)
    if short == "segments":  # (a segment at a time: no prefix is skipped; a message may need no words)
        assert seen == set(range(len(acc) + 1))


def test_range_rules(oracle):
    good = oracle.write_message([mf.seg(0, 2)])
    off, ln, in_cap, buf = D.place([good, good, good])
    off = np.concatenate([off, np.array([in_cap + 1, in_cap - 1, 2**64 - 1, 0], np.uint64)])
    ln = np.concatenate([ln, np.array([0, 2, 2, 2**32], np.uint64)])
    m = M.batch(buf, off, ln, in_cap, mf.LIMIT, BIG, BIG)
    assert list(m.status) == [OK, OK, OK, EINVAL, EINVAL, EINVAL, EUNSUPPORTED]
    assert m.totals == (6, 3, 3) and m.mseg == [0, 1, 2, 3, 3, 3, 3, 3] and not m.used[3:].any()
    # an empty range at in_cap is a range; its table is cut short
    e = M.batch(buf, [in_cap], [0], in_cap, mf.LIMIT, BIG, BIG)
    assert list(e.status) == [ETRUNC] and e.totals == (0, 0, 0)
