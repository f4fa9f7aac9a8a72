"""Pins the message-framing corpus (tests/_message_frames.py) against the
oracle's Serialize.read (oracle/packed_oracle.c:cpko_read_message) and, for
the cases that have an unpacked form, against the restated unpacked read loop
of tests/test_gpu_encode_message_stream.py.  No GPU."""
import numpy as np

import _message_frames as mf
from test_gpu_encode_message_stream import _read_loop


def test_every_case_reads_as_recorded(oracle):
    """The recorded status and segment count are literals in the corpus: the
    oracle must produce them (a drifting oracle shows here too), and for a
    message read whole the segments the case was built from."""
    for case in mf.corpus().values():
        st, segs, used = oracle.read_message(case.packed, case.limit, out_cap=mf.oracle_cap(case))
        assert (st, len(segs)) == (case.status, case.nseg), case.name
        if st == mf.OK and case.words is not None:
            t = 8 * (1 + (case.nseg & ~1) // 2)
            assert b"".join(segs) == case.words[t:t + sum(len(s) for s in segs)], case.name
            sizes = np.frombuffer(case.words[4:4 + 4 * case.nseg], np.uint32)
            assert [len(s) // 8 for s in segs] == [int(v) for v in sizes], case.name


def test_unpacked_form_has_the_same_status():
    n = 0
    for case in mf.corpus().values():
        if case.words is None:
            continue
        n += 1
        off, mp, x, st, largest = _read_loop(np.frombuffer(case.words, np.uint64), case.limit)
        assert st == case.status, case.name
        assert (len(mp) - 1 >= 1) == (case.status == mf.OK), case.name
    assert n >= 50
    # only what has no unpacked form goes without: runs across boundaries
    # (CPK_EOVERRUN is a packed stream's) and cuts inside a word
    for case in mf.corpus().values():
        if case.words is None:
            assert case.status == mf.EOVERRUN or case.name.startswith("trunc/"), case.name


def test_the_corpus_covers_what_it_names():
    cases = mf.corpus()
    assert tuple(cases) == mf.NAMES and len(set(mf.NAMES)) == len(mf.NAMES)
    assert {c.status for c in cases.values()} == {mf.OK, mf.ETRUNC, mf.EOVERRUN, mf.EFRAME}
    # every piece boundary has its own run across it
    for b in mf.BOUNDARIES:
        hit = [c for c in cases.values() if c.boundary == b]
        assert len(hit) == 1 and hit[0].status == mf.EOVERRUN, b
    for c in (1, 2, 3, 4, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512):
        assert cases[f"count/{c}"].nseg == c
    for i in (0, 1, 63, 64, 65, 126, 127, 128, 511):
        assert cases[f"neg/segment-{i}"].status == mf.EFRAME
    # the reference's order: an earlier segment's failure ahead of the oversized segment's
    for at in (1, 64, 511):
        assert [cases[f"big/at-{at}/earlier-{k}"].status for k in ("complete", "truncated", "overrun")] == \
            [mf.EFRAME, mf.ETRUNC, mf.EOVERRUN]
    # sizes: a case and the small tail fit the one-launch reader's 6 KiB
    ts, small, tl, large = mf.tails()
    assert max(len(c.packed) for c in cases.values()) + len(ts) < 6 * 1024
    assert sum(len(c.packed) + len(c.words or b"") for c in cases.values()) < 1 << 20
    assert all(len(c.words or b"") <= 16 * 1024 for c in cases.values())
    assert 80 <= len(ts) <= 128 and 128 * 1024 < len(tl) < 200 * 1024 and 200 <= len(large) <= 500


def test_tails_are_valid_streams(oracle):
    ts, small, tl, large = mf.tails()
    for data, msgs in ((ts, small), (tl, large)):
        pos = 0
        for m in msgs:
            st, segs, used = oracle.read_message(data[pos:pos + 4096], mf.LIMIT, out_cap=mf.SMALL_CAP)
            assert st == oracle.OK and segs == m
            pos += used
        assert pos == len(data)
