"""Message framing parity: every case of tests/_message_frames.py (segment
table and piece-boundary edges) through every device reader that restates
Serialize.read (Serialize.java:119-178).  Expected values come from the
oracle (cpko_read_message, a loop of it for the streams) and, for the
unpacked-stream reader, from the restated read loop that
tests/test_gpu_encode_message_stream.py pins -- never from a device reader.

Which cases go to which reader, and why:

  reader                                   cases
  cpk_decode_messages (device, host)       all, as one batch per traversal limit
  cpk_read_message_host, one-launch wave   all
  ... workgroup reader (rm_mw_kernel)      all
  ... staged, then the workgroup reader    all
  ... block path (rm_table_kernel, ss)     all, and again by one wave
  ... record-index context (rm_table +     all
      the one-wave launch)
  cpk_read_message (device form)           count/, limit/, big/: the entry point differs from the
                                           host form only in where the info row and the offsets
                                           land, which is what is compared
  cpk_decode_message_stream                all (behind three good messages, before a small and a
                                           large tail); EOVERRUN and big/ again with the fallback off
  cpk_encode_message_stream                the cases that have an unpacked form (`words`): a run
                                           across a piece boundary and a cut inside a word exist
                                           only in packed bytes

The block path: a host stream of 128 KiB and more is staged by DMA and handed
to cpk_read_message, whose workgroup reader takes a reach under 512 KiB; the
block path proper starts there, or at a context's CPK_RM_MW_MAX_KB.  Both are
run (the second through a 64 KiB context), and the reach arithmetic is
asserted from the bounds documented in csrc/host_api.hip.

Capacity: cpk_read_message reports CPK_ENOMEM where a valid table declares
more words than out_cap_words (the oracle's CPK_EINVAL for a short buffer, at
the same place in the order of the checks); a message with an oversized
segment never does.  The only other divergence from the reference in the
header, a literal run cut short by the end of input, does not arise here.
"""
import contextlib
import os

import numpy as np
import pytest

import _message_frames as mf
from test_gpu_message_stream import _compare as _ms_compare, _device_bytes, _guarded, _oracle_loop, _untouched
from test_gpu_encode_message_stream import _compare as _ems_compare, _message

pytestmark = pytest.mark.gpu

OK, EINVAL, ETRUNC, EOVERRUN, ETRAILING, ENOMEM, EFRAME, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -7, -8
# csrc/host_api.hip: kRmMwMin, kRmMwMaxHost, kRmMwMax, kRmSsMin; include/capnp_packed.h: CPK_MSG_HEAD_WORDS
MW_MIN, MW_MAX_HOST, MW_MAX, SS_MIN, HEAD = 6 * 1024, 128 * 1024, 512 * 1024, 64 * 1024, 257


@contextlib.contextmanager
def _context(**env):
    """A context created (and used) with the given environment."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    c = None
    try:
        c = cp.Context(0)
        yield c
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if c is not None:
            c.close()


@pytest.fixture(scope="module")
def fctx():
    with _context() as c:
        yield c


def _by_limit(names):
    groups = {}
    for n in names:
        groups.setdefault(mf.corpus()[n].limit, []).append(n)
    return groups


def _batch_expect(oracle, case):
    st, segs, used = oracle.read_message(case.packed, case.limit, out_cap=mf.oracle_cap(case))
    assert (st, len(segs)) == (case.status, case.nseg), case.name
    if st == OK and used != len(case.packed):
        st = ETRAILING
    return st, segs


# ---- cpk_decode_messages -------------------------------------------------------

@pytest.mark.parametrize("order", ["corpus-order", "reversed"])
def test_decode_messages_batch(fctx, oracle, order):
    """All cases as one batch per traversal limit, d_msg_off cut at each
    case's end; in both orders (the largest-first tickets change which wave
    takes which message)."""
    import torch
    for limit, names in _by_limit(mf.NAMES).items():
        names = names[::-1] if order == "reversed" else names
        cases = [mf.corpus()[n] for n in names]
        nm = len(cases)
        moff = np.concatenate([[0], np.cumsum([len(c.packed) for c in cases])]).astype(np.int64)
        d_pk = _device_bytes(b"".join(c.packed for c in cases) + bytes(48))
        d_moff = torch.from_numpy(moff).cuda()
        bm, d_mseg = _guarded(nm + 1)
        bt = torch.full((nm + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_mst = bt[2:2 + nm]
        rc, W, S = fctx.decode_messages(d_pk, d_moff, None, None, None, None, d_mseg, d_mst, traversal_limit_words=limit)
        want_s = sum(c.tseg for c in cases)
        assert S == want_s, (limit, S, want_s)
        if S == 0:
            assert rc == OK
        else:
            assert rc == ENOMEM
            bo, d_out = _guarded(W)
            bw, d_swo = _guarded(S + 1)
            bi, d_sin = _guarded(S)
            bs = torch.full((S + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            rc, W2, S2 = fctx.decode_messages(d_pk, d_moff, d_out, d_swo, d_sin, bs[2:2 + S], d_mseg, d_mst,
                                              traversal_limit_words=limit)
            torch.cuda.synchronize()
            assert rc == OK and (W2, S2) == (W, S)
            assert all(_untouched(b) for b in (bo, bw, bi))
            g = bs.cpu().numpy()
            assert (g[:2] == 0x5A5A5A5A).all() and (g[-2:] == 0x5A5A5A5A).all()
            swo = d_swo.cpu().numpy()
        g = bt.cpu().numpy()
        assert (g[:2] == 0x5A5A5A5A).all() and (g[-2:] == 0x5A5A5A5A).all() and _untouched(bm)
        mseg, mst = d_mseg.cpu().numpy(), d_mst.cpu().numpy()
        assert mseg[0] == 0 and mseg[nm] == S
        for i, c in enumerate(cases):
            ost, segs = _batch_expect(oracle, c)
            assert mst[i] == ost, (c.name, int(mst[i]), ost)
            assert mseg[i + 1] - mseg[i] == c.tseg, c.name  # (none for a failed table)
            if ost in (OK, ETRAILING):
                a, b = int(swo[mseg[i]]), int(swo[mseg[i + 1]])
                out = d_out[a:b].cpu().numpy().view(np.uint8) if b > a else np.zeros(0, np.uint8)
                got = [out[8 * (int(swo[j]) - a): 8 * (int(swo[j + 1]) - a)].tobytes()
                       for j in range(mseg[i], mseg[i + 1])]
                assert got == segs, c.name


def test_decode_messages_host(fctx, oracle):
    for limit, names in _by_limit(mf.NAMES).items():
        cases = [mf.corpus()[n] for n in names]
        moff = np.concatenate([[0], np.cumsum([len(c.packed) for c in cases])]).astype(np.uint64)
        mst, msgs = fctx.decode_messages_host(b"".join(c.packed for c in cases), moff, traversal_limit_words=limit)
        for i, c in enumerate(cases):
            ost, segs = _batch_expect(oracle, c)
            assert mst[i] == ost, (c.name, int(mst[i]), ost)
            assert len(msgs[i]) == c.tseg, c.name
            if ost in (OK, ETRAILING):
                assert msgs[i] == segs, c.name


# ---- cpk_read_message ------------------------------------------------------------

def _reach(avail, cap):
    return min(avail, 10 * (cap + HEAD) + 16)  # (ss_reach: 10 bytes per word at most, 16 of slack)


def _rm_expect(oracle, case, data, cap):
    st, segs, used = oracle.read_message(data, case.limit, out_cap=mf.HUGE_CAP)
    assert st != EINVAL, case.name
    # (a valid table that declares more than the capacity: CPK_ENOMEM, the
    # oracle's CPK_EINVAL for a short buffer; never with an oversized segment)
    if not case.name.startswith("big/at-") and oracle.read_message(data, case.limit, out_cap=8 * cap)[0] == EINVAL:
        return ENOMEM, [], 0
    return st, segs, used


# path -> (context environment, tail, out_cap_words, one-wave, the reach the path needs)
RM_PATHS = {
    "one-launch-wave": ({}, "small", 4096, False, lambda r: r < MW_MIN),
    "workgroup": ({}, "large-40k", 4096, False, lambda r: MW_MIN <= r < MW_MAX_HOST),
    "staged-workgroup": ({}, "large", 16384, False, lambda r: MW_MAX_HOST <= r < MW_MAX),
    "block-path": ({"CPK_RM_MW_MAX_KB": "64"}, "large", 16384, False, lambda r: r >= max(64 * 1024, SS_MIN)),
    "block-path-one-wave": ({"CPK_RM_MW_MAX_KB": "64"}, "large", 16384, True, lambda r: r >= 64 * 1024),
    "record-index": ({"CPK_DECODER": "2"}, "small", 4096, False, lambda r: r < SS_MIN),
    # (bytes behind a case feed a message that is cut short: a truncation is seen only with nothing behind it,
    # which is a stream under 6 KiB)
    "one-launch-wave-bare": ({}, "none", 4096, False, lambda r: r < MW_MIN),
    "record-index-bare": ({"CPK_DECODER": "2"}, "none", 4096, False, lambda r: r < SS_MIN),
}


def _tail(kind):
    ts, _, tl, _ = mf.tails()
    return {"none": b"", "small": ts, "large": tl, "large-40k": tl[:40 * 1024]}[kind]


@pytest.mark.parametrize("path", list(RM_PATHS))
def test_read_message_host_paths(oracle, path):
    env, kind, cap, one, lands = RM_PATHS[path]
    tail = _tail(kind)
    seen = set()
    with _context(**env) as c:
        for case in mf.corpus().values():
            data = case.packed + tail
            assert lands(_reach(len(data), cap)), (case.name, len(data))
            want = _rm_expect(oracle, case, data, cap)
            if one:
                os.environ["CPK_STREAM_ONE_WAVE"] = "1"
            try:
                st, segs, used, info = c.read_message_host(np.frombuffer(data, np.uint8), out_cap_words=cap,
                                                           traversal_limit_words=case.limit)
            finally:
                os.environ.pop("CPK_STREAM_ONE_WAVE", None)
            assert st == want[0], (case.name, st, want[0])
            if st == OK:
                assert used == want[2] and segs == want[1], case.name
            seen.add(st)
    assert {OK, EOVERRUN, EFRAME} | ({ETRUNC} if kind == "none" else set()) <= seen


def test_read_message_device_form(fctx, oracle):
    """The info row and the segment offsets in device memory, for the
    oversized-segment, limit and count-edge cases."""
    import torch
    import capnp_packed as cp
    assert (cp.MSG_HEAD_WORDS, cp.MSG_INFO_WORDS) == (HEAD, 517)
    ts = _tail("small")
    cap = 4096
    for case in mf.corpus().values():
        if not case.name.startswith(("count/", "limit/", "big/")):
            continue
        for data in (case.packed + ts, case.packed):  # (and with nothing behind it: the truncations)
            want = _rm_expect(oracle, case, data, cap)
            d_pk = _device_bytes(data + bytes(64))
            bo, d_out = _guarded(cap + HEAD)
            bi, d_info = _guarded(cp.MSG_INFO_WORDS)
            fctx.read_message(d_pk, len(data), d_out, d_info, traversal_limit_words=case.limit)
            torch.cuda.synchronize()
            assert _untouched(bo) and _untouched(bi), case.name
            info = d_info.cpu().numpy()
            assert info[0] == want[0], (case.name, int(info[0]), want[0])
            if want[0] != OK:
                assert info[1] == 0, case.name
                if want[0] != ENOMEM:
                    assert info[2] == 0 and info[3] == 0, case.name
                continue
            sizes = [len(s) // 8 for s in want[1]]
            n = len(sizes)
            assert (info[1], info[2], info[3]) == (want[2], n, sum(sizes)), case.name
            t = 1 + (n & ~1) // 2  # (the table's words lead the output)
            assert [int(v) for v in info[4:5 + n]] == [t + int(v) for v in np.concatenate([[0], np.cumsum(sizes)])], case.name
            out = d_out.cpu().numpy().view(np.uint8)
            assert [out[8 * int(info[4 + i]): 8 * int(info[5 + i])].tobytes() for i in range(n)] == want[1], case.name
            if case.words is not None:  # (the pad half-word as read)
                assert out[:8 * t].tobytes() == case.words[:8 * t], case.name


# ---- cpk_decode_message_stream -----------------------------------------------------

def _stream(case, kind):
    import oracle
    ts, small, tl, large = mf.tails()
    return b"".join(oracle.write_message(m) for m in small) + case.packed + (ts if kind == "small" else tl)


@pytest.mark.parametrize("kind", ["small", "large"])
@pytest.mark.parametrize("name", mf.NAMES)
def test_decode_message_stream(fctx, oracle, name, kind):
    """Three good messages, the case, a tail: messages, segments, words, bytes
    consumed, tail status and d_msg_off as a loop of the oracle's read gives
    them; never CPK_EUNSUPPORTED."""
    case = mf.corpus()[name]
    _ms_compare(fctx, oracle, _stream(case, kind), case.limit, mf.oracle_cap(case))


def test_decode_message_stream_block_path_alone(oracle):
    """The runs across piece boundaries and the oversized segments with the
    one-wave fallback off: the block path itself makes the verdict."""
    with _context(CPK_STREAM_NO_FALLBACK="1") as c:
        for case in mf.corpus().values():
            if case.status == EOVERRUN or case.name.startswith("big/"):
                for kind in ("small", "large"):
                    _ms_compare(c, oracle, _stream(case, kind), case.limit, mf.oracle_cap(case))


def test_decode_message_stream_host_form(fctx, oracle):
    """One mixed stream: whole messages of every count edge, then a run into
    the next message."""
    names = [f"count/{c}" for c in (1, 2, 127, 128, 129, 192, 193, 256, 257, 512)] + ["pad/2-nonzero", "zero/300"]
    data = b"".join(mf.corpus()[n].packed for n in names) + _tail("small") + mf.corpus()["run/into-next-message"].packed
    want, offs, st = _oracle_loop(oracle, data)
    assert st == EOVERRUN and len(want) == len(names) + 299 + 3
    tail, got, consumed = fctx.decode_message_stream_host(data)
    assert (tail, consumed) == (st, offs[-1]) and got == want


# ---- cpk_encode_message_stream -----------------------------------------------------

WORDS_NAMES = tuple(n for n in mf.NAMES if mf.corpus()[n].words is not None)


@pytest.mark.parametrize("name", WORDS_NAMES)
def test_encode_message_stream(fctx, oracle, name):
    """Three good unpacked messages, the case's words, a good tail: counts,
    piece offsets, packed bytes, the result row against the restated read loop
    and the oracle's packer; whole messages equal SerializePacked.write."""
    case = mf.corpus()[name]
    _, small, _, _ = mf.tails()
    good = b"".join(_message(m) for m in small)
    # (nothing behind a message that is cut short: its words must end there)
    words = np.frombuffer(good + case.words + (b"" if case.status == ETRUNC else good), np.uint64).copy()
    e = _ems_compare(fctx, oracle, words, case.limit)  # (asserts every output against the restatement)
    # what the restatement must itself say about this stream
    nm = len(e["mp"]) - 1
    if case.status == OK:
        extra = 300 if name == "zero/300" else 1
        assert (nm, e["tail"]) == (3 + extra + 3, OK), name
    else:
        assert (nm, e["tail"]) == (3, case.status), name
        assert e["consumed"] == len(good) // 8, name
    # the complete messages are the oracle's SerializePacked.write of them ...
    head = b"".join(oracle.write_message(m) for m in small)
    assert e["bytes"][:len(head)] == head, name
    if case.status == OK and name not in ("zero/300",):
        t = 8 * (1 + (case.nseg & ~1) // 2)
        sizes = [int(v) for v in np.frombuffer(case.words[4:4 + 4 * case.nseg], np.uint32)]
        segs, o = [], t
        for s in sizes:
            segs.append(case.words[o:o + 8 * s])
            o += 8 * s
        ref = oracle.write_message(segs)
        mine = e["bytes"][len(head):len(e["bytes"]) - len(head)]
        if name.startswith("pad/"):
            # ... except that a nonzero pad half-word is kept (the header's
            # documented divergence): the table piece differs, reading the
            # bytes back gives the same segments
            assert mine != ref, name
            st, back, used = oracle.read_message(mine, case.limit, out_cap=mf.SMALL_CAP)
            assert (st, back, used) == (OK, segs, len(mine)), name
        else:
            assert mine == ref, name
        assert e["bytes"][-len(head):] == head, name
