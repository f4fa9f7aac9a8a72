"""cpk_encode_messages_at under graph capture: the call runs once uncaptured,
is captured on a side stream, and the graph is replayed twice with other words,
other segment sizes and other slot offsets written into the same device arrays.
Both replays must be exact against tests/_encode_messages_at_model.py (the
oracle's bytes), the buffer's sentinel bytes included.  Each form is replayed:
CPK_MSG_AT_FORM unset, wave and place."""
import os

import numpy as np
import pytest

import _encode_messages_at_model as M
import _high_offsets as H

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
MAXW = 3 * 8192 + 1
# per set: the messages' segment sizes (the same counts in every set, so nm
# and nseg are the captured ones), the generator preset, the first slot's byte
SETS = [
    ([[300], [2049, 17], [64, 0, 65], [3 * 8192 + 1], [1]], 2, 5),
    ([[17], [65, 8193], [0, 300, 1], [8192], [2048]], 3, 12),
    ([[8193], [1, 1], [4095, 64, 63], [100], [3 * 8192 + 1]], 4, 1),
]
SHORT = 2  # the message whose slot is one byte short in every set


@pytest.fixture(scope="module", params=[None, "wave", "place"], ids=["form-auto", "form-wave", "form-place"])
def mctx(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = os.environ.get("CPK_MSG_AT_FORM")
    if request.param is None:
        os.environ.pop("CPK_MSG_AT_FORM", None)
    else:
        os.environ["CPK_MSG_AT_FORM"] = request.param
    try:
        c = cp.Context(0)
    finally:
        if saved is None:
            os.environ.pop("CPK_MSG_AT_FORM", None)
        else:
            os.environ["CPK_MSG_AT_FORM"] = saved
    try:
        yield c
    finally:
        c.close()


def _set(oracle, k):
    """-> (messages, dst_off, dst_cap) of set k; slots descending for odd k."""
    shapes, cfg, start = SETS[k]
    sizes = [w for s in shapes for w in s]
    swo = H.rel_off(sizes).astype(np.int64)
    b = np.ascontiguousarray(oracle.generate(oracle.preset(cfg), swo.astype(np.uint64)), np.uint8).tobytes()
    segs = [b[8 * swo[i]:8 * swo[i + 1]] for i in range(len(sizes))]
    msgs, p = [], 0
    for s in shapes:
        msgs.append(segs[p:p + len(s)])
        p += len(s)
    n = [sum(len(x) for x in M.packed_pieces(oracle, m)) for m in msgs]
    cap = [x - 1 if m == SHORT else x + m % 3 for m, x in enumerate(n)]
    off, cur = [0] * len(msgs), start
    for m in (range(len(msgs)) if k % 2 == 0 else reversed(range(len(msgs)))):
        off[m] = cur
        cur += cap[m] + (5 * m + 3) % 16
    return msgs, off, cap


def test_replay_with_other_words_and_slots(mctx, oracle):
    import torch
    sets = [_set(oracle, k) for k in range(len(SETS))]
    nm = len(SETS[0][0])
    nseg = sum(len(s) for s in SETS[0][0])
    assert all(len(s[0]) == nm and sum(len(m) for m in s[0]) == nseg for s in sets)
    words = max(sum(len(x) for m in s[0] for x in m) for s in sets) // 8
    out_cap = max(o + c for s in sets for o, c in zip(s[1], s[2])) + 7
    i64 = dict(dtype=torch.int64, device="cuda")
    d_in = torch.zeros(words + 8, **i64)
    d_swo, d_mseg = torch.zeros(nseg + 1, **i64), torch.zeros(nm + 1, **i64)
    d_off, d_cap = torch.zeros(nm, **i64), torch.zeros(nm, **i64)
    buf = torch.empty(out_cap + 4096, dtype=torch.uint8, device="cuda")
    d_poff, d_len = torch.empty(nm + nseg + 1, **i64), torch.empty(nm + 1, **i64)
    d_st = torch.empty(nm + 1, dtype=torch.int32, device="cuda")

    def load(k):
        msgs, off, cap = sets[k]
        segs = [s for m in msgs for s in m]
        data = np.frombuffer(b"".join(segs), np.uint8).view(np.int64)
        d_in.zero_()
        d_in[:data.size].copy_(torch.from_numpy(data.copy()))
        d_swo.copy_(torch.from_numpy(H.rel_off([len(s) // 8 for s in segs]).astype(np.int64)))
        d_mseg.copy_(torch.from_numpy(H.rel_off([len(m) for m in msgs]).astype(np.int64)))
        d_off.copy_(torch.tensor(off, dtype=torch.int64))
        d_cap.copy_(torch.tensor(cap, dtype=torch.int64))
        buf.fill_(SENTINEL)
        d_poff.fill_(-1)
        d_len.fill_(-1)
        d_st.fill_(77)

    def call():
        mctx.encode_messages_at(d_in, d_swo, d_mseg, MAXW, buf, out_cap, d_off, d_cap, d_poff, d_len, d_st)

    def check(k, what):
        msgs, off, cap = sets[k]
        got = buf.cpu().numpy()
        exp = M.expected(oracle, msgs, off, cap, out_cap, MAXW, got.size, SENTINEL)
        st, ln, poff = d_st.cpu().tolist(), d_len.cpu().tolist(), d_poff.cpu().tolist()
        assert st == exp.status + [77] and SHORT == st.index(M.ENOMEM), what
        assert ln == exp.msg_len + [-1], what
        assert poff == exp.piece_off + [-1], what
        bad = np.nonzero((got != exp.image) & exp.care)[0]
        assert bad.size == 0, f"{what}: {bad.size} wrong bytes, the first at {bad[0]}"

    # 1. once uncaptured: the context's buffers grow here
    load(0)
    call()
    torch.cuda.synchronize()
    check(0, "uncaptured")
    # 2. captured on a side stream
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    # 3. replayed with other words, sizes and slots in the same arrays
    for k in (1, 2):
        load(k)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(k, f"replay with set {k}")
    # ... and an eager call after the replays
    load(0)
    call()
    torch.cuda.synchronize()
    check(0, "eager after the replays")
