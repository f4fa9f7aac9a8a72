"""The device entry points on a side stream, captured into a graph and replayed
with changing inputs (include/capnp_packed.h: "asynchronous on `stream`, no
host synchronisation").

For an entry point and its input sets (tests/_replay_cases.py; the sets share
every array length and host scalar) one helper, _run:
  1. allocates every device tensor once, each set's inputs also in pinned memory;
  2. runs set 0 eagerly on a side stream -- inputs copied in and outputs
     poisoned on that stream, that stream alone synchronised (this is also
     the warm-up that sizes the context's buffers: growth allocates);
  3. captures the one library call into a graph: nothing else in the capture,
     which is linear;
  4. replays the graph for every set in order: inputs overwritten in place,
     outputs poisoned, replay, synchronise, every output compared;
  5. makes one eager call with a set that is not the last replayed, then
     replays set 0 again: both must be right.
Every comparison is bit-exact against the cases' expectation, which comes from
the oracle and the CPU models built on it, and covers every byte of every
output and the poison behind it: what the contract leaves undefined is masked
there, what it says is untouched must still hold the poison.

A launch that went to the null stream, a ticket or gate word reset from the
host, a host-read value or a per-call counter baked into a launch argument
(the single pass's epoch), or words an earlier replay left behind: all show
here as wrong bytes on a later replay; a hidden synchronisation fails the
capture.  Calls documented to synchronise are not captured."""
import ctypes
import os
import time

import numpy as np
import pytest

import _replay_cases as R

pytestmark = pytest.mark.gpu

FORM_KEYS = ("CPK_ENCODER", "CPK_DECODER", "CPK_SP_FORM", "CPK_SIZE_FORM", "CPK_USIZE_FORM", "CPK_AT_FORM",
             "CPK_E4_ORDER")


def _context(**env):
    """A context created under `env` alone of FORM_KEYS (read at creation)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import capnp_packed as cp
    saved = {k: os.environ.get(k) for k in FORM_KEYS}
    for k in FORM_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return cp.Context(0)
    finally:
        for k in FORM_KEYS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


@pytest.fixture(scope="module")
def own(oracle):
    """A context with every form left to the device (CPK_AT_FORM, CPK_SIZE_FORM unset)."""
    c = _context()
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Rig:
    """The device tensors of one family: inputs (and their pinned copies per
    set) and outputs, all as bytes; outputs are the expectation's size, PAD
    bytes of poison included."""

    def __init__(self, fam, expect0, zeroed=()):
        import torch
        self.fam, self.zeroed = fam, zeroed
        self.pinned = [{k: torch.from_numpy(a.copy()).pin_memory() for k, a in s.inputs.items()} for s in fam.sets]
        self.T = {k: torch.zeros(a.size, dtype=torch.uint8, device="cuda") for k, a in fam.sets[0].inputs.items()}
        for k, (want, _) in expect0.items():
            assert k not in self.T
            self.T[k] = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
        self.outs = list(expect0)
        torch.cuda.synchronize()

    def p(self, name):
        return self.T[name].data_ptr()

    def load(self, i):
        """Set i in, outputs poisoned: on the current stream."""
        for k, h in self.pinned[i].items():
            self.T[k].copy_(h, non_blocking=True)
        for k in self.outs:
            self.T[k].fill_(R.POISON)
            if k in self.zeroed:  # (an accumulator the caller zeroes; the poison behind it stays)
                self.T[k][:-R.PAD].zero_()

    def check(self, expect, what):
        """Every output against its expectation; the report names each wrong one."""
        wrong = []
        for k in self.outs:
            want, care = expect[k]
            got = self.T[k].cpu().numpy()
            bad = np.nonzero((got != want) & care)[0]
            if bad.size:
                b = int(bad[0])
                w = b // 8 * 8
                wrong.append(f"{k}: {bad.size} wrong bytes, the first at byte {b} (8-byte word {b // 8}): "
                             f"{got[w:w + 8].tobytes().hex()}, expected {want[w:w + 8].tobytes().hex()}"
                             + (" -- written past what the contract allows" if want[b] == R.POISON else ""))
        if wrong:
            pytest.fail(f"{what}: " + "; ".join(wrong))


def _run(entry, fam, expects, call, rig, take_error=None, errs=None):
    """Steps 2 to 5 of the module's docstring.  call(): the library call on
    the current stream -> its return code.  take_error: the context whose
    cpk_ctx_take_error must say errs[i] (CPK_OK when None) after set i."""
    import torch
    names = [s.name for s in fam.sets]
    errs = errs or [R.OK] * len(names)

    def taken(i, stream=None):
        if take_error is not None:
            got = take_error.take_error(stream)
            assert got == errs[i], f"{entry}, set {names[i]}: cpk_ctx_take_error {got}, expected {errs[i]}"

    # 2. side-stream eager pass
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rig.load(0)
        rc = call()
    assert rc == R.OK, f"{entry}: eager on a side stream returned {rc}"
    side.synchronize()
    rig.check(expects[0], f"{entry}, eager on a side stream, set {names[0]}")
    taken(0, side)
    # 3. capture
    g = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(g):
        rcs.append(call())
    assert rcs == [R.OK], f"{entry}: returned {rcs[0]} while its stream was being captured"
    # 4. replays
    for i in range(len(names)):
        rig.load(i)
        g.replay()
        torch.cuda.synchronize()
        rig.check(expects[i], f"{entry}, replay {i}, set {names[i]}")
        taken(i)
    # 5. an eager call between replays
    k = len(names) - 2
    rig.load(k)
    rc = call()
    torch.cuda.synchronize()
    assert rc == R.OK, f"{entry}: eager after the replays returned {rc}"
    rig.check(expects[k], f"{entry}, eager after the replays, set {names[k]}")
    taken(k)
    rig.load(0)
    g.replay()
    torch.cuda.synchronize()
    rig.check(expects[0], f"{entry}, replay after an eager call, set {names[0]}")
    taken(0)
    return g


# ---- encoders ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["like", "units"])
@pytest.mark.parametrize("cap", ["trusted", "exact", "short"])
def test_encode_batch(ctx, kind, cap):
    """cpk_encode_batch and cpk_encode_batch_cap: out_cap the largest set's
    packed bytes exactly, and one byte short of them (that set's replay is
    CPK_ENOMEM and nothing at or past d_out + out_cap is stored)."""
    fam = R.encode_family(kind)
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    largest = max(int(s.facts["off"][-1]) for s in fam.sets)
    out_cap = {"trusted": None, "exact": largest, "short": largest - 1}[cap]
    both = [R.encode_expect(fam, s, out_cap) for s in fam.sets]
    expects, errs = [b[0] for b in both], [b[1] for b in both]
    assert (R.ENOMEM in errs) == (cap == "short")
    rig = Rig(fam, expects[0])
    if out_cap is None:
        call = lambda: L.cpk_encode_batch(h, rig.p("in"), rig.p("swo"), sc["n"], sc["max_seg_words"], rig.p("out"),
                                          rig.p("off"), _stream())
    else:
        call = lambda: L.cpk_encode_batch_cap(h, rig.p("in"), rig.p("swo"), sc["n"], sc["max_seg_words"],
                                              rig.p("out"), out_cap, rig.p("off"), _stream())
    _run("cpk_encode_batch" + ("_cap" if out_cap else ""), fam, expects, call, rig, take_error=ctx, errs=errs)


@pytest.mark.parametrize("which", ["small", "large"])
def test_encode_messages(ctx, which):
    fam = R.messages_family(which)
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [R.messages_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_encode_messages(h, rig.p("in"), rig.p("swo"), sc["nseg"], rig.p("mseg"), sc["nm"],
                                         sc["max_seg_words"], rig.p("out"), rig.p("off"), _stream())
    _run("cpk_encode_messages", fam, expects, call, rig, take_error=ctx)


@pytest.mark.parametrize("kind", ["like", "units"])
def test_packed_size_batch(own, kind):
    """The chunk form is reachable with the pieces of over one chunk, the wave
    form takes the others; CPK_SIZE_FORM is left alone."""
    fam = R.encode_family(kind)
    sc, L, h = fam.scalars, own._lib, own.handle
    expects = [R.size_expect(s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_packed_size_batch(h, rig.p("in"), rig.p("swo"), sc["n"], sc["max_seg_words"], rig.p("off"),
                                           _stream())
    _run("cpk_packed_size_batch", fam, expects, call, rig, take_error=own)


@pytest.mark.parametrize("which", ["small", "large"])
def test_packed_size_messages(ctx, which):
    fam = R.messages_family(which)
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [{"off": R.messages_expect(fam, s)["off"]} for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_packed_size_messages(h, rig.p("in"), rig.p("swo"), sc["nseg"], rig.p("mseg"), sc["nm"],
                                              sc["max_seg_words"], rig.p("off"), _stream())
    _run("cpk_packed_size_messages", fam, expects, call, rig, take_error=ctx)


def test_encode_batch_at(own):
    fam = R.encode_at_family()
    sc, L, h = fam.scalars, own._lib, own.handle
    expects = [R.encode_at_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_encode_batch_at(h, rig.p("in"), rig.p("swo"), sc["n"], sc["max_seg_words"], rig.p("grp"),
                                         sc["ng"], rig.p("out"), sc["out_cap"], rig.p("dst"), rig.p("cap"),
                                         rig.p("poff"), rig.p("glen"), rig.p("st"), _stream())
    _run("cpk_encode_batch_at", fam, expects, call, rig)


# ---- decoders ------------------------------------------------------------------------
def test_decode_batch(ctx):
    """n = 6: an uncaptured call reads its extent back, a captured one must not."""
    fam = R.decode_family()
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [R.decode_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_decode_batch(h, rig.p("pk"), rig.p("inoff"), rig.p("swo"), sc["n"], rig.p("out"),
                                      rig.p("st"), _stream())
    _run("cpk_decode_batch", fam, expects, call, rig)


def test_unpacked_size_batch(ctx):
    fam = R.decode_family()
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = []
    for s in fam.sets:
        e = R.unpacked_size_expect(s.facts["usz"])
        expects.append({"uswo": e["swo"], "ust": e["st"]})
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_unpacked_size_batch(h, rig.p("pk"), rig.p("inoff"), sc["n"], rig.p("uswo"), rig.p("ust"),
                                             _stream())
    _run("cpk_unpacked_size_batch", fam, expects, call, rig)


def test_decode_batch_at(own):
    fam = R.decode_at_family()
    sc, L, h = fam.scalars, own._lib, own.handle
    expects = [R.decode_at_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_decode_batch_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"), None,
                                         sc["n"], rig.p("swo"), sc["n"], rig.p("out"), rig.p("st"), rig.p("gst"),
                                         rig.p("gused"), _stream())
    _run("cpk_decode_batch_at", fam, expects, call, rig)


def test_unpacked_size_batch_at(own):
    fam = R.decode_at_family()
    sc, L, h = fam.scalars, own._lib, own.handle
    expects = []
    for s in fam.sets:
        e = R.unpacked_size_expect(s.facts["usz"])
        expects.append({"uswo": e["swo"], "ust": e["st"]})
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_unpacked_size_batch_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"),
                                                sc["n"], rig.p("uswo"), rig.p("ust"), _stream())
    _run("cpk_unpacked_size_batch_at", fam, expects, call, rig)


def test_decode_messages_at(own):
    """The fitting prefix and d_totals change from replay to replay."""
    fam = R.messages_at_family()
    sc, L, h = fam.scalars, own._lib, own.handle
    expects = [R.messages_at_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_decode_messages_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"), sc["nm"],
                                            sc["limit"], rig.p("out"), sc["out_cap_words"], rig.p("swo"),
                                            rig.p("sin"), rig.p("sst"), sc["seg_cap"], rig.p("mseg"), rig.p("mst"),
                                            rig.p("used"), rig.p("tot"), _stream())
    _run("cpk_decode_messages_at", fam, expects, call, rig)


@pytest.mark.parametrize("which", ["one-wave", "workgroup"])
def test_decode_stream(ctx, which):
    """Below 384 KiB only: from there on the call reads the word total back."""
    fam = R.stream_family(which)
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [R.stream_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_decode_stream(h, rig.p("pk"), sc["avail"], rig.p("swo"), sc["n"], rig.p("out"),
                                       rig.p("inoff"), rig.p("st"), _stream())
    _run("cpk_decode_stream", fam, expects, call, rig)


@pytest.mark.parametrize("which", ["small", "large"])
def test_read_message(ctx, which):
    fam = R.read_family(which)
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [R.read_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0])
    call = lambda: L.cpk_read_message(h, rig.p("pk"), sc["avail"], R.LIMIT, rig.p("out"), sc["out_cap_words"],
                                      rig.p("info"), _stream())
    _run("cpk_read_message", fam, expects, call, rig)


# ---- the benchmark's step in one graph -------------------------------------------------
def test_generate_encode_decode_count_chain(ctx):
    """cpk_generate -> cpk_encode_batch -> cpk_decode_batch -> cpk_count_mismatch
    captured as one graph and replayed with the piece sizes changed; then the
    checker itself, which must count one, two and three flipped words."""
    import torch
    import capnp_packed as cp
    fam = R.chain_family()
    sc, L, h = fam.scalars, ctx._lib, ctx.handle
    expects = [R.chain_expect(fam, s) for s in fam.sets]
    rig = Rig(fam, expects[0], zeroed=("cnt",))
    params = cp.preset(sc["cfg"])

    def count():
        return L.cpk_count_mismatch(h, rig.p("gen"), rig.p("dec"), sc["words"], rig.p("cnt"), _stream())

    def call():
        return (L.cpk_generate(h, ctypes.byref(params), rig.p("swo"), sc["n"], rig.p("gen"), _stream())
                or L.cpk_encode_batch(h, rig.p("gen"), rig.p("swo"), sc["n"], sc["max_seg_words"], rig.p("pk"),
                                      rig.p("off"), _stream())
                or L.cpk_decode_batch(h, rig.p("pk"), rig.p("off"), rig.p("swo"), sc["n"], rig.p("dec"), rig.p("st"),
                                      _stream())
                or count())

    _run("generate/encode/decode/count chain", fam, expects, call, rig, take_error=ctx)
    # set 0 is in place and decoded: flip one bit of three words of the decoded output
    total = int(fam.sets[0].facts["swo"][-1])
    mid = total // 2 + (1 if (total // 2) % 64 == 0 else 0)
    assert 0 < mid < total - 1 and mid % 64
    dec, cnt = rig.T["dec"].view(torch.int64), rig.T["cnt"].view(torch.int64)
    for k, (word, bit) in enumerate(((0, 0), (total - 1, 62), (mid, 17)), start=1):
        dec[word] ^= 1 << bit
        cnt.zero_()
        assert count() == R.OK
        torch.cuda.synchronize()
        assert int(cnt.cpu()[0]) == k, f"cpk_count_mismatch after {k} flipped words: {int(cnt.cpu()[0])}"


# ---- the single pass's epoch across its wrap ---------------------------------------------
def test_single_pass_epoch_wrap(oracle):
    """65,536 single-pass launches on one context: 64 pieces of 8192 config-2
    words at epoch 1, 65,533 launches of 2 pieces of 8 words with no
    synchronisation between them, then 64 pieces of 8192 config-3 words twice,
    at epochs 65535 and 1 -- the second across the wrap's clear, over words
    the first call tagged with epoch 1 too."""
    import torch
    import capnp_packed as cp
    c = _context(CPK_ENCODER="0")
    try:
        L, h = c._lib, c.handle
        swo = R.swo_of([8192] * 64)
        d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
        d_pk = torch.zeros(R.batch_capacity(swo), dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(65, dtype=torch.int64, device="cuda")

        def large(cfg):
            data = oracle.generate(oracle.preset(cfg), swo)
            want, woff = oracle.pack_batch(data, swo, threads=8)
            return torch.from_numpy(data.view(np.int64).copy()).cuda(), want.tobytes(), np.asarray(woff, np.uint64)

        def encode(d_in, want, woff, what):
            d_pk.zero_()
            d_off.fill_(-1)
            rc = L.cpk_encode_batch(h, d_in.data_ptr(), d_swo.data_ptr(), 64, 8192, d_pk.data_ptr(), d_off.data_ptr(),
                                    _stream())
            assert rc == cp.OK, what
            torch.cuda.synchronize()
            assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), woff), what
            assert d_pk.cpu().numpy()[:len(want)].tobytes() == want, what

        encode(*large(2), "epoch 1")
        s_swo = torch.tensor([0, 8, 16], dtype=torch.int64, device="cuda")
        s_in = torch.arange(1, 17, dtype=torch.int64, device="cuda")
        s_pk = torch.zeros(R.batch_capacity(np.array([0, 8, 16])), dtype=torch.uint8, device="cuda")
        s_off = torch.zeros(3, dtype=torch.int64, device="cuda")
        args = (h, s_in.data_ptr(), s_swo.data_ptr(), 2, 8, s_pk.data_ptr(), s_off.data_ptr(), _stream())
        t0 = time.perf_counter()
        for _ in range(65533):
            if L.cpk_encode_batch(*args) != cp.OK:
                pytest.fail("a small encode failed")
        three = large(3)
        encode(*three, "epoch 65535")
        encode(*three, "epoch 1, after the wrap")
        print(f"epoch wrap: 65,533 small launches and two large ones in {time.perf_counter() - t0:.1f} s")
        assert c.take_error() == cp.OK
    finally:
        c.close()
