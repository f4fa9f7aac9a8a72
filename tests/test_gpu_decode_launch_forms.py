"""The decode launch layer's branches under graph capture that no other file
forces (host_api.hip: dec_each_form, dec_launch): test_gpu_graph_replay.py
captures cpk_decode_batch_at and cpk_decode_messages_at with the device's gate
alone and without groups.  Here: the range-per-piece forms and
cpk_decode_messages_at under a forced decoder (no gate kernel, one form, no
skip word), and the grouped forms under the gate and under each forced decoder.

Every case goes through test_gpu_graph_replay.py's _run (eager on a side
stream, captured, replayed per input set, an eager call between replays) and is
compared bit for bit with the expectation the oracle gives (tests/_replay_cases.py,
tests/_decode_at_cases.py), never with the library alone.  The pieces are the
replay cases' six per set (8192 words at most, an empty and a 3-word one among
them); the groups hold 2, 1 and 3 of them."""
from functools import lru_cache

import numpy as np
import pytest

import _decode_at_cases as D
import _replay_cases as R
import test_gpu_graph_replay as G

pytestmark = pytest.mark.gpu

GROUPS = (2, 1, 3)
# per set: the LIKE set, the slots' order, the filler between them
GROUPED = (("a", "forward", "ff"), ("d", "shuffled", "00ff"), ("c", "reversed", "ff8ff"))


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.fixture
def dctx(request):
    """A context under the test's `decoder` parameter (CPK_DECODER; None: the device's gate)."""
    d = request.getfixturevalue("decoder")
    c = G._context(**({} if d is None else {"CPK_DECODER": d}))
    yield c
    c.close()


FORCED = pytest.mark.parametrize("decoder", ["1", "2"], ids=["dec-block-map", "dec-index"])
EVERY = pytest.mark.parametrize("decoder", [None, "1", "2"], ids=["dec-auto", "dec-block-map", "dec-index"])


@lru_cache(maxsize=None)
def grouped_family():
    """decode_at_family's pieces in groups: a slot per group, its pieces' packed bytes back to back."""
    import oracle
    like = {r["name"]: r for r in R.raw_pieces("like")}
    gpo = R.swo_of(GROUPS)
    rows = []
    for src, order, filler in GROUPED:
        r = like[src]
        assert len(r["sizes"]) == int(gpo[-1])
        items = [b"".join(R.piece_pack(r, i) for i in range(int(gpo[g]), int(gpo[g + 1]))) for g in range(len(GROUPS))]
        off, ln, in_cap, buf = D.place(items, order, filler=filler)
        rows.append(dict(name=f"{src}-{order}", r=r, off=off, ln=ln, in_cap=in_cap, buf=buf, filler=filler))
    in_cap = max(x["in_cap"] for x in rows)
    sets = []
    for x in rows:
        pat = D.FILLERS[x["filler"]]
        buf = np.frombuffer((pat * (R.round16(in_cap) // len(pat) + 1))[:R.round16(in_cap)], np.uint8).copy()
        buf[:x["in_cap"]] = x["buf"]
        sizes = [int(w) for w in x["r"]["sizes"]]
        groups = [sizes[int(gpo[g]):int(gpo[g + 1])] for g in range(len(GROUPS))]
        pst, pout, gst, used = D.batch_model(oracle, D.extract(buf, x["off"], x["ln"]), groups)
        assert (pst == R.OK).all() and (gst == R.OK).all() and list(used) == [int(v) for v in x["ln"]]
        x.update(pst=pst, pout=pout, gst=gst, used=used)
        sets.append(R.Set(x["name"], {"pk": buf, "srcoff": R.u8(x["off"]), "srclen": R.u8(x["ln"]), "grp": R.u8(gpo),
                                      "swo": R.u8(x["r"]["swo"])}, x))
    return R.Family("decode-at-grouped", dict(n=int(gpo[-1]), ng=len(GROUPS), in_cap=in_cap,
                                              out_words=max(int(x["r"]["swo"][-1]) for x in rows)), sets)


def grouped_expect(fam, s):
    x, sc = s.facts, fam.scalars
    out = R.Out(8 * sc["out_words"])
    for i, b in enumerate(x["pout"]):
        out.put(8 * int(x["r"]["swo"][i]), b)
    return {"out": out.done(), "st": R.Out(4 * sc["n"]).put(0, x["pst"]).done(),
            "gst": R.Out(4 * sc["ng"]).put(0, x["gst"]).done(), "gused": R.Out(8 * sc["ng"]).put(0, x["used"]).done()}


@EVERY
def test_grouped_forms_captured(dctx, decoder):
    """cpk_decode_batch_at with groups (the stream forms, a wave per group):
    under the gate all three forms are captured, under a forced decoder one."""
    fam = grouped_family()
    sc, L, h = fam.scalars, dctx._lib, dctx.handle
    expects = [grouped_expect(fam, s) for s in fam.sets]
    rig = G.Rig(fam, expects[0])
    call = lambda: L.cpk_decode_batch_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"), rig.p("grp"),
                                         sc["ng"], rig.p("swo"), sc["n"], rig.p("out"), rig.p("st"), rig.p("gst"),
                                         rig.p("gused"), G._stream())
    G._run("cpk_decode_batch_at (groups)", fam, expects, call, rig)


@FORCED
def test_range_per_piece_forms_forced_captured(dctx, decoder):
    """cpk_decode_batch_at without groups under a forced decoder: decode_at_kernel
    or decode2_at_kernel alone, no gate kernel in the graph (the gate's case is
    test_gpu_graph_replay.py::test_decode_batch_at)."""
    fam = R.decode_at_family()
    sc, L, h = fam.scalars, dctx._lib, dctx.handle
    expects = [R.decode_at_expect(fam, s) for s in fam.sets]
    rig = G.Rig(fam, expects[0])
    call = lambda: L.cpk_decode_batch_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"), None,
                                         sc["n"], rig.p("swo"), sc["n"], rig.p("out"), rig.p("st"), rig.p("gst"),
                                         rig.p("gused"), G._stream())
    G._run("cpk_decode_batch_at (forced)", fam, expects, call, rig)


@FORCED
def test_decode_messages_at_forced_captured(dctx, decoder):
    """cpk_decode_messages_at under a forced decoder: one stream form, no gate
    (the gate's case is test_gpu_graph_replay.py::test_decode_messages_at)."""
    fam = R.messages_at_family()
    sc, L, h = fam.scalars, dctx._lib, dctx.handle
    expects = [R.messages_at_expect(fam, s) for s in fam.sets]
    rig = G.Rig(fam, expects[0])
    call = lambda: L.cpk_decode_messages_at(h, rig.p("pk"), sc["in_cap"], rig.p("srcoff"), rig.p("srclen"), sc["nm"],
                                            sc["limit"], rig.p("out"), sc["out_cap_words"], rig.p("swo"),
                                            rig.p("sin"), rig.p("sst"), sc["seg_cap"], rig.p("mseg"), rig.p("mst"),
                                            rig.p("used"), rig.p("tot"), G._stream())
    G._run("cpk_decode_messages_at (forced)", fam, expects, call, rig)
