"""Input sets for the device entry points under graph capture and replay
(tests/test_gpu_graph_replay.py), built on the CPU; tests/test_replay_cases.py
pins what each set is for.

A family is one entry point's list of input sets.  The sets of a family have
the same array lengths and the same host scalars -- what a captured launch has
baked in -- and differ in data and in the device-resident offset arrays, so
that consecutive replays of one graph must not depend on anything an earlier
replay (or an eager call) left behind: look-back and run-state words, ticket
and gate words, a form chosen once.

Every expectation comes from the oracle (oracle.pack_batch, oracle.pack,
oracle.write_message, oracle.unpack_batch, oracle.generate) or from the CPU
models that are themselves built on it (tests/_decode_at_cases.py,
tests/_messages_at_model.py, tests/_unpacked_size_model.py), never from the
library.  An expectation covers every byte of an output buffer and PAD bytes
past it: `want` holds the bytes, `care` is False where the contract leaves
them undefined, and a byte the contract says is untouched is wanted as POISON,
the pattern every output is filled with before a call.
"""
from __future__ import annotations

import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _decode_at_cases as D
import _messages_at_model as M
import _unpacked_size_model as U

OK, EINVAL, ETRUNC, EOVERRUN, ETRAILING, ENOMEM = 0, -1, -2, -3, -4, -5
POISON = 0xA5
PAD = 256          # poison bytes wanted intact after every output
CHUNK = 8192       # the single pass's unit, in words
LIMIT = 8 * 1024 * 1024

# name, generator preset, piece sizes in words
LIKE = (("a", 2, (8192, 8192, 8191, 4100, 8192, 6000)),
        ("b", 3, (4096, 8192, 5000, 8192, 4097, 8000)),
        ("c", 4, (8192, 8192, 8191, 4100, 8192, 6000)),
        ("d", 2, (8192, 100, 3, 0, 8192, 17)),
        ("e", 2, (8192, 8192, 8191, 4100, 8192, 6000)))
LIKE_MAXW = 8192
UNITS = (("a", 2, (20000, 12000, 16384)),
         ("b", 3, (16385, 20000, 10001)),
         ("c", 4, (20000, 12000, 16384)))
UNITS_MAXW = 20000

# inputs: name -> uint8 array (the bytes of the device tensor of that name);
# facts: what the oracle says of the set, for the expectations below
Set = namedtuple("Set", "name inputs facts")
Family = namedtuple("Family", "name scalars sets")


# ---- small helpers ---------------------------------------------------------------
def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def u64(v):
    return np.asarray(list(v), dtype=np.uint64)


def swo_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def padded(a, nbytes, fill=0):
    a = u8(a)
    assert a.size <= nbytes, (a.size, nbytes)
    out = np.full(nbytes, fill, np.uint8)
    out[:a.size] = a
    return out


def round16(x):
    return (int(x) + 15) // 16 * 16


def batch_capacity(swo):
    """cpk_batch_packed_capacity."""
    w = np.diff(np.asarray(swo, dtype=np.int64))
    return int(8 * w.sum() + 2 * ((w + 1) // 2).sum() + 16)


class Out:
    """One output buffer's expectation: nbytes + PAD bytes, POISON until put."""

    def __init__(self, nbytes):
        self.want = np.full(int(nbytes) + PAD, POISON, np.uint8)
        self.care = np.ones(int(nbytes) + PAD, bool)

    def put(self, off, data):
        b = u8(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data)
        assert off + b.size <= self.want.size - PAD
        self.want[off:off + b.size] = b
        self.care[off:off + b.size] = True
        return self

    def free(self, lo, hi):
        """[lo, hi): undefined by the contract."""
        self.care[int(lo):int(hi)] = False
        return self

    def done(self):
        return self.want, self.care


def i32(v):
    return np.asarray(list(v), dtype=np.int32)


# ---- pieces ------------------------------------------------------------------------
@lru_cache(maxsize=None)
def raw_pieces(kind):
    """The piece sets of LIKE / UNITS: per set a dict of the words, the word
    offsets and the oracle's packed bytes and offsets."""
    import oracle
    out = []
    for name, cfg, sizes in (LIKE if kind == "like" else UNITS):
        swo = swo_of(sizes)
        data = oracle.generate(oracle.preset(cfg), swo)
        packed, off = oracle.pack_batch(data, swo)
        out.append(dict(name=name, cfg=cfg, sizes=sizes, swo=swo, data=data, packed=np.array(packed),
                        off=np.asarray(off, dtype=np.uint64)))
    return out


def piece_bytes(r, i):
    return r["data"][8 * int(r["swo"][i]):8 * int(r["swo"][i + 1])].tobytes()


def piece_pack(r, i):
    return r["packed"][int(r["off"][i]):int(r["off"][i + 1])].tobytes()


def sampled_zero_share(data, swo):
    """The zero share of the words e4_minmax_kernel samples for a batch of at
    most 256 pieces (one block: 256 words, one in each of 256 equal stretches
    of the batch at a hashed position), as e4_gate_kernel and at_gate_kernel
    hold it against 85 %."""
    words = u8(data).view(np.uint64)
    a, T, G = int(swo[0]), int(swo[-1]) - int(swo[0]), 256
    st = T // G
    zero = 0
    for g in range(G):
        h = ((g * 2654435761) & 0xFFFFFFFF) ^ (g >> 7)
        zero += int(words[a + g * T // G + (h % st if st else 0)] == 0)
    return zero / G


# ---- encode: cpk_encode_batch[_cap], cpk_packed_size_batch --------------------------
@lru_cache(maxsize=None)
def encode_family(kind):
    raw = raw_pieces(kind)
    n = len(raw[0]["sizes"])
    in_bytes = 8 * max(int(r["swo"][-1]) for r in raw) + 8
    out_bytes = max(batch_capacity(r["swo"]) for r in raw)
    sets = [Set(r["name"], {"in": padded(r["data"], in_bytes), "swo": u8(r["swo"])}, r) for r in raw]
    return Family(f"encode-{kind}", dict(n=n, max_seg_words=LIKE_MAXW if kind == "like" else UNITS_MAXW,
                                         in_bytes=in_bytes, out_bytes=out_bytes), sets)


def encode_expect(fam, s, out_cap=None):
    """-> ({"out", "off"}, what cpk_ctx_take_error must say).  out_cap None:
    cpk_encode_batch, which may use its documented capacity."""
    r = s.facts
    total, off = int(r["off"][-1]), r["off"]
    cap = batch_capacity(r["swo"]) if out_cap is None else int(out_cap)
    out = Out(fam.scalars["out_bytes"])
    if total <= cap:
        out.put(0, r["packed"]).free(total, cap)
        err = OK
    else:
        # pieces wholly below out_cap as usual, the crossing one undefined,
        # nothing at or past out_cap
        k = next(i for i in range(len(off) - 1) if int(off[i + 1]) > cap)
        out.put(0, r["packed"][:int(off[k])]).free(int(off[k]), cap)
        err = ENOMEM
    return {"out": out.done(), "off": Out(8 * len(off)).put(0, off).done()}, err


def size_expect(s):
    return {"off": Out(8 * len(s.facts["off"])).put(0, s.facts["off"]).done()}


# ---- messages: cpk_encode_messages, cpk_packed_size_messages --------------------------
MSG_SMALL = dict(nm=8, seeds=(101, 202, 303), counts=(1, 2, 3, 4, 9), sizes=(0, 1, 17, 300, 2000, 9000), nseg=44,
                 maxw=9000)
MSG_LARGE = dict(nm=300, seeds=(404, 505, 606), counts=(1, 2, 3, 4), sizes=(0, 1, 17, 300), nseg=800, maxw=300)


def gen_messages(seed, nm, counts, sizes, nseg):
    """test_gpu_packed_size._messages' generator, the segment counts padded
    (one more segment per message, round robin) to `nseg` in all."""
    rng = np.random.default_rng(seed)
    cnt = [int(rng.choice(counts)) for _ in range(nm)]
    assert sum(cnt) <= nseg, (seed, sum(cnt))
    i = 0
    while sum(cnt) < nseg:
        cnt[i % nm] += 1
        i += 1
    msgs = []
    for c in cnt:
        ws = [int(rng.choice(sizes)) for _ in range(c)]
        msgs.append([(rng.integers(0, 256, size=8 * w, dtype=np.uint8) * (rng.random(8 * w) < 0.6))
                     .astype(np.uint8).tobytes() for w in ws])
    return msgs


def table_bytes(m):
    tb = struct.pack("<I", len(m) - 1) + b"".join(struct.pack("<I", len(s) // 8) for s in m)
    return tb + b"\0" * (-len(tb) % 8)


@lru_cache(maxsize=None)
def message_sets(which):
    """Per set: the messages, each one's oracle.write_message bytes, and the
    packed piece offsets in message order (table, segments) from oracle.pack."""
    import oracle
    spec = MSG_SMALL if which == "small" else MSG_LARGE
    out = []
    for seed in spec["seeds"]:
        msgs = gen_messages(seed, spec["nm"], spec["counts"], spec["sizes"], spec["nseg"])
        packs = [oracle.write_message(m) for m in msgs]
        off, o = [0], 0
        for m in msgs:
            for piece in [table_bytes(m)] + m:
                o += len(oracle.pack(piece))
                off.append(o)
        assert o == sum(len(p) for p in packs)
        out.append(dict(name=f"seed{seed}", msgs=msgs, packs=packs, off=u64(off)))
    return out


@lru_cache(maxsize=None)
def messages_family(which):
    spec = MSG_SMALL if which == "small" else MSG_LARGE
    raw = message_sets(which)
    per = []
    for r in raw:
        segs = [s for m in r["msgs"] for s in m]
        swo = swo_of([len(s) // 8 for s in segs])
        cap = batch_capacity(swo) + sum(10 * ((len(m) + 2) // 2 + 1) for m in r["msgs"])
        per.append((b"".join(segs), swo, swo_of([len(m) for m in r["msgs"]]), cap))
    in_bytes = max(len(p[0]) for p in per) + 8
    out_bytes = max(p[3] for p in per)
    sets = [Set(r["name"], {"in": padded(np.frombuffer(p[0], np.uint8), in_bytes), "swo": u8(p[1]), "mseg": u8(p[2])},
                r) for r, p in zip(raw, per)]
    return Family(f"messages-{which}", dict(nm=spec["nm"], nseg=spec["nseg"], max_seg_words=spec["maxw"],
                                            in_bytes=in_bytes, out_bytes=out_bytes), sets)


def messages_expect(fam, s):
    r = s.facts
    total = int(r["off"][-1])
    out = Out(fam.scalars["out_bytes"]).put(0, b"".join(r["packs"])).free(total, fam.scalars["out_bytes"])
    return {"out": out.done(), "off": Out(8 * len(r["off"])).put(0, r["off"]).done()}


# ---- decode: cpk_decode_batch, cpk_unpacked_size_batch ---------------------------------
DECODE_BAND = {"a": "map", "b": "dense", "c": "index", "cut": "map"}


@lru_cache(maxsize=None)
def decode_family():
    """The oracle-packed bytes of LIKE (a) to (c), and config-2 data of (b)'s
    sizes with piece 2's last 3 packed bytes left out of the stream."""
    import oracle
    like = raw_pieces("like")
    rows = [(r["name"], r["packed"].tobytes(), r["off"], r["swo"], r["data"]) for r in like[:3]]
    swo = like[1]["swo"]
    data = oracle.generate(oracle.preset(2), swo)
    pk, off = oracle.pack_batch(data, swo)
    packs = [pk[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(swo) - 1)]
    packs[2] = packs[2][:-3]
    rows.append(("cut", b"".join(packs), swo_of([len(p) for p in packs]), swo, data))
    pk_bytes = round16(max(len(r[1]) for r in rows)) + 16
    out_words = max(int(r[3][-1]) for r in rows)
    sets = []
    for name, pk, off, swo, data in rows:
        dec, st = oracle.unpack_batch(np.frombuffer(pk, np.uint8), off, swo)
        usz = [U.unpacked_size(pk[int(off[i]):int(off[i + 1])]) for i in range(len(swo) - 1)]
        facts = dict(name=name, pk=pk, off=off, swo=swo, data=data, dec=dec, st=st, usz=usz)
        sets.append(Set(name, {"pk": padded(np.frombuffer(pk, np.uint8), pk_bytes, 0xFF), "inoff": u8(off),
                               "swo": u8(swo)}, facts))
    return Family("decode", dict(n=len(swo) - 1, pk_bytes=pk_bytes, out_words=out_words), sets)


def decode_expect(fam, s):
    f = s.facts
    out = Out(8 * fam.scalars["out_words"])
    for i, st in enumerate(f["st"]):
        a, b = 8 * int(f["swo"][i]), 8 * int(f["swo"][i + 1])
        if st == OK:
            out.put(a, f["dec"][a:b])
        else:
            out.free(a, b)
    return {"out": out.done(), "st": Out(4 * len(f["st"])).put(0, i32(f["st"])).done()}


def unpacked_size_expect(usz):
    """[(status, words)] per piece -> the offsets and statuses."""
    return {"swo": Out(8 * (len(usz) + 1)).put(0, swo_of([w for _, w in usz])).done(),
            "st": Out(4 * len(usz)).put(0, i32(st for st, _ in usz)).done()}


# ---- cpk_encode_batch_at ------------------------------------------------------------------
# per set: the LIKE set its pieces come from, the groups' piece counts, the
# slots' order in the buffer, the group whose slot is a byte too small
AT_ENCODE = (("a", (2, 1, 3), (0, 1, 2), None), ("b", (1, 3, 2), (2, 1, 0), None),
             ("c", (3, 2, 1), (1, 2, 0), None), ("b", (2, 2, 2), (0, 2, 1), 1))


@lru_cache(maxsize=None)
def encode_at_family():
    like = {r["name"]: r for r in raw_pieces("like")}
    rows = []
    for k, (src, groups, order, short) in enumerate(AT_ENCODE):
        r = like[src]
        n, ng = len(r["sizes"]), len(groups)
        gpo = swo_of(groups)
        bodies = [b"".join(piece_pack(r, i) for i in range(int(gpo[g]), int(gpo[g + 1]))) for g in range(ng)]
        cap = [len(b) + (3 * g + k) % 5 for g, b in enumerate(bodies)]
        if short is not None:
            cap[short] = len(bodies[short]) - 1
        # slots in `order`, a gap of every alignment before each
        off, cur = [0] * ng, 5
        for j, g in enumerate(order):
            cur += D.default_gap(j + k)
            off[g] = cur
            cur += cap[g]
        rows.append(dict(name=f"{src}-{''.join(map(str, order))}" + ("-short" if short is not None else ""), r=r, gpo=gpo, bodies=bodies,
                         cap=cap, dst=off, end=cur, n=n, ng=ng))
    out_cap = max(x["end"] for x in rows) + 3
    in_bytes = 8 * max(int(x["r"]["swo"][-1]) for x in rows) + 8
    sets = [Set(x["name"], {"in": padded(x["r"]["data"], in_bytes), "swo": u8(x["r"]["swo"]), "grp": u8(x["gpo"]),
                            "dst": u8(u64(x["dst"])), "cap": u8(u64(x["cap"]))}, x) for x in rows]
    return Family("encode-at", dict(n=rows[0]["n"], ng=rows[0]["ng"], max_seg_words=LIKE_MAXW, out_cap=out_cap,
                                    in_bytes=in_bytes), sets)


def encode_at_expect(fam, s):
    x = s.facts
    out = Out(round16(fam.scalars["out_cap"]))
    st, poff = [], []
    for g in range(x["ng"]):
        body, d0 = x["bodies"][g], x["dst"][g]
        fits = len(body) <= x["cap"][g] and d0 + x["cap"][g] <= fam.scalars["out_cap"]
        st.append(OK if fits else ENOMEM)
        if fits:
            out.put(d0, body)
        else:  # (the bytes inside a refused group's own slot are undefined)
            out.free(d0, d0 + x["cap"][g])
        o = d0
        for i in range(int(x["gpo"][g]), int(x["gpo"][g + 1])):
            poff.append(o)
            o += len(piece_pack(x["r"], i))
    return {"out": out.done(), "poff": Out(8 * x["n"]).put(0, u64(poff)).done(),
            "glen": Out(8 * x["ng"]).put(0, u64(len(b) for b in x["bodies"])).done(),
            "st": Out(4 * x["ng"]).put(0, i32(st)).done()}


# ---- cpk_decode_batch_at, cpk_unpacked_size_batch_at -------------------------------------
# per set: the LIKE set, the slots' order, the filler between them, the piece
# whose range is 2 bytes longer than its packed bytes
AT_DECODE = (("a", "forward", "ff", None), ("b", "shuffled", "00ff", None), ("c", "reversed", "ff8ff", None),
             ("a", "shuffled", "ff", 3))


@lru_cache(maxsize=None)
def decode_at_family():
    import oracle
    like = {r["name"]: r for r in raw_pieces("like")}
    rows = []
    for src, order, filler, longer in AT_DECODE:
        r = like[src]
        n = len(r["sizes"])
        items = [piece_pack(r, i) for i in range(n)]
        if longer is not None:
            items[longer] += D.FILLERS[filler] * 2
        off, ln, in_cap, buf = D.place(items, order, filler=filler)
        rows.append(dict(name=f"{src}-{order}" + ("-trailing" if longer is not None else ""), r=r, off=off, ln=ln,
                         in_cap=in_cap, buf=buf, filler=filler, n=n))
    in_cap = max(x["in_cap"] for x in rows)
    out_words = max(int(x["r"]["swo"][-1]) for x in rows)
    sets = []
    for x in rows:
        pat = D.FILLERS[x["filler"]]
        buf = np.frombuffer((pat * (round16(in_cap) // len(pat) + 1))[:round16(in_cap)], np.uint8).copy()
        buf[:x["in_cap"]] = x["buf"]
        streams = D.extract(buf, x["off"], x["ln"])
        sizes = [int(w) for w in x["r"]["sizes"]]
        pst, pout, gst, used = D.batch_model(oracle, streams, [[w] for w in sizes])
        x.update(pst=pst, pout=pout, gst=gst, used=used, usz=[U.unpacked_size(b) for b in streams])
        sets.append(Set(x["name"], {"pk": buf, "srcoff": u8(x["off"]), "srclen": u8(x["ln"]),
                                    "swo": u8(x["r"]["swo"])}, x))
    return Family("decode-at", dict(n=rows[0]["n"], in_cap=in_cap, out_words=out_words), sets)


def decode_at_expect(fam, s):
    x = s.facts
    out = Out(8 * fam.scalars["out_words"])
    swo = x["r"]["swo"]
    for i, b in enumerate(x["pout"]):
        a, e = 8 * int(swo[i]), 8 * int(swo[i + 1])
        if b is None:
            out.free(a, e)
        else:
            out.put(a, b)
    return {"out": out.done(), "st": Out(4 * x["n"]).put(0, x["pst"]).done(),
            "gst": Out(4 * x["n"]).put(0, x["gst"]).done(), "gused": Out(8 * x["n"]).put(0, x["used"]).done()}


# ---- cpk_decode_messages_at ---------------------------------------------------------------
@lru_cache(maxsize=None)
def messages_at_family():
    """The small message sets, each message's oracle.write_message bytes in a
    slot of its own; out_cap_words is the smallest capacity at which the
    fitting prefix has a different length, neither none nor all, in every set."""
    import oracle
    raw = message_sets("small")
    nm, nseg = MSG_SMALL["nm"], MSG_SMALL["nseg"]
    rows = []
    for r, order, filler in zip(raw, D.ORDERS, ("ff", "00ff", "ff8ff")):
        off, ln, in_cap, buf = D.place(r["packs"], order, filler=filler)
        words = np.cumsum([sum(len(s) // 8 for s in m) for m in r["msgs"]])
        rows.append(dict(name=f"{r['name']}-{order}", msgs=r["msgs"], off=off, ln=ln, in_cap=in_cap, buf=buf,
                         filler=filler, cum=[int(w) for w in words]))
    in_cap = max(x["in_cap"] for x in rows)
    prefix = lambda x, cap: sum(1 for w in x["cum"] if w <= cap)
    out_cap = next(c for c in sorted({w for x in rows for w in x["cum"]})
                   if len({prefix(x, c) for x in rows}) == len(rows) and all(0 < prefix(x, c) < nm for x in rows))
    sets = []
    for x in rows:
        pat = D.FILLERS[x["filler"]]
        buf = np.frombuffer((pat * (round16(in_cap) // len(pat) + 1))[:round16(in_cap)], np.uint8).copy()
        buf[:x["in_cap"]] = x["buf"]
        model = M.batch(buf, x["off"], x["ln"], in_cap, LIMIT, out_cap, nseg)
        # the segments' packed starts: the table's packed bytes, then each segment's
        sin = [0] * model.F
        for m, msg in enumerate(x["msgs"]):
            if not model.fits[m]:
                continue
            assert model.status[m] == OK
            pos = int(x["off"][m]) + len(oracle.pack(table_bytes(msg)))
            for j, seg in enumerate(msg):
                sin[model.mseg[m] + j] = pos
                pos += len(oracle.pack(seg))
            assert pos == int(x["off"][m]) + int(model.used[m])
        x.update(model=model, sin=sin, prefix=prefix(x, out_cap))
        sets.append(Set(x["name"], {"pk": buf, "srcoff": u8(x["off"]), "srclen": u8(x["ln"])}, x))
    return Family("messages-at", dict(nm=nm, in_cap=in_cap, out_cap_words=out_cap, seg_cap=nseg, limit=LIMIT), sets)


def messages_at_expect(fam, s):
    x, sc = s.facts, fam.scalars
    m = x["model"]
    out = Out(8 * sc["out_cap_words"])
    for i, segs in enumerate(m.segs):
        if segs is not None:
            out.put(8 * m.swo[m.mseg[i]], b"".join(segs))
    return {"out": out.done(),
            "swo": Out(8 * (sc["seg_cap"] + 1)).put(0, u64(m.swo)).done(),
            "sin": Out(8 * sc["seg_cap"]).put(0, u64(x["sin"])).done(),
            "sst": Out(4 * sc["seg_cap"]).put(0, i32([OK] * m.F)).done(),
            "mseg": Out(8 * (sc["nm"] + 1)).put(0, u64(m.mseg)).done(),
            "mst": Out(4 * sc["nm"]).put(0, m.status).done(),
            "used": Out(8 * sc["nm"]).put(0, m.used).done(),
            "tot": Out(8 * 3).put(0, u64(m.totals)).done()}


# ---- cpk_decode_stream ---------------------------------------------------------------------
STREAMS = {"one-wave": dict(avail=6000, sets=((2, (100, 0, 300)), (3, (250, 7, 60)), (4, (300, 90, 0)))),
           "workgroup": dict(avail=200 * 1024, sets=((2, (8192, 100, 4000)), (3, (4000, 8192, 3000)),
                                                     (4, (8192, 8000, 8192))))}


@lru_cache(maxsize=None)
def stream_family(which):
    """Pieces back to back in one stream of `avail` bytes; the bytes after
    them are the same stream again (later messages, not to be consumed)."""
    import oracle
    spec = STREAMS[which]
    avail = spec["avail"]
    rows = []
    for cfg, sizes in spec["sets"]:
        swo = swo_of(sizes)
        data = oracle.generate(oracle.preset(cfg), swo)
        pk, off = oracle.pack_batch(data, swo)
        assert 0 < len(pk) <= avail
        rows.append(dict(name=f"cfg{cfg}", swo=swo, data=data, off=np.asarray(off, np.uint64),
                         pk=(pk.tobytes() * (avail // len(pk) + 2))[:avail]))
    out_words = max(int(r["swo"][-1]) for r in rows)
    sets = [Set(r["name"], {"pk": padded(np.frombuffer(r["pk"], np.uint8), round16(avail) + 16, 0xFF),
                            "swo": u8(r["swo"])}, r) for r in rows]
    return Family(f"stream-{which}", dict(n=len(rows[0]["swo"]) - 1, avail=avail, out_words=out_words), sets)


def stream_expect(fam, s):
    r = s.facts
    n = fam.scalars["n"]
    return {"out": Out(8 * fam.scalars["out_words"]).put(0, r["data"]).done(),
            "inoff": Out(8 * (n + 1)).put(0, r["off"]).done(),
            "st": Out(4 * n).put(0, i32([OK] * n)).done()}


# ---- cpk_read_message ----------------------------------------------------------------------
MSG_HEAD_WORDS, MSG_INFO_WORDS = 257, 517
READS = {"small": dict(avail=4096, cap=600, sets=((2, (3, 0, 40)), (3, (100, 7)), (4, (1, 1, 1, 200)))),
         "large": dict(avail=120000, cap=12000, sets=((3, (9000, 512)), (2, (6000, 5900, 100)), (3, (512, 8400))))}


@lru_cache(maxsize=None)
def read_family(which):
    """One message at the front of `avail` bytes, a second message and 0xFF
    bytes after it."""
    import oracle
    spec = READS[which]
    avail = spec["avail"]
    rows = []
    for cfg, sizes in spec["sets"]:
        swo = swo_of(sizes)
        data = oracle.generate(oracle.preset(cfg), swo)
        segs = [data[8 * int(swo[i]):8 * int(swo[i + 1])].tobytes() for i in range(len(sizes))]
        pk = oracle.write_message(segs)
        st, got, used = oracle.read_message(pk + oracle.write_message([b"\1" * 32, b""]), out_cap=8 * spec["cap"])
        assert (st, got, used) == (OK, segs, len(pk)) and len(pk) + 64 <= avail
        rows.append(dict(name=f"cfg{cfg}-{len(sizes)}seg", segs=segs, used=used,
                         pk=padded(np.frombuffer(pk + oracle.write_message([b"\1" * 32, b""]), np.uint8),
                                   round16(avail) + 16, 0xFF)))
    sets = [Set(r["name"], {"pk": r["pk"]}, r) for r in rows]
    return Family(f"read-{which}", dict(avail=avail, out_cap_words=spec["cap"]), sets)


def read_expect(fam, s):
    """d_info: status, bytes consumed, count, words, the segments' word
    offsets behind the table's words; d_out: the table's words, the segments."""
    r = s.facts
    segs = r["segs"]
    count, words = len(segs), [len(x) // 8 for x in segs]
    head = 1 + (count & ~1) // 2
    info = [0, r["used"], count, sum(words)] + [head + int(v) for v in swo_of(words)]
    cap_bytes = 8 * (fam.scalars["out_cap_words"] + MSG_HEAD_WORDS)
    out = Out(cap_bytes).put(0, table_bytes(segs) + b"".join(segs)).free(8 * (head + sum(words)), cap_bytes)
    return {"out": out.done(),
            "info": Out(8 * MSG_INFO_WORDS).put(0, u64(info)).free(8 * len(info), 8 * MSG_INFO_WORDS).done()}


# ---- the benchmark's chain ------------------------------------------------------------------
CHAIN_CFG = 2
CHAIN_SIZES = (LIKE[0][2], LIKE[1][2], LIKE[3][2])  # like-sized, like-sized, unlike: both encoders in one graph


@lru_cache(maxsize=None)
def chain_family():
    """cpk_generate -> cpk_encode_batch -> cpk_decode_batch -> cpk_count_mismatch
    with the generator's parameters fixed and the piece sizes changing."""
    import oracle
    rows = []
    for sizes in CHAIN_SIZES:
        swo = swo_of(sizes)
        data = oracle.generate(oracle.preset(CHAIN_CFG), swo)
        packed, off = oracle.pack_batch(data, swo)
        rows.append(dict(name="-".join(str(w) for w in sizes), swo=swo, data=data, packed=np.array(packed),
                         off=np.asarray(off, np.uint64)))
    words = max(int(r["swo"][-1]) for r in rows)
    out_bytes = max(batch_capacity(r["swo"]) for r in rows)
    sets = [Set(r["name"], {"swo": u8(r["swo"])}, r) for r in rows]
    return Family("chain", dict(n=len(CHAIN_SIZES[0]), max_seg_words=LIKE_MAXW, words=words, out_bytes=out_bytes,
                                cfg=CHAIN_CFG), sets)


def chain_expect(fam, s):
    r = s.facts
    n, sc = fam.scalars["n"], fam.scalars
    total, w = int(r["off"][-1]), 8 * int(r["swo"][-1])
    return {"gen": Out(8 * sc["words"] + 8).put(0, r["data"]).done(),
            "pk": Out(sc["out_bytes"]).put(0, r["packed"]).free(total, batch_capacity(r["swo"])).done(),
            "off": Out(8 * (n + 1)).put(0, r["off"]).done(),
            "dec": Out(8 * sc["words"] + 8).put(0, r["data"]).done(),
            "st": Out(4 * n).put(0, i32([OK] * n)).done(),
            "cnt": Out(8).put(0, u64([0])).done()}
