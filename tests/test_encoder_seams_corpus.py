"""The encoder seam corpus (tests/_encoder_seams.py) pinned on the CPU: every
case is what its name says (walked word class by word class in plain Python,
heads and counts read back from the oracle's packed bytes), and the
mask-algebra model of tools/step_model.py packs the planted cases as the
oracle does.  tests/test_gpu_encoder_seams.py runs the corpora on the GPU.
No GPU needed.
"""
import re

import numpy as np
import pytest

import _encoder_seams as S
from _packed_records import parse_records

# the model pass runs on every MODEL_STRIDE-th case of each planted family
# (the full pass takes about 6 s on its own, which with the walks is over the
# module's budget; at this stride the module runs in about 4 s)
MODEL_STRIDE = 4


@pytest.fixture(scope="module")
def corpora():
    yield S.corpora()
    S.release()


@pytest.fixture(scope="module")
def packed(oracle, corpora):
    """{corpus: (packed bytes, offsets)} by the oracle, one batch each."""
    out = {}
    for name, cases in corpora.items():
        data, swo = S.batch_arrays(cases)
        out[name] = oracle.pack_batch(data, swo, threads=8)
    return out


def _piece_packed(packed, name, i):
    pk, off = packed[name]
    return pk[int(off[i]):int(off[i + 1])].tobytes()


def test_constants_are_the_sources():
    """Named constants are parsed from the kernel sources, the unnamed ones
    pinned to the text of the line they were read from."""
    assert set(S.CONST) == set(S._CONSTANTS) and all(v > 0 for v in S.CONST.values())
    S.check_pins()
    assert S.GROUP == S.STEP * S.GROUP_STEPS == 4096 and S.WAVE == 2048
    assert S.kE4ScanBlock == S.CONST["kE4ScanThreads"] * S.CONST["kE4ScanPer"]
    assert S.MANY == (S.kE4ScanBlock - 1, S.kE4ScanBlock, S.kE4ScanBlock + 1, 2 * S.kE4ScanBlock + 1)
    # the ring holds whole 16-byte lines, a string's overhang (three dwords) fits the overhang lines
    assert S.kE4RingBytes % 16 == 0 and 16 * S.kE4Ov >= 12
    # either side of the loads' batches, 64 PF and 64 EPF words
    assert {S.EPF - 1, S.EPF, S.EPF + 1, S.PF, S.PF + 1} <= set(S.STEP_K)


def test_names_and_counts(corpora):
    """Names are unique; every family has the cases its sweep implies."""
    names = [c.name for cs in corpora.values() for c in cs]
    assert len(set(names)) == len(names)
    names = set(names)
    n = {k: len(v) for k, v in corpora.items()}
    # step: 6 edges x 4 kinds x 4 d x 5 lengths x start / end = 960, less the
    # 24 runs that would start before word 0, and 2 wave edges x 160
    assert n["step"] == 936 + 320
    assert n["group"] == 160 + 36 + 18
    assert n["zcap"] == 28 + 6 + 4 + 4
    assert n["long"] == 2 * 3 * 7 * 2
    assert n["count"] == 238
    assert n["ring"] == 2 * 3 * 11 + 2 * 2 * 16
    assert n["lines"] == 600 and n["sizes"] == 19
    assert [n[f"many{k}"] for k in (4095, 4096, 4097, 8193)] == [4095, 4096, 4097, 8193]
    for seam, ks in (("step64", [64 * k for k in (1, 3, 4, 5, 8, 9)]), ("step2048", [2048, 6144]),
                     ("grp4096", [4096])):
        for at in ks:
            for kind in ("zero", "dense", "dense+L", "L"):
                for d in (-2, -1, 0, 1):
                    for ln in (1, 2, 63, 64, 65):
                        assert f"{seam}/{kind}/start@{at}{d:+d}/len{ln}" in names
                        assert f"{seam}/{kind}/end@{at}{d:+d}/len{ln}" in names or at + d - ln < 0
    for kind in ("zero", "dense", "dense+L", "L"):
        assert f"grp4096/{kind}/cover-1+1/len4098" in names and f"grp4096/{kind}/cover-300+300/len4696" in names
    for x in (255, 256, 257):
        for kind in ("dense", "dense+L", "D+L"):
            assert f"grp4096/{kind}/head@-{x}/len{x + 100}" in names
    for ln in (255, 256, 257, 511, 512, 513, 769):
        for lane in (0, 31, 32, 63):
            assert f"zcap/zero/cap@step6.lane{lane}/len{ln}" in names
    for d in (-1, 0):
        assert f"zcap/zero/cap1@4096{d:+d}/len257" in names and f"zcap/zero/cap2@4096{d:+d}/len769" in names
        assert sum(nm.startswith("zcap/zero/carried-") and f"cap@8192{d:+d}" in nm for nm in names) == 2
    for seam in ("step320", "grp4096"):
        for kind in ("dense", "D+L", "L+D"):
            for e in (191, 192, 193):
                assert f"{seam}/{kind}/enter{e}@+0/len600" in names
    for tag in ("zero", "ff"):
        for h in (0, 31, 32, 63):
            for run in (255, 256, 257, 64 - h, 127 - h, 5 * 64 - h, 5 * 64 + 63 - h):
                assert f"count/{tag}/head@step2.lane{h}/run{run}" in names
            for j in range(5):
                assert f"count/{tag}/head@last-{j}.lane{h}/toend/W512" in names
        for run in (31, 32, 33, 34):
            assert f"count/{tag}/head@step2.lane0/run{run}" in names
    for probe in ("ff10", "z2", "mem8"):
        for k in range(1, 12):
            for r in (1, 3):
                assert f"ring/{probe}/ring@2048-{k}/round{r}" in names
    for ph in range(16):
        assert f"ring/dense/obase%16={ph}/len800" in names and f"ring/dense+L/obase%16={ph}/len800" in names
    assert {(c.nwords + 63) // 64 % 8 for c in corpora["sizes"]} == set(range(8))
    assert {c.nwords for c in corpora["sizes"]} >= {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097,
                                                    8191, 8192, 8193}
    # pieces as short as their seam allows
    assert max(c.nwords for c in corpora["step"] if c.name.startswith("step64/")) <= 64 * 9 + 1 + 65 + 70
    assert max(c.nwords for c in corpora["long"] + corpora["count"]) <= 4096 + 700
    assert max(c.nwords for c in corpora["group"] + corpora["zcap"]) == 3 * 4096 + 1


ALLOWED = {"zero": "Z+", "dense": "D+", "dense+L": "(DDL)*D{0,2}", "L": "L+", "D+L": "DL*", "L+D": "L*DL*"}


def _check_run(c, cls):
    """The planted run is of its kind, between background words, and nothing
    else is planted."""
    s, ln = c.meta["start"], c.meta["length"]
    run = cls[s:s + ln]
    assert len(run) == ln and re.fullmatch(ALLOWED[c.meta["kind"]], run), c.name
    assert set(cls[:s]) <= {"M"} and set(cls[s + ln:]) <= {"M"}, c.name
    # (the piece goes on after the run: its end is decided by a word, not by the piece's)
    assert s + ln < len(cls) or "/toend/" in c.name, c.name


@pytest.mark.parametrize("family", ["step", "group", "zcap", "long"])
def test_planted_runs_stand_where_the_names_say(corpora, packed, family):
    """Walked from the bytes alone: the run's start and end against the
    position in the name; for `long` the stretch's length where it enters the
    named step; for `zcap` the cap head, a 00 record of the oracle's packed
    bytes, at the named word."""
    for i, c in enumerate(corpora[family]):
        cls = S.word_classes(c.words)
        assert len(cls) == c.nwords
        _check_run(c, cls)
        s, ln = c.meta["start"], c.meta["length"]
        seam, kind, where = c.name.split("/")[:3]
        assert f"/len{ln}" in c.name and kind == c.meta["kind"]
        m = re.fullmatch(r"(start|end)@(\d+)([+-]\d)", where)
        if m:
            at = int(m.group(2)) + int(m.group(3))
            assert int(m.group(2)) % 64 == 0 and seam in (f"step64", "step2048", "grp4096")
            assert (s if m.group(1) == "start" else s + ln) == at, c.name
            assert cls[at] == ("M" if m.group(1) == "end" else cls[s]) and (s == 0 or cls[s - 1] == "M")
        elif where.startswith("cover-"):
            a, b = (int(x) for x in where[6:].split("+"))
            assert (s, s + ln) == (4096 - a, 8192 + b) and c.nwords == 3 * 4096 + 1, c.name
        elif where.startswith("head@-"):
            x = int(where[6:])
            assert s == 4096 - x and cls[s] == "D" and s + ln > 4096 + 64, c.name
            if kind == "D+L":  # it stays the first group's last head
                assert "D" not in cls[s + 1:]
        elif where.startswith("enter"):
            e = int(re.fullmatch(r"enter(\d+)@\+0", where).group(1))
            at = {"step320": 320, "grp4096": 4096}[seam]
            assert at - s == e and s + ln >= at + 64, c.name
            assert set(cls[s:at]) == ({"D"} if kind == "dense" else {"L"} if kind == "L+D" else {"D", "L"})
            if kind == "L+D":   # no head when the step is entered
                assert cls[at + 10] == "D" and cls.count("D") == 1, c.name
        else:
            assert family == "zcap", c.name
        if family == "zcap":
            recs = {w: k for _, w, k in parse_records(_piece_packed(packed, family, i))}
            heads = sorted(w for w, k in recs.items() if k[0] == "Z")
            assert heads == list(range(s, s + ln, 256)), c.name
            assert recs[s] == f"Z{min(ln - 1, 255)}" and recs[heads[-1]] == f"Z{(ln - 1) % 256}", c.name
            cap = c.meta["cap"]
            if ln <= 256:
                assert cap is None and len(heads) == 1
                continue
            assert cap in heads and (cap - s) % 256 == 0, c.name
            m = re.fullmatch(r"cap@step6\.lane(\d+)", where)
            if m:
                assert cap == s + 256 == 64 * 6 + int(m.group(1)), c.name
            elif where.startswith("carried-from"):
                d = int(c.name.split("cap@8192")[1].split("/")[0])
                assert cap == 8192 + d and s == int(where[12:]) <= 4096 and s + ln > 8192 + 64, c.name
            else:
                nth, d = re.fullmatch(r"cap(\d)@4096([+-]\d)", where).groups()
                assert cap == 4096 + int(d) == s + 256 * int(nth), c.name


def test_count_heads_carry_the_named_count(corpora, packed):
    """From the oracle's packed bytes: the head named by the case carries
    min(run - 1, 255); a run of 257 and more gives 255, then a new head."""
    for i, c in enumerate(corpora["count"]):
        cls = S.word_classes(c.words)
        _check_run(c, cls)
        head, ln = c.meta["head"], c.meta["length"]
        assert head == c.meta["start"]
        tag, where = c.name.split("/")[1:3]
        letter = {"zero": "Z", "ff": "F"}[tag]
        m = re.fullmatch(r"head@step2\.lane(\d+)", where)
        if m:
            assert head == 128 + int(m.group(1)) and c.name.endswith(f"/run{ln}"), c.name
            assert c.nwords % 64 in (0, 1, 63) and c.nwords > head + ln
        else:
            j, lane = (int(x) for x in re.fullmatch(r"head@last-(\d)\.lane(\d+)", where).groups())
            assert head == 64 * ((c.nwords + 63) // 64 - 1 - j) + lane and head + ln == c.nwords, c.name
            assert c.nwords % 64 in (0, 1, 63)
        recs = {w: k for _, w, k in parse_records(_piece_packed(packed, "count", i))}
        assert recs[head] == f"{letter}{min(ln - 1, 255)}" == f"{letter}{c.meta['count']}", c.name
        if ln > 256:
            assert recs[head + 256] == f"{letter}{min(ln - 257, 255)}", c.name
        else:
            assert not any(k[0] in "ZF" for w, k in recs.items() if w != head), c.name
    runs = {(c.name.split("/")[1], c.meta["length"]): c.meta["count"] for c in corpora["count"]}
    assert [runs["ff", n] for n in (255, 256, 257)] == [254, 255, 255]
    assert [runs["zero", n] for n in (255, 256, 257)] == [254, 255, 255]


def test_ring_strings_lie_at_the_ring_end(oracle, corpora, packed):
    """len(oracle.pack(prefix)) % 2048 == 2048 - k, the next string is the
    10-, 2- or 8-byte one, and in the batch every position case starts at a
    multiple of the ring; the dense stretches pack at 8 bytes per word and
    more and start at every obase % 16."""
    pk, off = packed["ring"]
    phases = {"dense": set(), "dense+L": set()}
    for i, c in enumerate(corpora["ring"]):
        kind = c.meta["kind"]
        if kind == "filler":
            continue
        if kind in phases:
            assert len(oracle.pack(c.words[: 8 * S.RING_DENSE])) >= 8 * S.RING_DENSE >= 3 * S.kE4RingBytes, c.name
            assert int(off[i]) == c.meta["obase"] and int(off[i]) % 16 == int(c.name.split("%16=")[1].split("/")[0])
            phases[kind].add(int(off[i]) % 16)
            continue
        k, npre = c.meta["k"], c.meta["prefix"]
        P = len(oracle.pack(c.words[: 8 * npre]))
        assert P % S.kE4RingBytes == S.kE4RingBytes - k and f"-{k}/round" in c.name, c.name
        assert int(off[i]) % S.kE4RingBytes == 0, c.name
        recs = {p: (w, kd) for p, w, kd in parse_records(_piece_packed(packed, "ring", i))}
        if kind == "ff10":
            assert recs[P] == (npre, "F0") and P + 10 in recs, c.name
        elif kind == "z2":
            assert recs[P] == (npre, "Z0") and P + 2 in recs, c.name
        else:  # the member's 8 bytes follow the head's ten
            assert recs[P - 10] == (npre - 1, "F1") and P + 8 in recs and P not in recs, c.name
    assert phases == {"dense": set(range(16)), "dense+L": set(range(16))}
    assert {c.meta["k"] for c in corpora["ring"] if "k" in c.meta} == set(range(1, 12))


def test_small_pieces_share_lines(corpora, packed):
    """lines: several pieces start in one 16-byte output line, empty pieces
    first, last and in between.  many: the scan's block edges."""
    cases = corpora["lines"]
    _, off = packed["lines"]
    assert cases[0].nwords == 0 and cases[-1].nwords == 0 and sum(c.nwords == 0 for c in cases) >= 120
    assert {c.nwords for c in cases} == {0, 1, 2, 3}
    starts = np.bincount((off[:-1] // 16).astype(np.int64))
    assert (starts >= 3).sum() >= 50, starts.max()
    for n in S.MANY:
        assert {c.nwords for c in corpora[f"many{n}"]} == {0, 1, 2, 3}


def test_model_packs_the_planted_cases_as_the_oracle(corpora, packed):
    """tools/step_model.encode_model (the single pass's mask algebra, chunks
    of 128 steps, waves of 32) == the oracle on a fixed-stride subsample of
    the planted families, which still holds every family, every offset d,
    every kind and every length of the edge sweeps."""
    import step_model
    seen = {"d": set(), "kind": set(), "len": set(), "where": set()}
    bad, n = [], 0
    for family in S.PLANTED:
        cases = corpora[family]
        pick = range(0, len(cases), MODEL_STRIDE)
        assert len(pick) >= 10, family
        for i in pick:
            c = cases[i]
            n += 1
            if "d" in c.meta:
                seen["d"].add(c.meta["d"])
                seen["len"].add(c.meta["length"])
                seen["where"].add((c.name.split("/")[0], c.meta["side"]))
            seen["kind"].add(c.meta["kind"])
            if step_model.encode_model(c.words, 32, 4) != _piece_packed(packed, family, i):
                bad.append(c.name)
    assert not bad, (len(bad), bad[:8])
    assert seen["d"] == set(S.EDGE_D) and seen["len"] == set(S.EDGE_LEN)
    assert seen["kind"] == set(S.KINDS) | {"D+L", "L+D"}
    assert seen["where"] == {(s, side) for s in ("step64", "step2048", "grp4096") for side in ("start", "end")}
    print(f"\nmodel == oracle on {n} of {sum(len(corpora[f]) for f in S.PLANTED)} planted cases")


def test_corpus_totals(corpora, packed):
    """No corpus, which is what one GPU call moves, passes 64 MiB packed or
    256 MiB unpacked; the totals are printed."""
    print()
    for name, cases in corpora.items():
        P, U = len(packed[name][0]), 8 * sum(c.nwords for c in cases)
        print(f"{name:9s} {len(cases):5d} cases {P / 2**20:6.2f} MiB packed {U / 2**20:6.2f} MiB unpacked, "
              f"largest piece {max(c.nwords for c in cases)} words")
        assert P <= S.LIMIT_PACKED and U <= S.LIMIT_WORDS, name
