"""What each input set of tests/_replay_cases.py is for, pinned on the CPU: a
set that no longer meets its condition would leave
tests/test_gpu_graph_replay.py passing for the wrong reason."""
import numpy as np
import pytest

import _replay_cases as R


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _families():
    return [R.encode_family("like"), R.encode_family("units"), R.messages_family("small"),
            R.messages_family("large"), R.decode_family(), R.encode_at_family(), R.decode_at_family(),
            R.messages_at_family(), R.stream_family("one-wave"), R.stream_family("workgroup"),
            R.read_family("small"), R.read_family("large"), R.chain_family()]


def test_sets_of_a_family_have_equal_lengths():
    """Same arrays, same lengths: a captured launch has them baked in.  (The
    host scalars are the family's, one value for all its sets.)"""
    for fam in _families():
        assert len(fam.sets) >= 2, fam.name
        first = fam.sets[0].inputs
        for s in fam.sets[1:]:
            assert {k: v.size for k, v in s.inputs.items()} == {k: v.size for k, v in first.items()}, (fam.name, s.name)
        # ... and consecutive sets differ
        for a, b in zip(fam.sets, fam.sets[1:]):
            assert any(not np.array_equal(a.inputs[k], b.inputs[k]) for k in first), (fam.name, a.name, b.name)


def test_like_sized_sets_and_the_unlike_one():
    for r in R.raw_pieces("like"):
        lo, hi = min(r["sizes"]), max(r["sizes"])
        like = lo >= 4096 and hi <= 2 * lo
        assert like == (r["name"] != "d"), r["name"]
        assert hi <= R.LIKE_MAXW == R.CHUNK  # (one unit each)
    assert np.array_equal(R.raw_pieces("like")[0]["data"], R.raw_pieces("like")[4]["data"])  # (e) is (a) again
    for r in R.raw_pieces("units"):
        lo, hi = min(r["sizes"]), max(r["sizes"])
        assert lo >= 4096 and hi <= 2 * lo and hi > R.CHUNK and hi <= R.UNITS_MAXW
        # the size query's chunk form: a piece of over one chunk and at least 1/2048 of the words
        assert hi * 2048 >= sum(r["sizes"])


def test_zero_share_as_the_gate_samples_it():
    for kind in ("like", "units"):
        for r in R.raw_pieces(kind):
            share = R.sampled_zero_share(r["data"], r["swo"])
            assert (share >= 0.85) == (r["cfg"] == 4), (kind, r["name"], share)


def test_decode_sets_fall_in_their_bands():
    fam = R.decode_family()
    assert fam.scalars["n"] == 6  # at most 32: an uncaptured call would read its extent back
    for s in fam.sets:
        f = s.facts
        ratio = (int(f["off"][-1]) - int(f["off"][0])) / (8 * int(f["swo"][-1]))
        band = "index" if ratio < 0.15 else "dense" if ratio >= 0.80 else "map"
        assert band == R.DECODE_BAND[s.name], (s.name, ratio)
    cut = fam.sets[3].facts
    assert [int(v) for v in cut["st"]] == [R.OK, R.OK, R.ETRUNC, R.OK, R.OK, R.OK]
    assert all(st == R.OK and w == int(n) for s in fam.sets[:3] for (st, w), n in
               zip(s.facts["usz"], np.diff(s.facts["swo"].astype(np.int64))))


@pytest.mark.parametrize("fam,key", [("like", "off"), ("units", "off"), ("msg-small", "off"), ("msg-large", "off"),
                                     ("decode", "off")])
def test_consecutive_sets_differ_in_every_later_offset(fam, key):
    """A look-back prefix (or a scan) left by the previous replay is visible:
    every piece after the first starts somewhere else.  One pair cannot meet
    this for piece 1: the like-sized sets (d) and (e) both begin with the same
    8192 config-2 words (the generator is seeded per configuration and piece
    index), so piece 1 starts at the same byte in both; every later piece and
    the total differ there too."""
    sets = {"like": lambda: R.encode_family("like").sets, "units": lambda: R.encode_family("units").sets,
            "msg-small": lambda: R.messages_family("small").sets, "msg-large": lambda: R.messages_family("large").sets,
            "decode": lambda: R.decode_family().sets}[fam]()
    for a, b in zip(sets, sets[1:]):
        oa, ob = a.facts[key], b.facts[key]
        assert len(oa) == len(ob) and oa[0] == ob[0] == 0
        same_first = fam == "like" and (a.name, b.name) == ("d", "e")
        if same_first:
            assert R.piece_bytes(a.facts, 0) == R.piece_bytes(b.facts, 0)
        assert (oa[2 if same_first else 1:] != ob[2 if same_first else 1:]).all(), (fam, a.name, b.name)


def test_message_families_on_their_side_of_1024_pieces():
    small, large = R.messages_family("small"), R.messages_family("large")
    assert small.scalars["nm"] + small.scalars["nseg"] <= 1024 < large.scalars["nm"] + large.scalars["nseg"]
    for fam in (small, large):
        for s in fam.sets:
            assert len(s.facts["msgs"]) == fam.scalars["nm"]
            assert sum(len(m) for m in s.facts["msgs"]) == fam.scalars["nseg"]
            assert max(len(x) // 8 for m in s.facts["msgs"] for x in m) <= fam.scalars["max_seg_words"]
    assert all(len(m) <= 4 + 3 for s in large.sets for m in s.facts["msgs"])  # (small messages, the padding included)


def test_placed_encode_sets():
    fam = R.encode_at_family()
    orders, statuses = set(), []
    for s in fam.sets:
        x = s.facts
        exp = R.encode_at_expect(fam, s)
        st = exp["st"][0][:4 * x["ng"]].view(np.int32)
        statuses.append([int(v) for v in st])
        orders.add(tuple(np.argsort(x["dst"])))
        slots = sorted((x["dst"][g], x["dst"][g] + x["cap"][g]) for g in range(x["ng"]))
        assert all(a[1] < b[0] for a, b in zip(slots, slots[1:]))       # gaps between the slots
        assert slots[-1][1] <= fam.scalars["out_cap"]
        assert max(int(v) for v in np.diff(x["gpo"].astype(np.int64))) > 1  # a group that looks back
    assert any(d % 2 for s in fam.sets for d in s.facts["dst"])          # odd byte alignment
    assert len(orders) >= 3
    assert statuses[:3] == [[R.OK] * 3] * 3 and statuses[3] == [R.OK, R.ENOMEM, R.OK]


def test_placed_decode_sets():
    fam = R.decode_at_family()
    for s in fam.sets[:3]:
        assert (s.facts["gst"] == R.OK).all() and (s.facts["pst"] == R.OK).all()
    last = fam.sets[3].facts
    assert [int(v) for v in last["gst"]] == [R.OK, R.OK, R.OK, R.ETRAILING, R.OK, R.OK]
    assert int(last["used"][3]) == int(last["ln"][3]) - 2
    assert len({tuple(np.argsort(s.facts["off"])) for s in fam.sets}) >= 3
    assert any(int(o) % 2 for s in fam.sets for o in s.facts["off"])


def test_placed_messages_fit_a_different_prefix_in_each_set():
    fam = R.messages_at_family()
    lens = [s.facts["prefix"] for s in fam.sets]
    assert len(set(lens)) == len(lens) and all(0 < k < fam.scalars["nm"] for k in lens), lens
    tots = [s.facts["model"].totals for s in fam.sets]
    assert len(set(tots)) == len(tots)
    for s, k in zip(fam.sets, lens):
        m = s.facts["model"]
        assert m.totals[2] == k and m.fits == [True] * k + [False] * (fam.scalars["nm"] - k)
        assert [int(v) for v in m.status] == [R.OK] * k + [R.ENOMEM] * (fam.scalars["nm"] - k)


def test_stream_and_read_sets_take_the_intended_forms():
    one, wg = R.stream_family("one-wave"), R.stream_family("workgroup")
    assert one.scalars["avail"] < 6 * 1024 <= wg.scalars["avail"] < 384 * 1024
    small, large = R.read_family("small"), R.read_family("large")
    reach = lambda f: min(f.scalars["avail"], 10 * (f.scalars["out_cap_words"] + R.MSG_HEAD_WORDS) + 16)
    assert reach(small) < 6 * 1024 and 64 * 1024 <= reach(large) < 512 * 1024
    for s in large.sets:
        assert sum(len(x) for x in s.facts["segs"]) >= 64 * 1024  # (the message: its words)
    assert large.sets[0].facts["used"] >= 64 * 1024                 # (... and the first one's packed bytes)


def test_chain_sets_change_the_piece_sizes():
    fam = R.chain_family()
    sizes = [tuple(np.diff(s.facts["swo"].astype(np.int64))) for s in fam.sets]
    assert len(set(sizes)) == len(sizes)
    like = [min(z) >= 4096 and max(z) <= 2 * min(z) for z in sizes]
    assert True in like and False in like  # both encoders from one captured graph
