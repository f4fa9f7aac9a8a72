"""tests/_unpacked_size_model.py against the oracle (no GPU): the GPU tests of
cpk_unpacked_size_batch compare the library with this model, never with
itself, so the model is pinned here to the reference vectors, to the record
builder's word counts and to oracle.unpack."""
import json
from pathlib import Path

import pytest

import _packed_records as R
import _unpacked_size_model as M

GOLD = json.loads((Path(__file__).parent / "golden" / "reference_kats.json").read_text())


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    R.release()


def _consumes_all(oracle, packed, words):
    st, _, used = oracle.unpack(packed, 8 * words)
    return st == 0 and used == len(packed)


def test_kats(oracle):
    for k in GOLD["kats"]:
        packed, unpacked = bytes.fromhex(k["packed"]), bytes.fromhex(k["unpacked"])
        assert M.unpacked_size(packed) == (M.OK, len(unpacked) // 8), k.get("name")
        assert _consumes_all(oracle, packed, len(unpacked) // 8)


@pytest.mark.parametrize("name", R.VALID)
def test_valid_corpora(oracle, name):
    for c in R.corpora()[name]:
        assert M.unpacked_size(c.packed) == (M.OK, c.nwords), c.name
        assert _consumes_all(oracle, c.packed, c.nwords), c.name


def test_geometry_is_a_swept_window():
    """The seam corpora sweep records across the 3584- and 3072-byte window
    edges: the size kernel's window must be one of them (else the GPU test
    needs a sweep of its own)."""
    assert M.kUsWin in (R.kWin, R.kD2Win)


def test_prefixes_of_the_hand_built_pieces(oracle):
    pieces = M.hand_built()
    assert any(b"\xff" in p and len(p) > 2050 for p in pieces)
    for p in pieces:
        ends = {0}
        for q, _, _ in R.parse_records(p)[1:]:
            ends.add(q)
        ends.add(len(p))
        for pre in M.prefixes(p):
            st, w = M.unpacked_size(pre)
            assert (st == M.OK) == (len(pre) in ends), len(pre)
            if st == M.OK:
                assert _consumes_all(oracle, pre, w), len(pre)
                continue
            assert w == 0
            done, wc, (ln, nw) = M.walk(pre)
            tries = [wc, wc + 1] + ([wc + nw] if nw is not None else [])
            for t in tries:
                assert not _consumes_all(oracle, pre, t), (len(pre), t)
