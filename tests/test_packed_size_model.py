"""The chunk-parallel size form (csrc/encode_size.hip, sz_chunk_kernel) in the
role algebra's Python model (tools/step_model.py), without a GPU: a piece is
sized chunk by chunk, every wave's entry state from state_at, the state handed
from chunk to chunk the way the kernel hands it -- published early from a
fresh entering state when the chunk's masks alone decide it, else computed
from the state the predecessor handed over -- and no bytes are built.  Every
size equals len(oracle.pack(piece)) on the hand-built boundary pieces of
tests/_packed_size_cases.py, which also shows that the oracle itself takes
every one of them."""
import numpy as np

import step_model as sm
from _packed_size_cases import boundary_pieces, PIECE_WORDS

M64 = sm.M64
WS, NW = 32, 4  # kSpWS, kSpWaves: 128 steps = 8192 words per chunk


def _masks(data):
    """Per step (V, Z, DL, D) of a piece, vectorised (sm.step_masks per word
    is the same rule)."""
    w = np.frombuffer(bytes(data), np.uint8).reshape(-1, 8)
    W = len(w)
    nzb = (w != 0).sum(1)
    ns = (W + 63) // 64

    def bits(flags):
        f = np.zeros(ns * 64, np.uint8)
        f[:W] = flags
        return [int.from_bytes(np.packbits(row, bitorder="little").tobytes(), "little") for row in f.reshape(ns, 64)]
    V, Z, DL, D = bits(np.ones(W, bool)), bits(nzb == 0), bits(nzb >= 7), bits(nzb == 8)
    return list(zip(V, Z, DL, D)), int(nzb.sum())


def size_model(data):
    """-> (packed size, chunks whose leaving state was published early,
    chunks that published after taking their entering state)."""
    masks_all, nonzero_bytes = _masks(data)
    CS = WS * NW
    size, early, late = nonzero_bytes, 0, 0
    handed = sm.FRESH  # what the predecessor unit's status word holds
    for c0 in range(0, len(masks_all), CS):
        masks = masks_all[c0:c0 + CS]
        last_chunk = c0 + CS >= len(masks_all)
        cst, handed, was_early = sm.handover(masks, handed, c0 == 0, last_chunk)
        early += was_early
        late += not last_chunk and not was_early
        for wv in range(NW):
            a, b = wv * WS, min((wv + 1) * WS, len(masks))
            if a >= b:
                continue
            st = sm.state_at(masks, a, cst)
            for V, Z, DL, D in masks[a:b]:
                Zh, Mem, Dh, st = sm.roles(Z, DL, D, st)
                HC, ZO = Zh | (D & ~Mem), (Z & ~Zh) | (~V & M64)
                # tags and literal-run members' zero bytes, counts
                size += bin(~ZO & ~Mem & M64).count("1") + bin(Mem & ~D).count("1") + bin(HC).count("1")
    return size, early, late


def test_boundary_pieces_sized_chunk_by_chunk(oracle):
    early = late = 0
    for name, piece in boundary_pieces():
        assert piece.size == 8 * PIECE_WORDS
        got, e, l = size_model(piece)
        assert got == len(oracle.pack(piece)), name
        early += e
        late += l
    # both hand-overs are exercised: a leaving state the masks decide, and one
    # that needs the entering state (all-zero, all-dense, dense-from-5)
    assert early > 0 and late >= 6


def test_random_pieces_sized_chunk_by_chunk(oracle):
    rng = np.random.default_rng(11)
    for _ in range(4):
        d = sm.rand_piece(rng, int(rng.integers(8193, 30000)))
        assert size_model(d)[0] == len(oracle.pack(d))
