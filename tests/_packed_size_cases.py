"""Hand-built pieces for the size query's chunk boundaries, shared by
tests/test_packed_size_model.py (CPU) and tests/test_gpu_packed_size.py.

Each piece is 3 x 8192 + 1 words of a background word that is nonzero with
six zero bytes (it resets every run state), with one planted run starting at
word 8192 + d: the smallest inputs that put a run's start, its 255 / 256
caps and its end on either side of a chunk boundary, so that a chunk's
leaving state is both published early and waited for."""
import numpy as np

CHUNK = 8192
PIECE_WORDS = 3 * CHUNK + 1
BG = np.array([0, 0, 9, 0, 1, 0, 0, 0], np.uint8)        # M: >= 2 zero bytes, nonzero
DENSE = np.full(8, 7, np.uint8)                          # D: all 8 bytes nonzero
ONE_ZERO = np.array([1, 2, 3, 0, 5, 6, 7, 8], np.uint8)  # L: exactly one zero byte
OFFSETS = (-257, -256, -255, -1, 0, 1)
LENGTHS = (255, 256, 257, 600)
KINDS = ("zero", "dense", "dense+L")


def _run(kind, length):
    r = np.zeros((length, 8), np.uint8)
    if kind != "zero":
        r[:] = DENSE
        if kind == "dense+L":
            r[2::3] = ONE_ZERO  # literal-run members that are not heads
    return r


def boundary_pieces():
    """-> [(name, uint8 array of PIECE_WORDS * 8 bytes)]"""
    out = []
    for kind in KINDS:
        for length in LENGTHS:
            for d in OFFSETS:
                w = np.tile(BG, (PIECE_WORDS, 1))
                w[CHUNK + d:CHUNK + d + length] = _run(kind, length)
                out.append((f"{kind}-{length}@{d:+d}", w.reshape(-1)))
    out.append(("all-zero", np.zeros(PIECE_WORDS * 8, np.uint8)))
    # heads every 256 words across both boundaries: every chunk's leaving
    # state depends on the one entering it
    out.append(("all-dense", np.tile(DENSE, PIECE_WORDS)))
    w = np.tile(DENSE, (PIECE_WORDS, 1))
    w[:5] = BG  # the heads' phase is not aligned to the chunks
    out.append(("dense-from-5", w.reshape(-1)))
    return out
