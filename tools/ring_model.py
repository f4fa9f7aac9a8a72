"""The single pass's output ring (encode_sp.hip: sp_b, sp_flush_rel) as a
schedule: which relative 16-byte lines hold bytes not yet stored after every
pair of steps, given the bytes each 64-word step emits.

A wave lays a pair of steps out at its relative position `rel`, then (once
its offset is known, after `defer` steps) stores complete lines in groups of
64.  Relative line t lives in ring line t % (ring / 16), so the lines in
flight -- [ft, ceil(rel / 16)) -- must never be more than the ring has: two
that share a ring line are OR-ed together when the older one is stored, and
the younger one's bytes are cleared with it.

`schedule="drain"` is the kernel's: every whole group of 64 complete lines
is stored after a pair, and once when the offset arrives.  `schedule="one"`
is what it was before: one group per pair, none when the offset arrives; kept
to show what the ring tests found (all-nonzero words through the 4 KiB ring).
"""

LINE = 16
GROUP = 64        # lines per full-wave store
STEP_MAX = 640    # bytes of a step's strings at most (64 words x 10)


def defer_steps(ring):
    return ((ring - 16) // STEP_MAX) & ~1


def wave(step_bytes, ring, schedule="drain"):
    """Lays out the steps' bytes; returns (most lines in flight, the relative
    bytes that met an unstored line of the ring's earlier revolution)."""
    lines = ring // LINE
    defer = defer_steps(ring)
    fits = sum(step_bytes) + 16 <= ring
    rel = ft = 0
    most, hit = 0, []
    known = False

    def drain():
        nonlocal ft
        done = rel // LINE
        if done - ft >= GROUP:
            ft += (done - ft) // GROUP * GROUP if schedule == "drain" else GROUP

    for j in range(0, len(step_bytes), 2):
        if j == defer and not fits and len(step_bytes) > defer:
            known = True
            if schedule == "drain":
                drain()
        rel += sum(step_bytes[j:j + 2])
        top = -(-rel // LINE)
        most = max(most, top - ft)
        if top - ft > lines:
            hit.append((LINE * (ft + lines), rel - 1))
        if known:
            drain()
    return most, hit


def steps_of(kind, n=32):
    """Bytes per step of the stretches tests/test_gpu_sp_ring.py uses, and
    of the bound the kernel's layout assumes."""
    if kind == "all_nonzero":      # 2,050 bytes per 256 words
        return [514 if j % 4 == 0 else 512 for j in range(n)]
    if kind == "d_x":              # 10 + 7 bytes per two words
        return [544] * n
    if kind == "l_only":           # tag + 7 bytes per word
        return [512] * n
    if kind == "bound":
        return [STEP_MAX] * n
    raise ValueError(kind)
