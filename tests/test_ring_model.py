"""The output ring's schedule (tools/ring_model.py) against the constants and
the drain of the kernel's source (csrc/encode_sp.hip), and the invariant the
schedule keeps: the lines in flight never exceed the ring.  No GPU needed;
tests/test_gpu_sp_ring.py is the same pressure on the kernel itself."""
import re
from pathlib import Path

import pytest

import ring_model as rm

SRC = (Path(__file__).resolve().parents[1] / "capnproto-java_amd" / "csrc" / "encode_sp.hip").read_text()


def _define(name):
    return int(re.search(r"#define " + name + r" (\d+)", SRC).group(1))


RINGS = {"sparse": _define("CPK_SPARSE_RING"), "dense": _define("CPK_SP_RING_DENSE")}


def test_model_has_the_kernels_constants():
    assert RINGS == {"sparse": 4096, "dense": 11264}
    assert f"kDefer = ((int)(F::kRing - 16) / {rm.STEP_MAX}) & ~1;" in SRC
    assert [rm.defer_steps(r) for r in RINGS.values()] == [6, 16]
    # the drain: every whole group of 64 lines, after a pair and when the offset arrives
    assert f"if (done - ft >= {rm.GROUP}u)" in SRC
    assert f"ft + ((done - ft) & ~{rm.GROUP - 1}u)" in SRC
    assert re.search(r"known = true;\s*drain\(\);", SRC)
    # and the assertion of what it leaves room for
    assert f"static_assert({rm.GROUP} * {rm.LINE} + 2 * {rm.STEP_MAX} <= F::kRing" in SRC


@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("steps", [32, 16, 8])
@pytest.mark.parametrize("kind", ["all_nonzero", "d_x", "l_only", "bound"])
def test_lines_in_flight_fit_the_ring(form, steps, kind):
    ring = RINGS[form]
    most, hit = rm.wave(rm.steps_of(kind, steps), ring)
    assert not hit and most <= ring // rm.LINE, (most, hit[:3])
    # the bound behind the static_assert: a pair behind an incomplete group
    if steps > rm.defer_steps(ring):
        assert most <= max(rm.defer_steps(ring) * rm.STEP_MAX // rm.LINE,
                           rm.GROUP + 2 * rm.STEP_MAX // rm.LINE)


def test_one_group_per_pair_overran_the_sparse_ring():
    """The schedule before the drain, as the ring tests met it on the GPU:
    all-nonzero words pass the 4 KiB ring by 4 bytes at the first pair after
    the deferred steps and stay past it (the partial line after every pair
    meets the oldest unstored line), 8.5 B/word likewise; 8.0 B/word (one
    zero byte per word) fills it exactly and the 11 KiB ring holds all
    three."""
    most, hit = rm.wave(rm.steps_of("all_nonzero"), RINGS["sparse"], schedule="one")
    assert hit[0] == (4096, 4099) and len(hit) == 13 and most == 257
    assert rm.wave(rm.steps_of("d_x"), RINGS["sparse"], schedule="one")[1]
    assert not rm.wave(rm.steps_of("l_only"), RINGS["sparse"], schedule="one")[1]
    for kind in ("all_nonzero", "d_x", "l_only"):
        assert not rm.wave(rm.steps_of(kind), RINGS["dense"], schedule="one")[1]
