"""cpk_decode_batch_at and cpk_unpacked_size_batch_at at the C-ABI boundary, no
GPU needed: the header declares them with their signatures and states the
contract, the Python binding lists them with matching ctypes signatures, and
the built library exports them (inspected as tests/test_encode_at_abi.py
inspects it: the library the build left in the tree)."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
PROTOTYPES = {
    "cpk_decode_batch_at": [
        "cpk_ctx ctx", "const void *d_packed", "uint64_t in_cap",
        "const uint64_t *d_src_off", "const uint64_t *d_src_len",
        "const uint64_t *d_grp_piece_off", "uint32_t ng",
        "const uint64_t *d_seg_word_off", "uint32_t n",
        "void *d_out",
        "int32_t *d_status", "int32_t *d_grp_status", "uint64_t *d_grp_used",
        "void *stream"],
    "cpk_unpacked_size_batch_at": [
        "cpk_ctx ctx", "const void *d_packed", "uint64_t in_cap",
        "const uint64_t *d_src_off", "const uint64_t *d_src_len", "uint32_t n",
        "uint64_t *d_seg_word_off", "int32_t *d_status", "void *stream"],
}
NAMES = sorted(PROTOTYPES)


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype(name):
    """The parameter list of `int name(...);` in the header, as a list of declarations."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_it(name):
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", _header(), re.M)  # additive: the version stays
    assert _prototype(name) == PROTOTYPES[name]


def test_header_states_the_contract():
    hdr = _header()
    doc = hdr[hdr.index("Decode from caller-given ranges"):hdr.index("int cpk_decode_batch_at")]
    for word in ("CPK_ETRAILING", "CPK_EINVAL", "CPK_EUNSUPPORTED", "in_cap", "d_grp_piece_off == NULL", "only",
                 "read", "d_grp_used", "cpk_decode_stream", "cpk_encode_batch_at"):
        assert word in doc, word
    assert "only read" in " ".join(doc.replace("*", " ").split())
    size = hdr[hdr.index("int cpk_decode_batch_at"):hdr.index("int cpk_unpacked_size_batch_at")]
    for word in ("CPK_ETRUNC", "CPK_EINVAL", "CPK_EUNSUPPORTED", "in_cap", "only read"):
        assert word in " ".join(size.replace("*", " ").split()), word


@pytest.mark.parametrize("name", NAMES)
def test_python_binding_lists_it(name):
    import capnp_packed as cp
    assert name in cp.EXPORTS
    assert callable(getattr(cp.Context, name[len("cpk_"):]))


@pytest.mark.parametrize("name", NAMES)
def test_python_signature_matches_the_header(name):
    import capnp_packed as cp
    L = cp.load()
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in p or p.startswith("cpk_ctx") else ctype[p.split()[0]] for p in _prototype(name)]
    f = getattr(L, name)
    assert list(f.argtypes) == want
    assert f.restype is ctypes.c_int


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it(name):
    import capnp_packed as cp
    L = ctypes.CDLL(str(cp.LIB_PATH))
    assert hasattr(L, name)
    assert cp.load().cpk_abi_version() == 1
