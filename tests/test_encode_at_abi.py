"""cpk_encode_batch_at at the C-ABI boundary, no GPU needed: the header
declares it with its signature and states the contract, the Python binding
lists it with a matching ctypes signature, and the built library exports it
(inspected as tests/test_packed_size_abi.py inspects it: the library the build
left in the tree)."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
NAME = "cpk_encode_batch_at"
PROTOTYPE = [
    "cpk_ctx ctx", "const void *d_in", "const uint64_t *d_seg_word_off", "uint32_t n",
    "uint64_t max_seg_words",
    "const uint64_t *d_grp_piece_off", "uint32_t ng",
    "void *d_out", "uint64_t out_cap",
    "const uint64_t *d_dst_off", "const uint64_t *d_dst_cap",
    "uint64_t *d_piece_off", "uint64_t *d_grp_len", "int32_t *d_status",
    "void *stream"]


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype():
    """The parameter list of `int cpk_encode_batch_at(...);` in the header, as a list of declarations."""
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{NAME} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_it():
    hdr = _header()
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", hdr, re.M)  # additive: the version stays
    assert _prototype() == PROTOTYPE


def test_header_states_the_contract():
    hdr = _header()
    doc = hdr[hdr.index("Encode to caller-given offsets"):hdr.index("int " + NAME)]
    for word in ("CPK_ENOMEM", "d_dst_cap", "out_cap", "CPK_EINVAL", "d_grp_piece_off == NULL", "never written"):
        assert word in doc, word


def test_python_binding_lists_it():
    import capnp_packed as cp
    assert NAME in cp.EXPORTS
    assert callable(cp.Context.encode_batch_at)


def test_python_signature_matches_the_header():
    import capnp_packed as cp
    L = cp.load()
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in p or p.startswith("cpk_ctx") else ctype[p.split()[0]] for p in _prototype()]
    f = getattr(L, NAME)
    assert list(f.argtypes) == want
    assert f.restype is ctypes.c_int


def test_library_exports_it():
    import capnp_packed as cp
    L = ctypes.CDLL(str(cp.LIB_PATH))
    assert hasattr(L, NAME)
    assert cp.load().cpk_abi_version() == 1
