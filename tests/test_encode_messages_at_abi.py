"""cpk_encode_messages_at at the C-ABI boundary, no GPU needed: the header
declares it with its signature and states the contract, the Python binding
lists it with a matching ctypes signature, and the built library exports it
(inspected as tests/test_encode_at_abi.py inspects it: the library the build
left in the tree)."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
NAME = "cpk_encode_messages_at"
PROTOTYPE = [
    "cpk_ctx ctx", "const void *d_in", "const uint64_t *d_seg_word_off", "uint32_t nseg",
    "const uint64_t *d_msg_seg_off", "uint32_t nm", "uint64_t max_seg_words",
    "void *d_out", "uint64_t out_cap",
    "const uint64_t *d_dst_off", "const uint64_t *d_dst_cap",
    "uint64_t *d_piece_off", "uint64_t *d_msg_len", "int32_t *d_status",
    "void *stream"]


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype():
    """The parameter list of `int cpk_encode_messages_at(...);` in the header, as a list of declarations."""
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{NAME} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_it():
    hdr = _header()
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", hdr, re.M)  # additive: the version stays
    assert _prototype() == PROTOTYPE


def test_header_states_the_contract():
    hdr = _header()
    doc = hdr[hdr.index("Encode messages to caller-given slots"):hdr.index("int " + NAME)]
    for word in ("CPK_ENOMEM", "d_dst_cap", "d_msg_len", "never written", "no host synchronisation"):
        assert word in doc, word


def test_header_lists_it_for_graph_capture():
    hdr = _header()
    assert NAME in hdr[hdr.index("Graph capture:"):hdr.index("#ifndef CAPNP_PACKED_H")]


def test_python_binding_lists_it():
    import capnp_packed as cp
    assert NAME in cp.EXPORTS
    assert callable(cp.Context.encode_messages_at)


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
