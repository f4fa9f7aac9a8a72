"""cpk_decode_messages_at at the C-ABI boundary, no GPU needed: the header
declares it and CPK_MAT_TOTALS and states the contract, the Python binding
lists it with a matching ctypes signature, the built library exports it
(inspected as tests/test_decode_at_abi.py inspects it: the library the build
left in the tree), and the one call that needs no context -- a NULL one -- is
refused.  The other argument checks need a context and are in
tests/test_gpu_decode_messages_at.py."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
NAME = "cpk_decode_messages_at"
PROTOTYPE = [
    "cpk_ctx ctx", "const void *d_packed", "uint64_t in_cap",
    "const uint64_t *d_src_off", "const uint64_t *d_src_len", "uint32_t nm",
    "uint64_t traversal_limit_words",
    "void *d_out", "uint64_t out_cap_words",
    "uint64_t *d_seg_word_off", "uint64_t *d_seg_in_off", "int32_t *d_seg_status",
    "uint32_t seg_cap",
    "uint64_t *d_msg_seg_off", "int32_t *d_msg_status", "uint64_t *d_msg_used",
    "uint64_t *d_totals", "void *stream"]


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype():
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{NAME} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_it():
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", _header(), re.M)  # additive: the version stays
    assert re.search(r"^#define\s+CPK_MAT_TOTALS\s+3\s*$", _header(), re.M)
    assert _prototype() == PROTOTYPE


def test_header_states_the_contract():
    hdr = _header()
    doc = " ".join(hdr[hdr.index("Decode messages from caller-given ranges"):hdr.index("int " + NAME)]
                   .replace("*", " ").split())
    for word in ("CPK_EUNSUPPORTED", "CPK_EINVAL", "CPK_EFRAME", "CPK_ETRUNC", "CPK_EOVERRUN", "CPK_ENOMEM",
                 "CPK_ETRAILING", "in_cap", "only read", "d_totals[CPK_MAT_TOTALS]", "prefix", "d_msg_used",
                 "d_msg_seg_off", "may be NULL", "no host synchronisation", "one wave", "no host form",
                 "cpk_encode_batch_at", "nm == 0"):
        assert word in doc, word


def test_python_binding_lists_it():
    import capnp_packed as cp
    assert NAME in cp.EXPORTS and cp.MAT_TOTALS == 3
    assert callable(cp.Context.decode_messages_at)


def test_python_signature_matches_the_header():
    import capnp_packed as cp
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in p or p.startswith("cpk_ctx") else ctype[p.split()[0]] for p in _prototype()]
    f = getattr(cp.load(), NAME)
    assert list(f.argtypes) == want
    assert f.restype is ctypes.c_int


def test_library_exports_it():
    import capnp_packed as cp
    assert hasattr(ctypes.CDLL(str(cp.LIB_PATH)), NAME)
    assert cp.load().cpk_abi_version() == 1


def test_null_context_is_refused():
    """nm == 0 with every array NULL is a valid call but for the context."""
    import capnp_packed as cp
    tot = (ctypes.c_uint64 * 3)(7, 7, 7)
    mseg = (ctypes.c_uint64 * 1)(7)
    rc = cp.load().cpk_decode_messages_at(None, None, 0, None, None, 0, 1 << 23, None, 0, None, None, None, 0,
                                          ctypes.addressof(mseg), None, None, ctypes.addressof(tot), None)
    assert rc == cp.EINVAL
    assert list(tot) == [7, 7, 7] and mseg[0] == 7  # (nothing is written)
