"""cpk_encode_message_stream / cpk_encode_message_stream_host at the C-ABI
boundary, no GPU needed: the header declares them, the Python binding lists
them with their signatures, and the built library exports them (inspected as
tests/test_capi.py inspects it: the library the build left in the tree)."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
NAMES = ("cpk_encode_message_stream", "cpk_encode_message_stream_host")


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype(name):
    """The parameter list of `int name(...);` in the header, as a list of declarations."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_both_functions_and_the_info_size():
    hdr = _header()
    assert re.search(r"^#define\s+CPK_EMS_INFO_WORDS\s+6\s*$", hdr, re.M)
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", hdr, re.M)  # additive: the version stays
    dev = _prototype(NAMES[0])
    assert dev == ["cpk_ctx ctx", "const void *d_in", "uint64_t avail_words", "uint64_t traversal_limit_words",
                   "void *d_out", "uint64_t out_cap", "uint64_t *d_out_off", "uint32_t piece_cap",
                   "uint64_t *d_msg_piece", "uint32_t msg_cap", "uint64_t *h_info", "void *stream"]
    host = _prototype(NAMES[1])
    # the same, every pointer in host memory, no stream
    assert [p.split()[:-1] for p in host] == [p.split()[:-1] for p in dev[:-1]]
    # the sizing protocol and the divergence are stated where the caller reads them
    doc = hdr[hdr.index("UNPACKED messages"):hdr.index("#define CPK_EMS_INFO_WORDS")]
    assert "NULL" in doc and "CPK_ENOMEM" in doc and "pad" in doc


def test_python_binding_lists_them():
    import capnp_packed as cp
    for name in NAMES:
        assert name in cp.EXPORTS
    assert cp.EMS_INFO_WORDS == 6
    assert callable(cp.Context.encode_message_stream) and callable(cp.Context.encode_message_stream_host)


def test_python_signatures_match_the_header():
    import capnp_packed as cp
    L = cp.load()
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    for name in NAMES:
        want = [ctypes.c_void_p if "*" in p or p.startswith("cpk_ctx") else ctype[p.split()[0]]
                for p in _prototype(name)]
        f = getattr(L, name)
        assert list(f.argtypes) == want, name
        assert f.restype is ctypes.c_int, name


def test_library_exports_them():
    import capnp_packed as cp
    L = ctypes.CDLL(str(cp.LIB_PATH))
    for name in NAMES:
        assert hasattr(L, name), name
    assert cp.load().cpk_abi_version() == 1
