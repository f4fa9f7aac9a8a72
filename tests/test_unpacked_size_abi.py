"""cpk_unpacked_size_batch / _host at the C-ABI boundary, no GPU needed: the
header declares them with their signatures and states their contract, the
Python binding lists them, and the built library exports them (inspected as
tests/test_packed_size_abi.py inspects its four)."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
PROTOTYPES = {
    "cpk_unpacked_size_batch": [
        "cpk_ctx ctx", "const void *d_packed", "const uint64_t *d_in_off", "uint32_t n",
        "uint64_t *d_seg_word_off", "int32_t *d_status", "void *stream"],
    "cpk_unpacked_size_host": [
        "cpk_ctx ctx", "const void *h_packed", "const uint64_t *h_in_off", "uint32_t n",
        "uint64_t *h_seg_word_off", "int32_t *h_status"],
}


def _header():
    return (REPO / "include" / "capnp_packed.h").read_text()


def _prototype(name):
    """The parameter list of `int name(...);` in the header, as a list of declarations."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in include/capnp_packed.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_two_functions():
    hdr = _header()
    assert re.search(r"^#define\s+CPK_ABI_VERSION\s+1\s*$", hdr, re.M)  # additive: the version stays
    for name, want in PROTOTYPES.items():
        assert _prototype(name) == want, name
    # the contract is stated where the caller reads it
    doc = hdr[hdr.index("Unpacked sizes without decoding"):hdr.index("int cpk_unpacked_size_batch")]
    for word in ("CPK_ETRUNC", "[0] = 0", "cpk_decode_batch", "CPK_ETRAILING", "2^32-1"):
        assert word in doc, word


def test_python_binding_lists_them():
    import capnp_packed as cp
    for name in PROTOTYPES:
        assert name in cp.EXPORTS
    for method in ("unpacked_size_batch", "unpacked_size_host"):
        assert callable(getattr(cp.Context, method)), method


def test_python_signatures_match_the_header():
    import capnp_packed as cp
    L = cp.load()
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    for name in PROTOTYPES:
        want = [ctypes.c_void_p if "*" in p or p.startswith("cpk_ctx") else ctype[p.split()[0]]
                for p in _prototype(name)]
        f = getattr(L, name)
        assert list(f.argtypes) == want, name
        assert f.restype is ctypes.c_int, name


def test_library_exports_them():
    import capnp_packed as cp
    L = ctypes.CDLL(str(cp.LIB_PATH))
    for name in PROTOTYPES:
        assert hasattr(L, name), name
    assert cp.load().cpk_abi_version() == 1
