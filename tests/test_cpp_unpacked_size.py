"""computeUnpackedSizeInWords of the C++ mirror (tests/cpp/unpacked_size_test.cpp):
the words packed bytes unpack to, without unpacking them.  Compiles everywhere;
runs on a GPU."""
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
LIB = REPO / "capnproto-java_amd" / "lib"


def _build(tmp_path):
    exe = tmp_path / "unpacked_size_test"
    # the oracle is linked in as the source of the packed bytes
    obj = tmp_path / "packed_oracle.o"
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-c", "-o", str(obj),
                    str(REPO / "oracle" / "packed_oracle.c")], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", str(exe),
                    str(REPO / "tests" / "cpp" / "unpacked_size_test.cpp"), str(obj),
                    f"-L{LIB}", "-lcapnp_packed_hip", f"-Wl,-rpath,{LIB}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_unpacked_size_compiles(tmp_path):
    import capnp_packed  # noqa: F401  (library present)
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_unpacked_size(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "all passed" in r.stdout
