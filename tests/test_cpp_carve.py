"""The context scratch carver (csrc/carve.hip) checked on the host
(tests/cpp/carve_test.cpp): the counted size of a layout is the sum of its
takes and the carved arrays do not overlap.  No GPU, no library: the program
includes the carver alone and runs under the address and undefined-behaviour
sanitizers."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_cpp_carve(tmp_path):
    exe = tmp_path / "carve_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    str(REPO / "tests" / "cpp" / "carve_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "all passed" in r.stdout
