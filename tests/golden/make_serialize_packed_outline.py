"""Regenerates serialize_packed_outline.json: where each public static method
of capnproto-java's SerializePacked.java stands (names, parameter types and
line numbers only, no source text), for tests/test_integration_patch.py.
Run: python tests/golden/make_serialize_packed_outline.py <capnproto-java checkout>"""
import json
import re
import sys
from pathlib import Path

REL = "runtime/src/main/java/org/capnproto/SerializePacked.java"
java = (Path(sys.argv[1]) / REL).read_text()


def line_of(pos):
    return java.count("\n", 0, pos) + 1


methods = []
for m in re.finditer(r"public static [^;{]*?\b(\w+)\(([^)]*)\)[^{;]*\{", java):
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(java[i], 0)
        i += 1
    body = java[m.end(): i - 1]
    # parameter types without their package (java.nio.channels.X -> X)
    params = [p.split()[0].rsplit(".", 1)[-1] for p in m.group(2).split(",")]
    fwd = re.fullmatch(r"\s*return (\w+)\(input, ReaderOptions\.DEFAULT_READER_OPTIONS\);\s*", body)
    methods.append({"name": m.group(1), "params": params,
                    "decl_line": line_of(m.start()), "open_line": line_of(m.end() - 1),
                    "close_line": line_of(i - 1),
                    # a one-line overload: the same call with the default ReaderOptions
                    "forwards_with_default_options_to": fwd.group(1) if fwd else None})

out = Path(__file__).with_name("serialize_packed_outline.json")
json.dump({"note": "Outline (data only) of the unpatched file named in 'source': 1-based line numbers.",
           "source": REL, "lines": java.count("\n"), "methods": methods}, out.open("w"), indent=1)
print(out, len(methods), "methods")
