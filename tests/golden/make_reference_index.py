#!/usr/bin/env python3
"""Regenerates tests/golden/reference_index.json from a checkout of the reference's sources:

    python tests/golden/make_reference_index.py <reference>/src

The suite never reads the reference tree itself; this file carries the two facts it checks against it, as data:
  tables       SHA-256 and element count of the numeric tables as tools/extract_reference_tables.py parses them out of the reference
               source (SobolMatrices32 as uint32; CIE_X / CIE_Y / CIE_Z as float32) — tests/test_golden.py compares the shipped
               hikari.jl_amd/data/*.bin with them.
  definitions  every `# ref: Hikari.<name> <file>:<line>` citation of julia/make_reference_fixtures.jl whose cited line was found to
               define <name> (function / struct / const / constructor) — tests/test_reference_fixtures.py requires every citation to be
               in this list.  A citation that does not resolve stops the script."""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(HERE, "reference_index.json")
JULIA = os.path.join(ROOT, "julia", "make_reference_fixtures.jl")


def table_entry(arr):
    return {"count": int(arr.size), "dtype": str(arr.dtype), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}


def tables(src):
    import extract_reference_tables as ex
    out = {}
    sob = ex.grab_block(open(os.path.join(src, "sampler/sobol_matrices.jl")).read(), "SobolMatrices32")
    out["SobolMatrices32"] = table_entry(np.array([int(t, 16) for t in sob], dtype=np.uint32))
    col = open(os.path.join(src, "spectral/color.jl")).read()
    for nm in ("CIE_X", "CIE_Y", "CIE_Z"):
        t = ex.grab_block(col, nm)
        out[nm] = table_entry(np.array([float(re.sub(r"f0$", "", x)) for x in t], dtype=np.float32))
    return out


def definitions(src):
    refs = re.findall(r"# ref: Hikari\.(\w+) (\S+):(\d+)", open(JULIA).read())
    found = []
    for name, rel, line in sorted(set(refs)):
        path = next((p for p in (os.path.join(src, rel), os.path.join(src, "integrators", rel)) if os.path.isfile(p)), None)
        if path is None:
            raise SystemExit("%s: %s not in the reference tree" % (name, rel))
        text = open(path).read().splitlines()[int(line) - 1]
        if not re.search(r"(function|struct)\s+%s\b|^%s\(|const\s+%s\b" % (name, name, name), text):
            raise SystemExit("%s is not defined at %s:%s" % (name, rel, line))
        found.append([name, rel, int(line)])
    return found


def main(argv):
    if len(argv) != 2 or not os.path.isdir(argv[1]):
        raise SystemExit(__doc__)
    src = argv[1]
    with open(OUT, "w") as f:
        json.dump({"tables": tables(src), "definitions": definitions(src)}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv)
