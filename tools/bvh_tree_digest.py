#!/usr/bin/env python3
"""Digests of the HOST builder's trees (hikari.jl_amd/csrc/bvh_build.cpp) over a fixed set of scenes; no device needed.

    python tools/bvh_tree_digest.py            # print the digests
    python tools/bvh_tree_digest.py --write    # ... and write tests/golden/bvh_tree_digests.json

The committed file was written at the commit BEFORE the builder's per-node decision moved into hk_bvh_decide.h (shared with the
device builder of hk_scene_rebuild_bvh); tests/test_bvh_rebuild_host.py holds the builder to it, so a refactoring that changes one bit
of one tree fails.  tests/native/bvh_tree_digest.cpp says what is hashed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bvh_scenes import GOLDEN, digest, scenes_to_digest  # noqa: E402  (the scenes and the runner live beside the tests that use them)


def main():
    out = {}
    for name, (P, leaf, bins) in scenes_to_digest().items():
        d = digest(P, leaf, bins)
        d.pop("medians")          # (a count the builder reports since hk_bvh_decide.h; not part of the recorded tree)
        d.update(leaf=leaf, bins=bins)
        out[name] = d
        print(name, json.dumps(d))
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
