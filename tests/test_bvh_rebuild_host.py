"""The BVH rebuild without a device (-m "not gpu"): the two new entry points are declared alike by the header, the ctypes mirror and the
Julia shim; the host builder, whose per-node decision now lives in hk_bvh_decide.h, still builds the trees recorded before the move
(tests/golden/bvh_tree_digests.json, written by tools/bvh_tree_digest.py); and the device builder's algorithm, written sequentially
around the same decision function (tests/native/bvh_decide_check.cpp, plain and under AddressSanitizer + UBSan: a stand-alone program,
nothing sanitised is loaded into Python), gives the recorded host trees."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bvh_scenes as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "bvh_tree_digests.json")))
CTYPES_OF = {"hk_scene*": C.c_void_p, "int32_t*": C.POINTER(C.c_int32)}


@pytest.fixture(scope="module")
def scenes():
    return D.scenes_to_digest()


def test_abi_declares_the_two_entry_points_as_the_header_does(hk):
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    A = hk._abi
    for name, n_args in (("hk_scene_rebuild_bvh", 1), ("hk_scene_bvh_leaves", 3)):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]            # the parameter names dropped
        argtypes, restype = A.PROTOTYPES[name]
        assert len(args) == n_args and restype is C.c_int32 and list(argtypes) == [CTYPES_OF[a] for a in args], (name, args)
        assert name in A.EXPORTED_SYMBOLS
        fn = getattr(hk._lib.lib(), name)                                                  # the built library exports it, the loader installed the prototype
        assert list(fn.argtypes) == list(argtypes) and fn.restype is C.c_int32
    src = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()
    for needle in ("function rebuild_bvh!(", "function bvh_leaves(", "ccall((:hk_scene_rebuild_bvh, LIB), Int32, (Ptr{Cvoid},)",
                   "ccall((:hk_scene_bvh_leaves, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32})"):
        assert needle in src, needle
    assert callable(hk.Scene.rebuild_bvh) and callable(hk.Scene.bvh_leaves)


def test_host_builder_still_builds_the_recorded_trees(scenes):
    """Byte for byte: boxes, child references and leaf order of every recorded scene."""
    assert set(scenes) == set(GOLDEN)
    assert GOLDEN["box_cloud_scale6"]["depth"] > 16 and GOLDEN["cornell_two_spheres"]["depth"] <= 16
    for name, (P, leaf, bins) in scenes.items():
        got = D.digest(P, leaf, bins)
        want = GOLDEN[name]
        assert (leaf, bins) == (want["leaf"], want["bins"])
        for key in ("triangles", "nodes", "depth", "nodes_fnv", "prims_fnv", "topology_fnv"):
            assert got[key] == want[key], (name, key)
    # which of them take the median fallback (the device rebuild is compared tree for tree only where none is taken)
    medians = {name: D.digest(P, leaf, bins)["medians"] for name, (P, leaf, bins) in scenes.items()}
    assert medians["degenerate_200_of_250"] > 0 and medians["skewed_clusters"] > 0
    assert all(medians[n] == 0 for n in ("cornell_two_spheres", "box_cloud", "box_cloud_scale6", "box_cloud_scale6_leaf2_bins16", "skewed_clusters_12"))


def _decide_check(tag, flags):
    exe = os.path.join(tempfile.gettempdir(), "hk_bvh_decide_check_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "bvh_decide_check.cpp"), os.path.join(csrc, "bvh_build.cpp")]
    deps = src + [os.path.join(csrc, "hk_bvh_decide.h"), os.path.join(csrc, "bvh_build.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", csrc, "-I", os.path.join(ROOT, "include")] + flags + src + ["-o", exe])
    return exe


@pytest.mark.parametrize("tag,flags", [("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_shared_decision_function_gives_the_recorded_host_trees(scenes, tag, flags):
    """The level-by-level builder around hk_bvh_decide, bins filled in reverse order, stable partition, breadth-first numbering:
    the recorded topology (child references, and the set of triangles of every leaf) wherever no median split is taken — the skewed
    chain deeper than 16 levels, the deep cloud under two knob settings, the Cornell scene; on the degenerate set (200 coincident
    triangles) the same child references, every triangle in one leaf; where the depth budget bites, a valid tree inside the budget."""
    exe = _decide_check(tag, flags)
    for name in ("degenerate_200_of_250", "skewed_clusters", "skewed_clusters_12", "cornell_two_spheres", "box_cloud_scale6", "box_cloud_scale6_leaf2_bins16"):
        P, leaf, bins = scenes[name]
        with tempfile.NamedTemporaryFile(suffix=".f32") as f:
            f.write(np.ascontiguousarray(P, np.float32).tobytes())
            f.flush()
            r = subprocess.run([exe, f.name, str(leaf), str(bins)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("{"), (name, r.stdout, r.stderr)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        got, want = json.loads(r.stdout), GOLDEN[name]
        assert got["host_topology_fnv"] == want["topology_fnv"]                  # the host builder linked in is the recorded one
        assert got["triangles"] == want["triangles"] and got["depth"] <= 30
        if got["host_medians"] == 0:
            assert got["medians"] == 0 and got["refs_equal"]
            assert (got["nodes"], got["depth"], got["topology_fnv"]) == (want["nodes"], want["depth"], want["topology_fnv"]), name
        else:
            assert got["medians"] > 0
        if name == "degenerate_200_of_250":                                     # coincident centroids: split by count alone on both sides
            assert got["refs_equal"] and (got["nodes"], got["depth"]) == (want["nodes"], want["depth"])
