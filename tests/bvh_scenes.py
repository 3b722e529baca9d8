"""Scenes and the digest runner of the BVH builder tests (tests/test_bvh_rebuild_host.py, tests/test_bvh_rebuild.py) and of
tools/bvh_tree_digest.py: triangle soups that steer the binned-SAH builder — a degenerate set, clusters at shrinking spacing, the box
cloud of test_vertex_edits.py — and `digest`, which runs the HOST builder over a soup in a stand-alone program
(tests/native/bvh_tree_digest.cpp, built once with g++; no device)."""
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bvh_tree_digests.json")
f32 = np.float32


def degenerate_positions(n_same=200, n_other=50, seed=5):
    """n_same copies of one triangle among n_other distinct ones (the copies in the middle of the array)."""
    rng = np.random.default_rng(seed)
    other = (rng.random((n_other, 1, 3)) * 4.0 + 0.2 * rng.random((n_other, 3, 3))).astype(f32)
    same = np.broadcast_to(np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [1.0, 1.5, 1.25]], f32), (n_same, 3, 3))
    return np.ascontiguousarray(np.concatenate([other[:n_other // 2], same, other[n_other // 2:]]), f32)


def skewed_positions(n_clusters=48, per_cluster=64, ratio=0.5, seed=9):
    """Clusters of small triangles along x at geometrically shrinking spacing (cluster k at 8 ratio^k, its triangles a tenth of that
    wide): a bin boundary only ever separates the few outermost clusters from the rest, so the SAH tree is a long chain."""
    rng = np.random.default_rng(seed)
    k = np.repeat(np.arange(n_clusters), per_cluster)
    x = 8.0 * ratio ** k
    c = np.stack([x * (1.0 + 0.1 * rng.random(len(k))), 0.5 + x * 0.1 * rng.random(len(k)), 0.5 + x * 0.1 * rng.random(len(k))], axis=1)
    tri = c[:, None, :] + (0.02 * x)[:, None, None] * rng.random((len(k), 3, 3))
    return np.ascontiguousarray(tri, f32)


def spread_positions(n_clusters=48, per_cluster=64, seed=9):
    """The same number of triangles laid out evenly (what the skewed scene is created as: a shallow tree)."""
    rng = np.random.default_rng(seed)
    n = n_clusters * per_cluster
    c = rng.random((n, 1, 3)) * 4.0
    return np.ascontiguousarray(c + 0.05 * rng.random((n, 3, 3)), f32)


def box_cloud_positions(scale=None):
    """The box cloud of tests/test_vertex_edits.py as pushed, or with its middle mesh under the deformation of that scale."""
    from types import SimpleNamespace
    import test_scene_edits as E
    import test_vertex_edits as T
    P = np.ascontiguousarray(E._boxes(T.N_BOXES, 3)[0], f32)
    if scale is not None:
        P = P.copy()
        P[T.SPLIT_A:T.SPLIT_B] = T._deep_deformed(SimpleNamespace(positions=P[T.SPLIT_A:T.SPLIT_B]), scale).positions
    return P


def cornell_positions():
    from hikari_jl_amd import scenes
    s, _, _ = scenes.cornell_box(64, 64, objects="two_spheres")
    d = s.desc
    return np.ctypeslib.as_array(d.positions, (d.n_triangles, 3, 3)).copy()


def scenes_to_digest():
    """name -> (positions [T, 3, 3] float32, leaf size, bins)"""
    cloud6 = box_cloud_positions(6.0)
    return {
        "cornell_two_spheres": (cornell_positions(), 4, 32),
        "box_cloud": (box_cloud_positions(), 4, 32),
        "box_cloud_scale6": (cloud6, 4, 32),
        "box_cloud_scale6_leaf2_bins16": (cloud6, 2, 16),
        "degenerate_200_of_250": (degenerate_positions(), 4, 32),
        "skewed_clusters": (skewed_positions(), 4, 32),                       # the depth budget bites: median splits
        "skewed_clusters_12": (skewed_positions(12, 256, 0.25), 4, 32),      # deeper than 16 levels without one
    }


def native(extra_flags=(), tag="plain"):
    """The digest program, built once per change of its sources."""
    exe = os.path.join(tempfile.gettempdir(), "hk_bvh_tree_digest_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "bvh_tree_digest.cpp"), os.path.join(csrc, "bvh_build.cpp")]
    deps = src + [os.path.join(csrc, h) for h in ("bvh_build.h", "hk_bvh_decide.h") if os.path.exists(os.path.join(csrc, h))]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", csrc, "-I", os.path.join(ROOT, "include")] + list(extra_flags) + src + ["-o", exe])
    return exe


def digest(positions, leaf=4, bins=32, exe=None):
    """The host builder's tree of `positions`: dict(triangles, nodes, depth, nodes_fnv, prims_fnv, topology_fnv, medians)."""
    positions = np.ascontiguousarray(positions, f32)
    with tempfile.NamedTemporaryFile(suffix=".f32") as f:
        f.write(positions.tobytes())
        f.flush()
        out = subprocess.run([exe or native(), f.name, str(leaf), str(bins)], capture_output=True, text=True, check=True).stdout
    return json.loads(out)
