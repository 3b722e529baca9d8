"""hk_scene_rebuild_bvh on the device: a scene whose mesh was deformed in place and whose BVH was then REBUILT on the device holds the tree
a scene BUILT FRESH from the deformed mesh holds — node count, depth, every child reference, the set of triangles of every leaf, every
box — because both builders take the per-node decision of hk_bvh_decide.h from order-free bins.  Every comparison is np.array_equal;
the helpers are those of test_scene_edits.py / test_vertex_edits.py, the scenes without a median split are confirmed as such with the
host builder (bvh_scenes.digest)."""
import ctypes as C

import numpy as np
import pytest

import bvh_scenes as D
import test_scene_edits as E
import test_vertex_edits as T
import vertex_ref as V

pytestmark = pytest.mark.gpu
f32 = np.float32


def _info(hk, ctx, s):
    n, t, d = C.c_int32(), C.c_int32(), C.c_int32()
    hk._lib.check(hk._lib.lib().hk_scene_bvh_info(hk.scene_handle(ctx, s), C.byref(n), C.byref(t), C.byref(d)), "hk_scene_bvh_info")
    return n.value, t.value, d.value


def _tree(hk, ctx, s):
    boxes, refs = T._bvh_copy(hk, hk.scene_handle(ctx, s))
    return dict(info=_info(hk, ctx, s), boxes=boxes, refs=refs, leaves=s.bvh_leaves(ctx))


def _leaf_sets(tree):
    """the sorted triangle indices of every leaf, in node order (left child first)"""
    out = []
    for ref in tree["refs"].reshape(-1):
        if ref < 0:
            first, count = (~int(ref)) >> 3, ((~int(ref)) & 7) + 1
            out.append(tuple(sorted(tree["leaves"][first:first + count].tolist())))
    return out


def _assert_same_tree(a, b):
    assert a["info"] == b["info"]                                              # node count, leaf slots, depth
    ra, rb = a["refs"], b["refs"]
    assert ra.shape == rb.shape and np.array_equal(ra >= 0, rb >= 0)
    assert np.array_equal(ra[ra >= 0], rb[rb >= 0])                            # inner references
    assert np.array_equal((~ra[ra < 0]) & 7, (~rb[rb < 0]) & 7)                # leaf references: the count bits
    assert _leaf_sets(a) == _leaf_sets(b)                                      # ... and the same triangles in every leaf
    assert np.array_equal(a["boxes"], b["boxes"])                              # as float values: +0 == -0
    assert sorted(a["leaves"].tolist()) == list(range(len(a["leaves"])))


def _no_median(s, leaf=4, bins=32):
    d = s.desc
    P = np.ctypeslib.as_array(d.positions, (d.n_triangles, 3, 3))
    return D.digest(P, leaf, bins)["medians"] == 0


def _deep_rays(new):
    """the ray set of test_hits_deep_tree_quantised_nodes_packed_records: the last 10 000 aimed at the triangles carried outside"""
    rng = np.random.default_rng(13)
    o, d, tmax = E._rays(rng, 100_000, (-7, -7, -7), (7, 7, 7))
    aim = new.positions[rng.integers(0, 600, 10_000)].mean(axis=1).astype(f32)
    o[90_000:] = aim + f32(0.5) * d[90_000:]
    d[90_000:] = -d[90_000:]
    return o, d, tmax


def test_small_tree_rebuilt_is_the_fresh_tree(hk, gpu_ctx):
    sphere = E._sphere(tess=24)
    new = T._rippled(sphere, 0.1)
    se, insts, sf = T._pair(hk, [(sphere, T._white(hk), None, new)])
    assert _no_median(sf)
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    fresh = _tree(hk, gpu_ctx, sf)
    assert not np.array_equal(_tree(hk, gpu_ctx, se)["boxes"], fresh["boxes"])
    (before, after), = se.rebuild_bvh(gpu_ctx)
    _assert_same_tree(_tree(hk, gpu_ctx, se), fresh)
    now, created = se.bvh_cost(gpu_ctx)
    fresh_created = sf.bvh_cost(gpu_ctx)[1]
    assert now == created == after and created == pytest.approx(fresh_created, rel=1e-9) and before > 0
    o, d, tmax = T._cornell_rays(11)
    a, b = E._trace(hk, gpu_ctx, se, o, d, tmax), E._trace(hk, gpu_ctx, sf, o, d, tmax)
    assert (a[0][1] >= insts[0].first_tri).sum() > 1000
    E._assert_same_hits(a, b)
    assert np.array_equal(E._film(hk, se), E._film(hk, sf))
    assert np.array_equal(E._film(hk, se, one_sample=True), E._film(hk, sf, one_sample=True))   # the fused small pass


@pytest.fixture(scope="module")
def deep(hk, gpu_ctx):
    """The box cloud under its scale-6 deformation, deformed in place (se) and built fresh (sf), and the fresh tree."""
    se, insts, sf, meshes, new = T._deep_pair(hk, scale=6.0)
    assert _no_median(sf)                                                      # (another seed or scale if it ever does)
    T._assert_deep(hk, gpu_ctx, se)
    se.set_vertices(insts[1], new.positions, normals=new.normals)
    return dict(se=se, insts=insts, sf=sf, new=new, fresh=_tree(hk, gpu_ctx, sf))


def test_deep_tree_rebuilt_is_the_fresh_tree(hk, gpu_ctx, deep):
    se, sf, new, insts = deep["se"], deep["sf"], deep["new"], deep["insts"]
    a, e = insts[1].first_tri, insts[1].first_tri + insts[1].n_tris
    assert a % 1024 != 0 and e % 1024 != 0 and e < se.desc.n_triangles           # a range off the block size at both ends
    drifted, created = se.bvh_cost(gpu_ctx)
    assert drifted > created
    se.rebuild_bvh(gpu_ctx)
    _assert_same_tree(_tree(hk, gpu_ctx, se), deep["fresh"])
    assert _info(hk, gpu_ctx, se)[2] > 16
    now, created2 = se.bvh_cost(gpu_ctx)
    assert now < drifted and now == created2 == pytest.approx(sf.bvh_cost(gpu_ctx)[1], rel=1e-9)
    o, d, tmax = _deep_rays(new)
    got, want = E._trace(hk, gpu_ctx, se, o, d, tmax), E._trace(hk, gpu_ctx, sf, o, d, tmax)
    hit = got[0][1]
    assert ((hit >= a) & (hit < a + 600)).sum() > 1000 and ((hit >= a + 600) & (hit < e)).sum() > 1000
    E._assert_same_hits(got, want)


def test_refit_agrees_with_the_build(hk, gpu_ctx, deep):
    se, insts, new = deep["se"], deep["insts"], deep["new"]
    se.rebuild_bvh(gpu_ctx)
    built = _tree(hk, gpu_ctx, se)
    se.set_vertices(insts[1], new.positions, normals=new.normals)              # the very same arrays: the refit recomputes every box
    again = _tree(hk, gpu_ctx, se)
    assert np.array_equal(again["boxes"], built["boxes"]) and np.array_equal(again["refs"], built["refs"]) and np.array_equal(again["leaves"], built["leaves"])


def test_both_binning_paths_and_two_builds_in_a_row(hk, gpu_ctx, deep, knobs):
    se = deep["se"]
    trees = []
    for small in ("0", "1000000000", None, None):                               # every node through memory, every node in LDS, the default twice
        if small is None:
            knobs.delenv("HK_BVH_BUILD_SMALL")
        else:
            knobs.setenv("HK_BVH_BUILD_SMALL", small)
        se.rebuild_bvh(gpu_ctx)
        trees.append(_tree(hk, gpu_ctx, se))
    for t in trees[1:]:
        assert t["info"] == trees[0]["info"] and np.array_equal(t["refs"], trees[0]["refs"]) and np.array_equal(t["leaves"], trees[0]["leaves"])
        assert np.array_equal(t["boxes"].view(np.uint32), trees[0]["boxes"].view(np.uint32))   # reproducible bits
    _assert_same_tree(trees[0], deep["fresh"])


def test_edits_go_on_working_on_the_new_topology(hk, gpu_ctx):
    sa, sb = E._sphere(tess=16), E._sphere((0.4, 0.35, 0.3), 0.3, 12)
    first, second = T._rippled(sa, 0.1), T._rippled(sa, 0.06, phase=1.0)
    se, insts, _ = T._pair(hk, [(sa, T._white(hk), None, None), (sb, T._white(hk), None, None)])            # as pushed, no transform yet
    _, _, sf = T._pair(hk, [(sa, T._white(hk), None, second), (sb, T._white(hk), T.M_B, None)])
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], first.positions, normals=first.normals)
    se.rebuild_bvh(gpu_ctx)
    se.set_vertices(insts[0], second.positions, normals=second.normals)        # through the slot table of the new leaf order
    se.set_transform(insts[1], T.M_B)
    o, d, tmax = T._cornell_rays(29, 60_000)
    got = E._trace(hk, gpu_ctx, se, o, d, tmax)
    for inst in insts:
        assert ((got[0][1] >= inst.first_tri) & (got[0][1] < inst.first_tri + inst.n_tris)).sum() > 300
    E._assert_same_hits(got, E._trace(hk, gpu_ctx, sf, o, d, tmax))
    assert np.array_equal(E._film(hk, se, spp=4), E._film(hk, sf, spp=4))
    se.rebuild_bvh(gpu_ctx)                                                     # and once more, over the moved instance
    assert _no_median(sf)
    _assert_same_tree(_tree(hk, gpu_ctx, se), _tree(hk, gpu_ctx, sf))


def _cluster_scene(hk, P):
    from hikari_jl_amd.geometry import Mesh
    s = hk.Scene()
    inst = s.push_instance(Mesh(P, V.face_normals(P), None), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6)))
    s.push(hk.PointLight((2.0, 2.0, -2.0), hk.RGBSpectrum(40.0)))
    s.sync()
    return s, inst


def _cluster_rays(P, seed):
    rng = np.random.default_rng(seed)
    o, d, tmax = E._rays(rng, 40_000, (-0.5, -0.5, -1.0), (9.0, 1.5, 1.5))
    aim = P[rng.integers(0, len(P), 20_000)].mean(axis=1).astype(f32)           # half of them look back at a triangle from nearby
    o[20_000:] = aim + f32(0.05) * np.abs(aim[:, :1]) * d[20_000:]
    d[20_000:] = -d[20_000:]
    return o, d, tmax


def _cluster_frame(hk, vp, s, film, one_sample):
    """4 samples of `s` on `vp` from a camera that has the clusters (and the even layout) in view"""
    cam = hk.PerspectiveCamera((5.0, 0.9, -6.5), (5.0, 0.9, 0.9), film, fov=60.0)
    vp._ensure(film)
    vp.clear()
    if one_sample:
        for i in range(1, 5):
            vp.render_samples(s, film, cam, 1, first=i, readback=False)
    else:
        vp.render_samples(s, film, cam, 4, first=1, readback=False)
    return vp.read_accumulators(film).copy()


def test_depth_class_changes_in_both_directions(hk, gpu_ctx):
    """Created 12 levels deep, deformed into clusters at geometrically shrinking spacing (a chain 22 levels deep on the host builder,
    without a median split), rebuilt; then back.  ONE integrator renders the edited scene throughout, so its path state and view key
    live across both changes of the depth class; every fresh scene gets an integrator of its own."""
    flat, chain = D.spread_positions(12, 256), D.skewed_positions(12, 256, 0.25)
    d_flat, d_chain = D.digest(flat), D.digest(chain)
    assert d_flat["depth"] <= 16 < d_chain["depth"] and d_flat["medians"] == 0 and d_chain["medians"] == 0
    se, inst = _cluster_scene(hk, flat)
    s_chain, _ = _cluster_scene(hk, chain)
    s_flat, _ = _cluster_scene(hk, flat)
    hk.scene_handle(gpu_ctx, se)
    assert _info(hk, gpu_ctx, se)[2] == d_flat["depth"]
    film = hk.Film((96, 64))
    kept = hk.VolPath(max_depth=5, samples=4)
    try:
        created = _cluster_frame(hk, kept, se, film, False)                     # the kept integrator has a state laid out for the shallow class
        for P, fresh, want in ((chain, s_chain, d_chain), (flat, s_flat, d_flat)):
            se.set_vertices(inst, P, normals=V.face_normals(P))
            assert _info(hk, gpu_ctx, se)[2] != want["depth"]                   # the refit keeps the topology it has
            se.rebuild_bvh(gpu_ctx)
            assert _info(hk, gpu_ctx, se)[2] == want["depth"] == _info(hk, gpu_ctx, fresh)[2]
            _assert_same_tree(_tree(hk, gpu_ctx, se), _tree(hk, gpu_ctx, fresh))
            o, d, tmax = _cluster_rays(P, 31)
            got = E._trace(hk, gpu_ctx, se, o, d, tmax)
            assert (got[0][1] >= 0).sum() > 5000
            E._assert_same_hits(got, E._trace(hk, gpu_ctx, fresh, o, d, tmax))
            for one_sample in (False, True, False):                             # (the last: the same view again, on the kept state)
                own = hk.VolPath(max_depth=5, samples=4)
                try:
                    ref = _cluster_frame(hk, own, fresh, film, one_sample)
                finally:
                    own.close()
                got_film = _cluster_frame(hk, kept, se, film, one_sample)
                lit = (ref.reshape(4, -1)[:3] > 0).any(axis=0).sum()          # planes r, g, b, weight
                assert np.isfinite(ref).all() and ref.max() > 0 and lit > 20      # the geometry is in the frame, lit
                assert np.array_equal(got_film, ref)
        assert np.array_equal(got_film, created)                                # back where it began
    finally:
        kept.close()


def test_median_fallback_builds_a_valid_tree(hk, gpu_ctx):
    P = D.degenerate_positions()
    assert D.digest(P)["medians"] > 0
    se, _ = _cluster_scene(hk, P)
    sf, _ = _cluster_scene(hk, P)
    hk.scene_handle(gpu_ctx, se)
    se.rebuild_bvh(gpu_ctx)
    t = _tree(hk, gpu_ctx, se)
    n_nodes, n_slots, depth = t["info"]
    assert n_slots == len(P) and depth <= 30
    assert sorted(t["leaves"].tolist()) == list(range(len(P)))                   # every triangle in exactly one leaf
    refs, boxes = t["refs"], t["boxes"].reshape(-1, 2, 2, 3)
    lo, hi = np.empty((n_nodes, 3), f32), np.empty((n_nodes, 3), f32)
    used = np.zeros(len(P), int)
    for i in range(n_nodes - 1, -1, -1):                                         # children come after their parent: bottom-up
        for c in range(2):
            ref = int(refs[i, c])
            if ref >= 0:
                assert ref > i
                want = (lo[ref], hi[ref])
            else:
                first, count = (~ref) >> 3, ((~ref) & 7) + 1
                assert count <= 4
                used[first:first + count] += 1
                tri = P[t["leaves"][first:first + count]].reshape(-1, 3)
                want = (tri.min(axis=0), tri.max(axis=0))
            assert np.array_equal(boxes[i, c, 0], want[0]) and np.array_equal(boxes[i, c, 1], want[1])
        lo[i], hi[i] = boxes[i, :, 0].min(axis=0), boxes[i, :, 1].max(axis=0)
    assert (used == 1).all()
    rng = np.random.default_rng(37)
    o, d, tmax = E._rays(rng, 40_000, (-0.5, -0.5, -0.5), (4.7, 4.7, 4.7))
    aim = P[rng.integers(0, len(P), 20_000)].mean(axis=1).astype(f32)           # half of them look back at a triangle (250 small ones fill little of the box)
    o[20_000:] = aim + f32(0.3) * d[20_000:]
    d[20_000:] = -d[20_000:]
    got = E._trace(hk, gpu_ctx, se, o, d, tmax)
    assert (got[0][1] >= 0).sum() > 1000
    E._assert_same_hits(got, E._trace(hk, gpu_ctx, sf, o, d, tmax))


def test_contract_null_root_leaf_untouched_scene(hk, gpu_ctx):
    from hikari_jl_amd.geometry import Mesh
    L, A = hk._lib.lib(), hk._abi
    assert L.hk_scene_rebuild_bvh(None) == A.HK_ERR_INVALID and L.hk_last_error()
    n = C.c_int32()
    assert L.hk_scene_bvh_leaves(None, C.byref(n), None) == A.HK_ERR_INVALID
    one = hk.Scene()
    one.push(Mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], f32), None, None), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))
    one.push(hk.PointLight((0, 1, 3), hk.RGBSpectrum(1.0)))
    one.sync()
    before = _info(hk, gpu_ctx, one)
    assert before[0] == 0 and one.bvh_leaves(gpu_ctx).tolist() == [0]
    assert L.hk_scene_rebuild_bvh(hk.scene_handle(gpu_ctx, one)) == A.HK_OK
    assert _info(hk, gpu_ctx, one) == before and one.bvh_cost(gpu_ctx) == (0.0, 0.0)
    # an untouched scene gets the tree it was created with
    sphere = E._sphere(tess=12)
    s, _, _ = T._pair(hk, [(sphere, T._white(hk), None, None)])
    assert _no_median(s)
    created = _tree(hk, gpu_ctx, s)
    cost = s.bvh_cost(gpu_ctx)
    assert s.rebuild_bvh() == [(cost[0], pytest.approx(cost[1], rel=1e-9))]       # (ctx=None: every device scene of the Scene)
    _assert_same_tree(_tree(hk, gpu_ctx, s), created)
    now, base = s.bvh_cost(gpu_ctx)
    assert now == base


def test_rebuild_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the mesh and the tree as they were when the call was made; the next one sees the new vertices
    on the rebuilt tree.  (A rebuild changes no hit, so by itself it cannot show in a film whether the noted call ran before or
    after it: what this sequence holds is that the noted call is rendered before the buffers of its tree are let go, and that the
    deformation and the rebuild together land between the two calls.)"""
    sphere = E._sphere()
    new = T._rippled(sphere, 0.1)
    se, insts, sf = T._pair(hk, [(sphere, T._white(hk), None, new)])
    s_old, _, _ = T._pair(hk, [(sphere, T._white(hk), None, None)])
    hk.scene_handle(gpu_ctx, se)

    def run(first, then, edit):
        film = hk.Film((E.W, E.H))
        cam = E._camera(hk, film)
        vp = hk.VolPath(**E.KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)        # noted, not yet rendered
        if edit:
            se.set_vertices(insts[0], new.positions, normals=new.normals)
            se.rebuild_bvh(gpu_ctx, costs=False)
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(se, se, True)
    assert np.array_equal(got, run(s_old, sf, False))
    assert not np.array_equal(got, run(sf, sf, False))                          # (the first call did render the mesh as it was)


def test_view_cache_survives_a_rebuild(hk, gpu_ctx, knobs):
    knobs.setenv("HK_BATCH_PATHS_M", "0")
    knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    knobs.delenv("HK_VIEW_CACHE")
    sphere = E._sphere(tess=16)
    new = T._rippled(sphere, 0.1)
    se, insts, sf = T._pair(hk, [(sphere, T._white(hk), None, new)])
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    depth = _info(hk, gpu_ctx, se)[2]

    def frames(s, rebuild):
        film = hk.Film((37, 29))
        cam = E._camera(hk, film)
        vp = hk.VolPath(max_depth=3, samples=16)
        out = []
        for k in range(2):
            vp._ensure(film)
            vp.clear()
            vp.reset_stats()
            vp.render_samples(s, film, cam, 16, first=1, readback=False)
            out.append((vp.read_accumulators(film).copy(), int(vp.stats().view_cache_hits)))
            if rebuild and k == 0:
                s.rebuild_bvh(gpu_ctx)
        vp.close()
        return out

    got, want = frames(se, True), frames(sf, False)
    assert _info(hk, gpu_ctx, se)[2] <= 16 and depth <= 16                      # the depth class is kept
    assert [g[1] for g in got] == [0, 1] == [w[1] for w in want]                 # the second frame kept the camera records
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0])


def test_leaf_size_and_bin_count_of_the_context_are_honoured(hk, gpu_ctx, knobs):
    knobs.setenv("HK_BVH_LEAF", "2")
    knobs.setenv("HK_BVH_BINS", "16")
    sphere = E._sphere(tess=16)
    new = T._rippled(sphere, 0.1)
    se, insts, sf = T._pair(hk, [(sphere, T._white(hk), None, new)])              # both created under the knobs
    assert _no_median(sf, 2, 16)
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    se.rebuild_bvh(gpu_ctx)
    fresh, got = _tree(hk, gpu_ctx, sf), _tree(hk, gpu_ctx, se)
    _assert_same_tree(got, fresh)
    assert (((~got["refs"][got["refs"] < 0]) & 7) + 1).max() == 2
    knobs.restore()
    default, _, _ = T._pair(hk, [(sphere, T._white(hk), None, new)])
    assert _tree(hk, gpu_ctx, default)["info"] != fresh["info"]                   # (the knobs do change the tree)
