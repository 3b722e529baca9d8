"""Vertex edits on the device (hk_scene_set_vertices) and the tree cost (hk_scene_bvh_cost, hk_scene_bvh_copy).  The yardstick is the one
of tests/test_scene_edits.py: closest hits are the lexicographic minimum of (t, prim) whatever the BVH, so a scene whose mesh was
DEFORMED IN PLACE and whose tree was refit renders bit for bit like a scene BUILT FRESH from the deformed mesh.  Every film and hit
comparison is np.array_equal; the helpers are those of test_scene_edits.py and xform_ref.py."""
import ctypes as C

import numpy as np
import pytest

import test_scene_edits as E
import vertex_ref as V
import xform_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32
PI32 = C.POINTER(C.c_int32)


def _white(hk):
    return lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))


def _pair(hk, objects, walls=True):
    """objects: [(mesh as pushed, material factory, 4x4 or None, mesh as edited or None)].  -> (scene to edit, its instances, scene
    built fresh from the edited meshes, moved by tests/xform_ref.py where the instance has a transform)."""
    from hikari_jl_amd.geometry import Mesh
    se, sf = hk.Scene(), hk.Scene()
    if walls:
        E._box(hk, se)
        E._box(hk, sf)
    insts = []
    for mesh, mat, m, new in objects:
        insts.append(se.push_instance(mesh, mat(), m))
        new = mesh if new is None else new
        if m is None:
            sf.push(new, mat())
        else:
            P, N, _ = X.transform_mesh(m[:3], new.positions, new.normals)
            sf.push(Mesh(P, N, new.uvs), mat())
    se.sync()
    sf.sync()
    return se, insts, sf


def _rippled(mesh, amplitude=0.1, uvs=None, **kw):
    from hikari_jl_amd.geometry import Mesh
    P, N = V.ripple(mesh.positions, mesh.normals, amplitude, **kw)
    return Mesh(P, N, mesh.uvs if uvs is None else uvs)


def _cornell_rays(seed, n=100_000):
    return E._rays(np.random.default_rng(seed), n, (-0.98, 0.02, -0.98), (0.98, 1.97, 0.98))


def test_hits_small_tree_deformed_sphere_matches_fresh(hk, gpu_ctx):
    sphere = E._sphere(tess=24)
    new = _rippled(sphere, 0.1)
    se, insts, sf = _pair(hk, [(sphere, _white(hk), None, new)])
    hk.scene_handle(gpu_ctx, se)                   # created first: the edit is the in-place one
    o, d, tmax = _cornell_rays(11)
    before = E._trace(hk, gpu_ctx, se, o, d, tmax)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    a, b = E._trace(hk, gpu_ctx, se, o, d, tmax), E._trace(hk, gpu_ctx, sf, o, d, tmax)
    assert (a[0][1] >= insts[0].first_tri).sum() > 1000
    assert not np.array_equal(a[0][0], before[0][0])
    E._assert_same_hits(a, b)


# ---- the deep scene: a box cloud of 33 600 triangles in three meshes; the middle one, [1500, 21504 - 3), is the one deformed ----
N_BOXES, SPLIT_A, SPLIT_B = 2800, 125 * 12, 1791 * 12 + 9


def _deep_meshes(hk):
    from hikari_jl_amd.geometry import Mesh
    P, N = E._boxes(N_BOXES, 3)
    P, N = np.ascontiguousarray(P, f32), np.ascontiguousarray(N, f32)
    assert SPLIT_A % 1024 != 0 and SPLIT_B % 1024 != 0
    return [Mesh(P[:SPLIT_A], N[:SPLIT_A], None), Mesh(P[SPLIT_A:SPLIT_B], N[SPLIT_A:SPLIT_B], None), Mesh(P[SPLIT_B:], N[SPLIT_B:], None)]


def _deep_deformed(mesh, scale=1.0):
    """Every corner of the middle mesh pushed by a smooth field of about one box size (times `scale`), the first 600 triangles carried
    5 units past the cloud's bounds in +x: the root box as created does not hold them."""
    from hikari_jl_amd.geometry import Mesh
    P = mesh.positions
    disp = np.stack([np.sin(f32(3) * P[..., 1] + f32(1)), np.cos(f32(2) * P[..., 2]), np.sin(f32(4) * P[..., 0])], axis=-1).astype(f32)
    Q = (P + f32(0.05 * scale) * disp).astype(f32)
    Q[:600, :, 0] += f32(13.0)
    Q = np.ascontiguousarray(Q)
    return Mesh(Q, V.face_normals(Q), None)


def _deep_pair(hk, scale=1.0):
    meshes = _deep_meshes(hk)
    new = _deep_deformed(meshes[1], scale)
    grey = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6))
    se, insts, sf = _pair(hk, [(meshes[0], grey, None, None), (meshes[1], grey, None, new), (meshes[2], grey, None, None)], walls=False)
    for s in (se, sf):
        s.push(hk.PointLight((0.0, 0.0, 8.0), hk.RGBSpectrum(40.0)))
        s.sync()
    return se, insts, sf, meshes, new


def _assert_deep(hk, gpu_ctx, s):
    sh = hk.scene_handle(gpu_ctx, s)
    depth = C.c_int32()
    hk._lib.check(hk._lib.lib().hk_scene_bvh_info(sh, None, None, C.byref(depth)), "hk_scene_bvh_info")
    assert depth.value > 16 and s.desc.n_triangles >= 32768          # quantised nodes and packed shading records: neither path is skipped
    return sh


def test_hits_deep_tree_quantised_nodes_packed_records(hk, gpu_ctx):
    se, insts, sf, meshes, new = _deep_pair(hk)
    _assert_deep(hk, gpu_ctx, se)
    a, e = insts[1].first_tri, insts[1].first_tri + insts[1].n_tris
    assert a % 1024 != 0 and e % 1024 != 0 and e < se.desc.n_triangles
    lo, hi = se.bounds[0], se.bounds[1]
    assert new.positions[..., 0].max() > hi[0] + 1.0                 # the grid of the quantised nodes has to grow
    se.set_vertices(insts[1], new.positions, normals=new.normals)
    rng = np.random.default_rng(13)
    o, d, tmax = E._rays(rng, 100_000, (-7, -7, -7), (7, 7, 7))
    # the last 10 000 rays start half a unit from a triangle carried outside, in the direction generated for them, and look back at it
    aim = new.positions[rng.integers(0, 600, 10_000)].mean(axis=1).astype(f32)
    o[90_000:] = aim + f32(0.5) * d[90_000:]
    d[90_000:] = -d[90_000:]
    got, want = E._trace(hk, gpu_ctx, se, o, d, tmax), E._trace(hk, gpu_ctx, sf, o, d, tmax)
    hit = got[0][1]
    assert ((hit >= a) & (hit < a + 600)).sum() > 1000 and ((hit >= a + 600) & (hit < e)).sum() > 1000
    E._assert_same_hits(got, want)


def test_films_matte_cornell_deformed_matches_fresh(hk, gpu_ctx):
    sphere = E._sphere(tess=24)
    new = _rippled(sphere, 0.1)
    se, insts, sf = _pair(hk, [(sphere, _white(hk), None, new), (E._sphere((0.4, 0.35, 0.3), 0.3), _white(hk), None, None)])
    hk.scene_handle(gpu_ctx, se)
    created = E._film(hk, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    edited = E._film(hk, se)
    assert not np.array_equal(edited, created)
    assert np.array_equal(edited, E._film(hk, sf))
    assert np.array_equal(E._film(hk, se, one_sample=True), E._film(hk, sf, one_sample=True))   # one-sample calls: the fused small pass


def test_films_textured_mesh_with_new_uvs_matches_fresh(hk, gpu_ctx):
    rng = np.random.default_rng(4)
    tex = hk.Texture(rng.random((16, 24, 3)).astype(f32))
    textured = lambda: hk.MatteMaterial(Kd=tex)
    sphere = E._sphere((0.0, 0.7, 0.0), 0.5, 16)
    new = _rippled(sphere, 0.08, uvs=V.swirl_uvs(sphere.uvs))
    se, insts, sf = _pair(hk, [(sphere, textured, None, new)])
    hk.scene_handle(gpu_ctx, se)
    created = E._film(hk, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals, uvs=new.uvs)
    edited = E._film(hk, se)
    assert not np.array_equal(edited, created)
    assert np.array_equal(edited, E._film(hk, sf))
    # the uvs alone change the picture: positions and normals as they are, the texture coordinates back to the pushed ones
    se.set_vertices(insts[0], new.positions, uvs=sphere.uvs)
    back = E._film(hk, se)
    assert not np.array_equal(back, edited) and not np.array_equal(back, created)


def test_films_glass_sphere_with_medium_deformed_matches_fresh(hk, gpu_ctx):
    glass = lambda: hk.MediumInterface(hk.GlassMaterial(index=1.45), inside=hk.HomogeneousMedium(sigma_a=hk.RGBSpectrum(0.3), sigma_s=hk.RGBSpectrum(2.0)))
    sphere = E._sphere((0.0, 0.6, 0.0), 0.45, 16)
    new = _rippled(sphere, 0.05)
    se, insts, sf = _pair(hk, [(sphere, glass, None, new)])
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    assert np.array_equal(E._film(hk, se), E._film(hk, sf))


M_A = X.affine(rot_deg=35.0, axis=(0.3, 1, 0.2), scale=1.2, translate=(0.55, 0.15, -0.1))
M_B = X.affine(rot_deg=-50.0, axis=(1, 0.2, 0), scale=0.8, translate=(0.1, 0.5, 0.2))


def test_transforms_are_kept_in_either_order(hk, gpu_ctx):
    sphere = E._sphere(tess=12)
    new = _rippled(sphere, 0.1)
    o, d, tmax = _cornell_rays(17, 60_000)
    _, _, fresh_moved = _pair(hk, [(sphere, _white(hk), M_A, new)])
    want = E._trace(hk, gpu_ctx, fresh_moved, o, d, tmax)
    # the transform first, then the vertices
    se, insts, _ = _pair(hk, [(sphere, _white(hk), None, None)])
    hk.scene_handle(gpu_ctx, se)
    se.set_transform(insts[0], M_A)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    first = E._trace(hk, gpu_ctx, se, o, d, tmax)
    assert (first[0][1] >= insts[0].first_tri).sum() > 500
    E._assert_same_hits(first, want)
    # the vertices first, then the transform
    s2, i2, _ = _pair(hk, [(sphere, _white(hk), None, None)])
    hk.scene_handle(gpu_ctx, s2)
    s2.set_vertices(i2[0], new.positions, normals=new.normals)
    s2.set_transform(i2[0], M_A)
    E._assert_same_hits(E._trace(hk, gpu_ctx, s2, o, d, tmax), want)
    # a later m34 that is exactly the identity hands the new base back bit for bit
    _, _, fresh_unmoved = _pair(hk, [(sphere, _white(hk), None, new)])
    se.set_transform(insts[0], np.eye(4, dtype=f32))
    E._assert_same_hits(E._trace(hk, gpu_ctx, se, o, d, tmax), E._trace(hk, gpu_ctx, fresh_unmoved, o, d, tmax))
    # and a scene created after the edit (from the kept mesh, under the kept transform) is the fresh scene too
    s2.sync()
    E._assert_same_hits(E._trace(hk, gpu_ctx, s2, o, d, tmax), want)
    assert np.array_equal(E._film(hk, s2, spp=4), E._film(hk, fresh_moved, spp=4))             # normals through the normal matrix


def test_one_range_straddling_two_transforms(hk, gpu_ctx):
    from hikari_jl_amd.geometry import Mesh
    A = hk._abi
    sa, sb = E._sphere((-0.4, 0.4, 0.0), 0.3, 10), E._sphere((0.4, 0.5, 0.2), 0.25, 12)
    na, nb = _rippled(sa, 0.06), _rippled(sb, 0.06, phase=1.0)
    objects = [(sa, _white(hk), M_A, na), (sb, _white(hk), M_B, nb), (E._sphere((0.0, 1.3, 0.0), 0.2, 8), _white(hk), None, None)]
    se, insts, sf = _pair(hk, objects)
    sh = hk.scene_handle(gpu_ctx, se)
    assert insts[1].first_tri == insts[0].first_tri + insts[0].n_tris
    # ONE call of the library over both instances and the first 7 triangles of the third (identity) mesh, which get their own values back
    tail = objects[2][0]
    P = np.ascontiguousarray(np.concatenate([na.positions, nb.positions, tail.positions[:7]]), f32)
    N = np.ascontiguousarray(np.concatenate([na.normals, nb.normals, tail.normals[:7]]), f32)
    hk._lib.check(hk._lib.lib().hk_scene_set_vertices(sh, insts[0].first_tri, len(P), E._pf(hk, P), E._pf(hk, N), None, None), "hk_scene_set_vertices")
    o, d, tmax = _cornell_rays(19, 60_000)
    got = E._trace(hk, gpu_ctx, se, o, d, tmax)
    for inst in insts[:2]:
        assert ((got[0][1] >= inst.first_tri) & (got[0][1] < inst.first_tri + inst.n_tris)).sum() > 300
    E._assert_same_hits(got, E._trace(hk, gpu_ctx, sf, o, d, tmax))
    assert np.array_equal(E._film(hk, se, spp=4), E._film(hk, sf, spp=4))


def test_null_normals_keep_the_base_normals(hk, gpu_ctx):
    from hikari_jl_amd.geometry import Mesh
    sphere = E._sphere(tess=16)
    P, N = V.ripple(sphere.positions, sphere.normals, 0.1)
    se, insts, sf = _pair(hk, [(sphere, _white(hk), M_A, Mesh(P, sphere.normals, sphere.uvs))])   # new positions, the normals as pushed
    _, _, s_new_normals = _pair(hk, [(sphere, _white(hk), M_A, Mesh(P, N, sphere.uvs))])
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], P)
    film = E._film(hk, se)
    assert np.array_equal(film, E._film(hk, sf))
    assert not np.array_equal(film, E._film(hk, s_new_normals))                                  # (the normals do show in the film)


def test_edit_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the mesh as it was when the call was made; the next one sees the new vertices."""
    sphere = E._sphere()
    new = _rippled(sphere, 0.1)
    se, insts, sf = _pair(hk, [(sphere, _white(hk), None, new)])
    s_old, _, _ = _pair(hk, [(sphere, _white(hk), None, None)])
    hk.scene_handle(gpu_ctx, se)

    def run(first, then, edit):
        film = hk.Film((E.W, E.H))
        cam = E._camera(hk, film)
        vp = hk.VolPath(**E.KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)      # noted, not yet rendered
        if edit:
            se.set_vertices(insts[0], new.positions, normals=new.normals)
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(se, se, True)
    want = run(s_old, sf, False)
    assert np.array_equal(got, want)


def test_refused_calls_leave_the_scene_untouched(hk, gpu_ctx):
    from hikari_jl_amd.geometry import Mesh
    A = hk._abi
    L = hk._lib.lib()
    sphere = E._sphere(tess=10)
    se, insts, _ = _pair(hk, [(sphere, _white(hk), M_A, None)])
    sh = hk.scene_handle(gpu_ctx, se)
    o, d, tmax = _cornell_rays(23, 40_000)
    before = E._trace(hk, gpu_ctx, se, o, d, tmax)
    T, a, n = se.desc.n_triangles, insts[0].first_tri, insts[0].n_tris
    P, N = V.ripple(sphere.positions, sphere.normals, 0.1)
    U = V.swirl_uvs(sphere.uvs)
    pf = lambda x: E._pf(hk, x)
    call = lambda *args: L.hk_scene_set_vertices(*args)
    assert call(None, a, n, pf(P), None, None, None) == A.HK_ERR_INVALID
    assert call(sh, a, n, None, pf(N), None, None) == A.HK_ERR_INVALID
    assert call(sh, a, 0, pf(P), None, None, None) == A.HK_ERR_INVALID
    assert call(sh, a, -3, pf(P), None, None, None) == A.HK_ERR_INVALID
    assert call(sh, -1, n, pf(P), None, None, None) == A.HK_ERR_INVALID
    assert call(sh, T - n + 1, n, pf(P), None, None, None) == A.HK_ERR_INVALID
    assert call(sh, T, 1, pf(P), None, None, None) == A.HK_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        Pb = P.copy()
        Pb[n - 1, 2, 1] = bad                                                      # the last float but one of the range
        assert call(sh, a, n, pf(Pb), pf(N), None, pf(U)) == A.HK_ERR_INVALID
        assert L.hk_last_error()
    assert call(sh, a, n, pf(P), None, pf(N), None) == A.HK_ERR_INVALID             # tangents: no scene of this mirror has them
    assert np.array_equal(se._keep[0][a:a + n], sphere.positions)                  # (the library was called directly: the mirror is as pushed)
    E._assert_same_hits(E._trace(hk, gpu_ctx, se, o, d, tmax), before)
    # a scene created without normals and uvs refuses them; one without triangles refuses everything
    tri = Mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 0, 1], [0, 1, 1]]], f32), None, None)
    bare = hk.Scene()
    bare.push_instance(tri, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))
    bare.push(hk.PointLight((0, 1, 3), hk.RGBSpectrum(1.0)))
    bare.sync()
    assert not bare.desc.normals and not bare.desc.uvs
    bh = hk.scene_handle(gpu_ctx, bare)
    P2 = (tri.positions + f32(0.25)).astype(f32)
    assert call(bh, 0, 2, pf(P2), pf(P2), None, None) == A.HK_ERR_INVALID
    assert call(bh, 0, 2, pf(P2), None, None, pf(np.zeros((2, 3, 2), f32))) == A.HK_ERR_INVALID
    assert call(bh, 0, 2, pf(P2), None, None, None) == A.HK_OK                       # (and takes positions alone)
    empty = hk.Scene()
    empty.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(1.0)))
    empty.sync()
    assert call(hk.scene_handle(gpu_ctx, empty), 0, 1, pf(P), None, None, None) == A.HK_ERR_INVALID


def _light_bvh(hk, s, sh):
    L = hk._lib.lib()
    n = C.c_int32()
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), None, None), "hk_scene_light_bvh_copy")
    nodes = np.empty(16 * n.value, f32)
    trails = np.empty(s.desc.n_lights, np.uint32)
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), E._pf(hk, nodes), trails.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_light_bvh_copy")
    return nodes.tobytes() + trails.tobytes()


def test_move_lights_rebuilds_the_instance_lights(hk, gpu_ctx):
    glow = lambda: hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(3.0)))
    lamp = E._sphere((0, 1.0, 0), 0.25, 8)
    new = _rippled(lamp, 0.08)
    se, insts, sf = _pair(hk, [(lamp, glow, None, new)])
    sh = hk.scene_handle(gpu_ctx, se)
    assert se.desc.n_lights == sf.desc.n_lights > 20          # the same faces emit (no face of the deformed lamp is degenerate that was not)
    created = _light_bvh(hk, se, sh)
    se.set_vertices(insts[0], new.positions, normals=new.normals)              # the default: the lights stay (Q18)
    E._film(hk, se, spp=2)
    assert _light_bvh(hk, se, sh) == created
    se.set_vertices(insts[0], new.positions, normals=new.normals, move_lights=True)
    assert hk.scene_handle(gpu_ctx, se) is sh
    moved = _light_bvh(hk, se, sh)
    assert moved != created and moved == _light_bvh(hk, sf, hk.scene_handle(gpu_ctx, sf))
    assert np.array_equal(E._film(hk, se), E._film(hk, sf))


def _bvh_copy(hk, sh):
    L = hk._lib.lib()
    n = C.c_int32()
    hk._lib.check(L.hk_scene_bvh_copy(sh, C.byref(n), None, None), "hk_scene_bvh_copy")
    boxes, refs = np.empty((n.value, 12), f32), np.empty((n.value, 2), np.int32)
    hk._lib.check(L.hk_scene_bvh_copy(sh, C.byref(n), E._pf(hk, boxes), refs.ctypes.data_as(PI32)), "hk_scene_bvh_copy")
    return boxes, refs


def _cost_numpy(boxes, refs):
    """The header's formula in float64: sum over nodes and both children of A(child) * w / A(root); an empty box has no area."""
    b = boxes.astype(np.float64).reshape(-1, 2, 2, 3)            # node, child, lo / hi, axis
    lo, hi = b[:, :, 0], b[:, :, 1]
    valid = (lo <= hi).all(axis=-1)
    with np.errstate(invalid="ignore"):
        d = hi - lo
        area = np.where(valid, 2.0 * ((d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2]) + d[..., 1] * d[..., 2]), 0.0)
    w = np.where(refs >= 0, 1, ((~refs) & 7) + 1)
    rl, rh = lo[0][valid[0]].min(axis=0), hi[0][valid[0]].max(axis=0)
    rd = rh - rl
    root = 2.0 * ((rd[0] * rd[1] + rd[0] * rd[2]) + rd[1] * rd[2])
    return float((area * w).sum() / root)


def test_tree_cost_and_copy(hk, gpu_ctx):
    se, insts, _, meshes, _ = _deep_pair(hk)
    sh = _assert_deep(hk, gpu_ctx, se)
    boxes0, refs0 = _bvh_copy(hk, sh)
    assert len(boxes0) > 8000 and (refs0 < 0).any() and (refs0 >= 0).any() and refs0.max() < len(boxes0)
    now, created = se.bvh_cost(gpu_ctx)
    ref = _cost_numpy(boxes0, refs0)
    # all terms are positive, so any summation order is within (n - 1) * 2^-53 relative of the exact sum: 1e-9 is generous for 2.4e4 terms
    assert created > 1.0 and now == pytest.approx(created, rel=1e-9) and now == pytest.approx(ref, rel=1e-9) and created == pytest.approx(ref, rel=1e-9)
    assert se.bvh_cost(gpu_ctx) == (now, created)                 # no atomics: the same tree gives the same bits
    # the deformation of the hits test with the displacement scaled to several box sizes: the boxes of the old topology grow
    wild = _deep_deformed(meshes[1], scale=6.0)
    se.set_vertices(insts[1], wild.positions, normals=wild.normals)
    now2, created2 = se.bvh_cost(gpu_ctx)
    boxes2, refs2 = _bvh_copy(hk, sh)
    assert created2 == created and now2 > created and np.array_equal(refs2, refs0) and not np.array_equal(boxes2, boxes0)
    assert now2 == pytest.approx(_cost_numpy(boxes2, refs2), rel=1e-9)
    assert se.bvh_cost(gpu_ctx) == (now2, created2)
    # back to the arrays as pushed: the refit tree is the built tree, bit for bit
    se.set_vertices(insts[1], meshes[1].positions, normals=meshes[1].normals)
    boxes3, refs3 = _bvh_copy(hk, sh)
    assert np.array_equal(boxes3, boxes0) and np.array_equal(refs3, refs0)
    assert se.bvh_cost(gpu_ctx) == (now, created)
    # a scene whose root is a leaf has no inner node: both costs are 0
    from hikari_jl_amd.geometry import Mesh
    one = hk.Scene()
    one.push(Mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], f32), None, None), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))
    one.push(hk.PointLight((0, 1, 3), hk.RGBSpectrum(1.0)))
    one.sync()
    if len(_bvh_copy(hk, hk.scene_handle(gpu_ctx, one))[0]) == 0:
        assert one.bvh_cost(gpu_ctx) == (0.0, 0.0)
