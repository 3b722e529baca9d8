"""Scene edits on the device (hk_scene_set_transform, hk_scene_update_materials).  Closest hits are the lexicographic minimum of
(t, prim) whatever the BVH, so a scene whose tree was REFIT after a move renders bit-identically to a scene BUILT FRESH from the moved
triangles (moved here by tests/xform_ref.py, the NumPy reference of the header's arithmetic).  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import xform_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 48, 40
KW = dict(max_depth=5, samples=16)


def _pf(hk, a):
    return a.ctypes.data_as(hk._abi.PF)


def _box(hk, s):
    """Cornell walls + area light (never moved: area lights keep the geometry of their push, Q18)."""
    from hikari_jl_amd import geometry as G
    white, red, green = (hk.MatteMaterial(Kd=hk.RGBSpectrum(*c)) for c in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15)))
    s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), white)
    s.push(G.rect3f((-1, 1.99, -1), (2, 0.01, 2)), white)
    s.push(G.rect3f((-1, 0, 0.99), (2, 2, 0.01)), white)
    s.push(G.rect3f((-1, 0, -1), (0.01, 2, 2)), red)
    s.push(G.rect3f((0.99, 0, -1), (0.01, 2, 2)), green)
    q = G.quad((-0.25, 1.98, -0.25), (0.25, 1.98, -0.25), (0.25, 1.98, 0.25), (-0.25, 1.98, 0.25), normal=(0, -1, 0))
    s.push(q, hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(6.0))))


def _pair(hk, objects, walls=True):
    """objects: [(mesh, material factory, 4x4 or None)].  Returns (refit scene + its instances, fresh scene): the refit scene carries
    the meshes as pushed and is moved after hk_scene_create; the fresh one is built from the meshes the reference moved."""
    from hikari_jl_amd.geometry import Mesh
    sr, sf = hk.Scene(), hk.Scene()
    if walls:
        _box(hk, sr)
        _box(hk, sf)
    insts = []
    for mesh, mat, m in objects:
        insts.append(sr.push_instance(mesh, mat()))
        if m is None:
            sf.push(mesh, mat())
        else:
            P, N, _ = X.transform_mesh(m[:3], mesh.positions, mesh.normals)
            sf.push(Mesh(P, N, mesh.uvs), mat())
    sr.sync()
    sf.sync()
    return sr, insts, sf


def _move(hk, ctx, s, insts, objects):
    hk.scene_handle(ctx, s)                     # created first: the edit is the in-place one
    for inst, (_, _, m) in zip(insts, objects):
        if m is not None:
            s.set_transform(inst, m)


def _camera(hk, film):
    return hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0)


def _film(hk, s, spp=16, one_sample=False, kw=KW):
    film = hk.Film((W, H))
    cam = _camera(hk, film)
    vp = hk.VolPath(**kw)
    vp._ensure(film)
    vp.clear()
    if one_sample:
        for i in range(1, spp + 1):
            vp.render_samples(s, film, cam, 1, first=i, readback=False)
    else:
        vp.render_samples(s, film, cam, spp, first=1, readback=False)
    acc = vp.read_accumulators(film).copy()
    vp.close()
    return acc


def _rays(rng, n, lo, hi):
    o = rng.uniform(lo, hi, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:500] = np.array([0, -1, 0], f32)
    tmax = np.full(n, np.inf, f32)
    tmax[::5] = rng.uniform(0, 2, len(tmax[::5])).astype(f32)
    return o, d.astype(f32), tmax


def _trace(hk, ctx, s, o, d, tmax):
    L = hk._lib.lib()
    sh = hk.scene_handle(ctx, s)
    n = len(o)
    out = []
    t, p, uv = np.empty(n, f32), np.empty(n, np.int32), np.empty((n, 2), f32)
    hk._lib.check(L.hk_trace_closest(ctx.h, sh, n, _pf(hk, o), _pf(hk, d), _pf(hk, tmax), _pf(hk, t), p.ctypes.data_as(C.POINTER(C.c_int32)), _pf(hk, uv)), "hk_trace_closest")
    out.append((t, p, uv))
    for anyhit in (0, 1):
        t, p, uv = np.empty(n, f32), np.empty(n, np.int32), np.empty((n, 2), f32)
        hk._lib.check(L.hk_test_trace_lean(ctx.h, sh, anyhit, n, _pf(hk, o), _pf(hk, d), _pf(hk, tmax), _pf(hk, t), p.ctypes.data_as(C.POINTER(C.c_int32)), _pf(hk, uv)),
                      "hk_test_trace_lean")
        out.append((t, p, uv))
    return out


def _assert_same_hits(a, b):
    for k in range(2):   # closest hit, both traversals: (t, prim, uv)
        assert np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][2], b[k][2])
    assert np.array_equal(a[2][1] >= 0, b[2][1] >= 0)   # any-hit: occluded or not


def _sphere(c=(-0.4, 0.4, 0.0), r=0.35, tess=24):
    from hikari_jl_amd import geometry as G
    return G.sphere(c, r, tess)


M_SPHERE = X.affine(rot_deg=35.0, axis=(0.3, 1, 0.2), scale=1.2, translate=(0.55, 0.15, -0.1))


def test_traversal_refit_matches_fresh_cornell(hk, gpu_ctx):
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = [(_sphere(), white, M_SPHERE), (_sphere((0.4, 0.35, 0.3), 0.3), white, None)]
    sr, insts, sf = _pair(hk, objects)
    _move(hk, gpu_ctx, sr, insts, objects)
    o, d, tmax = _rays(np.random.default_rng(5), 400_000, (-0.98, 0.02, -0.98), (0.98, 1.97, 0.98))
    a, b = _trace(hk, gpu_ctx, sr, o, d, tmax), _trace(hk, gpu_ctx, sf, o, d, tmax)
    assert (a[0][1] >= insts[0].first_tri).sum() > 1000 and (a[0][1] >= 0).mean() > 0.5
    _assert_same_hits(a, b)


def _boxes(n_boxes, seed):
    from hikari_jl_amd import scenes
    rng = np.random.default_rng(seed)
    layer = rng.integers(0, 12, n_boxes)
    radius = 1.0 + 0.45 * layer + 0.1 * rng.random(n_boxes)
    phi = rng.random(n_boxes) * 2 * np.pi
    centers = np.stack([radius * np.cos(phi), radius * np.sin(phi), (rng.random(n_boxes) * 2 - 1) * 6.0], axis=1)
    half = 0.012 + 0.03 * rng.random((n_boxes, 3))
    return scenes._boxes_mesh(centers, half, rng.random(n_boxes) * np.pi)


def million_triangle_pair(hk, moved_frac=0.01, shift=0.05):
    """~10^6 triangles of boxes in barrel layers (the many-light layout, lit by a point light), tree deeper than 16 levels (quantised
    nodes); the first `moved_frac` of the boxes is an instance moved by about one box size."""
    from hikari_jl_amd.geometry import Mesh
    P, N = _boxes(83334, 1)
    k = int(83334 * moved_frac) * 12
    objects = [(Mesh(P[:k], N[:k], None), lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6)), X.affine(translate=(shift, -shift, shift))),
               (Mesh(P[k:], N[k:], None), lambda: hk.ConductorMaterial(roughness=0.2), None)]
    sr, insts, sf = _pair(hk, objects, walls=False)
    for s in (sr, sf):
        s.push(hk.PointLight((0.0, 0.0, 8.0), hk.RGBSpectrum(40.0)))
        s.sync()
    return sr, insts, sf, objects


def test_traversal_refit_matches_fresh_million_triangles(hk, gpu_ctx):
    sr, insts, sf, objects = million_triangle_pair(hk)
    _move(hk, gpu_ctx, sr, insts, objects)
    depth = C.c_int32()
    hk._lib.lib().hk_scene_bvh_info(hk.scene_handle(gpu_ctx, sr), None, None, C.byref(depth))
    assert depth.value > 16
    o, d, tmax = _rays(np.random.default_rng(7), 300_000, (-7, -7, -7), (7, 7, 7))
    a, b = _trace(hk, gpu_ctx, sr, o, d, tmax), _trace(hk, gpu_ctx, sf, o, d, tmax)
    assert ((a[0][1] >= 0) & (a[0][1] < insts[0].n_tris)).sum() > 20
    _assert_same_hits(a, b)


def test_films_matte_cornell_refit_matches_fresh(hk, gpu_ctx):
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = [(_sphere(), white, M_SPHERE), (_sphere((0.4, 0.35, 0.3), 0.3), white, None)]
    sr, insts, sf = _pair(hk, objects)
    _move(hk, gpu_ctx, sr, insts, objects)
    assert np.array_equal(_film(hk, sr), _film(hk, sf))
    assert np.array_equal(_film(hk, sr, one_sample=True), _film(hk, sf, one_sample=True))   # one-sample calls: the fused small pass


def test_films_glass_sphere_with_medium_refit_matches_fresh(hk, gpu_ctx):
    glass = lambda: hk.MediumInterface(hk.GlassMaterial(index=1.45), inside=hk.HomogeneousMedium(sigma_a=hk.RGBSpectrum(0.3), sigma_s=hk.RGBSpectrum(2.0)))
    objects = [(_sphere(), glass, M_SPHERE)]
    sr, insts, sf = _pair(hk, objects)
    _move(hk, gpu_ctx, sr, insts, objects)
    assert np.array_equal(_film(hk, sr), _film(hk, sf))


def test_films_alpha_panel_and_mixed_normals_refit_matches_fresh(hk, gpu_ctx):
    from hikari_jl_amd import geometry as G
    panel = G.quad((-0.5, 0.2, 0.2), (0.5, 0.2, 0.2), (0.5, 1.4, 0.2), (-0.5, 1.4, 0.2))                    # no normals
    alpha = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.8, 0.7, 0.6, 0.5))
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = [(panel, alpha, X.affine(rot_deg=-20, axis=(0, 1, 0), translate=(0.1, 0.1, -0.2))),
               (_sphere((0.4, 0.35, 0.3), 0.3), white, X.affine(translate=(-0.2, 0.3, 0.0))),                    # with normals
               (G.quad((-0.9, 0.01, -0.9), (-0.2, 0.01, -0.9), (-0.2, 0.01, -0.2), (-0.9, 0.01, -0.2)), white, X.affine(translate=(0, 0.3, 0)))]
    sr, insts, sf = _pair(hk, objects)
    _move(hk, gpu_ctx, sr, insts, objects)
    assert np.array_equal(_film(hk, sr), _film(hk, sf))


def test_round_trip_identity_restores_the_created_scene(hk, gpu_ctx):
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = [(_sphere(), white, M_SPHERE)]
    sr, insts, _ = _pair(hk, objects)
    hk.scene_handle(gpu_ctx, sr)
    created = _film(hk, sr)
    sr.set_transform(insts[0], M_SPHERE)
    moved = _film(hk, sr)
    sr.set_transform(insts[0], np.eye(4, dtype=f32))
    assert not np.array_equal(moved, created)
    assert np.array_equal(_film(hk, sr), created)


def test_edit_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the scene as it was when the call was made; the next one sees the move."""
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = [(_sphere(), white, M_SPHERE)]
    sr, insts, sf = _pair(hk, objects)
    s_old, _, _ = _pair(hk, [(_sphere(), white, None)])
    hk.scene_handle(gpu_ctx, sr)

    def run(first, then, move):
        film = hk.Film((W, H))
        cam = _camera(hk, film)
        vp = hk.VolPath(**KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)      # noted, not yet rendered
        if move:
            sr.set_transform(insts[0], M_SPHERE)
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(sr, sr, True)
    want = run(s_old, sf, False)
    assert np.array_equal(got, want)


def _material_objects(hk, new):
    from hikari_jl_amd import geometry as G
    if not new:
        mats = [lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7, 0.2, 0.2)), lambda: hk.GlassMaterial(index=1.5),
                lambda: hk.ConductorMaterial(roughness=0.3),
                lambda: hk.MixMaterial((hk.MatteMaterial(Kd=hk.RGBSpectrum(0.2, 0.7, 0.2)), hk.ConductorMaterial(roughness=0.1)), amount=0.3)]
    else:
        mats = [lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.1, 0.3, 0.8)), lambda: hk.GlassMaterial(index=1.9),
                lambda: hk.ConductorMaterial(roughness=0.05),
                lambda: hk.MixMaterial((hk.MatteMaterial(Kd=hk.RGBSpectrum(0.2, 0.7, 0.2)), hk.ConductorMaterial(roughness=0.1)), amount=0.8)]
    spots = [((-0.5, 0.3, -0.3), 0.25), ((0.45, 0.3, -0.3), 0.25), ((-0.45, 1.0, 0.4), 0.3), ((0.45, 1.0, 0.4), 0.3)]
    return [(G.sphere(c, r, 16), m, None) for (c, r), m in zip(spots, mats)]


def test_material_updates_match_fresh(hk, gpu_ctx):
    old = _material_objects(hk, False)
    new = _material_objects(hk, True)
    sr, insts, _ = _pair(hk, old)
    _, _, sf = _pair(hk, new)
    hk.scene_handle(gpu_ctx, sr)
    before = _film(hk, sr)
    for inst, (_, mat, _) in zip(insts, new):
        sr.update_material(inst.mi_idx, mat())
    after = _film(hk, sr)
    assert not np.array_equal(before, after)
    assert np.array_equal(after, _film(hk, sf))


def test_refused_edits_leave_the_scene_untouched(hk, gpu_ctx):
    A = hk._abi
    L = hk._lib.lib()
    white = lambda: hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73))
    objects = _material_objects(hk, False) + [(_sphere((0, 1.4, 0), 0.2, 12), white, None)]
    sr, insts, _ = _pair(hk, objects)
    sh = hk.scene_handle(gpu_ctx, sr)
    before = _film(hk, sr)
    d = sr.desc
    nm, T = d.n_materials, d.n_triangles
    rec = lambda i: A.hk_material.from_buffer_copy(d.materials[i])
    matte = sr.media_interfaces[insts[0].mi_idx][0]
    mix = sr.media_interfaces[insts[3].mi_idx][0]
    refusals = []
    r = rec(matte); r.kind = A.HK_MAT_GLASS; refusals.append((matte, r))                     # another kind
    r = rec(matte); r.rgb[0].c[3] = 0.5; refusals.append((matte, r))                         # opacity class
    r = rec(matte); r.rgb[0].tex = 0; refusals.append((matte, r))                            # texture out of range (and alpha-tested)
    r = rec(matte); r.f[0].tex = 3; refusals.append((matte, r))                              # float texture out of range
    r = rec(mix); r.i[0] = r.i[1]; refusals.append((mix, r))                                 # Mix children
    r = rec(mix); r.mix_key[1] += 1; refusals.append((mix, r))
    cond = sr.media_interfaces[insts[2].mi_idx][0]
    r = rec(cond); r.spectrum[0] = 2; refusals.append((cond, r))                             # spectrum out of range
    for idx, r in refusals:
        assert L.hk_scene_update_materials(sh, idx, 1, C.byref(r)) == A.HK_ERR_INVALID, idx
        assert L.hk_last_error()
    ok = rec(matte)
    assert L.hk_scene_update_materials(sh, nm, 1, C.byref(ok)) == A.HK_ERR_INVALID
    assert L.hk_scene_update_materials(sh, -1, 1, C.byref(ok)) == A.HK_ERR_INVALID
    assert L.hk_scene_update_materials(sh, 0, 0, C.byref(ok)) == A.HK_ERR_INVALID
    assert L.hk_scene_update_materials(sh, 0, 1, None) == A.HK_ERR_INVALID
    # a two-record update whose second record is bad changes neither
    two = (A.hk_material * 2)(rec(matte), rec(matte))
    two[0].rgb[0].c[0] = 0.01
    two[1].kind = A.HK_MAT_MIRROR
    assert L.hk_scene_update_materials(sh, matte, 2, two) == A.HK_ERR_INVALID
    m = X.affine(translate=(0.1, 0, 0))[:3].copy()
    assert L.hk_scene_set_transform(sh, T - 1, 2, _pf(hk, m)) == A.HK_ERR_INVALID
    assert L.hk_scene_set_transform(sh, -1, 1, _pf(hk, m)) == A.HK_ERR_INVALID
    assert L.hk_scene_set_transform(sh, 0, 0, _pf(hk, m)) == A.HK_ERR_INVALID
    assert L.hk_scene_set_transform(sh, 0, 1, None) == A.HK_ERR_INVALID
    for bad in (np.inf, np.nan):
        mb = m.copy()
        mb[1, 3] = bad
        assert L.hk_scene_set_transform(sh, 0, 1, _pf(hk, mb)) == A.HK_ERR_INVALID
    sing = m.copy()
    sing[2, :3] = sing[0, :3]
    assert L.hk_scene_set_transform(sh, 0, 1, _pf(hk, sing)) == A.HK_ERR_INVALID
    assert np.array_equal(_film(hk, sr), before)
    # a scene without triangles refuses a transform
    empty = hk.Scene()
    empty.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(1.0)))
    empty.sync()
    assert L.hk_scene_set_transform(hk.scene_handle(gpu_ctx, empty), 0, 1, _pf(hk, m)) == A.HK_ERR_INVALID


def test_moving_an_emissive_instance_keeps_the_light_bvh(hk, gpu_ctx):
    L = hk._lib.lib()
    s = hk.Scene()
    _box(hk, s)
    inst = s.push_instance(_sphere((0, 1.0, 0), 0.2, 8), hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(3.0))))
    s.sync()
    sh = hk.scene_handle(gpu_ctx, s)

    def copy():
        n = C.c_int32()
        hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), None, None), "hk_scene_light_bvh_copy")
        nodes = np.empty(16 * n.value, f32)
        trails = np.empty(s.desc.n_lights, np.uint32)
        hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), _pf(hk, nodes), trails.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_light_bvh_copy")
        return nodes.tobytes() + trails.tobytes()

    before = copy()
    s.set_transform(inst, X.affine(rot_deg=40, translate=(0.3, -0.2, 0.1)))
    _film(hk, s, spp=2)
    assert copy() == before
