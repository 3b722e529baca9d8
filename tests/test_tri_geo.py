"""The per-triangle geometry table (DScene::tri_geo; hk_device.h: tri_geo_of, surface_at).  The geometric normal and the area of the hit
triangle are a function of its three world positions, which change only on a geometry edit: a row (n.x, n.y, n.z, area) per triangle
is written on the device wherever positions are written — k_tri_geo at hk_scene_create, k_xform_tris (hk_scene_set_transform),
k_set_tris (hk_scene_set_vertices) — by the ONE function surface_at calls where it computes them, and the lean k_shade (Matte under
simple lights: the Cornell frame's shading kernel) reads the row in place of the three positions.  Checked here:

  rows    hk_test_tri_geo copies the table back, and has a kernel of its own compute the rows from the positions the device holds
          through the shared function: equal as uint32 (NaN payloads of zero-area triangles included), for a created scene of every
          geometry kind and after every edit — where they also equal the rows of a scene CREATED in the edited state;
  films   under HK_TRI_GEO=0 (surface_at computes, as before the table) and the default: film accumulators and the ray / vertex / hit /
          light-node counters bit for bit — the lean kernel's slot and queue walks, and the scenes whose kernels (the general k_shade,
          k_scatter, k_small_pass, k_light_select_pool) keep computing: the knob must be neutral there too.

Small films at depth 3 on the staged path, as in test_shade_slot_walk.py."""
import ctypes as C

import numpy as np
import pytest

import test_scene_edits as E
import test_shade_slot_walk as SW
import test_vertex_edits as VE

pytestmark = pytest.mark.gpu
f32 = np.float32
PF = C.POINTER(C.c_float)


def _rows(hk, ctx, s, recompute):
    sh = hk.scene_handle(ctx, s)
    L = hk._lib.lib()
    n, has = C.c_int32(), C.c_int32()
    hk._lib.check(L.hk_test_tri_geo(sh, recompute, C.byref(n), C.byref(has), None), "hk_test_tri_geo")
    assert n.value == s.desc.n_triangles and has.value == 1
    out = np.zeros((n.value, 4), f32)
    hk._lib.check(L.hk_test_tri_geo(sh, recompute, C.byref(n), C.byref(has), out.ctypes.data_as(PF)), "hk_test_tri_geo")
    return out.view(np.uint32)


def _assert_table(hk, ctx, s, positions=None):
    """the table equals the shared function on the device's positions, bit for bit; and (positions given: the world positions, [T, 3, 3])
    is the unit normal and the area of every triangle that has one, by float64 arithmetic"""
    table, fresh = _rows(hk, ctx, s, 0), _rows(hk, ctx, s, 1)
    assert np.array_equal(table, fresh)
    if positions is not None:
        # Against float64 on the same inputs.  The subtractions b - a, c - a round by at most 2^-24 of the largest coordinate per
        # component, which moves the cross product by about sqrt(3) 2^-24 max|p| (|e1| + |e2|); its products and sums add 2^-22 of the
        # result.  Four times the first term and the second bound |cross|; half of it the area.
        P = np.asarray(positions, np.float64)
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        cr = np.cross(e1, e2)
        nrm = np.linalg.norm(cr, axis=1)
        tol = 4.0 * 2.0 ** -24 * np.abs(P).max(axis=(1, 2)) * (np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)) + 2.0 ** -22 * nrm
        rows = table.view(f32).astype(np.float64)
        ok = nrm > 0
        assert (np.abs(rows[ok, 3] - 0.5 * nrm[ok]) <= 0.5 * tol[ok]).all()
        well = nrm > 1000.0 * tol          # the direction is known to a thousandth there
        assert well.sum() > len(P) // 2
        assert np.abs(np.linalg.norm(rows[well, :3], axis=1) - 1.0).max() < 1e-6
        assert (np.einsum("ij,ij->i", rows[well, :3], cr[well] / nrm[well, None]) > 1.0 - 1e-5).all()
    return table


def _soup():
    """random triangles without normals; zero-area ones (two vertices equal, three equal, three in a line), coplanar overlapping pairs"""
    rng = np.random.default_rng(17)
    P = (rng.random((300, 3, 3)) * 2 - 1).astype(f32)
    P[10:20, 1] = P[10:20, 0]                                    # an edge of length 0
    P[20:30, 1] = P[20:30, 0]
    P[20:30, 2] = P[20:30, 0]                                    # a point
    P[30:40] = np.round(P[30:40] * 256) / 256                    # (multiples of 2^-8: the differences and their products are exact)
    P[30:40, 2] = P[30:40, 0] + f32(2.0) * (P[30:40, 1] - P[30:40, 0])   # three points of a line: the cross product is exactly 0
    P[40:60, :, 1] = f32(0.25)                                   # twenty triangles of one plane, overlapping
    P[60:70] = P[40:50]                                          # and ten of them twice
    return np.ascontiguousarray(P)


def _scene_of(hk, mesh, light=True):
    s = hk.Scene()
    if light:
        s.push(hk.PointLight((0.0, 1.5, -2.0), hk.RGBSpectrum(8.0)))
    s.push(mesh, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    s.sync()
    return s


def test_created_cornell_box(hk, gpu_ctx):
    from hikari_jl_amd import scenes
    s = scenes.cornell_box(37, 29, light="area", tess=8)[0]
    t = _assert_table(hk, gpu_ctx, s)
    assert np.isfinite(t.view(f32)).all()


def test_created_sphere(hk, gpu_ctx):
    from hikari_jl_amd import geometry as G
    m = G.sphere((0.1, 0.2, 0.3), 0.7, 12)
    _assert_table(hk, gpu_ctx, _scene_of(hk, m), m.positions)


def test_created_soup_zero_area_coplanar_no_normals(hk, gpu_ctx):
    from hikari_jl_amd.geometry import Mesh
    P = _soup()
    t = _assert_table(hk, gpu_ctx, _scene_of(hk, Mesh(P, None, None)), P).view(f32)
    assert np.isnan(t[10:40, :3]).all() and (t[10:40, 3] == 0).all()      # 1 / 0 times 0: the NaNs compared as bits above
    assert np.isfinite(t[40:70]).all() and np.array_equal(t[60:70], t[40:50])


def test_created_packed_records(hk, gpu_ctx):
    """33 600 triangles: the scene takes the packed 128-byte records, and the rows are their last four words"""
    meshes = VE._deep_meshes(hk)
    s = hk.Scene()
    for m in meshes:
        s.push(m, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6)))
    s.push(hk.PointLight((0.0, 0.0, 8.0), hk.RGBSpectrum(40.0)))
    s.sync()
    assert s.desc.n_triangles >= 32768
    _assert_table(hk, gpu_ctx, s, np.concatenate([m.positions for m in meshes]))


def test_packed_records_of_a_small_scene(hk, gpu_ctx, knobs):
    """HK_TRI_PACK=1 / 0 on the same soup: the rows are the same wherever they are kept"""
    from hikari_jl_amd.geometry import Mesh
    P = _soup()
    knobs.setenv("HK_TRI_PACK", "1")
    a = _assert_table(hk, gpu_ctx, _scene_of(hk, Mesh(P, None, None)))
    knobs.setenv("HK_TRI_PACK", "0")
    b = _assert_table(hk, gpu_ctx, _scene_of(hk, Mesh(P, None, None)))
    assert np.array_equal(a, b)


def test_rows_follow_set_transform(hk, gpu_ctx):
    sphere = E._sphere(tess=12)
    se, insts, sf = VE._pair(hk, [(sphere, VE._white(hk), VE.M_A, None)])      # placed by hk_scene_set_transform right after the create
    placed = _assert_table(hk, gpu_ctx, se)
    assert np.array_equal(placed, _assert_table(hk, gpu_ctx, sf))               # ... as a scene created from the moved mesh has them
    se.set_transform(insts[0], VE.M_B)
    moved = _assert_table(hk, gpu_ctx, se)
    a, e = insts[0].first_tri, insts[0].first_tri + insts[0].n_tris
    assert np.array_equal(moved[:a], placed[:a]) and np.array_equal(moved[e:], placed[e:]) and not np.array_equal(moved[a:e], placed[a:e])
    _, _, sf_b = VE._pair(hk, [(sphere, VE._white(hk), VE.M_B, None)])
    assert np.array_equal(moved, _assert_table(hk, gpu_ctx, sf_b))


@pytest.mark.parametrize("packed", [False, True])
def test_rows_follow_set_vertices_whole_and_sub_range(hk, gpu_ctx, knobs, packed):
    from hikari_jl_amd.geometry import Mesh
    knobs.setenv("HK_TRI_PACK", "1" if packed else "0")
    sphere = E._sphere(tess=12)
    new = VE._rippled(sphere, 0.1)
    se, insts, sf = VE._pair(hk, [(sphere, VE._white(hk), None, new)])
    sh = hk.scene_handle(gpu_ctx, se)
    created = _rows(hk, gpu_ctx, se, 0)
    a, n = insts[0].first_tri, insts[0].n_tris
    # a sub-range first (no multiple of the 64 rows a wave takes, not at the mesh's start): the library call itself
    lo, cnt = 37, 101
    assert lo + cnt < n
    sub = np.ascontiguousarray(new.positions[lo:lo + cnt], f32)
    subn = np.ascontiguousarray(new.normals[lo:lo + cnt], f32)
    hk._lib.check(hk._lib.lib().hk_scene_set_vertices(sh, a + lo, cnt, sub.ctypes.data_as(PF), subn.ctypes.data_as(PF), None, None), "hk_scene_set_vertices")
    part = _assert_table(hk, gpu_ctx, se)
    keep = np.ones(len(created), bool)
    keep[a + lo:a + lo + cnt] = False
    assert np.array_equal(part[keep], created[keep]) and not np.array_equal(part[~keep], created[~keep])
    mixed = sphere.positions.copy()
    mixed[lo:lo + cnt] = sub
    s_part = hk.Scene()
    E._box(hk, s_part)
    s_part.push(Mesh(mixed, None, None), VE._white(hk)())
    s_part.sync()
    assert np.array_equal(part, _rows(hk, gpu_ctx, s_part, 0))
    # then the whole mesh
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    whole = _assert_table(hk, gpu_ctx, se)
    assert np.array_equal(whole, _assert_table(hk, gpu_ctx, sf))


def test_rows_under_a_transform_then_new_vertices_then_rebuild(hk, gpu_ctx):
    """set_vertices on an instance that is under a transform (k_set_tris applies it), then hk_scene_rebuild_bvh (moves no vertex): the
    rows of a scene created in that state"""
    sphere = E._sphere(tess=12)
    new = VE._rippled(sphere, 0.1)
    se, insts, sf = VE._pair(hk, [(sphere, VE._white(hk), VE.M_A, new)])
    hk.scene_handle(gpu_ctx, se)
    se.set_vertices(insts[0], new.positions, normals=new.normals)
    edited = _assert_table(hk, gpu_ctx, se)
    want = _assert_table(hk, gpu_ctx, sf)
    assert np.array_equal(edited, want)
    se.rebuild_bvh(gpu_ctx)
    assert np.array_equal(_assert_table(hk, gpu_ctx, se), want)


# ---- films and counters under HK_TRI_GEO=0 and the default ----
def _ab(hk, knobs, build, spp, depth, env=None, **kw):
    env = {"HK_DYNAMIC_SEGMENTS": "1"} if env is None else env
    knobs.delenv("HK_TRI_GEO")
    on = SW._render(hk, knobs, build, spp, depth, env, **kw)
    off = SW._render(hk, knobs, build, spp, depth, env, ("HK_TRI_GEO", "0"), **kw)
    knobs.delenv("HK_TRI_GEO")
    assert np.isfinite(on[0]).all() and on[0].max() > 0 and on[1][0] > 0 and on[1][3] > 0
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32)), "film differs under HK_TRI_GEO=0"
    assert on[1] == off[1], (on[1], off[1])
    return on


@pytest.mark.parametrize("size", [(37, 29), (64, 48)])
@pytest.mark.parametrize("view", ["open", "closed", "light"])
def test_box_films(hk, knobs, view, size):
    """the lean k_shade (slot walk) and its emission pass; "light": the view that sees the light"""
    _ab(hk, knobs, SW._box(hk, size[0], size[1], view), 16, 3)


def test_queue_walk_and_general_matte_films(hk, knobs):
    for switch in (("HK_SHADE_SLOT_WALK", "0"), ("HK_SHADE_LEAN", "0")):
        _ab(hk, knobs, SW._box(hk, 37, 29, "light"), 16, 3, {"HK_DYNAMIC_SEGMENTS": "1", switch[0]: switch[1]})


def test_mix_scene_films(hk, knobs):
    """a Mix of Matte and Mirror on the sphere: the general k_shade of two kinds"""
    from hikari_jl_amd import scenes

    def build():
        mix = hk.MixMaterial((hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7, 0.3, 0.2)), hk.MirrorMaterial()), 0.4)
        return scenes.cornell_box(37, 29, objects="two_spheres", tess=8, object_material=mix)

    desc = build()[0].desc
    kinds = {desc.materials[i].kind for i in range(desc.n_materials)}
    assert hk._abi.HK_MAT_MIX in kinds and hk._abi.HK_MAT_MIRROR in kinds
    _ab(hk, knobs, build, 16, 3)


def test_media_scene_films(hk, knobs):
    """fog around matte surfaces: k_scatter and the general shading kernels behind the tracking kernels"""
    from hikari_jl_amd import scenes
    seen = []
    _ab(hk, knobs, lambda: scenes.integration_test_scene(37, 29, with_fog=True), 16, 3, {}, probe=lambda vp, st: seen.append(int(st.scatter_vertices)))
    assert seen[0] > 0


def test_one_sample_calls_films(hk, knobs):
    """one-sample calls on a small film: k_small_pass (no explicit HK_DYNAMIC_SEGMENTS, which would keep the stages)"""
    knobs.delenv("HK_DYNAMIC_SEGMENTS")
    fused = []
    _ab(hk, knobs, SW._box(hk, 37, 29, "light"), 1, 3, {}, probe=lambda vp, st: fused.append(int(st.fused_passes)), fused=True, calls=4)
    assert fused[0] > 0 and fused[1] > 0, fused


def test_many_lights_films(hk, knobs):
    """>= 64 lights in the light BVH: k_light_select_pool chooses the light (surface_at on its own) before the shade kernels"""
    from hikari_jl_amd import scenes
    seen = []
    build = lambda: scenes.many_light_scene(64, 48, n_boxes=400, box_scale=5.0)
    assert build()[0].desc.n_lights >= 64
    _ab(hk, knobs, build, 16, 3, probe=lambda vp, st: seen.append(int(st.select_launches)))
    assert seen[0] > 0 and seen[1] > 0, seen


def test_packed_scene_films(hk, knobs):
    """the same box with packed records (HK_TRI_PACK=1): the row comes from the record"""
    knobs.setenv("HK_TRI_PACK", "1")
    _ab(hk, knobs, SW._box(hk, 37, 29, "light"), 16, 3)
