"""Lights and environment maps edited in place on the device (hk_scene_update_lights, hk_scene_update_envmap).  The contract: after
an edit the device scene is, bit for bit, the scene hk_scene_create builds from the edited description — so every test edits one
scene after its creation, builds a second one FRESH from the edited description, and compares films, the light BVH (nodes and bit
trails), light selection and light sampling with np.array_equal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import xform_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 40, 32
KW = dict(max_depth=5, samples=4)


def _pf(hk, a):
    return a.ctypes.data_as(hk._abi.PF)


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _camera(hk, film):
    return hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0)


def _film(hk, s, spp=4, one_sample=False, kw=KW, camera=_camera):
    film = hk.Film((W, H))
    cam = camera(hk, film)
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


def _tree(hk, ctx, s):
    """(node count, nodes, bit trails) of the scene's light BVH in the host order (hk_scene_light_bvh_copy)."""
    L = hk._lib.lib()
    sh = hk.scene_handle(ctx, s)
    n = C.c_int32()
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), None, None), "hk_scene_light_bvh_copy")
    nodes = np.zeros(16 * max(n.value, 1), f32)
    trails = np.zeros(max(s.desc.n_lights, 1), np.uint32)
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), _pf(hk, nodes), trails.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_light_bvh_copy")
    return n.value, nodes.tobytes(), trails.tobytes()


def _select(hk, ctx, s, n=300, seed=2):
    """(light, pmf) the device's sampler picks at n random shading points, and the pmf of every light in turn (the device tables)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3)).astype(f32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[::4] = 0                                           # no normal: a medium point
    u = rng.random(n).astype(f32)
    query = (1 + np.arange(n) % max(s.desc.n_lights, 1)).astype(np.int32)
    li, pmf, qp = np.empty(n, np.int32), np.empty(n, f32), np.empty(n, f32)
    L = hk._lib.lib()
    hk._lib.check(L.hk_test_light_bvh(ctx.h, hk.scene_handle(ctx, s), n, _pf(hk, p), _pf(hk, nrm), _pf(hk, u), _pi(li), _pf(hk, pmf), _pi(query), _pf(hk, qp)), "hk_test_light_bvh")
    return li, pmf, qp


def _light(hk, ctx, s, mode, light_1based, n=400, seed=4):
    """hk_test_light: mode 0 samples the light from n random points, mode 1 evaluates an escaped ray (radiance + environment pdf)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(f32)
    x = rng.random((n, 3)).astype(f32)
    if mode == 1:
        x = rng.normal(size=(n, 3)).astype(f32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    lam = rng.uniform(360, 830, (n, 4)).astype(f32)
    out = np.zeros((n, 12), f32)
    hk._lib.check(hk._lib.lib().hk_test_light(ctx.h, hk.scene_handle(ctx, s), mode, light_1based, n, _pf(hk, p), _pf(hk, x), _pf(hk, lam), _pf(hk, out)), "hk_test_light")
    return out


def _same_scene(hk, ctx, a, b, **film_kw):
    fa, fb = _film(hk, a, **film_kw), _film(hk, b, **film_kw)
    assert np.array_equal(fa, fb)
    assert _tree(hk, ctx, a) == _tree(hk, ctx, b)
    for x, y in zip(_select(hk, ctx, a), _select(hk, ctx, b)):
        assert np.array_equal(x, y)
    return fa


def _fresh(build, edits):
    """The scene `build()` gives, with lights[i] replaced by edits[i](scene) BEFORE it is flattened: created from the edited description."""
    s = build()
    for i, make in edits.items():
        s.lights[i] = make(s)
    s.sync()
    return s


def _edited(hk, ctx, build, edits):
    s = build()
    hk.scene_handle(ctx, s)                                # created first: the edits are the in-place ones
    before = _film(hk, s)
    for i, make in edits.items():
        s.update_light(i, make(s))
    return s, before


def _cornell(hk, light, tess=12):
    from hikari_jl_amd import scenes
    return lambda: scenes.cornell_box(W, H, light=light, tess=tess)[0]


def test_point_light_moved_and_dimmed_equals_fresh(hk, gpu_ctx):
    edits = {0: lambda s: hk.PointLight((0.35, 1.4, -0.3), hk.RGBSpectrum(4.0, 3.0, 2.0))}
    build = _cornell(hk, "point")
    s, before = _edited(hk, gpu_ctx, build, edits)
    after = _same_scene(hk, gpu_ctx, s, _fresh(build, edits))
    assert not np.array_equal(before, after)
    assert np.array_equal(_film(hk, s, one_sample=True), _film(hk, _fresh(build, edits), one_sample=True))   # one-sample calls: the fused small pass


def _lamp_camera(hk, film):
    return hk.PerspectiveCamera((0, 0.3, 0), (0, 1.98, 0), film, up=(0, 0, 1), fov=50.0)


def test_area_light_recoloured_equals_fresh_and_direct_hits_show_it(hk, gpu_ctx):
    """Le * scale goes from 1 to (0.8, 0.4, 0.1): inside [0, 1], where the bounded uplift of an emitter's colour (Q3) does not clamp."""
    from hikari_jl_amd import lights as LT
    recolour = lambda i: (lambda s: LT.DiffuseAreaLight(s.lights[i].vertices, s.lights[i].normal, s.lights[i].area, s.lights[i].uv, hk.RGBSpectrum(1.6, 0.8, 0.2), 0.5, False))
    edits = {0: recolour(0), 1: recolour(1)}
    build = _cornell(hk, "area")
    s, before = _edited(hk, gpu_ctx, build, edits)
    f = _fresh(build, edits)
    after = _same_scene(hk, gpu_ctx, s, f)
    assert not np.array_equal(before, after)
    # a camera under the lamp looking up at it: the emission a path meets directly
    lamp_old = _film(hk, build(), camera=_lamp_camera)
    lamp_new = _film(hk, s, camera=_lamp_camera)
    assert np.array_equal(lamp_new, _film(hk, f, camera=_lamp_camera))
    n = W * H
    assert 0 < lamp_new[:3 * n].sum() < 0.7 * lamp_old[:3 * n].sum()
    for k in (1, 2):
        assert np.array_equal(_light(hk, gpu_ctx, s, 0, k), _light(hk, gpu_ctx, f, 0, k))


def test_spot_light_cone_and_matrices_equal_fresh(hk, gpu_ctx):
    edits = {0: lambda s: hk.SpotLight((0.6, 1.8, -0.7), (-0.2, 0.2, 0.2), hk.RGBSpectrum(10.0, 14.0, 18.0), 35.0, 10.0)}
    build = _cornell(hk, "spot")
    s, before = _edited(hk, gpu_ctx, build, edits)
    f = _fresh(build, edits)
    after = _same_scene(hk, gpu_ctx, s, f)
    assert not np.array_equal(before, after)
    a, b = _light(hk, gpu_ctx, s, 0, 1), _light(hk, gpu_ctx, f, 0, 1)
    assert np.array_equal(a, b) and (a[:, 4:8] > 0).any()


def _sky(hk):
    from hikari_jl_amd import scenes
    return lambda: scenes.sky_scene(W, H, env_res=32, tess=16, analytic=True)[0]


def _sky_camera(hk, film):
    return hk.PerspectiveCamera((4.0, -5.0, 2.5), (0, 0, -0.3), film, up=(0, 0, 1), fov=40.0)


def test_sun_and_sky_scale_equal_fresh(hk, gpu_ctx):
    """The infinite-light list only: both lights are infinite, the tree is empty before and after."""
    from hikari_jl_amd.envmap import EnvironmentLight
    from hikari_jl_amd.lights import SunLight
    edits = {0: lambda s: EnvironmentLight(s.lights[0].env_map, hk.RGBSpectrum(3e-4, 2e-4, 1e-4)),
             1: lambda s: SunLight.from_rgb((2.0, 3.0, 4.5), (-3.0, 1.0, -5.0))}
    build = _sky(hk)
    s = build()
    hk.scene_handle(gpu_ctx, s)
    kw = dict(camera=_sky_camera, kw=dict(max_depth=6, samples=4))
    before = _film(hk, s, **kw)
    for i, make in edits.items():
        s.update_light(i, make(s))
    f = _fresh(build, edits)
    after = _same_scene(hk, gpu_ctx, s, f, **kw)
    assert not np.array_equal(before, after)
    assert _tree(hk, gpu_ctx, s)[0] == 0
    for k in (1, 2):
        assert np.array_equal(_light(hk, gpu_ctx, s, 0, k), _light(hk, gpu_ctx, f, 0, k))
    assert np.array_equal(_light(hk, gpu_ctx, s, 1, 1), _light(hk, gpu_ctx, f, 1, 1))


POINTS = [((-0.5, 1.5, -0.3), 3.0), ((0.5, 1.2, 0.2), 9.0), ((0.0, 0.6, -0.6), 5.0)]   # (position, power): the second is the largest


def _three_points(hk, powers):
    def build():
        s = _cornell(hk, "none")()
        for (pos, _), w in zip(POINTS, powers):
            s.push(hk.PointLight(pos, hk.RGBSpectrum(w)))
        s.sync()
        return s
    return build


def test_lights_leave_and_enter_the_tree(hk, gpu_ctx):
    full = [w for _, w in POINTS]
    steps = [[3.0, 0.0, 5.0], full, [0.0, 0.0, 0.0], full, [0.0, 0.0, 5.0]]   # the largest leaves, comes back; the tree empties, refills; one light alone
    s = _three_points(hk, full)()
    hk.scene_handle(gpu_ctx, s)
    assert _tree(hk, gpu_ctx, s)[0] == 5
    have = list(full)
    for powers in steps:
        for i, w in enumerate(powers):
            if w != have[i]:
                s.update_light(i, hk.PointLight(POINTS[i][0], hk.RGBSpectrum(w)))
        have = list(powers)
        f = _three_points(hk, powers)()
        film = _same_scene(hk, gpu_ctx, s, f)
        lit = sum(1 for w in powers if w > 0)
        assert _tree(hk, gpu_ctx, s)[0] == max(2 * lit - 1, 0)
        assert (film[:3 * W * H].max() > 0) == (lit > 0)
        assert np.array_equal(_film(hk, s, one_sample=True), _film(hk, f, one_sample=True))


def _strips(n, x0, y):
    """n small downward-facing triangles in a row under the ceiling."""
    P = np.zeros((n, 3, 3), f32)
    for i in range(n):
        x = x0 + 0.05 * i
        P[i] = [(x, y, -0.1 + 0.002 * i), (x + 0.04, y, -0.1), (x + 0.04, y, 0.1 + 0.003 * i)]
    return P


def test_deep_tree_recoloured_and_moved_equals_fresh(hk, gpu_ctx):
    """hk::preselect_lights is true from HK_PRESELECT_MIN = 64 lights in the tree (hk_shade.h; no media): k_light_select then
    chooses the next-event light.  64 emissive triangles in two meshes (40 + 24, so the moved lights are a contiguous run that is not
    the whole set); every third emitter re-coloured, the second mesh moved with its lights."""
    from hikari_jl_amd import lights as LT
    from hikari_jl_amd.geometry import Mesh
    src = open(os.path.join(ROOT, "hikari.jl_amd", "csrc", "hk_shade.h")).read()
    assert re.search(r"#define HK_PRESELECT_MIN (\d+)", src).group(1) == "64"
    em = lambda: hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(5.0), scale=1.0, two_sided=True))
    A_, B_ = _strips(40, -0.95, 1.9), _strips(24, -0.6, 1.6)
    M = X.affine(rot_deg=25, axis=(0.1, 1, 0.2), scale=1.1, translate=(0.05, -0.4, 0.1))
    recolour = lambda l, i: LT.DiffuseAreaLight(l.vertices, l.normal, l.area, l.uv, hk.RGBSpectrum(0.2 + 0.01 * i, 0.9, 0.5), 0.8, i % 2 == 0)
    s = _cornell(hk, "none")()
    s.push_instance(Mesh(A_, None, None), em())
    inst = s.push_instance(Mesh(B_, None, None), em())
    s.sync()
    assert s.desc.n_lights == 64
    hk.scene_handle(gpu_ctx, s)
    before = _film(hk, s)
    for i in range(0, 64, 3):
        s.update_light(i, recolour(s.lights[i], i))
    s.set_transform(inst, M, move_lights=True)
    f = _cornell(hk, "none")()
    f.push(Mesh(A_, None, None), em())
    f.push(Mesh(X.transform_points(M[:3], B_), None, None), em())
    for i in range(0, 64, 3):                              # the lights stated explicitly
        f.lights[i] = recolour(f.lights[i], i)
    f.sync()
    after = _same_scene(hk, gpu_ctx, s, f)
    assert not np.array_equal(before, after)
    assert _tree(hk, gpu_ctx, s)[0] == 127
    assert np.array_equal(_film(hk, s, one_sample=True), _film(hk, f, one_sample=True))


def test_light_edit_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the lights as they were when the call was made; the next one sees the new ones."""
    old = [w for _, w in POINTS]
    new_light = lambda: hk.PointLight((0.2, 1.7, 0.4), hk.RGBSpectrum(0.0, 12.0, 2.0))
    s = _three_points(hk, old)()
    s_old = _three_points(hk, old)()
    s_new = _three_points(hk, old)()
    s_new.lights[1] = new_light()
    s_new.sync()
    hk.scene_handle(gpu_ctx, s)

    def run(first, then, edit):
        film = hk.Film((W, H))
        cam = _camera(hk, film)
        vp = hk.VolPath(**KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)      # noted, not yet rendered
        if edit:
            s.update_light(1, new_light())
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(s, s, True)
    assert np.array_equal(got, run(s_old, s_new, False))
    assert not np.array_equal(got, run(s_new, s_new, False)) and not np.array_equal(got, run(s_old, s_old, False))


def _env_scene(hk, data, rotation=None, scale=1.0):
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap
    s = hk.Scene()
    s.push(G.rect3f((-2, -2, -1), (4, 4, 0.01)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    s.push(G.sphere((0, 0, 0), 1.0, 12), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6, 0.7, 0.8)))
    em = EnvironmentMap(data, rotation)
    s.push(EnvironmentLight(em, hk.RGBSpectrum(scale)))
    s.sync()
    return s, em


def _map(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    d = (0.05 + rng.random((h, w, 3)) * np.array([1.0, 2.0, 4.0])).astype(f32)
    d[h // 3, w // 2] = 50.0                               # a hot texel: importance sampling matters
    if kind == "zero_row":
        d[h // 2] = 0.0
    if kind == "black":
        d[:] = 0.0
    return d


@pytest.mark.parametrize("kind", ["random", "zero_row", "black"])
@pytest.mark.parametrize("w,h", [(16, 8), (37, 19), (130, 70)])   # small; odd sizes; more rows than a wave and more than 64 columns
def test_envmap_tables_built_on_the_device_equal_the_host_tables(hk, gpu_ctx, w, h, kind):
    """New texels through hk_scene_update_envmap: the device builds conditional / marginal func, cdf and integrals itself.  The fresh
    scene's tables come from envmap.py.  The film reads the map through sampling (cdf tables) and through escaped rays' MIS (func,
    integrals); hk_test_light mode 0 samples it from random u (both cdf tables, the pdf), mode 1 evaluates escaped rays (pdf)."""
    old, new = _map("random", w, h, 1), _map(kind, w, h, 2)
    s, em = _env_scene(hk, old)
    hk.scene_handle(gpu_ctx, s)
    kw = dict(camera=_sky_camera)
    before = _film(hk, s, **kw)
    s.update_envmap(em, data=new)
    f, _ = _env_scene(hk, new)
    after = _film(hk, s, **kw)
    assert np.array_equal(after, _film(hk, f, **kw))
    assert not np.array_equal(before, after)
    for mode in (0, 1):
        a, b = _light(hk, gpu_ctx, s, mode, 1, n=2000), _light(hk, gpu_ctx, f, mode, 1, n=2000)
        assert np.array_equal(a, b, equal_nan=True), mode
    if kind != "black":
        assert (a[:, 4] > 0).any() and (_light(hk, gpu_ctx, s, 0, 1, n=2000)[:, 3] > 0).any()


def test_envmap_rotation_only_equals_fresh(hk, gpu_ctx):
    from hikari_jl_amd.envmap import rotation_matrix
    data = _map("random", 37, 19, 5)
    R = rotation_matrix(70.0, (0.3, 0.2, 1.0))
    s, em = _env_scene(hk, data)
    hk.scene_handle(gpu_ctx, s)
    kw = dict(camera=_sky_camera)
    before = _film(hk, s, **kw)
    s.update_envmap(em, rotation=R)
    f, _ = _env_scene(hk, data, R)
    after = _film(hk, s, **kw)
    assert np.array_equal(after, _film(hk, f, **kw)) and not np.array_equal(before, after)
    for mode in (0, 1):
        assert np.array_equal(_light(hk, gpu_ctx, s, mode, 1), _light(hk, gpu_ctx, f, mode, 1))
    # texels, then a rotation alone: the record keeps the integral the device wrote into it
    new = _map("zero_row", 37, 19, 6)
    s.update_envmap(em, data=new)
    R2 = rotation_matrix(-20.0, (1.0, 0.0, 0.2))
    s.update_envmap(em, rotation=R2)
    f2, _ = _env_scene(hk, new, R2)
    assert np.array_equal(_film(hk, s, **kw), _film(hk, f2, **kw))
    for mode in (0, 1):
        assert np.array_equal(_light(hk, gpu_ctx, s, mode, 1), _light(hk, gpu_ctx, f2, mode, 1))


def test_refused_light_edits_leave_the_scene_untouched(hk, gpu_ctx):
    A = hk._abi
    L = hk._lib.lib()
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap
    s = _cornell(hk, "both")()                               # a point light and the two triangles of the lamp
    em = EnvironmentMap(_map("random", 16, 8, 3))
    s.push(EnvironmentLight(em, hk.RGBSpectrum(0.2)))
    s.sync()
    sh = hk.scene_handle(gpu_ctx, s)
    d = s.desc
    kinds = [d.lights[i].kind for i in range(d.n_lights)]
    assert kinds == [A.HK_LIGHT_POINT, A.HK_LIGHT_DIFFUSE_AREA, A.HK_LIGHT_DIFFUSE_AREA, A.HK_LIGHT_ENVIRONMENT] and d.n_textures == 0 and d.n_envmaps == 1
    state = lambda: (_film(hk, s).tobytes(), _tree(hk, gpu_ctx, s), [x.tobytes() for x in _select(hk, gpu_ctx, s)], _light(hk, gpu_ctx, s, 1, 4).tobytes())
    before = state()
    rec = lambda i: A.hk_light.from_buffer_copy(d.lights[i])

    def refused(status, needle):
        assert status == A.HK_ERR_INVALID
        assert needle in L.hk_last_error(), L.hk_last_error()

    ok = rec(0)
    ok.i_rgb[0] = 99.0
    refused(L.hk_scene_update_lights(None, 0, 1, C.byref(ok)), b"null argument")
    refused(L.hk_scene_update_lights(sh, 0, 1, None), b"null argument")
    refused(L.hk_scene_update_lights(sh, 4, 1, C.byref(ok)), b"range outside")
    refused(L.hk_scene_update_lights(sh, -1, 1, C.byref(ok)), b"range outside")
    refused(L.hk_scene_update_lights(sh, 3, 2, (A.hk_light * 2)(rec(3), rec(3))), b"range outside")
    refused(L.hk_scene_update_lights(sh, 0, 0, C.byref(ok)), b"range outside")
    r = rec(0); r.kind = A.HK_LIGHT_SPOT
    refused(L.hk_scene_update_lights(sh, 0, 1, C.byref(r)), b"kind differs")
    r = rec(1); r.kind = A.HK_LIGHT_POINT
    refused(L.hk_scene_update_lights(sh, 1, 1, C.byref(r)), b"kind differs")
    for bad in (1, -1):
        r = rec(3); r.envmap = bad
        refused(L.hk_scene_update_lights(sh, 3, 1, C.byref(r)), b"missing envmap")
    r = rec(2); r.Le.tex = 0
    refused(L.hk_scene_update_lights(sh, 2, 1, C.byref(r)), b"Le texture index")
    two = (A.hk_light * 2)(rec(0), rec(1))                   # a two-record update whose second record is bad changes neither
    two[0].i_rgb[0] = 99.0
    two[1].kind = A.HK_LIGHT_SPOT
    refused(L.hk_scene_update_lights(sh, 0, 2, two), b"light 1: the kind differs")
    texels = np.ascontiguousarray(_map("random", 16, 8, 9).transpose(1, 0, 2))
    texels = np.concatenate([texels, np.ones((16, 8, 1), f32)], axis=2).copy()
    R = np.eye(3, dtype=f32)
    refused(L.hk_scene_update_envmap(None, 0, _pf(hk, texels), _pf(hk, R)), b"null scene")
    refused(L.hk_scene_update_envmap(sh, 0, None, None), b"neither texels nor a rotation")
    refused(L.hk_scene_update_envmap(sh, 1, _pf(hk, texels), None), b"map index out of range")
    refused(L.hk_scene_update_envmap(sh, -1, None, _pf(hk, R)), b"map index out of range")
    for bad in (np.inf, np.nan):
        Rb = R.copy()
        Rb[1, 2] = bad
        refused(L.hk_scene_update_envmap(sh, 0, _pf(hk, texels), _pf(hk, Rb)), b"non-finite rotation")
    assert state() == before
    # the same calls with good arguments are accepted (the refusals above were about the arguments)
    assert L.hk_scene_update_lights(sh, 0, 1, C.byref(ok)) == 0
    assert L.hk_scene_update_envmap(sh, 0, _pf(hk, texels), _pf(hk, R)) == 0
    assert state() != before
