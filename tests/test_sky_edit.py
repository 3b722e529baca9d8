"""A Hosek-Wilkie sky baked into an environment map on the device (hk_scene_update_envmap_sky, Scene.update_sky(build="device")).
What is checked, and how hard:
  texels   against the NumPy bake under the metric of sky_cases.py (ground and alpha equal, the bounds of sky_cases.check);
  tables   to the bit: a fresh scene from the READ-BACK texels has the edited scene's film and light samples, and the read-back tables
           are Distribution2D of the read-back texels — texels -> device tables -> sampling -> film without a tolerance;
  state    an update leaves what the last call alone leaves; rotation, sun record; ordering behind noted calls; the refusals.
The bounds and why there are three of them: sky_cases.py; the measurements: LAB_NOTEBOOK.md (the sky bake)."""
import ctypes as C

import numpy as np
import pytest

import sky_cases as SC

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 48, 32
KW = dict(max_depth=5, samples=4)
NEW = dict(direction=(-0.5, 0.3, 0.6), turbidity=4.2, ground_enabled=True)
THEN = dict(direction=(-0.5, 0.3, 0.6), turbidity=7.0, ground_enabled=True)


def _pf(hk, a):
    return a.ctypes.data_as(hk._abi.PF)


def _camera(hk, film):
    return hk.PerspectiveCamera((4.0, -5.0, 2.5), (0, 0, -0.3), film, up=(0, 0, 1), fov=40.0)


def _film(hk, s, spp=4, kw=KW):
    film = hk.Film((W, H))
    cam = _camera(hk, film)
    vp = hk.VolPath(**kw)
    vp._ensure(film)
    vp.clear()
    vp.render_samples(s, film, cam, spp, first=1, readback=False)
    acc = vp.read_accumulators(film).copy()
    vp.close()
    return acc


def _scene(hk, res, **kw):
    """test_light_edits.py's small sky scene with the baked sky: [EnvironmentLight, SunLight]"""
    from hikari_jl_amd import scenes
    return scenes.sky_scene(W, H, env_res=res, tess=16, **kw)[0]


def _fresh(hk, texels, like, rotation=None):
    """A scene created from texels ([v, u, 4]) and the lights of `like` as they are now."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap
    from hikari_jl_amd.materials import Gold
    s = hk.Scene()
    s.push(G.sphere((0, 0, 0), 1.0, 16), hk.GlassMaterial(Kr=hk.RGBSpectrum(1.0), Kt=hk.RGBSpectrum(1.0), index=1.5))
    s.push(G.rect3f((-2, -2, -1), (4, 4, 0.01)), Gold(roughness=0.01))
    s.push(EnvironmentLight(EnvironmentMap(texels, rotation), like.lights[0].scale_rgb))
    s.push(like.lights[1])                                       # the SunLight itself: its record is the one `like` holds
    s.sync()
    return s


def _map_scene(hk, data):
    """A slab under an environment map of any shape."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap
    s = hk.Scene()
    s.push(G.rect3f((-2, -2, -1), (4, 4, 0.01)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    s.push(EnvironmentLight(EnvironmentMap(data)))
    s.sync()
    return s


def _copy(hk, ctx, s, idx=0):
    """hk_scene_envmap_copy -> dict(texels [v, u, 4], conditional_func [v, u], conditional_cdf [v, u + 1], marginal_func, marginal_cdf, marginal_func_int)"""
    L = hk._lib.lib()
    sh = hk.scene_handle(ctx, s)
    w, h = C.c_int32(), C.c_int32()
    hk._lib.check(L.hk_scene_envmap_copy(sh, idx, C.byref(w), C.byref(h), None, None, None, None, None, None), "hk_scene_envmap_copy")
    w, h = w.value, h.value
    out = dict(texels=np.zeros((w, h, 4), f32), conditional_func=np.zeros((h, w), f32), conditional_cdf=np.zeros((h, w + 1), f32), marginal_func=np.zeros(h, f32),
               marginal_cdf=np.zeros(h + 1, f32), marginal_func_int=np.zeros(1, f32))
    hk._lib.check(L.hk_scene_envmap_copy(sh, idx, None, None, *[_pf(hk, out[k]) for k in ("texels", "conditional_func", "conditional_cdf", "marginal_func", "marginal_cdf",
                                                                                         "marginal_func_int")]), "hk_scene_envmap_copy")
    out["texels"] = np.ascontiguousarray(out["texels"].transpose(1, 0, 2))
    return out


def _same_copy(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _light(hk, ctx, s, mode, light_1based, n=1500, seed=4):
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


def _same_sky(hk, ctx, a, b):
    fa = _film(hk, a)
    assert np.array_equal(fa, _film(hk, b))
    env = a._flat_index(0) + 1
    assert b._flat_index(0) + 1 == env
    for mode in (0, 1):
        x, y = _light(hk, ctx, a, mode, env), _light(hk, ctx, b, mode, env)
        assert np.array_equal(x, y, equal_nan=True), mode
    return fa


# ---- 1. texels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", SC.RESOLUTIONS)
def test_device_texels_agree_with_the_numpy_bake(hk, gpu_ctx, res):
    """Every case of the parameter set at this resolution, one scene edited 40 times; ground and alpha equal; the bounds of sky_cases.check."""
    s = _scene(hk, res)
    hk.scene_handle(gpu_ctx, s)
    results, dark = [], []
    for c in (c for c in SC.CASES if c["res"] == res):
        s.update_sky(s.lights[0], **SC.sky_kwargs(hk, c))
        texels = _copy(hk, gpu_ctx, s)["texels"]
        results.append((c, SC.agreement(texels, c)))
        if SC.dark_family(c):
            dark.append((c, SC.agreement_with_host_build(texels, c)))
    assert s.lights[0].env_map._sky is not None                # nobody asked the host for its bake
    assert len(dark) == 4
    SC.check(results, dark, "device")


# ---- 2. tables, to the bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", SC.RESOLUTIONS)
def test_tables_sampling_and_film_are_those_of_the_read_back_texels(hk, gpu_ctx, res):
    from hikari_jl_amd.envmap import EnvironmentMap
    s = _scene(hk, res)
    hk.scene_handle(gpu_ctx, s)
    before = _film(hk, s)
    s.update_sky(s.lights[0], **NEW)
    got = _copy(hk, gpu_ctx, s)
    assert got["texels"].shape == (res, res, 4) and (got["texels"][..., :3] > 0).any()
    after = _same_sky(hk, gpu_ctx, s, _fresh(hk, got["texels"], s))
    assert not np.array_equal(before, after)
    D = EnvironmentMap(got["texels"]).distribution
    for k in ("conditional_func", "conditional_cdf", "marginal_func", "marginal_cdf"):
        assert np.array_equal(got[k], getattr(D, k)), k
    assert got["marginal_func_int"][0] == D.marginal_func_int
    assert s.lights[0].env_map._sky is not None                # all of that without the host bake


# ---- 3. no state -------------------------------------------------------------------------------------------------------------
def test_an_update_leaves_what_the_last_call_alone_leaves(hk, gpu_ctx):
    from hikari_jl_amd import sunsky
    from hikari_jl_amd.envmap import rotation_matrix
    res = 33
    one = _scene(hk, res)
    hk.scene_handle(gpu_ctx, one)
    one.update_sky(one.lights[0], **THEN)
    want = _copy(hk, gpu_ctx, one)
    # the sun moves, then the turbidity changes
    two = _scene(hk, res)
    hk.scene_handle(gpu_ctx, two)
    two.update_sky(two.lights[0], **dict(THEN, direction=(0.2, 0.7, 0.3), turbidity=NEW["turbidity"]))
    two.update_sky(two.lights[0], **dict(THEN, turbidity=NEW["turbidity"]))
    assert not _same_copy(_copy(hk, gpu_ctx, two), want)
    two.update_sky(two.lights[0], **THEN)
    assert _same_copy(_copy(hk, gpu_ctx, two), want)
    assert np.array_equal(_film(hk, two), _film(hk, one))
    # new texels after a sky: what update_envmap alone leaves; and a sky after new texels
    texels = np.random.default_rng(5).uniform(0.05, 2.0, (res, res, 3)).astype(f32)
    plain = _scene(hk, res)
    hk.scene_handle(gpu_ctx, plain)
    plain.update_envmap(plain.lights[0].env_map, data=texels)
    two.update_envmap(two.lights[0].env_map, data=texels)
    assert _same_copy(_copy(hk, gpu_ctx, two), _copy(hk, gpu_ctx, plain))
    assert np.array_equal(two.lights[0].env_map.data[..., :3], texels)           # the mirror holds the texels, not the sky it never baked
    plain.update_sky(plain.lights[0], **THEN)
    assert _same_copy(_copy(hk, gpu_ctx, plain), want)
    # a rotation set before survives
    R = rotation_matrix(70.0, (0.3, 0.2, 1.0))
    plain.update_envmap(plain.lights[0].env_map, rotation=R)
    plain.update_sky(plain.lights[0], **NEW)
    assert np.array_equal(plain.lights[0].env_map.rotation, R)
    turned = _copy(hk, gpu_ctx, plain)
    f = _same_sky(hk, gpu_ctx, plain, _fresh(hk, turned["texels"], plain, rotation=R))
    assert not np.array_equal(f, _film(hk, _fresh(hk, turned["texels"], plain)))
    # intensity and sun: the lights of a fresh sunsky_to_envlight scene
    env, sun = sunsky.sunsky_to_envlight(intensity=2.5, resolution=res, **NEW)
    one.update_sky(one.lights[0], intensity=2.5, sun=one.lights[1], **NEW)
    fresh = hk.Scene()
    fresh.push_light(env), fresh.push_light(sun)
    fresh.sync()
    assert one._stale_media == set() and one.lights[0].env_map._sky is not None
    kept = one._description(bake_skies=False)
    assert [bytes(kept.lights[i]) for i in range(2)] == [bytes(fresh.desc.lights[i]) for i in range(2)]
    _same_sky(hk, gpu_ctx, one, _fresh(hk, _copy(hk, gpu_ctx, one)["texels"], fresh))


def test_a_later_scene_holds_the_host_bake(hk, gpu_ctx):
    """The documented consequence: a scene created later from the kept description holds sky_texels — within the bound, not the bits."""
    from hikari_jl_amd import sunsky
    res = 33
    s = _scene(hk, res)
    hk.scene_handle(gpu_ctx, s)
    s.update_sky(s.lights[0], **NEW)
    dev = _copy(hk, gpu_ctx, s)["texels"]
    s.close()                                                    # the next handle is created from the kept description
    later = _copy(hk, gpu_ctx, s)["texels"]
    assert np.array_equal(later[..., :3], sunsky.sky_texels(resolution=res, **NEW)) and s.lights[0].env_map._sky is None
    top = later[..., :3].max(axis=2, keepdims=True).astype(np.float64)
    assert (np.abs(dev[..., :3].astype(np.float64) - later[..., :3])[top[..., 0] > 0] / top[top[..., 0] > 0]).max() <= 4 * SC.bounds()["device"]


# ---- 4. ordering -------------------------------------------------------------------------------------------------------------
def test_sky_edit_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the sky as it was when the call was made; the next one sees the new one."""
    res = 33
    probe = _scene(hk, res)
    hk.scene_handle(gpu_ctx, probe)
    probe.update_sky(probe.lights[0], **NEW)
    s_new = _fresh(hk, _copy(hk, gpu_ctx, probe)["texels"], probe)
    s, s_old = _scene(hk, res), _scene(hk, res)
    hk.scene_handle(gpu_ctx, s)

    def run(first, then, edit):
        film = hk.Film((W, H))
        cam = _camera(hk, film)
        vp = hk.VolPath(**KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)      # noted, not yet rendered
        if edit:
            s.update_sky(s.lights[0], **NEW)
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(s, s, True)
    assert np.array_equal(got, run(s_old, s_new, False))
    assert not np.array_equal(got, run(s_new, s_new, False)) and not np.array_equal(got, run(s_old, s_old, False))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refused_sky_edits_leave_the_scene_untouched(hk, gpu_ctx):
    from hikari_jl_amd import sunsky
    from hikari_jl_amd.envmap import Distribution2D
    A = hk._abi
    L = hk._lib.lib()
    s = _scene(hk, 16)
    sh = hk.scene_handle(gpu_ctx, s)
    state = lambda: (_film(hk, s).tobytes(), [v.tobytes() for v in _copy(hk, gpu_ctx, s).values()])
    before = state()
    good = lambda: sunsky.sky_params(**NEW)

    def refused(status, needle):
        assert status == A.HK_ERR_INVALID
        assert needle in L.hk_last_error(), L.hk_last_error()

    refused(L.hk_scene_update_envmap_sky(None, 0, C.byref(good())), b"hk_scene_update_envmap_sky: null scene")
    refused(L.hk_scene_update_envmap_sky(sh, 0, None), b"hk_scene_update_envmap_sky: null params")
    for idx in (1, -1):
        refused(L.hk_scene_update_envmap_sky(sh, idx, C.byref(good())), b"map index out of range")
    for bad in (np.nan, np.inf, -np.inf):
        for poison in (lambda p: p.sun_dir.__setitem__(1, bad), lambda p: p.ground_rgb.__setitem__(2, bad), lambda p: p.config[10].__setitem__(8, bad),
                       lambda p: p.config[0].__setitem__(0, bad), lambda p: p.radiance.__setitem__(10, bad), lambda p: p.xyz_weight[2].__setitem__(12, bad),
                       lambda p: p.xyz_weight[0].__setitem__(0, bad)):
            p = good()
            poison(p)
            refused(L.hk_scene_update_envmap_sky(sh, 0, C.byref(p)), b"non-finite entry")
    for scale in (0.0, 0.99, 1.01, 2.0):                          # squared lengths 0, 0.9801, 1.0201, 4
        p = good()
        p.sun_dir[:] = [scale * x for x in p.sun_dir]
        refused(L.hk_scene_update_envmap_sky(sh, 0, C.byref(p)), b"sun_dir is not a unit vector")
    for r in (1, -1):
        p = good()
        p.reserved = r
        refused(L.hk_scene_update_envmap_sky(sh, 0, C.byref(p)), b"reserved is not 0")
    refused(L.hk_scene_envmap_copy(None, 0, None, None, None, None, None, None, None, None), b"hk_scene_envmap_copy: null scene")
    refused(L.hk_scene_envmap_copy(sh, 1, None, None, None, None, None, None, None, None), b"hk_scene_envmap_copy: map index out of range")
    assert state() == before
    # a map that is not square; a map whose tables are of half its texels' resolution
    wide = _map_scene(hk, np.full((8, 16, 3), 0.5, f32))
    refused(L.hk_scene_update_envmap_sky(hk.scene_handle(gpu_ctx, wide), 0, C.byref(good())), b"the map is not square")
    assert np.array_equal(_copy(hk, gpu_ctx, wide)["texels"][..., :3], np.full((8, 16, 3), 0.5, f32))
    coarse = _map_scene(hk, np.full((8, 8, 3), 0.5, f32))
    D = Distribution2D(np.full((4, 4), 0.5, f32))
    rec = coarse.desc.envmaps[0]
    rec.nu = rec.nv = 4
    for name in ("conditional_func", "conditional_cdf", "conditional_func_int", "marginal_func", "marginal_cdf"):
        setattr(rec, name, _pf(hk, getattr(D, name)))
    ch = hk.scene_handle(gpu_ctx, coarse)
    refused(L.hk_scene_update_envmap_sky(ch, 0, C.byref(good())), b"tables are not of its texels' resolution")
    texels, table = np.zeros((8, 8, 4), f32), np.full(9 * 8, -7.0, f32)
    for k in range(4):                                           # a caller sizes its table buffers from width and height: refused, nothing written
        args = [None] * 4
        args[k] = _pf(hk, table)
        refused(L.hk_scene_envmap_copy(ch, 0, None, None, _pf(hk, texels), *args, None), b"hk_scene_envmap_copy: the map's tables are not of its texels' resolution")
    assert (table == -7.0).all() and not texels.any()
    hk._lib.check(L.hk_scene_envmap_copy(ch, 0, None, None, _pf(hk, texels), None, None, None, None, None), "hk_scene_envmap_copy")
    assert np.array_equal(texels[..., :3], np.full((8, 8, 3), 0.5, f32))
    # the same call with good arguments is accepted (the refusals above were about the arguments)
    assert L.hk_scene_update_envmap_sky(sh, 0, C.byref(good())) == 0
    assert state() != before
    # and Scene.update_sky raises before it calls
    with pytest.raises(ValueError):
        wide.update_sky(wide.lights[0], (0, 0, 1))
    with pytest.raises(ValueError):
        s.update_sky(s.lights[0], (0, 0, 0))
