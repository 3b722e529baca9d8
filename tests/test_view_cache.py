"""The view cache (hk_render.cpp): a one-pass frame whose camera records would be, value for value, those of the pass before it on the same
path state keeps them — k_camera writes a generation of its own (DPathState::gen_cam) that no bounce overwrites — and does not launch
k_camera.  Every sequence below is rendered twice, with the cache at its default and under HK_VIEW_CACHE=0, and compared frame by frame:
film accumulators and the ray / vertex / collision counters bit for bit, and hk_stats.view_cache_hits against what the sequence must give.

Small films with padding and both film_tile paths (37 x 29: 16 spp tiles the 64-slot steps, 64 spp is one pixel per step; the tile frames
render a range that is no multiple of 8), max_depth 3 (depth 1 rewrites generation 0), the staged path (no batching, no fused pass)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(37, 29), (64, 48)]
SPPS = [16, 64]
DEPTH = 3


def _counters(st):
    return tuple(int(getattr(st, n)) for n in ("rays_closest", "rays_shadow", "hits_accepted", "path_vertices", "medium_collisions",
                                                 "track_collisions", "shadow_collisions", "scatter_vertices", "light_bvh_nodes"))


class _Frame:
    """One frame of a sequence: which integrator, what to render, and an edit to make first."""

    def __init__(self, vp=0, moved=False, film=None, first=1, stride=1, n=None, tile=None, edit=None, expect_hit=None):
        self.vp, self.moved, self.film, self.first, self.stride, self.n, self.tile, self.edit, self.expect_hit = vp, moved, film, first, stride, n, tile, edit, expect_hit


def _play(hk, knobs, cache, build, frames, spp, vp_kw=None, timing=False):
    """build() -> (scene, film, camera(film, moved), extras); frames: [_Frame]; returns [(accumulators, counters, hits, stats)] per frame"""
    knobs.setenv("HK_BATCH_PATHS_M", "0")
    knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    if cache is True:
        knobs.delenv("HK_VIEW_CACHE")
    else:
        knobs.setenv("HK_VIEW_CACHE", cache or "0")      # ("2": the A/B variant that clears L with a memset on a hit)
    scene, film0, camera, extras = build()
    vps = {}
    out = []
    try:
        for f in frames:
            if f.edit is not None:
                f.edit(scene, extras)
            film = f.film if f.film is not None else film0
            cam = camera(film, f.moved)
            if f.vp not in vps:
                kw = dict(max_depth=DEPTH, samples=spp)
                kw.update((vp_kw or {}).get(f.vp, {}))
                vps[f.vp] = hk.VolPath(**kw)
                if timing:
                    vps[f.vp].enable_counters(time_kernels=True)
            vp = vps[f.vp]
            vp._ensure(film)
            vp.clear()
            vp.reset_stats()
            vp.render_samples(scene, film, cam, f.n if f.n is not None else spp, stride=f.stride, first=f.first, readback=False, tile=f.tile)
            acc = vp.read_accumulators(film).copy()
            st = vp.stats()
            out.append((acc, _counters(st), int(st.view_cache_hits), st))
    finally:
        for vp in vps.values():
            vp.close()
        if timing:
            hk.VolPath().enable_counters()      # (the context's flags: off again)
    return out


def _compare(hk, knobs, build, frames, spp, cache=True, **kw):
    """the sequence with the cache and without: equal frames, the expected hits with it, none without"""
    got = _play(hk, knobs, cache, build, frames, spp, **kw)
    ref = _play(hk, knobs, False, build, frames, spp, **kw)
    for i, (f, g, r) in enumerate(zip(frames, got, ref)):
        assert np.isfinite(r[0]).all() and r[0].max() > 0, i
        assert np.array_equal(g[0].view(np.uint32), r[0].view(np.uint32)), "frame %d: film differs from HK_VIEW_CACHE=0" % i
        assert g[1] == r[1], "frame %d: counters %r != %r" % (i, g[1], r[1])
        assert r[2] == 0, i
        if f.expect_hit is not None:
            assert g[2] == (1 if f.expect_hit else 0), "frame %d: view_cache_hits %d" % (i, g[2])
    return got, ref


def _box_camera(hk, lens=0.0):
    return lambda film, moved: hk.PerspectiveCamera((0.2, 1.1, -3.4) if moved else (0, 1, -3.5), (0, 1, 0), film, fov=40.0, lens_radius=lens,
                                                    focal_distance=3.5 if lens > 0 else 1e6)


def _cornell(hk, w, h, lens=0.0):
    from hikari_jl_amd import scenes

    def build():
        s, film, _ = scenes.cornell_box(w, h, light="area", tess=8)
        return s, film, _box_camera(hk, lens), None
    return build


def _sky(hk, w, h):
    from hikari_jl_amd import scenes

    def build():
        s, film, _ = scenes.sky_scene(w, h, env_res=32, tess=8)
        return s, film, (lambda film, moved: hk.PerspectiveCamera((3.5, -5.2, 2.8) if moved else (4.0, -5.0, 2.5), (0, 0, -0.3), film, up=(0, 0, 1), fov=40.0)), None
    return build


def _builders(hk, w, h):
    return {"cornell": _cornell(hk, w, h), "sky": _sky(hk, w, h), "thin_lens": _cornell(hk, w, h, lens=0.05)}


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("which", ["cornell", "sky", "thin_lens"])
def test_identical_frames_hit(hk, knobs, which, size, spp):
    """1. Three identical frames: the first generates the camera records, the two after it keep them."""
    frames = [_Frame(expect_hit=False), _Frame(expect_hit=True), _Frame(expect_hit=True)]
    got, _ = _compare(hk, knobs, _builders(hk, *size)[which], frames, spp)
    assert sum(g[2] for g in got) == 2
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], got[2][0])


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("which", ["cornell", "sky", "thin_lens"])
def test_changed_view_misses_then_hits(hk, knobs, which, spp):
    """2. Whatever the camera records depend on, changed between frames: the changed frame is a miss and correct, its repeat a hit.  Camera
    position, first sample, stride, count, tile rectangle, film size on the same integrator; the filter radius (an integrator of its own:
    the filter is part of hk_integrator_params) on the same context."""
    w, h = SIZES[0]
    w2, h2 = SIZES[1]
    other = hk.Film((w2, h2))
    frames = [_Frame(expect_hit=False), _Frame(expect_hit=True)]
    for kw in (dict(), dict(first=5), dict(first=5, stride=3), dict(first=5, stride=3, n=spp // 2 + 3), dict(tile=(3, 2, 30, 21)), dict(tile=(3, 2, 31, 21)),
               dict(film=other)):
        frames += [_Frame(moved=True, expect_hit=False, **kw), _Frame(moved=True, expect_hit=True, **kw)]
    frames += [_Frame(vp=1, expect_hit=False), _Frame(vp=1, expect_hit=True)]
    _compare(hk, knobs, _builders(hk, w, h)[which], frames, spp, vp_kw={1: dict(filter=hk.GaussianFilter(radius=(1.0, 1.0), sigma=0.5))})


def _edit_scene(hk, w, h):
    """the box of test_scene_edits with a movable sphere, a box with a material of its own and a point light"""
    from hikari_jl_amd import geometry as G

    def build():
        s = hk.Scene()
        white, red, green = (hk.MatteMaterial(Kd=hk.RGBSpectrum(*c)) for c in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15)))
        s.push(hk.PointLight((0.5, 1.6, -0.4), hk.RGBSpectrum(6.0, 5.0, 3.0)))
        s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), white)
        s.push(G.rect3f((-1, 1.99, -1), (2, 0.01, 2)), white)
        s.push(G.rect3f((-1, 0, 0.99), (2, 2, 0.01)), white)
        s.push(G.rect3f((-1, 0, -1), (0.01, 2, 2)), red)
        s.push(G.rect3f((0.99, 0, -1), (0.01, 2, 2)), green)
        q = G.quad((-0.25, 1.98, -0.25), (0.25, 1.98, -0.25), (0.25, 1.98, 0.25), (-0.25, 1.98, 0.25), normal=(0, -1, 0))
        s.push(q, hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(6.0))))
        sphere = s.push_instance(G.sphere((-0.4, 0.4, 0.0), 0.35, 8), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73)))
        slab = s.push_instance(G.rect3f((0.15, 0.0, -0.1), (0.5, 0.6, 0.5)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7, 0.2, 0.2)))
        s.sync()
        film = hk.Film((w, h))
        hk.scene_handle(hk.Context.get(0), s)      # created now: the edits below are the in-place ones
        return s, film, _box_camera(hk), dict(sphere=sphere, slab=slab)
    return build


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES)
def test_scene_edits_keep_the_cache_warm(hk, knobs, size, spp):
    """3. The camera records do not depend on the scene: after hk_scene_set_transform, a material update and a light update the next frame
    is a hit, and its film is the HK_VIEW_CACHE=0 render of the edited scene (which differs from the frame before the edit)."""
    move = np.eye(4, dtype=np.float32)
    move[:3, 3] = (0.2, 0.3, -0.1)
    frames = [_Frame(expect_hit=False),
              _Frame(edit=lambda s, x: s.set_transform(x["sphere"], move), expect_hit=True),
              _Frame(edit=lambda s, x: s.update_material(x["slab"].mi_idx, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.1, 0.3, 0.8))), expect_hit=True),
              _Frame(edit=lambda s, x: s.update_light(0, hk.PointLight((-0.5, 1.5, -0.3), hk.RGBSpectrum(2.0, 5.0, 7.0))), expect_hit=True)]
    got, _ = _compare(hk, knobs, _edit_scene(hk, *size), frames, spp)
    for a, b in zip(got, got[1:]):
        assert not np.array_equal(a[0], b[0])      # every edit shows


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("which", ["cornell", "sky"])
def test_two_pass_frames_never_hit(hk, knobs, which, spp):
    """4. A frame of two passes (samples_per_pass = spp / 2) overwrites the first pass's records with the second's: nothing is kept."""
    frames = [_Frame(expect_hit=False)] * 3
    got, _ = _compare(hk, knobs, _builders(hk, *SIZES[0])[which], frames, spp, vp_kw={0: dict(samples_per_pass=spp // 2)})
    assert sum(g[2] for g in got) == 0


@pytest.mark.parametrize("spp", SPPS)
def test_two_integrators_keep_their_own_keys(hk, knobs, spp):
    """5. Two integrators alternating on one context (different sample ranges): each hits on its own second frame and after."""
    frames = [_Frame(vp=0, expect_hit=False), _Frame(vp=1, first=3, expect_hit=False), _Frame(vp=0, expect_hit=True), _Frame(vp=1, first=3, expect_hit=True),
              _Frame(vp=0, expect_hit=True), _Frame(vp=1, first=3, expect_hit=True)]
    _compare(hk, knobs, _cornell(hk, *SIZES[0]), frames, spp)


@pytest.mark.parametrize("spp", SPPS)
def test_timed_frames_hit_and_report_finite_class_times(hk, knobs, spp):
    """6. With per-kernel timing on, frames hit all the same; the skipped camera leaves no event pair, the class times are finite and the
    `other` class still holds the film and the work lists."""
    frames = [_Frame(expect_hit=False), _Frame(expect_hit=True), _Frame(expect_hit=True)]
    got, _ = _compare(hk, knobs, _cornell(hk, *SIZES[1]), frames, spp, timing=True)
    for g in got:
        st = g[3]
        for name in ("seconds_trace", "seconds_shadow", "seconds_shade", "seconds_other", "seconds_total"):
            v = float(getattr(st, name))
            assert np.isfinite(v) and v > 0, (name, v)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("which", ["cornell", "sky", "thin_lens"])
def test_memset_clear_variant(hk, knobs, which, spp):
    """HK_VIEW_CACHE=2 (a hit clears L with one memset instead of k_film's zero stores): the same hits, the same films."""
    frames = [_Frame(expect_hit=False), _Frame(expect_hit=True), _Frame(moved=True, expect_hit=False), _Frame(moved=True, expect_hit=True)]
    _compare(hk, knobs, _builders(hk, *SIZES[0])[which], frames, spp, cache="2")

