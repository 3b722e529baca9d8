"""How k_shade finds the emissive hits of a segment (hk_shade.h: shade_body).  The trace kernels put the flag "this hit sits on an
area light" into the top bit of the kind-queue entry (HK_MATQ_EMISSIVE); the shading wave gathers the flagged entries from the queue
load its main pass makes anyway and runs the dense emission pass whenever 64 of them wait, and once more after the segment's last
chunk.  HK_SHADE_PRESCAN=1 brings back the scan of mat_id over the whole queue before the first vertex.  Either way the same additions
reach the same L entries.  The LEAN instantiation also stages the next chunk's hit, ray_d and meta word in LDS (global->LDS loads issued
from the middle of a chunk through a queue entry requested a chunk earlier); HK_SHADE_PREFETCH=0 loads them directly.  Every case is
rendered four ways — the default, HK_SHADE_PRESCAN=1, HK_SHADE_PREFETCH=0 and HK_SHADE_LEAN=0 (the general instantiation) — and
compared bit for bit: film accumulators and the ray / vertex / light-BVH counters.

Small films on the staged path (no batching, no fused pass; an explicit HK_DYNAMIC_SEGMENTS keeps work lists and tickets or the static
stride for a film this size).  37 x 29 pads to 40 x 32 pixels: the last 64-chunk of a segment is ragged."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("rays_closest", "rays_shadow", "hits_accepted", "path_vertices", "light_bvh_nodes")
WAYS = (("HK_SHADE_PRESCAN", "1"), ("HK_SHADE_PREFETCH", "0"), ("HK_SHADE_LEAN", "0"))
HK_MAT_MATTE = 0


def _queue_counts(hk, vp, depth, kind=HK_MAT_MATTE, flagged=False):
    """Entries of the kind's shading queue per wave segment at bounce `depth` of the last pass (hk_test_queue_counts); flagged: also how
    many of them carry the emissive flag (`depth` must then be the last bounce the pass traced)."""
    L = hk._lib.lib()
    n = C.c_int32(0)
    PI = C.POINTER(C.c_int32)
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), None, None), "hk_test_queue_counts")
    out, fl = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), out.ctypes.data_as(PI), fl.ctypes.data_as(PI) if flagged else None), "hk_test_queue_counts")
    return (out, fl) if flagged else out


def _render(hk, knobs, build, spp, depth, env, switch=None, probe=None, fused=False):
    knobs.setenv("HK_BATCH_PATHS_M", "0")
    if fused:
        knobs.delenv("HK_SMALL_PASS_FUSED")
    else:
        knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    for k, v in env.items():
        knobs.setenv(k, v)
    for k, _ in WAYS:
        knobs.delenv(k)
    if switch is not None:
        knobs.setenv(*switch)
    scene, film, cam = build()   # (a film counts the samples it has received: every render gets a fresh one)
    vp = hk.VolPath(max_depth=depth, samples=spp)
    try:
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        vp.render_samples(scene, film, cam, spp, readback=False)
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        if probe is not None:
            probe(vp)
        return acc, tuple(int(getattr(st, n)) for n in COUNTERS)
    finally:
        vp.close()


def _compare(hk, knobs, build, spp, depth, env=None, ways=WAYS, probe=None):
    env = {"HK_DYNAMIC_SEGMENTS": "1"} if env is None else env
    ref = _render(hk, knobs, build, spp, depth, env, probe=probe)
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0
    assert ref[1][0] > 0 and ref[1][3] > 0
    for switch in ways:
        got = _render(hk, knobs, build, spp, depth, env, switch)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "film differs under %s=%s" % switch
        assert got[1] == ref[1], "counters %r != %r under %s=%s" % ((got[1], ref[1]) + switch)
    return ref


def _cornell(hk, w, h, lens=0.0, mirror=False):
    from hikari_jl_amd import scenes
    from hikari_jl_amd.materials import MirrorMaterial

    def build():
        s, film, _ = scenes.cornell_box(w, h, light="area", tess=8, object_material=MirrorMaterial() if mirror else None)
        cam = hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0, lens_radius=lens, focal_distance=3.5 if lens > 0 else 1e6)
        return s, film, cam
    return build


def _panel(hk, w, h):
    """The Cornell box with a large one-sided quad light that also reflects (Kd 0.5) one unit in front of the camera, covering most of
    the view but not all of it: nearly every depth-0 vertex is an emissive hit that still samples a light and continues."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd import scenes
    from hikari_jl_amd.materials import Emissive, MatteMaterial, MediumInterface, RGBSpectrum

    def build():
        s, film, cam = scenes.cornell_box(w, h, light="area", tess=8)
        z = -2.5
        q = G.quad((-0.22, 0.55, z), (-0.22, 1.45, z), (0.4, 1.45, z), (0.4, 0.55, z), normal=(0, 0, -1))
        s.push(q, MediumInterface(MatteMaterial(Kd=RGBSpectrum(0.5)), emission=Emissive(Le=RGBSpectrum(0.6, 0.5, 0.4), scale=1.0, two_sided=False)))
        s.sync()
        return s, film, cam
    return build


def _open_stage(hk, w, h):
    """A floor, a back wall, a matte and a mirror sphere under the Cornell quad light, nothing else: about half of the paths escape
    at every bounce, so the matte queue of a 128-path segment holds anything from a few entries to all 128."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.film import Film
    from hikari_jl_amd.materials import Emissive, MatteMaterial, MediumInterface, MirrorMaterial, RGBSpectrum
    from hikari_jl_amd.scene import Scene

    def build():
        white = MatteMaterial(Kd=RGBSpectrum(0.73, 0.73, 0.73))
        s = Scene()
        s.push(G.rect3f((-1.0, 0, -1.0), (2.0, 0.01, 2.0)), white)
        s.push(G.rect3f((-1.0, 0, 0.99), (2.0, 2.0, 0.01)), white)
        s.push(G.sphere((-0.4, 0.4, 0.0), 0.35, 8), white)
        s.push(G.sphere((0.4, 0.35, 0.0), 0.3, 8), MirrorMaterial())
        y = 1.98
        q = G.quad((-0.25, y, -0.25), (0.25, y, -0.25), (0.25, y, 0.25), (-0.25, y, 0.25), normal=(0, -1, 0))
        s.push(q, MediumInterface(MatteMaterial(Kd=RGBSpectrum(0.0)), emission=Emissive(Le=RGBSpectrum(1.0), scale=1.0, two_sided=False)))
        s.sync()
        film = Film((w, h))
        return s, film, hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0)
    return build


@pytest.mark.parametrize("segments", ["1", "0"])
@pytest.mark.parametrize("spp", [16, 64])
@pytest.mark.parametrize("depth", [3, 1])
@pytest.mark.parametrize("size", [(37, 29), (64, 48)])
def test_cornell(hk, knobs, size, depth, spp, segments):
    """Cornell box with the area light: ragged and whole last chunks, with and without a continuation record (max_depth 1: the second
    half of a vertex never runs), 16 and 64 samples, tickets and the static stride."""
    _compare(hk, knobs, _cornell(hk, *size), spp, depth, {"HK_DYNAMIC_SEGMENTS": segments})


@pytest.mark.parametrize("size,spp", [((37, 29), 16), ((64, 48), 16)])
def test_emitter_fills_the_view(hk, knobs, size, spp):
    """One segment per CU (HK_WAVES_PER_CU=1): a segment holds 128 (37 x 29) or 192 (64 x 48) depth-0 vertices, most of them on the
    reflecting panel light.  The list is emptied at 64 inside the loop, part of a chunk's flagged entries waits for the next, and the
    rest goes after the last chunk; the flagged vertices cast their shadow rays and continue like any other."""
    seen = {}

    def probe(vp):
        seen["n"] = _queue_counts(hk, vp, 0)

    env = {"HK_DYNAMIC_SEGMENTS": "1", "HK_WAVES_PER_CU": "1"}
    ref = _compare(hk, knobs, _panel(hk, *size), spp, 3, env, probe=probe)
    assert seen["n"].max() > 64, seen["n"].max()       # more than one chunk in a segment
    # the flags of the depth-0 entries, from a pass that traces depth 0 only (the same camera paths; every bounce overwrites the queue)
    _render(hk, knobs, _panel(hk, *size), spp, 1, env, probe=lambda vp: seen.update(zip(("n1", "flagged"), _queue_counts(hk, vp, 0, flagged=True))))
    assert np.array_equal(seen["n1"], seen["n"])
    assert seen["flagged"].max() > 64, seen["flagged"].max()                       # the list is emptied inside the loop
    assert any(f > 64 and f % 64 for f in seen["flagged"]), seen["flagged"].max()  # and a rest goes after the last chunk
    assert (seen["flagged"] < seen["n"]).any()                                     # chunks that mix flagged and plain entries
    assert ref[1][1] > 0 and ref[1][4] > 0             # shadow rays were cast; the emission pass walked the light BVH for its MIS weight


def test_segment_sizes_around_the_chunk(hk, knobs):
    """Segments of 0, fewer than 64, exactly 64, 65 and 128 entries of the matte kind in one render.  64 x 32 pixels x 64 samples over
    four segments per CU of 256 CUs give every segment 128 camera paths (two pixels); in the open stage about half of a segment's
    paths escape per bounce and the mirror sphere takes others, so the matte queue sizes of bounces 0 - 2 spread over the whole
    range.  The sizes come from hk_test_queue_counts on this very render, and the test insists that the five it is about occurred."""
    sizes = set()

    def probe(vp):
        for d in range(3):
            sizes.update(int(c) for c in _queue_counts(hk, vp, d))

    _compare(hk, knobs, _open_stage(hk, 64, 32), 64, 3, {"HK_DYNAMIC_SEGMENTS": "1", "HK_WAVES_PER_CU": "4"}, probe=probe)
    assert {0, 64, 65, 128} <= sizes and any(0 < c < 64 for c in sizes), sorted(sizes)


def test_fused_small_pass(hk, knobs):
    """A call of four samples on a small film is one k_small_pass launch: its trace stage writes the flagged entries, its shade stage
    (the general body) reads them.  Default against HK_SHADE_PRESCAN=1."""
    env, fused = {}, []

    def probe(vp):
        fused.append(int(vp.stats().fused_passes))

    ref = _render(hk, knobs, _cornell(hk, 37, 29), 4, 3, env, probe=probe, fused=True)
    got = _render(hk, knobs, _cornell(hk, 37, 29), 4, 3, env, ("HK_SHADE_PRESCAN", "1"), probe=probe, fused=True)
    assert fused[0] > 0 and fused[1] > 0, fused
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0 and ref[1][3] > 0
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and got[1] == ref[1]


def test_two_kinds(hk, knobs):
    """Matte plus mirror: the mirror kernel is not the first kind of its launch and takes the general body; a segment's generation
    holds entries of both kinds."""
    _compare(hk, knobs, _cornell(hk, 37, 29, mirror=True), 16, 3)


def test_thin_lens(hk, knobs):
    """A thin-lens camera: depth-0 origins are stored per path (the pinhole stores one per segment)."""
    _compare(hk, knobs, _cornell(hk, 37, 29, lens=0.05), 16, 3)


def test_hashing_instantiation(hk, knobs):
    """HK_SOBOL_TABLE_ONLY=0: the instantiation with the digit-hashing fallback in it."""
    _compare(hk, knobs, _cornell(hk, 37, 29), 16, 3, {"HK_DYNAMIC_SEGMENTS": "1", "HK_SOBOL_TABLE_ONLY": "0"})


def test_preselected_lights(hk, knobs):
    """150 emissive boxes, 1800 area lights in the light BVH (HK_PRESELECT_MIN is 64): k_light_select_pool reads the flagged queue before
    the shade kernels do, and so does the per-lane kernel under HK_SELECT_POOL=0."""
    from hikari_jl_amd import scenes
    build = lambda: scenes.many_light_scene(37, 29, n_boxes=600, emissive_frac=0.25, box_scale=8.0)
    ref = _compare(hk, knobs, build, 16, 3, ways=WAYS[:1])
    assert ref[1][4] > 0
    _compare(hk, knobs, build, 16, 3, {"HK_DYNAMIC_SEGMENTS": "1", "HK_SELECT_POOL": "0"}, ways=WAYS[:1])


@pytest.mark.parametrize("grey", [True, False])
def test_medium(hk, knobs, grey):
    """A slab of fog in front of a large emitter, a second emitter inside the fog: the general k_trace flags the entries of rays that
    travel outside the medium, the tracking kernels those of the hits that survive the fog (grey: the compact kernels; chromatic:
    the general one).  The general shade body masks and uses the flag."""
    from hikari_jl_amd import scenes
    from hikari_jl_amd.materials import RGBSpectrum
    from hikari_jl_amd.media import HomogeneousMedium
    ss = RGBSpectrum(0.5) if grey else RGBSpectrum(0.7, 0.5, 0.3)
    build = lambda: scenes.slab_scene(37, 29, medium=HomogeneousMedium(sigma_a=RGBSpectrum(0.05), sigma_s=ss, Le=RGBSpectrum(0.0), g=0.2), inner_emitter=True)
    _compare(hk, knobs, build, 16, 4, ways=WAYS[:1])
