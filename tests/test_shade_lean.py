"""The LEAN instantiation of k_shade<Matte> (hk_shade.h: shade_body): in a lean scene (all surfaces opaque, no media) whose state
holds the lean records, the record layouts, r_u == 1 and "no medium" are compile-time facts, the values of a vertex's second half wait
in LDS while the light is sampled, and the kernel runs at five waves per SIMD.  Every step only removes operations whose result is fixed
or moves values, so each case below is rendered at the default and under HK_SHADE_LEAN=0 (the general instantiation) and compared bit for
bit: film accumulators and the ray / vertex / light-BVH counters.

Small films on the staged path (no batching, no fused pass; an explicit HK_DYNAMIC_SEGMENTS keeps work lists and tickets or the static
stride for a film this size).  37 x 29 pads to 40 x 32 pixels: the last 64-chunk of a segment is ragged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("rays_closest", "rays_shadow", "hits_accepted", "path_vertices", "light_bvh_nodes")


def _render(hk, knobs, lean, build, spp, depth, env):
    knobs.setenv("HK_BATCH_PATHS_M", "0")
    knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    for k, v in env.items():
        knobs.setenv(k, v)
    if lean:
        knobs.delenv("HK_SHADE_LEAN")
    else:
        knobs.setenv("HK_SHADE_LEAN", "0")
    scene, film, cam = build()
    vp = hk.VolPath(max_depth=depth, samples=spp)
    try:
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        vp.render_samples(scene, film, cam, spp, readback=False)
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        return acc, tuple(int(getattr(st, n)) for n in COUNTERS)
    finally:
        vp.close()


def _compare(hk, knobs, build, spp, depth, env=None):
    env = {"HK_DYNAMIC_SEGMENTS": "1"} if env is None else env
    got = _render(hk, knobs, True, build, spp, depth, env)
    ref = _render(hk, knobs, False, build, spp, depth, env)
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0
    assert np.isfinite(got[0]).all() and got[0].max() > 0
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "film differs from HK_SHADE_LEAN=0"
    assert got[1] == ref[1], "counters %r != %r (HK_SHADE_LEAN=0)" % (got[1], ref[1])
    assert ref[1][0] > 0 and ref[1][3] > 0
    return got, ref


def _cornell(hk, w, h, lens=0.0, mirror=False):
    from hikari_jl_amd import scenes
    from hikari_jl_amd.materials import MirrorMaterial

    def build():
        s, film, _ = scenes.cornell_box(w, h, light="area", tess=8, object_material=MirrorMaterial() if mirror else None)
        cam = hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0, lens_radius=lens, focal_distance=3.5 if lens > 0 else 1e6)
        return s, film, cam
    return build


def _fog(hk, w, h):
    from hikari_jl_amd import scenes
    return lambda: scenes.integration_test_scene(w, h, with_fog=True)


@pytest.mark.parametrize("segments", ["1", "0"])
@pytest.mark.parametrize("spp", [16, 20])
def test_ragged_chunks(hk, knobs, spp, segments):
    """Cornell box, 37 x 29, depth 8: ragged last chunks, roulette from depth 4, emitter hits with and without MIS; tickets and the static stride."""
    _compare(hk, knobs, _cornell(hk, 37, 29), spp, 8, {"HK_DYNAMIC_SEGMENTS": segments})


@pytest.mark.parametrize("spp", [4, 64])
def test_draw_paths(hk, knobs, spp):
    """4 spp: no sample-bit table (the instantiation that hashes the digits); 64 spp: every draw a table load."""
    _compare(hk, knobs, _cornell(hk, 37, 29), spp, 8)


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_extremes(hk, knobs, depth):
    """max_depth 1: the second half of a vertex never runs, nothing is read back from the stash; max_depth 2: it runs once."""
    _compare(hk, knobs, _cornell(hk, 37, 29), 16, depth)


def test_thin_lens_against_pinhole(hk, knobs):
    """A thin-lens camera has no constant origin at depth 0; the pinhole has.  Both agree with the general kernel, and differ from each other."""
    lens, _ = _compare(hk, knobs, _cornell(hk, 37, 29, lens=0.05), 16, 8)
    pin, _ = _compare(hk, knobs, _cornell(hk, 37, 29), 16, 8)
    assert not np.array_equal(lens[0], pin[0])


def test_two_kinds(hk, knobs):
    """Matte plus mirror: the matte kernel is the first kind (counts from zero) and the mirror kernel continues from its counts."""
    _compare(hk, knobs, _cornell(hk, 37, 29, mirror=True), 16, 8)


def test_fallback_dispatch(hk, knobs):
    """A scene with a medium is not lean: the general kernel runs whatever the switch says."""
    _compare(hk, knobs, _fog(hk, 37, 29), 16, 8)


@pytest.mark.parametrize("segments", ["1", "0"])
def test_five_wave_grid(hk, knobs, segments):
    """20 segments per CU: every resident wave of the five-wave grid (5 blocks of 4 waves per CU) holds a segment."""
    _compare(hk, knobs, _cornell(hk, 64, 48), 64, 8, {"HK_DYNAMIC_SEGMENTS": segments, "HK_WAVES_PER_CU": "20"})
