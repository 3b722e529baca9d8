"""k_shade's slot walk (hk_shade.h: shade_body<.., LEAN, SLOTS>).  In a lean scene whose material records are all of one kind the
kind queue sorts nothing: the LEAN k_shade walks a segment's generation itself, slot = seg + i for every ray of the generation, and
skips the entries whose ray escaped — the single-kind flush of k_trace_lean leaves HK_MAT_ESCAPED in their mat_id word.  Per path
nothing changes, only the order in which a wave meets its vertices; so every case is rendered five ways — the default (slot walk),
HK_SHADE_SLOT_WALK=0, HK_SHADE_PREFETCH=0 (slot walk without the fetch-ahead), HK_SHADE_PRESCAN=1 and HK_SHADE_LEAN=0 (both: queue
walk) — and compared bit for bit: film accumulators and the ray / vertex / hit counters.

Small films on the staged path (no batching, no fused pass; an explicit HK_DYNAMIC_SEGMENTS keeps work lists and tickets or the static
stride for a film this size), as in test_shade_chunks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_leaf_steps as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hikari.jl_amd", "csrc")
gpu = pytest.mark.gpu

COUNTERS = ("rays_closest", "rays_shadow", "hits_accepted", "path_vertices", "light_bvh_nodes")
WAYS = (("HK_SHADE_SLOT_WALK", "0"), ("HK_SHADE_PREFETCH", "0"), ("HK_SHADE_PRESCAN", "1"), ("HK_SHADE_LEAN", "0"))
HK_MAT_MATTE = 0
RAYS, ESCAPED = -1, -2   # hk_test_queue_counts: the generation's rays, and those of them that escaped


def _counts(hk, vp, depth, kind):
    L = hk._lib.lib()
    n = C.c_int32(0)
    PI = C.POINTER(C.c_int32)
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), None, None), "hk_test_queue_counts")
    out = np.zeros(n.value, np.int32)
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), out.ctypes.data_as(PI), None), "hk_test_queue_counts")
    return out


def _render(hk, knobs, build, spp, depth, env, switch=None, probe=None, fused=False, calls=1):
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
    vp = hk.VolPath(max_depth=depth, samples=spp * calls)
    try:
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        for c in range(calls):
            vp.render_samples(scene, film, cam, spp, first=1 + c * spp, readback=False)
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        if probe is not None:
            probe(vp, st)
        return acc, tuple(int(getattr(st, n)) for n in COUNTERS)
    finally:
        vp.close()


def _compare(hk, knobs, build, spp, depth, env=None, ways=WAYS, probe=None, **kw):
    env = {"HK_DYNAMIC_SEGMENTS": "1"} if env is None else env
    ref = _render(hk, knobs, build, spp, depth, env, probe=probe, **kw)
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0
    assert ref[1][0] > 0 and ref[1][3] > 0
    for switch in ways:
        got = _render(hk, knobs, build, spp, depth, env, switch, **kw)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "film differs under %s=%s" % switch
        assert got[1] == ref[1], "counters %r != %r under %s=%s" % ((got[1], ref[1]) + switch)
    return ref


def _box(hk, w, h, view):
    """The Cornell box, every record Matte (the light's too).  view "open": the camera outside, turned to the right so that a good part
    of the film looks past the box — rays escape at depth 0 and, through the open front, at every later depth; "light": the usual view,
    which sees the underside of the light — emissive hits at depth 0 and later; "closed": a sixth slab closes the front and the camera
    sits inside (the slabs overlap at every edge: no ray leaves)."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd import scenes
    from hikari_jl_amd.materials import MatteMaterial, RGBSpectrum

    def build():
        s, film, cam = scenes.cornell_box(w, h, light="area", tess=8)
        if view == "closed":
            s.push(G.rect3f((-1.0, 0, -1.0), (2.0, 2.0, 0.01)), MatteMaterial(Kd=RGBSpectrum(0.73, 0.73, 0.73)))
            s.sync()
            cam = hk.PerspectiveCamera((0, 1, -0.9), (0, 0.9, 0), film, fov=75.0)
        elif view == "open":
            cam = hk.PerspectiveCamera((0, 1, -3.5), (1.1, 1.3, 0), film, fov=40.0)
        return s, film, cam
    return build


def _open_stage(hk, w, h):
    """test_shade_chunks' open stage with a second matte sphere in place of the mirror (ONE material kind): a floor, a back wall and
    two spheres under the quad light.  About half of the paths escape at every bounce — whole pixels of them above the wall and beside
    the floor — so the generations of a 128-path segment hold anything from nothing to all 128."""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.film import Film
    from hikari_jl_amd.materials import Emissive, MatteMaterial, MediumInterface, RGBSpectrum
    from hikari_jl_amd.scene import Scene

    def build():
        white = MatteMaterial(Kd=RGBSpectrum(0.73, 0.73, 0.73))
        s = Scene()
        s.push(G.rect3f((-1.0, 0, -1.0), (2.0, 0.01, 2.0)), white)
        s.push(G.rect3f((-1.0, 0, 0.99), (2.0, 2.0, 0.01)), white)
        s.push(G.sphere((-0.4, 0.4, 0.0), 0.35, 8), white)
        s.push(G.sphere((0.4, 0.35, 0.0), 0.3, 8), white)
        y = 1.98
        q = G.quad((-0.25, y, -0.25), (0.25, y, -0.25), (0.25, y, 0.25), (-0.25, y, 0.25), normal=(0, -1, 0))
        s.push(q, MediumInterface(MatteMaterial(Kd=RGBSpectrum(0.0)), emission=Emissive(Le=RGBSpectrum(1.0), scale=1.0, two_sided=False)))
        s.sync()
        film = Film((w, h))
        return s, film, hk.PerspectiveCamera((0.3, 1.2, -3.5), (0, 0.8, 0), film, fov=40.0)
    return build


def _single_kind(hk, scene):
    return {scene.desc.materials[i].kind for i in range(scene.desc.n_materials)} == {hk._abi.HK_MAT_MATTE}


@gpu
@pytest.mark.parametrize("spp", [16, 64])
@pytest.mark.parametrize("size", [(37, 29), (64, 48)])
@pytest.mark.parametrize("view", ["open", "closed", "light"])
def test_box_bit_for_bit(hk, knobs, view, size, spp):
    """The three boxes at depth 3, ragged (37 x 29 pads to 40 x 32) and whole last chunks, 16 and 64 samples."""
    seen = {}

    def probe(vp, st):
        seen["rays"] = [_counts(hk, vp, d, RAYS) for d in range(3)]
        seen["escaped"] = [_counts(hk, vp, d, ESCAPED) for d in range(3)]
        seen["matte"] = [_counts(hk, vp, d, HK_MAT_MATTE) for d in range(3)]

    build = _box(hk, *size, view)
    assert _single_kind(hk, build()[0])
    _compare(hk, knobs, build, spp, 3, probe=probe)
    for d in range(3):   # a generation is its hits and its escaped rays, segment by segment
        assert np.array_equal(seen["rays"][d], seen["matte"][d] + seen["escaped"][d])
    escaped = [int(e.sum()) for e in seen["escaped"]]
    if view == "open":
        assert min(escaped) > 0, escaped
    if view == "closed":
        assert escaped == [0, 0, 0], escaped


@gpu
@pytest.mark.parametrize("segments", ["1", "0"])
def test_deep_paths(hk, knobs, segments):
    """Depth 8: Russian roulette (from the fourth bounce on) thins the generations; tickets and the static stride."""
    _compare(hk, knobs, _box(hk, 37, 29, "open"), 16, 8, {"HK_DYNAMIC_SEGMENTS": segments})


@gpu
def test_camera_sees_the_light(hk, knobs):
    """The "light" view has emissive hits at depth 0 (flagged entries of the kind queue, which the trace kernel still writes) and the
    emission pass of later bounces walks the light BVH for its MIS weight."""
    seen = {}

    def probe(vp, st):
        n = C.c_int32(0)
        PI = C.POINTER(C.c_int32)
        L = hk._lib.lib()
        hk._lib.check(L.hk_test_queue_counts(vp._integ, 0, HK_MAT_MATTE, C.byref(n), None, None), "hk_test_queue_counts")
        out, fl = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        hk._lib.check(L.hk_test_queue_counts(vp._integ, 0, HK_MAT_MATTE, C.byref(n), out.ctypes.data_as(PI), fl.ctypes.data_as(PI)), "hk_test_queue_counts")
        seen["flagged"] = int(fl.sum())

    _render(hk, knobs, _box(hk, 64, 48, "light"), 16, 1, {"HK_DYNAMIC_SEGMENTS": "1"}, probe=probe)
    assert seen["flagged"] > 0


def _escaped_pixels(hk, oracle, build, w, h, margin=2):
    """pixels whose own first hit and that of every pixel within `margin` is a miss by the oracle's first-hit depth (pixel centres): the
    filter's support is narrower than the margin, so every camera sample of such a pixel escapes"""
    s, _, cam = build()
    _, _, depth = oracle.OracleScene(s).fill_aux(cam, w, h)
    miss = ~np.isfinite(depth) | (depth <= 0)
    inner = miss.copy()
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            inner &= np.roll(np.roll(miss, dy, 0), dx, 1)
    inner[:margin] = inner[-margin:] = False
    inner[:, :margin] = inner[:, -margin:] = False
    return int(inner.sum()), int(miss.sum()), miss.size


@gpu
def test_segment_sizes_around_the_chunk(hk, oracle, knobs):
    """Generations of 0, fewer than 64, exactly 64, 65 and 128 rays in one render, and chunks made up of escaped entries alone.  64 x 32
    pixels x 64 samples over four segments per CU of 256 CUs give every segment 128 camera paths — two pixels, one per 64-entry chunk.
    The sizes come from hk_test_queue_counts on this very render, and the test insists that the five it is about occurred.  By the
    oracle's hit mask the view has pixels whose samples all escape: at depth 0 such a pixel is a 64-slot run of escaped entries, and
    the render had segments whose two chunks were both of that sort, and segments that mix a hit chunk and an escaped one."""
    sizes, seen = set(), {}

    def probe(vp, st):
        for d in range(3):
            sizes.update(int(c) for c in _counts(hk, vp, d, RAYS))
        seen["rays0"], seen["escaped0"] = _counts(hk, vp, 0, RAYS), _counts(hk, vp, 0, ESCAPED)

    build = _open_stage(hk, 64, 32)
    assert _single_kind(hk, build()[0])
    all_escaped, missed, total = _escaped_pixels(hk, oracle, build, 64, 32)
    assert all_escaped >= 64 and missed < total // 2 + total // 4, (all_escaped, missed, total)
    _compare(hk, knobs, build, 64, 3, {"HK_DYNAMIC_SEGMENTS": "1", "HK_WAVES_PER_CU": "4"}, probe=probe)
    assert {0, 64, 65, 128} <= sizes and any(0 < c < 64 for c in sizes), sorted(sizes)
    r0, e0 = seen["rays0"], seen["escaped0"]
    assert (r0 == 128).all()
    assert (e0 == 128).any()                     # both chunks of the segment hold escaped entries only
    assert (e0 == 64).any() and ((e0 > 0) & (e0 < 64)).any() and (e0 == 0).any()


@gpu
def test_unreferenced_mirror_record_takes_the_queue_walk(hk, gpu_ctx, knobs):
    """A Mirror record that no triangle refers to makes the scene one of two kinds: the queue walk.  Same film, counters and queue
    sizes as the same geometry without it (the slot walk) — and as that one under HK_SHADE_SLOT_WALK=0."""
    one, two, (cam_args, size) = LS._pair(hk, gpu_ctx, knobs, "cornell")
    kw = dict(max_depth=4, samples=16)
    ref = LS._render(hk, knobs, two, cam_args, size, kw, 16)
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0 and min(ref[1]) > 0
    LS._same(LS._render(hk, knobs, one, cam_args, size, kw, 16), ref)
    LS._same(LS._render(hk, knobs, one, cam_args, size, kw, 16, {"HK_SHADE_SLOT_WALK": "0"}), ref)


@gpu
def test_material_edits_switch_the_walk(hk, gpu_ctx, knobs):
    """Matte -> Mix -> Matte through hk_scene_update_materials: the walk goes off and on again with DScene::single_kind, and each
    render equals that of a scene created that way (_edit_round_trip's own comparisons); the last state, all Matte again, renders the
    same film with the walk switched off."""
    keep, sh, mixes, mix_recs, matte, plain, kinds = LS._edit_round_trip(hk, gpu_ctx, knobs, lambda: LS._matte_mix_scene(hk), 48, 48)
    assert len(mixes) == 1
    kw = dict(max_depth=4, samples=8)
    on = LS._render(hk, knobs, keep[1], LS.CORNELL_CAM, (48, 48), kw, 8)
    off = LS._render(hk, knobs, keep[1], LS.CORNELL_CAM, (48, 48), kw, 8, {"HK_SHADE_SLOT_WALK": "0"})
    LS._same(on, off)


@gpu
def test_view_cache(hk, knobs):
    """Three identical frames of one view: the second and third do not launch k_camera (view-cache hits 2) and give the first's film,
    with the slot walk and without."""
    films, hits = [], []

    def frames(switch):
        knobs.setenv("HK_BATCH_PATHS_M", "0")
        knobs.setenv("HK_SMALL_PASS_FUSED", "0")
        knobs.setenv("HK_DYNAMIC_SEGMENTS", "1")
        knobs.delenv("HK_SHADE_SLOT_WALK")
        if switch:
            knobs.setenv("HK_SHADE_SLOT_WALK", "0")
        scene, _, cam = _box(hk, 37, 29, "open")()
        vp = hk.VolPath(max_depth=3, samples=16)
        try:
            out = []
            vp._ensure_ctx()
            before = int(vp.stats().view_cache_hits)   # (the hit count is the context's, summed over its integrators)
            for _ in range(3):
                film = hk.Film((37, 29))
                vp._ensure(film)
                vp.clear()
                vp.render_samples(scene, film, hk.PerspectiveCamera((0, 1, -3.5), (1.1, 1.3, 0), film, fov=40.0), 16, readback=False)
                out.append(vp.read_accumulators(film).copy())
            hits.append(int(vp.stats().view_cache_hits) - before)
            return out
        finally:
            vp.close()

    on, off = frames(False), frames(True)
    assert hits == [2, 2], hits
    for f in on[1:] + off:
        assert np.array_equal(f.view(np.uint32), on[0].view(np.uint32))
    assert np.isfinite(on[0]).all() and on[0].max() > 0


@gpu
def test_small_passes(hk, knobs):
    """One-sample calls on a small film are k_small_pass launches (no explicit HK_DYNAMIC_SEGMENTS: that would keep the stages), which
    keep the queue walk and their own flush: unchanged by the knob."""
    knobs.delenv("HK_DYNAMIC_SEGMENTS")
    fused = []
    probe = lambda vp, st: fused.append(int(st.fused_passes))
    a = _render(hk, knobs, _box(hk, 37, 29, "open"), 1, 3, {}, probe=probe, fused=True, calls=4)
    b = _render(hk, knobs, _box(hk, 37, 29, "open"), 1, 3, {}, ("HK_SHADE_SLOT_WALK", "0"), probe=probe, fused=True, calls=4)
    assert fused[0] > 0 and fused[1] > 0, fused
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1]


PROGRAM = r"""
#include "hk_edit_host.h"
#include <cstdio>
int main() {
    // knob, HK_SHADE_PRESCAN=1, HK_SHADE_LEAN
    std::printf("%d %d %d %d %d\n", hk::shade_slot_walk_wanted(true, false, true), hk::shade_slot_walk_wanted(false, false, true), hk::shade_slot_walk_wanted(true, true, true),
                hk::shade_slot_walk_wanted(true, false, false), hk::shade_slot_walk_wanted(true, true, false));
    // per launch: wanted, single_kind, the launch's kind, the trace launch ran the single-kind flush
    std::printf("%d %d %d %d %d\n", hk::shade_slot_walk_launch(1, 0, 0, true), hk::shade_slot_walk_launch(0, 0, 0, true), hk::shade_slot_walk_launch(1, -1, 0, true),
                hk::shade_slot_walk_launch(1, 1, 0, true), hk::shade_slot_walk_launch(1, 0, 0, false));
    return 0;
}
"""


def test_knob_is_listed_read_and_overruled(tmp_path):
    """Host side: HK_SHADE_SLOT_WALK is on the list of record and ensure_state reads it into DPathState::shade_slot_walk through
    hk::shade_slot_walk_wanted, which HK_SHADE_PRESCAN=1 and HK_SHADE_LEAN=0 overrule; launch_shade asks hk::shade_slot_walk_launch,
    which wants a scene of the launch's one kind and the single-kind flush.  Both are plain C++ (hk_edit_host.h): a stand-alone program
    under the sanitizers prints their tables."""
    import re
    ctx = open(os.path.join(CSRC, "hk_ctx.cpp")).read()
    listed = re.search(r"KNOB_NAMES\[\]\s*=\s*\{(.*?)\};", ctx, re.S).group(1)
    assert '"HK_SHADE_SLOT_WALK"' in listed
    render = re.sub(r"//.*", "", open(os.path.join(CSRC, "hk_render.cpp")).read())
    assert re.search(r'st\.shade_slot_walk\s*=\s*hk::shade_slot_walk_wanted\(hk::knob_on\("HK_SHADE_SLOT_WALK"\),\s*I->st\.shade_prescan != 0,\s*hk::knob_on\("HK_SHADE_LEAN"\)\)', render)
    launch = re.sub(r"//.*", "", open(os.path.join(CSRC, "hk_launch_impl.h")).read())
    assert re.search(r"shade_slot_walk_launch\(st\.shade_slot_walk,\s*sc\.single_kind,\s*kind,\s*lean_flush\(sc, fr\) == 2\)", launch)
    assert "HK_SHADE_SLOT_WALK" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = tmp_path / "walk.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "walk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:2] == ["1 0 0 0 0", "1 0 0 0 0"]
