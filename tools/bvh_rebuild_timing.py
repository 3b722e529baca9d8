"""hk_scene_rebuild_bvh on the 10^6-triangle scene (scenes.many_light_scene) against the alternative it replaces, hk_scene_create of the
deformed description, and what the new tree is worth per frame.

The scene is deformed in place with the ripple of tools/vertex_edit_timing.py, its amplitude doubled until hk_scene_bvh_cost reports
now / created > --ratio (1.5).  Prints one JSON line:
  amplitude, cost_ratio_before   the deformation reached and the drift of the refit tree under it
  rebuild_ms         wall time of the hk_scene_rebuild_bvh call on an idle context (median of --reps, 15): the call waits for the build
  rebuild_done_ms    ... until hk_sync returns (the refit of the new tree and its cost reduction are only enqueued by the call)
  create_s           hk_scene_create + hk_sync of the deformed description in the same process (median of --reps)
  cost_ratio_after   now / created of the FRESH scene's cost against the rebuilt tree's (1 when the trees are the same)
  nodes, depth       of the rebuilt tree and of the fresh one
  frame_ms           one --size^2 frame of --spp samples, depth 5 (median of 7 after a warm-up): refit tree, rebuilt tree, fresh scene
Usage: python tools/bvh_rebuild_timing.py [--size 512] [--spp 4] [--ratio 1.5] [--reps 15]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402
from vertex_edit_timing import ripple  # noqa: E402

f32 = np.float32
PF = hk._abi.PF


def frame_ms(vp, s, film, cam, spp, reps=8):
    times = []
    for _ in range(reps):                                   # the first frame warms the path state
        vp.clear()
        vp.sync()
        t0 = time.perf_counter()
        vp.render_samples(s, film, cam, spp, first=1, readback=False)
        vp.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times[1:])), 3)


def info(sh):
    n, d = C.c_int32(), C.c_int32()
    hk._lib.check(hk._lib.lib().hk_scene_bvh_info(sh, C.byref(n), None, C.byref(d)), "hk_scene_bvh_info")
    return n.value, d.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ratio", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    L = hk._lib.lib()
    ctx = hk.Context.get(0)
    s, _, _ = scenes.many_light_scene(64, 64)
    d = s.desc
    T = d.n_triangles
    kept_p = s._keep[0]
    base = kept_p.copy()
    sh = hk.scene_handle(ctx, s)
    res = dict(triangles=T)
    amplitude, now, created = 0.01, 0.0, 1.0
    while True:
        P = ripple(base, amplitude)
        hk._lib.check(L.hk_scene_set_vertices(sh, 0, T, P.ctypes.data_as(PF), None, None, None), "hk_scene_set_vertices")
        now, created = s.bvh_cost(ctx)
        if now / created > a.ratio or amplitude > 10.0:
            break
        amplitude *= 2.0
    res.update(amplitude=amplitude, cost_ratio_before=round(now / created, 4))
    film = hk.Film((a.size, a.size))
    cam = hk.PerspectiveCamera((0.0, -0.2, 9.0), (0.8, 0.3, 0.0), film, up=(0, 1, 0), fov=60.0)   # (the scene's own view)
    vp = hk.VolPath(max_depth=5, samples=a.spp)
    vp._ensure(film)
    frames = dict(refit=frame_ms(vp, s, film, cam, a.spp))
    call, done = [], []
    for _ in range(a.reps):
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t0 = time.perf_counter()
        hk._lib.check(L.hk_scene_rebuild_bvh(sh), "hk_scene_rebuild_bvh")
        t1 = time.perf_counter()
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        call.append((t1 - t0) * 1e3)
        done.append((time.perf_counter() - t0) * 1e3)
    res.update(rebuild_ms=round(float(np.median(call)), 3), rebuild_done_ms=round(float(np.median(done)), 3))
    rebuilt_now, rebuilt_created = s.bvh_cost(ctx)
    frames["rebuilt"] = frame_ms(vp, s, film, cam, a.spp)
    # the yardstick: a scene created from the deformed description
    kept_p[:] = P
    create = []
    fresh = C.c_void_p()
    for k in range(a.reps):
        if fresh:
            L.hk_scene_destroy(fresh)
        fresh = C.c_void_p()
        t0 = time.perf_counter()
        hk._lib.check(L.hk_scene_create(ctx.h, C.byref(d), C.byref(fresh)), "hk_scene_create")
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        create.append(time.perf_counter() - t0)
    res["create_s"] = round(float(np.median(create)), 3)
    fc = C.c_double()
    hk._lib.check(L.hk_scene_bvh_cost(fresh, None, C.byref(fc)), "hk_scene_bvh_cost")
    res["cost_ratio_after"] = round(rebuilt_now / fc.value, 6)
    res["nodes_depth"] = dict(rebuilt=info(sh), fresh=info(fresh))
    L.hk_scene_destroy(fresh)
    # the fresh scene's frame, through the mirror (which creates it from the same description)
    s.close()                                               # drops the rebuilt device scene; the next render creates the scene anew
    frames["fresh"] = frame_ms(vp, s, film, cam, a.spp)
    res["frame_ms"] = frames
    vp.close()
    s.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
