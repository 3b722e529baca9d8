"""Light and environment-map edits against recreating the scene: hk_scene_update_lights on the many-light scene
(scenes.many_light_scene: 10^6 triangles, ~5 * 10^4 emitters) and a texel update of a 1024 x 512 map through hk_scene_update_envmap.

Prints one JSON line (wall times; every "_sync" figure includes the hk_sync that waits for the enqueued copies / kernels):
  lights, bvh_lights           the scene's light count and how many are in the light BVH
  create_s                     hk_scene_create of the scene (what an edit replaces; unchanged by the edit entry points)
  update_one_host_ms / _sync_ms
                               hk_scene_update_lights of ONE light: the call (host rebuild of the whole light BVH + enqueue), then with the wait
  update_all_host_ms / _sync_ms
                               the same touching every light
  envmap_update_host_ms / _sync_ms
                               hk_scene_update_envmap with new texels of a 1024 x 512 map: staging copy + enqueue, then with the device table build
  envmap_host_tables_ms        envmap.py's table build for the same texels (EnvironmentMap(...)), the host chain's first half
  envmap_create_ms             hk_scene_create of the small scene that holds the map (uploads texels and five tables), its second half
Usage: python tools/light_edit_timing.py [--reps 5] [--skip-lights]
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
from hikari_jl_amd import geometry as G  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402
from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap  # noqa: E402


def timed(ctx, fn, reps):
    """median (call, call + hk_sync) in ms over reps runs, the stream idle before each"""
    L = hk._lib.lib()
    host, both = [], []
    for _ in range(reps):
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3)
        both.append((t2 - t0) * 1e3)
    return round(float(np.median(host)), 3), round(float(np.median(both)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-lights", action="store_true")
    a = ap.parse_args()
    L = hk._lib.lib()
    A = hk._abi
    ctx = hk.Context.get(0)
    out = {}
    if not a.skip_lights:
        s, _, _ = scenes.many_light_scene(64, 64)
        d = s.desc
        t0 = time.perf_counter()
        sh = hk.scene_handle(ctx, s)
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        out["create_s"] = round(time.perf_counter() - t0, 3)
        n = C.c_int32()
        hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(n), None, None), "hk_scene_light_bvh_copy")
        out["lights"], out["bvh_lights"] = d.n_lights, (n.value + 1) // 2
        one = A.hk_light.from_buffer_copy(d.lights[d.n_lights // 2])
        one.scale *= 0.5
        upd = lambda first, count, recs: hk._lib.check(L.hk_scene_update_lights(sh, first, count, recs), "hk_scene_update_lights")
        out["update_one_host_ms"], out["update_one_sync_ms"] = timed(ctx, lambda: upd(d.n_lights // 2, 1, C.byref(one)), a.reps)
        out["update_all_host_ms"], out["update_all_sync_ms"] = timed(ctx, lambda: upd(0, d.n_lights, d.lights), a.reps)
        s.close()
    # the sky: a 1024 x 512 map over a small scene
    rng = np.random.default_rng(1)
    w, h = 1024, 512
    tex = [(0.05 + rng.random((h, w, 3))).astype(np.float32) for _ in range(2)]
    t0 = time.perf_counter()
    em = EnvironmentMap(tex[0])
    out["envmap_host_tables_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    e = hk.Scene()
    e.push(G.rect3f((-2, -2, -1), (4, 4, 0.01)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    e.push(EnvironmentLight(em, hk.RGBSpectrum(1.0)))
    e.sync()
    t0 = time.perf_counter()
    eh = hk.scene_handle(ctx, e)
    hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    out["envmap_create_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    jl = [np.ascontiguousarray(np.transpose(np.concatenate([t, np.ones((h, w, 1), np.float32)], axis=2), (1, 0, 2))) for t in tex]
    k = [0]

    def new_texels():
        k[0] += 1
        hk._lib.check(L.hk_scene_update_envmap(eh, 0, jl[k[0] % 2].ctypes.data_as(A.PF), None), "hk_scene_update_envmap")

    new_texels()                                           # (warm: the staging block is allocated by the first call)
    out["envmap_update_host_ms"], out["envmap_update_sync_ms"] = timed(ctx, new_texels, a.reps)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
