"""Refitting the light BVH on the device against rebuilding it on the host: hk_scene_refit_lights and hk_scene_update_lights on the
many-light scene (scenes.many_light_scene: 10^6 triangles, ~5 * 10^4 emitters), for ONE light, a scattered 1 % and ALL lights.

Prints one JSON line (wall times, medians of --reps runs, the stream idle before each; "_sync" includes the hk_sync that follows):
  lights, bvh_lights
  refit_{one,pct,all}_host_ms / _sync_ms     hk_scene_refit_lights: the call, then with the wait (the first refit of the scene, which
                                             also uploads the tree as built, is reported apart: refit_first_sync_ms)
  update_{one,pct,all}_sync_ms               hk_scene_update_lights + hk_sync of the same records (pct: the contiguous range of that size)
  twin_{one,pct,all}_ms                      the host twin alone (hk_test_light_refit_host with the refit, minus without: the build)
  frame_created_ms                           a 512 x 512 4-spp frame of the scene as created
  frame_refit_all_ms, frame_rebuilt_ms       the same frame after the all-lights refit, and after hk_scene_update_lights rebuilt the
                                             tree from the same records (the fresh scene): what the kept topology costs
Usage: python tools/light_refit_timing.py [--reps 15]
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
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    L = hk._lib.lib()
    A = hk._abi
    ctx = hk.Context.get(0)
    s, film, cam = scenes.many_light_scene(512, 512)
    d = s.desc
    n = d.n_lights
    sh = hk.scene_handle(ctx, s)
    nn = C.c_int32()
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(nn), None, None), "hk_scene_light_bvh_copy")
    trails = np.zeros(n, np.uint32)
    nodes = np.zeros(16 * nn.value, np.float32)
    hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(nn), nodes.ctypes.data_as(A.PF), trails.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_light_bvh_copy")
    out = {"lights": n, "bvh_lights": (nn.value + 1) // 2}

    vp = hk.VolPath(max_depth=4, samples=4)
    vp._ensure(film)

    def frame():
        vp.clear()
        vp.render_samples(s, film, cam, 4, first=1, readback=False)

    frame()                                                  # (warm: path state, kernels)
    out["frame_created_ms"] = timed(ctx, frame, a.reps)[1]

    def dimmed(i, k):
        r = A.hk_light.from_buffer_copy(d.lights[i])
        r.scale *= 0.9 + 0.01 * (k % 10)                     # another value every call; a light of zero power stays one
        if r.kind == A.HK_LIGHT_DIFFUSE_AREA:                # and the emitter drifts, so that the kept topology has something to cost
            for j in range(9):
                r.v[j] += 0.05 * (((i * 7 + (j % 3) * 3 + k) % 11) - 5) / 5.0
        return r

    rng = np.random.default_rng(3)
    sets = {"one": [n // 2], "pct": sorted(int(i) for i in rng.choice(n, max(n // 100, 1), replace=False)), "all": list(range(n))}
    calls = [0]

    def refit(idx):
        calls[0] += 1
        recs = (A.hk_light * len(idx))(*[dimmed(i, calls[0]) for i in idx])
        ii = (C.c_int32 * len(idx))(*idx)
        return lambda: hk._lib.check(L.hk_scene_refit_lights(sh, len(idx), ii, recs), "hk_scene_refit_lights")

    t0 = time.perf_counter()
    refit(sets["one"])()
    hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    out["refit_first_sync_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    for name, idx in sets.items():
        fn = refit(idx)
        out["refit_%s_host_ms" % name], out["refit_%s_sync_ms" % name] = timed(ctx, fn, a.reps)
    calls[0] = 2
    refit(sets["all"])()                                     # the records the rebuild below sends too (dimmed(i, 3))
    frame()
    out["frame_refit_all_ms"] = timed(ctx, frame, a.reps)[1]

    # the host twin alone: the entry builds the tree first, so the build is measured and taken off
    orig = (A.hk_light * n)(*[A.hk_light.from_buffer_copy(d.lights[i]) for i in range(n)])

    def twin(idx):
        recs = (A.hk_light * max(len(idx), 1))(*[dimmed(i, 1) for i in idx]) if idx else None
        ii = (C.c_int32 * max(len(idx), 1))(*idx)
        cn = (C.c_int32 * 1)(len(idx))
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            hk._lib.check(L.hk_test_light_refit_host(orig, n, 1 if idx else 0, cn, ii, recs, C.byref(nn), None, None, None), "hk_test_light_refit_host")
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    build = twin([])
    out["twin_build_ms"] = round(build, 3)
    for name, idx in sets.items():
        out["twin_%s_ms" % name] = round(twin(idx) - build, 3)

    # the rebuild of the same edits (the parent's cost), last: it drops the refit state and gives the fresh tree of the current records
    first = {"one": n // 2, "pct": n // 3, "all": 0}
    for name, idx in sets.items():
        k = len(idx)
        recs = (A.hk_light * k)(*[dimmed(first[name] + j, 3) for j in range(k)])
        fn = lambda: hk._lib.check(L.hk_scene_update_lights(sh, first[name], k, recs), "hk_scene_update_lights")
        out["update_%s_sync_ms" % name] = timed(ctx, fn, max(a.reps // 3, 3))[1]
    frame()
    out["frame_rebuilt_ms"] = timed(ctx, frame, a.reps)[1]
    vp.close()
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
