"""Vertex edits on the 10^6-triangle scene (scenes.many_light_scene): what hk_scene_set_vertices costs against the alternative it
replaces, hk_scene_create of the deformed description.

Prints one JSON line:
  all / range_10pct  new positions and normals for every triangle / for one 10 % range that starts and ends off the block size:
      call_ms            wall time of the hk_scene_set_vertices call on an idle context (median of 15): staging copy, finite check and
                         block boxes on the host, everything else only enqueued
      done_ms            wall time from the call until hk_sync returns (median of 15): upload, k_set_tris, refit of every level
      upload_bytes       positions + normals of the range (the interval table adds under 1 KB)
  create_s           hk_scene_create + hk_sync of the deformed description (median of 3): host SAH build, light BVH, packing, upload
  cost_ratio         hk_scene_bvh_cost now / created after the deformation (a ripple of a fifth of a box size)
  deep               the box cloud of tests/test_vertex_edits.py (33 600 triangles, tree deeper than 16): for every --scales entry the
                     deformation field of the test times that factor -> cost ratio and the trace-class kernel time (k_trace_lean) of one
                     --size^2 frame of --spp samples, depth 5, from the library's kernel timers
Usage: python tools/vertex_edit_timing.py [--size 512] [--spp 4] [--scales 0,1,6,20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402

f32 = np.float32
PF = hk._abi.PF


def ripple(P, amplitude):
    d = np.stack([np.sin(f32(3) * P[..., 1] + f32(1)), np.cos(f32(2) * P[..., 2]), np.sin(f32(4) * P[..., 0])], axis=-1).astype(f32)
    return np.ascontiguousarray((P + f32(amplitude) * d).astype(f32))


def timed_edit(ctx, sh, first, P, N, reps=15):
    L = hk._lib.lib()
    call, done = [], []
    for _ in range(reps):
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t0 = time.perf_counter()
        hk._lib.check(L.hk_scene_set_vertices(sh, first, len(P), P.ctypes.data_as(PF), N.ctypes.data_as(PF) if N is not None else None, None, None), "hk_scene_set_vertices")
        t1 = time.perf_counter()
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t2 = time.perf_counter()
        call.append((t1 - t0) * 1e3)
        done.append((t2 - t0) * 1e3)
    return dict(call_ms=round(float(np.median(call)), 3), done_ms=round(float(np.median(done)), 3), upload_bytes=int(P.nbytes + (N.nbytes if N is not None else 0)))


def deep_section(ctx, size, spp, scales):
    from hikari_jl_amd.geometry import Mesh
    rng = np.random.default_rng(3)                          # tests/test_scene_edits.py::_boxes(2800, 3)
    n = 2800
    layer = rng.integers(0, 12, n)
    radius = 1.0 + 0.45 * layer + 0.1 * rng.random(n)
    phi = rng.random(n) * 2 * np.pi
    centers = np.stack([radius * np.cos(phi), radius * np.sin(phi), (rng.random(n) * 2 - 1) * 6.0], axis=1)
    half = 0.012 + 0.03 * rng.random((n, 3))
    P, N = scenes._boxes_mesh(centers, half, rng.random(n) * np.pi)
    P, N = np.ascontiguousarray(P, f32), np.ascontiguousarray(N, f32)
    s = hk.Scene()
    inst = s.push_instance(Mesh(P, N, None), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.6)))
    s.push(hk.PointLight((0.0, 0.0, 8.0), hk.RGBSpectrum(40.0)))
    s.sync()
    film = hk.Film((size, size))
    cam = hk.PerspectiveCamera((0.0, -0.2, 9.0), (0.8, 0.3, 0.0), film, up=(0, 1, 0), fov=60.0)
    vp = hk.VolPath(max_depth=5, samples=spp)
    vp._ensure(film)
    hk.scene_handle(ctx, s)
    out = []
    for scale in scales:
        s.set_vertices(inst, ripple(P, 0.05 * scale))       # (the normals stay: they do not enter the traversal)
        now, created = s.bvh_cost(ctx)
        times = []
        for rep in range(4):                                # the first frame warms the path state
            vp.enable_counters(time_kernels=True)
            vp.reset_stats()
            vp.clear()
            vp.render_samples(s, film, cam, spp, first=1, readback=False)
            vp.sync()
            times.append(vp.stats().seconds_trace * 1e3)
        out.append(dict(scale=scale, cost_ratio=round(now / created, 4), trace_ms_per_frame=round(float(np.median(times[1:])), 3)))
    vp.enable_counters()
    vp.close()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--scales", default="0,1,6,20")
    a = ap.parse_args()
    L = hk._lib.lib()
    ctx = hk.Context.get(0)
    s, _, _ = scenes.many_light_scene(64, 64)
    d = s.desc
    T = d.n_triangles
    kept_p, kept_n = s._keep[0], s._keep[1]                 # the arrays the description points into
    P = ripple(kept_p, 0.01)
    N = np.ascontiguousarray(kept_n, f32)
    sh = hk.scene_handle(ctx, s)
    res = dict(triangles=T)
    res["all"] = timed_edit(ctx, sh, 0, P, N)
    now, created = s.bvh_cost(ctx)
    res["cost_ratio"] = round(now / created, 4)
    a0 = T // 2 + 5
    n10 = T // 10 + 3
    res["range_10pct"] = timed_edit(ctx, sh, a0, P[a0:a0 + n10], N[a0:a0 + n10])
    # what an application had to do before: create a scene from the deformed description
    kept_p[:] = P
    create = []
    for _ in range(3):
        h = C.c_void_p()
        t0 = time.perf_counter()
        hk._lib.check(L.hk_scene_create(ctx.h, C.byref(d), C.byref(h)), "hk_scene_create")
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        create.append(time.perf_counter() - t0)
        L.hk_scene_destroy(h)
    res["create_s"] = round(float(np.median(create)), 3)
    s.close()
    res["deep"] = deep_section(ctx, a.size, a.spp, [float(x) for x in a.scales.split(",")])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
