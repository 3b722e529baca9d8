"""Scene edits on the 10^6-triangle scene (scenes.many_light_scene): what hk_scene_set_transform costs against recreating the scene.

Prints one JSON line:
  create_s           hk_scene_create wall time (host SAH BVH build, light BVH, packing, upload)
  set_transform_host_ms_in_flight
                     host time of hk_scene_set_transform while a render of >= 25 ms is in flight (the call does not wait for it)
  in_flight_render_ms
                     how long the hk_sync after it still waited: the render was indeed running
  update_device_ms   HIP-event time of the update on the idle stream (median of 10): transform of the moved range + refit of every level
  update_full_device_ms
                     the same for a transform of all 10^6 triangles
  nodes_per_ray_before / _after, shadow_nodes_per_ray_before / _after
                     BVH node steps per closest-hit / shadow cast before and after moving 1 % of the boxes by about one box size
Usage: python tools/scene_edit_timing.py [--size 512] [--spp 4]
"""
import argparse
import json
import os
import sys
import time

import torch   # first: the HIP runtime the process initialises is torch's; its events bracket the library's (null) stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402
from hikari_jl_amd.scene import SceneInstance  # noqa: E402


def translate(dx, dy, dz):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (dx, dy, dz)
    return m


def node_steps(vp, s, film, cam, spp):
    vp.enable_counters(count_nodes=True)
    vp.reset_stats()
    vp.clear()
    vp.render_samples(s, film, cam, spp, first=1, readback=False)
    vp.sync()
    st = vp.stats()
    vp.enable_counters()
    return st.trace_nodes / max(1, st.rays_closest), st.shadow_nodes / max(1, st.rays_shadow)


def device_ms(ctx, fn, reps=10):
    L = hk._lib.lib()
    out = []
    for _ in range(reps):
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    torch.zeros(1, device="cuda")
    L = hk._lib.lib()
    s, film, cam = scenes.many_light_scene(a.size, a.size)
    T = s.desc.n_triangles
    ctx = hk.Context.get(0)
    t0 = time.perf_counter()
    sh = hk.scene_handle(ctx, s)
    hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    create_s = time.perf_counter() - t0
    # the matte boxes are the scene's first mesh: its first 1 % of the boxes (12 triangles each) is the moved block
    n_boxes = 83334
    block = SceneInstance(0, 0, (n_boxes // 100) * 12)
    everything = SceneInstance(0, 0, T)
    vp = hk.VolPath(max_depth=5, samples=a.spp)
    vp._ensure(film)
    before = node_steps(vp, s, film, cam, a.spp)
    # host time of the edit while a big render is in flight (> 8 M paths: enqueued by hk_render itself)
    big = hk.Film((1024, 1024))
    big_cam = hk.PerspectiveCamera((0.0, -0.2, 9.0), (0.8, 0.3, 0.0), big, up=(0, 1, 0), fov=60.0)
    vp2 = hk.VolPath(max_depth=5, samples=16)
    vp2._ensure(big)
    vp2.clear()
    vp2.render_samples(s, big, big_cam, 16, first=1, readback=False)
    hk._lib.check(L.hk_sync(ctx.h), "hk_sync")   # (warm: path state allocated)
    vp2.render_samples(s, big, big_cam, 16, first=17, readback=False)
    t0 = time.perf_counter()
    s.set_transform(block, translate(0.05, -0.05, 0.05))
    t1 = time.perf_counter()
    hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    t2 = time.perf_counter()
    vp2.close()
    after = node_steps(vp, s, film, cam, a.spp)
    upd = device_ms(ctx, lambda: s.set_transform(block, translate(0.05, -0.05, 0.05)))
    full = device_ms(ctx, lambda: s.set_transform(everything, translate(0.0, 0.01, 0.0)))
    s.set_transform(everything, np.eye(4, dtype=np.float32))
    restored = node_steps(vp, s, film, cam, a.spp)
    vp.close()
    nodes, depth = C.c_int32(), C.c_int32()
    L.hk_scene_bvh_info(sh, C.byref(nodes), None, C.byref(depth))
    print(json.dumps(dict(triangles=T, bvh_nodes=nodes.value, bvh_depth=depth.value, create_s=round(create_s, 3),
                          set_transform_host_ms_in_flight=round((t1 - t0) * 1e3, 3), in_flight_render_ms=round((t2 - t1) * 1e3, 2),
                          update_device_ms=round(upd, 3), update_full_device_ms=round(full, 3),
                          nodes_per_ray_before=round(before[0], 2), nodes_per_ray_after=round(after[0], 2), nodes_per_ray_restored=round(restored[0], 2),
                          shadow_nodes_per_ray_before=round(before[1], 2), shadow_nodes_per_ray_after=round(after[1], 2))))


if __name__ == "__main__":
    main()
