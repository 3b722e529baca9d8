"""A new sky (sun direction, turbidity) for the sun-sky scene: the host bake + hk_scene_update_envmap against hk_scene_update_envmap_sky,
which bakes the texels on the device.  The two paths are interleaved in one process, at each map resolution.

Prints one JSON line per resolution (wall times in ms, medians of --reps; the stream is idle before each):
  res, bytes_record, bytes_texels   what crosses to the device: the parameter record against 16 * res^2
  host_bake_ms                      (a) sunsky.sky_texels on the host ...
  host_path_ms                      (a) ... + hk_scene_update_envmap + hk_sync: what a caller does without the entry point
  params_ms                         (b) sunsky.sky_params (cooking the coefficients on the host)
  device_call_ms, device_path_ms    (b) hk_scene_update_envmap_sky alone, and with hk_sync (texel kernel + table kernels)
  tables_only_ms                    hk_scene_update_envmap of resident texels + hk_sync: the upload and the table kernels alone, for where (b)'s time goes
  frame_before_ms, frame_after_ms   a frame of the scene (--frame-spp samples at 256 x 256) before and after the edits: it should not move
  e_device                          the device texels against the host bake under the metric of tests/sky_cases.py (one parameter set)
Usage: python tools/sky_edit_timing.py [--reps 15] [--res 512 1024] [--frame-spp 4]
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
from hikari_jl_amd import scenes, sunsky  # noqa: E402


def median_ms(samples):
    return round(float(np.median(samples)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frame-spp", type=int, default=4)
    a = ap.parse_args()
    L = hk._lib.lib()
    A = hk._abi
    ctx = hk.Context.get(0)
    sync = lambda: hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    skies = [dict(direction=(np.cos(0.1 * k), 0.4, 0.2 + 0.05 * k), turbidity=2.0 + 0.3 * k, ground_enabled=False) for k in range(a.reps + 1)]
    for res in a.res:
        s, film, cam = scenes.sky_scene(256, 256, env_res=res, tess=32)
        sh = hk.scene_handle(ctx, s)
        vp = hk.VolPath(max_depth=6, samples=a.frame_spp)

        def frame():
            vp.clear()
            sync()
            t0 = time.perf_counter()
            vp.render_samples(s, film, cam, a.frame_spp, first=1, readback=False)
            sync()
            return time.perf_counter() - t0

        vp._ensure(film)
        frame()
        before = [frame() for _ in range(5)]
        out = dict(res=res, bytes_record=C.sizeof(A.hk_sky_params), bytes_texels=16 * res * res)
        t = dict(host_bake=[], host_path=[], params=[], device_call=[], device_path=[], tables_only=[])
        for k in range(a.reps + 1):                          # (round 0 warms both paths: staging block, code objects)
            sky = skies[k]
            sync()
            t0 = time.perf_counter()
            texels = sunsky.sky_texels(resolution=res, **sky)
            t1 = time.perf_counter()
            jl = np.ascontiguousarray(np.transpose(np.concatenate([texels, np.ones((res, res, 1), np.float32)], axis=2), (1, 0, 2)))
            hk._lib.check(L.hk_scene_update_envmap(sh, 0, jl.ctypes.data_as(A.PF), None), "hk_scene_update_envmap")
            sync()
            t2 = time.perf_counter()
            params = sunsky.sky_params(**sky)
            t3 = time.perf_counter()
            hk._lib.check(L.hk_scene_update_envmap_sky(sh, 0, C.byref(params)), "hk_scene_update_envmap_sky")
            t4 = time.perf_counter()
            sync()
            t5 = time.perf_counter()
            hk._lib.check(L.hk_scene_update_envmap(sh, 0, jl.ctypes.data_as(A.PF), None), "hk_scene_update_envmap")
            sync()
            t6 = time.perf_counter()
            if k:
                for name, v in (("host_bake", t1 - t0), ("host_path", t2 - t0), ("params", t3 - t2), ("device_call", t4 - t3), ("device_path", t5 - t3), ("tables_only", t6 - t5)):
                    t[name].append(v)
        for name, v in t.items():
            out[name + "_ms"] = median_ms(v)
        out["speedup"] = round(out["host_path_ms"] / out["device_path_ms"], 1)
        # agreement of the last sky, and the frame afterwards (the device's sky is the one in place)
        hk._lib.check(L.hk_scene_update_envmap_sky(sh, 0, C.byref(params)), "hk_scene_update_envmap_sky")
        got = np.zeros((res, res, 4), np.float32)
        hk._lib.check(L.hk_scene_envmap_copy(sh, 0, None, None, got.ctypes.data_as(A.PF), None, None, None, None, None), "hk_scene_envmap_copy")
        got = got.transpose(1, 0, 2)[..., :3].astype(np.float64)
        top = texels.max(axis=2, keepdims=True).astype(np.float64)
        out["e_device"] = float((np.abs(got - texels)[top[..., 0] > 0] / top[top[..., 0] > 0]).max())
        after = [frame() for _ in range(5)]
        out["frame_before_ms"], out["frame_after_ms"] = median_ms(before), median_ms(after)
        print(json.dumps(out), flush=True)
        vp.close()
        s.close()


if __name__ == "__main__":
    main()
