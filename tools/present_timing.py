"""The display chain of a viewer on the Cornell box at 800^2 (default DenoiseConfig, ACES with gamma 2.2): what showing a frame costs
through the host chain and through hk_film_present.

Prints one JSON line (every figure the median of --reps warm repetitions, spread = the quartiles of the same repetitions):
  host_chain_wall_ms       hk_film_read_rgb -> hk_denoise -> hk_postprocess with the aux buffers already on the host
  present_wall_ms          hk_film_present (the same frame, bit for bit), wall time of the call
  present_device_ms        the same call between two events on the context's stream (kernels + the one copy)
  loop_present_async_ms    ms per call of a loop of one-sample renders with hk_film_present_async one call behind
  loop_read_rgb_async_ms   the same loop with the plain hk_film_read_rgb_async: the difference is what the denoise costs on top
  step1_old_device_ms      one step-1 pass of k_atrous<PlanarPixels>: event time of hk_denoise with 1 iteration minus with 0 (no variance;
                           uploads and downloads are the same in both)
  step1_new_device_ms      one step-1 pass of k_atrous<PackedPixels> plus the packed k_finalize: event time of hk_film_present with 1
                           iteration (no variance, no postprocess) minus the plain finalize-and-copy — an upper bound for the pass
                           Both are differences of event times around whole calls: the quartiles are a quarter of the values.  They
                           say whether a pass got slower, not by how much it got faster; a kernel trace gives the durations.
Usage: python tools/present_timing.py [--size 800] [--reps 15]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch   # first: the HIP runtime the process initialises is torch's; its events bracket the library's (null) stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402
from hikari_jl_amd.postprocess import make_params  # noqa: E402


def stats(samples):
    q1, med, q3 = np.percentile(samples, [25, 50, 75])
    return round(float(med), 4), [round(float(q1), 4), round(float(q3), 4)]


def wall_ms(ctx, fn, reps):
    L = hk._lib.lib()
    out = []
    for _ in range(reps):
        hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_ms(ctx, fn, reps):
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    assert a.reps >= 10
    torch.zeros(1, device="cuda")
    L = hk._lib.lib()
    PF = hk._abi.PF
    w = h = a.size
    s, film, cam = scenes.cornell_box(w, h, light="area")
    ctx = hk.Context.get(0)
    vp = hk.VolPath(max_depth=5, samples=8)
    vp._ensure(film)
    vp.clear()
    vp.render_samples(s, film, cam, 8, first=1, readback=False)
    fh, sh, camrec = vp._film[0], hk.scene_handle(ctx, s), cam.record()
    check = hk._lib.check
    dn, pp = hk.DenoiseConfig().record(), make_params(tonemap="aces", gamma=2.2)
    dn_p, pp_p = C.byref(dn), C.byref(pp)
    rgb, den, out_host, out_dev = (np.empty((w, h, 3), np.float32) for _ in range(4))
    alb, nrm, dep = np.empty((w, h, 3), np.float32), np.empty((w, h, 3), np.float32), np.empty((w, h), np.float32)
    check(L.hk_film_fill_aux(ctx.h, sh, C.byref(camrec), w, h, 0, alb.ctypes.data_as(PF), nrm.ctypes.data_as(PF), dep.ctypes.data_as(PF)), "hk_film_fill_aux")
    check(L.hk_film_update_aux(ctx.h, fh, sh, C.byref(camrec), 0), "hk_film_update_aux")

    def host_chain():
        check(L.hk_film_read_rgb(ctx.h, fh, rgb.ctypes.data_as(PF)), "hk_film_read_rgb")
        check(L.hk_denoise(ctx.h, dn_p, w, h, rgb.ctypes.data_as(PF), nrm.ctypes.data_as(PF), dep.ctypes.data_as(PF), den.ctypes.data_as(PF), None), "hk_denoise")
        check(L.hk_postprocess(ctx.h, pp_p, w, h, den.ctypes.data_as(PF), None, out_host.ctypes.data_as(PF)), "hk_postprocess")

    def present(d=dn_p, p=pp_p):
        check(L.hk_film_present(ctx.h, fh, d, p, out_dev.ctypes.data_as(PF)), "hk_film_present")

    for _ in range(3):                       # warm: every buffer of both chains exists, the kernels are loaded
        host_chain()
        present()
    same = bool(np.array_equal(out_host.view(np.uint32), out_dev.view(np.uint32)))
    res = dict(size=a.size, reps=a.reps, frames_bit_equal=same)
    # (a), (b) interleaved, so that a drift of the machine hits both
    ha, pb = [], []
    for _ in range(a.reps):
        ha += wall_ms(ctx, host_chain, 1)
        pb += wall_ms(ctx, present, 1)
    res["host_chain_wall_ms"], res["host_chain_wall_quartiles"] = stats(ha)
    res["present_wall_ms"], res["present_wall_quartiles"] = stats(pb)
    res["present_device_ms"], res["present_device_quartiles"] = stats(device_ms(ctx, present, a.reps))

    # (d), (e): a viewer's loop, the frame shown one call behind
    def loop(enqueue, calls=40):
        first = [film.iteration_index + 1]

        def step():
            vp.render_samples(s, film, cam, 1, first=first[0], readback=False)
            first[0] += 1
            check(L.hk_flush(ctx.h), "hk_flush")
            check(L.hk_film_read_wait(ctx.h, fh, None, None), "hk_film_read_wait")
            enqueue()
        enqueue()
        for _ in range(8):
            step()
        out = []
        for _ in range(a.reps):
            check(L.hk_sync(ctx.h), "hk_sync")
            enqueue()
            t0 = time.perf_counter()
            for _ in range(calls):
                step()
            check(L.hk_film_read_wait(ctx.h, fh, None, None), "hk_film_read_wait")
            out.append((time.perf_counter() - t0) * 1e3 / calls)
        return out

    la = loop(lambda: check(L.hk_film_present_async(ctx.h, fh, dn_p, pp_p), "hk_film_present_async"))
    lb = loop(lambda: check(L.hk_film_read_rgb_async(ctx.h, fh), "hk_film_read_rgb_async"))
    res["loop_present_async_ms"], res["loop_present_async_quartiles"] = stats(la)
    res["loop_read_rgb_async_ms"], res["loop_read_rgb_async_quartiles"] = stats(lb)

    # (f) one step-1 pass, old kernel against new, as differences of event times (interleaved)
    def one(iterations):
        p = hk.DenoiseConfig(iterations=iterations, use_variance=False).record()
        return C.byref(p), p

    d0, d1 = one(0), one(1)

    def old(d):
        check(L.hk_denoise(ctx.h, d[0], w, h, rgb.ctypes.data_as(PF), nrm.ctypes.data_as(PF), dep.ctypes.data_as(PF), den.ctypes.data_as(PF), None), "hk_denoise")

    def pass_times():
        o0, o1, n0, n1 = [], [], [], []
        for _ in range(a.reps):
            o0 += device_ms(ctx, lambda: old(d0), 1)
            o1 += device_ms(ctx, lambda: old(d1), 1)
            n0 += device_ms(ctx, lambda: present(None, None), 1)
            n1 += device_ms(ctx, lambda: present(d1[0], None), 1)
        return np.array(o1) - np.array(o0), np.array(n1) - np.array(n0)

    present(d1[0], None)
    o, n = pass_times()
    res["step1_old_device_ms"], res["step1_old_device_quartiles"] = stats(o)
    res["step1_new_device_ms"], res["step1_new_device_quartiles"] = stats(n)
    vp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
