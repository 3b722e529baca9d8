"""Medium edits against recreating the scene, for the two media the library was sized for: the bench's cloud (scenes.bomex_scene:
256 x 256 x 128 voxels as a NanoVDB tree, 64^3 majorant) and a 256 x 256 x 128 GridMedium with the default 16^3 majorant.  Each
alternates between the field and the field shifted by 32 voxels along x — a time series of two steps — and measures, interleaved on
the same device, medians of --reps (15) wall times of
  (a) hk_scene_update_medium + hk_sync: the voxels, or the tree bytes and the block table, cross to the device, which builds the
      majorant grid, the zero-cell mask and the NanoVDB bricks;
  (b) the only way to the same state without the entry point: the host majorant build of media.py, then hk_scene_create of the edited
      description, then hk_sync (the scene is destroyed outside the timed region).
The NanoVDB tree itself (build_nanovdb_from_dense) is input to both and is built once per volume, outside the timed regions.

Prints one JSON line; per medium
  update_call_ms / update_sync_ms    (a): the call alone (host block table, staging copy, enqueue), then with the wait for the device
  host_majorant_ms, create_sync_ms   the two halves of (b);  recreate_ms = their sum per repetition, median
  update_bytes / recreate_bytes      what each path sends to the device FOR THE MEDIUM (the geometry, lights and BVH of (b) come on top)
and, with --frames N (default 3; 0 skips it), the cloud configuration rendered as bench.py --config cloud renders it (1024 x 1024, depth 32,
256 spp): frame_before_s, then frame_after_s after an update to the SAME data — the edit must not change the frame time.
A third leg, on the bench cloud and on a 256 x 256 x 128 field with half of its 8^3 blocks filled ("dense_cloud", "dense_half"): the
time step arrives as a dense field, and the medium is updated, interleaved on the same device, by
  (a') the path the device builder replaces: build_nanovdb_from_dense on the host + hk_scene_update_medium + hk_sync;
  (c)  hk_scene_update_medium_dense + hk_sync, once from host memory (dense_host_*) and once from a torch device tensor (dense_device_*);
with the bytes each sends to the device, and frame_after_dense_s: the cloud's frame time after a dense update to the same data.
Usage: python tools/medium_edit_timing.py [--reps 15] [--frames 3] [--only cloud|grid|dense]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

try:
    import torch   # first: the HIP runtime the process initialises has to be torch's for a device tensor to be handed over
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402


def ms(t0, t1):
    return (t1 - t0) * 1e3


def med3(xs):
    return round(float(np.median(xs)), 3)


def medium_bytes(medium, recreate):
    """bytes the medium's data takes on its way to the device: (a) voxels or tree + block table; (b) also majorant, mask and bricks"""
    ncell = int(np.prod(medium.majorant_res))
    if isinstance(medium, hk.NanoVDBMedium):
        lo = [v >> 3 for v in medium.meta["index_min"]]
        hi = [v >> 3 for v in medium.meta["index_max"]]
        blocks = int(np.prod([max(h - l + 3, 3) for l, h in zip(lo, hi)]))
        sent = medium.buffer.size + blocks * 8
        return sent + (ncell * 4 + (ncell + 31) // 32 * 4 + blocks * 729 * 4 if recreate else 0)
    sent = medium.density.size * 4
    return sent + (ncell * 4 + (ncell + 31) // 32 * 4 if recreate else 0)


def measure(ctx, make_scene, volumes, reps):
    """make_scene(volume) -> (Scene, medium).  Alternates the device scene of volumes[0] between the two volumes by (a), and creates a
    scene of the same target by (b), `reps` times each, interleaved."""
    L = hk._lib.lib()
    A = hk._abi
    sync = lambda: hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    built = [make_scene(v) for v in volumes]                 # the host objects of both time steps (trees built here, once)
    keep = []
    recs = []
    for s, m in built:
        r = A.hk_medium()
        m.fill_record(r, keep, majorant=False)
        recs.append(r)
    live, _ = built[0]
    sh = hk.scene_handle(ctx, live)
    sync()
    hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(recs[1])), "hk_scene_update_medium")   # warm: staging block, grown buffers
    hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(recs[0])), "hk_scene_update_medium")
    sync()
    call, both, host_maj, create, recreate = [], [], [], [], []
    for k in range(reps):
        target = (k + 1) % 2
        sync()
        t0 = time.perf_counter()
        hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(recs[target])), "hk_scene_update_medium")
        t1 = time.perf_counter()
        sync()
        t2 = time.perf_counter()
        call.append(ms(t0, t1))
        both.append(ms(t0, t2))
        s, m = built[target]
        d = s.desc
        t0 = time.perf_counter()
        maj = m._majorant = m._build_majorant()
        d.media[0].majorant = maj.ctypes.data_as(A.PF)
        t1 = time.perf_counter()
        h = C.c_void_p()
        hk._lib.check(L.hk_scene_create(ctx.h, C.byref(d), C.byref(h)), "hk_scene_create")
        sync()
        t2 = time.perf_counter()
        L.hk_scene_destroy(h)
        host_maj.append(ms(t0, t1))
        create.append(ms(t1, t2))
        recreate.append(ms(t0, t2))
    out = dict(update_call_ms=med3(call), update_sync_ms=med3(both), host_majorant_ms=med3(host_maj), create_sync_ms=med3(create), recreate_ms=med3(recreate),
               update_bytes=medium_bytes(built[0][1], False), recreate_bytes=medium_bytes(built[0][1], True), reps=reps)
    return out, live, sh, recs


def half_filled_field(res=(256, 256, 128), seed=7):
    """half of the 8^3 blocks filled with values in [0.1, 1], the others empty"""
    rng = np.random.default_rng(seed)
    nb = tuple(r // 8 for r in res)
    on = rng.permutation(int(np.prod(nb))) < int(np.prod(nb)) // 2
    mask = np.repeat(np.repeat(np.repeat(on.reshape(nb), 8, axis=0), 8, axis=1), 8, axis=2)
    return np.where(mask, rng.uniform(0.1, 1.0, res), 0.0).astype(np.float32)


def measure_dense(ctx, live, sh, med, volumes, reps):
    """The device scene `sh` of `live` (medium `med`) alternates between the two dense fields by (a'), (c) from host memory and (c) from
    a device tensor, `reps` times each, interleaved; every path ends in the same device state."""
    from hikari_jl_amd import media
    L, A = hk._lib.lib(), hk._abi
    sync = lambda: hk._lib.check(L.hk_sync(ctx.h), "hk_sync")
    origin = med.bounds[0]
    extent = tuple(float(np.float32(med.bounds[1][k]) - np.float32(med.bounds[0][k])) for k in range(3))
    keep = []
    lean = A.hk_medium()
    med.fill_record(lean, keep, majorant=False, tree=False)

    def field(volume, tensor):
        f = A.hk_dense_field()
        f.res[:] = volume.shape
        f.layout = A.HK_DENSE_Z_FASTEST
        if tensor is None:
            f.data, f.on_device = volume.ctypes.data_as(A.PF), 0
        else:
            f.data, f.on_device = C.cast(C.c_void_p(tensor.data_ptr()), A.PF), 1
        return f

    tensors = [torch.from_numpy(v).cuda() for v in volumes] if torch is not None and torch.cuda.is_available() else None
    if tensors is not None:
        torch.cuda.synchronize()
    host_fields = [field(v, None) for v in volumes]
    dev_fields = [field(v, t) for v, t in zip(volumes, tensors)] if tensors is not None else None
    for f in host_fields[::-1] + (dev_fields or []):         # warm: staging block, working set, grown buffers
        hk._lib.check(L.hk_scene_update_medium_dense(sh, 0, C.byref(lean), C.byref(f)), "hk_scene_update_medium_dense")
    sync()
    t = dict(host_build=[], host_path=[], dense_host_call=[], dense_host=[], dense_device_call=[], dense_device=[])
    sent = 0
    for k in range(reps):
        target = (k + 1) % 2
        sync()
        t0 = time.perf_counter()                              # (a')
        med.buffer, med.meta = media.build_nanovdb_from_dense(volumes[target], origin, extent)
        t1 = time.perf_counter()
        rec = A.hk_medium()
        med.fill_record(rec, keep, majorant=False)
        hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(rec)), "hk_scene_update_medium")
        sync()
        t2 = time.perf_counter()
        t["host_build"].append(ms(t0, t1))
        t["host_path"].append(ms(t0, t2))
        sent = medium_bytes(med, False)
        for name, fields in (("dense_host", host_fields), ("dense_device", dev_fields)):   # (c)
            if fields is None:
                continue
            sync()
            t0 = time.perf_counter()
            hk._lib.check(L.hk_scene_update_medium_dense(sh, 0, C.byref(lean), C.byref(fields[target])), "hk_scene_update_medium_dense")
            t1 = time.perf_counter()
            sync()
            t2 = time.perf_counter()
            t[name + "_call"].append(ms(t0, t1))
            t[name].append(ms(t0, t2))
    out = {k + "_ms": med3(v) for k, v in t.items() if v}
    n = C.c_int64()                                           # the tree the last (c) left is the tree the last (a') built
    hk._lib.check(L.hk_scene_medium_tree_copy(sh, 0, None, C.byref(n), None, None, None, None), "hk_scene_medium_tree_copy")
    got = np.zeros(n.value, np.uint8)
    hk._lib.check(L.hk_scene_medium_tree_copy(sh, 0, None, C.byref(n), got.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None), "hk_scene_medium_tree_copy")
    out["tree_equals_host_build"] = bool(np.array_equal(got, med.buffer))
    out.update(host_path_bytes=sent, dense_host_bytes=int(volumes[0].size) * 4, dense_device_bytes=0, reps=reps)
    return out


def frame_times(ctx, scene, film, cam, n):
    vp = hk.VolPath(max_depth=32, samples=256)
    vp._ensure(film)
    ts = []
    for k in range(n + 2):                                   # two warm frames, as bench.py --warmup 2
        vp.clear()
        hk._lib.check(hk._lib.lib().hk_sync(ctx.h), "hk_sync")
        t0 = time.perf_counter()
        vp.render_samples(scene, film, cam, 256, first=1, readback=False)
        hk._lib.check(hk._lib.lib().hk_sync(ctx.h), "hk_sync")
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    vp.close()
    return round(float(np.median(ts)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["cloud", "grid", "dense"])
    a = ap.parse_args()
    ctx = hk.Context.get(0)
    L = hk._lib.lib()
    out = {}
    if a.only in (None, "cloud"):
        dens = scenes.bomex_density((256, 256, 128), 0.05, 620.0)
        shifted = np.ascontiguousarray(np.roll(dens, 32, axis=0))
        parts = {}

        def cloud(volume):
            s, film, cam = scenes.bomex_scene(1024, 1024, res=(256, 256, 128), majorant_res=(64, 64, 64))
            med = s.media[0]
            if volume is not dens:
                s.update_medium(med, data=volume)            # (no device scene yet: the kept description of the second time step)
            parts.setdefault("film_cam", (film, cam))
            return s, med

        res, live, sh, recs = measure(ctx, cloud, [dens, shifted], a.reps)
        out["cloud_nanovdb_64"] = res
        if a.frames > 0:
            film, cam = parts["film_cam"]
            hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(recs[0])), "hk_scene_update_medium")
            live_fresh, _ = cloud(dens)                       # a scene no edit has touched
            res["frame_before_s"] = frame_times(ctx, live_fresh, film, cam, a.frames)
            live_fresh.close()
            hk._lib.check(L.hk_scene_update_medium(sh, 0, C.byref(recs[0])), "hk_scene_update_medium")
            res["frame_after_s"] = frame_times(ctx, live, film, cam, a.frames)
        live.close()
    if a.only in (None, "dense"):
        dens = scenes.bomex_density((256, 256, 128), 0.05, 620.0)
        s, film, cam = scenes.bomex_scene(1024, 1024, res=(256, 256, 128), majorant_res=(64, 64, 64))
        sh = hk.scene_handle(ctx, s)
        res = measure_dense(ctx, s, sh, s.media[0], [dens, np.ascontiguousarray(np.roll(dens, 32, axis=0))], a.reps)
        out["dense_cloud"] = res
        if a.frames > 0:
            fresh, _, _ = scenes.bomex_scene(1024, 1024, res=(256, 256, 128), majorant_res=(64, 64, 64))   # a scene no edit has touched
            res["frame_before_s"] = frame_times(ctx, fresh, film, cam, a.frames)
            fresh.close()
            s.update_medium(s.media[0], data=dens, build="device")
            res["frame_after_dense_s"] = frame_times(ctx, s, film, cam, a.frames)
        s.close()
        half = half_filled_field()
        s, _, _ = scenes.bomex_scene(64, 64, res=(256, 256, 128), majorant_res=(64, 64, 64))
        sh = hk.scene_handle(ctx, s)
        out["dense_half"] = measure_dense(ctx, s, sh, s.media[0], [half, np.ascontiguousarray(np.roll(half, 32, axis=0))], a.reps)
        s.close()
    if a.only in (None, "grid"):
        dens = scenes.bomex_density((256, 256, 128), 0.05, 620.0)
        shifted = np.ascontiguousarray(np.roll(dens, 32, axis=0))

        def grid(volume):
            s, _, _ = scenes.bomex_scene(64, 64, res=(256, 256, 128), majorant_res=(16, 16, 16), kind="grid")
            med = s.media[0]
            if volume is not dens:
                s.update_medium(med, density=volume)
            return s, med

        res, live, _, _ = measure(ctx, grid, [dens, shifted], a.reps)
        out["grid_256x256x128_16"] = res
        live.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
