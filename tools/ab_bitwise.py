#!/usr/bin/env python3
"""Film accumulators of a few small scenes, and every frame of both display chains on three small films, under two builds of the
library (HK_LIB_PATH), compared bit for bit: for changes that only re-schedule or re-arrange work (loop shapes, kernel splits, shared
code).   python tools/ab_bitwise.py <specA> <specB>
A spec is a library path, or comma-separated VAR=value settings (the shipped library under those environment variables), or both
joined by commas: "HK_GREY_FLAT=0", "hikari.jl_amd/csrc/libx.so,HK_GREY=0"."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
import hikari_jl_amd as hk
from hikari_jl_amd import scenes
out = {}
cases = {"cloud_nanovdb": (lambda: scenes.cloud_scene(40, 36, "nanovdb", res=(48, 48, 24)), 10),
         "cloud_grid": (lambda: scenes.cloud_scene(40, 36, "grid", res=(48, 48, 24)), 10),
         "bomex": (lambda: scenes.bomex_scene(48, 48, res=(64, 64, 32)), 16),
         "integration": (lambda: scenes.integration_test_scene(40, 36), 5),
         "cornell": (lambda: scenes.cornell_box(40, 36, light="area"), 6)}
for name, (mk, depth) in cases.items():
    s, film, cam = mk()
    vp = hk.VolPath(max_depth=depth, samples=64)
    vp._ensure(film); vp.clear()
    vp.render_samples(s, film, cam, 24, first=1, readback=False)
    out[name] = vp.read_accumulators(film).copy()
    st = vp.stats()
    out[name + "_counts"] = np.array([st.rays_closest, st.rays_shadow, st.medium_collisions], np.int64)
    vp.close()

# The display chains, host arrays (hk_film_read_rgb / hk_film_fill_aux / hk_denoise / hk_postprocess / hk_film_postprocess) and film
# buffers (hk_film_update_aux / hk_film_read_aux / hk_film_present).  37 x 29: both sides under 33, so the step-16 taps clamp on both
# edges; most pixels of the single triangle escape: +Inf depths, the kept-pixel NaN branch, a non-trivial mask.
import ctypes as C, itertools
from hikari_jl_amd.postprocess import make_params, TONEMAPS
L, PF = hk._lib.lib(), hk._abi.PF
pf = lambda a: a.ctypes.data_as(PF)
W, H = 37, 29
DENOISE = (None, (0, True), (1, True), (2, False), (5, True))
PPS = [("none", None)] + [("%%s_g%%d_m%%d" %% (t, g, m), make_params(exposure=1.3, tonemap=t, gamma=2.2 if g else None, background=(0.1, 0.2, 0.3) if m else None))
                          for t, g, m in itertools.product(TONEMAPS, (0, 1), (0, 1))]
films = {"cornell": (lambda: scenes.cornell_box(W, H, light="area"), {}), "triangle": (lambda: scenes.single_triangle(W, H), {}),
         "cornell_f64": (lambda: scenes.cornell_box(W, H, light="area"), dict(accumulation_eltype="Float64"))}
for name, (mk, kw) in films.items():
    s, film, cam = mk()
    ctx = hk.Context.get(0)
    vp = hk.VolPath(max_depth=3, samples=8, **kw)
    vp._ensure(film); vp.clear()
    vp.render_samples(s, film, cam, 8, first=1, readback=False)
    fh, sh, camrec = vp._film[0], hk.scene_handle(ctx, s), cam.record()
    def call(fn, *args):
        assert fn(*args) == 0, (fn.__name__, L.hk_last_error())
    def frame():
        return np.full((W, H, 3), -1.0, np.float32)
    rgb = frame()
    call(L.hk_film_read_rgb, ctx.h, fh, pf(rgb))
    out["display_%%s_rgb" %% name] = rgb
    for inf in (0, 1):
        key = "display_%%s_inf%%d_" %% (name, inf)
        alb, nrm, dep = frame(), frame(), np.full((W, H), -1.0, np.float32)
        call(L.hk_film_fill_aux, ctx.h, sh, C.byref(camrec), W, H, inf, pf(alb), pf(nrm), pf(dep))
        call(L.hk_film_update_aux, ctx.h, fh, sh, C.byref(camrec), inf)
        alb2, nrm2, dep2 = frame(), frame(), np.full((W, H), -1.0, np.float32)
        call(L.hk_film_read_aux, ctx.h, fh, pf(alb2), pf(nrm2), pf(dep2))
        out[key + "fill_aux"] = np.concatenate([a.ravel() for a in (alb, nrm, dep)])
        out[key + "read_aux"] = np.concatenate([a.ravel() for a in (alb2, nrm2, dep2)])
        for tag, pp in PPS[1:]:
            a, b = frame(), frame()
            call(L.hk_postprocess, ctx.h, C.byref(pp), W, H, pf(rgb), pf(dep), pf(a))
            call(L.hk_film_postprocess, ctx.h, fh, C.byref(pp), pf(dep), pf(b))
            out[key + "postprocess_" + tag], out[key + "film_postprocess_" + tag] = a, b
        for d in DENOISE:
            dn = None if d is None else hk.DenoiseConfig(iterations=d[0], use_variance=d[1]).record()
            dtag = "dn_none" if d is None else "dn%%d_v%%d" %% (d[0], int(d[1]))
            if dn is not None:
                a, after = frame(), frame()
                call(L.hk_denoise, ctx.h, C.byref(dn), W, H, pf(rgb), pf(nrm), pf(dep), pf(a), pf(after))
                out[key + "denoise_" + dtag], out[key + "denoise_after_" + dtag] = a, after
            for tag, pp in PPS:
                a = frame()
                call(L.hk_film_present, ctx.h, fh, None if dn is None else C.byref(dn), None if pp is None else C.byref(pp), pf(a))
                out[key + "present_" + dtag + "_" + tag] = a
    vp.close()
np.savez(sys.argv[1], **out)
'''


def main(lib_a, lib_b):
    import numpy as np
    outs = []
    for i, lib in enumerate((lib_a, lib_b)):
        path = "/tmp/ab_bitwise_%d.npz" % i
        env = dict(os.environ)
        for part in lib.split(","):
            if "=" in part:
                k, v = part.split("=", 1)
                env[k] = v
            elif part and part != "-":
                env["HK_LIB_PATH"] = os.path.abspath(part)
        subprocess.check_call([sys.executable, "-c", CHILD % {"root": ROOT}, path], env=env, timeout=900)
        outs.append(np.load(path))
    ok, frames = True, 0
    for k in outs[0].files:
        a, b = outs[0][k], outs[1][k]
        same = np.array_equal(a.view(np.uint8), b.view(np.uint8))
        ok &= same
        frames += k.startswith("display_")
        if same and k.startswith("display_"):   # some 1200 frames: only the differing ones are named
            continue
        print("%-58s %s" % (k, "identical" if same else "DIFFERENT (max abs %.3g)" % float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())))
    print("display chains: %d outputs compared" % frames)
    print("ALL IDENTICAL" if ok else "DIFFERENCES")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
