"""The pin that turns "parity unpinned" into "pinned once": outputs of Hikari's OWN per-stage functions, dumped by
julia/make_reference_fixtures.jl on the first box that has Julia + Hikari (this image has neither), compared here with the oracle
(CPU) and — `-m gpu` — with the device, on the committed inputs of tests/golden/reference_inputs/.

  * `tests/golden/reference/` is EMPTY until that script has run: the comparing tests then SKIP with a loud reason (they do not pass).
  * What runs here and now: the committed inputs are what their script writes; the Julia script names only reference functions that
    exist at the lines it cites, reads only committed inputs and writes exactly the arrays this module consumes; and the whole
    comparison pipeline is exercised end to end on a stand-in fixture set written FROM THE ORACLE'S OWN OUTPUTS into a temporary
    directory (it proves the loaders, scene mirrors and tolerances run — not parity).

The stage computations run in a child process (`python tests/test_reference_fixtures.py <side> <fixture dir> <out dir>`) with
HK_RGB2SPEC_TABLE pointing at the RGB -> spectrum table the Julia side dumped, when there is one: this repo regenerates that table
(the reference's blob is lost), so both sides must look colours up in the SAME table for ulp-level comparisons to mean
anything.  Tolerances are SURVEY 8(d)'s: bit-exact for integer work, <= 2 ulp for the table look-ups, and the recorded bounds of
the existing device-vs-oracle tests where libm differs (Julia's own exp / log / sincos against glibc's and the device's)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fixture_io  # noqa: E402

REF_DIR = os.path.join(HERE, "golden", "reference")
IN_DIR = os.path.join(HERE, "golden", "reference_inputs")
JULIA = os.path.join(ROOT, "julia", "make_reference_fixtures.jl")
REFERENCE_INDEX = os.path.join(HERE, "golden", "reference_index.json")   # citations checked against the reference tree
f32 = np.float32
FILTER_NAMES = ("box", "triangle", "gaussian", "mitchell", "lanczos")
N_MATERIALS = 14


# ------------------------------------------------------------------------------------------------ the scenes of the Julia script, mirrored
def reference_palette(hk):
    """palette() of julia/make_reference_fixtures.jl, index for index"""
    R = hk.RGBSpectrum
    eta, k = R(0.2, 0.92, 1.1), R(3.9, 2.45, 2.14)
    return [
        hk.MatteMaterial(Kd=R(0.6, 0.4, 0.2)),
        hk.MatteMaterial(Kd=R(0.6, 0.4, 0.2), sigma=20.0),
        hk.MirrorMaterial(Kr=R(0.9, 0.8, 0.7)),
        hk.GlassMaterial(Kr=R(0.9), Kt=R(0.8, 0.9, 1.0), index=1.5),
        hk.ConductorMaterial(eta=eta, k=k, roughness=0.09),
        hk.ConductorMaterial(eta=eta, k=k, roughness=0.0),
        hk.Gold(roughness=0.04),
        hk.CoatedDiffuseMaterial(reflectance=R(0.5, 0.3, 0.2), u_roughness=0.1, v_roughness=0.1, thickness=0.01, eta=1.5, albedo=R(0.0), g=0.0, max_depth=10, n_samples=1),
        hk.CoatedDiffuseMaterial(reflectance=R(0.4, 0.5, 0.6), u_roughness=0.0, v_roughness=0.0, thickness=0.05, eta=1.33, albedo=R(0.6, 0.7, 0.8), g=0.3, max_depth=10, n_samples=2),
        hk.ThinDielectricMaterial(eta=1.5),
        hk.DiffuseTransmissionMaterial(reflectance=R(0.5, 0.4, 0.3), transmittance=R(0.3, 0.4, 0.5), scale=1.0),
        hk.CoatedDiffuseTransmissionMaterial(reflectance=R(0.5, 0.3, 0.2), transmittance=R(0.2, 0.3, 0.4), u_roughness=0.15, v_roughness=0.15, thickness=0.01, eta=1.5,
                                             albedo=R(0.0), g=0.0, max_depth=10, n_samples=1),
        hk.CoatedConductorMaterial(interface_u_roughness=0.05, interface_v_roughness=0.05, interface_eta=1.5, conductor_eta=eta, conductor_k=k,
                                   conductor_u_roughness=0.1, conductor_v_roughness=0.1, thickness=0.01, albedo=R(0.0), g=0.0, max_depth=10, n_samples=1),
        hk.CoatedConductorMaterial(interface_u_roughness=0.0, interface_v_roughness=0.0, interface_eta=1.5, conductor_eta=eta, conductor_k=k,
                                   conductor_u_roughness=0.0, conductor_v_roughness=0.0, thickness=0.01, albedo=R(0.0), g=0.0, max_depth=10, n_samples=1),
    ]


def palette_scene(hk):
    from hikari_jl_amd import geometry as G
    s = hk.Scene()
    for i, m in enumerate(reference_palette(hk)):
        s.push(G.quad((i, 0, 0), (i + 0.5, 0, 0), (i + 0.5, 0.5, 0), (i, 0.5, 0)), m)
    s.push(hk.PointLight((0, 3, 0), hk.RGBSpectrum(1.0)))
    s.sync()
    return s


def reference_light_scene(hk):
    """light_scene() of the Julia script: five analytic lights + 24 emissive boxes (12 faces each) under the ceiling"""
    from hikari_jl_amd import geometry as G
    R = hk.RGBSpectrum
    s = hk.Scene()
    s.push(hk.AmbientLight(R(0.5, 0.6, 0.9)))
    s.push(hk.SpotLight((-0.7, 1.7, -0.8), (0.1, 0.3, 0.1), R(20.0, 18.0, 14.0), 25.0, 15.0))
    s.push(hk.DirectionalLight(R(2.0, 1.9, 1.6), (0.25, -0.45, 1.0)))
    s.push(hk.PointLight((0.5, 1.6, -0.4), R(6.0, 5.0, 3.0)))
    s.push(hk.SunLight(R(3.0, 2.8, 2.5), (-0.3, -0.8, 0.2)))
    s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), hk.MatteMaterial(Kd=R(0.73, 0.73, 0.73)))
    for ix in range(6):
        for iz in range(4):
            x0, z0 = f32(-0.9) + f32(0.3) * f32(ix), f32(-0.6) + f32(0.3) * f32(iz)
            Le = R(0.2 + 0.1 * ix, 0.9 - 0.1 * iz, 0.5)
            s.push(G.rect3f((x0, 1.97, z0), (0.2, 0.005, 0.2)), hk.Emissive(Le=Le, scale=float(f32(1) + f32(0.25) * f32(iz)), two_sided=False))
    s.sync()
    return s


def reference_nanovdb_scene(hk, density):
    from hikari_jl_amd import geometry as G
    s = hk.Scene()
    med = hk.NanoVDBMedium(density, ((-0.5, 0.0, -0.3), (0.5, 0.6, 0.2)), sigma_a=hk.RGBSpectrum(0.0), sigma_s=hk.RGBSpectrum(1.0), g=0.877, majorant_res=(16, 16, 16))
    glass = hk.GlassMaterial(Kr=hk.RGBSpectrum(0.0), Kt=hk.RGBSpectrum(1.0), index=1.0)
    s.push(G.rect3f((-0.5, 0.0, -0.3), (1.0, 0.6, 0.5)), hk.MediumInterface(glass, inside=med, outside=None))
    s.push(hk.PointLight((0, 3, 0), hk.RGBSpectrum(1.0)))
    s.sync()
    return s, med


def integration_scene(hk, with_fog):
    from hikari_jl_amd import scenes
    return scenes.integration_test_scene(64, 64, with_fog=with_fog)


def nvdb_value(buf, root_off, root_n, i, j, k):
    """nanovdb_get_value (nanovdb.jl:315-388) over the raw tree bytes: root tile by key (linear search) -> upper 32^3 -> lower 16^3 -> leaf
    8^3; a tile without a child holds a constant; child offsets are relative to the parent node (offsets 1-based like the reference's)"""
    rd = lambda off1, dt: np.frombuffer(buf, dt, 1, off1 - 1)[0]          # noqa: E731
    u = [v & 0xFFFFFFFF for v in (i, j, k)]
    key = ((u[2] >> 12) & 0x1fffff) | (((u[1] >> 12) & 0x1fffff) << 21) | (((u[0] >> 12) & 0x1fffff) << 42)
    tile = None
    for t in range(root_n):
        off = root_off + 64 + t * 32
        if int(rd(off, np.uint64)) == key:
            tile = off
            break
    if tile is None:
        return f32(rd(root_off + 28, np.float32))
    child = int(rd(tile + 8, np.int64))
    if child == 0:
        return f32(rd(tile + 20, np.float32))
    up = root_off + child
    n_up = (((u[0] >> 7) & 31) << 10) | (((u[1] >> 7) & 31) << 5) | ((u[2] >> 7) & 31)
    if not (int(buf[up + 4128 - 1 + (n_up >> 3)]) >> (n_up & 7)) & 1:
        return f32(rd(up + 8256 + n_up * 8, np.float32))
    lw = up + int(rd(up + 8256 + n_up * 8, np.int64))
    n_lw = (((u[0] >> 3) & 15) << 8) | (((u[1] >> 3) & 15) << 4) | ((u[2] >> 3) & 15)
    if not (int(buf[lw + 544 - 1 + (n_lw >> 3)]) >> (n_lw & 7)) & 1:
        return f32(rd(lw + 1088 + n_lw * 8, np.float32))
    leaf = lw + int(rd(lw + 1088 + n_lw * 8, np.int64))
    return f32(rd(leaf + 96 + (((i & 7) << 6) | ((j & 7) << 3) | (k & 7)) * 4, np.float32))


# ------------------------------------------------------------------------------------------------ one side's outputs, in the fixture's names
def compute(side, IN, stages=None):
    """-> {array name: what `side` ("oracle" | "device") computes for the committed inputs}, the names julia/make_reference_fixtures.jl writes"""
    import ctypes as C
    import hikari_jl_amd as hk
    import oracle as O
    out = {}
    dev = side == "device"
    if dev:
        ctx = hk.Context.get(0)
        L = hk._lib.lib()
    PF = hk._abi.PF
    pf = lambda a: a.ctypes.data_as(PF)                                   # noqa: E731
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                 # noqa: E731
    want = lambda s: stages is None or s in stages                       # noqa: E731

    if want("sobol"):
        px, py, si, dm = (np.ascontiguousarray(IN["sobol_" + k]) for k in ("px", "py", "sidx", "dim"))
        if dev:
            o1, o2 = np.empty(len(px), f32), np.empty((len(px), 2), f32)
            hk._lib.check(L.hk_test_sobol(ctx.h, 64, 64, 4096, 0, len(px), pi(px), pi(py), pi(si), pi(dm), pf(o1), pf(o2)), "hk_test_sobol")
        else:
            o1, o2 = O.sobol(64, 64, 4096, 0, px, py, si, dm)
        out["sobol_1d"], out["sobol_2d"] = o1, o2

    if want("camera"):
        film = hk.Film((64, 64))
        cam = hk.PerspectiveCamera((0.0, 1.0, -3.5), (0.0, 1.0, 0.0), film, fov=40.0)
        px, py, si = (np.ascontiguousarray(IN["cam_" + k]) for k in ("px", "py", "sidx"))
        filters = dict(box=hk.BoxFilter((0.5, 0.5)), triangle=hk.TriangleFilter((2.0, 2.0)), gaussian=hk.GaussianFilter((1.5, 1.5), 0.5),
                       mitchell=hk.MitchellFilter((2.0, 2.0), 1.0 / 3.0, 1.0 / 3.0), lanczos=hk.LanczosSincFilter((4.0, 4.0), 3.0))
        for name in FILTER_NAMES:
            p = hk.integrator_params(max_depth=5, samples=64, filter=filters[name])
            if dev:
                integ = C.c_void_p()
                hk._lib.check(L.hk_integrator_create(ctx.h, C.byref(p), C.byref(integ)), "hk_integrator_create")
                o = np.empty((len(px), 15), f32)
                rec = cam.record()
                hk._lib.check(L.hk_test_camera(ctx.h, integ, C.byref(rec), 64, 64, len(px), pi(px), pi(py), pi(si), pf(o)), "hk_test_camera")
                L.hk_integrator_destroy(integ)
            else:
                o = O.camera_samples(p, cam, 64, 64, px, py, si)
            out["camera_" + name] = o

    if want("uplift"):
        rgb, lam = np.ascontiguousarray(IN["uplift_rgb"]), np.ascontiguousarray(IN["uplift_lambda"])
        for mode, name in enumerate(("bounded", "unbounded", "illuminant")):
            if dev:
                o = np.empty_like(lam)
                hk._lib.check(L.hk_test_uplift(ctx.h, mode, len(rgb), pf(rgb), pf(lam), pf(o)), "hk_test_uplift")
            else:
                o = O.uplift(mode, rgb, lam)
            out["uplift_" + name] = o

    if want("bsdf"):
        s = palette_scene(hk)
        a = [np.ascontiguousarray(IN["bsdf_" + k]) for k in ("wo", "wi", "ns", "lambda", "u", "uc")]
        n = len(a[0])
        osc = None if dev else O.OracleScene(s)
        sh = hk.scene_handle(ctx, s) if dev else None
        for k in range(N_MATERIALS):
            for mode, reg, name in ((0, False, "bsdf_sample_%d_reg0" % k), (0, True, "bsdf_sample_%d_reg1" % k), (1, False, "bsdf_eval_%d" % k)):
                if dev:
                    o = np.zeros((n, 10), f32)
                    hk._lib.check(L.hk_test_bsdf(ctx.h, sh, mode, k, 1 if reg else 0, n, *[pf(x) for x in a], pf(o)), "hk_test_bsdf")
                else:
                    o = osc.bsdf(mode, k, *a, regularize=reg)
                if mode == 1:
                    o = o.copy()
                    o[:, 5:] = 0
                out[name] = o
        if osc:
            osc.close()

    if want("lights"):
        s = reference_light_scene(hk)
        p, nrm, u1 = (np.ascontiguousarray(IN["light_" + k]) for k in ("p", "n", "u1"))
        lam, u2 = np.ascontiguousarray(IN["light_lambda"]), np.ascontiguousarray(IN["light_u2"])
        n, n_lights = len(p), int(s.desc.n_lights)
        query = np.array([1 + (i * 7) % n_lights for i in range(1, n + 1)], np.int32)
        which = np.array([1 + (i - 1) % n_lights for i in range(1, n + 1)], np.int32)
        x = np.zeros((n, 3), f32)
        x[:, :2] = u2
        ls = np.zeros((n, 12), f32)
        if dev:
            sh = hk.scene_handle(ctx, s)
            li, pmf, qp = np.empty(n, np.int32), np.empty(n, f32), np.empty(n, f32)
            hk._lib.check(L.hk_test_light_bvh(ctx.h, sh, n, pf(p), pf(nrm), pf(u1), pi(li), pf(pmf), pi(query), pf(qp)), "hk_test_light_bvh")
            for flat in range(1, n_lights + 1):
                rows = np.nonzero(which == flat)[0]
                if len(rows) == 0:
                    continue
                o = np.zeros((len(rows), 12), f32)
                a = [np.ascontiguousarray(v[rows]) for v in (p, x, lam)]
                hk._lib.check(L.hk_test_light(ctx.h, sh, 0, flat, len(rows), *[pf(v) for v in a], pf(o)), "hk_test_light")
                ls[rows] = o
            nn = C.c_int32()
            hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(nn), None, None), "hk_scene_light_bvh_copy")
            nodes = np.zeros((max(nn.value, 1), 16), f32)
            trails = np.zeros(max(n_lights, 1), np.uint32)
            hk._lib.check(L.hk_scene_light_bvh_copy(sh, C.byref(nn), pf(nodes), trails.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_light_bvh_copy")
            nodes, trails = nodes[:nn.value], trails[:n_lights]
        else:
            osc = O.OracleScene(s)
            li, pmf, qp = osc.light_bvh(p, nrm, u1, query)
            for flat in range(1, n_lights + 1):
                rows = np.nonzero(which == flat)[0]
                if len(rows):
                    ls[rows] = osc.light(0, flat, p[rows], x[rows], lam[rows])
            nodes, trails = osc.light_bvh_nodes()
            osc.close()
        out.update(lightbvh_choice=li, lightbvh_pmf=pmf, lightbvh_query=query, lightbvh_query_pmf=qp, light_sample=ls, light_index=which,
                   lightbvh_nodes=np.ascontiguousarray(nodes, f32), lightbvh_bit_trails=np.ascontiguousarray(trails, np.uint32),
                   lightbvh_counts=np.array([int(s.desc.n_lights) - 3, 3, int(s.desc.n_lights)], np.int32))     # (infinite: ambient, directional, sun)

    if want("envlight"):
        from hikari_jl_amd import geometry as G
        env = hk.EnvironmentMap(np.ascontiguousarray(IN["env_rgb"]))
        s = hk.Scene()
        s.push(hk.EnvironmentLight(env, hk.RGBSpectrum(0.8, 1.0, 1.2)))
        s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.73, 0.73, 0.73)))
        s.sync()
        p, lam, u2 = (np.ascontiguousarray(IN[k]) for k in ("light_p", "light_lambda", "light_u2"))
        x = np.zeros((len(p), 3), f32)
        x[:, :2] = u2
        if dev:
            o = np.zeros((len(p), 12), f32)
            hk._lib.check(L.hk_test_light(ctx.h, hk.scene_handle(ctx, s), 0, 1, len(p), pf(p), pf(x), pf(lam), pf(o)), "hk_test_light")
        else:
            osc = O.OracleScene(s)
            o = osc.light(0, 1, p, x, lam)
            osc.close()
        out["envlight_sample"] = o
        D = env.distribution                                   # (the host-side builder, hikari.jl_amd/envmap.py restating sampler/sampling.jl:179-262 — the same on both sides)
        out["envlight_marginal_cdf"] = np.ascontiguousarray(D.marginal_cdf, f32).reshape(-1)
        out["envlight_conditional_cdf"] = np.ascontiguousarray(D.conditional_cdf, f32).reshape(-1)

    if want("nanovdb"):
        s, med = reference_nanovdb_scene(hk, np.ascontiguousarray(IN["nvdb_density"]))
        pw, lam = np.ascontiguousarray(IN["nvdb_p"]), np.ascontiguousarray(IN["light_lambda"])
        if dev:
            sh = hk.scene_handle(ctx, s)
            o = np.zeros((len(pw), 13), f32)
            hk._lib.check(L.hk_test_medium(ctx.h, sh, 0, 0, len(pw), pf(pw), None, None, pf(lam), pf(o)), "hk_test_medium")
        else:
            osc = O.OracleScene(s)
            o = osc.medium(0, 0, pw, lam)
            osc.close()
        out["nvdb_sample_point"] = o
        # the host-side builder (hikari.jl_amd/media.py restates nanovdb.jl:602-858, 1169-1235) — the same on both sides
        out["nvdb_buffer"] = np.ascontiguousarray(med.buffer, np.uint8)
        out["nvdb_majorant"] = np.ascontiguousarray(med.majorant, f32).reshape(-1)
        out["nvdb_values"] = np.array([nvdb_value(out["nvdb_buffer"], int(med.meta["root_offset"]), int(med.meta["root_table_size"]), int(i), int(j), int(k))
                                       for i, j, k in IN["nvdb_ijk"]], f32)
        out["nvdb_index_bbox"] = np.array(list(med.meta["index_min"]) + list(med.meta["index_max"]), np.int32)

    if want("frame"):
        for name, fog, res, spp, depth in (("frame_surfaces_64_spp4_depth5", False, 64, 4, 5), ("frame_fog_32_spp1024_depth4", True, 32, 1024, 4)):
            from hikari_jl_amd import scenes
            s, film, cam = scenes.integration_test_scene(res, res, with_fog=fog)
            kw = dict(max_depth=depth, samples=spp)
            if dev:
                vp = hk.VolPath(**kw)
                vp(s, film, cam)
                img = film.framebuffer.copy()
                vp.close()
            else:
                osc = O.OracleScene(s)
                acc, _ = osc.render(hk.integrator_params(**kw), cam, res, res, spp)
                osc.close()
                img = O.finalize(acc, res, res)
            out[name] = np.ascontiguousarray(img, f32)
    return out


# ------------------------------------------------------------------------------------------------ comparison
def ulp_diff(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def compare(got, ref):
    """-> list of (array name, problem) — empty when `got` matches the fixture set `ref` within the stage tolerances"""
    bad = []

    def need(name):
        if name not in ref:
            return False
        if name not in got:
            bad.append((name, "not computed"))
            return False
        if got[name].shape != ref[name].shape:
            bad.append((name, "shape %s vs %s" % (got[name].shape, ref[name].shape)))
            return False
        return True

    def frac_close(name, cols, rtol, atol, min_frac):
        g, r = got[name][:, cols], ref[name][:, cols]
        ok = np.isclose(g, r, rtol=rtol, atol=atol).all(axis=1).mean()
        if ok < min_frac:
            bad.append((name, "%.5f of the rows agree (need %.5f)" % (ok, min_frac)))

    for name in ("sobol_1d", "sobol_2d", "nvdb_values", "nvdb_majorant", "nvdb_index_bbox", "lightbvh_bit_trails", "lightbvh_counts", "light_index", "lightbvh_query"):
        if need(name) and not np.array_equal(got[name], ref[name]):
            bad.append((name, "not bit-equal (%d entries differ)" % int((got[name] != ref[name]).sum())))
    if need("nvdb_buffer") and not np.array_equal(got["nvdb_buffer"], ref["nvdb_buffer"]):
        bad.append(("nvdb_buffer", "tree bytes differ (%d of %d)" % (int((got["nvdb_buffer"] != ref["nvdb_buffer"]).sum()), ref["nvdb_buffer"].size)))
    for name in ["camera_" + f for f in FILTER_NAMES]:
        if need(name):
            g, r = got[name], ref[name]
            if ulp_diff(g[:, :4], r[:, :4]).max() > 8:          # wavelengths: atanh (Julia's libm vs the device's log2 / rcp form: 2 ulp achieved device vs oracle)
                bad.append((name, "lambda %d ulp" % ulp_diff(g[:, :4], r[:, :4]).max()))
            if not np.allclose(g[:, 4:8], r[:, 4:8], rtol=2e-5, atol=1e-9):
                bad.append((name, "wavelength pdf"))
            if ulp_diff(g[:, 8], r[:, 8]).max() > 2:
                bad.append((name, "filter weight %d ulp" % ulp_diff(g[:, 8], r[:, 8]).max()))
            if not np.array_equal(g[:, 9:12], r[:, 9:12]) or ulp_diff(g[:, 12:15], r[:, 12:15]).max() > 4:
                bad.append((name, "camera ray"))
    for name in ("uplift_bounded", "uplift_unbounded", "uplift_illuminant"):
        if need(name) and ulp_diff(got[name], ref[name]).max() > 2:
            bad.append((name, "%d ulp" % ulp_diff(got[name], ref[name]).max()))
    for k in range(N_MATERIALS):
        for name in ("bsdf_sample_%d_reg0" % k, "bsdf_sample_%d_reg1" % k, "bsdf_eval_%d" % k):
            if need(name):
                frac_close(name, slice(0, 10), 2e-4, 1e-6, 0.999)      # (a Fresnel-vs-uc knife edge may flip a lobe on a few rows)
    if need("lightbvh_nodes") and not np.allclose(got["lightbvh_nodes"], ref["lightbvh_nodes"], rtol=1e-6, atol=1e-7):
        bad.append(("lightbvh_nodes", "node array differs"))
    if need("lightbvh_choice"):
        same = got["lightbvh_choice"] == ref["lightbvh_choice"]
        if same.mean() < 0.999:
            bad.append(("lightbvh_choice", "%.5f of the choices agree" % same.mean()))
        elif need("lightbvh_pmf") and not np.allclose(got["lightbvh_pmf"][same], ref["lightbvh_pmf"][same], rtol=2e-5, atol=0):
            bad.append(("lightbvh_pmf", "pmf of the chosen light"))
    if need("lightbvh_query_pmf") and not np.allclose(got["lightbvh_query_pmf"], ref["lightbvh_query_pmf"], rtol=2e-5, atol=1e-12):
        bad.append(("lightbvh_query_pmf", "pmf of the queried light"))
    if need("light_sample"):
        g, r = got["light_sample"], ref["light_sample"]
        if not np.array_equal(g[:, 3] > 0, r[:, 3] > 0):
            bad.append(("light_sample", "accept / reject decisions differ"))
        elif not np.allclose(g, r, rtol=2e-5, atol=1e-6):
            bad.append(("light_sample", "max rel %.3g" % float(np.max(np.abs(g - r) / (np.abs(r) + 1e-6)))))
    for name in ("envlight_marginal_cdf", "envlight_conditional_cdf"):
        if need(name) and ulp_diff(got[name], ref[name]).max() > 2:
            bad.append((name, "%d ulp" % ulp_diff(got[name], ref[name]).max()))
    if need("envlight_sample"):
        g, r = got["envlight_sample"], ref["envlight_sample"]
        same = np.isclose(g, r, rtol=2e-5, atol=1e-6).all(axis=1).mean()
        if same < 0.999:      # (a sample within an ulp of a cdf entry may land in the neighbouring texel)
            bad.append(("envlight_sample", "%.5f of the rows agree" % same))
    if need("nvdb_sample_point") and not np.array_equal(got["nvdb_sample_point"], ref["nvdb_sample_point"]):
        bad.append(("nvdb_sample_point", "max abs %.3g" % float(np.abs(got["nvdb_sample_point"] - ref["nvdb_sample_point"]).max())))
    name = "frame_surfaces_64_spp4_depth5"
    if need(name):
        a, b = got[name].astype(np.float64), ref[name].astype(np.float64)
        rel_mse = float(np.mean((a - b) ** 2 / (b ** 2 + 1e-3)))
        d = np.sqrt(((a - b) ** 2).sum(axis=2)) / np.maximum(np.sqrt((b ** 2).sum(axis=2)), 1e-6)
        if not (np.isfinite(a).all() and rel_mse <= 1e-3 and (d <= 1e-2).mean() >= 0.99):
            bad.append((name, "relMSE %.3g, %.4f of the pixels within 1e-2 (SURVEY 8d: <= 1e-3, >= 0.99)" % (rel_mse, float((d <= 1e-2).mean()))))
    name = "frame_fog_32_spp1024_depth4"
    if need(name):
        a, b = got[name].astype(np.float64), ref[name].astype(np.float64)
        for c in range(3):
            if abs(a[..., c].sum() / b[..., c].sum() - 1.0) > 0.01:
                bad.append((name, "channel %d mean off by %.3f %%" % (c, 100 * (a[..., c].sum() / b[..., c].sum() - 1.0))))
    return bad


# ------------------------------------------------------------------------------------------------ child process: one side's outputs -> a directory
def _child(side, fixture_dir, out_dir, stages):
    IN = fixture_io.read_set(IN_DIR)
    got = compute(side, IN, stages)
    fixture_io.write_set(out_dir, got)


def run_side(side, fixture_dir, out_dir, stages=None):
    env = dict(os.environ)
    table = os.path.join(fixture_dir, "srgb_spectrum_table.dat")
    if os.path.isfile(table):
        env["HK_RGB2SPEC_TABLE"] = table
    cmd = [sys.executable, os.path.abspath(__file__), side, fixture_dir, out_dir] + (list(stages) if stages else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    return fixture_io.read_set(out_dir)


def _reference_or_skip():
    ref = fixture_io.read_set(REF_DIR)
    if not ref:
        pytest.skip("NO REFERENCE FIXTURES: tests/golden/reference/ is empty — julia/make_reference_fixtures.jl has never run (no Julia in the build image). "
                    "The oracle is NOT pinned to Hikari; run that script on a box with Julia + Hikari.jl and commit its output.")
    return ref


# ------------------------------------------------------------------------------------------------ tests
def test_inputs_are_what_the_script_writes(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_reference_inputs as M
    want = M.inputs()
    have = fixture_io.read_set(IN_DIR)
    assert set(want) == set(have)
    for k in want:
        assert want[k].dtype == have[k].dtype and np.array_equal(want[k], have[k]), k
    fixture_io.write_set(str(tmp_path), want)                      # the raw format round-trips
    back = fixture_io.read_set(str(tmp_path))
    assert all(np.array_equal(back[k], want[k]) and back[k].shape == want[k].shape for k in want)


def test_julia_generator_static():
    """Every `# ref: Hikari.<name> <file>:<line>` of the generator points at a definition of that name in the reference tree; every input it
    reads is committed; every array it writes is consumed by compare(); every stage it lists has a function."""
    src = open(JULIA).read()
    reads = set(re.findall(r'IN\["(\w+)"\]', src))
    assert reads and reads <= set(fixture_io.read_set(IN_DIR)), reads - set(fixture_io.read_set(IN_DIR))
    written = set()
    for m in re.finditer(r'put!\("([^"]+)"', src):
        name = m.group(1)
        if "$" in name:
            continue
        written.add(name)
    for k in range(N_MATERIALS):
        written |= {"bsdf_sample_%d_reg0" % k, "bsdf_sample_%d_reg1" % k, "bsdf_eval_%d" % k}
    written |= {"camera_" + f for f in FILTER_NAMES}
    assert 'put!("bsdf_sample_$(k - 1)_reg$(Int(regularize))"' in src and 'put!("bsdf_eval_$(k - 1)"' in src and 'put!("camera_" * name' in src
    assert len(re.findall(r"^    Hikari\.\w+Material\(|^    Hikari\.Gold\(", src, re.M)) == N_MATERIALS
    for f in FILTER_NAMES:
        assert '("%s", Hikari.' % f in src
    consumed = set(re.findall(r'"((?:sobol|nvdb|lightbvh|light|envlight|uplift|frame)_\w+)"', open(os.path.abspath(__file__)).read()))
    consumed |= {n for n in written if n.startswith(("bsdf_", "camera_"))}
    assert written <= consumed, written - consumed
    for s in re.search(r'stages = isempty\(ARGS\) \? \[([^\]]+)\]', src).group(1).replace('"', "").split(","):
        assert "function stage_%s()" % s.strip() in src, s
    refs = re.findall(r"# ref: Hikari\.(\w+) (\S+):(\d+)", src)
    assert len(refs) >= 30
    called = set(re.findall(r"Hikari\.(\w+)\(", src))
    cited = {r[0] for r in refs}
    stage_fns = {"zsobol_sample_1d", "zsobol_sample_2d", "compute_pixel_sample", "filter_sample", "sample_wavelengths_visible", "generate_ray", "uplift_rgb",
                 "uplift_rgb_unbounded", "uplift_rgb_illuminant", "sample_bsdf_spectral", "evaluate_bsdf_spectral", "bvh_sample_light", "bvh_pmf",
                 "sample_light_spectral", "nanovdb_get_value", "sample_point", "BVHLightSampler", "NanoVDBMedium", "VolPath", "EnvironmentMap", "EnvironmentLight"}
    assert stage_fns <= called and stage_fns <= cited, (stage_fns - called, stage_fns - cited)
    verified = {tuple(d) for d in json.load(open(REFERENCE_INDEX))["definitions"]}
    missing = {(name, rel, int(line)) for name, rel, line in refs} - verified
    assert not missing, ("citations not checked against the reference tree (tests/golden/make_reference_index.py)", sorted(missing))


def test_pipeline_runs_end_to_end_on_a_stand_in(tmp_path):
    """NOT a parity test: the oracle's own outputs are written as a fixture set, read back, and compared with a second run of the oracle
    in the child process — loaders, scene mirrors, every stage's hook and every comparison execute.  A planted error must be found."""
    import oracle as O
    O.build()
    stand_in = str(tmp_path / "stand_in")
    stages = ["sobol", "camera", "uplift", "bsdf", "lights", "envlight", "nanovdb", "frame"]
    ref = run_side("oracle", stand_in, stand_in, stages)
    assert {"sobol_1d", "camera_gaussian", "uplift_bounded", "bsdf_sample_7_reg1", "bsdf_eval_13", "lightbvh_choice", "light_sample", "nvdb_values",
            "nvdb_sample_point", "nvdb_buffer", "envlight_sample", "envlight_conditional_cdf"} <= set(ref)
    assert int(ref["lightbvh_counts"][2]) == 5 + 24 * 12 and (ref["lightbvh_pmf"] > 0).mean() > 0.9 and (ref["nvdb_values"] > 0).mean() > 0.1
    got = run_side("oracle", stand_in, str(tmp_path / "again"), stages)
    assert compare(got, ref) == []
    # planted errors: one ulp in a bit-exact stage, a wrong lobe in 1 % of the rows, a different light
    wrong = dict(got)
    wrong["sobol_1d"] = np.nextafter(got["sobol_1d"], f32(2))
    wrong["bsdf_sample_3_reg0"] = got["bsdf_sample_3_reg0"].copy()
    wrong["bsdf_sample_3_reg0"][::50, 3] += 0.5
    wrong["lightbvh_choice"] = got["lightbvh_choice"].copy()
    wrong["lightbvh_choice"][::100] += 1
    found = {n for n, _ in compare(wrong, ref)}
    assert {"sobol_1d", "bsdf_sample_3_reg0", "lightbvh_choice"} <= found, found


def test_oracle_against_reference_fixtures(tmp_path):
    ref = _reference_or_skip()
    import oracle as O
    O.build()
    got = run_side("oracle", REF_DIR, str(tmp_path / "oracle"))
    bad = compare(got, ref)
    assert not bad, bad


@pytest.mark.gpu
def test_device_against_reference_fixtures(tmp_path):
    ref = _reference_or_skip()
    got = run_side("device", REF_DIR, str(tmp_path / "device"))
    bad = compare(got, ref)
    assert not bad, bad


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:] or None)
