"""GPU parity tests (-m gpu): the HIP path, driven through the C-ABI, against the CPU oracle on the same
seeded inputs.  Bars: sub-kernels bit-exact or <= 2 ulp; traversal hit identity exact;
frames: relMSE <= 1e-3 and >= 99 % of pixels within 1e-2 relative L2 (tolerance is written in the test)."""
import ctypes as C

import numpy as np
import pytest

import ulp_bounds

pytestmark = pytest.mark.gpu


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def frame_metrics(gpu, ref):
    rel_mse = float(np.mean((gpu - ref) ** 2 / (ref ** 2 + 1e-3)))
    num = np.sqrt(((gpu - ref) ** 2).sum(axis=2))
    den = np.sqrt((ref ** 2).sum(axis=2)) + 1e-6
    frac_ok = float(np.mean(num / den <= 1e-2))
    return rel_mse, frac_ok


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_sobol_bit_exact(hk, oracle, gpu_ctx):
    rng = np.random.default_rng(11)
    n = 100000
    px = rng.integers(1, 1025, n).astype(np.int32)
    py = rng.integers(1, 1025, n).astype(np.int32)
    s = rng.integers(1, 4097, n).astype(np.int32)
    dim = rng.integers(1, 230, n).astype(np.int32)
    for spp in (4096, 8192):
        o1, o2 = oracle.sobol(1024, 1024, spp, 0, px, py, s, dim)
        g1 = np.empty(n, np.float32)
        g2 = np.empty((n, 2), np.float32)
        L = hk._lib.lib()
        hk._lib.check(L.hk_test_sobol(gpu_ctx.h, 1024, 1024, spp, 0, n, _pi(px), _pi(py), _pi(s), _pi(dim),
                                      g1.ctypes.data_as(hk._abi.PF), g2.ctypes.data_as(hk._abi.PF)), "hk_test_sobol")
        assert np.array_equal(o1, g1) and np.array_equal(o2, g2)


def test_uplift_le_2ulp(hk, oracle, gpu_ctx):
    rng = np.random.default_rng(12)
    n = 50000
    rgb = rng.random((n, 3), dtype=np.float32)
    rgb[:100] = rgb[:100, :1]          # grays
    rgb[100:200] *= 20.0               # > 1 (clamped by the bounded uplift, scaled by the others)
    lam = (360 + 470 * rng.random((n, 4), dtype=np.float32)).astype(np.float32)
    L = hk._lib.lib()
    for mode in (0, 1, 2):
        ref = oracle.uplift(mode, rgb, lam)
        out = np.empty_like(ref)
        hk._lib.check(L.hk_test_uplift(gpu_ctx.h, mode, n, rgb.ctypes.data_as(hk._abi.PF), lam.ctypes.data_as(hk._abi.PF),
                                       out.ctypes.data_as(hk._abi.PF)), "hk_test_uplift")
        assert ulp_diff(out, ref).max() <= 2, mode


def test_camera_stage(hk, oracle, gpu_ctx):
    """K1: wavelengths (atanh/cosh differ by <= a few ulp between glibc and the device libm), filter weight and ray."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cornell_box(800, 800)
    p = hk.integrator_params(max_depth=8, samples=256)
    rng = np.random.default_rng(13)
    n = 20000
    px = rng.integers(1, 801, n).astype(np.int32)
    py = rng.integers(1, 801, n).astype(np.int32)
    si = rng.integers(1, 257, n).astype(np.int32)
    ref = oracle.camera_samples(p, cam, 800, 800, px, py, si)
    L = hk._lib.lib()
    integ = C.c_void_p()
    hk._lib.check(L.hk_integrator_create(gpu_ctx.h, C.byref(p), C.byref(integ)), "hk_integrator_create")
    out = np.empty((n, 15), np.float32)
    rec = cam.record()
    hk._lib.check(L.hk_test_camera(gpu_ctx.h, integ, C.byref(rec), 800, 800, n, _pi(px), _pi(py), _pi(si), out.ctypes.data_as(hk._abi.PF)), "hk_test_camera")
    L.hk_integrator_destroy(integ)
    # the sampler's atanh / cosh go through the hardware's log2 / exp2 / rcp (hk_device.h: atanh_sampler, cosh_sampler); against a
    # float64 evaluation of the same formulas they must stay within 2.5e-4 nm (four float spacings at 540 nm) and 4e-6 relative
    print("camera stage: max |d lambda| = %.3g nm, max rel d pdf = %.3g (GPU vs oracle/glibc)" % (
        np.abs(out[:, :4] - ref[:, :4]).max(), (np.abs(out[:, 4:8] - ref[:, 4:8]) / np.maximum(ref[:, 4:8], 1e-12)).max()))
    ulp_bounds.check("camera/lambda", out[:, :4], ref[:, :4], floor=1.0)
    ulp_bounds.check("camera/lambda_pdf", out[:, 4:8], ref[:, 4:8], floor=1e-6)
    ulp_bounds.check("camera/filter_weight", out[:, 8], ref[:, 8], floor=1e-6)
    ulp_bounds.check("camera/ray_direction", out[:, 12:15], ref[:, 12:15], floor=1e-3)
    assert np.allclose(out[:, :4], ref[:, :4], rtol=0, atol=2.5e-4)          # lambda [nm]
    assert np.allclose(out[:, 4:8], ref[:, 4:8], rtol=4e-6, atol=1e-9)       # pdf (follows the 2-spacing difference in lambda)
    assert ulp_diff(out[:, 8], ref[:, 8]).max() <= 2                          # filter weight
    assert np.array_equal(out[:, 9:12], ref[:, 9:12])                         # ray origin (no lens): exact
    assert ulp_diff(out[:, 12:15], ref[:, 12:15]).max() <= 2                  # ray direction


def _random_rays(rng, n, lo, hi):
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


@pytest.mark.parametrize("which", ["cornell", "single", "integration"])
def test_closest_hit_parity_1M_rays(hk, oracle, gpu_ctx, which):
    """K3 traversal over the product's SAH BVH vs the oracle's median BVH: same
    (t, prim, bary) for 1 M random rays, including axis-aligned rays and rays grazing shared edges."""
    from hikari_jl_amd import scenes
    s, film, cam = {"cornell": scenes.cornell_box, "single": scenes.single_triangle, "integration": scenes.integration_test_scene}[which](64, 64)
    rng = np.random.default_rng(21)
    n = 1_000_000 if which == "cornell" else 200_000
    o, d = _random_rays(rng, n, np.array([-1.2, -0.2, -1.2]), np.array([1.2, 2.2, 1.2]))
    d[:1000] = np.array([0, -1, 0], np.float32)                  # axis-aligned
    d[1000:2000] = np.array([1, 0, 0], np.float32)
    tri = np.array(np.ctypeslib.as_array(s.desc.positions, shape=(s.desc.n_triangles * 9,))).reshape(-1, 3, 3)
    k = min(20000, n - 2000)
    tsel = rng.integers(0, tri.shape[0], k)
    e = rng.random(k)[:, None]
    target = tri[tsel, 0] * (1 - e) + tri[tsel, 1] * e            # points exactly on triangle edges
    dd = target - o[2000:2000 + k]
    d[2000:2000 + k] = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)
    tmax = np.full(n, np.inf, np.float32)
    tmax[::7] = rng.random(len(tmax[::7])).astype(np.float32) * 2.0
    rt, rp, ruv = oracle.OracleScene(s).trace(o, d, tmax)
    sh = hk.scene_handle(gpu_ctx, s)
    gt = np.empty(n, np.float32)
    gp = np.empty(n, np.int32)
    guv = np.empty((n, 2), np.float32)
    L = hk._lib.lib()
    hk._lib.check(L.hk_trace_closest(gpu_ctx.h, sh, n, o.ctypes.data_as(hk._abi.PF), d.ctypes.data_as(hk._abi.PF), tmax.ctypes.data_as(hk._abi.PF),
                                     gt.ctypes.data_as(hk._abi.PF), _pi(gp), guv.ctypes.data_as(hk._abi.PF)), "hk_trace_closest")
    assert (rp >= 0).mean() > 0.05
    assert np.array_equal(rp, gp)
    assert np.array_equal(rt, gt)
    assert np.array_equal(ruv, guv)


def test_light_bvh_parity(hk, oracle, gpu_ctx):
    """Light-BVH: identical tree (host builders are independent) and <= 2 ulp sample/pmf on the device."""
    from hikari_jl_amd import geometry as G
    rng = np.random.default_rng(31)
    s = hk.Scene()
    s.push(hk.PointLight((0.3, 1.5, 0.2), hk.RGBSpectrum(15.0)))
    s.push(hk.SpotLight((0.5, 1.9, -0.5), (0, 0, 0), hk.RGBSpectrum(30.0), 40.0, 30.0))
    s.push(hk.AmbientLight(hk.RGBSpectrum(0.1, 0.2, 0.4)))
    s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), hk.MatteMaterial())
    for i in range(40):  # emissive quads scattered in the box
        c = rng.random(3) * np.array([1.6, 1.6, 1.6]) + np.array([-0.8, 0.2, -0.8])
        q = G.quad(c, c + [0.1, 0, 0], c + [0.1, 0, 0.1], c + [0, 0, 0.1])
        s.push(q, hk.MediumInterface(hk.MatteMaterial(), emission=hk.Emissive(Le=hk.RGBSpectrum(*(0.2 + 0.8 * rng.random(3))), scale=1.0 + i % 3, two_sided=bool(i % 2))))
    s.sync()
    osc = oracle.OracleScene(s)
    on, ot = osc.light_bvh_nodes()
    sh = hk.scene_handle(gpu_ctx, s)
    L = hk._lib.lib()
    nn = C.c_int32()
    L.hk_scene_light_bvh_copy(sh, C.byref(nn), None, None)
    gn = np.zeros((nn.value, 16), np.float32)
    gtr = np.zeros(s.desc.n_lights, np.uint32)
    L.hk_scene_light_bvh_copy(sh, C.byref(nn), gn.ctypes.data_as(hk._abi.PF), gtr.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert gn.shape == on.shape and np.array_equal(gtr, ot)
    assert np.array_equal(gn[:, 12:15], on[:, 12:15])                         # topology identical
    assert ulp_diff(gn[:, :12], on[:, :12]).max() <= 4                        # cone unions go through acos/sin/cos
    n = 50000
    p = (rng.random((n, 3)) * 2 - 1).astype(np.float32) + np.array([0, 1, 0], np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[:500] = 0                                                             # medium scattering: n = 0
    u = rng.random(n, dtype=np.float32)
    q = rng.integers(1, s.desc.n_lights + 1, n).astype(np.int32)
    rl, rpmf, rq = osc.light_bvh(p, nrm, u, q)
    gl = np.empty(n, np.int32)
    gpmf = np.empty(n, np.float32)
    gq = np.empty(n, np.float32)
    hk._lib.check(L.hk_test_light_bvh(gpu_ctx.h, sh, n, p.ctypes.data_as(hk._abi.PF), nrm.ctypes.data_as(hk._abi.PF), u.ctypes.data_as(hk._abi.PF),
                                      _pi(gl), gpmf.ctypes.data_as(hk._abi.PF), _pi(q), gq.ctypes.data_as(hk._abi.PF)), "hk_test_light_bvh")
    same = gl == rl
    assert same.mean() > 0.999                                                # a 1-ulp node difference may flip a knife-edge choice
    assert np.allclose(gpmf[same], rpmf[same], rtol=2e-5, atol=0)
    assert np.allclose(gq, rq, rtol=2e-5, atol=1e-12)
    # achieved accuracy against its recorded bound (the pmf is a product of up to ~8 importance ratios, each a quotient of sums)
    ulp_bounds.check("light_bvh/pmf_of_choice", gpmf[same], rpmf[same], floor=1e-12)
    ulp_bounds.check("light_bvh/pmf_of_query", gq, rq, floor=1e-12)
    assert len(set(gl.tolist())) > 20


FRAME_CASES = [
    ("single", dict(max_depth=4, samples=16), (80, 60)),
    ("cornell_area", dict(max_depth=8, samples=8), (96, 96)),
    ("cornell_point", dict(max_depth=5, samples=8), (64, 64)),
    ("cornell_two_spheres", dict(max_depth=8, samples=8), (64, 64)),   # SURVEY 8(d)'s own Cornell geometry (3 782 triangles: the BVH no longer fits the LDS node cache whole)
    ("integration_nofog", dict(max_depth=5, samples=4), (64, 64)),
    ("many_light", dict(max_depth=4, samples=4), (64, 64)),   # config 5 in miniature: 48 k triangles, ~2.5 k area lights in the light BVH
    ("textured", dict(max_depth=1, samples=8), (64, 64)),   # deeper: alpha tests / coated walks re-seed from ray bits -> statistical case below
]

# Scenes with participating media.  The reference seeds its delta-tracking / ratio-tracking RNGs by hashing the
# BIT PATTERNS of ray origins and directions (delta-tracking.jl:28-45, intersection.jl:455): a 1-ulp libm
# difference in a scattered direction (sinf/cosf on glibc vs the device) re-seeds the stream and the path
# diverges into a statistically equivalent one.  Per-pixel identity is therefore impossible for these paths on
# ANY two platforms (including the reference's own CPU vs GPU back-ends); parity is statistical: the GPU frame
# must be as close to the oracle frame A as an independent oracle frame B (other sample indices) is.
MEDIA_CASES = [
    ("integration", dict(max_depth=4, samples=32), (48, 48)),
    ("slab_homogeneous", dict(max_depth=6, samples=64), (24, 24)),
    ("slab_absorbing", dict(max_depth=6, samples=16), (24, 24)),
    ("slab_grid", dict(max_depth=6, samples=64), (24, 24)),
    ("textured", dict(max_depth=5, samples=32), (40, 40)),
    ("slab_rgbgrid", dict(max_depth=6, samples=64), (24, 24)),
    ("slab_rgbgrid_absorbing", dict(max_depth=6, samples=16), (24, 24)),
    ("cloud_nanovdb", dict(max_depth=12, samples=32), (40, 40)),
    ("cloud_grid", dict(max_depth=12, samples=32), (40, 40)),
]


def _scene(name, w, h):
    from hikari_jl_amd import scenes
    if name == "single":
        return scenes.single_triangle(w, h)
    if name == "cornell_area":
        return scenes.cornell_box(w, h, light="area")
    if name == "cornell_point":
        return scenes.cornell_box(w, h, light="point")
    if name == "cornell_two_spheres":
        return scenes.cornell_box(w, h, light="area", objects="two_spheres")
    if name == "integration_nofog":
        return scenes.integration_test_scene(w, h, with_fog=False)
    if name == "textured":
        return scenes.textured_scene(w, h)
    if name == "many_light":
        return scenes.many_light_scene(w, h, n_boxes=4000)
    if name == "slab_homogeneous":
        import hikari_jl_amd as hk
        return scenes.slab_scene(w, h, hk.HomogeneousMedium(sigma_a=hk.RGBSpectrum(0.2, 0.3, 0.1), sigma_s=hk.RGBSpectrum(0.8, 0.6, 0.9), Le=hk.RGBSpectrum(0.05, 0.0, 0.0), g=0.4))
    if name == "slab_absorbing":
        import hikari_jl_amd as hk
        return scenes.slab_scene(w, h, hk.HomogeneousMedium(sigma_a=hk.RGBSpectrum(0.7, 0.9, 1.2), sigma_s=hk.RGBSpectrum(0.0), Le=hk.RGBSpectrum(0.1, 0.05, 0.0)))
    if name == "slab_grid":
        import hikari_jl_amd as hk
        import numpy as np
        rng = np.random.default_rng(5)
        dens = (rng.random((12, 10, 6)) ** 2).astype(np.float32) * 3.0
        return scenes.slab_scene(w, h, hk.GridMedium(dens, sigma_a=hk.RGBSpectrum(0.1), sigma_s=hk.RGBSpectrum(1.0, 0.9, 0.8), g=-0.2,
                                                    bounds=((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0)), majorant_res=(4, 4, 2)))
    if name in ("slab_rgbgrid", "slab_rgbgrid_absorbing"):
        import hikari_jl_amd as hk
        import numpy as np
        rng = np.random.default_rng(11)
        sa = (rng.random((10, 8, 6, 3)) * np.array([0.6, 0.9, 1.3])).astype(np.float32)
        ss = (rng.random((10, 8, 6, 3)) ** 2 * np.array([2.0, 1.6, 1.2])).astype(np.float32)
        le = (rng.random((10, 8, 6, 3)) * np.array([0.3, 0.1, 0.02])).astype(np.float32)
        if name == "slab_rgbgrid_absorbing":
            ss = np.zeros_like(ss)
        return scenes.slab_scene(w, h, hk.RGBGridMedium(sigma_a_grid=sa, sigma_s_grid=ss, Le_grid=le, sigma_scale=1.5, Le_scale=0.8, g=0.3,
                                                       bounds=((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0)), majorant_res=(4, 4, 2)))
    if name == "cloud_nanovdb":
        return scenes.cloud_scene(w, h, "nanovdb", res=(48, 48, 24))
    if name == "cloud_grid":
        return scenes.cloud_scene(w, h, "grid", res=(48, 48, 24))
    return scenes.integration_test_scene(w, h)


@pytest.mark.parametrize("name,kw,res", FRAME_CASES)
def test_frame_parity(hk, oracle, name, kw, res):
    """Whole-frame parity, same seed (0), same spp.  Tolerance: relMSE <= 1e-3 and >= 99 % of
    pixels with relative L2 over RGB <= 1e-2.  (In practice the two agree to ~1e-6 except at the few pixels
    where an atanh/cosh/sin/cos ulp flips a branch.)"""
    w, h = res
    s, film, cam = _scene(name, w, h)
    p = hk.integrator_params(**kw)
    acc, ost = oracle.OracleScene(s).render(p, cam, w, h, kw["samples"])
    ref = oracle.finalize(acc, w, h)
    vp = hk.VolPath(**kw)
    vp(s, film, cam)
    rel_mse, frac_ok = frame_metrics(film.framebuffer, ref)
    assert np.isfinite(film.framebuffer).all()
    assert rel_mse <= 1e-3 and frac_ok >= 0.99, (name, rel_mse, frac_ok)
    st = vp.stats()
    # same work: identical ray counts up to the few flipped branches
    assert abs(int(st.rays_closest) - int(ost.rays_closest)) <= 0.002 * ost.rays_closest + 4
    assert abs(int(st.rays_shadow) - int(ost.rays_shadow)) <= 0.002 * ost.rays_shadow + 4
    # samples_per_pass is a pure scheduling knob: 1 sample/pass == auto
    film2 = hk.Film((w, h))
    vp2 = hk.VolPath(samples_per_pass=1, **kw)
    vp2(s, film2, cam)
    assert np.array_equal(film2.framebuffer, film.framebuffer)
    vp.close()
    vp2.close()


from test_layered_materials import MATERIAL_NAMES, material as _material_pair


def _material(hk, name):
    return _material_pair(hk, name)


@pytest.mark.parametrize("name", MATERIAL_NAMES)
def test_material_frame_parity(hk, oracle, name):
    """Row a18.  ThinDielectric / DiffuseTransmission / CoatedConductor are closed-form per vertex: strict parity at every
    depth.  The two LayeredBxDF kinds run a PCG32 walk seeded from the BIT PATTERNS of wo_local / wi_local
    (spectral-eval.jl:1316, :1636): strict parity wherever those are bit-identical (first vertex from the camera: depth 1,
    and all but the layered->layered second vertices at depth 2); deeper, a 1-ulp libm difference in an incoming direction
    re-seeds the walk, so the comparison is statistical there (GPU far closer to oracle frame A than an independent oracle
    frame B is)."""
    from hikari_jl_amd import scenes
    w = h = 48
    m, panel = _material(hk, name)
    s, film, cam = scenes.material_scene(w, h, m, thin_panel=panel)
    osc = oracle.OracleScene(s)
    walk = name.startswith("cd")

    def dist(x, y):
        return float(np.mean((x - y) ** 2 / (0.25 * (x + y) ** 2 + 1e-2)))

    for depth, spp in ((1, 8), (2, 8), (5, 16)):
        kw = dict(max_depth=depth, samples=spp)
        p = hk.integrator_params(**kw)
        acc, ost = osc.render(p, cam, w, h, spp)
        A = oracle.finalize(acc, w, h)
        vp = hk.VolPath(**kw)
        vp(s, film, cam)
        G = film.framebuffer.copy()
        st = vp.stats()
        vp.close()
        assert np.isfinite(G).all() and (G >= 0).all()
        rel_mse, frac_ok = frame_metrics(G, A)
        if not walk or depth == 1:
            assert rel_mse <= 1e-3 and frac_ok >= 0.99, (name, depth, rel_mse, frac_ok)
        elif depth == 2:
            assert rel_mse <= 1e-2 and frac_ok >= 0.92, (name, depth, rel_mse, frac_ok)
        else:
            accB, _ = osc.render(p, cam, w, h, spp, first=spp + 1)
            B = oracle.finalize(accB, w, h)
            d_ab, d_ga = dist(A, B), dist(G, A)
            assert d_ga <= 0.25 * d_ab + 1e-4, (name, depth, d_ga, d_ab)
            for c in range(3):
                assert abs(G[..., c].mean() - A[..., c].mean()) <= 0.01 * A[..., c].mean() + 1e-3, (name, c)
        assert abs(int(st.rays_closest) - int(ost.rays_closest)) <= 0.005 * ost.rays_closest + 8
        assert abs(int(st.rays_shadow) - int(ost.rays_shadow)) <= 0.005 * ost.rays_shadow + 8


@pytest.mark.parametrize("name,kw,res", MEDIA_CASES)
def test_media_frame_parity_statistical(hk, oracle, name, kw, res):
    w, h = res
    n = kw["samples"]
    s, film, cam = _scene(name, w, h)
    p = hk.integrator_params(**kw)
    osc = oracle.OracleScene(s)
    accA, ostA = osc.render(p, cam, w, h, n, first=1)
    accB, _ = osc.render(p, cam, w, h, n, first=n + 1)
    A, B = oracle.finalize(accA, w, h), oracle.finalize(accB, w, h)
    vp = hk.VolPath(**kw)
    vp(s, film, cam)
    G = film.framebuffer.copy()
    assert np.isfinite(G).all() and (G >= 0).all()

    def dist(x, y):
        return float(np.mean((x - y) ** 2 / (0.25 * (x + y) ** 2 + 1e-2)))

    d_ab, d_ga = dist(A, B), dist(G, A)
    assert d_ga <= 1.5 * d_ab + 1e-4, (name, d_ga, d_ab)           # GPU is no farther from A than an independent oracle frame
    for c in range(3):                                              # and unbiased: channel means agree within 3 %
        assert abs(G[..., c].mean() - A[..., c].mean()) <= 0.03 * A[..., c].mean() + 1e-3, (name, c, G[..., c].mean(), A[..., c].mean())
    st = vp.stats()
    assert abs(int(st.rays_closest) - int(ostA.rays_closest)) <= 0.03 * ostA.rays_closest + 8
    assert int(st.rays_shadow) <= int(ostA.rays_shadow) * 1.03 + 8   # opaque early-exit can only save shadow segments
    if name in ("slab_absorbing", "slab_rgbgrid_absorbing"):        # no scattering => no re-seeding => strict parity holds
        rel_mse, frac_ok = frame_metrics(G, A)
        assert rel_mse <= 1e-3 and frac_ok >= 0.99, (rel_mse, frac_ok)
        assert int(st.medium_collisions) == int(ostA.medium_collisions)
    vp.close()


def test_progressive_and_sharded_rendering(hk):
    """render! adds one sample on top of the accumulators (volpath.jl:488-499); sample-index sharding
     over strided index sets reproduces the single-device film up to fp32 summation order."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cornell_box(64, 64, light="area")
    vp = hk.VolPath(max_depth=6, samples=8)
    vp(s, film, cam)
    full = film.framebuffer.copy()
    acc_full = vp.read_accumulators(film)
    film2 = hk.Film((64, 64))
    vp2 = hk.VolPath(max_depth=6, samples=8)
    vp2._ensure(film2)
    vp2.clear()
    for _ in range(8):
        vp2.render(s, film2, cam)
    assert film2.iteration_index == 8
    assert np.array_equal(film2.framebuffer, full)
    parts = []
    for rank in range(2):
        f = hk.Film((64, 64))
        v = hk.VolPath(max_depth=6, samples=8)
        v._ensure(f)
        v.clear()
        v.render_samples(s, f, cam, 4, stride=2, first=rank + 1, readback=False)
        parts.append(v.read_accumulators(f))
        v.close()
    assert np.allclose(parts[0] + parts[1], acc_full, rtol=1e-5, atol=1e-6)
    vp.close()
    vp2.close()


@pytest.mark.parametrize("which", ["cornell", "cloud", "sky"])
def test_progressive_calls_pipeline_bit_equal(hk, knobs, which):
    """64 one-sample calls (render!, volpath.jl:445-450) with no read-back in between are BATCHED (hk_render_tile notes small calls that
    continue each other and renders them as one pass when something looks) or, with HK_BATCH_PATHS_M=0 and HK_PIPELINE > 1, run PIPELINED on
    the library's lanes (hk_ctx::Lane: consecutive small calls beside each other, film kernels chained in call order): the accumulators
    equal, bit for bit, those of the same calls rendered at once, one after the other, of the one-shot 64-sample frame, and of a mix of
    call sizes; statistics add up; a clear in the middle is ordered behind the calls before it."""
    from hikari_jl_amd import scenes
    w, h, n = 40, 36, 64
    if which == "cornell":
        s, film, cam = scenes.cornell_box(w, h, light="area")
        depth = 6
    elif which == "cloud":
        s, film, cam = scenes.cloud_scene(w, h, "nanovdb", res=(48, 48, 24))
        depth = 8
    else:
        s, film, cam = scenes.sky_scene(w, h, env_res=32)
        depth = 6

    def run(env, plan):
        knobs.delenv("HK_PIPELINE", raising=False)
        knobs.delenv("HK_BATCH_PATHS_M", raising=False)
        knobs.setenv("HK_PIPELINE_AFTER", "0")     # (the lanes start with the first small call, not after a run of four)
        for k, v in env.items():
            knobs.setenv(k, v)
        vp = hk.VolPath(max_depth=depth, samples=n)
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        first = 1
        for k in plan:
            vp.render_samples(s, film, cam, k, first=first, readback=False)
            first += k
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        vp.close()
        # (a scene with media casts one extra ray per rendered PASS: the camera-medium detection, intersection.jl:690-747 — one per call
        # when every call is rendered at once, fewer when small calls are batched: then the closest-hit count is left out)
        batched = env.get("HK_BATCH_PATHS_M", "32") != "0"
        closest = -1 if (which == "cloud" and batched) else int(st.rays_closest) - (len(plan) if which == "cloud" else 0)
        return acc, (closest, int(st.rays_shadow), int(st.medium_collisions), int(st.path_vertices))

    off = {"HK_BATCH_PATHS_M": "0"}                       # every call rendered at once, one after the other: the reference
    ref, rays = run({**off, "HK_PIPELINE": "1"}, [1] * n)
    assert np.isfinite(ref).all() and ref.max() > 0
    for env, plan in (({}, [1] * n), ({}, [1, 2, 1, 28, 1, 1, 30]), ({"HK_BATCH_PATHS_M": "1"}, [1] * n), ({}, [n]),      # small calls batched (the default)
                      ({**off, "HK_PIPELINE": "7"}, [1] * n), ({**off, "HK_PIPELINE": "2"}, [1, 2, 1, 28, 1, 1, 30]), ({**off, "HK_PIPELINE": "8"}, [3] * 20 + [4]),
                      ({**off, "HK_PIPELINE": "8", "HK_PIPELINE_AFTER": "4"}, [1] * n)):                                   # ... or run beside each other on lanes
        got, r2 = run(env, plan)
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), (env, plan[:4])
        assert r2[1:] == rays[1:] and (r2[0] < 0 or r2[0] == rays[0]), (env, r2, rays)
    # a clear between pipelined calls: what is rendered before it is gone, what comes after it is all there
    for env in ({}, {**off, "HK_PIPELINE": "8"}):
        knobs.delenv("HK_PIPELINE", raising=False)
        knobs.delenv("HK_BATCH_PATHS_M", raising=False)
        knobs.setenv("HK_PIPELINE_AFTER", "0")
        for k, v in env.items():
            knobs.setenv(k, v)
        vp = hk.VolPath(max_depth=depth, samples=n)
        vp._ensure(film)
        vp.clear()
        for i in range(8):
            vp.render_samples(s, film, cam, 1, first=100 + i, readback=False)
        vp.clear()
        for i in range(n):
            vp.render_samples(s, film, cam, 1, first=i + 1, readback=False)
        got = vp.read_accumulators(film).copy()
        vp.close()
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), env
    knobs.delenv("HK_PIPELINE", raising=False)
    knobs.delenv("HK_BATCH_PATHS_M", raising=False)


def test_readback_every_call_and_pipelined(hk, knobs):
    """What an interactive viewer does (volpath.jl:617-633 writes the frame after every sample): one-sample calls, each followed by the
    frame.  hk_film_read_rgb through the pinned path (the same host buffer every time: registered from the second call on) and the
    hk_film_read_rgb_async / hk_film_read_wait pair (frame i while call i + 1 renders) must hand out, bit for bit, the frames of the
    plain loop 'render one sample, read the frame into fresh memory'; with HK_READBACK_PIN=0 too."""
    from hikari_jl_amd import scenes
    w, h, n = 40, 36, 12
    s, film, cam = scenes.cornell_box(w, h, light="area")

    def loop(mode, pin=None):
        if pin is not None:
            knobs.setenv("HK_READBACK_PIN", pin)
        vp = hk.VolPath(max_depth=5, samples=n)
        vp._ensure(film)
        vp.clear()
        frames = []
        for i in range(n):
            vp.render_samples(s, film, cam, 1, first=i + 1, readback=mode)
            if mode == "fresh":
                vp._readback = None                      # a new destination every call: never pinned
                vp.read_framebuffer(film)
            frames.append(np.array(film.framebuffer, copy=True))
        if mode == "pipelined":
            vp.finish_pipelined(film)
            frames.append(np.array(film.framebuffer, copy=True))
        acc = vp.read_accumulators(film).copy()
        vp.close()
        knobs.delenv("HK_READBACK_PIN")
        return frames, acc

    ref, acc_ref = loop("fresh")
    assert np.isfinite(ref[-1]).all() and ref[-1].max() > 0 and not np.array_equal(ref[0], ref[-1])
    # "view" names its one buffer with hk_film_pin_host (the copy lands there directly); HK_READBACK_PIN=1 is round 5's automatic
    # registration of a destination that comes twice in a row; without either the frame goes through the film's staging buffers
    for mode, pin in (("view", None), ("view", "1"), (True, "1"), (True, None)):
        got, acc = loop(mode, pin)
        assert np.array_equal(acc.view(np.uint32), acc_ref.view(np.uint32)), (mode, pin)
        for i in range(n):
            assert np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32)), (mode, pin, i)
    got, acc = loop("pipelined")
    assert np.array_equal(acc.view(np.uint32), acc_ref.view(np.uint32))
    for i in range(1, n + 1):        # after call i the film shows frame i - 1; finish_pipelined brings the last one in
        assert np.array_equal(got[i].view(np.uint32), ref[i - 1].view(np.uint32)), i


def test_lane_pipeline_rebuilds_the_sample_bit_table_behind_the_lanes(hk, knobs):
    """with HK_PIPELINE >= 2 and batching off, consecutive small calls of >= 16 samples each rebuild the sample-bit
    table in the SAME buffer; a lane may still be drawing from the old one.  [16, 16, 16, 16] at samples = 256 must equal the same
    calls rendered one after the other, bit for bit, and repeatedly."""
    from hikari_jl_amd import scenes
    w, h = 48, 40
    s, film, cam = scenes.cornell_box(w, h, light="area")

    def run(env, plan):
        for k in ("HK_PIPELINE", "HK_BATCH_PATHS_M", "HK_PIPELINE_AFTER"):
            knobs.delenv(k)
        for k, v in env.items():
            knobs.setenv(k, v)
        vp = hk.VolPath(max_depth=6, samples=256)
        vp._ensure(film)
        vp.clear()
        first = 1
        for k in plan:
            vp.render_samples(s, film, cam, k, first=first, readback=False)
            first += k
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    plan = [16, 16, 16, 16, 32, 16]
    ref = run({"HK_BATCH_PATHS_M": "0", "HK_PIPELINE": "1"}, plan)
    for rep in range(3):
        for lanes in ("2", "4"):
            got = run({"HK_BATCH_PATHS_M": "0", "HK_PIPELINE": lanes, "HK_PIPELINE_AFTER": "0"}, plan)
            assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), (rep, lanes)
    for k in ("HK_PIPELINE", "HK_BATCH_PATHS_M", "HK_PIPELINE_AFTER"):
        knobs.delenv(k)


_EXTERNAL_ACCUM_SCRIPT = r"""
import sys
import numpy as np
import torch                                             # first: torch brings its own HIP runtime, which has to be the one the process initialises
sys.path[:0] = [%r, %r]
import hikari_jl_amd as hk
from hikari_jl_amd import scenes
w, h = 32, 32
s, film, cam = scenes.cornell_box(w, h, light="area")
accum = torch.zeros(4 * w * h, dtype=torch.float32, device="cuda")
vp = hk.VolPath(max_depth=4, samples=4)
vp.use_external_accumulators(accum.data_ptr())
vp._ensure(film)
vp.clear()
vp.sync()
for i in range(4):
    vp.render_samples(s, film, cam, 1, first=i + 1, readback=False)
torch.cuda.synchronize()                                 # no hk_* call in between: the caller's own ordering
seen = accum.cpu().numpy().copy()
assert seen[3 * w * h:].min() > 0, "a pixel is missing samples"
assert np.array_equal(seen.view(np.uint32), vp.read_accumulators(film).view(np.uint32))
vp.close()
own = hk.VolPath(max_depth=4, samples=4)                 # the same calls into a library-owned film (batched): identical sums
own._ensure(film)
own.clear()
for i in range(4):
    own.render_samples(s, film, cam, 1, first=i + 1, readback=False)
assert np.array_equal(seen.view(np.uint32), own.read_accumulators(film).view(np.uint32))
own.close()
print("external accumulators ok")
"""


def test_small_calls_into_external_accumulators_are_stream_ordered():
    """hk_render's ordering contract: a film with EXTERNAL accumulators (a torch tensor the host reduces) is never only noted — after
    the call, work the caller orders behind the stream (torch.cuda.synchronize()) sees the samples without any hk_* call in between.
    (A process of its own: torch has to initialise the GPU before the library does, as in bench.py.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _EXTERNAL_ACCUM_SCRIPT % (root, os.path.join(root, "oracle"))], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "external accumulators ok" in out.stdout, out.stderr[-2000:]


def test_context_options(hk, gpu_ctx, monkeypatch):
    """hk_ctx_set_option / hk_ctx_get_option: knobs live in the context; the environment is read by hk_ctx_create only."""
    L = hk._lib.lib()
    assert L.hk_ctx_set_option(gpu_ctx.h, b"HK_NO_SUCH_KNOB", b"1") == hk._abi.HK_ERR_INVALID and b"unknown option" in L.hk_last_error()
    assert L.hk_ctx_set_option(gpu_ctx.h, None, b"1") == hk._abi.HK_ERR_INVALID
    before = gpu_ctx.get_option("HK_WAVES_PER_CU")
    monkeypatch.setenv("HK_WAVES_PER_CU", "7")           # after the context exists: not seen
    assert gpu_ctx.get_option("HK_WAVES_PER_CU") == before
    with gpu_ctx.options(HK_WAVES_PER_CU=5):
        assert gpu_ctx.get_option("HK_WAVES_PER_CU") == "5"
    assert gpu_ctx.get_option("HK_WAVES_PER_CU") == before
    fresh = hk.Context(0)                                # a new context picks the environment up once
    try:
        assert fresh.get_option("HK_WAVES_PER_CU") == "7"
    finally:
        L.hk_ctx_destroy(fresh.h)
    gpu_ctx.flush()
    gpu_ctx.trim_cache()


def test_converged_image_within_mc_variance(hk, oracle):
    """SURVEY 8(d) converged-image check: a 256-spp GPU frame of sample indices the oracle never saw (1025..1280) against the
    oracle's 1024-spp frame (indices 1..1024).  Both estimate the same image, so their relMSE is var/256 + var/1024; var/256 is
    measured on the oracle itself (its two 512-sample halves differ by var/512 + var/512).  Bound: 2 x that figure."""
    from hikari_jl_amd import scenes
    w = h = 32
    kw = dict(max_depth=6, samples=1024)
    s, film, cam = scenes.cornell_box(w, h, light="area")
    p = hk.integrator_params(**kw)
    osc = oracle.OracleScene(s)
    a1, _ = osc.render(p, cam, w, h, 512, first=1)
    a2, _ = osc.render(p, cam, w, h, 512, first=513)
    half1, half2 = oracle.finalize(a1, w, h), oracle.finalize(a2, w, h)
    ref = oracle.finalize(a1 + a2, w, h)
    vp = hk.VolPath(**kw)
    vp._ensure(film)
    vp.clear()
    vp.render_samples(s, film, cam, 256, stride=1, first=1025, readback=True)
    gpu = film.framebuffer.copy()
    vp.close()
    osc.close()
    def rel_mse(a, b):
        return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-3)))
    var_256 = rel_mse(half1, half2)
    got = rel_mse(gpu, ref)
    assert np.isfinite(gpu).all() and var_256 > 0
    assert got <= 2.0 * var_256, (got, var_256)
    # and no bias: the mean radiance agrees within 3 standard errors of the 256-sample mean
    assert abs(gpu.mean() - ref.mean()) <= 3.0 * np.sqrt(var_256 / gpu.size) * max(ref.mean(), 1e-3) + 1e-3 * ref.mean()


def test_full_size_properties(hk):
    """BASELINE config 2 at full size (800x800, depth 8) on a few samples: size-independent properties —
    finite, non-negative, deterministic re-render, weight sum == spp * filter integral."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cornell_box(800, 800, light="area")
    vp = hk.VolPath(max_depth=8, samples=4)
    vp(s, film, cam)
    a = film.framebuffer.copy()
    acc = vp.read_accumulators(film)
    assert np.isfinite(a).all() and (a >= 0).all() and a.mean() > 0.05
    vp(s, film, cam)
    assert np.array_equal(a, film.framebuffer)
    w = acc[3 * 640000:]
    assert np.allclose(w, w[0], rtol=1e-2) and w[0] > 0
    st = vp.stats()
    assert st.rays_closest >= 4 * 640000
    # a pass this size of a small closed scene takes the static stride on one stream (hk_render.cpp ensure_state, "mid"); the tickets and
    # the second stream of a full-size pass must give the same film, bit for bit
    with hk.Context.get(0).options(HK_MID_PASS_PATHS_M=0):
        vp(s, film, cam)
    assert np.array_equal(a, film.framebuffer)
    vp.close()


def test_error_behaviour(hk, gpu_ctx):
    L = hk._lib.lib()
    p = hk.integrator_params(max_depth=0)
    h = C.c_void_p()
    assert L.hk_integrator_create(gpu_ctx.h, C.byref(p), C.byref(h)) == hk._abi.HK_ERR_INVALID
    assert b"max_depth" in L.hk_last_error()
    with pytest.raises(AssertionError):
        hk.VolPath(material_coherence="bogus")


@pytest.mark.parametrize("tonemap", [None, "reinhard", "reinhard_extended", "aces", "uncharted2", "filmic"])
def test_postprocess_parity(hk, oracle, gpu_ctx, tonemap):
    """postprocess! on the device (hk_postprocess / Film.postprocess) vs the oracle: same kernel arguments, <= 2e-6 absolute
    (powf ulps); sensor white balance and the escaped-ray background mask included."""
    from hikari_jl_amd.postprocess import make_params
    rng = np.random.default_rng(4)
    film = hk.Film((37, 23))
    film.framebuffer[...] = (rng.random((23, 37, 3)) ** 3 * 6).astype(np.float32)
    film.depth = np.where(rng.random((23, 37)) < 0.3, np.inf, 1.0).astype(np.float32)
    kw = dict(exposure=1.3, tonemap=tonemap, gamma=2.2, white_point=3.0, sensor=hk.FilmSensor(iso=90, white_balance=5000), background=(0.1, 0.2, 0.3))
    got = film.postprocess(**kw)
    ref = oracle.postprocess(make_params(**kw), film.framebuffer, film.depth)
    assert got.shape == (23, 37, 3) and np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 2e-6, np.abs(got - ref).max()
    got2 = film.postprocess(exposure=1.0, tonemap=tonemap, gamma=None)
    assert np.abs(got2 - oracle.postprocess(make_params(exposure=1.0, tonemap=tonemap, gamma=None), film.framebuffer)).max() <= 1e-6


def test_aux_buffers_parity(hk, oracle, gpu_ctx):
    """fill_aux_buffers! (src/film.jl:410-483): first-hit normal / depth / albedo per pixel centre, GPU == oracle (depth and
    normal bit-exact: same intersection arithmetic), and the escaped mask they feed into postprocess."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.sky_scene(48, 40, env_res=16, tess=16, analytic=True)
    film.fill_aux_buffers(s, cam)
    a, n, d = oracle.OracleScene(s).fill_aux(cam, 48, 40)
    assert film.depth.shape == (40, 48) and np.array_equal(film.depth, d) and np.array_equal(film.normal, n) and np.array_equal(film.albedo, a)
    assert np.isinf(d).any() and (d[np.isfinite(d)] > 0).all() and set(np.unique(a)) == {np.float32(0.0), np.float32(0.8)}
    film.fill_aux_buffers(s, cam, has_infinite_lights=True)
    assert not np.isinf(film.depth).any() and (film.depth.max() == np.float32(1e30))


def test_edge_cases(hk, oracle):
    """Empty / ragged inputs: a scene without triangles, a scene without lights, film sizes that are not multiples
    of the 8x8 tile (incl. 1x1), sample counts that are not multiples of samples_per_pass, depth 1 — all against the oracle."""
    from hikari_jl_amd import geometry as G
    from test_gpu_parity import frame_metrics

    def both(s, cam, w, h, **kw):
        film = hk.Film((w, h))
        vp = hk.VolPath(**kw)
        vp(s, film, cam)
        st = vp.stats()
        vp.close()
        kw.pop("samples_per_pass", None)
        acc, ost = oracle.OracleScene(s).render(hk.integrator_params(**kw), cam, w, h, kw["samples"])
        return film.framebuffer.copy(), oracle.finalize(acc, w, h), st, ost

    # no geometry, one ambient light: every ray escapes at depth 0
    s = hk.Scene()
    s.push(hk.AmbientLight(hk.RGBSpectrum(0.2, 0.4, 0.8)))
    s.sync()
    cam = hk.PerspectiveCamera((0, 0, -3), (0, 0, 0), hk.Film((13, 7)), fov=40.0)
    g, r, st, ost = both(s, cam, 13, 7, max_depth=3, samples=5, samples_per_pass=2)
    # (the oracle, like render!, probes the camera medium once per sample: +1 cast each; the device decides it once per call and only
    #  when the scene has media, the result being a constant of the scene)
    assert np.isfinite(g).all() and g.mean() > 0 and frame_metrics(g, r)[1] == 1.0 and st.rays_closest == 13 * 7 * 5 and ost.rays_closest == 13 * 7 * 5 + 5
    # geometry but no lights at all: black, and no shadow rays
    s = hk.Scene()
    s.push(G.rect3f((-1, -1, 0), (2, 2, 0.1)), hk.MatteMaterial())
    s.sync()
    g, r, st, ost = both(s, cam, 13, 7, max_depth=4, samples=3)
    assert not g.any() and not r.any() and st.rays_shadow == 0
    # 1x1 film, depth 1, a single sample
    s, _, _ = __import__("hikari_jl_amd").scenes.cornell_box(8, 8, light="point")
    cam1 = hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), hk.Film((1, 1)), fov=40.0)
    g, r, st, ost = both(s, cam1, 1, 1, max_depth=1, samples=1)
    assert g.shape == (1, 1, 3) and np.allclose(g, r, rtol=1e-4, atol=1e-6) and st.rays_closest == 1
    # ragged film (not a multiple of 8 in either direction) and ragged pass count (7 samples, 3 per pass)
    cam2 = hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), hk.Film((21, 11)), fov=40.0)
    g, r, st, ost = both(s, cam2, 21, 11, max_depth=5, samples=7, samples_per_pass=3)
    rel_mse, frac = frame_metrics(g, r)
    assert rel_mse <= 1e-3 and frac >= 0.98 and abs(int(st.rays_closest) - int(ost.rays_closest)) <= 0.01 * ost.rays_closest + 4


def test_full_size_media_properties(hk):
    """BASELINE configs[3] stand-in at full size (1024^2, depth 32) on one sample: finite, non-negative, deterministic re-render,
    collision counter consistent between two renders, weight sum == filter integral."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cloud_scene(1024, 1024, "nanovdb", res=(128, 128, 64), sigma_scale=60.0)
    vp = hk.VolPath(max_depth=32, samples=1)
    vp(s, film, cam)
    a = film.framebuffer.copy()
    c1 = int(vp.stats().medium_collisions)
    assert np.isfinite(a).all() and (a >= 0).all() and a.mean() > 0.01 and c1 > 1_000_000
    vp(s, film, cam)
    assert np.array_equal(a, film.framebuffer) and int(vp.stats().medium_collisions) == c1
    vp.close()


def test_small_pass_in_one_launch(hk, knobs):
    """k_small_pass: a small pass of a closed all-matte scene — the reference's interactive call, one sample of every pixel (volpath.jl:445-450)
    — is ONE launch in which the wave that owns a segment runs the camera rays and every bounce's trace / shade / shadow stage of that
    segment (a path never leaves its segment).  The accumulators must equal, bit for bit, those of the same calls rendered as launches
    (HK_SMALL_PASS_FUSED=0), for one-sample calls and for a 24-sample pass, with an odd segment count too; hk_stats says which way was
    taken; scenes with Mirror / Glass / Conductor surfaces or escape lights take the GENERAL instantiation, and scenes that are not its
    case (a layered kind, media) keep the launches.  Inside it the shadow rays of a bounce
    and the rays of the next one share one refill loop (trace_shadow_body; HK_SMALL_PASS_MERGED=0: two stages)."""
    from hikari_jl_amd import scenes
    w, h = 72, 56

    def run(scene, cam, film, env, plan, depth=7, eltype="Float32"):
        for k in ("HK_SMALL_PASS_FUSED", "HK_WAVES_PER_CU", "HK_SMALL_PASS_WAVES", "HK_SMALL_PASS_MERGED"):
            knobs.delenv(k, raising=False)
        knobs.setenv("HK_BATCH_PATHS_M", "0")              # every call rendered at once
        for k, v in env.items():
            knobs.setenv(k, v)
        vp = hk.VolPath(max_depth=depth, samples=64, accumulation_eltype=eltype)
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        first = 1
        for k in plan:
            vp.render_samples(scene, film, cam, k, first=first, readback=False)
            first += k
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        vp.close()
        return acc, st

    for objects in ("sphere_box", "two_spheres"):
        s, film, cam = scenes.cornell_box(w, h, light="area", objects=objects)
        for plan in ([1] * 6, [24], [1, 3, 1]):
            ref, st0 = run(s, cam, film, {"HK_SMALL_PASS_FUSED": "0"}, plan)
            assert int(st0.fused_passes) == 0 and int(st0.trace_launches) == 7 * len(plan)
            assert np.isfinite(ref).all() and ref.max() > 0
            for env in ({}, {"HK_SMALL_PASS_WAVES": "4"}, {"HK_SMALL_PASS_WAVES": "16"}, {"HK_WAVES_PER_CU": "3"}, {"HK_SMALL_PASS_MERGED": "0"}, {"HK_SMALL_PASS_MERGED": "0", "HK_SMALL_PASS_WAVES": "16"}):      # (256- / 512-thread blocks of k_small_pass, the launches at 16 per CU, an odd segment count)
                got, st1 = run(s, cam, film, env, plan)
                if max(plan) == 1 and env.get("HK_SMALL_PASS_WAVES") != "16":      # (larger passes have their Sobol draws in tables — k_shade's table-only instantiation —
                    assert int(st1.fused_passes) == len(plan) and int(st1.trace_launches) == 0, (env, plan)     # and keep the launches; so do 16 segments per CU)
                assert int(st1.fused_passes) * 7 + int(st1.trace_launches) == 7 * len(plan)
                assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), (objects, env, plan)
                assert (int(st1.rays_closest), int(st1.rays_shadow), int(st1.hits_accepted), int(st1.path_vertices)) == \
                       (int(st0.rays_closest), int(st0.rays_shadow), int(st0.hits_accepted), int(st0.path_vertices))
    # a Float64 film (the one-sample pass adds its paths to the film inside the launch: film_tile<double>)
    s, film, cam = scenes.cornell_box(w, h, light="area")
    ref, st0 = run(s, cam, film, {"HK_SMALL_PASS_FUSED": "0"}, [1] * 5, eltype="Float64")
    got, st1 = run(s, cam, film, {}, [1] * 5, eltype="Float64")
    assert ref.dtype == np.float64 and int(st1.fused_passes) == 5 and int(st0.fused_passes) == 0 and np.array_equal(ref.view(np.uint64), got.view(np.uint64))
    # the GENERAL instantiation (Matte under any lights, Mirror, Glass, Conductor; K7 for escape lights): the sky scene (glass sphere, gold
    # slab, environment map + sun), the box with a rough conductor / a glass / a mirror object, every light kind at once
    R = hk.RGBSpectrum
    cases = [scenes.sky_scene(w, h, env_res=32),
             scenes.cornell_box(w, h, light="area", object_material=hk.ConductorMaterial(roughness=0.2)),
             scenes.cornell_box(w, h, light="all", object_material=hk.GlassMaterial(Kr=R(1.0), Kt=R(1.0), index=1.5)),
             scenes.cornell_box(w, h, light="both", object_material=hk.MirrorMaterial(Kr=R(0.9)))]
    # ... and the many-light barrel: >= 64 lights in the light BVH (the launches choose the next-event light in k_light_select; inside
    # k_small_pass the shade body descends itself), once with a tree of at most 16 levels and once deeper (32-entry stacks)
    cases.append(scenes.many_light_scene(w, h, n_boxes=500, emissive_frac=0.25, box_scale=8.0))
    cases.append(scenes.many_light_scene(w, h, n_boxes=20000, emissive_frac=0.05, box_scale=2.0))
    for s, film, cam in cases:
        for plan in ([1] * 4, [2, 1]):
            ref, st0 = run(s, cam, film, {"HK_SMALL_PASS_FUSED": "0"}, plan)
            assert int(st0.fused_passes) == 0 and np.isfinite(ref).all() and ref.max() > 0
            for env in ({}, {"HK_SMALL_PASS_WAVES": "4"}, {"HK_SMALL_PASS_MERGED": "0"}):
                got, st1 = run(s, cam, film, env, plan)
                if max(plan) == 1:
                    assert int(st1.fused_passes) == len(plan), (env, plan)
                assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), (env, plan)
                assert (int(st1.rays_closest), int(st1.rays_shadow), int(st1.hits_accepted), int(st1.path_vertices)) == \
                       (int(st0.rays_closest), int(st0.rays_shadow), int(st0.hits_accepted), int(st0.path_vertices))
            # HK_SMALL_PASS_FUSED=1: only the all-matte instantiation; 16 segments per CU: the general one does not fit four waves per SIMD
            assert int(run(s, cam, film, {"HK_SMALL_PASS_FUSED": "1"}, plan)[1].fused_passes) == 0
            got, st1 = run(s, cam, film, {"HK_SMALL_PASS_WAVES": "16"}, plan)
            assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    s, film, cam = scenes.cornell_box(w, h, light="point")          # a point light only: still the all-matte case
    ref, st0 = run(s, cam, film, {"HK_SMALL_PASS_FUSED": "0"}, [1, 1])
    got, st1 = run(s, cam, film, {"HK_SMALL_PASS_FUSED": "1"}, [1, 1])
    assert int(st1.fused_passes) == 2 and np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    # not its case: a layered kind, a medium
    s, film, cam = scenes.cornell_box(w, h, light="area", object_material=hk.CoatedDiffuseMaterial())
    assert int(run(s, cam, film, {}, [1, 1])[1].fused_passes) == 0
    s, film, cam = scenes.cloud_scene(w, h, "grid", res=(24, 24, 12))
    assert int(run(s, cam, film, {}, [1, 1], depth=5)[1].fused_passes) == 0
    for k in ("HK_SMALL_PASS_FUSED", "HK_WAVES_PER_CU", "HK_SMALL_PASS_WAVES", "HK_SMALL_PASS_MERGED", "HK_BATCH_PATHS_M"):
        knobs.delenv(k, raising=False)
    # HK_WAVES_PER_CU is not sticky any more (the envs after {"HK_WAVES_PER_CU": "3"} above used to run at 3 segments per CU):
    # with the knob unset the default policy applies again
    s, film, cam = scenes.cornell_box(w, h, light="area")
    assert int(run(s, cam, film, {}, [1])[1].fused_passes) == 1


@pytest.mark.parametrize("which", ["cornell", "textured", "sky", "manylight", "mix"])
def test_packed_triangle_records_are_result_neutral(hk, knobs, which):
    """Round 6: the shade kernels read a triangle's positions / vertex normals / uvs / meta from ONE 128-byte record (DScene::tri_shade)
    instead of four arrays.  Same values, same arithmetic: films bit-identical to HK_TRI_PACK=0 (the knob is read when the scene is
    created, so each side builds its own scene) — meshes with and without vertex normals and uvs, textures (uv-dependent), the
    many-light barrel (light selection reads the surface too), a Mix material (resolved from uv in the trace flush)."""
    from hikari_jl_amd import scenes
    w, h = 40, 32

    def build():
        if which == "cornell":
            return scenes.cornell_box(w, h, light="all", objects="two_spheres") + (dict(max_depth=6, samples=16),)
        if which == "textured":
            return scenes.textured_scene(w, h) + (dict(max_depth=5, samples=16),)
        if which == "sky":
            return scenes.sky_scene(w, h, env_res=32) + (dict(max_depth=8, samples=16),)
        if which == "manylight":
            return scenes.many_light_scene(w, h, n_boxes=500, emissive_frac=0.25, box_scale=8.0) + (dict(max_depth=5, samples=16),)
        from test_parity_holes import _mix_scene
        return _mix_scene(hk, frame=True, w=w, h=h) + (dict(max_depth=6, samples=16),)

    def run(pack):
        knobs.setenv("HK_TRI_PACK", pack)            # (the default builds the records from 32 768 triangles up: these scenes are smaller)
        s, film, cam, kw = build()
        vp = hk.VolPath(**kw)
        vp(s, film, cam)
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        vp.close()
        return acc, (int(st.rays_closest), int(st.rays_shadow), int(st.path_vertices))

    a, ca = run("0")
    b, cb = run("1")
    assert np.isfinite(a).all() and a.max() > 0 and ca == cb, (ca, cb)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), float(np.abs(a - b).max())
    knobs.delenv("HK_TRI_PACK")
