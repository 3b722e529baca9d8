"""Scene edits on the host (CPU): the NumPy reference of hk_scene_set_transform's arithmetic, Scene.push_instance ranges, the argument
checks of Scene.set_transform / Scene.update_material (raised before any device call), the C prototypes, and the library's own
refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import xform_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _rng_affines(rng, n):
    return [X.affine(rng.uniform(0, 360), rng.normal(size=3), rng.uniform(0.2, 5.0), rng.uniform(-10, 10, 3))[:3] for _ in range(n)]


def test_identity_copies_exactly():
    rng = np.random.default_rng(1)
    p = rng.normal(size=(500, 3, 3)).astype(f32)
    p[0, 0] = (-0.0, 0.0, -0.0)
    n = rng.normal(size=(500, 3, 3)).astype(f32)
    P, N, T = X.transform_mesh(X.IDENTITY, p, n, n)
    assert P.tobytes() == p.tobytes() and N.tobytes() == n.tobytes() and T.tobytes() == n.tobytes()   # -0 stays -0 (arithmetic would give +0)


def test_translation_is_an_exact_add():
    rng = np.random.default_rng(2)
    p = rng.uniform(-4, 4, (2000, 3)).astype(f32)
    t = np.array([0.375, -1.25, 3.0625], f32)
    m = X.IDENTITY.copy()
    m[:, 3] = t
    assert np.array_equal(X.transform_points(m, p), p + t)


def test_points_agree_with_float64():
    """Three rounded products and three rounded sums: |p' - exact| <= 4 * 2^-24 * (sum_j |m[k][j] x_j| + |m[k][3]|), i.e. at most 4 ulp
    of that magnitude (measured worst: 1.95).  Relative to the result itself no bound exists (cancellation)."""
    rng = np.random.default_rng(3)
    for m in _rng_affines(rng, 20):
        p = rng.uniform(-3, 3, (20000, 3)).astype(f32)
        q = X.transform_points(m, p).astype(np.float64)
        m64 = m.astype(np.float64)
        exact = p.astype(np.float64) @ m64[:, :3].T + m64[:, 3]
        mag = np.abs(p.astype(np.float64)) @ np.abs(m64[:, :3]).T + np.abs(m64[:, 3])
        assert (np.abs(q - exact) <= 4 * np.spacing(mag.astype(f32)).astype(np.float64)).all()


def test_normals_are_unit_to_two_ulp():
    rng = np.random.default_rng(4)
    for m in _rng_affines(rng, 20):
        n = rng.normal(size=(20000, 3)).astype(f32)
        out = X.transform_dirs(X.normal_matrix(m), n).astype(np.float64)
        assert (np.abs(np.linalg.norm(out, axis=1) - 1.0) <= 2 * np.spacing(f32(1))).all()
        # the normal matrix is the inverse transpose: transformed normals stay perpendicular to transformed tangent directions
        e = rng.normal(size=(20000, 3)).astype(np.float64)
        e -= (e * n).sum(1, keepdims=True) * n / (n.astype(np.float64) ** 2).sum(1, keepdims=True)
        e2 = e @ m[:, :3].astype(np.float64).T
        cos = np.abs((out * e2).sum(1)) / np.linalg.norm(e2, axis=1)
        assert cos.max() < 1e-5


def test_nan_normals_pass_through():
    m = X.affine(30, (1, 2, 3), 2.0, (1, 1, 1))[:3]
    n = np.full((4, 3, 3), np.nan, f32)
    _, N, _ = X.transform_mesh(m, np.zeros((4, 3, 3), f32), n)
    assert np.isnan(N).all()


def test_singular_transform_is_refused():
    m = np.eye(4, dtype=f32)
    m[2, 2] = 0.0
    with pytest.raises(ValueError):
        X.normal_matrix(m[:3])
    from hikari_jl_amd.scene import _affine_3x4
    with pytest.raises(ValueError, match="singular"):
        _affine_3x4(m)
    bad_row = np.eye(4, dtype=f32)
    bad_row[3, 0] = 1.0
    with pytest.raises(ValueError, match="last row"):
        _affine_3x4(bad_row)
    inf = np.eye(4, dtype=f32)
    inf[0, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        _affine_3x4(inf)


def _scene(hk):
    from hikari_jl_amd import geometry as G
    s = hk.Scene()
    a = s.push_instance(G.rect3f((0, 0, 0), (1, 1, 1)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))
    b = s.push(G.sphere((0, 0, 0), 0.5, 8), hk.GlassMaterial(index=1.5))
    c = s.push_instance(G.sphere((1, 0, 0), 0.3, 6), hk.ConductorMaterial(roughness=0.2), transform=X.affine(translate=(0, 1, 0)))
    d = s.push_instance(G.rect3f((0, 0, 0), (1, 1, 1)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.2)))
    return s, a, b, c, d


def test_push_instance_ranges(hk):
    from hikari_jl_amd import geometry as G
    s, a, b, c, d = _scene(hk)
    n_sphere8 = G.sphere((0, 0, 0), 0.5, 8).n_faces
    n_sphere6 = G.sphere((1, 0, 0), 0.3, 6).n_faces
    assert (a.first_tri, a.n_tris) == (0, 12)
    assert (c.first_tri, c.n_tris) == (12 + n_sphere8, n_sphere6)
    assert (d.first_tri, d.n_tris) == (12 + n_sphere8 + n_sphere6, 12)
    assert s.desc.n_triangles == 24 + n_sphere8 + n_sphere6
    # the description carries the instance UN-transformed; the transform waits for hk_scene_create
    P = np.ctypeslib.as_array(s.desc.positions, shape=(s.desc.n_triangles, 3, 3))
    assert np.array_equal(P[c.first_tri:c.first_tri + c.n_tris], G.sphere((1, 0, 0), 0.3, 6).positions)
    assert set(s._transforms) == {(c.first_tri, c.n_tris)}
    assert isinstance(b, int) and c.mi_idx != a.mi_idx


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("device call %s made before the arguments were checked" % name)


def test_argument_errors_come_before_any_device_call(hk, monkeypatch):
    s, a, b, c, d = _scene(hk)
    s.desc
    s._device = {0: C.c_void_p(1)}                # as if a device scene existed: any library call would be a bug
    monkeypatch.setattr(hk._lib, "lib", lambda: _NoDevice())
    try:
        with pytest.raises(ValueError):
            s.set_transform(a, np.zeros((4, 4), f32))                           # singular, last row wrong
        with pytest.raises(ValueError):
            s.set_transform(a, np.eye(3, dtype=f32))                            # not 4x4
        with pytest.raises(TypeError):
            s.set_transform((0, 12), np.eye(4, dtype=f32))                      # not an instance
        with pytest.raises(ValueError):
            s.set_transform(hk.scene.SceneInstance(0, 10 ** 6, 12), np.eye(4, dtype=f32))
        with pytest.raises(TypeError):
            s.update_material(a.mi_idx, hk.GlassMaterial())                     # another type
        with pytest.raises(IndexError):
            s.update_material(99, hk.MatteMaterial())
        with pytest.raises(ValueError, match="texture"):
            s.update_material(a.mi_idx, hk.MatteMaterial(Kd=hk.Texture(np.ones((4, 4, 4), f32))))   # a texture the scene does not hold
        with pytest.raises(ValueError, match="opaque"):
            s.update_material(a.mi_idx, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5, 0.5, 0.5, 0.5)))   # alpha < 1: another opacity class
        with pytest.raises(TypeError):
            s.update_material(a.mi_idx, hk.Emissive())
        assert len(s.textures) == 0 and len(s.spectra) == 0
        assert s.materials[s.media_interfaces[a.mi_idx][0]].Kd.c[0] == f32(0.5)
    finally:
        s._device = {}


def test_update_material_rewrites_the_kept_description(hk):
    s, a, b, c, d = _scene(hk)
    s.desc
    s.update_material(a.mi_idx, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.1, 0.2, 0.3)))
    i = s.media_interfaces[a.mi_idx][0]
    assert tuple(s.desc.materials[i].rgb[0].c) == (f32(0.1), f32(0.2), f32(0.3), 1.0)
    s.sync()                                                                  # a later sync keeps the update
    assert tuple(s.desc.materials[i].rgb[0].c) == (f32(0.1), f32(0.2), f32(0.3), 1.0)


def test_prototypes_compile_c99(tmp_path):
    src = tmp_path / "edit.c"
    src.write_text('#include "hikari_mi355x.h"\n'
                   "int use(hk_scene* s, const hk_material* m) {\n"
                   "    static const float id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};\n"
                   "    int32_t (*f)(hk_scene*, int32_t, int32_t, const float*) = hk_scene_set_transform;\n"
                   "    int32_t (*g)(hk_scene*, int32_t, int32_t, const hk_material*) = hk_scene_update_materials;\n"
                   "    return f(s, 0, 1, id) + g(s, 0, 1, m);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "edit.o")])


def test_library_refuses_null_arguments_without_a_device(hk):
    if not os.path.isfile(hk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = hk._lib.lib()
    m = X.IDENTITY.copy()
    assert L.hk_scene_set_transform(None, 0, 1, m.ctypes.data_as(hk._abi.PF)) == hk._abi.HK_ERR_INVALID
    assert b"null" in L.hk_last_error()
    rec = hk._abi.hk_material()
    assert L.hk_scene_update_materials(None, 0, 1, C.byref(rec)) == hk._abi.HK_ERR_INVALID
