"""Light and environment-map edits without a device (-m "not gpu"): the host code path from light records to the device tables
(tests/native/light_rebuild_check.cpp, plain and under AddressSanitizer + UBSan), the Python mirror (Scene.update_light,
Scene.update_envmap, Scene.set_transform(move_lights=True)) and the ctypes stubs of the two entry points against the header."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import xform_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _native(tag, flags):
    exe = os.path.join(tempfile.gettempdir(), "hk_light_rebuild_check_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "light_rebuild_check.cpp"), os.path.join(csrc, "light_bvh.cpp")]
    deps = src + [os.path.join(csrc, "bvh_build.h"), os.path.join(ROOT, "include", "hikari_mi355x.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc] + flags + src + ["-o", exe])
    return exe


@pytest.mark.parametrize("tag,flags", [("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_light_tables_after_edits_equal_tables_from_scratch(tag, flags):
    """A few hundred random edit sequences over 1 .. 200 lights of mixed kinds: update-then-derive == derive-from-scratch, byte for
    byte, and every table fits the capacity hk_scene_create allocates (a stand-alone host program: no GPU, no Python process)."""
    r = subprocess.run([_native(tag, flags), "300", "11"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _light_bytes(d, i):
    return bytes(d.lights[i])


def test_update_light_goes_through_the_flat_order(hk):
    A = hk._abi
    s = hk.Scene()
    s.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(5.0)))          # lights[0] -> flat 0
    s.push(hk.AmbientLight(hk.RGBSpectrum(0.1)))                   # lights[1] -> flat 2
    s.push(hk.PointLight((1, 1, 0), hk.RGBSpectrum(2.0)))          # lights[2] -> flat 1 (type slots in first-seen order)
    d = s.desc
    assert [d.lights[i].kind for i in range(3)] == [A.HK_LIGHT_POINT, A.HK_LIGHT_POINT, A.HK_LIGHT_AMBIENT]
    assert [s._flat_index(i) for i in range(3)] == [0, 2, 1]
    before = [_light_bytes(d, i) for i in range(3)]
    new = hk.PointLight((3, 2, 1), hk.RGBSpectrum(7.0))
    s.update_light(2, new)
    assert s.desc is d and s.lights[2] is new                      # the kept description is rewritten, not rebuilt
    assert tuple(d.lights[1].position) == (3.0, 2.0, 1.0) and d.lights[1].i_rgb[0] == 7.0
    assert _light_bytes(d, 0) == before[0] and _light_bytes(d, 2) == before[2]
    s.update_light(1, hk.AmbientLight(hk.RGBSpectrum(0.5)))
    assert d.lights[2].i_rgb[0] == 0.5 and d.lights[2].kind == A.HK_LIGHT_AMBIENT
    # a fresh flatten of the edited scene gives the same records
    kept = [_light_bytes(d, i) for i in range(3)]
    s.sync()
    assert [_light_bytes(s.desc, i) for i in range(3)] == kept
    # refusals change nothing
    kept_lights = list(s.lights)
    with pytest.raises(TypeError):
        s.update_light(0, hk.AmbientLight(hk.RGBSpectrum(1.0)))    # another class
    with pytest.raises(IndexError):
        s.update_light(3, hk.PointLight((0, 0, 0), hk.RGBSpectrum(1.0)))
    with pytest.raises(IndexError):
        s.update_light(-1, hk.PointLight((0, 0, 0), hk.RGBSpectrum(1.0)))
    assert s.lights == kept_lights and [_light_bytes(s.desc, i) for i in range(3)] == kept
    # before the first sync there is no description: the light is swapped and flattened later
    t = hk.Scene()
    t.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(5.0)))
    t.update_light(0, hk.PointLight((0, 2, 0), hk.RGBSpectrum(5.0)))
    assert t.desc.lights[0].position[1] == 2.0


def test_update_light_recolours_an_emitter_and_refuses_a_new_texture(hk):
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd import lights as L
    s = hk.Scene()
    q = G.quad((-0.25, 1.98, -0.25), (0.25, 1.98, -0.25), (0.25, 1.98, 0.25), (-0.25, 1.98, 0.25), normal=(0, -1, 0))
    s.push(q, hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(6.0))))
    d = s.desc
    assert d.n_lights == 2
    old = s.lights[1]
    s.update_light(1, L.DiffuseAreaLight(old.vertices, old.normal, old.area, old.uv, hk.RGBSpectrum(1.0, 2.0, 3.0), 0.5, True))
    r = d.lights[1]
    assert tuple(r.Le.c)[:3] == (1.0, 2.0, 3.0) and r.scale == 0.5 and r.two_sided == 1 and r.Le.tex == -1
    tex = hk.Texture(np.ones((2, 2, 4), f32))
    with pytest.raises(ValueError):
        s.update_light(0, L.DiffuseAreaLight(old.vertices, old.normal, old.area, old.uv, tex, 1.0, False))
    assert s.textures == [] and d.lights[0].Le.tex == -1
    # update_material keeps refusing emission
    with pytest.raises(TypeError):
        s.update_material(0, hk.Emissive(Le=hk.RGBSpectrum(1.0)))


def _emissive(hk):
    return hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(3.0), scale=2.0))


def test_move_lights_gives_the_records_of_a_mesh_pushed_moved(hk):
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.geometry import Mesh
    mesh = G.sphere((0, 1.0, 0), 0.2, 6)
    M = X.affine(rot_deg=40, axis=(0.2, 1, 0.3), scale=1.3, translate=(0.3, -0.2, 0.1))
    a, b = hk.Scene(), hk.Scene()
    for s in (a, b):
        s.push(hk.PointLight((0, 1.9, 0), hk.RGBSpectrum(1.0)))
        s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    inst = a.push_instance(mesh, _emissive(hk))
    a.push(hk.PointLight((0, 0.2, 0), hk.RGBSpectrum(1.0)))         # a Point pushed later: the area lights are NOT a suffix of the flat order's prefix
    P, N, _ = X.transform_mesh(M[:3], mesh.positions, mesh.normals)
    b.push(Mesh(P, N, mesh.uvs), _emissive(hk))
    b.push(hk.PointLight((0, 0.2, 0), hk.RGBSpectrum(1.0)))
    da = a.desc
    created = [_light_bytes(da, i) for i in range(da.n_lights)]
    a.set_transform(inst, M)                                        # the default: the lights stay (Q18)
    assert [_light_bytes(da, i) for i in range(da.n_lights)] == created
    a.set_transform(inst, M, move_lights=True)
    db = b.desc
    assert a.desc is da and da.n_lights == db.n_lights == mesh.n_faces + 2
    assert [_light_bytes(da, i) for i in range(da.n_lights)] == [_light_bytes(db, i) for i in range(db.n_lights)]
    assert not [_light_bytes(da, i) for i in range(da.n_lights)] == created
    # a later flatten keeps them, and the identity brings the created ones back
    a.set_transform(inst, np.eye(4, dtype=f32), move_lights=True)
    assert [_light_bytes(da, i) for i in range(da.n_lights)] == created


def test_move_lights_keeps_a_degenerate_face_with_zero_area(hk):
    from hikari_jl_amd import geometry as G
    tri = G.quad((0, 0, 0), (0.1, 0, 0), (0.1, 0.1, 0), (0, 0.1, 0))
    s = hk.Scene()
    inst = s.push_instance(tri, _emissive(hk))
    d = s.desc
    assert d.n_lights == 2 and d.lights[0].area > 0
    tiny = X.affine(scale=1e-6, translate=(1, 2, 3))               # edges 1e-7: the cross product's length 1e-14 is under the 1e-10 cut-off
    normal = tuple(d.lights[0].normal)
    s.set_transform(inst, tiny, move_lights=True)
    moved = X.transform_points(tiny[:3], tri.positions)
    for i in range(2):
        assert d.lights[i].area == 0.0 and tuple(d.lights[i].normal) == normal
        assert np.array_equal(np.array(d.lights[i].v, f32).reshape(3, 3), moved[i])
    s.set_transform(inst, X.affine(scale=2.0), move_lights=True)    # and back into the tree with the next transform
    assert d.lights[0].area == pytest.approx(0.02)


def test_environment_map_update_is_in_place_and_equals_a_fresh_map(hk):
    from hikari_jl_amd import envmap as E
    rng = np.random.default_rng(3)
    old, new = rng.random((19, 37, 3)).astype(f32), rng.random((19, 37, 3)).astype(f32)
    new[4] = 0.0
    em = E.EnvironmentMap(old)
    s = hk.Scene()
    s.push(E.EnvironmentLight(em, hk.RGBSpectrum(1.0)))
    d = s.desc
    rec = d.envmaps[0]
    addr = [C.addressof(getattr(rec, n).contents) for n in ("data", "conditional_func", "conditional_cdf", "conditional_func_int", "marginal_func", "marginal_cdf")]
    R = E.rotation_matrix(30.0, (0, 0, 1))
    s.update_envmap(em, data=new, rotation=R)
    fresh_map = E.EnvironmentMap(new, R)                             # (kept alive: the record points into its arrays)
    fresh = fresh_map.record()
    assert addr == [C.addressof(getattr(rec, n).contents) for n in ("data", "conditional_func", "conditional_cdf", "conditional_func_int", "marginal_func", "marginal_cdf")]
    assert tuple(rec.rotation) == tuple(fresh.rotation) and rec.marginal_func_int == fresh.marginal_func_int
    sizes = {"data": 37 * 19 * 4, "conditional_func": 37 * 19, "conditional_cdf": 38 * 19, "conditional_func_int": 19, "marginal_func": 19, "marginal_cdf": 20}
    for n, k in sizes.items():
        assert np.array_equal(np.ctypeslib.as_array(getattr(rec, n), (k,)), np.ctypeslib.as_array(getattr(fresh, n), (k,))), n
    for bad in (dict(), dict(data=rng.random((19, 36, 3)).astype(f32)), dict(rotation=np.full((3, 3), np.nan, f32))):
        with pytest.raises(ValueError):
            s.update_envmap(em, **bad)
    with pytest.raises(ValueError):
        s.update_envmap(E.EnvironmentMap(old), rotation=R)          # a map of no light of this scene
    assert tuple(rec.rotation) == tuple(fresh.rotation)


CTYPES_OF = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.POINTER(C.c_float)}


def test_stubs_of_the_light_edit_entry_points_agree_with_the_header(hk, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    L = hk._lib.lib()
    ctypes_of = dict(CTYPES_OF)
    ctypes_of["const hk_light*"] = C.POINTER(hk._abi.hk_light)
    for name in ("hk_scene_update_lights", "hk_scene_update_envmap"):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]     # drop the parameter names
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [ctypes_of[a] for a in args], (name, args)
        assert name in hk._abi.EXPORTED_SYMBOLS
    # the records the two calls take, against gcc's layout
    fields = ["kind", "scale", "position", "world_to_light", "cos_total_width", "v", "area", "Le", "two_sided", "envmap"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hikari_mi355x.h"\nint main(){printf("%zu\\n", sizeof(hk_light));' +
                   "".join('printf("%%zu\\n", offsetof(hk_light, %s));' % f for f in fields) + "return 0;}")
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == C.sizeof(hk._abi.hk_light)
    assert out[1:] == [getattr(hk._abi.hk_light, f).offset for f in fields]


def test_julia_shim_forwards_the_two_entry_points():
    src = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()
    for needle in ("function update_light!(", "function update_envmap!(", "ccall((:hk_scene_update_lights, LIB)", "ccall((:hk_scene_update_envmap, LIB)"):
        assert needle in src, needle
