"""The light-BVH refit without a device (-m "not gpu"): the shared arithmetic and the host twin (tests/native/light_refit_check.cpp,
plain and under AddressSanitizer + UBSan), the Python mirror (Scene.update_light(s)(tree="refit"), set_transform / set_vertices
(move_lights="refit")), the ctypes stubs against the header, the Julia shim and the recorded figures."""
import ctypes as C
import json
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
    exe = os.path.join(tempfile.gettempdir(), "hk_light_refit_check_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "light_refit_check.cpp"), os.path.join(csrc, "light_bvh.cpp")]
    deps = src + [os.path.join(csrc, "bvh_build.h"), os.path.join(csrc, "hk_light_bounds.h"), os.path.join(ROOT, "include", "hikari_mi355x.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc] + flags + src + ["-o", exe])
    return exe


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "light_refit_bounds.json")))


@pytest.mark.parametrize("tag,flags", [("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_refit_twin_invariants_and_functions(tag, flags):
    """A few hundred random light sets and edit sequences: the invariants of a refit tree, an unchanged-records refit against the
    built tree, sequential against batched refits, the header's asin / acos / sin / cos against libm in double (a stand-alone host
    program: no GPU, no Python process).  The program's figures do not depend on the optimisation level (no contraction, no libm in
    the header), so both builds must print the recorded function errors."""
    r = subprocess.run([_native(tag, flags), "300", "11"], capture_output=True, text=True)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.startswith("ok"), (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = last.split()
    fig = {words[i]: float(words[i + 1]) for i in range(1, len(words) - 1, 2)}
    print(last)
    rec = _golden()["function_ulp"]
    for name in ("ulp_asin", "ulp_acos", "abs_sin_ulp1", "abs_cos_ulp1", "ulp_cos"):
        assert abs(fig[name] - rec[name]) < 2e-3, (name, fig[name], rec[name])
    assert fig["refit_residual"] <= 4 * fig["libm_residual"]
    nat = _golden()["native_check"]                          # the residuals come from host arithmetic alone: libm's in the built trees, the header's in the refit ones
    assert abs(fig["libm_residual"] / nat["cone_residual_libm_built"] - 1) < 1e-3 and abs(fig["refit_residual"] / nat["cone_residual_refit"] - 1) < 1e-3
    assert abs(fig["worst_ratio"] / nat["worst_ratio_per_tree"] - 1) < 1e-2


def test_recorded_figures_are_numbers():
    g = _golden()
    for key in ("cone_residual_libm_built", "cone_residual_refit", "relmse_refit_vs_fresh_256spp", "relmse_fresh_vs_fresh_256spp"):
        assert isinstance(g[key], float) and np.isfinite(g[key]) and g[key] >= 0, key
    assert g["cone_residual_refit"] <= 4 * g["cone_residual_libm_built"] and g["relmse_refit_vs_fresh_256spp"] <= 2 * g["relmse_fresh_vs_fresh_256spp"]
    for key, v in g["function_ulp"].items():
        assert key == "note" or (isinstance(v, float) and np.isfinite(v)), key


def _light_bytes(d, i):
    return bytes(d.lights[i])


class _Calls:
    """Stands in for the library: records the refit / update calls the mirror would make on a device scene."""

    def __init__(self, hk):
        self.calls = []
        self.A = hk._abi

    def hk_scene_refit_lights(self, h, n, idx, recs):
        self.calls.append(("refit", [idx[i] for i in range(n)], [bytes(recs[i]) for i in range(n)]))
        return 0

    def hk_scene_update_lights(self, h, first, n, recs):
        self.calls.append(("update", list(range(first, first + n)), [bytes(recs[i]) for i in range(n)]))
        return 0

    def hk_scene_destroy(self, h):
        return 0

    def hk_scene_set_transform(self, *a):
        self.calls.append(("transform",))
        return 0

    def hk_scene_set_vertices(self, *a):
        self.calls.append(("vertices",))
        return 0


@pytest.fixture
def fake_lib(hk, monkeypatch):
    calls = _Calls(hk)
    monkeypatch.setattr(hk._lib, "lib", lambda: calls)
    monkeypatch.setattr(hk._lib, "check", lambda status, what: None)
    return calls


def test_update_lights_refit_rewrites_the_description_and_sends_one_call(hk, fake_lib):
    A = hk._abi
    s = hk.Scene()
    s.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(5.0)))          # lights[0] -> flat 0
    s.push(hk.AmbientLight(hk.RGBSpectrum(0.1)))                   # lights[1] -> flat 2
    s.push(hk.PointLight((1, 1, 0), hk.RGBSpectrum(2.0)))          # lights[2] -> flat 1
    d = s.desc
    s._device = {"ctx": 1234}
    before = [_light_bytes(d, i) for i in range(3)]
    a, b = hk.PointLight((3, 2, 1), hk.RGBSpectrum(7.0)), hk.AmbientLight(hk.RGBSpectrum(0.5))
    s.update_lights([(2, a), (1, b)], tree="refit")
    assert s.desc is d and s.lights[2] is a and s.lights[1] is b
    assert tuple(d.lights[1].position) == (3.0, 2.0, 1.0) and d.lights[2].i_rgb[0] == 0.5 and _light_bytes(d, 0) == before[0]
    assert fake_lib.calls == [("refit", [1, 2], [_light_bytes(d, 1), _light_bytes(d, 2)])]          # flat indices, in the order given, ONE call
    del fake_lib.calls[:]
    s.update_light(0, hk.PointLight((0, 2, 0), hk.RGBSpectrum(5.0)), tree="refit")
    assert fake_lib.calls == [("refit", [0], [_light_bytes(d, 0)])] and d.lights[0].position[1] == 2.0
    del fake_lib.calls[:]
    s.update_light(0, hk.PointLight((0, 3, 0), hk.RGBSpectrum(5.0)))                                # the default is the rebuild
    assert [c[0] for c in fake_lib.calls] == ["update"]
    # a fresh flatten of the edited scene gives the same records: a scene created later has the fresh tree of these lights
    kept = [_light_bytes(d, i) for i in range(3)]
    s.sync()
    assert [_light_bytes(s.desc, i) for i in range(3)] == kept
    # refusals change nothing
    lights = list(s.lights)
    del fake_lib.calls[:]
    with pytest.raises(ValueError):
        s.update_lights([(0, hk.PointLight((0, 0, 0), hk.RGBSpectrum(1.0))), (0, hk.PointLight((1, 0, 0), hk.RGBSpectrum(1.0)))], tree="refit")
    with pytest.raises(ValueError):
        s.update_light(0, hk.PointLight((0, 0, 0), hk.RGBSpectrum(1.0)), tree="device")
    with pytest.raises(TypeError):
        s.update_light(0, hk.AmbientLight(hk.RGBSpectrum(1.0)), tree="refit")
    with pytest.raises(IndexError):
        s.update_lights([(3, hk.PointLight((0, 0, 0), hk.RGBSpectrum(1.0)))], tree="refit")
    assert s.lights == lights and [_light_bytes(s.desc, i) for i in range(3)] == kept and fake_lib.calls == []


def test_a_refit_the_library_refuses_leaves_the_mirror_untouched(hk, monkeypatch):
    s = hk.Scene()
    s.push(hk.PointLight((0, 1, 0), hk.RGBSpectrum(5.0)))
    d = s.desc
    s._device = {"ctx": 1234}

    class Refusing:
        def hk_scene_refit_lights(self, *a):
            return -1

        def hk_last_error(self):
            return b"the light would leave the light tree"

    monkeypatch.setattr(hk._lib, "lib", lambda: Refusing())
    kept, light = _light_bytes(d, 0), s.lights[0]
    with pytest.raises(hk._lib.HikariMI355XError):
        s.update_light(0, hk.PointLight((0, 1, 0), hk.RGBSpectrum(0.0)), tree="refit")
    assert _light_bytes(d, 0) == kept and s.lights[0] is light


def _emissive(hk):
    return hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(3.0), scale=2.0))


def test_move_lights_refit_sends_the_moved_records_in_one_call(hk, fake_lib):
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.geometry import Mesh
    mesh = G.sphere((0, 1.0, 0), 0.2, 6)
    M = X.affine(rot_deg=40, axis=(0.2, 1, 0.3), scale=1.3, translate=(0.3, -0.2, 0.1))
    a, b = hk.Scene(), hk.Scene()
    for s in (a, b):
        s.push(hk.PointLight((0, 1.9, 0), hk.RGBSpectrum(1.0)))
    inst = a.push_instance(mesh, _emissive(hk))
    a.push(hk.PointLight((0, 0.2, 0), hk.RGBSpectrum(1.0)))         # a Point pushed later: the area lights are not a suffix of the flat order
    P, N, _ = X.transform_mesh(M[:3], mesh.positions, mesh.normals)
    b.push(Mesh(P, N, mesh.uvs), _emissive(hk))
    b.push(hk.PointLight((0, 0.2, 0), hk.RGBSpectrum(1.0)))
    da, db = a.desc, b.desc
    a._device = {"ctx": 1}
    a.set_transform(inst, M, move_lights="refit")
    assert [_light_bytes(da, i) for i in range(da.n_lights)] == [_light_bytes(db, i) for i in range(db.n_lights)]
    assert [c[0] for c in fake_lib.calls] == ["transform", "refit"]
    idx = fake_lib.calls[1][1]
    assert sorted(idx) == list(range(2, 2 + mesh.n_faces)) and fake_lib.calls[1][2] == [_light_bytes(da, i) for i in idx]
    # new vertices: the same single call
    del fake_lib.calls[:]
    a.set_vertices(inst, mesh.positions * f32(1.1), move_lights="refit")
    assert [c[0] for c in fake_lib.calls] == ["vertices", "refit"] and len(fake_lib.calls[1][1]) == mesh.n_faces
    del fake_lib.calls[:]
    a.set_transform(inst, M, move_lights=True)                     # True keeps its meaning: rebuilds, one call per contiguous run
    assert [c[0] for c in fake_lib.calls] == ["transform", "update"]
    with pytest.raises(ValueError):
        a.set_transform(inst, M, move_lights="rebuild")


def test_move_lights_refit_refuses_a_degenerating_face_before_anything_moves(hk, fake_lib):
    from hikari_jl_amd import geometry as G
    tri = G.quad((0, 0, 0), (0.1, 0, 0), (0.1, 0.1, 0), (0, 0.1, 0))
    s = hk.Scene()
    inst = s.push_instance(tri, _emissive(hk))
    d = s.desc
    s._device = {"ctx": 1}
    kept, transforms = [_light_bytes(d, i) for i in range(2)], dict(s._transforms)
    tiny = X.affine(scale=1e-6, translate=(1, 2, 3))               # the moved edges' cross product falls under the 1e-10 cut-off: area 0
    with pytest.raises(ValueError):
        s.set_transform(inst, tiny, move_lights="refit")
    with pytest.raises(ValueError):
        s.set_vertices(inst, tri.positions * f32(1e-6), move_lights="refit")
    assert fake_lib.calls == [] and [_light_bytes(d, i) for i in range(2)] == kept and s._transforms == transforms
    s.set_transform(inst, tiny, move_lights=True)                  # the rebuild takes it
    assert [c[0] for c in fake_lib.calls] == ["transform", "update"] and d.lights[0].area == 0.0


CTYPES_OF = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32), "float*": C.POINTER(C.c_float),
             "uint32_t*": C.POINTER(C.c_uint32)}


def test_stubs_of_the_refit_entry_points_agree_with_the_header(hk):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read(), flags=re.S)
    L = hk._lib.lib()
    ctypes_of = dict(CTYPES_OF)
    ctypes_of["const hk_light*"] = C.POINTER(hk._abi.hk_light)
    for name in ("hk_scene_refit_lights", "hk_test_light_refit_host", "hk_test_light_table_copy"):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]     # drop the parameter names
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [ctypes_of[a] for a in args], (name, args)
        assert name in hk._abi.EXPORTED_SYMBOLS


def test_host_twin_entry_point_runs_without_a_device(hk):
    """hk_test_light_refit_host through ctypes: an unchanged-records refit keeps boxes, phi and cos_e; a refused edit is HK_ERR_INVALID."""
    A = hk._abi
    L = hk._lib.lib()
    s = hk.Scene()
    for i in range(5):
        s.push(hk.SpotLight((0.3 * i, 1.0, 0.1 * i), (0.1 * i, 0, 0.3), hk.RGBSpectrum(4.0 + i), 30.0, 10.0))
    s.push(hk.AmbientLight(hk.RGBSpectrum(0.1)))
    d = s.desc
    n = d.n_lights
    recs = (A.hk_light * n)(*[A.hk_light.from_buffer_copy(d.lights[i]) for i in range(n)])

    def run(n_calls, idx, new):
        nn = C.c_int32()
        nodes, trails, table = np.zeros((2 * n, 16), f32), np.zeros(n, np.uint32), np.zeros((2 * n, 16), np.uint32)
        st = L.hk_test_light_refit_host(recs, n, n_calls, (C.c_int32 * 1)(len(idx)), (C.c_int32 * max(len(idx), 1))(*idx), (A.hk_light * max(len(new), 1))(*new) if new else None,
                                        C.byref(nn), nodes.ctypes.data_as(A.PF), trails.ctypes.data_as(C.POINTER(C.c_uint32)), table.ctypes.data_as(C.POINTER(C.c_uint32)))
        return st, nodes[:nn.value], trails, table

    st, built, trails, table = run(0, [], [])
    assert st == 0 and len(built) == 9 and (trails == 0xFFFFFFFF).sum() == 1
    st, same, trails2, table2 = run(1, list(range(n)), [recs[i] for i in range(n)])
    assert st == 0 and np.array_equal(trails, trails2)
    assert np.array_equal(same[:, :6], built[:, :6]) and np.array_equal(same[:, 9], built[:, 9]) and np.array_equal(same[:, 11:], built[:, 11:])
    assert np.allclose(same[:, 6:11], built[:, 6:11], atol=2e-6)
    assert np.array_equal(table2[:, 12:14], table[:, 12:14])
    dark = A.hk_light.from_buffer_copy(recs[0])
    dark.i_rgb[0] = dark.i_rgb[1] = dark.i_rgb[2] = 0.0
    assert run(1, [0], [dark])[0] == A.HK_ERR_INVALID


def test_julia_shim_forwards_the_refit():
    src = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()
    for needle in ("function refit_lights!(", "tree::Symbol = :rebuild", "ccall((:hk_scene_refit_lights, LIB)", "tree === :refit"):
        assert needle in src, needle
