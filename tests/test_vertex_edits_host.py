"""Vertex edits without a device (-m "not gpu"): the Python mirror (Scene.set_vertices rewrites the kept mesh and the kept description,
with move_lights=True the light records too), its ValueErrors, the ctypes prototypes of the three new entry points against the header,
and the host arithmetic of hk_scene_set_vertices / hk_scene_bvh_cost (tests/native/vertex_edit_check.cpp, plain and under
AddressSanitizer + UBSan: a stand-alone program, nothing sanitised is loaded into Python)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import vertex_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _native(tag, flags):
    exe = os.path.join(tempfile.gettempdir(), "hk_vertex_edit_check_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "vertex_edit_check.cpp")]
    deps = src + [os.path.join(csrc, "hk_edit_host.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", csrc] + flags + src + ["-o", exe])
    return exe


@pytest.mark.parametrize("tag,flags", [("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_block_boxes_and_tree_cost_on_the_host(tag, flags):
    """Random edit sequences over block sizes 1 / 7 / 64 / 1024: every block box contains its triangles, whole blocks exactly, a
    non-finite range is refused before anything changes; tree_cost equals a long double evaluation of the header's formula."""
    r = subprocess.run([_native(tag, flags), "300", "11"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _emissive(hk):
    return hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(3.0)))


def _scene(hk, sphere, emissive_sphere):
    from hikari_jl_amd import geometry as G
    s = hk.Scene()
    s.push(G.rect3f((-1, 0, -1), (2, 0.01, 2)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7)))
    a = s.push_instance(sphere, hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))
    b = s.push_instance(emissive_sphere, _emissive(hk))
    s.push(hk.PointLight((0, 1.5, 0), hk.RGBSpectrum(2.0)))
    return s, a, b


def _arrays(d):
    T = d.n_triangles
    out = [np.ctypeslib.as_array(d.positions, (T, 3, 3)).copy(), np.ctypeslib.as_array(d.normals, (T, 3, 3)).copy(), np.ctypeslib.as_array(d.uvs, (T, 3, 2)).copy()]
    return out + [b"".join(bytes(d.lights[i]) for i in range(d.n_lights))]


def _meshes(with_uvs=True):
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.geometry import Mesh
    a, b = G.sphere((-0.4, 0.4, 0.0), 0.35, 8), G.sphere((0.4, 0.5, 0.1), 0.2, 6)
    rng = np.random.default_rng(2)
    return Mesh(a.positions, a.normals, rng.random((a.n_faces, 3, 2)).astype(f32) if with_uvs else None), b


def test_set_vertices_rewrites_the_kept_description(hk):
    from hikari_jl_amd.geometry import Mesh
    a, b = _meshes()
    s, ia, ib = _scene(hk, a, b)
    d = s.desc
    Pa, Na = V.ripple(a.positions, a.normals, 0.1)
    Ua = V.swirl_uvs(a.uvs)
    Pb, Nb = V.ripple(b.positions, b.normals, 0.05)
    before = _arrays(d)
    s.set_vertices(ia, Pa, normals=Na, uvs=Ua)
    s.set_vertices(ib, Pb, normals=Nb, move_lights=True)
    assert s.desc is d                                        # rewritten in place, not flattened again
    fresh, _, _ = _scene(hk, Mesh(Pa, Na, Ua), Mesh(Pb, Nb, b.uvs))
    got, want = _arrays(d), _arrays(fresh.desc)
    assert not np.array_equal(got[0], before[0]) and got[3] != before[3]
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w, equal_nan=True)
    assert got[3] == want[3] and d.n_lights == fresh.desc.n_lights > 1
    assert all(np.array_equal(x, y) for x, y in zip(s.bounds[:3], fresh.bounds[:3]))
    # a later flatten of the edited Scene gives the same arrays: the kept mesh was replaced
    s.sync()
    again = _arrays(s.desc)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(again[:3], want[:3])) and again[3] == want[3]


def test_set_vertices_defaults_keep_normals_uvs_and_lights(hk):
    from hikari_jl_amd.geometry import Mesh
    a, b = _meshes()
    s, ia, ib = _scene(hk, a, b)
    d = s.desc
    before = _arrays(d)
    Pa, _ = V.ripple(a.positions, a.normals, 0.1)
    Pb, _ = V.ripple(b.positions, b.normals, 0.05)
    s.set_vertices(ia, Pa)
    s.set_vertices(ib, Pb)                                     # move_lights=False: the lights stay where the mesh was pushed
    got = _arrays(d)
    fresh, _, _ = _scene(hk, Mesh(Pa, a.normals, a.uvs), Mesh(Pb, b.normals, b.uvs))
    want = _arrays(fresh.desc)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], before[1], equal_nan=True) and np.array_equal(got[2], before[2])
    assert got[3] == before[3] and got[3] != want[3]
    # before the first flatten there is no description: the edit replaces the kept mesh only
    s2, ia2, _ = _scene(hk, a, b)
    s2.set_vertices(ia2, Pa)
    assert s2._desc is None
    assert np.array_equal(_arrays(s2.desc)[0][ia2.first_tri:ia2.first_tri + ia2.n_tris], Pa)


def test_set_vertices_value_errors(hk):
    a, b = _meshes(with_uvs=False)
    s, ia, ib = _scene(hk, a, b)
    d = s.desc
    before = _arrays(d)[0]
    P, N = V.ripple(a.positions, a.normals, 0.1)
    bad = P.copy()
    bad[3, 1, 2] = np.nan
    inf = P.astype(np.float64)
    inf[0, 0, 0] = 1e300                                       # overflows binary32
    from hikari_jl_amd import geometry as G
    flat = s.push_instance(G.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.5)))   # no normals
    cases = [dict(positions=P[:-1]), dict(positions=P.reshape(-1, 9)), dict(positions=bad), dict(positions=inf), dict(positions=P, normals=N[:5]),
             dict(positions=P, uvs=np.zeros((a.n_faces, 3, 2), f32)),                       # the mesh was pushed without uvs
             dict(positions=P, uvs=np.zeros((a.n_faces, 2, 3), f32))]
    for kw in cases:
        with pytest.raises(ValueError):
            s.set_vertices(ia, **kw)
    with pytest.raises(ValueError):
        s.set_vertices(flat, np.zeros((2, 3, 3), f32), normals=np.zeros((2, 3, 3), f32))    # normals for a mesh pushed without normals
    with pytest.raises(ValueError):
        s.set_vertices(hk.scene.SceneInstance(ia.mi_idx, ia.first_tri + 1, ia.n_tris), P)   # not a mesh of this scene
    with pytest.raises(TypeError):
        s.set_vertices(0, P)
    assert np.array_equal(np.ctypeslib.as_array(d.positions, (d.n_triangles, 3, 3)), before)


CTYPES_OF = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32),
             "double*": C.POINTER(C.c_double)}


def test_abi_declares_the_three_entry_points_as_the_header_does(hk):
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    A = hk._abi
    for name, n_args in (("hk_scene_set_vertices", 7), ("hk_scene_bvh_cost", 3), ("hk_scene_bvh_copy", 4)):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]            # the parameter names dropped
        argtypes, restype = A.PROTOTYPES[name]
        assert len(args) == n_args and restype is C.c_int32 and list(argtypes) == [CTYPES_OF[a] for a in args], (name, args)
        assert name in A.EXPORTED_SYMBOLS
        fn = getattr(hk._lib.lib(), name)                                                  # the built library exports it, the loader installed the prototype
        assert list(fn.argtypes) == list(argtypes) and fn.restype is C.c_int32
    src = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()
    for needle in ("function set_vertices!(", "function bvh_cost(", "ccall((:hk_scene_set_vertices, LIB)", "ccall((:hk_scene_bvh_cost, LIB)"):
        assert needle in src, needle
