"""Host side of the sky bake (hk_scene_update_envmap_sky), no GPU: hk_sky.h compiled alone with g++ against sunsky.sky_texels under the
metric of sky_cases.py; sunsky_to_envlight unchanged by its split into sky_params / sky_texels; Scene.update_sky on the kept description
(build="host" equals update_envmap; build="device" bakes on the host only when asked); what it refuses; the two entry points and the
record in the header, the ctypes mirror and the Julia shim; the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sky_cases as SC

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
JL = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()


# ---- hk_sky.h on the host ----------------------------------------------------------------------------------------------------
def _texel_check(tag, flags):
    exe = os.path.join(tempfile.gettempdir(), "hk_sky_texel_check_%s_%d" % (tag, os.getuid()))
    csrc = os.path.join(ROOT, "hikari.jl_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "sky_texel_check.cpp")]
    deps = src + [os.path.join(csrc, "hk_sky.h"), os.path.join(ROOT, "include", "hikari_mi355x.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", csrc, "-I", os.path.join(ROOT, "include")] + flags + src + ["-o", exe])
    return exe


def _run_texel_check(hk, exe, c, tmp):
    from hikari_jl_amd import sunsky
    params = sunsky.sky_params(**SC.sky_kwargs(hk, c))
    fin, fout = os.path.join(tmp, "params.bin"), os.path.join(tmp, "texels.bin")
    with open(fin, "wb") as f:
        f.write(np.array([c["res"], 0], np.int32).tobytes() + bytes(params))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("{"), (SC.case_id(c), r.stdout, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return SC.from_device_layout(np.fromfile(fout, f32), c["res"])


@pytest.mark.parametrize("tag,flags", [("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_shared_texel_function_agrees_with_the_numpy_bake(hk, tag, flags, tmp_path):
    """Every case of the parameter set; ground and alpha equal; the bounds of sky_cases.check."""
    exe = _texel_check(tag, flags)
    got = [(c, _run_texel_check(hk, exe, c, str(tmp_path))) for c in SC.CASES]
    SC.check([(c, SC.agreement(t, c)) for c, t in got], [(c, SC.agreement_with_host_build(t, c)) for c, t in got if SC.dark_family(c)], "host")


# ---- the split of sunsky_to_envlight ----------------------------------------------------------------------------------------
PARENT_CASES = {"r16": dict(direction=(0.3, 0.2, 0.8), resolution=16),
                "r32": dict(direction=(1.0, -2.0, 0.4), intensity=2.0, turbidity=3.3, ground_enabled=False, resolution=32)}


def test_sunsky_to_envlight_returns_what_it_returned_before_the_split(hk):
    """tests/golden/sunsky_to_envlight_parent.npz: texels, tables, light scale and sun record computed by the function before it was
    split into sky_params / sky_texels / sky_scale / sun_light."""
    from hikari_jl_amd import sunsky
    want = np.load(os.path.join(ROOT, "tests", "golden", "sunsky_to_envlight_parent.npz"))
    for key, kw in PARENT_CASES.items():
        kw = dict(kw)
        if key == "r32":
            kw["ground_albedo"] = hk.RGBSpectrum(0.2, 0.4, 0.1)
        env, sun = sunsky.sunsky_to_envlight(**kw)
        m = env.env_map
        assert m.data.dtype == f32 and np.array_equal(m.data, want[key + "_data"])
        for t in m._TABLES:
            assert np.array_equal(getattr(m.distribution, t), want[key + "_" + t]), (key, t)
        assert f32(m.distribution.marginal_func_int) == want[key + "_marginal_func_int"]
        assert np.array_equal(np.asarray(env.scale_rgb.c, np.float64), want[key + "_env_scale"])
        assert np.array_equal(np.asarray(list(sun.i.poly) + [sun.i.scale, sun.scale] + list(sun.direction), np.float64), want[key + "_sun"])
        # and the parts are the whole
        sky = {k: v for k, v in kw.items() if k not in ("intensity", "resolution")}
        assert np.array_equal(sunsky.sky_texels(resolution=kw["resolution"], **sky), want[key + "_data"][..., :3])


def test_sky_params_fills_the_record_from_the_hosek_state(hk):
    from hikari_jl_amd import sunsky
    A = hk._abi
    direction, turbidity = (1.0, -2.0, 0.4), 3.3
    p = sunsky.sky_params(direction, turbidity, hk.RGBSpectrum(0.2, 0.4, 0.1), False)
    assert isinstance(p, A.hk_sky_params) and p.reserved == 0 and p.ground_enabled == 0
    d = np.asarray(direction, f32)
    d = (f32(1) / np.sqrt((d * d).sum(dtype=f32))) * d
    assert np.array_equal(np.asarray(p.sun_dir[:], f32), d)
    assert np.array_equal(np.asarray(p.ground_rgb[:], f32), np.asarray([0.2, 0.4, 0.1], f32) * f32(0.3))
    state = sunsky.HosekState(float(f32(turbidity)), 0.5, float(np.arcsin(np.clip(d[2], f32(0), f32(1)))))
    assert np.array_equal(np.ctypeslib.as_array(p.config), np.stack(state.configs))
    assert np.array_equal(np.ctypeslib.as_array(p.radiance), np.asarray(state.radiances))
    W = np.ctypeslib.as_array(p.xyz_weight)
    assert W.shape == (3, 13) and np.isfinite(W).all() and abs(W[1].sum() - 1.0) < 1e-3     # Y of the flat spectrum 1 is 1 (the weights are / CIE_Y_INTEGRAL)
    assert sunsky.sky_params(direction, ground_enabled=True).ground_enabled == 1
    assert np.array_equal(np.asarray(sunsky.sky_params(direction).ground_rgb[:], f32), np.full(3, f32(0.3) * f32(0.3)))


# ---- Scene.update_sky on the kept description ---------------------------------------------------------------------------------
def _scene(hk, res=16, **kw):
    from hikari_jl_amd import scenes
    return scenes.sky_scene(48, 32, env_res=res, tess=4, **kw)[0]


NEW = dict(direction=(-0.5, 0.3, 0.6), turbidity=4.2, ground_enabled=True)


def _map_state(m):
    D = m.distribution
    return [m.data.copy(), m._jl.copy()] + [getattr(D, t).copy() for t in m._TABLES] + [np.float32(D.marginal_func_int), m.rotation.copy()]


def _desc_state(s):
    d, out = s.desc, []
    for i in range(d.n_lights):
        out.append(bytes(d.lights[i]))
    e = d.envmaps[0]
    out.append(np.ctypeslib.as_array(e.data, (e.width * e.height * 4,)).tobytes())
    out.append(np.ctypeslib.as_array(e.conditional_cdf, ((e.nu + 1) * e.nv,)).tobytes())
    out.append(np.ctypeslib.as_array(e.marginal_cdf, (e.nv + 1,)).tobytes())
    out.append((e.marginal_func_int, list(e.rotation)))
    return out


def test_update_sky_host_build_equals_update_envmap_of_the_host_bake(hk):
    from hikari_jl_amd import sunsky
    a, b = _scene(hk), _scene(hk)
    a.update_sky(a.lights[0], build="host", **NEW)
    b.update_envmap(b.lights[0].env_map, data=sunsky.sky_texels(resolution=16, **NEW))
    for x, y in zip(_map_state(a.lights[0].env_map), _map_state(b.lights[0].env_map)):
        assert np.array_equal(x, y)
    assert _desc_state(a) == _desc_state(b)
    # intensity and sun: the lights sunsky_to_envlight gives
    a.update_sky(a.lights[0], build="host", intensity=2.5, sun=a.lights[1], **NEW)
    env, sun = sunsky.sunsky_to_envlight(intensity=2.5, resolution=16, **NEW)
    f = hk.Scene()
    f.push_light(env), f.push_light(sun)
    f.sync()
    da, df = a.desc, f.desc
    assert [bytes(da.lights[i]) for i in range(2)] == [bytes(df.lights[i]) for i in range(2)]
    assert a.lights[1].direction == sun.direction and a.lights[0].scale_rgb.c == env.scale_rgb.c
    # without an intensity the sun only turns
    before = (a.lights[1].i.poly, a.lights[1].i.scale, a.lights[1].scale)
    a.update_sky(a.lights[0], direction=(0.1, 0.1, 0.9), sun=a.lights[1], build="host")
    assert (a.lights[1].i.poly, a.lights[1].i.scale, a.lights[1].scale) == before
    assert a.lights[1].direction == sunsky.sun_light((0.1, 0.1, 0.9)).direction


def test_update_sky_device_build_bakes_on_the_host_only_when_asked(hk, monkeypatch):
    from hikari_jl_amd import sunsky
    calls = []
    real = sunsky.sky_texels
    monkeypatch.setattr(sunsky, "sky_texels", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    want = real(resolution=16, **NEW)
    for ask in ("data", "distribution", "record", "desc", "description_without_skies", "overwrite"):
        s = _scene(hk)
        m = s.lights[0].env_map
        old = m._data.copy()
        del calls[:]
        s.update_sky(s.lights[0], **NEW)                      # build="device": no device scene here, nothing to call
        s.update_sky(s.lights[0], **dict(NEW, turbidity=2.0))
        s.update_sky(s.lights[0], **NEW)
        s.update_envmap(m, rotation=np.eye(3, dtype=f32))     # a rotation asks for no texel
        assert calls == [] and np.array_equal(m._data, old), ask
        if ask == "data":
            got = m.data
        elif ask == "distribution":
            got = (m.distribution, m.data)[1]
        elif ask == "record":
            got = (m.record(), m.data)[1]
        elif ask == "desc":                                    # what hk_scene_create of a later scene reads
            e = s.desc.envmaps[0]
            got = SC.from_device_layout(np.ctypeslib.as_array(e.data, (16 * 16 * 4,)), 16)
            assert e.marginal_func_int == float(m.distribution.marginal_func_int)
        elif ask == "description_without_skies":               # what a scene that has its device scene reads: no bake
            s._description(bake_skies=False)
            assert calls == [] and np.array_equal(m._data, old)
            continue
        else:                                                  # new texels replace the pending sky: it is never baked
            s.update_envmap(m, data=np.full((16, 16, 3), 0.25, f32))
            assert calls == [] and np.array_equal(m.data[..., :3], np.full((16, 16, 3), 0.25, f32)) and calls == []
            continue
        assert calls == [1], ask                               # the last parameters, once
        assert np.array_equal(got[..., :3], want), ask
        fresh = hk.EnvironmentMap(want)
        for x, y in zip(_map_state(m), _map_state(fresh)):
            assert np.array_equal(x, y), ask
        assert calls == [1]


def test_update_sky_refuses_what_the_library_would(hk):
    from hikari_jl_amd.envmap import EnvironmentLight, EnvironmentMap
    s = _scene(hk)
    env, sun = s.lights[0], s.lights[1]
    before = (_map_state(env.env_map), _desc_state(s))
    bad = [dict(direction=(0, 0, 0)), dict(direction=(np.nan, 0, 1)), dict(direction=(np.inf, 0, 1)), dict(direction=(1, 0)),
           dict(direction=(0, 0, 1), turbidity=np.nan), dict(direction=(0, 0, 1), turbidity=np.inf), dict(direction=(0, 0, 1), intensity=np.nan),
           dict(direction=(0, 0, 1), ground_albedo=hk.RGBSpectrum(np.nan)), dict(direction=(0, 0, 1), build="gpu"),
           dict(direction=(0, 0, 1), sun=env)]
    for kw in bad:
        for build in ("device", "host"):
            with pytest.raises(ValueError):
                s.update_sky(env, **dict(dict(build=build), **kw))
    with pytest.raises(ValueError):
        s.update_sky(sun, (0, 0, 1))                                           # not an environment light
    with pytest.raises(ValueError):
        s.update_sky(EnvironmentLight(EnvironmentMap(np.ones((8, 8, 3), f32))), (0, 0, 1))     # of no light of this scene
    wide = hk.Scene()
    wide.push_light(EnvironmentLight(EnvironmentMap(np.ones((8, 16, 3), f32))))
    wide.sync()
    for build in ("device", "host"):
        with pytest.raises(ValueError):
            wide.update_sky(wide.lights[0], (0, 0, 1), build=build)            # not square
    after = (_map_state(env.env_map), _desc_state(s))
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    assert env.env_map._sky is None


# ---- header, stubs, Julia shim ------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, HDR, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in args.split(",")]     # the parameter names dropped


def test_entry_points_in_header_stubs_and_julia_shim(hk):
    A = hk._abi
    ctypes_of = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32), "float*": A.PF, "const hk_sky_params*": C.POINTER(A.hk_sky_params)}
    assert _prototype("hk_scene_update_envmap_sky") == ["hk_scene*", "int32_t", "const hk_sky_params*"]
    assert _prototype("hk_scene_envmap_copy") == ["hk_scene*", "int32_t", "int32_t*", "int32_t*"] + ["float*"] * 6
    L = hk._lib.lib()
    for name in ("hk_scene_update_envmap_sky", "hk_scene_envmap_copy"):
        fn = getattr(L, name)                                 # the built library exports it
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [ctypes_of[a] for a in _prototype(name)], name
        assert name in A.EXPORTED_SYMBOLS
        call = re.search(r"ccall\(\(:%s, LIB\), Int32, \(([^)]*)\)" % name, JL)
        assert call and len(call.group(1).split(",")) == len(_prototype(name)), name
    contract = HDR[HDR.index("ORDERING CONTRACT"):HDR.index("int32_t hk_render(")]
    assert "hk_scene_update_envmap_sky" in contract           # it renders the noted calls first, like the other edits
    for needle in ("function update_sky!(", "function envmap_copy(", "direction", "turbidity", "ground_albedo", "ground_enabled"):
        assert needle in JL[JL.index("struct SkyParamsRecord"):], needle


def test_the_sky_record_has_the_header_layout(hk, tmp_path):
    A = hk._abi
    body = HDR[HDR.index("typedef struct hk_sky_params {"):HDR.index("} hk_sky_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s+(float|int32_t|double)\s+(\w+)((?:\[\d+\])*);", body, re.M)
    names = ["sun_dir", "ground_enabled", "ground_rgb", "reserved", "config", "radiance", "xyz_weight"]
    assert [f[1] for f in fields] == [n for n, _ in A.hk_sky_params._fields_] == names
    dims = {f[1]: [int(x) for x in re.findall(r"\d+", f[2])] for f in fields}
    assert dims == {"sun_dir": [3], "ground_enabled": [], "ground_rgb": [3], "reserved": [], "config": [11, 9], "radiance": [11], "xyz_weight": [3, 13]}
    # gcc's layout of the header's record
    src = tmp_path / "sky.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hikari_mi355x.h"\nint main(){printf("%zu", sizeof(hk_sky_params));' +
                   "".join('printf(" %%zu", offsetof(hk_sky_params, %s));' % n for n in names) + "return 0;}")
    exe = tmp_path / "sky"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == C.sizeof(A.hk_sky_params) == 1224
    assert out[1:] == [getattr(A.hk_sky_params, n).offset for n in names] == [0, 12, 16, 28, 32, 824, 912]
    assert np.ctypeslib.as_array(A.hk_sky_params().config).shape == (11, 9) and np.ctypeslib.as_array(A.hk_sky_params().xyz_weight).shape == (3, 13)
    # the Julia mirror: same fields, same order, same C layout
    m = re.search(r"^struct SkyParamsRecord\n(.*?)^end", JL, re.S | re.M)
    assert [l.strip() for l in m.group(1).splitlines()] == ["sun_dir::NTuple{3,Float32}", "ground_enabled::Int32", "ground_rgb::NTuple{3,Float32}", "reserved::Int32",
                                                          "config::NTuple{99,Float64}", "radiance::NTuple{11,Float64}", "xyz_weight::NTuple{39,Float64}"]


def test_null_arguments_are_refused_without_a_device(hk):
    from hikari_jl_amd import sunsky
    A = hk._abi
    L = hk._lib.lib()
    p = sunsky.sky_params((0.0, 0.0, 1.0))
    assert L.hk_scene_update_envmap_sky(None, 0, C.byref(p)) == A.HK_ERR_INVALID
    assert b"hk_scene_update_envmap_sky: null scene" in L.hk_last_error()
    assert L.hk_scene_update_envmap_sky(None, 0, None) == A.HK_ERR_INVALID
    assert b"hk_scene_update_envmap_sky: null params" in L.hk_last_error()
    w, h = C.c_int32(-7), C.c_int32(-7)
    assert L.hk_scene_envmap_copy(None, 0, C.byref(w), C.byref(h), None, None, None, None, None, None) == A.HK_ERR_INVALID
    assert b"hk_scene_envmap_copy: null scene" in L.hk_last_error() and (w.value, h.value) == (-7, -7)
