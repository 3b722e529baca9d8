"""Host side of hk_scene_update_medium_dense: the two entry points and the field record in the header, the ctypes mirror and the Julia
shim; what NanoVDBMedium.update(build="device") refuses; and the host tree it does not build until something asks for it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = ((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0))
HDR = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
JL = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()


def _prototype(name):
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, HDR, re.S)
    assert m, name
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]     # the parameter names dropped


def test_entry_points_in_header_stubs_and_julia_shim(hk):
    A = hk._abi
    ctypes_of = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "uint8_t*": C.POINTER(C.c_uint8),
                 "uint32_t*": C.POINTER(C.c_uint32), "const hk_medium*": C.POINTER(A.hk_medium), "hk_medium*": C.POINTER(A.hk_medium),
                 "const hk_dense_field*": C.POINTER(A.hk_dense_field)}
    assert _prototype("hk_scene_update_medium_dense") == ["hk_scene*", "int32_t", "const hk_medium*", "const hk_dense_field*"]
    assert _prototype("hk_scene_medium_tree_copy") == ["hk_scene*", "int32_t", "hk_medium*", "int64_t*", "uint8_t*", "int32_t*", "int32_t*", "uint32_t*"]
    L = hk._lib.lib()
    for name in ("hk_scene_update_medium_dense", "hk_scene_medium_tree_copy"):
        fn = getattr(L, name)                                 # the built library exports it
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [ctypes_of[a] for a in _prototype(name)], name
        assert name in A.EXPORTED_SYMBOLS
        call = re.search(r"ccall\(\(:%s, LIB\), Int32, \(([^)]*)\)" % name, JL)
        assert call and len(call.group(1).split(",")) == len(_prototype(name)), name
    contract = HDR[HDR.index("ORDERING CONTRACT"):HDR.index("int32_t hk_render(")]
    assert "hk_scene_update_medium_dense" in contract         # it renders the noted calls first, like the other edits
    assert "function update_medium_dense!(" in JL and "HK_DENSE_X_FASTEST" in JL[JL.index("function update_medium_dense!("):]


def test_the_field_record_has_the_header_layout(hk):
    A = hk._abi
    body = HDR[HDR.index("typedef struct hk_dense_field {"):HDR.index("} hk_dense_field;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s+(const float\*|int32_t)\s+(\w+)(\[3\])?;", body, re.M)
    assert [f[1] for f in fields] == [n for n, _ in A.hk_dense_field._fields_] == ["data", "res", "layout", "on_device"]
    assert C.sizeof(A.hk_dense_field) == 32 and A.hk_dense_field.res.offset == 8 and A.hk_dense_field.layout.offset == 20 and A.hk_dense_field.on_device.offset == 24
    for name, value in re.findall(r"\b(HK_DENSE_\w+)\s*=\s*(\d+)", HDR):
        assert getattr(A, name) == int(value)
        assert re.search(r"const HK_DENSE_X_FASTEST, HK_DENSE_Z_FASTEST = Int32\(0\), Int32\(1\)", JL)
    # the Julia mirror: same fields, same order, same C layout (a pointer, three Int32, two Int32)
    m = re.search(r"^struct DenseFieldRecord\n(.*?)^end", JL, re.S | re.M)
    assert [l.strip() for l in m.group(1).splitlines()] == ["data::Ptr{Float32}", "res::NTuple{3,Int32}", "layout::Int32", "on_device::Int32"]


def _fields():
    rng = np.random.default_rng(11)
    a = np.zeros((20, 17, 9), f32)
    a[:8] = rng.uniform(0.2, 3.0, (8, 17, 9))
    b = np.zeros((20, 17, 9), f32)
    b[8:] = rng.uniform(0.2, 3.0, (12, 17, 9))
    return a, b


def _medium(hk, data):
    return hk.NanoVDBMedium(data, bounds=BOUNDS, sigma_s=hk.RGBSpectrum(0.5), majorant_res=(5, 4, 3))


def test_the_device_build_argument_is_checked(hk):
    a, b = _fields()
    med = _medium(hk, a)
    before = med.buffer.copy()
    with pytest.raises(ValueError):
        med.update(data=np.ones((4, 4), f32), build="device")                 # ndim
    with pytest.raises(ValueError):
        med.update(data=np.ones((4, 4, 4, 1), f32), build="device")
    for bad in (np.nan, np.inf):
        poisoned = b.copy()
        poisoned[3, 2, 1] = bad
        with pytest.raises(ValueError):
            med.update(data=poisoned, build="device")
    with pytest.raises(ValueError):
        med.update(filepath="x.nvdb", build="device")
    with pytest.raises(ValueError):
        med.update(sigma_s=hk.RGBSpectrum(0.4), build="device")               # nothing to build
    with pytest.raises(ValueError):
        med.update(data=b, build="gpu")
    with pytest.raises(ValueError):
        med.update(data=b, build="device", majorant_res=(5, 4, 4))
    assert med._field is None and np.array_equal(med.buffer, before)          # a refused update changes nothing
    med.update(data=b)                                                        # the default stays the host build, at once
    assert med._field is None and np.array_equal(med._buffer, _medium(hk, b).buffer)


def test_the_host_tree_is_built_when_it_is_asked_for(hk):
    from hikari_jl_amd import media, scenes
    a, b = _fields()
    wide = ((-2.75, -2.5, 0.75), (2.5, 2.75, 2.25))
    med = _medium(hk, a)
    s = scenes.slab_scene(16, 16, medium=med)[0]
    s.update_medium(med, data=b, bounds=wide, build="device")
    assert not s._device                                                      # no device scene: only the description is marked stale
    assert med._field is not None and med._buffer is None and med._meta is None and med._majorant is None
    bb = tuple(tuple(float(f32(v)) for v in p) for p in wide)
    extent = tuple(float(f32(bb[1][k]) - f32(bb[0][k])) for k in range(3))
    want_buf, want_meta = media.build_nanovdb_from_dense(b, bb[0], extent)
    assert np.array_equal(med.buffer, want_buf) and med._field is None
    assert med.meta.keys() == want_meta.keys()
    for k, v in want_meta.items():
        assert np.array_equal(med.meta[k], v) if isinstance(v, np.ndarray) else med.meta[k] == v, k
    fresh = hk.NanoVDBMedium(b, bounds=wide, sigma_s=hk.RGBSpectrum(0.5), majorant_res=(5, 4, 3))
    assert med.max_density == fresh.max_density
    # the kept description of the scene is that of a scene built from the edited medium
    rec, want = s.desc.media[0], scenes.slab_scene(16, 16, medium=fresh)[0].desc.media[0]
    assert rec.nvdb_size == want.nvdb_size and rec.leaf_count == want.leaf_count and tuple(rec.vec) == tuple(want.vec) and tuple(rec.inv_mat) == tuple(want.inv_mat)
    assert np.array_equal(np.ctypeslib.as_array(rec.nvdb_bytes, (rec.nvdb_size,)), np.ctypeslib.as_array(want.nvdb_bytes, (want.nvdb_size,)))
    ncell = 5 * 4 * 3
    assert np.array_equal(np.ctypeslib.as_array(rec.majorant, (ncell,)), np.ctypeslib.as_array(want.majorant, (ncell,)))


def test_the_gpu_tests_fields_have_the_features_they_were_built_for(hk):
    """a check of the fixtures of test_medium_dense_build.py (no device code runs here)"""
    from test_medium_dense_build import _field
    assert _field("4104x8x8")[2]["upper_count"] == 2 and _field("8x8x4104")[2]["upper_count"] == 2 and _field("4104x8x8")[2]["leaf_count"] == 513
    for name in ("136x8x8", "8x136x9", "8x8x136"):
        assert _field(name)[2]["lower_count"] == 2
    assert _field("lone-voxel")[2]["index_min"] == (8, 8, 8)
    assert _field("minus-zero")[1].size == _field("all-zero")[1].size == 64
    assert 0 < _field("holes-b")[2]["leaf_count"] < 3 * 3 * 2
    for name in ("minus-zero-is-the-min", "plus-zero-is-the-max"):
        assert _field(name)[2]["leaf_count"] == 1


def test_leaf_min_and_max_order_minus_zero_below_plus_zero(hk):
    """Julia's min / max (nanovdb.jl:714-722): -0.0 < +0.0, wherever the zeros stand in the leaf.  The words are compared as bits."""
    from hikari_jl_amd import media
    u32 = lambda v: int(np.array([v], f32).view(np.uint32)[0])

    def bounds(vals):
        buf, meta = media.build_nanovdb_from_dense(vals.reshape(8, 8, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        leaf = meta["leaf_offset"] - 1
        w = buf[leaf + media.LEAF_MIN_OFF:leaf + media.LEAF_MIN_OFF + 8].view(np.uint32)
        return int(w[0]), int(w[1])

    for first, second in ((-0.0, 0.0), (0.0, -0.0)):          # either order of the two zeros
        v = np.zeros(512, f32)
        v[3], v[400], v[77] = first, second, 0.7
        assert bounds(v) == (u32(-0.0), u32(0.7))
        v = np.full(512, -0.5, f32)
        v[3], v[400] = first, second
        assert bounds(v) == (u32(-0.5), u32(0.0))
    v = np.random.default_rng(4).uniform(-2.0, 3.0, 512).astype(f32)
    assert bounds(v) == (u32(v.min()), u32(v.max()))             # without zeros: numpy's own


def test_a_later_host_update_drops_the_kept_field(hk):
    a, b = _fields()
    med = _medium(hk, a)
    med.update(data=b, build="device")
    med.update(data=a)                                                        # a host build after a device one: the kept field is gone
    assert med._field is None and np.array_equal(med.buffer, _medium(hk, a).buffer)
    med.update(data=b, build="device")
    med.save(os.devnull)                                                      # save asks for the tree
    assert med._field is None and np.array_equal(med._buffer, _medium(hk, b).buffer)
