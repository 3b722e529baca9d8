"""Host side of the in-place medium edits: the two entry points in the header, the ctypes stubs and the Julia shim against it, the
update() methods of the media mirror (what they change, what they refuse) and Scene.update_medium on a scene that has no device
scene yet — the kept description must then be the description of a scene built from the edited medium from scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = ((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0))
POINTERS = ("density", "sigma_a_grid", "sigma_s_grid", "Le_grid", "majorant", "nvdb_bytes")


def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\);" % name, hdr, re.S)
    assert m, name
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]     # the parameter names dropped


def test_entry_points_in_header_stubs_and_julia_shim(hk):
    A = hk._abi
    ctypes_of = {"hk_scene*": C.c_void_p, "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32), "float*": C.POINTER(C.c_float),
                 "uint32_t*": C.POINTER(C.c_uint32), "const hk_medium*": C.POINTER(A.hk_medium)}
    assert _prototype("hk_scene_update_medium") == ["hk_scene*", "int32_t", "const hk_medium*"]
    assert _prototype("hk_scene_medium_copy") == ["hk_scene*", "int32_t", "int32_t*", "float*", "uint32_t*"]
    L = hk._lib.lib()
    for name in ("hk_scene_update_medium", "hk_scene_medium_copy", "hk_test_medium_bricks"):
        fn = getattr(L, name)                                 # the built library exports it
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [ctypes_of[a] for a in _prototype(name)], name
        assert name in A.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    contract = hdr[hdr.index("ORDERING CONTRACT"):hdr.index("int32_t hk_render(")]
    assert "hk_scene_update_medium" in contract               # it renders the noted calls first, like the other edits
    src = open(os.path.join(ROOT, "julia", "HikariMI355X.jl")).read()
    assert "function update_medium!(" in src
    call = re.search(r"ccall\(\(:hk_scene_update_medium, LIB\), Int32, \(([^)]*)\)", src)
    assert call and len(call.group(1).split(",")) == len(_prototype("hk_scene_update_medium"))


def _scene(hk, medium):
    from hikari_jl_amd import scenes
    return scenes.slab_scene(16, 16, medium=medium)[0]


def _record_state(rec, medium):
    """every field of the record that is no pointer, and what the pointers point to"""
    A = type(rec)
    plain = {}
    for name, ctype in A._fields_:
        if name in POINTERS:
            continue
        v = getattr(rec, name)
        plain[name] = tuple(v) if hasattr(v, "__len__") else v
    ncell = int(np.prod(medium.majorant_res)) if hasattr(medium, "majorant_res") else 0
    nvox = int(np.prod(tuple(rec.res)))
    arrays = {"majorant": np.ctypeslib.as_array(rec.majorant, (ncell,)).copy() if ncell else None}
    if rec.density:
        arrays["density"] = np.ctypeslib.as_array(rec.density, (nvox,)).copy()
    for g in ("sigma_a_grid", "sigma_s_grid", "Le_grid"):
        p = getattr(rec, g)
        arrays[g] = np.ctypeslib.as_array(p, (nvox * 4,)).copy() if p else None
    if rec.nvdb_bytes:
        arrays["nvdb"] = np.ctypeslib.as_array(rec.nvdb_bytes, (rec.nvdb_size,)).copy()
    return plain, arrays


def _same_records(a, b):
    assert a[0] == b[0]
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert (a[1][k] is None) == (b[1][k] is None), k
        assert a[1][k] is None or np.array_equal(a[1][k], b[1][k]), k


def _cases(hk):
    rng = np.random.default_rng(11)
    da, db = (rng.uniform(0.0, 2.0, (13, 10, 7)).astype(f32) for _ in range(2))
    ra, rb = (rng.uniform(0.0, 1.0, (6, 5, 4, 3)).astype(f32) for _ in range(2))
    na = np.zeros((20, 17, 9), f32)
    na[:8] = rng.uniform(0.2, 3.0, (8, 17, 9))
    nb = np.zeros((20, 17, 9), f32)
    nb[8:] = rng.uniform(0.2, 3.0, (12, 17, 9))
    T = np.eye(4, dtype=f32)
    T[:3, 3] = (0.1, -0.2, 0.05)
    grid = dict(sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(4, 3, 9))
    nv = dict(bounds=BOUNDS, sigma_s=hk.RGBSpectrum(0.5), majorant_res=(5, 4, 3))
    return {
        "grid": (lambda: hk.GridMedium(da, **grid), dict(density=db, g=0.3, transform=T), lambda: hk.GridMedium(db, g=0.3, transform=T, **grid)),
        "rgb": (lambda: hk.RGBGridMedium(sigma_s_grid=ra, sigma_scale=1.5, bounds=BOUNDS, majorant_res=(3, 2, 5)), dict(sigma_s_grid=rb, sigma_scale=0.75),
                lambda: hk.RGBGridMedium(sigma_s_grid=rb, sigma_scale=0.75, bounds=BOUNDS, majorant_res=(3, 2, 5))),
        "nanovdb": (lambda: hk.NanoVDBMedium(na, **nv), dict(data=nb, sigma_s=hk.RGBSpectrum(0.25)), lambda: hk.NanoVDBMedium(nb, **dict(nv, sigma_s=hk.RGBSpectrum(0.25)))),
        "homogeneous": (lambda: hk.HomogeneousMedium(sigma_s=hk.RGBSpectrum(0.4)), dict(sigma_a=hk.RGBSpectrum(0.1, 0.2, 0.3), g=0.5),
                        lambda: hk.HomogeneousMedium(sigma_a=hk.RGBSpectrum(0.1, 0.2, 0.3), sigma_s=hk.RGBSpectrum(0.4), g=0.5)),
    }


@pytest.mark.parametrize("kind", ["grid", "rgb", "nanovdb", "homogeneous"])
@pytest.mark.parametrize("synced", [False, True], ids=["before-sync", "after-sync"])
def test_update_medium_without_a_device_scene_updates_the_kept_description(hk, kind, synced):
    make_a, change, make_b = _cases(hk)[kind]
    med = make_a()
    s = _scene(hk, med)                                       # (slab_scene syncs)
    if not synced:
        s._desc = None                                        # as before the first sync(): there is no description to patch
    s.update_medium(med, **change)
    assert not s._device                                      # nothing was created on a device
    fresh_med = make_b()
    fresh = _scene(hk, fresh_med)
    assert s.desc.n_media == fresh.desc.n_media == 1
    _same_records(_record_state(s.desc.media[0], med), _record_state(fresh.desc.media[0], fresh_med))


def test_update_methods_refuse_what_the_library_refuses(hk):
    c = _cases(hk)
    grid, rgb, nano, homog = (c[k][0]() for k in ("grid", "rgb", "nanovdb", "homogeneous"))
    before = grid.density.copy(), grid.bounds, grid.majorant.copy()
    with pytest.raises(ValueError):
        grid.update(density=np.zeros((12, 10, 7), f32))       # res
    with pytest.raises(ValueError):
        grid.update(majorant_res=(4, 3, 8))
    with pytest.raises(ValueError):
        grid.update(density=np.ones((13, 10, 7), f32), bounds=((0, 0, 0), (1, np.inf, 1)))   # a bad bound changes nothing, not even the density
    with pytest.raises(ValueError):
        grid.update(transform=np.full((4, 4), np.nan, f32))
    with pytest.raises(ValueError):
        grid.update(g=float("nan"))
    assert np.array_equal(grid.density, before[0]) and grid.bounds == before[1] and np.array_equal(grid.majorant, before[2])
    with pytest.raises(ValueError):
        rgb.update(sigma_a_grid=np.ones((6, 5, 4, 3), f32))   # a grid that appears
    with pytest.raises(ValueError):
        rgb.update(sigma_s_grid=np.ones((6, 5, 5, 3), f32))   # res
    with pytest.raises(ValueError):
        rgb.update(majorant_res=(3, 2, 4))
    with pytest.raises(ValueError):
        rgb.update(sigma_scale=float("inf"))
    with pytest.raises(ValueError):
        nano.update(majorant_res=(5, 4, 4))
    with pytest.raises(ValueError):
        nano.update(data=np.ones((4, 4, 4), f32), filepath="x.nvdb")
    with pytest.raises(ValueError):
        nano.update(bounds=((0, 0, 0), (1, 1, np.nan)))
    with pytest.raises(ValueError):
        homog.update(g=float("inf"))
    # through the scene: a medium of another scene (no index), a change the kind does not have (a kind change), the class of a grey medium
    s = _scene(hk, grid)
    with pytest.raises(ValueError):
        s.update_medium(c["grid"][0](), density=np.ones((13, 10, 7), f32))
    with pytest.raises(ValueError):
        s.update_medium(grid, data=np.ones((13, 10, 7), f32))
    with pytest.raises(ValueError):
        _scene(hk, homog).update_medium(homog, density=np.ones((2, 2, 2), f32))
    with pytest.raises(ValueError):
        s.update_medium(grid, sigma_s=hk.RGBSpectrum(0.9, 0.5, 0.2))
    assert grid.sigma_s.c[:3] == (float(f32(0.6)),) * 3
    s.update_medium(grid, sigma_s=hk.RGBSpectrum(0.8))        # grey stays grey


def test_an_update_marks_the_host_majorant_stale_and_rebuilds_it_on_demand(hk):
    from hikari_jl_amd import media
    make_a, change, make_b = _cases(hk)["grid"]
    med = make_a()
    med.update(**change)
    assert med._majorant is None                              # hk_scene_update_medium does not read it: nothing was built
    assert np.array_equal(med.majorant, media.build_majorant_grid(med.density, med.majorant_res))
    assert np.array_equal(med.majorant, make_b().majorant)
