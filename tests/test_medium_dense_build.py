"""A NanoVDB medium updated from a dense field, the tree built on the device (hk_scene_update_medium_dense).  The contract: the scene
holds, bit for bit, what hk_scene_update_medium leaves for the host-built tree (media.build_nanovdb_from_dense) of the same field.
Every test drives two scenes, one through each call, and compares them with np.array_equal: the tree bytes, the record and the block
table (hk_scene_medium_tree_copy), majorant grid and zero mask (hk_scene_medium_copy), halo bricks (hk_test_medium_bricks), films.
There are no tolerances.

Shapes are the smallest at which each mechanism can go wrong: one padded block ((8,8,8), (1,1,1)); the ragged fields with holes and
absent blocks of test_media_edits.py ((20,17,9)); two lower nodes along each axis (136 = 17 blocks); two upper nodes, two root tiles and
513 leaves (4104 = 513 blocks, along x — the slowest axis of the numbering — and along z, the fastest); an index box that does not
start at 0; and fields without a leaf (all zeros, a lone -0.0).  Each runs in both layouts, from host memory and from a device tensor."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 40, 32
KW = dict(max_depth=5, samples=4)
BOUNDS = ((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0))          # the slab of scenes.slab_scene
MRES = (5, 4, 3)
POINTERS = ("density", "sigma_a_grid", "sigma_s_grid", "Le_grid", "majorant", "nvdb_bytes")


# ---- fields ---------------------------------------------------------------------------------------------------------------------
def _nvdb_volumes():
    """the two 20x17x9 fields of test_media_edits.py: holes inside a leaf, absent blocks, a ragged shape"""
    rng = np.random.default_rng(21)
    a = np.zeros((20, 17, 9), f32)
    a[:8] = rng.uniform(0.2, 3.0, (8, 17, 9)).astype(f32)
    a[2:5, 3:9, 1:4] = 0.0
    a[:8, 8:16, :8] = 0.0
    b = np.zeros((20, 17, 9), f32)
    b[8:] = rng.uniform(0.2, 3.0, (12, 17, 9)).astype(f32)
    b[10:13, 0:5, 2:8] = 0.0
    b[16:20, 0:8, 0:8] = 0.0
    return a, b


def _random(shape, seed):
    return np.random.default_rng(seed).uniform(0.1, 1.0, shape).astype(f32)


def _lone(value):
    d = np.zeros((9, 9, 9), f32)
    d[8, 8, 8] = value
    return d


def _zeros_in_a_leaf(fill, extra):
    """a populated leaf in which the sign of a zero decides a bound: -0.0 < +0.0 (Julia's min / max, nanovdb.jl:714-722)"""
    d = np.full((8, 8, 8), fill, f32)
    d[1, 2, 3], d[5, 0, 7] = -0.0, 0.0
    if extra is not None:
        d[7, 7, 0] = extra
    return d


FIELDS = {
    "minus-zero-is-the-min": lambda: _zeros_in_a_leaf(0.0, 0.7),       # zeros of both signs and one 0.7: min = -0.0
    "plus-zero-is-the-max": lambda: _zeros_in_a_leaf(-0.5, None),      # -0.5 with one -0.0 and one +0.0: max = +0.0
    "8x8x8": lambda: _random((8, 8, 8), 1),
    "1x1x1": lambda: _random((1, 1, 1), 2),
    "holes-a": lambda: _nvdb_volumes()[0],
    "holes-b": lambda: _nvdb_volumes()[1],
    "136x8x8": lambda: _random((136, 8, 8), 3),
    "8x136x9": lambda: _random((8, 136, 9), 4),
    "8x8x136": lambda: _random((8, 8, 136), 5),
    "4104x8x8": lambda: _random((4104, 8, 8), 6),
    "8x8x4104": lambda: _random((8, 8, 4104), 7),
    "lone-voxel": lambda: _lone(0.75),
    "minus-zero": lambda: _lone(-0.0),
    "all-zero": lambda: np.zeros((9, 9, 9), f32),
}
_host_trees = {}


def _field(name):
    """the field and its host tree, built once and left unchanged"""
    if name not in _host_trees:
        from hikari_jl_amd import media
        data = FIELDS[name]()
        extent = tuple(float(f32(BOUNDS[1][k]) - f32(BOUNDS[0][k])) for k in range(3))
        buf, meta = media.build_nanovdb_from_dense(data, tuple(float(f32(v)) for v in BOUNDS[0]), extent)
        data.setflags(write=False)
        buf.setflags(write=False)
        _host_trees[name] = (data, buf, meta)
    return _host_trees[name]


# ---- scenes, the two calls, read-backs ------------------------------------------------------------------------------------------
def _medium(hk, data):
    return hk.NanoVDBMedium(data, bounds=BOUNDS, sigma_a=hk.RGBSpectrum(0.02), sigma_s=hk.RGBSpectrum(0.5), g=0.3, majorant_res=MRES)


def _scene(hk, ctx, data):
    from hikari_jl_amd import scenes
    med = _medium(hk, data)
    s = scenes.slab_scene(W, H, medium=med)[0]
    return s, med, hk.scene_handle(ctx, s)


def _host_update(hk, sh, med, data):
    """hk_scene_update_medium with the host-built tree of `data` -> status"""
    med.update(data=data)
    keep, rec = [], hk._abi.hk_medium()
    med.fill_record(rec, keep, majorant=False)
    return hk._lib.lib().hk_scene_update_medium(sh, 0, C.byref(rec))


def _dense_args(hk, med, data, layout, source, keep):
    A = hk._abi
    rec = A.hk_medium()
    med.fill_record(rec, keep, majorant=False, tree=False)
    arr = np.ascontiguousarray(data if layout == A.HK_DENSE_Z_FASTEST else data.transpose(2, 1, 0))   # C [z][y][x] == Julia [nx,ny,nz]
    field = A.hk_dense_field()
    field.res[:] = data.shape
    field.layout = layout
    if source == "device":
        import torch
        t = torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()
        keep.append(t)
        field.data, field.on_device = C.cast(C.c_void_p(t.data_ptr()), A.PF), 1
    else:
        keep.append(arr)
        field.data, field.on_device = arr.ctypes.data_as(A.PF), 0
    return rec, field


def _dense_update(hk, sh, med, data, layout, source):
    keep = []
    rec, field = _dense_args(hk, med, data, layout, source, keep)
    status = hk._lib.lib().hk_scene_update_medium_dense(sh, 0, C.byref(rec), C.byref(field))
    hk._lib.check(hk._lib.lib().hk_sync(hk.Context.get(0).h), "hk_sync")          # (the field is borrowed until the build has run)
    return status


def _tree(hk, sh):
    """record (plain fields), bytes, table extent, origin and entries of medium 0"""
    A, L = hk._abi, hk._lib.lib()
    rec, n = A.hk_medium(), C.c_int64()
    dims, tmin = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    hk._lib.check(L.hk_scene_medium_tree_copy(sh, 0, C.byref(rec), C.byref(n), None, dims, tmin, None), "hk_scene_medium_tree_copy")
    bytes_ = np.full(n.value, 0xA5, np.uint8)
    table = np.full((dims[0], dims[1], dims[2], 2), 0xdeadbeef, np.uint32)
    hk._lib.check(L.hk_scene_medium_tree_copy(sh, 0, None, C.byref(n), bytes_.ctypes.data_as(C.POINTER(C.c_uint8)), dims, tmin, table.ctypes.data_as(C.POINTER(C.c_uint32))),
                  "hk_scene_medium_tree_copy")
    plain = {}
    for name, _ in A.hk_medium._fields_:
        v = getattr(rec, name)
        if name in POINTERS:
            assert not v, name                               # pointers NULL
        else:
            plain[name] = tuple(v) if hasattr(v, "__len__") else v
    return dict(record=plain, bytes=bytes_, dims=tuple(dims), min=tuple(tmin), table=table)


def _same_tree(a, b):
    assert a["record"] == b["record"]
    assert a["dims"] == b["dims"] and a["min"] == b["min"]
    assert np.array_equal(a["bytes"], b["bytes"])
    assert np.array_equal(a["table"], b["table"])


def _device_majorant(hk, sh):
    L = hk._lib.lib()
    n = C.c_int32()
    hk._lib.check(L.hk_scene_medium_copy(sh, 0, C.byref(n), None, None), "hk_scene_medium_copy")
    maj = np.full(max(n.value, 1), np.nan, f32)
    mask = np.full((max(n.value, 1) + 31) // 32, 0xdeadbeef, np.uint32)
    hk._lib.check(L.hk_scene_medium_copy(sh, 0, C.byref(n), maj.ctypes.data_as(hk._abi.PF), mask.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_medium_copy")
    return n.value, maj, mask


def _device_bricks(hk, sh):
    L = hk._lib.lib()
    dims = (C.c_int32 * 3)()
    hk._lib.check(L.hk_test_medium_bricks(sh, 0, dims, None), "hk_test_medium_bricks")
    d = tuple(dims)
    if d == (0, 0, 0):
        return d, None
    out = np.full(d + (9, 9, 9), np.nan, f32)
    hk._lib.check(L.hk_test_medium_bricks(sh, 0, dims, out.ctypes.data_as(hk._abi.PF)), "hk_test_medium_bricks")
    return d, out


def _film(hk, s, spp=4, one_sample=False):
    film = hk.Film((W, H))
    cam = hk.PerspectiveCamera((0, 0, -2), (0, 0, 1), film, fov=20.0)
    vp = hk.VolPath(**KW)
    vp._ensure(film)
    vp.clear()
    if one_sample:
        for i in range(1, spp + 1):
            vp.render_samples(s, film, cam, 1, first=i, readback=False)
    else:
        vp.render_samples(s, film, cam, spp, first=1, readback=False)
    acc = vp.read_accumulators(film).copy()
    vp.close()
    return acc


@pytest.fixture(scope="module")
def pair(hk, gpu_ctx):
    """two scenes created alike: one goes through the device builder, the other through the host-built tree"""
    start = _field("holes-a")[0]
    return _scene(hk, gpu_ctx, start), _scene(hk, gpu_ctx, start)


# ---- tree, record and table -------------------------------------------------------------------------------------------------------
def _check_case(hk, pair, name, layout, source):
    (sd, med_d, hd), (sh_, med_h, hh) = pair
    data, buf, meta = _field(name)
    before = _tree(hk, hd), _tree(hk, hh)
    _same_tree(*before)
    want = _host_update(hk, hh, med_h, data)
    got = _dense_update(hk, hd, med_d, data, layout, source)
    assert got == want                                       # the verdict of the host path ...
    after = _tree(hk, hd), _tree(hk, hh)
    _same_tree(*after)                                       # ... and its state
    if want == 0:
        assert np.array_equal(after[0]["bytes"], buf)
        assert after[0]["record"]["leaf_count"] == meta["leaf_count"] and after[0]["record"]["upper_count"] == meta["upper_count"]
        assert after[0]["record"]["index_bbox_min"] == meta["index_min"] and after[0]["record"]["index_bbox_max"] == meta["index_max"]
    else:
        _same_tree(after[0], before[0])


@pytest.mark.parametrize("layout", [0, 1], ids=["x-fastest", "z-fastest"])
@pytest.mark.parametrize("name", list(FIELDS))
def test_tree_record_and_table_equal_the_host_path(hk, pair, name, layout):
    _check_case(hk, pair, name, layout, "host")


# (that the fields have the features they were built for is checked without a device: test_medium_dense_host.py)


# ---- majorant, zero mask, bricks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense_mb", [None, "0"], ids=["bricks", "no-bricks"])
@pytest.mark.parametrize("name", ["holes-b", "136x8x8"])
def test_majorant_mask_and_bricks_equal_the_host_path(hk, gpu_ctx, knobs, name, dense_mb):
    if dense_mb is not None:
        knobs.setenv("HK_NVDB_DENSE_MB", dense_mb)
    start, data = _field("holes-a")[0], _field(name)[0]
    (sd, med_d, hd), (sh_, med_h, hh) = _scene(hk, gpu_ctx, start), _scene(hk, gpu_ctx, start)
    assert _host_update(hk, hh, med_h, data) == 0
    assert _dense_update(hk, hd, med_d, data, hk._abi.HK_DENSE_Z_FASTEST, "host") == 0
    n_d, maj_d, mask_d = _device_majorant(hk, hd)
    n_h, maj_h, mask_h = _device_majorant(hk, hh)
    assert n_d == n_h == int(np.prod(MRES))
    assert np.array_equal(maj_d, maj_h) and np.array_equal(mask_d, mask_h)
    assert (maj_h > 0).any()
    dims_d, bricks_d = _device_bricks(hk, hd)
    dims_h, bricks_h = _device_bricks(hk, hh)
    assert dims_d == dims_h
    if dense_mb == "0":
        assert dims_d == (0, 0, 0)
    else:
        assert dims_d != (0, 0, 0) and np.array_equal(bricks_d, bricks_h)


# ---- films ----------------------------------------------------------------------------------------------------------------------
def test_films_after_the_dense_update(hk, gpu_ctx):
    a, b = _field("holes-a")[0], _field("holes-b")[0]
    (sd, med_d, hd), (sh_, med_h, hh) = _scene(hk, gpu_ctx, a), _scene(hk, gpu_ctx, a)
    created = _film(hk, sd)
    assert _dense_update(hk, hd, med_d, b, hk._abi.HK_DENSE_Z_FASTEST, "host") == 0
    assert _host_update(hk, hh, med_h, b) == 0
    film_b = _film(hk, sd)
    assert np.array_equal(film_b, _film(hk, sh_))
    assert not np.array_equal(film_b, created)
    assert _dense_update(hk, hd, med_d, a, hk._abi.HK_DENSE_X_FASTEST, "host") == 0
    assert np.array_equal(_film(hk, sd), created)            # A -> B -> A: the created scene again


def test_a_noted_call_renders_the_medium_as_it_was(hk, gpu_ctx):
    """two one-sample calls (left noted), the edit, two more: samples 1-2 see A, samples 3-4 see B"""
    a, b = _field("holes-a")[0], _field("holes-b")[0]

    def run(first_two, last_two, edit=None):
        film = hk.Film((W, H))
        cam = hk.PerspectiveCamera((0, 0, -2), (0, 0, 1), film, fov=20.0)
        vp = hk.VolPath(**KW)
        vp._ensure(film)
        vp.clear()
        for i in (1, 2):
            vp.render_samples(first_two, film, cam, 1, first=i, readback=False)
        if edit is not None:
            edit()
        for i in (3, 4):
            vp.render_samples(last_two, film, cam, 1, first=i, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    sd, med_d, hd = _scene(hk, gpu_ctx, a)
    keep = []
    rec, field = _dense_args(hk, med_d, b, hk._abi.HK_DENSE_Z_FASTEST, "host", keep)
    edited = run(sd, sd, edit=lambda: hk._lib.check(hk._lib.lib().hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(field)), "hk_scene_update_medium_dense"))
    want = run(_scene(hk, gpu_ctx, a)[0], _scene(hk, gpu_ctx, b)[0])
    assert np.array_equal(edited, want)
    assert not np.array_equal(edited, _film(hk, _scene(hk, gpu_ctx, b)[0], one_sample=True))


# ---- growth -----------------------------------------------------------------------------------------------------------------------
def test_buffers_grow_and_are_reused(hk, gpu_ctx):
    small, large = _field("8x8x8"), _field("4104x8x8")
    (sd, med_d, hd), (sh_, med_h, hh) = _scene(hk, gpu_ctx, small[0]), _scene(hk, gpu_ctx, small[0])
    for data, buf, _ in (large, small):                      # the tree grows past every buffer, then the small one sits in the large buffers
        assert _dense_update(hk, hd, med_d, data, hk._abi.HK_DENSE_Z_FASTEST, "host") == 0
        assert _host_update(hk, hh, med_h, data) == 0
        td, th = _tree(hk, hd), _tree(hk, hh)
        _same_tree(td, th)
        assert np.array_equal(td["bytes"], buf)
        assert np.array_equal(_film(hk, sd), _film(hk, sh_))


# ---- the Python mirror --------------------------------------------------------------------------------------------------------------
def _check_mirror(hk, ctx, as_field):
    """Scene.update_medium(build="device") with a numpy array or (as_field = to a device tensor) a torch tensor"""
    a, b = _field("holes-a")[0], _field("holes-b")[0]
    (sd, med_d, hd), (sh_, med_h, hh) = _scene(hk, ctx, a), _scene(hk, ctx, a)
    sh_.update_medium(med_h, data=b)
    sd.update_medium(med_d, data=as_field(b), build="device")
    assert med_d._field is not None and med_d._buffer is None          # nothing was built on the host
    _same_tree(_tree(hk, hd), _tree(hk, hh))
    assert np.array_equal(_film(hk, sd), _film(hk, sh_))
    sd.update_medium(med_d, data=as_field(a), build="device")
    assert np.array_equal(_tree(hk, hd)["bytes"], _field("holes-a")[1])
    assert np.array_equal(med_d.buffer, _field("holes-a")[1]) and med_d._field is None    # asked for: built from the kept field


def test_the_mirror_updates_a_device_scene_and_builds_the_host_tree_late(hk, gpu_ctx):
    _check_mirror(hk, gpu_ctx, np.array)


# ---- device tensors -----------------------------------------------------------------------------------------------------------------
def _torch_child():
    """Every field in both layouts from a torch device tensor, the non-finite refusals from device memory, and the mirror with a
    tensor.  Runs in a process in which torch was imported first."""
    import hikari_jl_amd as hk
    ctx = hk.Context.get(0)
    A, L = hk._abi, hk._lib.lib()
    start = _field("holes-a")[0]
    pair = _scene(hk, ctx, start), _scene(hk, ctx, start)
    for name in FIELDS:
        for layout in (A.HK_DENSE_X_FASTEST, A.HK_DENSE_Z_FASTEST):
            _check_case(hk, pair, name, layout, "device")
    (sd, med_d, hd) = pair[0]
    assert _dense_update(hk, hd, med_d, _field("holes-a")[0], A.HK_DENSE_Z_FASTEST, "device") == 0      # (a medium that shows in the film)
    before, film, aux = _tree(hk, hd), _film(hk, sd), (_device_majorant(hk, hd), _device_bricks(hk, hd))
    for bad in (np.nan, np.inf):
        for layout in (A.HK_DENSE_X_FASTEST, A.HK_DENSE_Z_FASTEST):
            poisoned = np.array(_field("holes-b")[0])
            poisoned[19, 16, 8] = bad
            assert _dense_update(hk, hd, med_d, poisoned, layout, "device") == A.HK_ERR_INVALID and b"non-finite voxel" in L.hk_last_error()
            _same_tree(_tree(hk, hd), before)                # the refused call left the tree, ...
            now = _device_majorant(hk, hd), _device_bricks(hk, hd)
            assert all(np.array_equal(x, y) for x, y in zip(now[0], aux[0])) and now[1][0] == aux[1][0] and np.array_equal(now[1][1], aux[1][1])
            assert np.array_equal(_film(hk, sd), film)       # ... majorant, mask, bricks and the film as they were
    import torch
    _check_mirror(hk, ctx, lambda d: torch.from_numpy(np.array(d)).cuda())
    print("device tensors ok")


def test_device_tensors_in_a_process_torch_initialised():
    """(A process of its own: torch brings its own HIP runtime, which has to be the one the process initialises — as in
    test_gpu_parity.py's external accumulators.)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    script = "import sys\nimport torch\nsys.path[:0] = [%r, %r]\nimport test_medium_dense_build as T\nT._torch_child()\n" % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "device tensors ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_scene_untouched(hk, gpu_ctx, knobs):
    A, L = hk._abi, hk._lib.lib()
    a, b = _field("holes-a")[0], _field("holes-b")[0]
    sd, med_d, hd = _scene(hk, gpu_ctx, a)
    state = dict(tree=_tree(hk, hd), film=_film(hk, sd))
    keep = []
    rec, field = _dense_args(hk, med_d, b, A.HK_DENSE_Z_FASTEST, "host", keep)

    def refused(status, needle):
        assert status == A.HK_ERR_INVALID
        msg = L.hk_last_error()
        assert msg and needle in msg, msg
        _same_tree(_tree(hk, hd), state["tree"])
        assert np.array_equal(_film(hk, sd), state["film"])

    copy = lambda r: type(r).from_buffer_copy(r)
    refused(L.hk_scene_update_medium_dense(None, 0, C.byref(rec), C.byref(field)), b"null argument")
    refused(L.hk_scene_update_medium_dense(hd, 0, None, C.byref(field)), b"null argument")
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), None), b"null argument")
    f = copy(field); f.data = None
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(f)), b"null argument")
    refused(L.hk_scene_update_medium_dense(hd, 1, C.byref(rec), C.byref(field)), b"index out of range")
    refused(L.hk_scene_update_medium_dense(hd, -1, C.byref(rec), C.byref(field)), b"index out of range")
    f = copy(field); f.res[1] = 0
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(f)), b"res below 1")
    f = copy(field); f.layout = 2
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(f)), b"unknown layout")
    f = copy(field); f.res[:] = (1 << 15, 1 << 12, 1 << 10)  # 2^28 blocks: refused by its extent alone, before a voxel is read
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(f)), b"more than 2^27 blocks")
    r = copy(rec); r.majorant_res[2] = 8
    refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(r), C.byref(field)), b"majorant_res cannot change")
    for bad in (np.nan, np.inf):                             # (from device memory: test_device_tensors_in_a_process_torch_initialised)
        for layout in (A.HK_DENSE_X_FASTEST, A.HK_DENSE_Z_FASTEST):
            poisoned = np.array(b)
            poisoned[19, 16, 8] = bad                        # the last voxel of the field, in a block that sticks out of it
            r2, f2 = _dense_args(hk, med_d, poisoned, layout, "host", keep)
            refused(L.hk_scene_update_medium_dense(hd, 0, C.byref(r2), C.byref(f2)), b"non-finite voxel")
    knobs.setenv("HK_NVDB_DENSE_MB", "0")                    # the scene was created with bricks: they no longer fit
    assert L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(field)) == A.HK_ERR_INVALID
    assert b"grey_bricks" in L.hk_last_error()
    knobs.restore()
    _same_tree(_tree(hk, hd), state["tree"])
    assert np.array_equal(_film(hk, sd), state["film"])
    assert L.hk_scene_update_medium_dense(hd, 0, C.byref(rec), C.byref(field)) == 0      # the refusals were about the arguments
    assert not np.array_equal(_film(hk, sd), state["film"])

    # a Grid medium
    from hikari_jl_amd import scenes
    gm = hk.GridMedium(_random((13, 10, 7), 9), sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(4, 3, 9))
    gs = scenes.slab_scene(W, H, medium=gm)[0]
    gh = hk.scene_handle(gpu_ctx, gs)
    film = _film(hk, gs)
    assert L.hk_scene_update_medium_dense(gh, 0, C.byref(rec), C.byref(field)) == A.HK_ERR_INVALID
    assert b"not a NanoVDB medium" in L.hk_last_error()
    n = C.c_int64()
    assert L.hk_scene_medium_tree_copy(gh, 0, None, C.byref(n), None, None, None, None) == A.HK_ERR_INVALID
    assert np.array_equal(_film(hk, gs), film)
