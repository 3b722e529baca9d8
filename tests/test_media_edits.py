"""Media edited in place on the device (hk_scene_update_medium).  The contract is that of test_light_edits.py: after an edit the device
scene is, bit for bit, the scene hk_scene_create builds from the edited description.  Every test creates a scene from volume A, updates
it to volume B in place, and holds it against a second source: the majorant grid and its zero-cell mask against the host builders of
media.py (hk_scene_medium_copy), the NanoVDB halo bricks against the layout recomputed in NumPy from the dense field
(hk_test_medium_bricks), the films against a scene created FRESH from B.  Comparisons are np.array_equal; there are no tolerances.

Shapes are the smallest at which the build kernels can go wrong: 13x10x7 voxels under a (4, 3, 9) majorant (boxes that do not divide
evenly, a z axis finer than the data — single voxels shared between cells —, 108 cells = a last mask word that is partly used),
150x6x5 under (2, 2, 2) (75 voxels along x per cell: more than a wave's width, so the lane stride and the cross-lane reduce both run),
(5, 5, 3) = 75 cells (the mask crosses a 64-cell ballot), and for NanoVDB a 20x17x9 field with holes under (5, 4, 3) whose update
activates a block, drops another, and changes the block-grid extent and the tree size.  Each majorant case runs with a cell per wave
(the default at these sizes) and with a cell per block (HK_MAJORANT_BLOCK_VOXELS=0), the two ways the launcher can go."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 40, 32
KW = dict(max_depth=5, samples=4)
BOUNDS = ((-2.5, -2.6, 1.0), (2.5, 2.6, 2.0))          # the slab of scenes.slab_scene
CELL_MODES = [pytest.param(None, id="wave-per-cell"), pytest.param("0", id="block-per-cell")]


# ---- scenes, films, read-backs ------------------------------------------------------------------------------------------------
def _scene(hk, medium):
    from hikari_jl_amd import scenes
    return scenes.slab_scene(W, H, medium=medium)[0]


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


def _device_majorant(hk, ctx, s, idx=0):
    L = hk._lib.lib()
    sh = hk.scene_handle(ctx, s)
    n = C.c_int32()
    hk._lib.check(L.hk_scene_medium_copy(sh, idx, C.byref(n), None, None), "hk_scene_medium_copy")
    maj = np.full(max(n.value, 1), np.nan, f32)
    mask = np.full((max(n.value, 1) + 31) // 32, 0xdeadbeef, np.uint32)
    hk._lib.check(L.hk_scene_medium_copy(sh, idx, C.byref(n), maj.ctypes.data_as(hk._abi.PF), mask.ctypes.data_as(C.POINTER(C.c_uint32))), "hk_scene_medium_copy")
    return n.value, maj, mask


def _pack_mask(maj):
    """bit c of the mask <=> maj[c] == 0, 32 cells per word, the unused bits of the last word 0 (bake_medium's packing)"""
    bits = np.zeros((maj.size + 31) // 32 * 32, np.uint8)
    bits[:maj.size] = maj == 0
    return np.packbits(bits, bitorder="little").view(np.uint32)


def _device_bricks(hk, ctx, s, idx=0):
    L = hk._lib.lib()
    sh = hk.scene_handle(ctx, s)
    dims = (C.c_int32 * 3)()
    hk._lib.check(L.hk_test_medium_bricks(sh, idx, dims, None), "hk_test_medium_bricks")
    d = tuple(dims)
    if d == (0, 0, 0):
        return d, None
    out = np.full(d + (9, 9, 9), np.nan, f32)
    hk._lib.check(L.hk_test_medium_bricks(sh, idx, dims, out.ctypes.data_as(hk._abi.PF)), "hk_test_medium_bricks")
    return d, out


def _numpy_bricks(meta):
    """nvdb_dense_bricks' layout from the dense field the tree was built from: the block table spans the blocks of the index bounding
    box and one block of margin; brick (bx, by, bz) is the block's 8^3 voxels and the first plane of its +x / +y / +z neighbours."""
    lo = [v >> 3 for v in meta["index_min"]]
    hi = [v >> 3 for v in meta["index_max"]]
    nvb_min = [l - 1 for l in lo]
    dim = tuple(max(h - l + 3, 3) for l, h in zip(lo, hi))
    field = np.full(tuple(8 * d + 1 for d in dim), f32(meta["background"]), f32)
    pad = meta["dense"]                                      # block-aligned, voxel (0, 0, 0) at index (0, 0, 0)
    o = [-8 * m for m in nvb_min]
    field[o[0]:o[0] + pad.shape[0], o[1]:o[1] + pad.shape[1], o[2]:o[2] + pad.shape[2]] = pad
    out = np.empty(dim + (9, 9, 9), f32)
    for bx in range(dim[0]):
        for by in range(dim[1]):
            for bz in range(dim[2]):
                out[bx, by, bz] = field[8 * bx:8 * bx + 9, 8 * by:8 * by + 9, 8 * bz:8 * bz + 9]
    return dim, out


def _box(i, n, r):
    """0-based voxel slice of majorant cell i along an axis of n voxels and r cells (media.jl:1459-1493), for placing test values"""
    return slice(max(1, i * n // r + 1) - 1, min(n, -(-(i + 1) * n // r)))


def _check_majorant(hk, ctx, s, medium):
    """the device's grid and mask against the host builder of media.py for the medium as it is now"""
    want = medium._build_majorant()
    n, maj, mask = _device_majorant(hk, ctx, s)
    assert n == want.size == int(np.prod(medium.majorant_res))
    assert np.array_equal(maj, want)
    assert np.array_equal(mask, _pack_mask(want))
    return want


# ---- volumes ------------------------------------------------------------------------------------------------------------------
def _grid_volumes(shape, mres, seed, negatives=True):
    """A: random; B: random, with a whole cell of zeros, a whole cell of negative values (`negatives`: the volumes that are rendered
    have a second cell of zeros instead), and the maximum of a cell in the last voxel of its box's last row.
    -> A, B, {cell: expected majorant value of B}"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 2.0, shape).astype(f32)
    b = rng.uniform(0.1, 2.0, shape).astype(f32)
    last = tuple(r - 1 for r in mres)
    cells = {"zero": (0, 0, 0), "negative": last, "corner": (min(1, mres[0] - 1), 0, min(1, mres[2] - 1))}
    box = lambda c: tuple(_box(c[k], shape[k], mres[k]) for k in range(3))
    b[box(cells["zero"])] = 0.0
    b[box(cells["negative"])] = -rng.uniform(0.5, 1.0, b[box(cells["negative"])].shape).astype(f32) if negatives else 0.0
    cb = box(cells["corner"])
    b[cb[0].stop - 1, cb[1].stop - 1, cb[2].stop - 1] = 9.0
    flat = lambda c: c[0] + mres[0] * (c[1] + mres[1] * c[2])
    return a, b, {flat(cells["zero"]): 0.0, flat(cells["negative"]): 0.0, flat(cells["corner"]): 9.0}


def _rgb_volumes(shape, seed):
    """voxels whose largest channel changes from place to place (the box maximum sits in another channel per cell)"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 1.0, shape + (3,)).astype(f32)
    x, y, z = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    ch = (x // 3 + y // 3 + z) % 3
    for c in range(3):
        g[..., c] += np.where(ch == c, f32(2.0), f32(0.0))
    return g


def _nvdb_volumes():
    """20x17x9 fields with holes.  A lives in x < 8 (one block along x, the +z layer of blocks partly empty); B lives in x >= 8 (two blocks
    along x): every block A had is dropped, blocks A lacked are activated, the index bounding box, the block-grid extent and the tree
    size all change (B's tree is the larger one)."""
    rng = np.random.default_rng(21)
    a = np.zeros((20, 17, 9), f32)
    a[:8] = rng.uniform(0.2, 3.0, (8, 17, 9)).astype(f32)
    a[2:5, 3:9, 1:4] = 0.0                                   # a hole inside a leaf
    a[:8, 8:16, :8] = 0.0                                    # a whole block absent
    b = np.zeros((20, 17, 9), f32)
    b[8:] = rng.uniform(0.2, 3.0, (12, 17, 9)).astype(f32)
    b[10:13, 0:5, 2:8] = 0.0
    b[16:20, 0:8, 0:8] = 0.0                                 # block (2, 0, 0) absent
    return a, b


# ---- the majorant and the mask against the second source -----------------------------------------------------------------------
@pytest.mark.parametrize("block_voxels", CELL_MODES)
@pytest.mark.parametrize("shape,mres", [((13, 10, 7), (4, 3, 9)), ((150, 6, 5), (2, 2, 2))])
def test_grid_majorant_built_on_the_device_equals_the_host_builder(hk, gpu_ctx, knobs, shape, mres, block_voxels):
    if block_voxels is not None:
        knobs.setenv("HK_MAJORANT_BLOCK_VOXELS", block_voxels)
    a, b, expect = _grid_volumes(shape, mres, seed=3)
    med = hk.GridMedium(a, sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), g=0.2, bounds=BOUNDS, majorant_res=mres)
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    s.update_medium(med, density=b)
    want = _check_majorant(hk, gpu_ctx, s, med)
    for cell, value in expect.items():                       # the volume has the features it was built to have
        assert want[cell] == value
    assert (want == 0).sum() >= 2


@pytest.mark.parametrize("block_voxels", CELL_MODES)
def test_zero_mask_crosses_a_ballot(hk, gpu_ctx, knobs, block_voxels):
    """(5, 5, 3) = 75 cells over 10x10x6 voxels (boxes of 2x2x2, disjoint): cells 60 .. 70 are empty in B, so the set bits run across
    the 64-cell boundary of the wave that builds the mask, and the third word has 11 cells in use."""
    if block_voxels is not None:
        knobs.setenv("HK_MAJORANT_BLOCK_VOXELS", block_voxels)
    rng = np.random.default_rng(5)
    a = rng.uniform(0.1, 1.0, (10, 10, 6)).astype(f32)
    b = rng.uniform(0.1, 1.0, (10, 10, 6)).astype(f32)
    for cell in range(60, 71):
        ix, iy, iz = cell % 5, (cell // 5) % 5, cell // 25
        b[2 * ix:2 * ix + 2, 2 * iy:2 * iy + 2, 2 * iz:2 * iz + 2] = 0.0
    med = hk.GridMedium(a, sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(5, 5, 3))
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    _, _, mask_a = _device_majorant(hk, gpu_ctx, s)
    assert not mask_a.any()
    s.update_medium(med, density=b)
    want = _check_majorant(hk, gpu_ctx, s, med)
    assert list(np.flatnonzero(want == 0)) == list(range(60, 71))


@pytest.mark.parametrize("block_voxels", CELL_MODES)
@pytest.mark.parametrize("with_sigma_a", [False, True], ids=["sigma_a-absent", "both-grids"])
def test_rgb_grid_majorant_built_on_the_device_equals_the_host_builder(hk, gpu_ctx, knobs, with_sigma_a, block_voxels):
    if block_voxels is not None:
        knobs.setenv("HK_MAJORANT_BLOCK_VOXELS", block_voxels)
    shape, mres = (13, 10, 7), (4, 3, 9)
    grids_a = dict(sigma_s_grid=_rgb_volumes(shape, 1) * f32(0.3))
    grids_b = dict(sigma_s_grid=_rgb_volumes(shape, 2) * f32(0.4))
    if with_sigma_a:
        grids_a["sigma_a_grid"] = _rgb_volumes(shape, 3) * f32(0.05)
        grids_b["sigma_a_grid"] = _rgb_volumes(shape, 4) * f32(0.07)
        grids_b["sigma_a_grid"][tuple(_box(c, n, r) for c, n, r in zip((3, 2, 8), shape, mres))] = -1.0   # a cell of negative voxels: clamped at 0
    med = hk.RGBGridMedium(sigma_scale=1.3, g=0.1, bounds=BOUNDS, majorant_res=mres, **grids_a)
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    s.update_medium(med, sigma_scale=1.7, **grids_b)
    want = _check_majorant(hk, gpu_ctx, s, med)
    top = np.argmax(med.sigma_s_grid[..., :3].reshape(-1, 3), axis=1)
    assert len(set(top.tolist())) == 3                      # every channel is the largest somewhere
    assert np.isfinite(want).all() and (want > 0).all()
    if not with_sigma_a:                                    # (the other volume has negative absorption in a cell: it is not rendered)
        assert np.array_equal(_film(hk, s), _film(hk, _scene(hk, hk.RGBGridMedium(sigma_scale=1.7, g=0.1, bounds=BOUNDS, majorant_res=mres, **grids_b))))


@pytest.mark.parametrize("block_voxels", CELL_MODES)
@pytest.mark.parametrize("dense_mb", [None, "0"], ids=["bricks", "no-bricks"])
def test_nanovdb_majorant_and_bricks_built_on_the_device(hk, gpu_ctx, knobs, dense_mb, block_voxels):
    if dense_mb is not None:
        knobs.setenv("HK_NVDB_DENSE_MB", dense_mb)
    if block_voxels is not None:
        knobs.setenv("HK_MAJORANT_BLOCK_VOXELS", block_voxels)
    a, b = _nvdb_volumes()
    kw = dict(bounds=BOUNDS, sigma_a=hk.RGBSpectrum(0.02), sigma_s=hk.RGBSpectrum(0.5), g=0.3, majorant_res=(5, 4, 3))
    med = hk.NanoVDBMedium(a, **kw)
    size_a, bbox_a = med.buffer.size, (med.meta["index_min"], med.meta["index_max"])
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    dims_a, bricks_a = _device_bricks(hk, gpu_ctx, s)
    s.update_medium(med, data=b)
    assert med.buffer.size > size_a and (med.meta["index_min"], med.meta["index_max"]) != bbox_a   # the tree grew, the extent moved
    want = _check_majorant(hk, gpu_ctx, s, med)
    assert (want == 0).any() and (want > 0).any()
    dims, bricks = _device_bricks(hk, gpu_ctx, s)
    if dense_mb == "0":
        assert dims == dims_a == (0, 0, 0)
    else:
        want_dims, want_bricks = _numpy_bricks(med.meta)
        assert dims == want_dims and dims != dims_a
        assert np.array_equal(bricks, want_bricks)
        assert np.array_equal(bricks_a, _numpy_bricks(hk.NanoVDBMedium(a, **kw).meta)[1])   # (and the read-back shows hk_scene_create's host build too)
    fresh = _scene(hk, hk.NanoVDBMedium(b, **kw))
    assert np.array_equal(_film(hk, s), _film(hk, fresh))
    assert np.array_equal(_film(hk, s, one_sample=True), _film(hk, fresh, one_sample=True))


# ---- every kind of change: the edited scene renders the fresh scene's film -------------------------------------------------------
def _media(hk):
    """kind -> (constructor keywords of A, the update, constructor keywords of B)"""
    ga, gb, _ = _grid_volumes((13, 10, 7), (4, 3, 9), seed=8, negatives=False)
    grid = dict(sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), g=0.2, bounds=BOUNDS, majorant_res=(4, 3, 9))
    T = np.eye(4, dtype=f32)
    T[:3, :3] *= f32(1.25)
    T[:3, 3] = (0.1, -0.2, 0.05)
    wide = ((-2.75, -2.5, 0.75), (2.5, 2.75, 2.25))
    return {
        "grid-data": (hk.GridMedium, dict(grid, density=ga), dict(density=gb), dict(grid, density=gb)),
        "grid-coefficients": (hk.GridMedium, dict(grid, density=ga), dict(sigma_a=hk.RGBSpectrum(0.3), sigma_s=hk.RGBSpectrum(0.25), g=-0.4),
                              dict(grid, density=ga, sigma_a=hk.RGBSpectrum(0.3), sigma_s=hk.RGBSpectrum(0.25), g=-0.4)),
        "grid-bounds-transform": (hk.GridMedium, dict(grid, density=ga), dict(bounds=wide, transform=T), dict(grid, density=ga, bounds=wide, transform=T)),
        "homogeneous-coefficients": (hk.HomogeneousMedium, dict(sigma_a=hk.RGBSpectrum(0.02), sigma_s=hk.RGBSpectrum(0.4), g=0.1),
                                     dict(sigma_a=hk.RGBSpectrum(0.1, 0.2, 0.3), sigma_s=hk.RGBSpectrum(0.9, 0.5, 0.2), Le=hk.RGBSpectrum(0.05), g=0.6),
                                     dict(sigma_a=hk.RGBSpectrum(0.1, 0.2, 0.3), sigma_s=hk.RGBSpectrum(0.9, 0.5, 0.2), Le=hk.RGBSpectrum(0.05), g=0.6)),
    }


@pytest.mark.parametrize("case", ["grid-data", "grid-coefficients", "grid-bounds-transform", "homogeneous-coefficients"])
def test_edited_medium_renders_the_fresh_scene(hk, gpu_ctx, case):
    cls, kw_a, change, kw_b = _media(hk)[case]
    kw = lambda d: {k: v for k, v in d.items() if k != "density"}
    make = lambda d: cls(d["density"], **kw(d)) if "density" in d else cls(**d)
    med = make(kw_a)
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)                              # created first: the edit is the in-place one
    before = _film(hk, s)
    s.update_medium(med, **change)
    after = _film(hk, s)
    fresh = _scene(hk, make(kw_b))
    assert np.array_equal(after, _film(hk, fresh))
    assert not np.array_equal(before, after)
    assert np.array_equal(_film(hk, s, one_sample=True), _film(hk, fresh, one_sample=True))   # one-sample calls: noted, then one pass
    if cls is not hk.HomogeneousMedium:
        _check_majorant(hk, gpu_ctx, s, med)


def test_a_to_b_to_a_gives_the_created_scene_again(hk, gpu_ctx):
    a, b = _nvdb_volumes()
    kw = dict(bounds=BOUNDS, sigma_a=hk.RGBSpectrum(0.02), sigma_s=hk.RGBSpectrum(0.5), g=0.3, majorant_res=(5, 4, 3))
    med = hk.NanoVDBMedium(a, **kw)
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    created = (_film(hk, s), _device_majorant(hk, gpu_ctx, s), _device_bricks(hk, gpu_ctx, s))
    s.update_medium(med, data=b)
    assert not np.array_equal(_film(hk, s), created[0])
    s.update_medium(med, data=a)                             # the smaller tree again, in the buffers B made larger
    again = (_film(hk, s), _device_majorant(hk, gpu_ctx, s), _device_bricks(hk, gpu_ctx, s))
    assert np.array_equal(again[0], created[0])
    assert again[1][0] == created[1][0] and np.array_equal(again[1][1], created[1][1]) and np.array_equal(again[1][2], created[1][2])
    assert again[2][0] == created[2][0] and np.array_equal(again[2][1], created[2][1])
    ga, gb, _ = _grid_volumes((13, 10, 7), (4, 3, 9), seed=8, negatives=False)
    gm = hk.GridMedium(ga, sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(4, 3, 9))
    gs = _scene(hk, gm)
    hk.scene_handle(gpu_ctx, gs)
    first = (_film(hk, gs), _device_majorant(hk, gpu_ctx, gs))
    gs.update_medium(gm, density=gb)
    gs.update_medium(gm, density=ga)
    assert np.array_equal(_film(hk, gs), first[0]) and np.array_equal(_device_majorant(hk, gpu_ctx, gs)[1], first[1][1])


def test_noted_calls_render_the_medium_as_it_was(hk, gpu_ctx):
    """two one-sample calls (left noted), the edit, two more: samples 1-2 see A, samples 3-4 see B"""
    ga, gb, _ = _grid_volumes((13, 10, 7), (4, 3, 9), seed=8, negatives=False)
    kw = dict(sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), g=0.2, bounds=BOUNDS, majorant_res=(4, 3, 9))

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

    med = hk.GridMedium(ga, **kw)
    s = _scene(hk, med)
    hk.scene_handle(gpu_ctx, s)
    edited = run(s, s, edit=lambda: s.update_medium(med, density=gb))
    want = run(_scene(hk, hk.GridMedium(ga, **kw)), _scene(hk, hk.GridMedium(gb, **kw)))
    assert np.array_equal(edited, want)
    assert not np.array_equal(edited, _film(hk, _scene(hk, hk.GridMedium(gb, **kw)), one_sample=True))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _record(hk, medium, keep):
    rec = hk._abi.hk_medium()
    medium.fill_record(rec, keep, majorant=False)
    return rec


def test_refused_medium_edits_leave_the_scene_untouched(hk, gpu_ctx, knobs):
    A = hk._abi
    L = hk._lib.lib()
    keep = []
    ga, gb, _ = _grid_volumes((13, 10, 7), (4, 3, 9), seed=8, negatives=False)
    gm = hk.GridMedium(ga, sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(4, 3, 9))
    gs = _scene(hk, gm)
    gh = hk.scene_handle(gpu_ctx, gs)
    state = {"s": gs, "film": _film(hk, gs)}

    def refused(status, needle):
        assert status == A.HK_ERR_INVALID
        msg = L.hk_last_error()
        assert msg and needle in msg, msg
        assert np.array_equal(_film(hk, state["s"]), state["film"])     # the scene renders what it rendered before the call

    ok = _record(hk, hk.GridMedium(gb, sigma_a=hk.RGBSpectrum(0.05), sigma_s=hk.RGBSpectrum(0.6), bounds=BOUNDS, majorant_res=(4, 3, 9)), keep)
    copy = lambda r: A.hk_medium.from_buffer_copy(r)
    refused(L.hk_scene_update_medium(None, 0, C.byref(ok)), b"null argument")
    refused(L.hk_scene_update_medium(gh, 0, None), b"null argument")
    refused(L.hk_scene_update_medium(gh, 1, C.byref(ok)), b"index out of range")
    refused(L.hk_scene_update_medium(gh, -1, C.byref(ok)), b"index out of range")
    r = copy(ok); r.kind = A.HK_MEDIUM_HOMOGENEOUS
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"kind differs")
    r = copy(ok); r.res[0] = 12
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"res cannot change")
    r = copy(ok); r.majorant_res[2] = 8
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"majorant_res cannot change")
    for bad in (np.inf, np.nan):
        r = copy(ok); r.bounds_max[1] = bad
        refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"non-finite bounds")
    r = copy(ok); r.render_to_medium[5] = np.nan
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"non-finite transform")
    r = copy(ok); r.sigma_s[:] = (0.9, 0.5, 0.2, 1.0)             # the one medium of the scene is grey: it runs the grey kernels
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"class of the scene's media")
    r = copy(ok); r.density = None
    refused(L.hk_scene_update_medium(gh, 0, C.byref(r)), b"without density")
    assert L.hk_scene_update_medium(gh, 0, C.byref(ok)) == 0       # the refusals were about the arguments
    assert not np.array_equal(_film(hk, gs), state["film"])

    # an RGB grid that appears
    shape = (13, 10, 7)
    rm = hk.RGBGridMedium(sigma_s_grid=_rgb_volumes(shape, 1) * f32(0.3), bounds=BOUNDS, majorant_res=(4, 3, 9))
    rs = _scene(hk, rm)
    rh = hk.scene_handle(gpu_ctx, rs)
    state.update(s=rs, film=_film(hk, rs))
    both = _record(hk, hk.RGBGridMedium(sigma_a_grid=_rgb_volumes(shape, 3) * f32(0.05), sigma_s_grid=_rgb_volumes(shape, 2) * f32(0.4), bounds=BOUNDS, majorant_res=(4, 3, 9)), keep)
    refused(L.hk_scene_update_medium(rh, 0, C.byref(both)), b"cannot appear or disappear")
    r = copy(both); r.sigma_a_grid = None; r.sigma_s_grid = None
    refused(L.hk_scene_update_medium(rh, 0, C.byref(r)), b"RGBGridMedium needs")

    # bricks that no longer fit the budget
    a, b = _nvdb_volumes()
    kw = dict(bounds=BOUNDS, sigma_a=hk.RGBSpectrum(0.02), sigma_s=hk.RGBSpectrum(0.5), majorant_res=(5, 4, 3))
    nm = hk.NanoVDBMedium(a, **kw)
    ns = _scene(hk, nm)
    nh = hk.scene_handle(gpu_ctx, ns)
    state.update(s=ns, film=_film(hk, ns))
    nb = _record(hk, hk.NanoVDBMedium(b, **kw), keep)
    r = copy(nb); r.inv_mat[4] = np.inf
    refused(L.hk_scene_update_medium(nh, 0, C.byref(r)), b"non-finite inv_mat")
    knobs.setenv("HK_NVDB_DENSE_MB", "0")
    assert L.hk_scene_update_medium(nh, 0, C.byref(nb)) == A.HK_ERR_INVALID
    assert b"grey_bricks" in L.hk_last_error()
    knobs.restore()
    assert np.array_equal(_film(hk, ns), state["film"])
    assert L.hk_scene_update_medium(nh, 0, C.byref(nb)) == 0
    assert np.array_equal(_film(hk, ns), _film(hk, _scene(hk, hk.NanoVDBMedium(b, **kw))))
