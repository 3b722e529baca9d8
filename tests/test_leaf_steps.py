"""The flush of the closest-hit kernel of opaque scenes without media (k_trace_lean) follows the scene's materials: without the
MixMaterial resolve when no record is a Mix (DScene::has_mix), and for ONE material kind when all records share it
(DScene::single_kind).  Neither touches the arithmetic nor the order of the queue entries: films, ray counts and queue sizes are
compared exactly.  Films this small would be ONE k_small_pass launch, which keeps its own flush: every render here runs the stages as
launches (HK_SMALL_PASS_FUSED=0).  (The single-triangle leaf steps this file was named for were measured and not kept: LAB_NOTEBOOK.)"""
import ctypes as C

import numpy as np
import pytest

import bvh_scenes as D
import test_bvh_rebuild as B
import test_parity_holes as P

pytestmark = pytest.mark.gpu
f32 = np.float32
PI = C.POINTER(C.c_int32)
COUNTERS = ("rays_closest", "rays_shadow", "hits_accepted", "path_vertices")
KNOBS = ("HK_NODE_CACHE", "HK_SMALL_PASS_FUSED", "HK_QNODES")
CORNELL_CAM = ((0, 1, -3.5), (0, 1, 0), 40.0)


def _queue_counts(hk, vp, depth, kind):
    """entries of the kind's shading queue per wave segment at bounce `depth` of the last pass, and how many carry the emissive flag"""
    L = hk._lib.lib()
    n = C.c_int32()
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), None, None), "hk_test_queue_counts")
    out, fl = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    hk._lib.check(L.hk_test_queue_counts(vp._integ, depth, kind, C.byref(n), out.ctypes.data_as(PI), fl.ctypes.data_as(PI)), "hk_test_queue_counts")
    return out, fl


def _render(hk, knobs, s, cam_args, size, kw, spp, env=None):
    """film accumulators, counters, and the Matte queue's segment sizes at bounces 0 and 1"""
    knobs.delenv("HK_NODE_CACHE", raising=False)
    knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    for k, v in (env or {}).items():
        knobs.setenv(k, v)
    film = hk.Film(size)
    cam = hk.PerspectiveCamera(cam_args[0], cam_args[1], film, fov=cam_args[2])
    vp = hk.VolPath(**kw)
    try:
        vp._ensure(film)
        vp.clear()
        vp.reset_stats()
        vp.render_samples(s, film, cam, spp, first=1)
        acc = vp.read_accumulators(film).copy()
        st = vp.stats()
        assert int(st.fused_passes) == 0
        queues = [_queue_counts(hk, vp, d, hk._abi.HK_MAT_MATTE) for d in (0, 1)]
        return acc, tuple(int(getattr(st, k)) for k in COUNTERS), queues
    finally:
        vp.close()


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert a[1] == b[1], (a[1], b[1])
    for (qa, fa), (qb, fb) in zip(a[2], b[2]):
        assert np.array_equal(qa, qb) and np.array_equal(fa, fb)


def _pair(hk, ctx, knobs, which):
    """the same all-Matte geometry twice: as it is (one material kind), and with a Mirror record no triangle refers to (two kinds)"""
    from hikari_jl_amd import scenes
    out = []
    for extra in (False, True):
        if which == "cornell":      # the whole tree in the block's LDS
            s, _, _ = scenes.cornell_box(64, 64, objects="two_spheres")
            view = (CORNELL_CAM, (64, 64))
        else:                       # a chain of clusters 22 levels deep: 32-entry stacks, quantised nodes unless created with HK_QNODES=0
            if which == "deep_float":
                knobs.setenv("HK_QNODES", "0")
            s, _ = B._cluster_scene(hk, D.skewed_positions(12, 256, 0.25))
            view = (((5.0, 0.9, -6.5), (5.0, 0.9, 0.9), 60.0), (64, 48))
        if extra:
            s.push_material(hk.MirrorMaterial())
            s.sync()
        kinds = {s.desc.materials[i].kind for i in range(s.desc.n_materials)}
        assert kinds == ({hk._abi.HK_MAT_MATTE, hk._abi.HK_MAT_MIRROR} if extra else {hk._abi.HK_MAT_MATTE})
        hk.scene_handle(ctx, s)     # (HK_QNODES is read when the device scene is built)
        assert (B._info(hk, ctx, s)[2] > 16) == (which != "cornell")
        out.append(s)
    return out[0], out[1], view


@pytest.mark.parametrize("which", ["cornell", "deep", "deep_float"])
def test_single_kind_flush_is_result_neutral(hk, gpu_ctx, knobs, which):
    """A scene whose records are all Matte runs the single-kind flush; a Mirror record that no triangle refers to makes it a scene of
    two kinds, which runs the general Mix-free one.  Same film, same rays and hits, the same entries per segment of the Matte queue
    and the same emissive flags among them — with the node cache and without."""
    one, two, (cam_args, size) = _pair(hk, gpu_ctx, knobs, which)
    kw = dict(max_depth=4, samples=16)
    try:
        ref = _render(hk, knobs, two, cam_args, size, kw, 16)
        lit = (ref[0].reshape(4, -1)[:3] > 0).any(axis=0).sum()
        assert np.isfinite(ref[0]).all() and lit > 100 and min(ref[1]) > 0, (lit, ref[1])
        assert all(q.sum() > 0 for q, _ in ref[2])
        if which == "cornell":
            assert ref[2][0][1].sum() > 0                                        # camera rays that hit the light: flagged entries
        for s in (one, two):
            for env in ({}, {"HK_NODE_CACHE": "0"}):
                _same(_render(hk, knobs, s, cam_args, size, kw, 16, env), ref)
    finally:
        for k in KNOBS:
            knobs.delenv(k, raising=False)


def _edit_round_trip(hk, ctx, knobs, make, w, h):
    """make() builds a scene with MixMaterials.  A second copy is created with a Matte record in place of every Mix, rendered, edited
    into the first (hk_scene_update_materials), rendered, edited back, rendered."""
    A = hk._abi
    L = hk._lib.lib()
    s_mix, s_edit = make(), make()
    d_mix, d_edit = s_mix.desc, s_edit.desc
    kinds = [d_mix.materials[i].kind for i in range(d_mix.n_materials)]
    mixes = [i for i, k in enumerate(kinds) if k == A.HK_MAT_MIX]
    matte = kinds.index(A.HK_MAT_MATTE)
    assert mixes
    mix_recs = [A.hk_material.from_buffer_copy(d_mix.materials[i]) for i in mixes]
    plain = A.hk_material.from_buffer_copy(d_mix.materials[matte])
    for i in mixes:                                                              # before the device scene exists: created without a Mix
        d_edit.materials[i] = plain
    sh = hk.scene_handle(ctx, s_edit)
    kw = dict(max_depth=4, samples=8)
    render = lambda s: _render(hk, knobs, s, CORNELL_CAM, (w, h), kw, 8)
    try:
        with_mix = render(s_mix)
        created = render(s_edit)
        assert np.isfinite(with_mix[0]).all() and with_mix[0].max() > 0 and not np.array_equal(with_mix[0], created[0])
        for i, r in zip(mixes, mix_recs):
            hk._lib.check(L.hk_scene_update_materials(sh, i, 1, C.byref(r)), "hk_scene_update_materials")
        _same(render(s_edit), with_mix)
        for i in mixes:
            hk._lib.check(L.hk_scene_update_materials(sh, i, 1, C.byref(plain)), "hk_scene_update_materials")
        _same(render(s_edit), created)
    finally:
        for k in KNOBS:
            knobs.delenv(k, raising=False)
    return (s_mix, s_edit), sh, mixes, mix_recs, matte, plain, kinds       # (the scenes own the device scene behind `sh`)


def test_mix_free_kernel_follows_the_scene(hk, gpu_ctx, knobs):
    """A scene created WITHOUT a MixMaterial runs the closest-hit kernel without the resolve.  An edit turns three of its materials
    into the mixes of test_mix_resolve_bit_exact's scene: the film must be, bit for bit, that of the scene created with them; the edit
    back gives the first film again.  What stays refused: a change of kind that involves no Mix, a Mix child out of range."""
    A = hk._abi
    L = hk._lib.lib()
    keep, sh, mixes, mix_recs, matte, plain, kinds = _edit_round_trip(hk, gpu_ctx, knobs, lambda: P._mix_scene(hk, w=48, h=48)[0], 48, 48)
    assert len(mixes) == 3 and len(set(kinds) - {A.HK_MAT_MIX}) > 1
    bad = A.hk_material.from_buffer_copy(plain)
    bad.kind = A.HK_MAT_GLASS
    assert L.hk_scene_update_materials(sh, matte, 1, C.byref(bad)) == A.HK_ERR_INVALID
    r = A.hk_material.from_buffer_copy(mix_recs[0])
    r.i[0] = len(kinds)
    assert L.hk_scene_update_materials(sh, mixes[0], 1, C.byref(r)) == A.HK_ERR_INVALID


def _matte_mix_scene(hk):
    """the two-spheres Cornell box with a Mix of two Matte materials on the first sphere: Matte is the only kind a hit resolves to"""
    from hikari_jl_amd import scenes
    mix = hk.MixMaterial((hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7, 0.3, 0.2)), hk.MatteMaterial(Kd=hk.RGBSpectrum(0.2, 0.3, 0.7))), 0.4)
    return scenes.cornell_box(48, 48, objects="two_spheres", tess=12, object_material=mix)[0]


def test_single_kind_follows_the_scene(hk, gpu_ctx, knobs):
    """All records Matte: the single-kind flush.  One of them becomes a Mix of two Matte records (the flush with the resolve), and a
    Matte again: the films of the scenes created that way, bit for bit.  A Mix cannot become a kind the scene was not created with."""
    A = hk._abi
    L = hk._lib.lib()
    keep, sh, mixes, mix_recs, matte, plain, kinds = _edit_round_trip(hk, gpu_ctx, knobs, lambda: _matte_mix_scene(hk), 48, 48)
    assert len(mixes) == 1 and set(kinds) == {A.HK_MAT_MIX, A.HK_MAT_MATTE}
    hk._lib.check(L.hk_scene_update_materials(sh, mixes[0], 1, C.byref(mix_recs[0])), "hk_scene_update_materials")
    bad = A.hk_material.from_buffer_copy(plain)
    bad.kind = A.HK_MAT_MIRROR
    assert L.hk_scene_update_materials(sh, mixes[0], 1, C.byref(bad)) == A.HK_ERR_INVALID
