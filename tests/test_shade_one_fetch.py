"""One mat_id read and one material index per vertex in shade_body (hk_shade.h).  The vertex used to read mat_id[slot] for matte_kd,
again for the next-event block and again for the BSDF block, each read followed by the indexed load of the material record; now the
index is taken once at the top of the vertex — from the mat_id word the chunk already holds under the slot walk, by one load under
the queue walk and in the general body — and every use of the record goes through it.  The change reaches every body shade_body
has, so every case is rendered the five ways of test_shade_slot_walk.py — the default (slot walk), HK_SHADE_SLOT_WALK=0,
HK_SHADE_PREFETCH=0, HK_SHADE_PRESCAN=1 (queue walk) and HK_SHADE_LEAN=0 (the general instantiation) — and compared bit for bit: film
accumulators and the ray / vertex / hit / light-node counters; and across a Matte -> Mix -> Matte edit of a material record, where the
walk goes off and on again with DScene::single_kind."""
import ctypes as C

import numpy as np
import pytest

import test_leaf_steps as LS
import test_shade_slot_walk as SW

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spp", [16, 64])
@pytest.mark.parametrize("size", [(37, 29), (64, 48)])
@pytest.mark.parametrize("view", ["open", "closed", "light"])
def test_five_ways_bit_for_bit(hk, knobs, view, size, spp):
    """the three boxes of several Matte records (white, red, green, the light's black) at depth 3"""
    build = SW._box(hk, size[0], size[1], view)
    desc = build()[0].desc
    assert len({bytes(desc.materials[i]) for i in range(desc.n_materials)}) >= 4      # the index matters: the records differ
    SW._compare(hk, knobs, build, spp, 3)


def test_five_ways_deep_paths(hk, knobs):
    """depth 8: the second half of the vertex (BSDF sampling, roulette) on thinned generations"""
    SW._compare(hk, knobs, SW._box(hk, 37, 29, "light"), 16, 8)


def test_two_kinds_and_a_mix(hk, knobs):
    """a Mix of Matte and Mirror: the general bodies of two kinds, each continuing the other's queues"""
    from hikari_jl_amd import scenes

    def build():
        mix = hk.MixMaterial((hk.MatteMaterial(Kd=hk.RGBSpectrum(0.7, 0.3, 0.2)), hk.MirrorMaterial()), 0.4)
        return scenes.cornell_box(37, 29, objects="two_spheres", tess=8, object_material=mix)

    SW._compare(hk, knobs, build, 16, 3)


def _five(hk, knobs, s, size, kw, spp):
    out = []
    for switch in (None,) + SW.WAYS:
        for k, _ in SW.WAYS:
            knobs.delenv(k)
        out.append(LS._render(hk, knobs, s, LS.CORNELL_CAM, size, kw, spp, None if switch is None else {switch[0]: switch[1]}))
    for k, _ in SW.WAYS:
        knobs.delenv(k)
    for got, switch in zip(out[1:], SW.WAYS):
        assert np.array_equal(got[0].view(np.uint32), out[0][0].view(np.uint32)), "film differs under %s=%s" % switch
        assert got[1] == out[0][1], (got[1], out[0][1], switch)
    return out[0]


def test_matte_mix_matte_edit(hk, gpu_ctx, knobs):
    """The two-spheres box, every record Matte: five ways.  One record becomes a Mix of two Matte records (hk_scene_update_materials):
    five ways, and the film of the scene created with the Mix.  The edit back: five ways, and the first film again."""
    A = hk._abi
    L = hk._lib.lib()
    size, kw, spp = (48, 48), dict(max_depth=4, samples=8), 8
    s_mix, s_edit = LS._matte_mix_scene(hk), LS._matte_mix_scene(hk)
    d_mix, d_edit = s_mix.desc, s_edit.desc
    kinds = [d_mix.materials[i].kind for i in range(d_mix.n_materials)]
    mixes = [i for i, k in enumerate(kinds) if k == A.HK_MAT_MIX]
    assert len(mixes) == 1
    mix_rec = A.hk_material.from_buffer_copy(d_mix.materials[mixes[0]])
    plain = A.hk_material.from_buffer_copy(d_mix.materials[kinds.index(A.HK_MAT_MATTE)])
    d_edit.materials[mixes[0]] = plain                                   # before the device scene exists: created all Matte
    sh = hk.scene_handle(gpu_ctx, s_edit)
    try:
        created = _five(hk, knobs, s_edit, size, kw, spp)
        with_mix = _five(hk, knobs, s_mix, size, kw, spp)
        assert np.isfinite(with_mix[0]).all() and with_mix[0].max() > 0 and not np.array_equal(with_mix[0], created[0])
        hk._lib.check(L.hk_scene_update_materials(sh, mixes[0], 1, C.byref(mix_rec)), "hk_scene_update_materials")
        LS._same(_five(hk, knobs, s_edit, size, kw, spp), with_mix)
        hk._lib.check(L.hk_scene_update_materials(sh, mixes[0], 1, C.byref(plain)), "hk_scene_update_materials")
        LS._same(_five(hk, knobs, s_edit, size, kw, spp), created)
    finally:
        for k in LS.KNOBS:
            knobs.delenv(k, raising=False)
