"""k_film's grouped fold (hk_film_kernels.h: film_tile<ACC, G>).  For a pass of S = 64 k samples per pixel a wave converts the 64-sample
steps of G consecutive pixels of its tile, and 4 G lanes — one per pixel and channel — add their pixel's 64 entries from LDS in sample
order; before, four lanes added one pixel's entries while sixty waited.  Per pixel and channel the additions and their order are the
same, so the film is the same bit for bit: every case renders under the default and under HK_FILM_FOLD=0 (the one-pixel fold) and
compares the accumulators as uint32.

S = 64, 128, 256 take the grouped arm; S = 32 (whole pixels per step) and S = 48 (one lane per pixel) take the arms it leaves alone.
37 x 29 pads to 40 x 32 (padding pixels inside the groups), 64 x 48 has none.  Each case renders one view three times on one
integrator: a frame, the same frame again on a fresh film (with the view cache it keeps the camera records, and its L is what k_film's
zero stores left), and a second pass of other samples added to that film (accumulators that start from values)."""
import numpy as np
import pytest

import test_shade_slot_walk as SW

pytestmark = pytest.mark.gpu

DEPTH = 3


def _frames(hk, knobs, size, spp, fold, f64, cache):
    knobs.setenv("HK_BATCH_PATHS_M", "0")
    knobs.setenv("HK_SMALL_PASS_FUSED", "0")
    knobs.setenv("HK_DYNAMIC_SEGMENTS", "1")
    if fold:
        knobs.delenv("HK_FILM_FOLD")
    else:
        knobs.setenv("HK_FILM_FOLD", "0")
    if cache:
        knobs.delenv("HK_VIEW_CACHE")
    else:
        knobs.setenv("HK_VIEW_CACHE", "0")
    scene, _, _ = SW._box(hk, size[0], size[1], "light")()
    vp = hk.VolPath(max_depth=DEPTH, samples=2 * spp, accumulation_eltype="Float64" if f64 else "Float32")
    cam = lambda film: hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0)
    out = []
    try:
        hits = 0
        for i in range(2):
            film = hk.Film(size)
            vp._ensure(film)
            vp.clear()
            vp.reset_stats()
            vp.render_samples(scene, film, cam(film), spp, readback=False)
            st = vp.stats()                                     # (of this frame: the counters were reset before it)
            assert int(st.shade_launches) == DEPTH              # one pass: S is spp
            hits += int(st.view_cache_hits)
            out.append(vp.read_accumulators(film).copy())
        vp.render_samples(scene, film, cam(film), spp, first=1 + spp, readback=False)      # added to the second frame's film
        out.append(vp.read_accumulators(film).copy())
        return out, hits
    finally:
        vp.close()


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("spp", [32, 48, 64, 128, 256])
@pytest.mark.parametrize("size", [(37, 29), (64, 48)])
def test_fold_bit_for_bit(hk, knobs, size, spp, f64, cache):
    on, hits_on = _frames(hk, knobs, size, spp, True, f64, cache)
    off, hits_off = _frames(hk, knobs, size, spp, False, f64, cache)
    assert hits_on == hits_off == (1 if cache else 0), (hits_on, hits_off)
    assert on[0].dtype == (np.float64 if f64 else np.float32)
    for i, (a, b) in enumerate(zip(on, off)):
        assert np.isfinite(b).all() and b.max() > 0, i
        assert np.array_equal(_bits(a), _bits(b)), "frame %d: film differs from HK_FILM_FOLD=0" % i
    assert np.array_equal(_bits(on[0]), _bits(on[1]))      # the kept camera records and the zeroed L give the first frame again
    assert not np.array_equal(on[1], on[2])
