"""hk_film_update_aux / hk_film_read_aux / hk_film_present / hk_film_present_async: the display chain kept on the device.

The yardstick is the host chain of the same library — hk_film_read_rgb -> hk_film_fill_aux -> hk_denoise -> hk_postprocess, pinned
to the oracle by test_gpu_denoise_matches_oracle, test_postprocess_parity and test_aux_buffers_parity.  Both chains instantiate the same
per-pixel functions (hk_display.h: finalize_pixel, first_hit_guides, variance_pixel, atrous_pixel, postprocess_pixel) over two pixel
layouts — k_finalize / k_aux / k_variance / k_atrous / k_postprocess<PlanarPixels> for the host chain, <PackedPixels> for the device
chain — so the frames are compared as uint32 views: equal, not close (NaN-free and NaN-kept pixels both count).  What is left to differ is the
layouts' loads and stores, the luminance kept in the packed record, and the postprocess fused into the last packed pass."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RENDER = dict(max_depth=3, samples=8)
DENOISE = ((0, True), (1, True), (2, False), (5, True))     # (iterations, use_variance)


def _pf(a):
    import hikari_jl_amd as hk
    return a.ctypes.data_as(hk._abi.PF)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dn(hk, iterations, use_variance):
    return hk.DenoiseConfig(iterations=iterations, use_variance=use_variance).record()


def _pps(hk):
    """ACES + gamma 2.2 + background mask, Reinhard without gamma, NULL"""
    from hikari_jl_amd.postprocess import make_params
    return (make_params(exposure=1.3, tonemap="aces", gamma=2.2, background=(0.1, 0.2, 0.3)), make_params(tonemap="reinhard", gamma=None), None)


class Chain:
    """One rendered film and both chains on it, through the C ABI"""

    def __init__(self, hk, ctx, scene, film, cam, **vp_kw):
        self.hk, self.ctx, self.L = hk, ctx, hk._lib.lib()
        self.scene, self.film, self.cam = scene, film, cam
        self.w, self.h = film.width, film.height
        self.vp = hk.VolPath(**dict(RENDER, **vp_kw))
        self.vp._ensure(film)
        self.vp.clear()
        self.sh = hk.scene_handle(ctx, scene)
        self.fh = self.vp._film[0]
        self.camrec = cam.record()

    def render(self, n, first):
        self.vp.render_samples(self.scene, self.film, self.cam, n, first=first, readback=False)

    def close(self):
        self.vp.close()

    def ok(self, status, what):
        assert status == 0, (what, status, self.L.hk_last_error())

    # -- the host chain --
    def read_rgb(self):
        out = np.empty((self.w, self.h, 3), np.float32)
        self.ok(self.L.hk_film_read_rgb(self.ctx.h, self.fh, _pf(out)), "hk_film_read_rgb")
        return out

    def fill_aux(self, inf):
        a, n, d = np.empty((self.w, self.h, 3), np.float32), np.empty((self.w, self.h, 3), np.float32), np.empty((self.w, self.h), np.float32)
        self.ok(self.L.hk_film_fill_aux(self.ctx.h, self.sh, C.byref(self.camrec), self.w, self.h, inf, _pf(a), _pf(n), _pf(d)), "hk_film_fill_aux")
        return a, n, d

    def host(self, rgb, aux, dn, pp):
        _, n, d = aux
        frame = rgb
        if dn is not None:
            frame = np.empty_like(rgb)
            self.ok(self.L.hk_denoise(self.ctx.h, C.byref(dn), self.w, self.h, _pf(rgb), _pf(n), _pf(d), _pf(frame), None), "hk_denoise")
        if pp is None:
            return frame
        out = np.empty_like(rgb)
        self.ok(self.L.hk_postprocess(self.ctx.h, C.byref(pp), self.w, self.h, _pf(frame), _pf(d), _pf(out)), "hk_postprocess")
        return out

    # -- the device chain --
    def update_aux(self, inf):
        self.ok(self.L.hk_film_update_aux(self.ctx.h, self.fh, self.sh, C.byref(self.camrec), inf), "hk_film_update_aux")

    def read_aux(self):
        a, n, d = np.empty((self.w, self.h, 3), np.float32), np.empty((self.w, self.h, 3), np.float32), np.empty((self.w, self.h), np.float32)
        self.ok(self.L.hk_film_read_aux(self.ctx.h, self.fh, _pf(a), _pf(n), _pf(d)), "hk_film_read_aux")
        return a, n, d

    def present(self, dn, pp):
        out = np.full((self.w, self.h, 3), -1.0, np.float32)
        self.ok(self.L.hk_film_present(self.ctx.h, self.fh, C.byref(dn) if dn is not None else None, C.byref(pp) if pp is not None else None, _pf(out)), "hk_film_present")
        return out

    def present_async(self, dn, pp):
        self.ok(self.L.hk_film_present_async(self.ctx.h, self.fh, C.byref(dn) if dn is not None else None, C.byref(pp) if pp is not None else None), "hk_film_present_async")

    def wait(self):
        out = np.full((self.w, self.h, 3), -1.0, np.float32)
        self.ok(self.L.hk_film_read_wait(self.ctx.h, self.fh, _pf(out), None), "hk_film_read_wait")
        return out

    def accum(self):
        return self.vp.read_accumulators(self.film).copy()


def _scene(name, w, h):
    from hikari_jl_amd import scenes
    return scenes.cornell_box(w, h, light="area") if name == "cornell" else scenes.single_triangle(w, h)


def _compare_all(hk, ch, denoise_cases=DENOISE):
    """every (has_infinite_lights, denoise, postprocess) combination: device chain == host chain, bit for bit; -> what was seen"""
    rgb = ch.read_rgb()
    assert np.array_equal(_bits(ch.present(None, None)), _bits(rgb))
    seen = dict(inf_depth=False, changed=False, masked=False, kept=False)
    for inf in (0, 1):
        aux = ch.fill_aux(inf)
        ch.update_aux(inf)
        got_aux = ch.read_aux()
        for g, want in zip(got_aux, aux):
            assert np.array_equal(_bits(g), _bits(want))
        seen["inf_depth"] |= bool(np.isinf(aux[2]).any())
        for pp in _pps(hk):
            assert np.array_equal(_bits(ch.present(None, pp)), _bits(ch.host(rgb, aux, None, pp)))
        for iterations, use_variance in denoise_cases:
            dn = _dn(hk, iterations, use_variance)
            for pp in _pps(hk):
                want, got = ch.host(rgb, aux, dn, pp), ch.present(dn, pp)
                diff = _bits(got) != _bits(want)
                assert not diff.any(), (ch.w, ch.h, inf, iterations, use_variance, None if pp is None else pp.tonemap, int(diff.sum()), np.argwhere(diff)[:4].tolist())
                if pp is None and iterations > 0:
                    seen["changed"] |= not np.array_equal(want, rgb)
                    # a pixel whose depth is +Inf has NaN weights against its +Inf neighbours and is kept as it was
                    esc = np.isinf(aux[2])
                    seen["kept"] |= bool(esc.any() and np.array_equal(want[esc], rgb[esc]))
                if pp is not None and pp.mask_escaped:
                    no_mask = hk._abi.hk_postprocess_params.from_buffer_copy(pp)
                    no_mask.mask_escaped = 0
                    seen["masked"] |= not np.array_equal(want, ch.host(rgb, aux, dn, no_mask))
    return seen


@pytest.mark.parametrize("scene_name", ["cornell", "triangle"])
@pytest.mark.parametrize("w,h", [(37, 29), (96, 64)])
def test_present_equals_the_host_chain_bit_for_bit(hk, gpu_ctx, scene_name, w, h):
    """37 x 29: both sides under 33, so the step-16 taps clamp on both edges in both directions, and no tile divides them;
    96 x 64: interior tiles without clamping and several workgroups per column.  The Cornell box is closed (every depth finite);
    most pixels of the single triangle escape: +Inf depth, the NaN-weight branch that keeps the pixel, a non-trivial escaped mask."""
    s, film, cam = _scene(scene_name, w, h)
    ch = Chain(hk, gpu_ctx, s, film, cam)
    try:
        ch.render(RENDER["samples"], 1)
        seen = _compare_all(hk, ch)
    finally:
        ch.close()
    assert seen["changed"]
    if scene_name == "triangle":
        assert seen["inf_depth"] and seen["masked"] and seen["kept"]


def test_present_is_non_destructive(hk, gpu_ctx):
    s, film, cam = _scene("cornell", 37, 29)
    dn, pp = _dn(hk, 5, True), _pps(hk)[0]

    def run(with_present):
        ch = Chain(hk, gpu_ctx, s, film, cam)
        try:
            ch.render(8, 1)
            ch.update_aux(0)
            before = ch.accum()
            aux = ch.read_aux()
            if with_present:
                ch.present(dn, pp)
                assert np.array_equal(_bits(ch.accum()), _bits(before))
                for g, want in zip(ch.read_aux(), aux):
                    assert np.array_equal(_bits(g), _bits(want))
            ch.render(4, 9)
            return ch.accum()
        finally:
            ch.close()

    assert np.array_equal(_bits(run(True)), _bits(run(False)))


def test_present_of_an_f64_film(hk, gpu_ctx):
    s, film, cam = _scene("cornell", 37, 29)
    ch = Chain(hk, gpu_ctx, s, film, cam, accumulation_eltype="Float64")
    try:
        ch.render(8, 1)
        assert ch.accum().dtype == np.float64
        _compare_all(hk, ch, denoise_cases=((5, True),))
    finally:
        ch.close()


def test_present_async_is_collected_by_read_wait(hk, gpu_ctx):
    s, film, cam = _scene("cornell", 37, 29)
    dn, pp = _dn(hk, 5, True), _pps(hk)[0]
    ch = Chain(hk, gpu_ctx, s, film, cam)
    try:
        ch.render(4, 1)
        ch.update_aux(0)
        aux = ch.read_aux()
        earlier = ch.present(dn, pp)
        ch.present_async(dn, pp)
        ch.render(4, 5)
        assert np.array_equal(_bits(ch.wait()), _bits(earlier))
        later = ch.present(dn, pp)
        assert not np.array_equal(later, earlier)
        assert np.array_equal(_bits(later), _bits(ch.host(ch.read_rgb(), aux, dn, pp)))
    finally:
        ch.close()


def test_aux_buffers_live_until_the_next_update(hk, gpu_ctx):
    """After the Cornell sphere has moved, a present still filters with the guides of the last update; the next update brings the new ones"""
    from hikari_jl_amd import geometry as G
    from hikari_jl_amd.scene import SceneInstance
    s, film, cam = _scene("cornell", 48, 40)
    first = 5 * G.rect3f((0, 0, 0), (1, 1, 1)).n_faces        # the five walls come first
    sphere = SceneInstance(5, first, G.sphere((-0.4, 0.4, 0.0), 0.35, 32).n_faces)
    dn, pp = _dn(hk, 5, True), _pps(hk)[0]
    ch = Chain(hk, gpu_ctx, s, film, cam)
    try:
        ch.render(8, 1)
        ch.update_aux(0)
        old = ch.fill_aux(0)
        rgb = ch.read_rgb()
        move = np.eye(4, dtype=np.float32)
        move[:3, 3] = (0.5, 0.4, -0.2)
        s.set_transform(sphere, move)
        assert np.array_equal(_bits(ch.present(dn, pp)), _bits(ch.host(rgb, old, dn, pp)))
        for g, want in zip(ch.read_aux(), old):
            assert np.array_equal(_bits(g), _bits(want))
        new = ch.fill_aux(0)
        assert not np.array_equal(new[2], old[2])               # the depth changes where the sphere was and where it is
        ch.update_aux(0)
        got = ch.present(dn, pp)
        assert np.array_equal(_bits(got), _bits(ch.host(rgb, new, dn, pp)))
        assert not np.array_equal(got, ch.host(rgb, old, dn, pp))
    finally:
        s.set_transform(sphere, np.eye(4, dtype=np.float32))
        ch.close()


def test_present_refuses_misuse(hk, gpu_ctx):
    A, L = hk._abi, hk._lib.lib()
    s, film, cam = _scene("cornell", 16, 12)
    ch = Chain(hk, gpu_ctx, s, film, cam)
    other = hk.Context(0)
    try:
        ch.render(2, 1)
        fh, ctx = ch.fh, gpu_ctx.h
        out = np.empty((16, 12, 3), np.float32)
        dn, pp = _dn(hk, 2, True), _pps(hk)[1]
        mask = _pps(hk)[0]
        camrec = ch.camrec

        def refused(status):
            return status == A.HK_ERR_INVALID and len(L.hk_last_error()) > 0

        # before any hk_film_update_aux
        assert refused(L.hk_film_read_aux(ctx, fh, _pf(out), None, None))
        assert refused(L.hk_film_present(ctx, fh, C.byref(dn), None, _pf(out)))
        assert refused(L.hk_film_present(ctx, fh, None, C.byref(mask), _pf(out)))
        assert refused(L.hk_film_present_async(ctx, fh, C.byref(dn), None))
        assert refused(L.hk_film_present_async(ctx, fh, None, C.byref(mask)))
        assert L.hk_film_present(ctx, fh, None, C.byref(pp), _pf(out)) == 0          # (no guides needed)
        # null handles, a film of another context, no destination
        assert refused(L.hk_film_update_aux(None, fh, ch.sh, C.byref(camrec), 0)) and refused(L.hk_film_update_aux(ctx, None, ch.sh, C.byref(camrec), 0))
        assert refused(L.hk_film_update_aux(other.h, fh, ch.sh, C.byref(camrec), 0))
        assert refused(L.hk_film_read_aux(None, fh, None, None, None)) and refused(L.hk_film_read_aux(ctx, None, None, None, None))
        assert refused(L.hk_film_present(None, fh, None, None, _pf(out))) and refused(L.hk_film_present(ctx, None, None, None, _pf(out)))
        assert refused(L.hk_film_present_async(None, fh, None, None)) and refused(L.hk_film_present_async(ctx, None, None, None))
        assert refused(L.hk_film_present(other.h, fh, None, None, _pf(out))) and refused(L.hk_film_present_async(other.h, fh, None, None))
        assert refused(L.hk_film_read_aux(other.h, fh, None, None, None))
        assert refused(L.hk_film_present(ctx, fh, None, None, None))
        ch.update_aux(0)
        for bad in (-1, 31):
            p = _dn(hk, bad, True)
            assert refused(L.hk_film_present(ctx, fh, C.byref(p), None, _pf(out))) and refused(L.hk_film_present_async(ctx, fh, C.byref(p), None))
        for bad in (-1, 6):
            p = A.hk_postprocess_params.from_buffer_copy(pp)
            p.tonemap = bad
            assert refused(L.hk_film_present(ctx, fh, None, C.byref(p), _pf(out))) and refused(L.hk_film_present_async(ctx, fh, None, C.byref(p)))
        # a correct call on the same film still succeeds, and nothing of the refused ones was enqueued
        aux, rgb = ch.read_aux(), ch.read_rgb()
        assert np.array_equal(_bits(ch.present(dn, mask)), _bits(ch.host(rgb, aux, dn, mask)))
    finally:
        ch.close()
        L.hk_ctx_destroy(other.h)


def test_python_surface(hk, gpu_ctx):
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cornell_box(48, 40, light="area")
    vp = hk.VolPath(max_depth=3, samples=4)
    try:
        vp(s, film, cam)
        vp.update_aux(s, film, cam, host_copy=True)
        got = vp.present(film, denoise=True, tonemap="aces").copy()
        assert got is not film.framebuffer and got.shape == (40, 48, 3)
        linear = vp.present(film).copy()
        assert np.array_equal(_bits(linear), _bits(film.framebuffer))
        host = hk.Film((48, 40))
        host.framebuffer = film.framebuffer.copy()
        host.fill_aux_buffers(s, cam)
        for a, b in ((host.albedo, film.albedo), (host.normal, film.normal), (host.depth, film.depth)):
            assert np.array_equal(_bits(a), _bits(b))
        host.framebuffer = host.denoise().copy()
        want = host.postprocess(tonemap="aces")
        assert np.array_equal(_bits(got), _bits(want))
        # a pipelined loop: each call hands out the frame of the call before; the final wait brings the last one
        frames = []
        for _ in range(4):
            vp.render_samples(s, film, cam, 1, readback=False)
            vp.present(film, denoise=True, pipelined=True, tonemap="aces")
            frames.append(film.postprocess_buffer.copy())
        last = vp.finish_present(film).copy()
        assert np.array_equal(_bits(last), _bits(vp.present(film, denoise=True, tonemap="aces")))
        assert not np.array_equal(last, frames[-1]) and not np.array_equal(frames[-1], frames[-2])
    finally:
        vp.close()


def test_python_pipelined_reads_of_both_kinds_share_the_staging_buffers(hk, gpu_ctx):
    """One read in flight per film: a pending presented frame collected by render_samples(readback="pipelined") goes to
    film.postprocess_buffer, not to film.framebuffer, and the other way round; a synchronous present in between clears the slot."""
    from hikari_jl_amd import scenes
    s, film, cam = scenes.cornell_box(48, 40, light="area")
    vp = hk.VolPath(max_depth=3, samples=2)
    try:
        vp(s, film, cam)
        vp.update_aux(s, film, cam)
        shown = vp.present(film, denoise=True, tonemap="aces").copy()
        raw = film.framebuffer.copy()
        film.postprocess_buffer = np.zeros_like(shown)
        vp.present(film, denoise=True, pipelined=True, tonemap="aces")          # in flight
        vp.render_samples(s, film, cam, 1, readback="pipelined")                # collects it, enqueues a raw frame
        assert np.array_equal(_bits(film.postprocess_buffer), _bits(shown)) and np.array_equal(_bits(film.framebuffer), _bits(raw))
        later = vp.present(film, denoise=True, pipelined=True, tonemap="aces")  # collects the raw frame of 3 samples
        assert np.array_equal(_bits(later), _bits(shown)) and not np.array_equal(film.framebuffer, raw)
        raw3 = film.framebuffer.copy()
        vp.present(film)                                                        # synchronous: overtakes the one in flight
        assert vp._read_pending is False
        vp.finish_pipelined(film)                                               # nothing left to collect
        assert np.array_equal(_bits(film.postprocess_buffer), _bits(raw3))
    finally:
        vp.close()
