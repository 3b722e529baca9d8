// hk_film.cpp — the film of the C-ABI: accumulators, read-back through pinned memory, post-processing, denoising and the auxiliary
// buffers (albedo / normal / depth).
#include "hk_host.h"

extern "C" int32_t hk_film_create(hk_ctx* c, int32_t w, int32_t h, int32_t f64, void* external, hk_film** out) {
    if (!c || !out || w < 1 || h < 1) return fail(HK_ERR_INVALID, "bad film arguments");
    HIP_TRY(hipSetDevice(c->device));
    hk_film* f = new hk_film();
    f->ctx = c;
    f->width = w;
    f->height = h;
    f->f64 = f64 != 0;
    size_t bytes = (size_t)4 * w * h * (f64 ? 8 : 4);
    f->external = external != nullptr;
    if (external)
        f->accum = external;
    else {
        HIP_TRY(f->own.alloc(bytes));
        f->accum = f->own.p;
        HIP_TRY(hipMemsetAsync(f->accum, 0, bytes, c->stream));
    }
    *out = f;
    return HK_OK;
}
extern "C" int32_t hk_film_destroy(hk_film* f) {
    int status = HK_OK;   // the object goes either way; a device error of a pass that was still noted / in flight is reported (hk_last_error)
    if (f) {
        (void)hipSetDevice(f->ctx->device);
        status = join_lanes(f->ctx);
        if (hipStreamSynchronize(f->ctx->stream) != hipSuccess && status == HK_OK) status = fail(HK_ERR_DEVICE, "hk_film_destroy: the context's stream reports an error");
        if (f->pinned_user) (void)hipHostUnregister(f->pinned_user);
        for (auto& st : f->staging)
            if (st) (void)hipHostFree(st);
        if (f->ev_read) (void)hipEventDestroy(f->ev_read);
        delete f;
    }
    return status;
}
extern "C" int32_t hk_film_clear(hk_film* f) {
    if (!f) return fail(HK_ERR_INVALID, "null film");
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (int e = join_lanes(f->ctx)) return e;
    HIP_TRY(hipMemsetAsync(f->accum, 0, (size_t)4 * f->width * f->height * (f->f64 ? 8 : 4), f->ctx->stream));
    return HK_OK;
}
extern "C" void* hk_film_accum_device_ptr(hk_film* f) {
    if (f) {
        (void)flush_pending(f->ctx);   // (whoever asks for the pointer is about to look: the noted calls are enqueued first)
        f->exposed = true;             // ... and may keep it: from now on calls into this film are enqueued at once (hk_render: ORDERING CONTRACT)
    }
    return f ? f->accum : nullptr;
}
extern "C" int32_t hk_film_read_accum(hk_ctx* c, hk_film* f, void* out) {
    if (!c || !f || !out) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipMemcpyAsync(out, f->accum, (size_t)4 * f->width * f->height * (f->f64 ? 8 : 4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HK_OK;
}
// hk_film_present's chain (the entry points and what they promise: the end of this file): K13 -> variance -> a-trous passes -> postprocess
// into `readback`, on packed buffers of the film.
namespace {
struct PresentJob {   // hk_film_present: what fills `readback` in place of the plain K13 (checked by check_present)
    const hk_denoise_params* dn;
    const hk_postprocess_params* pp;
};
// the refusals of both forms; nothing is enqueued before every one of them has passed
int check_present(hk_ctx* c, hk_film* f, const hk_denoise_params* dn, const hk_postprocess_params* pp) {
    if (!c || !f) return fail(HK_ERR_INVALID, "hk_film_present: null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "hk_film_present: film belongs to another context");
    if (dn && (dn->iterations < 0 || dn->iterations > 30)) return fail(HK_ERR_INVALID, "hk_film_present: iterations out of range");
    if (pp && (pp->tonemap < HK_TONEMAP_NONE || pp->tonemap > HK_TONEMAP_FILMIC)) return fail(HK_ERR_INVALID, "hk_film_present: unknown tonemap");
    if (dn && !f->have_aux) return fail(HK_ERR_INVALID, "hk_film_present: denoising needs hk_film_update_aux first");
    if (pp && pp->mask_escaped && !f->have_aux) return fail(HK_ERR_INVALID, "hk_film_present: the escaped mask needs hk_film_update_aux first");
    return HK_OK;
}
int enqueue_present_chain(hk_ctx* c, hk_film* f, const PresentJob& job) {
    const int w = f->width, h = f->height;
    const size_t n = (size_t)w * h;
    const int iterations = job.dn ? job.dn->iterations : 0;
    float* out = f->readback.as<float>();
    if (iterations == 0 && !job.pp) {   // linear and unfiltered: hk_film_read_rgb's frame
        hk::launch_finalize(c->stream, f->accum, f->f64, PlanarPixels{out, nullptr, nullptr}, w, h);
        return HK_OK;
    }
    if (f->frame[0].bytes != n * 16) HIP_TRY(f->frame[0].alloc(n * 16));
    if (iterations > 0 && f->frame[1].bytes != n * 16) HIP_TRY(f->frame[1].alloc(n * 16));
    if (iterations > 0 && f->variance.bytes != n * 4) HIP_TRY(f->variance.alloc(n * 4));
    float4* guides = f->have_aux ? f->guides.as<float4>() : nullptr;
    const PackedPixels px[2] = {{f->frame[0].as<float4>(), guides}, {f->frame[1].as<float4>(), guides}};
    hk::launch_finalize(c->stream, f->accum, f->f64, px[0], w, h);
    if (iterations == 0) {
        hk::launch_postprocess(c->stream, *job.pp, px[0], out, h, w);
        return HK_OK;
    }
    if (job.dn->use_variance) hk::launch_variance(c->stream, px[0], f->variance.as<float>(), h, w);
    for (int i = 1; i <= iterations; ++i)   // odd passes ping -> pong, even passes back (hk_denoise); the last one writes the output frame
        hk::launch_atrous(c->stream, *job.dn, 1 << (i - 1), px[(i & 1) ^ 1], f->variance.as<float>(), px[i & 1], i == iterations ? out : nullptr, job.pp, h, w);
    return HK_OK;
}
}  // namespace
// K13 + the device-to-host copy of the frame.  A pageable destination made this the most expensive part of an interactive viewer's loop
// (round 4: 3.7 ms of a 5.3-ms one-sample call at 800^2 — the runtime stages a pageable copy through small pinned buffers and the
// stream waits for each).  Now the frame lands in PINNED memory: the film's own staging buffers (two, in turn), or the caller's
// buffer itself once the same pointer has come twice in a row and hipHostRegister accepted it (a viewer reads into ONE framebuffer).
static int enqueue_frame_read(hk_ctx* c, hk_film* f, float* direct, const PresentJob* job) {   // job == nullptr: the plain frame
    const size_t bytes = (size_t)3 * f->width * f->height * 4;
    if (int e = join_lanes(c)) return e;
    if (f->readback.bytes != bytes) HIP_TRY(f->readback.alloc(bytes));
    if (!f->ev_read) HIP_TRY(hipEventCreateWithFlags(&f->ev_read, hipEventDisableTiming));
    if (job) {
        if (int e = enqueue_present_chain(c, f, *job)) return e;
    } else
        hk::launch_finalize(c->stream, f->accum, f->f64, PlanarPixels{f->readback.as<float>(), nullptr, nullptr}, f->width, f->height);
    HIP_TRY(hipGetLastError());
    float* dst = direct;
    if (!dst) {
        const int k = f->staging_next;
        if (!f->staging[k]) HIP_TRY(hipHostMalloc((void**)&f->staging[k], bytes, hipHostMallocDefault));
        dst = f->staging[k];
        f->staging_last = k;
        f->staging_next = k ^ 1;
    }
    HIP_TRY(hipMemcpyAsync(dst, f->readback.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(f->ev_read, c->stream));
    return HK_OK;
}
// an asynchronous read nobody waited for: its staging buffer is simply overtaken
static int settle_pending_read(hk_film* f) {
    if (f->read_in_flight) {
        HIP_TRY(hipEventSynchronize(f->ev_read));
        f->read_in_flight = false;
    }
    return HK_OK;
}
// the frame (job: hk_film_present's, else the plain K13) into `out`, now: straight into it when it is the film's registered host buffer, else through staging
static int read_frame_now(hk_ctx* c, hk_film* f, float* out, const PresentJob* job) {
    const bool direct = f->pinned_user == out;
    if (int e = enqueue_frame_read(c, f, direct ? out : nullptr, job)) return e;
    HIP_TRY(hipEventSynchronize(f->ev_read));
    if (!direct) std::memcpy(out, f->staging[f->staging_last], (size_t)3 * f->width * f->height * 4);
    return HK_OK;
}
extern "C" int32_t hk_film_read_rgb(hk_ctx* c, hk_film* f, float* out) {
    if (!c || !f || !out) return fail(HK_ERR_INVALID, "null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "film belongs to another context");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    const size_t bytes = (size_t)3 * f->width * f->height * 4;
    if (int e = settle_pending_read(f)) return e;
    // Caller memory is registered with the driver only on request (the library cannot know when a buffer it registered by
    // itself is freed — a C host that mallocs a frame buffer per frame gets the same address back, and the copy would go through a
    // stale registration): hk_film_pin_host names the buffer, or HK_READBACK_PIN=1 brings back "the same pointer twice in a row".
    // A registration that failed is remembered for that pointer and not tried again on every frame.
    const bool pin = hk::knob_int("HK_READBACK_PIN", 0) == 1;
    if (!f->pinned_explicit) {
        if (pin && f->pinned_user != out && f->last_out == out && f->pin_failed != out) {
            if (f->pinned_user) (void)hipHostUnregister(f->pinned_user);
            f->pinned_user = hipHostRegister(out, bytes, hipHostRegisterDefault) == hipSuccess ? out : nullptr;
            if (!f->pinned_user) f->pin_failed = out;
            (void)hipGetLastError();
        } else if (f->pinned_user && f->pinned_user != out) {
            (void)hipHostUnregister(f->pinned_user);
            f->pinned_user = nullptr;
        }
    }
    f->last_out = out;
    return read_frame_now(c, f, out, nullptr);
}
extern "C" int32_t hk_film_pin_host(hk_film* f, float* host_hw3) {
    if (!f || !host_hw3) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (int e = settle_pending_read(f)) return e;
    if (f->pinned_user == host_hw3 && f->pinned_explicit) return HK_OK;
    if (f->pinned_user) (void)hipHostUnregister(f->pinned_user);
    f->pinned_user = nullptr, f->pinned_explicit = false;
    if (hipHostRegister(host_hw3, (size_t)3 * f->width * f->height * 4, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HK_ERR_DEVICE, "hk_film_pin_host: hipHostRegister refused the buffer");
    }
    f->pinned_user = host_hw3, f->pinned_explicit = true;
    return HK_OK;
}
extern "C" int32_t hk_film_unpin_host(hk_film* f) {
    if (!f) return fail(HK_ERR_INVALID, "null film");
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (int e = settle_pending_read(f)) return e;
    if (f->pinned_user) (void)hipHostUnregister(f->pinned_user);
    f->pinned_user = nullptr, f->pinned_explicit = false, f->last_out = nullptr;
    return HK_OK;
}
extern "C" int32_t hk_film_read_rgb_async(hk_ctx* c, hk_film* f) {
    if (!c || !f) return fail(HK_ERR_INVALID, "null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "film belongs to another context");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (f->read_in_flight) HIP_TRY(hipEventSynchronize(f->ev_read));   // (two buffers: the one about to be refilled is the one BEFORE the last)
    if (int e = enqueue_frame_read(c, f, nullptr, nullptr)) return e;
    f->read_in_flight = true;
    return HK_OK;
}
extern "C" int32_t hk_film_read_wait(hk_ctx* c, hk_film* f, float* out, const float** frame) {
    if (!c || !f) return fail(HK_ERR_INVALID, "null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "film belongs to another context");
    if (f->staging_last < 0 || !f->ev_read) return fail(HK_ERR_INVALID, "hk_film_read_wait without hk_film_read_rgb_async");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(f->ev_read));
    f->read_in_flight = false;
    const float* src = f->staging[f->staging_last];
    if (out) std::memcpy(out, src, (size_t)3 * f->width * f->height * 4);
    if (frame) *frame = src;
    return HK_OK;
}

namespace {
int run_postprocess(hk_ctx* c, const hk_postprocess_params* P, int w, int h, float* src_dev, const float* depth_host, float* dst_host, DevBuf& out) {
    const size_t bytes = (size_t)3 * w * h * 4;
    HIP_TRY(out.alloc(bytes));
    DevBuf dd;
    if (depth_host && P->mask_escaped) HIP_TRY(dd.upload(depth_host, (size_t)w * h * 4));
    hk::launch_postprocess(c->stream, *P, PlanarPixels{src_dev, nullptr, dd.as<float>()}, out.as<float>(), h, w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst_host, out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HK_OK;
}
}  // namespace
extern "C" int32_t hk_film_postprocess(hk_ctx* c, hk_film* f, const hk_postprocess_params* P, const float* depth, float* dst) {
    if (!c || !f || !P || !dst) return fail(HK_ERR_INVALID, "null argument");
    if (P->tonemap < HK_TONEMAP_NONE || P->tonemap > HK_TONEMAP_FILMIC) return fail(HK_ERR_INVALID, "unknown tonemap");
    HIP_TRY(hipSetDevice(c->device));
    size_t bytes = (size_t)3 * f->width * f->height * 4;
    if (int e = join_lanes(c)) return e;
    if (f->readback.bytes != bytes) HIP_TRY(f->readback.alloc(bytes));
    hk::launch_finalize(c->stream, f->accum, f->f64, PlanarPixels{f->readback.as<float>(), nullptr, nullptr}, f->width, f->height);
    DevBuf out;
    return run_postprocess(c, P, f->width, f->height, f->readback.as<float>(), depth, dst, out);
}
extern "C" int32_t hk_postprocess(hk_ctx* c, const hk_postprocess_params* P, int32_t w, int32_t h, const float* src, const float* depth, float* dst) {
    if (!c || !P || !src || !dst || w <= 0 || h <= 0) return fail(HK_ERR_INVALID, "bad argument");
    if (P->tonemap < HK_TONEMAP_NONE || P->tonemap > HK_TONEMAP_FILMIC) return fail(HK_ERR_INVALID, "unknown tonemap");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf in, out;
    HIP_TRY(in.upload(src, (size_t)3 * w * h * 4));
    return run_postprocess(c, P, w, h, in.as<float>(), depth, dst, out);
}

extern "C" int32_t hk_denoise(hk_ctx* c, const hk_denoise_params* P, int32_t w, int32_t h, const float* src, const float* normal, const float* depth, float* dst,
                              float* src_after) {
    if (!c || !P || !src || !normal || !depth || !dst || w <= 0 || h <= 0) return fail(HK_ERR_INVALID, "bad argument");
    if (P->iterations < 0 || P->iterations > 30) return fail(HK_ERR_INVALID, "iterations out of range");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)w * h;
    DevBuf a, b, nn, dd, var;
    HIP_TRY(a.upload(src, npx * 12));
    HIP_TRY(b.alloc(npx * 12));
    HIP_TRY(nn.upload(normal, npx * 12));
    HIP_TRY(dd.upload(depth, npx * 4));
    HIP_TRY(var.alloc(npx * 4));
    const PlanarPixels px[2] = {{a.as<float>(), nn.as<float>(), dd.as<float>()}, {b.as<float>(), nn.as<float>(), dd.as<float>()}};
    if (P->use_variance) hk::launch_variance(c->stream, px[0], var.as<float>(), h, w);
    for (int i = 1; i <= P->iterations; ++i)   // odd passes a -> b, even passes b -> a (denoise.jl:337-361)
        hk::launch_atrous(c->stream, *P, 1 << (i - 1), px[(i & 1) ^ 1], var.as<float>(), px[i & 1], h, w);
    HIP_TRY(hipGetLastError());
    // film.postprocess <- the last written buffer; with iterations == 0 that is the untouched framebuffer (:365-371)
    HIP_TRY(hipMemcpyAsync(dst, (P->iterations & 1) ? b.p : a.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
    if (src_after) HIP_TRY(hipMemcpyAsync(src_after, a.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HK_OK;
}

extern "C" int32_t hk_film_fill_aux(hk_ctx* c, hk_scene* sc, const hk_camera* cam, int32_t w, int32_t h, int32_t has_infinite_lights, float* albedo, float* normal, float* depth) {
    if (!c || !sc || !cam || !albedo || !normal || !depth || w <= 0 || h <= 0) return fail(HK_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf da, dn, dd;
    const size_t n = (size_t)w * h;
    HIP_TRY(da.alloc(n * 12));
    HIP_TRY(dn.alloc(n * 12));
    HIP_TRY(dd.alloc(n * 4));
    hk::launch_aux(c->stream, sc->d, make_camera(*cam), h, w, has_infinite_lights ? 1e30f : INFINITY, da.as<float>(), PlanarPixels{nullptr, dn.as<float>(), dd.as<float>()});
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(albedo, da.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(normal, dn.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(depth, dd.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HK_OK;
}

// ---------------------------------------------------------------------------------------------------
// THE DISPLAY CHAIN ON THE DEVICE.  fill_aux_buffers!, denoise! and postprocess! of the reference work on the film's own device arrays
// (film.jl:410-483, denoise.jl:301-376, postprocess.jl:293-357); so do these: hk_film_update_aux keeps the guides in buffers of the
// film, hk_film_present runs K13 -> variance -> a-trous passes -> postprocess on packed buffers of the film and copies ONE frame to the
// host, through the pinned staging buffers of hk_film_read_rgb.  The arithmetic is that of hk_film_read_rgb -> hk_denoise ->
// hk_postprocess, bit for bit.
// ---------------------------------------------------------------------------------------------------
extern "C" int32_t hk_film_update_aux(hk_ctx* c, hk_film* f, hk_scene* sc, const hk_camera* cam, int32_t has_infinite_lights) {
    if (!c || !f || !sc || !cam) return fail(HK_ERR_INVALID, "hk_film_update_aux: null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "hk_film_update_aux: film belongs to another context");
    if (sc->ctx != c) return fail(HK_ERR_INVALID, "hk_film_update_aux: scene belongs to another context");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    const size_t n = (size_t)f->width * f->height;
    if (f->guides.bytes != n * 16) HIP_TRY(f->guides.alloc(n * 16));
    if (f->albedo.bytes != n * 12) HIP_TRY(f->albedo.alloc(n * 12));
    hk::launch_aux(c->stream, sc->d, make_camera(*cam), f->height, f->width, has_infinite_lights ? 1e30f : INFINITY, f->albedo.as<float>(), PackedPixels{nullptr, f->guides.as<float4>()});
    HIP_TRY(hipGetLastError());
    f->have_aux = true;
    return HK_OK;
}
extern "C" int32_t hk_film_read_aux(hk_ctx* c, hk_film* f, float* albedo, float* normal, float* depth) {
    if (!c || !f) return fail(HK_ERR_INVALID, "hk_film_read_aux: null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "hk_film_read_aux: film belongs to another context");
    if (!f->have_aux) return fail(HK_ERR_INVALID, "hk_film_read_aux before hk_film_update_aux");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;
    const size_t n = (size_t)f->width * f->height;
    std::vector<float> packed;
    if (normal || depth) {
        packed.resize(4 * n);
        HIP_TRY(hipMemcpyAsync(packed.data(), f->guides.p, n * 16, hipMemcpyDeviceToHost, c->stream));
    }
    if (albedo) HIP_TRY(hipMemcpyAsync(albedo, f->albedo.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n && (normal || depth); ++i) {
        if (normal) normal[3 * i] = packed[4 * i], normal[3 * i + 1] = packed[4 * i + 1], normal[3 * i + 2] = packed[4 * i + 2];
        if (depth) depth[i] = packed[4 * i + 3];
    }
    return HK_OK;
}
extern "C" int32_t hk_film_present(hk_ctx* c, hk_film* f, const hk_denoise_params* dn, const hk_postprocess_params* pp, float* out) {
    if (int e = check_present(c, f, dn, pp)) return e;
    if (!out) return fail(HK_ERR_INVALID, "hk_film_present: out_hw3 is null");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = settle_pending_read(f)) return e;
    const PresentJob job{dn, pp};
    return read_frame_now(c, f, out, &job);
}
extern "C" int32_t hk_film_present_async(hk_ctx* c, hk_film* f, const hk_denoise_params* dn, const hk_postprocess_params* pp) {
    if (int e = check_present(c, f, dn, pp)) return e;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (f->read_in_flight) HIP_TRY(hipEventSynchronize(f->ev_read));   // (two buffers: the one about to be refilled is the one BEFORE the last)
    const PresentJob job{dn, pp};
    if (int e = enqueue_frame_read(c, f, nullptr, &job)) return e;
    f->read_in_flight = true;
    return HK_OK;
}
