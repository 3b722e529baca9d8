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
// K13 + the device-to-host copy of the frame.  A pageable destination made this the most expensive part of an interactive viewer's loop
// (round 4: 3.7 ms of a 5.3-ms one-sample call at 800^2 — the runtime stages a pageable copy through small pinned buffers and the
// stream waits for each).  Now the frame lands in PINNED memory: the film's own staging buffers (two, in turn), or the caller's
// buffer itself once the same pointer has come twice in a row and hipHostRegister accepted it (a viewer reads into ONE framebuffer).
static int enqueue_frame_read(hk_ctx* c, hk_film* f, float* direct) {
    const size_t bytes = (size_t)3 * f->width * f->height * 4;
    if (int e = join_lanes(c)) return e;
    if (f->readback.bytes != bytes) HIP_TRY(f->readback.alloc(bytes));
    if (!f->ev_read) HIP_TRY(hipEventCreateWithFlags(&f->ev_read, hipEventDisableTiming));
    float* dst = direct;
    if (!dst) {
        const int k = f->staging_next;
        if (!f->staging[k]) HIP_TRY(hipHostMalloc((void**)&f->staging[k], bytes, hipHostMallocDefault));
        dst = f->staging[k];
        f->staging_last = k;
        f->staging_next = k ^ 1;
    }
    hk::launch_finalize(c->stream, f->accum, f->f64, f->readback.as<float>(), f->width, f->height);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, f->readback.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(f->ev_read, c->stream));
    return HK_OK;
}
extern "C" int32_t hk_film_read_rgb(hk_ctx* c, hk_film* f, float* out) {
    if (!c || !f || !out) return fail(HK_ERR_INVALID, "null argument");
    if (f->ctx != c) return fail(HK_ERR_INVALID, "film belongs to another context");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    const size_t bytes = (size_t)3 * f->width * f->height * 4;
    if (f->read_in_flight) {   // an asynchronous read nobody waited for: its staging buffer is simply overtaken
        HIP_TRY(hipEventSynchronize(f->ev_read));
        f->read_in_flight = false;
    }
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
    const bool direct = f->pinned_user == out;
    if (int e = enqueue_frame_read(c, f, direct ? out : nullptr)) return e;
    HIP_TRY(hipEventSynchronize(f->ev_read));
    if (!direct) std::memcpy(out, f->staging[f->staging_last], bytes);
    return HK_OK;
}
extern "C" int32_t hk_film_pin_host(hk_film* f, float* host_hw3) {
    if (!f || !host_hw3) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->read_in_flight) {
        HIP_TRY(hipEventSynchronize(f->ev_read));
        f->read_in_flight = false;
    }
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
    if (f->read_in_flight) {
        HIP_TRY(hipEventSynchronize(f->ev_read));
        f->read_in_flight = false;
    }
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
    if (int e = enqueue_frame_read(c, f, nullptr)) return e;
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
int run_postprocess(hk_ctx* c, const hk_postprocess_params* P, int w, int h, const float* src_dev, const float* depth_host, float* dst_host, DevBuf& out) {
    const size_t bytes = (size_t)3 * w * h * 4;
    HIP_TRY(out.alloc(bytes));
    DevBuf dd;
    if (depth_host && P->mask_escaped) HIP_TRY(dd.upload(depth_host, (size_t)w * h * 4));
    hk::launch_postprocess(c->stream, *P, src_dev, dd.as<float>(), out.as<float>(), h, w);
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
    hk::launch_finalize(c->stream, f->accum, f->f64, f->readback.as<float>(), f->width, f->height);
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
    if (P->use_variance) hk::launch_denoise_variance(c->stream, a.as<float>(), var.as<float>(), h, w);
    for (int i = 1; i <= P->iterations; ++i) {   // odd passes a -> b, even passes b -> a (denoise.jl:337-361)
        const float* in = (i & 1) ? a.as<float>() : b.as<float>();
        float* out = (i & 1) ? b.as<float>() : a.as<float>();
        hk::launch_denoise_atrous(c->stream, *P, 1 << (i - 1), in, nn.as<float>(), dd.as<float>(), var.as<float>(), out, h, w);
    }
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
    hk::launch_aux(c->stream, sc->d, make_camera(*cam), h, w, has_infinite_lights ? 1e30f : INFINITY, da.as<float>(), dn.as<float>(), dd.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(albedo, da.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(normal, dn.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(depth, dd.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HK_OK;
}
