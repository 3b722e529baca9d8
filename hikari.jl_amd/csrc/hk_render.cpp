// hk_render.cpp — the integrator (filter tabulation, path state) and the wavefront driver that replaces the reference's host loop
// `render!` (src/integrators/volpath/volpath.jl:445-636).  Unlike the reference loop (8-10 blocking `length(queue)` readbacks per
// bounce, workqueue.jl:108-111) nothing here reads the device back inside a frame: queue sizes stay in HBM and every kernel sizes
// itself from them.  render_tile_now is a sequence of named steps: pass size, lane, path state, sampler tables, camera medium, then
// PassCtx::enqueue_pass per pass (enqueue_stages / enqueue_depth when the pass is not one fused launch).
#include "hk_host.h"

// ---- integrator: filter tabulation (GPUFilterSamplerData, filter.jl:636-725) -------------------------
namespace {
float gaussian_1d(float x, float sigma) { return std::exp(-(x * x) / (2.0f * (sigma * sigma))); }
float mitchell_1d(float x, float B, float C) {
    x = std::fabs(x);
    if (x <= 1.0f) return ((12.0f - 9.0f * B - 6.0f * C) * (x * x * x) + (-18.0f + 12.0f * B + 6.0f * C) * (x * x) + (6.0f - 2.0f * B)) / 6.0f;
    if (x <= 2.0f) return ((-B - 6.0f * C) * (x * x * x) + (6.0f * B + 30.0f * C) * (x * x) + (-12.0f * B - 48.0f * C) * x + (8.0f * B + 24.0f * C)) / 6.0f;
    return 0.0f;
}
float sinc1(float x) {
    x = std::fabs(x);
    if (x < 1e-5f) return 1.0f;
    x *= 3.14159265358979323846f;
    return std::sin(x) / x;
}
float wsinc(float x, float r, float tau) {
    x = std::fabs(x);
    if (x > r) return 0.0f;
    return sinc1(x) * sinc1(x / tau);
}
float filter_eval(const hk_integrator_params& p, float ex, float ey, float x, float y) {
    float rx = p.filter_radius[0], ry = p.filter_radius[1];
    switch (p.filter_type) {
        case HK_FILTER_BOX: return (std::fabs(x) <= rx && std::fabs(y) <= ry) ? 1.0f : 0.0f;
        case HK_FILTER_TRIANGLE: return std::fmax(0.0f, rx - std::fabs(x)) * std::fmax(0.0f, ry - std::fabs(y));
        case HK_FILTER_GAUSSIAN: return std::fmax(0.0f, gaussian_1d(x, p.filter_param1) - ex) * std::fmax(0.0f, gaussian_1d(y, p.filter_param1) - ey);
        case HK_FILTER_MITCHELL: return mitchell_1d(2.0f * x / rx, p.filter_param1, p.filter_param2) * mitchell_1d(2.0f * y / ry, p.filter_param1, p.filter_param2);
        case HK_FILTER_LANCZOS: return wsinc(x, rx, p.filter_param1) * wsinc(y, ry, p.filter_param1);
    }
    return 0.0f;
}
}  // namespace

extern "C" int32_t hk_integrator_create(hk_ctx* c, const hk_integrator_params* p, hk_integrator** out) {
    if (!c || !p || !out) return fail(HK_ERR_INVALID, "null argument");
    if (p->max_depth < 1 || p->max_depth > 255) return fail(HK_ERR_INVALID, "max_depth must be in 1..255");
    if (p->filter_type < HK_FILTER_BOX || p->filter_type > HK_FILTER_LANCZOS) return fail(HK_ERR_INVALID, "bad filter type");
    if (p->material_coherence < 0 || p->material_coherence > 2) return fail(HK_ERR_INVALID, "material_coherence must be :none, :sorted, :per_type");
    HIP_TRY(hipSetDevice(c->device));
    hk_integrator* I = new hk_integrator();
    I->ctx = c;
    I->p = *p;
    DFilter& f = I->filter;
    f.type = p->filter_type;
    f.rx = p->filter_radius[0];
    f.ry = p->filter_radius[1];
    f.p1 = p->filter_param1;
    f.p2 = p->filter_param2;
    if (f.type != HK_FILTER_BOX && f.type != HK_FILTER_TRIANGLE) {
        float ex = 0, ey = 0;
        if (f.type == HK_FILTER_GAUSSIAN) {
            ex = gaussian_1d(f.rx, f.p1);
            ey = gaussian_1d(f.ry, f.p1);
        }
        int nx = (int)std::ceil(32 * f.rx), ny = (int)std::ceil(32 * f.ry);
        if (nx < 8) nx = 8;
        if (ny < 8) ny = 8;
        float dmin_x = -f.rx, dmin_y = -f.ry, dmax_x = f.rx, dmax_y = f.ry;
        float dx = (dmax_x - dmin_x) / (float)nx, dy = (dmax_y - dmin_y) / (float)ny;
        std::vector<float> func((size_t)nx * ny), mfunc(ny, 0.0f), mcdf(ny + 1, 0.0f), ccdf((size_t)ny * (nx + 1), 0.0f);
        for (int iy = 1; iy <= ny; ++iy)
            for (int ix = 1; ix <= nx; ++ix) {
                float px = dmin_x + ((float)ix - 0.5f) * dx, py = dmin_y + ((float)iy - 0.5f) * dy;
                float v = filter_eval(*p, ex, ey, px, py);
                func[(size_t)(iy - 1) * nx + ix - 1] = v > 0.0f ? v : 0.0f;
            }
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) mfunc[iy] += func[(size_t)iy * nx + ix];
        for (int iy = 0; iy < ny; ++iy) mcdf[iy + 1] = mcdf[iy] + mfunc[iy];
        float func_integral = mcdf[ny] * dx * dy;
        float end = mcdf[ny];
        if (end > 0.0f)
            for (auto& v : mcdf) v /= end;
        else
            for (int iy = 0; iy <= ny; ++iy) mcdf[iy] = (float)iy / (float)ny;
        for (int iy = 0; iy < ny; ++iy) {
            float* row = &ccdf[(size_t)iy * (nx + 1)];
            for (int ix = 0; ix < nx; ++ix) row[ix + 1] = row[ix] + func[(size_t)iy * nx + ix];
            float rs = row[nx];
            if (rs > 0.0f)
                for (int ix = 0; ix <= nx; ++ix) row[ix] /= rs;
            else
                for (int ix = 0; ix <= nx; ++ix) row[ix] = (float)ix / (float)nx;
        }
        HIP_TRY(I->f_func.upload(func.data(), func.size() * 4));
        HIP_TRY(I->f_mcdf.upload(mcdf.data(), mcdf.size() * 4));
        HIP_TRY(I->f_mfunc.upload(mfunc.data(), mfunc.size() * 4));
        HIP_TRY(I->f_ccdf.upload(ccdf.data(), ccdf.size() * 4));
        f.nx = nx;
        f.ny = ny;
        f.func = I->f_func.as<float>();
        f.marginal_cdf = I->f_mcdf.as<float>();
        f.marginal_func = I->f_mfunc.as<float>();
        f.conditional_cdf = I->f_ccdf.as<float>();
        f.dmin_x = dmin_x;
        f.dmin_y = dmin_y;
        f.dmax_x = dmax_x;
        f.dmax_y = dmax_y;
        f.func_integral = func_integral;
    }
    *out = I;
    return HK_OK;
}
extern "C" int32_t hk_integrator_destroy(hk_integrator* I) {
    int status = HK_OK;   // the object goes either way; a device error of a pass that was still noted / in flight is reported (hk_last_error)
    if (I) {
        (void)hipSetDevice(I->ctx->device);
        status = join_lanes(I->ctx);
        if (hipStreamSynchronize(I->ctx->stream) != hipSuccess && status == HK_OK) status = fail(HK_ERR_DEVICE, "hk_integrator_destroy: the context's stream reports an error");
        quiesce(I->ctx);
        delete I;
    }
    return status;
}

// ---- path state -----------------------------------------------------------------------------------------
namespace {
// the path-state arrays are carved from ONE allocation (a slab: see SlabCache) instead of ~40; HK_STATE_SLAB=0: one allocation each
template <class T>
hipError_t alloc_arr(hk_integrator* I, T*& dst, size_t n) {
    if (I->slab_mode != 0) {
        const size_t bytes = (n * sizeof(T) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        dst = I->slab_mode == 2 ? reinterpret_cast<T*>(static_cast<char*>(I->slab_base) + I->slab_off) : nullptr;
        I->slab_off += bytes;
        return hipSuccess;
    }
    I->bufs.emplace_back(new DevBuf());
    DevBuf* b = I->bufs.back().get();
    hipError_t e = b->alloc(n * sizeof(T));
    dst = b->as<T>();
    return e;
}
// what of a scene and a call decides the shape of a path state (ensure_state)
struct PassTraits {
    bool media, open_scene, small_scene, grey_compact;
    bool fusable;   // k_small_pass may take the pass (one launch)
    bool lean;      // hk::lean_scene (it implies !media)
};
PassTraits pass_traits(const hk_scene* sc, const hk_ctx* c, int n_samples, bool piped) {
    PassTraits t;
    t.media = sc->d.n_media > 0;
    t.open_scene = sc->d.has_escape_lights != 0;
    t.small_scene = sc->d.bvh_depth <= 16;
    t.grey_compact = sc->d.n_media > 0 && hk::grey_compact_ok(sc->d);
    // (the predicate of launch_small_pass, as far as it is known here: a call of >= 16 samples draws from the sample-bit table
    // and keeps the launches — those want 16 segments per CU, not k_small_pass's 8)
    t.fusable = !piped && !c->time_kernels && !c->count_nodes && n_samples < 16 && hk::small_pass_fusable(sc->d, sc->kinds_mask);
    t.lean = hk::lean_scene(sc->d);
    return t;
}
// the arrays of the path state I->st (capacity, n_waves and wave_cap set), in the order they are carved from the slab (alloc_arr)
int layout_state(hk_integrator* I, bool media, bool want_split, bool want_cam) {
    DPathState& s = I->st;
    const size_t P = (size_t)s.capacity, Q = (size_t)s.n_waves * s.wave_cap;
    const int n_cu = I->ctx->n_cu, W = s.n_waves;
    for (int gidx = 0; gidx < 2; ++gidx) {   // two generations of path records in queue order (DPathGen)
        DPathGen& g = s.gen[gidx];
        HIP_TRY(alloc_arr(I, g.ray_o, Q));
        HIP_TRY(alloc_arr(I, g.ray_d, Q));
        HIP_TRY(alloc_arr(I, g.beta, Q));
        HIP_TRY(alloc_arr(I, g.r_u, Q));
        HIP_TRY(alloc_arr(I, g.r_l, Q));
#if HK_LAMBDA_BY_SLOT
        g.lambda = nullptr;
#else
        HIP_TRY(alloc_arr(I, g.lambda, Q));
#endif
        HIP_TRY(alloc_arr(I, g.meta, Q));
    }
    HIP_TRY(alloc_arr(I, s.hit, Q));
    HIP_TRY(alloc_arr(I, s.mat_id, Q));
    s.sel_light = nullptr;
    if (!media) HIP_TRY(alloc_arr(I, s.sel_light, Q));   // k_light_select's results (8 B per entry)
    HIP_TRY(alloc_arr(I, s.lambda_s, P));
    s.pdf = nullptr;   // recomputed from lambda_s by k_film
    HIP_TRY(alloc_arr(I, s.L, P));
    HIP_TRY(alloc_arr(I, s.filter_w, P));
    HIP_TRY(alloc_arr(I, s.sh_o, Q));
    HIP_TRY(alloc_arr(I, s.sh_d, Q));
    HIP_TRY(alloc_arr(I, s.sh_Ld, Q));
    HIP_TRY(alloc_arr(I, s.sh_ru, Q));
    HIP_TRY(alloc_arr(I, s.sh_rl, Q));
    HIP_TRY(alloc_arr(I, s.sh_slot, Q));
    s.sh_T = nullptr, s.sh_aux = nullptr, s.sh_it = nullptr, s.wq_a = nullptr, s.wq_b = nullptr, s.wq_ctl = nullptr;
    if (want_split) {   // the split shadow walk of grey media (92 B per record; off by default)
        HIP_TRY(alloc_arr(I, s.sh_T, Q));
        HIP_TRY(alloc_arr(I, s.sh_aux, Q));
        HIP_TRY(alloc_arr(I, s.sh_it, 4 * Q));
        // worst case of gq_out_push: a chunk of 256 entries is closed (padded) as soon as the next push of up to 64 does not fit, so 193
        // pushes can use up 256 entries, plus one open chunk per resident wave (at most 32 waves per CU)
        const size_t wq_n = (Q / 193 + 1) * 256 + (size_t)256 * 32 * (size_t)n_cu;
        HIP_TRY(alloc_arr(I, s.wq_a, wq_n));
        HIP_TRY(alloc_arr(I, s.wq_b, wq_n));
        HIP_TRY(alloc_arr(I, s.wq_ctl, (size_t)(I->p.max_depth + 2) * 11 * 4));
    }
    HIP_TRY(alloc_arr(I, s.escaped_q, Q));
    HIP_TRY(alloc_arr(I, s.medium_q, Q));
    HIP_TRY(alloc_arr(I, s.scatter_q, Q));
    s.ticket_rows = I->p.max_depth + 2;
    HIP_TRY(alloc_arr(I, s.tickets, (size_t)s.ticket_rows * HK_TICKET_COLS * HK_TICKET_WAYS * HK_TICKET_STRIDE));
    HIP_TRY(alloc_arr(I, s.initial_medium, 1));
    if (I->slab_mode != 1) HIP_TRY(hipMemset(s.initial_medium, 0xff, sizeof(int)));
    HIP_TRY(alloc_arr(I, s.mat_q, Q * HK_MAX_KINDS));
    size_t nc = (size_t)(I->p.max_depth + 2) * Q_COUNT * W;
    HIP_TRY(alloc_arr(I, s.counters, nc));
    if (I->slab_mode != 1) HIP_TRY(hipMemset(s.counters, 0, nc * sizeof(int)));
    HIP_TRY(alloc_arr(I, s.seg_list, nc));
    HIP_TRY(alloc_arr(I, s.seg_list_n, (size_t)(I->p.max_depth + 2) * Q_COUNT));
    // the camera generation of the view cache (lean records: 16 + 16 + 4 B per entry; a pinhole camera touches one ray_o per segment).  Last,
    // and optional: without the slab an array that cannot be had leaves the set without one (cam_unfit) instead of failing the call.
    I->cam_gen = DPathGen{};
    I->cam_unfit = false;
    if (want_cam) {
        DPathGen g{};
        uint32_t* meta32 = nullptr;
        const size_t n_bufs = I->bufs.size();
        if (alloc_arr(I, g.ray_o, Q) == hipSuccess && alloc_arr(I, g.ray_d, Q) == hipSuccess && alloc_arr(I, meta32, Q) == hipSuccess) {
            g.meta = reinterpret_cast<uint2*>(meta32);
            I->cam_gen = g;
        } else {
            (void)hipGetLastError();
            I->bufs.resize(n_bufs);
            I->cam_unfit = true;
        }
    }
    return HK_OK;
}
// W virtual wave segments: every queue is split W ways and a segment is processed by one wave per kernel, so W is independent of each
// kernel's residency.  Finer segments balance better, but every segment should keep >= 16 chunks (1024 paths) so its per-kind queues
// fill whole waves: W = chunks / 16, capped per CU.  Measured on the four bench scenes (work lists + 64-way XCD-affine tickets):
//   media                     tickets, 96 per CU    (round 3, the 5 %-fill cloud: 1.22 s per frame at 256, 1.14 at 96, 1.18 at 64; the round-2 blob cloud preferred 256)
//   surfaces, closed scene    tickets, 192 per CU   (Cornell 7.19 -> 7.55, many-light 1.11 -> 1.19: trace -10 %, light-BVH shading -9 %)
//   surfaces, open scene      static stride, 48 per CU   (sky: most paths escape after 1-2 vertices; finer segments only fragment
//                             the per-kind queues: k_shade +7 % at 96, +15 % at 256, whichever way they are handed out)
// HK_WAVES_PER_CU / HK_DYNAMIC_SEGMENTS override.  stats rows are indexed by PHYSICAL wave (ctx->stat_rows).
// users: the stream of the lane whose set this is (its last call may still be running), or null
int ensure_state(hk_integrator* I, int capacity, const PassTraits& t, hipStream_t users) {
    const bool media = t.media, open_scene = t.open_scene, small_scene = t.small_scene, grey_compact = t.grey_compact, fusable = t.fusable, lean = t.lean;
    const int n_cu = I->ctx->n_cu;
    // a closed scene's pass of at most HK_MID_PASS_PATHS_M (48) million paths — a rank's share of a frame under 8-way strong scaling —
    // behaves like the open scene WHEN THE SCENE IS SMALL (BVH depth <= 16, the Cornell box): the deep bounces hold a few dozen rays per
    // segment and every visit costs a chunk's latency, so fewer segments and the static stride win (800^2 x 32 spp: 16.3 -> 14.4 ms per
    // frame; x 64: 29.1 -> 27.8; x 128 and x 256 prefer the tickets).  The 10^6-triangle scene's rays are too uneven for a static stride
    // at any size (1024^2 x 32 spp: 115 -> 128 ms).
    long mid_paths = 48L << 20;
    if (const char* e = hk::knob("HK_MID_PASS_PATHS_M")) mid_paths = std::atol(e) >= 0 ? std::atol(e) << 20 : mid_paths;
    const bool mid = !media && !open_scene && small_scene && (long)capacity <= mid_paths;
    I->mid_pass = mid;
    const long cap_per_cu = media ? 96 : ((open_scene || mid) ? 48 : 192);
    long W_want = ((long)(capacity + 63) / 64) / 16;
    if (W_want < 4L * n_cu) W_want = 4L * n_cu;
    if (W_want > cap_per_cu * n_cu) W_want = cap_per_cu * n_cu;
    // read per call (tests toggle it); an unset knob is the built-in policy again — not the last forced count
    I->ctx->waves_per_cu = hk::knob_int_in("HK_WAVES_PER_CU", 1, INT_MAX, 0);
    if (I->ctx->waves_per_cu > 0) W_want = (long)I->ctx->waves_per_cu * n_cu;
    W_want = (W_want + 3) / 4 * 4;
    I->st.dynamic_segments = (media || (!open_scene && !mid)) ? 1 : 0;
    I->st.dynamic_segments = hk::knob_int("HK_DYNAMIC_SEGMENTS", I->st.dynamic_segments) ? 1 : 0;
    I->st.compact = media ? (grey_compact ? 1 : 0) : 1;
    // slim shadow records of k_shadow's scenes (HK_SHADOW_FINAL=0: the 60-byte records of rounds 3-5; A/B switch, films bit-identical)
    I->st.sh_final = (lean && hk::knob_on("HK_SHADOW_FINAL")) ? 1 : 0;
    // lean generation records of the same scenes (HK_LEAN_RECORDS=0: 8-byte meta words, depth-0 origins stored; A/B switch, films bit-identical)
    I->st.meta32 = (lean && hk::knob_on("HK_LEAN_RECORDS")) ? 1 : 0;
    I->st.const_origin = 0;   // (per call: render_tile_now knows the camera)
    // HK_SHADE_PRESCAN=1: k_shade looks a segment's emissive hits up in mat_id before its first vertex, as it did before the flag travelled in the kind-queue entry (A/B switch, films bit-identical)
    I->st.shade_prescan = hk::knob_int("HK_SHADE_PRESCAN", 0) != 0 ? 1 : 0;
    I->st.shade_prefetch = hk::knob_on("HK_SHADE_PREFETCH") ? 1 : 0;   // 0: the LEAN k_shade loads every chunk's records directly (A/B switch, films bit-identical)
    // 0, or HK_SHADE_PRESCAN=1 / HK_SHADE_LEAN=0: the LEAN k_shade of a single-kind scene walks the kind queue, not the generation by slot (A/B switch, films bit-identical)
    I->st.shade_slot_walk = hk::shade_slot_walk_wanted(hk::knob_on("HK_SHADE_SLOT_WALK"), I->st.shade_prescan != 0, hk::knob_on("HK_SHADE_LEAN")) ? 1 : 0;
    I->st.ticket_share = hk::knob_int("HK_TICKET_SHARE", 1) ? 1 : 0;
    {   // a SMALL pass (at most 16 chunks for each of 4 waves per CU: a one-sample call at 800^2) hands segment g to wave g of every launch
        // (static stride where a grid is smaller): the 17 k_segment_lists launches of a call and the ticket round trips go, and the segment
        // count no longer has to stay below every kernel's residency, so it can be as fine as the latency of one wave's chunk wants it —
        // HK_SMALL_PASS_WAVES per CU.  HK_SMALL_PASS=0: lists and tickets as ever.
        const bool small_on = hk::knob_on("HK_SMALL_PASS");
        const bool small = W_want <= 4L * n_cu && small_on && hk::knob("HK_DYNAMIC_SEGMENTS") == nullptr;   // (an explicit HK_DYNAMIC_SEGMENTS keeps lists / tickets: the tests' small films)
        I->st.small_pass = small ? 1 : 0;
        if (mid && I->st.dynamic_segments == 0 && small_on && !hk::knob_int("HK_MID_LISTS", 0))
            I->st.small_pass = 1;   // a mid-size pass of a closed scene: its 48 segments per CU all hold paths down to the last bounce — the work lists (17 launches) list everything
        if (small) {
            I->st.dynamic_segments = 0;
            const int w = hk::knob_int_in("HK_SMALL_PASS_WAVES", 1, INT_MAX, 0);
            // (800^2, one sample per call.  Eight calls in flight on eight lanes (HK_PIPELINE): Cornell 0.99 / 0.89 / 1.03 / 1.30 ms per call at
            // 4 / 8 / 16 / 32 segments per CU, cloud 12.6 / 13.8 / 17.9 / 19.6.  ONE call at a time — the default since small calls are batched,
            // and what a caller that looks at every frame gets: Cornell 2.04 / 1.53 / 1.41 / 1.34 / 1.59 / 1.63 ms at 4 / 8 / 12 / 16 / 20 / 32,
            // cloud 29.8 / 26.0 / 25.4 at 4 / 8 / 16, 10^6 triangles 11.0 / 10.9 / 12.1 at 8 / 16 / 32, sky 2.32 / 2.39 / 2.49: one segment per
            // resident wave — 16 waves per CU is what k_trace_lean's 16-wave block and k_shade's 128 registers hold, and at 8 the 1024-thread
            // trace blocks covered half of the CUs.  An OPEN surface scene keeps 8: its deep bounces are empty and its glass / conductor
            // shade kernels hold fewer than 16 waves per CU.)
            // k_small_pass (`fusable`: the whole pass in one launch) likes 8: 1.05 ms against 1.14 at 16 — fuller chunks, no spills at two waves per SIMD.
            long per_cu = w > 0 ? w : (users ? (media ? 4 : 8) : (((open_scene && !media) || fusable) ? 8 : 16));
            const long chunks = ((long)capacity + 63) / 64;
            while (per_cu > 4 && per_cu * n_cu > chunks) per_cu /= 2;   // (no segment without a chunk)
            if (I->ctx->waves_per_cu <= 0) W_want = (per_cu * n_cu + 3) / 4 * 4;
        }
    }
    const bool want_split = media && hk::walk_split_mode();
    // the view cache's camera generation: sets of surface scenes that the context's own stream renders on (a lane's pass never keeps its records)
    const bool want_cam = !media && !users && hk::knob_on("HK_VIEW_CACHE");
    // the retained state must be of the same flavour: a state allocated for a scene with media has no sel_light (k_light_select would
    // silently not run in a later scene without media), one allocated without HK_WALK_SPLIT has no hand-over queues
    if (I->st_capacity >= capacity && I->st_depth >= I->p.max_depth && I->st.n_waves == (int)W_want && I->st_media == (media ? 1 : 0) && (!want_split || I->st.wq_a != nullptr) &&
        (!want_cam || I->cam_gen.ray_d != nullptr || I->cam_unfit))
        return HK_OK;
    I->view_key.clear();   // whatever the set held goes with its arrays
    if (users) HIP_TRY(hipStreamSynchronize(users));   // (a lane's set: its last call may still be running)
    if (!I->bufs.empty()) quiesce(I->ctx);             // the arrays about to be let go (a cached slab is handed on without a device-wide wait)
    I->bufs.clear();
    DPathState& s = I->st;
    const int W = (int)W_want;
    const int chunks = (capacity + 63) / 64;
    s.capacity = capacity;
    s.n_waves = W;
    s.wave_cap = ((chunks + W - 1) / W) * 64;
    // a generation index is below W * wave_cap; the kind queues keep the emissive flag in an entry's top bit (HK_MATQ_EMISSIVE)
    if ((size_t)W * (size_t)s.wave_cap > 0x7fffffffu) return fail(HK_ERR_INVALID, "pass too large");
    if (hk::knob_on("HK_STATE_SLAB")) {   // (0: one allocation per array, nothing cached)
        // the camera generation is part of the slab when the slab still fits with it (the pass is never made smaller for its sake):
        // measured with it first, and once more without when the memory is not there
        bool cam = want_cam;
        for (;;) {
            I->slab_mode = 1, I->slab_off = 0;
            if (int e = layout_state(I, media, want_split, cam)) {
                I->slab_mode = 0;
                return e;
            }
            size_t free_b = 0, total_b = 0;
            const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
            if (!known) (void)hipGetLastError();
            hipError_t he = hipErrorOutOfMemory;
            if (!(cam && known && I->slab_off > free_b + g_slabs.total(I->ctx->device))) {
                I->bufs.emplace_back(new DevBuf());
                he = I->bufs.back()->alloc_slab(I->ctx->device, I->slab_off);
            }
            if (he == hipSuccess) break;
            (void)hipGetLastError();
            I->bufs.clear();
            if (!cam) {
                I->slab_mode = 0;
                return fail(HK_ERR_DEVICE, "path-state slab allocation failed");
            }
            cam = false;
        }
        I->slab_base = I->bufs.back()->p;
        I->slab_mode = 2, I->slab_off = 0;
        const int e = layout_state(I, media, want_split, cam);
        I->slab_mode = 0;
        if (e) return e;
        I->cam_unfit = want_cam && !cam;
    } else if (int e = layout_state(I, media, want_split, want_cam))
        return e;
    I->st_capacity = capacity;
    I->st_depth = I->p.max_depth;
    I->st_media = media ? 1 : 0;
    if (hk::knob("HK_DEBUG_ALLOC"))
        std::fprintf(stderr, "HK_DEBUG_ALLOC capacity %d Q %zu: ray_o %p ray_d %p beta %p hit %p sh_o %p L %p medium_q %p mat_q %p counters %p\n", capacity, (size_t)W * s.wave_cap, (void*)s.gen[0].ray_o,
                     (void*)s.gen[0].ray_d, (void*)s.gen[0].beta, (void*)s.hit, (void*)s.sh_o, (void*)s.L, (void*)s.medium_q, (void*)s.mat_q, (void*)s.counters);
    return HK_OK;
}
}  // namespace
int ceil_log2(long v) {
    int l = 0;
    while ((1L << l) < v) ++l;
    return l;
}
DSobol make_sobol(const hk_integrator_params& p, int w, int h) {  // compute_zsobol_params, sobol.jl:317-323; volpath.jl:475
    DSobol s;
    int spp = p.samples_per_pixel > 4096 ? p.samples_per_pixel : 4096;
    s.log2_spp = ceil_log2(spp < 1 ? 1 : spp);
    int res_log2 = ceil_log2(w > h ? w : h);
    s.n_base4_digits = res_log2 + (s.log2_spp + 1) / 2;
    s.seed = p.sampler_seed;
    s.width = w;
    s.hi_table = nullptr;
    s.hi_rows = s.hi_stride = 0;
    s.lo_table = nullptr;
    s.lo_rows = s.lo_count = s.lo_offset = 0;
    return s;
}

// ---- a render call, step by step ----
namespace {
// samples per pass: the integrator's, or sized from the film and the free memory
int choose_samples_per_pass(hk_ctx* c, const hk_integrator* I, const DFrame& fr, int n_samples, int& S_out) {
    int S = I->p.samples_per_pass;
    if (S <= 0) {
        // auto: up to ~192 M paths in flight (256 spp of an 800x800 frame).  The chip holds 256 CUs x 16..32 waves x 64 lanes, and
        // the deeper bounces of a pass only keep it busy when the pass starts with hundreds of paths per lane (Cornell 800^2: 5.9 G
        // rays/s at 32 spp per pass, 6.3 at 64, 6.45 at 128, 6.56 at 256); path state is ~440 B per path, i.e. up to ~80 GB of the
        // 288 GB of HBM, halved until it fits in half of the free memory.  HK_MAX_PATHS_M overrides the cap (millions of paths).
        long max_paths = 192L << 20;
        if (const char* e = hk::knob("HK_MAX_PATHS_M")) max_paths = std::atol(e) > 0 ? std::atol(e) << 20 : max_paths;
        S = (int)(max_paths / fr.n_pixels_padded);
        if (S < 1) S = 1;
        if (S > 256) S = 256;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            free_b += g_slabs.total(c->device);   // (cached path-state slabs are given back when an allocation needs them)
            while (S > 1 && (size_t)S * fr.n_pixels_padded * 440 > free_b / 2) S /= 2;
        }
    }
    if (S > n_samples) S = n_samples;
    if ((long)S * fr.n_pixels_padded > 0x3fffffffL) return fail(HK_ERR_INVALID, "pass too large");
    S_out = S;
    return HK_OK;
}
// a small one-pass call goes to the next LANE (hk_ctx::Lane, created on first use): it runs beside the small calls before and after it.
// lane_idx -1: the call runs on the context's stream, which has waited for the lanes.
int pick_lane(hk_ctx* c, hk_integrator* I, const DFrame& fr, int S, int n_samples, int& lane_idx) {
    lane_idx = -1;
    // measured (Cornell 800^2, one sample per call, ms per call): 1 lane 2.47, 2 lanes 1.69, 4 lanes 1.66, 8 lanes 1.36, 16 lanes 1.21;
    // the lanes' path-state sets together stay below 8 GB (440 B per path)
    int n_lanes = 1;   // (off since small calls are batched — HK_PIPELINE = 2 .. 16 turns the lanes on for calls that cannot be: a read-back between them)
    long max_paths = 8L << 20;
    n_lanes = hk::knob_int_in("HK_PIPELINE", 1, 16, n_lanes);
    if (const char* e = hk::knob("HK_PIPELINE_MAX_PATHS_M")) max_paths = std::atol(e) > 0 ? std::atol(e) << 20 : max_paths;
    {
        const long by_memory = (8L << 30) / (440L * (long)S * fr.n_pixels_padded);
        if (n_lanes > by_memory) n_lanes = by_memory < 1 ? 1 : (int)by_memory;
    }
    // (the lanes are streams of their own — see the note on the second hardware queue at `overlap` below — so one small call, or a
    // handful, does not start them: only a run of HK_PIPELINE_AFTER = 4 small calls in a row does, i.e. a progressive viewer)
    const bool small_call = n_samples <= S && (long)S * fr.n_pixels_padded <= max_paths;
    int after = 4;
    after = hk::knob_int_in("HK_PIPELINE_AFTER", 0, INT_MAX, after);
    c->small_streak = small_call ? c->small_streak + 1 : 0;
    const bool lanes_started = c->ev_main != nullptr;
    if (n_lanes > 1 && !c->time_kernels && small_call && (lanes_started || c->small_streak > after)) {
        if ((int)I->lane_sets.size() < (int)hk_ctx::MAX_LANES) I->lane_sets.resize(hk_ctx::MAX_LANES);
        lane_idx = c->next_lane % n_lanes;
        c->next_lane = (lane_idx + 1) % n_lanes;
        hk_ctx::Lane& L = c->lanes[lane_idx];
        if (!L.stream) HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        if (!L.done) {
            HIP_TRY(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
            std::vector<DStats> zero((size_t)c->stat_rows);
            std::memset(zero.data(), 0, zero.size() * sizeof(DStats));
            HIP_TRY(L.stats.upload(zero.data(), zero.size() * sizeof(DStats)));
        }
        if (!c->ev_main) {
            HIP_TRY(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_film, hipEventDisableTiming));
        }
    } else {
        if (int e = join_lanes(c)) return e;
    }
    return HK_OK;
}
// pixel-digit table of the sampler (depends on film size, spp exponent and max_depth only) and the sample-bit table of a many-sample call
int ensure_sobol_tables(hk_ctx* c, hk_integrator* I, const DFrame& fr, DSobol& sob, int first_sample_idx, int n_samples, int sample_stride) {
    const int x0 = fr.x0, y0 = fr.y0;
    const int rows = 4 + 5 * (I->p.max_depth + 1);
    const bool table_same = !(I->sobol_rows != rows || I->sobol_stride != fr.n_pixels_padded || I->sobol_log2 != sob.log2_spp || I->sobol_digits != sob.n_base4_digits ||
                              I->sobol_x0 != x0 || I->sobol_y0 != y0 || I->sobol_tiles_x != fr.tiles_x);
    if (!table_same) {
        if (c->lanes_dirty) {   // lanes may still read the table that is about to be replaced
            if (int e = join_lanes(c)) return e;
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        HIP_TRY(I->sobol_table.alloc((size_t)rows * fr.n_pixels_padded * sizeof(uint2)));
        hk::launch_sobol_table(c->stream, sob, fr, I->sobol_table.as<uint2>(), rows);
        HIP_TRY(hipGetLastError());
        I->sobol_rows = rows;
        I->sobol_stride = fr.n_pixels_padded;
        I->sobol_log2 = sob.log2_spp;
        I->sobol_digits = sob.n_base4_digits;
        I->sobol_x0 = x0, I->sobol_y0 = y0, I->sobol_tiles_x = fr.tiles_x;
    }
    sob.hi_table = I->sobol_table.as<uint2>();
    sob.hi_rows = rows;
    sob.hi_stride = fr.n_pixels_padded;
    // sample-bit table: worth building when the call draws many samples per pixel (a frame), not for one-sample progressive calls.
    // Two bytes per (row, pixel, sample): rows are cut to HK_SOBOL_LO_GB (default 32 GB, and a quarter of the free memory) —
    // the deep rows serve few paths and fall back to hashing the sample digits.
    const long last_idx = (long)first_sample_idx + (long)(n_samples - 1) * sample_stride;
    if (n_samples >= 16 && sob.log2_spp >= 2 && sob.log2_spp <= 16 && (last_idx >> sob.log2_spp) == 0) {
        const int base = sample_stride == 1 ? (first_sample_idx & ~15) : first_sample_idx;
        const int count = (int)((((last_idx - base) / sample_stride + 1) + 15) & ~15L);
        bool same = table_same && I->lo_base == base && I->lo_sample_stride == sample_stride && I->lo_count == count && I->lo_rows > 0;
        if (!same) {
            if (c->lanes_dirty) {   // lanes may still draw from the table that is rebuilt in the same buffer (as for the hi table above)
                if (int e = join_lanes(c)) return e;
                HIP_TRY(hipStreamSynchronize(c->stream));
            }
            double gb = 32.0;
            if (const char* e = hk::knob("HK_SOBOL_LO_GB")) gb = std::atof(e);
            size_t budget = (size_t)(gb * 1e9), free_b = 0, total_b = 0;
            // the buffer of the previous table is reused when it is large enough (another sample range of the same film)
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (free_b + I->sobol_lo.bytes) / 4 < budget) budget = (free_b + I->sobol_lo.bytes) / 4;
            const size_t per_row = (size_t)fr.n_pixels_padded * count * sizeof(uint16_t);
            int lo_rows = (int)(budget / per_row < (size_t)rows ? budget / per_row : (size_t)rows);
            I->lo_rows = 0;
            if (lo_rows > 0 && (size_t)fr.n_pixels_padded * count < 0xffffffffull) {
                // the table is an optimisation: when its memory cannot be had (another context on the device took it since
                // hipMemGetInfo), the call renders with hashed digits instead of failing
                bool have_buf = true;
                if (I->sobol_lo.bytes < per_row * lo_rows || I->sobol_lo.bytes > 2 * per_row * lo_rows) {
                    while (lo_rows > 0 && I->sobol_lo.alloc(per_row * lo_rows) != hipSuccess) {
                        (void)hipGetLastError();
                        lo_rows /= 2;
                    }
                    have_buf = lo_rows > 0;
                }
                if (have_buf) {
                    hk::launch_sobol_lo_table(c->stream, sob, fr, I->sobol_lo.as<uint16_t>(), lo_rows, base, sample_stride, count);
                    HIP_TRY(hipGetLastError());
                    I->lo_rows = lo_rows;
                    I->lo_base = base;
                    I->lo_sample_stride = sample_stride;
                    I->lo_count = count;
                }
            }
        }
        if (I->lo_rows > 0) {
            sob.lo_table = I->sobol_lo.as<uint16_t>();
            sob.lo_rows = I->lo_rows;
            sob.lo_count = I->lo_count;
        }
    }
    return HK_OK;
}
// K14: camera medium, decided on the device (no readback)
int detect_camera_medium(hipStream_t s, hk_integrator* I, const hk_scene* sc, const hk_camera* cam, DStats* dstats) {
    if (sc->d.n_media > 0) {
        const float* m = cam->camera_to_world;
        float w = m[15];
        float cx = m[3], cy = m[7], cz = m[11];
        if (w != 1.0f) {
            float inv = 1.0f / w;
            cx *= inv;
            cy *= inv;
            cz *= inv;
        }
        hk::launch_detect_camera_medium(s, I->st, sc->d, cx, cy, cz, dstats);
    } else
        HIP_TRY(hipMemsetAsync(I->st.initial_medium, 0xff, sizeof(int), s));
    return HK_OK;
}
// The second stream of a pass (enqueue_stages).  Whatever way the pass is left while a shadow kernel runs on it, the stream is joined
// first: the next render's memsets of tickets and counters on `s` must not race with it.
struct ShadowStream {
    hk_ctx* c;
    bool overlap;             // the shadow launches of this pass go to c->aux
    bool in_flight = false;   // ev_join marks a shadow launch the first stream has not waited for
    ~ShadowStream() {
        if (in_flight && c->aux) (void)hipStreamSynchronize(c->aux);
    }
};
// what the passes of one render call share; fr and sob are this call's copies (enqueue_pass sets their per-pass fields)
struct PassCtx {
    hk_ctx* c;
    hk_scene* sc;
    hk_integrator* I;
    hk_film* film;
    DFrame fr;
    DSobol sob;
    DCamera dc;
    DStats* dstats;
    hipStream_t s;
    bool piped;
    int first_sample_idx, sample_stride;
    // VIEW CACHE.  Everything k_camera writes — the depth-0 records, lambda_s, filter_w, the per-segment ray counts, L = 0 — is a pure
    // function of film size, pixel range, sample range, sampler, filter, camera and the layout of the set; none of it depends on the
    // scene.  A one-pass frame on the integrator's own set therefore keeps the camera generation apart from the two that the bounces
    // ping-pong (DPathState::gen_cam), and the next such frame with the same key (view_key_of) does not launch k_camera: a frame
    // loop that edits a resident scene between frames, an animation under a fixed camera, a rank re-rendering its share of samples.
    // view_mode 0: off for this call (gen_cam is gen[0]); 1: k_film zeroes the L entries it has read; 2: a hit clears L with a memset.
    int view_mode = 0;
    std::string view_key_of() const;

    // fn's launches under a pair of events of timing class `cls` (hk_stats_enable_counters bit 1)
    template <class F>
    int timed(int cls, F&& fn) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (c->time_kernels) {
            e0 = get_event(c);
            e1 = get_event(c);
            if (hipEventRecord(e0, s) != hipSuccess) return fail(HK_ERR_DEVICE, "event record failed");
        }
        fn();
        if (c->time_kernels) {
            if (hipEventRecord(e1, s) != hipSuccess) return fail(HK_ERR_DEVICE, "event record failed");
            (cls == 0 ? c->trace_events : c->class_events[cls]).emplace_back(e0, e1);
        }
        return HK_OK;
    }
    // work lists: after every producer, the non-empty segments of the queues it filled (consumers never visit an empty segment)
    int lists(std::initializer_list<std::pair<int, int>> dq, bool kinds_of_depth = false, int kd = 0) {
        int dd[HK_MAX_KINDS + 6], qq[HK_MAX_KINDS + 6], n = 0;
        for (auto& e : dq) dd[n] = e.first, qq[n] = e.second, ++n;
        if (kinds_of_depth)
            for (int kind = 0; kind < HK_MAX_KINDS; ++kind)
                if (sc->kinds_mask & (1u << kind)) dd[n] = kd, qq[n] = Q_MAT0 + kind, ++n;
        if (I->st.small_pass) return HK_OK;
        return timed(3, [&] { hk::launch_segment_lists(s, I->st, n, dd, qq); });
    }
    int enqueue_depth(ShadowStream& sh, int depth);
    int enqueue_stages(bool view_hit);
    int enqueue_pass(int k, int done);
};
// what the camera records of the pass are a function of, byte for byte (fr and sob hold the pass's fields)
std::string PassCtx::view_key_of() const {
    std::string k;
    auto put = [&k](const void* p, size_t n) { k.append(static_cast<const char*>(p), n); };
    put(&dc, sizeof dc);   // (make_camera of the caller's hk_camera: all that generate_ray reads)
    put(&I->filter, sizeof I->filter);
    const int v[] = {fr.width, fr.height, fr.x0, fr.y0, fr.x1, fr.y1, fr.first_sample, fr.sample_stride, fr.samples_in_pass, sob.log2_spp, sob.n_base4_digits, (int)sob.seed, sob.width,
                     fr.implicit_ones, I->st.compact, I->st.meta32, I->st.const_origin, I->st.n_waves, I->st.wave_cap, I->st.dynamic_segments, view_mode, (int)c->tables_epoch};
    put(v, sizeof v);
    return k;
}
// one bounce: traversal, media, escaped rays, light selection, shading per material kind, shadow rays
int PassCtx::enqueue_depth(ShadowStream& sh, int depth) {
    if (int e = timed(0, [&] { hk::launch_trace(s, c->n_cu, I->st, sc->d, c->tables, fr, depth, dstats); })) return e;
    c->trace_launches++;
    if (sh.in_flight) {
        HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
        sh.in_flight = false;
    }
    int first_kind = 1;
    if (sc->d.n_media > 0) {
        if (int e = timed(4, [&] { hk::launch_medium(s, c->n_cu, I->st, sc->d, c->tables, fr, sob, depth, dstats); })) return e;
        c->media_launches += 2;   // k_track + k_scatter
        first_kind = 0;
    }
    if (sc->d.has_escape_lights) {
        if (int e = lists({{depth, Q_ESCAPED}}, true, depth)) return e;
        if (int e = timed(3, [&] { hk::launch_escaped(s, c->n_cu, I->st, sc->d, c->tables, fr, depth); })) return e;
    } else if (int e = lists({}, true, depth))
        return e;
    // scenes with a deep light BVH: the next-event light of every shading vertex of this depth, chosen by a kernel of its own
    // (per-lane descent with refill) — part of the shade class
    if (sc->d.n_lights > 0 && hk::preselect_lights(sc->d, I->st)) {
        if (int e = timed(5, [&] { hk::launch_light_select(s, c->n_cu, I->st, sc->d, c->tables, fr, sob, depth, sc->kinds_mask, dstats); })) return e;
        c->select_launches++;
    }
    for (int kind = 0; kind < HK_MAX_KINDS; ++kind)
        if (sc->kinds_mask & (1u << kind)) {
            if (int e = timed(2, [&] { hk::launch_shade(s, c->n_cu, kind, I->st, sc->d, c->tables, fr, sob, depth, first_kind, dstats); })) return e;
            first_kind = 0;
            c->shade_launches++;
        }
    if (int e = lists({{depth, Q_SHADOW}, {depth + 1, Q_RAY}})) return e;
    if (sc->d.n_lights > 0) {
        if (sh.overlap) {
            HIP_TRY(hipEventRecord(c->ev_fork, s));
            HIP_TRY(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
            hk::launch_shadow(c->aux, c->n_cu, I->st, sc->d, c->tables, fr, depth, dstats + c->stat_rows / 2);
            HIP_TRY(hipEventRecord(c->ev_join, c->aux));
            sh.in_flight = true;
        } else
            if (int e = timed(1, [&] { hk::launch_shadow(s, c->n_cu, I->st, sc->d, c->tables, fr, depth, dstats); })) return e;
        c->shadow_launches++;
    }
    return HK_OK;
}
// the pass as launches: the three clears, camera rays, then bounce by bounce (the launchers size their grids from residency: n_cu)
int PassCtx::enqueue_stages(bool view_hit) {
    HIP_TRY(hipMemsetAsync(I->st.tickets, 0, (size_t)I->st.ticket_rows * HK_TICKET_COLS * HK_TICKET_WAYS * HK_TICKET_STRIDE * sizeof(int), s));
    // queue sizes start every pass at zero: a depth at which no shade / scatter kernel runs (a triangle-free scene lit by an
    // environment map, say) must not see the ray / shadow counts an earlier render left behind.  A view-cache hit keeps row (0, Q_RAY),
    // the first of the block: the ray counts k_camera wrote.
    const size_t kept = view_hit ? (size_t)I->st.n_waves : 0;
    HIP_TRY(hipMemsetAsync(I->st.counters + kept, 0, ((size_t)(I->st_depth + 2) * Q_COUNT * I->st.n_waves - kept) * sizeof(int), s));
    if (I->st.wq_ctl) HIP_TRY(hipMemsetAsync(I->st.wq_ctl, 0, (size_t)(I->st_depth + 2) * 11 * 4 * sizeof(int), s));
    if (!view_hit) {
        if (int e = timed(3, [&] { hk::launch_camera(s, c->n_cu, I->st, fr, c->tables, I->filter, dc, sob, -1); })) return e;
    } else if (view_mode == 2)   // (mode 1: the film kernel of the pass before left L zeroed)
        HIP_TRY(hipMemsetAsync(I->st.L, 0, (size_t)fr.n_pixels_padded * fr.samples_in_pass * sizeof(float4), s));
    if (int e = lists({{0, Q_RAY}})) return e;
    // Two streams: k_shadow of bounce d touches only its shadow records and L; k_trace of bounce d + 1 touches neither.  The
    // shadow launch goes to a second stream behind the shade kernels, the next traversal starts beside it, and the first stream
    // waits for the shadows before anything that adds to L or rewrites shadow records (media tracking, escaped, shade).  The two
    // fill each other's tails and stalls.  With per-kernel timing on (hk_stats_enable_counters bit 1) everything stays on one
    // stream so that the class times add up.
    // (surfaces only: beside the long shadow walks of a media scene the next traversal only competes — cloud -4.5 %; Cornell +-0, sky +1 %, many-light +2.4 %)
    if (const char* e = hk::knob("HK_OVERLAP")) c->overlap = std::atoi(e) ? 1 : 0;
    else c->overlap = -1;
    // A SECOND HARDWARE QUEUE IS NOT FREE ON THIS CHIP: from the moment a process has used a second stream of its own, every kernel of
    // every stream takes 50 - 120 us longer (the completion of one and the start of the next, with or without events between the
    // streams, whatever their flags and priorities; GPU_MAX_HW_QUEUES=1 makes it go away, and so does never creating the stream) —
    // the "two speeds" of DESIGN.md §5: 8 % of a cloud frame (330 launches), 1 - 4 % of a Cornell frame.  The shadow launch on a
    // second stream repays that only where launches are long: the 10^6-triangle scene (+2.9 %); Cornell and sky +-0.1 % with
    // outliers of +4 %.  So: automatic for deep BVHs only, and never in a mid-size pass (800^2 x 32 spp: -4 %).
    const bool want_overlap = c->overlap < 0 ? sc->d.bvh_depth > 16 : c->overlap != 0;
    const bool overlap = want_overlap && !c->time_kernels && sc->d.n_lights > 0 && sc->d.n_media == 0 && !piped && (!I->mid_pass || c->overlap == 1);   // (an explicit HK_OVERLAP=1 is obeyed: the tests' small films)
    if (overlap && !c->aux) {
        HIP_TRY(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    ShadowStream sh{c, overlap};
    for (int depth = 0; depth < I->p.max_depth; ++depth)
        if (int e = enqueue_depth(sh, depth)) return e;
    if (sh.in_flight) {
        HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
        sh.in_flight = false;
    }
    return HK_OK;
}
// samples [done, done + k) of the call: one fused launch where that is the pass's case, else the stages; then the film
int PassCtx::enqueue_pass(int k, int done) {
    fr.samples_in_pass = k;
    {   // reciprocal of the pass's sample count: M = ceil(2^(30+L) / k), L = ceil(log2 k); exact for slots below 2^30 (checked above)
        int L = 0;
        while ((1 << L) < k) ++L;
        fr.s_shr = 30 + L;
        fr.s_mul = (uint32_t)((((uint64_t)1 << fr.s_shr) + (uint64_t)k - 1) / (uint64_t)k);
    }
    fr.first_sample = first_sample_idx + done * sample_stride;
    if (sob.lo_table) sob.lo_offset = (fr.first_sample - I->lo_base) / sample_stride;
    // a small pass of a closed all-matte scene: camera rays and every bounce in ONE launch (k_small_pass), then the film.  It takes no
    // tickets, and every queue size it reads was written before by the same wave: the three clears of enqueue_stages are not for it.
    const bool fused = !c->time_kernels && !piped && hk::launch_small_pass(s, c->n_cu, I->st, sc->d, c->tables, fr, I->filter, dc, sob, I->p.max_depth, sc->kinds_mask, dstats, true, nullptr, 0);
    // the camera generation of this pass: one of its own where the view cache applies, else generation 0
    const int vm = fused ? 0 : view_mode;
    I->st.view_cache = vm;
    I->st.gen_cam = vm ? I->cam_gen : I->st.gen[0];
    const std::string view_key = vm ? view_key_of() : std::string();
    const bool view_hit = vm && I->view_key == view_key;
    I->view_key.clear();   // (until this pass has run to its film: an error return on the way leaves the set without a key)
    bool film_inline = false;
    if (fused) {
        film_inline = fr.samples_in_pass == 1;   // a one-sample pass adds its paths to the film itself
        (void)hk::launch_small_pass(s, c->n_cu, I->st, sc->d, c->tables, fr, I->filter, dc, sob, I->p.max_depth, sc->kinds_mask, dstats, false, film->accum, film_inline ? (film->f64 ? 2 : 1) : 0);
        c->fused_passes++;
    } else if (int e = enqueue_stages(view_hit))
        return e;
    if (piped && c->film_chain) HIP_TRY(hipStreamWaitEvent(s, c->ev_film, 0));   // the film sums in call order
    if (!film_inline)
        if (int e = timed(3, [&] { hk::launch_film(s, I->st, fr, c->tables, film->accum, film->f64); })) return e;
    if (vm) I->view_key = view_key;
    if (view_hit) c->view_cache_hits++;
    if (piped) {
        HIP_TRY(hipEventRecord(c->ev_film, s));
        c->film_chain = true;
    }
    return HK_OK;
}
}  // namespace

extern "C" int32_t hk_render(hk_ctx* c, hk_scene* sc, hk_integrator* I, hk_film* film, const hk_camera* cam, int32_t first_sample_idx, int32_t n_samples,
                             int32_t sample_stride) {
    if (!film) return fail(HK_ERR_INVALID, "null argument");
    return hk_render_tile(c, sc, I, film, cam, first_sample_idx, n_samples, sample_stride, 0, 0, film->width, film->height);
}

static int render_tile_now(hk_ctx* c, hk_scene* sc, hk_integrator* I, hk_film* film, const hk_camera* cam, int32_t first_sample_idx, int32_t n_samples,
                           int32_t sample_stride, int32_t x0, int32_t y0, int32_t x1, int32_t y1);
int flush_pending(hk_ctx* c) {
    if (!c || !c->pending.active) return HK_OK;
    hk_ctx::Pending p = c->pending;
    c->pending.active = false;
    return render_tile_now(c, p.sc, p.I, p.film, &p.cam, p.first, p.n, p.stride, p.x0, p.y0, p.x1, p.y1);
}
extern "C" int32_t hk_render_tile(hk_ctx* c, hk_scene* sc, hk_integrator* I, hk_film* film, const hk_camera* cam, int32_t first_sample_idx, int32_t n_samples,
                                  int32_t sample_stride, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    if (!c || !sc || !I || !film || !cam) return fail(HK_ERR_INVALID, "null argument");
    if (x0 < 0 || y0 < 0 || x1 > film->width || y1 > film->height || x0 > x1 || y0 > y1) return fail(HK_ERR_INVALID, "pixel range outside the film");
    if (x0 == x1 || y0 == y1) return HK_OK;
    if (n_samples < 0 || sample_stride < 1 || first_sample_idx < 1) return fail(HK_ERR_INVALID, "bad sample range");
    if (!c->have_tables) return fail(HK_ERR_INVALID, "hk_ctx_set_tables must be called first");
    if (sc->ctx != c || I->ctx != c || film->ctx != c) return fail(HK_ERR_INVALID, "scene / integrator / film belong to another context");
    if (film->f64 != (I->p.accumulate_f64 != 0)) return fail(HK_ERR_INVALID, "film / integrator accumulation type mismatch");
    if (n_samples == 0) return HK_OK;
    KnobScope knobs(&c->knobs);
    // A small call (a one-sample `render!`: < 1 path per resident lane, 26 launches of 26 - 100 us whatever they hold) is worth a seventh
    // of its time as part of a larger pass, and the film does not depend on the pass size (k_film adds in sample order).  So a small call
    // is only NOTED; calls that continue it grow the note; the pass is rendered when the note holds HK_BATCH_PATHS_M (64) million paths,
    // when a call comes that does not continue it, or when anything looks at the result (flush_pending).  Rendering is asynchronous
    // either way: a device error of a deferred pass is reported by the call that flushes it.  HK_BATCH_PATHS_M=0: every call at once.
    {
        long batch_paths = 64L << 20, small_paths = 8L << 20;   // (Cornell 800^2, 64 one-sample calls: 0.49 / 0.46 / 0.45 ms per call at 32 / 48 / 64 M, cloud 3.8 / 3.7 / 2.8)
        if (const char* e = hk::knob("HK_BATCH_PATHS_M")) batch_paths = std::atol(e) >= 0 ? std::atol(e) << 20 : batch_paths;
        if (const char* e = hk::knob("HK_PIPELINE_MAX_PATHS_M")) small_paths = std::atol(e) > 0 ? std::atol(e) << 20 : small_paths;
        const long px = (long)((x1 - x0 + 7) / 8) * ((y1 - y0 + 7) / 8) * 64;
        hk_ctx::Pending& p = c->pending;
        // A caller that owns the stream or the accumulators may order its own work behind this call with stream / event calls the library
        // never sees (torch.cuda.synchronize(), a reduce of the accumulators): its calls are enqueued at once.  HK_DEFER_EXTERNAL=1: batched all the same.
        const bool visible_order = (c->own_stream_order && !film->external && !film->exposed) || hk::knob_int("HK_DEFER_EXTERNAL", 0);
        const bool small = batch_paths > 0 && visible_order && !c->time_kernels && (long)n_samples * px <= small_paths && I->p.samples_per_pass <= 0;
        if (p.active && small && p.sc == sc && p.I == I && p.film == film && std::memcmp(&p.cam, cam, sizeof(hk_camera)) == 0 && p.stride == sample_stride && p.x0 == x0 &&
            p.y0 == y0 && p.x1 == x1 && p.y1 == y1 && (long)p.first + (long)p.n * p.stride == first_sample_idx && (long)(p.n + n_samples) * px <= batch_paths) {
            p.n += n_samples;
            p.calls += 1;
            return HK_OK;
        }
        if (int e = flush_pending(c)) return e;
        if (small) {
            p.active = true;
            p.sc = sc, p.I = I, p.film = film, p.cam = *cam;
            p.first = first_sample_idx, p.n = n_samples, p.stride = sample_stride, p.x0 = x0, p.y0 = y0, p.x1 = x1, p.y1 = y1, p.calls = 1;
            return HK_OK;
        }
    }
    return render_tile_now(c, sc, I, film, cam, first_sample_idx, n_samples, sample_stride, x0, y0, x1, y1);
}
static int render_tile_now(hk_ctx* c, hk_scene* sc, hk_integrator* I, hk_film* film, const hk_camera* cam, int32_t first_sample_idx, int32_t n_samples,
                           int32_t sample_stride, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);   // (flush_pending reaches this from every entry point)
    const int W = film->width, H = film->height;
    DFrame fr{};
    fr.width = W;
    fr.height = H;
    fr.x0 = x0, fr.y0 = y0, fr.x1 = x1, fr.y1 = y1;
    fr.tiles_x = (x1 - x0 + 7) / 8;
    fr.tiles_y = (y1 - y0 + 7) / 8;
    fr.n_pixels_padded = fr.tiles_x * fr.tiles_y * 64;
    int S = 0, lane_idx = -1;
    if (int e = choose_samples_per_pass(c, I, fr, n_samples, S)) return e;
    if (int e = pick_lane(c, I, fr, S, n_samples, lane_idx)) return e;
    const bool piped = lane_idx >= 0;
    // the lane's path-state set stands in for the integrator's own for the duration of this call
    struct SetGuard {
        hk_integrator* I;
        hk_integrator::StateSet* ls;
        ~SetGuard() {
            if (ls) I->swap_set(*ls);
        }
    } set_guard{I, piped ? &I->lane_sets[lane_idx] : nullptr};
    if (piped) I->swap_set(I->lane_sets[lane_idx]);
    if (int e = ensure_state(I, S * fr.n_pixels_padded, pass_traits(sc, c, n_samples, piped), piped ? c->lanes[lane_idx].stream : nullptr)) return e;
    I->st.const_origin = (I->st.meta32 && !(cam->lens_radius > 0)) ? 1 : 0;   // a pinhole camera: generate_ray gives every path the same origin (hk_device.h), stored once per segment
    fr.sample_stride = sample_stride;
    fr.max_depth = I->p.max_depth;
    fr.regularize = I->p.regularize;
    fr.max_component_value = I->p.max_component_value;
    fr.count_nodes = c->count_nodes;
    fr.implicit_ones = sc->d.n_media == 0 ? 1 : 0;
    {   // loop shapes of the tracking state machines (measured defaults; read per call)
        auto knob = [](const char* name, int dflt) { return hk::knob_int_in(name, 1, 255, dflt); };
        // collision rounds of k_track_flat wait for HK_TRACK_MIN_PENDING lanes, for at most HK_TRACK_EXTRA_ADVANCE further cheap steps (0 = never wait)
        fr.track_gate = hk::knob_int_in("HK_TRACK_MIN_PENDING", 0, 64, 0) | (hk::knob_int_in("HK_TRACK_EXTRA_ADVANCE", 0, 255, 4) << 8);
        fr.delta_advance = knob("HK_DELTA_ADVANCE", 3);
        fr.refill_idle = knob("HK_TRACK_REFILL_IDLE", 24);
        fr.walk_tune = knob("HK_SHADOW_TRACK_BATCH", 8) | (knob("HK_TRACK_ADVANCE", 2) << 8) | (knob("HK_SHADOW_FEED_ROUNDS", 3) << 16) | ((knob("HK_WALK_REFILL_IDLE", 16) > 63 ? 63 : knob("HK_WALK_REFILL_IDLE", 16)) << 24);
    }
    DSobol sob = make_sobol(I->p, W, H);
    if (int e = ensure_sobol_tables(c, I, fr, sob, first_sample_idx, n_samples, sample_stride)) return e;
    DCamera dc = make_camera(*cam);
    DStats* dstats = c->stats.as<DStats>();
    hipStream_t s = c->stream;
    if (piped) {   // behind everything the context's stream holds so far (scene upload, film clear, sampler tables), beside the other lanes
        HIP_TRY(hipEventRecord(c->ev_main, c->stream));
        s = c->lanes[lane_idx].stream;
        HIP_TRY(hipStreamWaitEvent(s, c->ev_main, 0));
        dstats = c->lanes[lane_idx].stats.as<DStats>();
    }
    if (!c->have_span) {
        HIP_TRY(hipEventRecord(c->ev_begin, s));
        c->have_span = true;
    }
    if (int e = detect_camera_medium(s, I, sc, cam, dstats)) return e;
    PassCtx pass{c, sc, I, film, fr, sob, dc, dstats, s, piped, first_sample_idx, sample_stride};
    // the view cache serves lean records (hk::lean_scene: no kernel rewrites a depth-0 record in place, and the camera medium is none)
    // of a frame that is ONE pass on the integrator's own set; other layouts, multi-pass frames and lanes render as ever
    if (!piped && n_samples == S && I->cam_gen.ray_d != nullptr && I->st.meta32 && fr.implicit_ones) {
        const int mode = hk::knob_int("HK_VIEW_CACHE", 1);   // 0: off, 2: L cleared by a memset instead of by k_film (A/B switches; films bit-identical)
        pass.view_mode = mode == 2 ? 2 : (mode != 0 ? 1 : 0);
    }
    for (int done = 0; done < n_samples;) {
        const int k = n_samples - done < S ? n_samples - done : S;
        if (int e = pass.enqueue_pass(k, done)) return e;
        done += k;
    }
    HIP_TRY(hipGetLastError());
    if (piped) {
        HIP_TRY(hipEventRecord(c->lanes[lane_idx].done, s));
        c->lanes_dirty = true;
    } else
        HIP_TRY(hipEventRecord(c->ev_end, s));
    return HK_OK;
}
