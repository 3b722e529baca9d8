// hk_ctx.cpp — the context of the C-ABI (include/hikari_mi355x.h): the error slot, run-time knobs, the slab cache, hk_ctx_* with the
// spectral / sampler tables, hk_sync / hk_flush / hk_trim_cache and the statistics.  The other host files (hk_scene, hk_scene_edit,
// hk_film, hk_render, hk_test_api, hk_comm) share hk_host.h with this one.
#include "hk_host.h"

thread_local std::string g_err;
SlabCache g_slabs;

// (RUN-TIME KNOBS: hk_host.h)
namespace hk {
static thread_local const Knobs* tl_knobs = nullptr;
const char* knob(const char* name) {
    if (!tl_knobs) return nullptr;
    auto it = tl_knobs->kv.find(name);
    return it == tl_knobs->kv.end() ? nullptr : it->second.c_str();
}
static const char* const KNOB_NAMES[] = {
    "HK_BATCH_PATHS_M", "HK_BVH_LEAF", "HK_BVH_BINS", "HK_QNODES", "HK_DEBUG_ALLOC", "HK_DELTA_ADVANCE", "HK_DYNAMIC_SEGMENTS", "HK_GREY", "HK_GREY_COMPACT", "HK_GREY_FLAT", "HK_MAX_PATHS_M",
    "HK_MID_LISTS", "HK_MID_PASS_PATHS_M", "HK_NODE_CACHE", "HK_NVDB_DENSE_MB", "HK_OVERLAP", "HK_PIPELINE", "HK_PIPELINE_AFTER", "HK_PIPELINE_MAX_PATHS_M", "HK_PRESELECT",
    "HK_SELECT_MIN_IDLE", "HK_SHADOW_FEED_ROUNDS", "HK_SHADOW_TRACK_BATCH", "HK_SMALL_PASS", "HK_SMALL_PASS_WAVES", "HK_SOBOL_LO_GB", "HK_SOBOL_TABLE_ONLY",
    "HK_STATE_CACHE_GB", "HK_STATE_SLAB", "HK_TICKET_SHARE", "HK_TRACK_ADVANCE", "HK_TRACK_EXTRA_ADVANCE", "HK_TRACK_MIN_PENDING", "HK_TRACK_POOL", "HK_TRACK_REFILL_IDLE",
    "HK_WALK_POOL", "HK_WALK_REFILL_IDLE", "HK_WALK_SPLIT", "HK_WAVES_PER_CU", "HK_READBACK_PIN", "HK_DEFER_EXTERNAL", "HK_SELECT_POOL", "HK_SMALL_PASS_FUSED", "HK_SMALL_PASS_MERGED", "HK_OCC_SCALE", "HK_ESCAPED_UNROLL", "HK_SHADOW_FINAL", "HK_TRI_PACK", "HK_LEAN_RECORDS", "HK_VIEW_CACHE", "HK_MAJORANT_BLOCK_VOXELS", "HK_BVH_BUILD_SMALL", "HK_SHADE_LEAN", "HK_SHADE_PRESCAN", "HK_SHADE_PREFETCH", "HK_SHADE_SLOT_WALK", "HK_FILM_FOLD", "HK_TRI_GEO"};
static bool known_knob(const char* name) {
    for (const char* k : KNOB_NAMES)
        if (std::strcmp(k, name) == 0) return true;
    return false;
}
}  // namespace hk
KnobScope::KnobScope(const hk::Knobs* k) : prev(hk::tl_knobs) { hk::tl_knobs = k; }
KnobScope::~KnobScope() { hk::tl_knobs = prev; }

void quiesce(hk_ctx* c) {
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    for (auto& l : c->lanes)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
}
int join_lanes(hk_ctx* c) {
    if (!c) return HK_OK;
    if (int e = flush_pending(c)) return e;
    if (!c->lanes_dirty) return HK_OK;
    for (auto& l : c->lanes)
        if (l.done) HIP_TRY(hipStreamWaitEvent(c->stream, l.done, 0));
    c->lanes_dirty = false;
    c->film_chain = false;
    if (c->have_span) HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    return HK_OK;
}
hipEvent_t get_event(hk_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
DCamera make_camera(const hk_camera& c) {
    DCamera d;
    std::memcpy(d.r2c, c.raster_to_camera, 64);
    std::memcpy(d.c2w, c.camera_to_world, 64);
    d.lens_radius = c.lens_radius;
    d.focal_distance = c.focal_distance;
    d.shutter_open = c.shutter_open;
    d.shutter_close = c.shutter_close;
    return d;
}

// ---------------------------------------------------------------------------------------------------
extern "C" const char* hk_last_error(void) { return g_err.c_str(); }

extern "C" int32_t hk_ctx_create(int32_t device_id, void* stream, hk_ctx** out) {
    if (!out) return fail(HK_ERR_INVALID, "out is null");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(HK_ERR_INVALID, "bad device id");
    HIP_TRY(hipSetDevice(device_id));
    hk_ctx* c = new hk_ctx();
    c->device = device_id;
    c->stream = (hipStream_t)stream;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->own_stream_order = stream == nullptr;
    for (const char* name : hk::KNOB_NAMES)   // the ONLY place the library reads the environment (std::getenv below: nowhere else)
        if (const char* e = std::getenv(name)) c->knobs.kv[name] = e;
    KnobScope knobs(&c->knobs);
    {
        c->waves_per_cu = hk::knob_int_in("HK_WAVES_PER_CU", 1, INT_MAX, 0);
        c->stat_rows = c->n_cu * 32 * 2;   // second half: the kernels of the second stream (their waves have the same physical ids)
        if (const char* e = hk::knob("HK_OVERLAP")) c->overlap = std::atoi(e) ? 1 : 0;
        else c->overlap = -1;
        if (const char* e = hk::knob("HK_STATE_CACHE_GB"))
            if (std::atol(e) >= 0) g_slabs.cap_bytes = (size_t)std::atol(e) << 30;
    }
    {
        std::vector<DStats> zero((size_t)c->stat_rows);
        std::memset(zero.data(), 0, zero.size() * sizeof(DStats));
        HIP_TRY(c->stats.upload(zero.data(), zero.size() * sizeof(DStats)));
    }
    HIP_TRY(hipEventCreate(&c->ev_begin));
    HIP_TRY(hipEventCreate(&c->ev_end));
    *out = c;
    return HK_OK;
}
extern "C" int32_t hk_ctx_destroy(hk_ctx* c) {
    if (!c) return HK_OK;
    (void)hipSetDevice(c->device);
    int status = join_lanes(c);
    if (hipStreamSynchronize(c->stream) != hipSuccess && status == HK_OK) status = fail(HK_ERR_DEVICE, "hk_ctx_destroy: the context's stream reports an error");
    for (auto& l : c->lanes) {
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    if (c->ev_film) (void)hipEventDestroy(c->ev_film);
    for (auto& e : c->trace_events) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_end) (void)hipEventDestroy(c->ev_end);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    g_slabs.trim(c->device);
    delete c;
    return status;
}
extern "C" int32_t hk_ctx_set_option(hk_ctx* c, const char* name, const char* value) {
    if (!c || !name) return fail(HK_ERR_INVALID, "null argument");
    if (!hk::known_knob(name)) return fail(HK_ERR_INVALID, std::string("unknown option ") + name);
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;   // calls that were only noted are rendered under the options they were made with
    if (value) c->knobs.kv[name] = value;
    else c->knobs.kv.erase(name);
    if (std::strcmp(name, "HK_STATE_CACHE_GB") == 0) {
        g_slabs.cap_bytes = (size_t)(value && std::atol(value) >= 0 ? std::atol(value) : 128) << 30;
        if (g_slabs.cap_bytes == 0) g_slabs.trim(c->device);
    }
    return HK_OK;
}
extern "C" int32_t hk_ctx_get_option(hk_ctx* c, const char* name, char* out, int32_t out_bytes) {
    if (!c || !name || (out_bytes > 0 && !out)) return fail(HK_ERR_INVALID, "null argument");
    if (!hk::known_knob(name)) return fail(HK_ERR_INVALID, std::string("unknown option ") + name);
    auto it = c->knobs.kv.find(name);
    if (it == c->knobs.kv.end()) {   // unset: the built-in default applies — HK_UNSET, not an error code (HK_ERR_INVALID is -1: a typo must not read as "default")
        if (out_bytes > 0) out[0] = 0;
        return HK_UNSET;
    }
    if (out_bytes > 0) std::snprintf(out, (size_t)out_bytes, "%s", it->second.c_str());
    return (int32_t)it->second.size();
}
extern "C" int32_t hk_flush(hk_ctx* c) {
    if (!c) return fail(HK_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    return join_lanes(c);   // noted calls are enqueued on the context's stream (and the lanes joined): stream-ordered from here on
}
extern "C" int32_t hk_trim_cache(hk_ctx* c) {
    if (!c) return fail(HK_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    g_slabs.trim(c->device);
    return HK_OK;
}
extern "C" int32_t hk_ctx_set_tables(hk_ctx* c, const hk_tables* t) {
    if (!c || !t || !t->sobol_matrices || t->sobol_count < 104 || !t->cie_x || !t->rgb2spec_coeffs) return fail(HK_ERR_INVALID, "bad tables");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = flush_pending(c)) return e;   // (noted small calls are rendered with the tables they were made under)
    if (c->lanes_dirty) {   // renders in flight on the lanes read the tables that are about to be replaced
        if (int e = join_lanes(c)) return e;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(c->sobol.upload(t->sobol_matrices, 104 * sizeof(uint32_t)));  // only Sobol dims 0,1 are ever read
    std::vector<float> cie(3 * 471);
    std::memcpy(&cie[0], t->cie_x, 471 * 4);
    std::memcpy(&cie[471], t->cie_y, 471 * 4);
    std::memcpy(&cie[942], t->cie_z, 471 * 4);
    HIP_TRY(c->cie.upload(cie.data(), cie.size() * 4));
    int res = t->rgb2spec_res;
    size_t nco = (size_t)3 * res * res * res * 3;
    c->h_r2s_scale.assign(t->rgb2spec_scale, t->rgb2spec_scale + res);
    c->h_r2s_coeffs.assign(t->rgb2spec_coeffs, t->rgb2spec_coeffs + nco);
    c->r2s_host.res = res;
    c->r2s_host.scale = c->h_r2s_scale.data();
    c->r2s_host.coeffs = c->h_r2s_coeffs.data();
    HIP_TRY(c->r2s_scale.upload(t->rgb2spec_scale, res * 4));
    HIP_TRY(c->r2s_coeffs.upload(t->rgb2spec_coeffs, nco * 4));
    {   // corner-per-load copy of the coefficient table and the monotonicity the device's cell search relies on
        const size_t R = (size_t)res;
        std::vector<float> pts(3 * R * R * R * 4);
        for (size_t m = 0; m < 3; ++m)
            for (size_t z = 0; z < R; ++z)
                for (size_t y = 0; y < R; ++y)
                    for (size_t x = 0; x < R; ++x) {
                        float* o = &pts[((((m * R + z) * R + y) * R) + x) * 4];
                        for (size_t k = 0; k < 3; ++k) o[k] = t->rgb2spec_coeffs[m + 3 * (z + R * (y + R * (x + R * k)))];
                        o[3] = 0.0f;
                    }
        HIP_TRY(c->r2s_points.upload(pts.data(), pts.size() * 4));
        bool sorted = true;
        for (int i = 1; i < res; ++i)
            if (!(t->rgb2spec_scale[i - 1] <= t->rgb2spec_scale[i])) sorted = false;
        c->tables.rgb2spec_sorted = sorted ? 1 : 0;
    }
    // Sobol dims 0/1 have closed forms (hk_device.h sobol_matrix_product); use them only if the caller's table
    // really is that matrix, otherwise keep the table loop.
    bool closed = true;
    {
        uint32_t col = 0x80000000u;
        for (int b = 0; b < 52; ++b) {
            uint32_t d0 = b < 32 ? (0x80000000u >> b) : 0u;
            if (t->sobol_matrices[b] != d0) closed = false;
            if (b % 32 == 0) col = 0x80000000u;
            if (t->sobol_matrices[52 + b] != col) closed = false;
            col ^= col >> 1;
        }
    }
    c->tables.sobol = closed ? nullptr : c->sobol.as<uint32_t>();
    c->tables.cie = c->cie.as<float>();
    c->tables.rgb2spec_scale = c->r2s_scale.as<float>();
    c->tables.rgb2spec_coeffs = c->r2s_coeffs.as<float>();
    c->tables.rgb2spec_res = res;
    c->tables.rgb2spec_points = c->r2s_points.as<float4>();
    c->have_tables = true;
    c->tables_epoch++;
    return HK_OK;
}

extern "C" int32_t hk_sync(hk_ctx* c) {
    if (!c) return fail(HK_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->aux) HIP_TRY(hipStreamSynchronize(c->aux));   // a render that failed half-way may have left a shadow kernel on the second stream
    return HK_OK;
}
extern "C" int32_t hk_stats_enable_counters(hk_ctx* c, int32_t flags) {
    if (!c) return fail(HK_ERR_INVALID, "null ctx");
    if (int e = join_lanes(c)) return e;   // (noted small calls are rendered under the flags they were made with)
    c->count_nodes = (flags & 1) ? 1 : 0;
    c->time_kernels = (flags & 2) ? 1 : 0;
    return HK_OK;
}
extern "C" int32_t hk_stats_reset(hk_ctx* c) {
    if (!c) return fail(HK_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemset(c->stats.p, 0, (size_t)c->stat_rows * sizeof(DStats)));
    for (auto& l : c->lanes)
        if (l.stats.p) HIP_TRY(hipMemset(l.stats.p, 0, (size_t)c->stat_rows * sizeof(DStats)));
    for (auto& e : c->trace_events) {
        c->event_pool.push_back(e.first);
        c->event_pool.push_back(e.second);
    }
    c->trace_events.clear();
    for (auto& v : c->class_events) {
        for (auto& e : v) {
            c->event_pool.push_back(e.first);
            c->event_pool.push_back(e.second);
        }
        v.clear();
    }
    c->seconds_trace = c->seconds_total = 0.0;
    c->trace_launches = c->shadow_launches = c->shade_launches = c->media_launches = c->select_launches = 0;
    c->fused_passes = c->view_cache_hits = 0;
    c->have_span = false;
    return HK_OK;
}
extern "C" int32_t hk_stats_get(hk_ctx* c, hk_stats* out) {
    if (!c || !out) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    DStats h{};
    {
        // the context's own block + the blocks of the lanes that exist (none unless HK_PIPELINE > 1 has ever started them)
        std::vector<const void*> blocks{c->stats.p};
        for (const auto& l : c->lanes)
            if (l.stats.p) blocks.push_back(l.stats.p);
        std::vector<DStats> rows((size_t)c->stat_rows * blocks.size());
        for (size_t b = 0; b < blocks.size(); ++b)
            HIP_TRY(hipMemcpy(rows.data() + b * (size_t)c->stat_rows, blocks[b], (size_t)c->stat_rows * sizeof(DStats), hipMemcpyDeviceToHost));
        for (const DStats& r : rows) {
            h.rays_closest += r.rays_closest;
            h.rays_shadow += r.rays_shadow;
            h.nodes += r.nodes;
            h.tris += r.tris;
            h.hits += r.hits;
            h.vertices += r.vertices;
            h.collisions += r.collisions;
            h.light_nodes += r.light_nodes;
            h.sh_nodes += r.sh_nodes;
            h.sh_tris += r.sh_tris;
            h.sh_collisions += r.sh_collisions;
            h.nvdb_collisions += r.nvdb_collisions;
            h.sh_nvdb_collisions += r.sh_nvdb_collisions;
            h.dda_steps += r.dda_steps;
            h.sh_dda_steps += r.sh_dda_steps;
            h.scatter_vertices += r.scatter_vertices;
            h.sc_light_nodes += r.sc_light_nodes;
#ifdef HK_DEBUG_UTIL
            for (int k = 0; k < 32; ++k) h.dbg[k] += r.dbg[k];
#endif
        }
#ifdef HK_DEBUG_UTIL
        for (int k = 0; k < 16; ++k)
            if (h.dbg[2 * k]) std::fprintf(stderr, "HK_DEBUG_UTIL[%d]: %.3f of %llu lane-slots\n", k, (double)h.dbg[2 * k + 1] / (double)h.dbg[2 * k], h.dbg[2 * k]);
#endif
    }
    double tr = 0.0;
    for (auto& e : c->trace_events) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) tr += ms * 1e-3;
    }
    double total = 0.0;
    if (c->have_span) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev_begin, c->ev_end) == hipSuccess) total = ms * 1e-3;
    }
    std::memset(out, 0, sizeof *out);
    out->rays_closest = h.rays_closest;
    out->rays_shadow = h.rays_shadow;
    out->bvh_nodes_visited = h.nodes;
    out->tris_tested = h.tris;
    out->hits_accepted = h.hits;
    out->path_vertices = h.vertices;
    out->medium_collisions = h.collisions + h.sh_collisions;
    out->track_collisions = h.collisions;
    out->shadow_collisions = h.sh_collisions;
    out->track_dda_steps = h.dda_steps;
    out->shadow_dda_steps = h.sh_dda_steps;
    out->scatter_vertices = h.scatter_vertices;
    out->light_bvh_nodes = h.light_nodes + h.sc_light_nodes;
    out->seconds_trace = tr;
    out->seconds_total = total;
    out->trace_launches = c->trace_launches;
    out->trace_nodes = h.nodes;
    out->trace_tris = h.tris;
    out->shadow_nodes = h.sh_nodes;
    out->shadow_tris = h.sh_tris;
    out->bvh_nodes_visited = h.nodes + h.sh_nodes;
    out->tris_tested = h.tris + h.sh_tris;
    out->shadow_launches = c->shadow_launches;
    out->shade_launches = c->shade_launches;
    out->media_launches = c->media_launches;
    double cls[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 1; k < 6; ++k)
        for (auto& e : c->class_events[k]) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) cls[k] += ms * 1e-3;
        }
    out->seconds_shadow = cls[1];
    out->seconds_shade = cls[2] + cls[5];   // (the light selection of a deep light BVH is part of K9: inside the shade class, and on its own below)
    out->seconds_other = cls[3];
    out->seconds_media = cls[4];
    out->seconds_select = cls[5];
    out->select_launches = c->select_launches;
    out->fused_passes = c->fused_passes;
    out->view_cache_hits = c->view_cache_hits;
    {   // SURVEY 8(d) algorithmic bytes over the counted units
        const uint64_t hits_closest = h.hits < h.rays_closest ? h.hits : h.rays_closest;   // shading attributes are fetched once per accepted closest hit
        out->bytes_algorithmic_trace = h.rays_closest * (32 + 16) + 64 * h.nodes + 36 * h.tris + 96 * hits_closest;
        out->bytes_algorithmic_shadow = h.rays_shadow * (32 + 16) + 64 * h.sh_nodes + 36 * h.sh_tris;
        out->bytes_algorithmic_shade = h.vertices * (2 * 104 + 64 + 96) + 60 * h.light_nodes;
        // media: per collision 8 taps x 4 B + 4 B majorant = 36 B on a dense grid, 84 B through a NanoVDB tree (+ 8 B x 3
        // levels x 2 leaves); per majorant cell entered (DDA step) 4 B; the delta-tracking kernel reads and rewrites the path state
        // (2 x 104 B) once per tracked ray = per entry of the medium queue, which is what `track_rays` counts; a scattering vertex
        // (K5 + K6) is a path vertex without a material record.
        // The kernels count the collisions of NanoVDB scenes apart (DStats::nvdb_collisions), so a context that renders grid and NanoVDB
        // scenes in one statistics window charges each its own price.
        out->bytes_algorithmic_media = h.collisions * 36 + h.nvdb_collisions * (84 - 36) + 4 * h.dda_steps + h.scatter_vertices * (2 * 104 + 96) + 60 * h.sc_light_nodes;
        out->bytes_algorithmic_shadow += h.sh_collisions * 36 + h.sh_nvdb_collisions * (84 - 36) + 4 * h.sh_dda_steps;
    }
    return HK_OK;
}
