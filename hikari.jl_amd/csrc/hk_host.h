// hk_host.h — what the host-side translation units share (hk_ctx / hk_scene / hk_scene_edit / hk_film / hk_render / hk_test_api /
// hk_comm .cpp): the error slot, the knob scope, device buffers and the slab cache, the four opaque handle structs of the C-ABI and the
// few helpers more than one file calls.  Private to csrc/ and not installed.  Everything declared here has hidden visibility: the
// library exports the hk_* entry points of include/hikari_mi355x.h and nothing of this.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "bvh_build.h"
#include "hk_edit_host.h"
#include "hikari_mi355x.h"
#include "hk_launch.h"
#include "hk_nanovdb.h"
#include "hk_types.h"

#pragma GCC visibility push(hidden)

// the message of the last failing call on this thread, whichever file that call is in (hk_last_error); defined in hk_ctx.cpp
extern thread_local std::string g_err;
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ---------------------------------------------------------------------------------------------------
// RUN-TIME KNOBS.  The library never calls getenv on a render path: hk_ctx_create copies the HK_* variables it knows from the
// environment ONCE into the context, hk_ctx_set_option changes one afterwards, and the code asks hk::knob("HK_X") — a lookup in the
// table of the context whose entry point is running on this thread (KnobScope).  A host that setenv()s beside a render is harmless.
// ---------------------------------------------------------------------------------------------------
namespace hk {
struct Knobs {
    std::unordered_map<std::string, std::string> kv;
};
}  // namespace hk
struct KnobScope {   // the knobs of `k` answer hk::knob on this thread until the scope ends (entry points nest: the outer one is restored)
    const hk::Knobs* prev;
    explicit KnobScope(const hk::Knobs* k);
    ~KnobScope();
};
#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail(HK_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// PATH-STATE SLABS outlive the integrator that asked for them: the ~40 arrays of a path state are carved from one allocation, and a slab
// that is let go is kept (per device, up to HK_STATE_CACHE_GB = 128 in total, the smallest ones dropped first) for the next path state
// that fits it.  Two reasons, both measured on the cloud config (DESIGN.md §5 "two speeds"): allocating 84 GB takes 0.7 - 4 s, and where
// the driver places a LATER big allocation decides whether the gather-heavy kernels run 7 - 9 % slower for the life of that integrator.
// Everything cached is given back when a hipMalloc fails (then retried) and when a context of that device is destroyed.
struct SlabCache {
    struct Entry {
        void* p;
        size_t bytes;
        int dev;
    };
    std::mutex m;
    std::vector<Entry> free_list;
    size_t cap_bytes = (size_t)128 << 30;   // HK_STATE_CACHE_GB (process-wide: the last context created / option set decides)
    size_t cap() const { return cap_bytes; }
    size_t total(int dev) {
        std::lock_guard<std::mutex> g(m);
        size_t t = 0;
        for (const Entry& e : free_list) t += e.dev == dev ? e.bytes : 0;
        return t;
    }
    void* take(int dev, size_t need, size_t& got) {   // the smallest slab that holds `need` without being more than twice as large
        std::lock_guard<std::mutex> g(m);
        int best = -1;
        for (int i = 0; i < (int)free_list.size(); ++i) {
            const Entry& e = free_list[i];
            if (e.dev == dev && e.bytes >= need && e.bytes <= 2 * need + ((size_t)64 << 20) && (best < 0 || e.bytes < free_list[best].bytes)) best = i;
        }
        if (best < 0) return nullptr;
        void* p = free_list[best].p;
        got = free_list[best].bytes;
        free_list.erase(free_list.begin() + best);
        return p;
    }
    void give(int dev, void* p, size_t bytes) {
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> g(m);
            free_list.push_back(Entry{p, bytes, dev});
            size_t t = 0;
            for (const Entry& e : free_list) t += e.bytes;
            const size_t limit = cap();
            while (!free_list.empty() && (t > limit || free_list.size() > 8)) {   // the smallest goes first: the big ones are the expensive ones
                int k = 0;
                for (int i = 1; i < (int)free_list.size(); ++i)
                    if (free_list[i].bytes < free_list[k].bytes) k = i;
                t -= free_list[k].bytes;
                drop.push_back(free_list[k].p);
                free_list.erase(free_list.begin() + k);
            }
        }
        for (void* q : drop) (void)hipFree(q);
    }
    void trim(int dev) {   // dev < 0: every device
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> g(m);
            for (int i = (int)free_list.size() - 1; i >= 0; --i)
                if (dev < 0 || free_list[i].dev == dev) {
                    drop.push_back(free_list[i].p);
                    free_list.erase(free_list.begin() + i);
                }
        }
        for (void* q : drop) (void)hipFree(q);
    }
};
extern SlabCache g_slabs;
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int slab_dev = -1;   // >= 0: a path-state slab of that device (goes back to g_slabs, not to the driver)
    void release() {
        if (p && slab_dev >= 0) {
            // hipFree would have waited for the kernels that still use the memory; a slab goes back to the cache instead, so its OWNER
            // waits first — for the streams of its own context only (quiesce), not for every stream of the host application
            g_slabs.give(slab_dev, p, bytes);
        } else if (p)
            (void)hipFree(p);
        p = nullptr, bytes = 0, slab_dev = -1;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n) {
        release();
        bytes = n;
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {   // the cached slabs are memory too
            (void)hipGetLastError();
            g_slabs.trim(-1);
            e = hipMalloc(&p, n);
        }
        if (e != hipSuccess) p = nullptr, bytes = 0;
        return e;
    }
    hipError_t alloc_slab(int dev, size_t n) {   // a cached slab that fits, or a new one
        release();
        size_t got = 0;
        if (void* q = g_slabs.take(dev, n, got)) {
            p = q, bytes = got, slab_dev = dev;
            return hipSuccess;
        }
        const hipError_t e = alloc(n);
        if (e == hipSuccess) slab_dev = dev;
        return e;
    }
    hipError_t upload(const void* src, size_t n) {
        hipError_t e = alloc(n ? n : 4);
        if (e != hipSuccess) return e;
        if (n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
        return e;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

struct hk_ctx {
    int device = 0;
    hk::Knobs knobs;                      // HK_* as of hk_ctx_create, then hk_ctx_set_option
    bool own_stream_order = true;         // false: the caller handed hk_ctx_create a stream of its own and may order work after a render with stream / event calls
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;            // second stream: the shadow rays of bounce d run beside the traversal of bounce d + 1
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int overlap = -1;                     // the shadow kernels on a second stream: -1 auto (scenes with a deep BVH), HK_OVERLAP=0 / 1 never / always
    int small_streak = 0;                 // consecutive small one-pass render calls so far (the lanes start after HK_PIPELINE_AFTER of them)
    int n_cu = 256;
    int waves_per_cu = 0;      // HK_WAVES_PER_CU: fixed number of wave segments per CU (0 = sized from the pass)
    int stat_rows = 8192;      // DStats rows, indexed by PHYSICAL wave: n_cu * 32 (8 waves x 4 SIMDs is the residency limit)
    DevBuf sobol, cie, r2s_scale, r2s_coeffs, r2s_points, stats;
    DTables tables{};
    bool have_tables = false;
    unsigned tables_epoch = 0;            // counts hk_ctx_set_tables calls (part of the view-cache key: camera samples and wavelengths come from the tables)
    std::vector<float> h_r2s_scale, h_r2s_coeffs;
    hk::RGB2Spec r2s_host;
    int count_nodes = 0, time_kernels = 0;
    unsigned long long fused_passes = 0;   // passes rendered by k_small_pass (one launch)
    unsigned long long view_cache_hits = 0;   // passes that kept the camera records of the pass before them (hk_render.cpp: view cache)
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> trace_events;   // class 0
    std::vector<std::pair<hipEvent_t, hipEvent_t>> class_events[6];  // 1 shadow, 2 shade, 3 other, 4 media, 5 light selection (reported inside the shade class AND on its own)
    uint64_t shadow_launches = 0, shade_launches = 0, media_launches = 0, select_launches = 0;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool have_span = false;
    double seconds_trace = 0.0, seconds_total = 0.0;
    uint64_t trace_launches = 0;
    DStats host_stats{};
    // PIPELINED SMALL PASSES.  A one-sample call (the reference's render!, volpath.jl:445-450: what an interactive viewer drives) puts
    // < 1 path per resident lane in flight: its ~45 launches are each bound by the latency of ONE wave's chunk (50 - 90 us at any
    // path count, profiles/r04_progressive_timeline.txt), the chip idles.  Such calls are independent of each other (another sample
    // index of the same scene), so consecutive small calls go to HK_PIPELINE (default 4) LANES in turn — a stream, a path-state set
    // and a statistics block each — and run beside each other; only the film kernels are chained (sums in call order: the film stays
    // bit-identical to the sequential one).  Whatever reads or rewrites film / state / scene on the context's stream joins the
    // lanes first (join_lanes).
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        DevBuf stats;
    };
    enum { MAX_LANES = 16 };
    Lane lanes[MAX_LANES];        // (created on first use)
    int next_lane = 0;
    // SMALL RENDER CALLS ARE BATCHED (hk_render_tile): consecutive one-pass calls that continue each other — same scene, integrator, film,
    // camera, pixel range and stride, sample indices following on — are only noted here and rendered as ONE pass when something looks
    // (flush_pending: every entry point that reads or rewrites film / statistics / scene / integrator, hk_sync, a call that does not fit)
    struct Pending {
        bool active = false;
        hk_scene* sc = nullptr;
        hk_integrator* I = nullptr;
        hk_film* film = nullptr;
        hk_camera cam{};
        int first = 0, n = 0, stride = 1, x0 = 0, y0 = 0, x1 = 0, y1 = 0, calls = 0;
    } pending;
    bool lanes_dirty = false;     // a lane holds work the context's stream has not waited for
    bool film_chain = false;      // ev_film marks the last film kernel of a lane
    hipEvent_t ev_main = nullptr, ev_film = nullptr;
};

// every stream this context has launched on is idle afterwards (before path-state memory changes hands); other streams of the process are not touched
void quiesce(hk_ctx* c);
// the noted small calls are rendered (hk_render.cpp)
int flush_pending(hk_ctx* c);
// the context's stream waits for everything the lanes were given (cheap when nothing is pending)
int join_lanes(hk_ctx* c);
hipEvent_t get_event(hk_ctx* c);   // from the context's pool
DCamera make_camera(const hk_camera& c);

struct hk_scene {
    hk_ctx* ctx = nullptr;
    DevBuf nodes, qnodes, leaf_tris, positions, normals, uvs, tangents, meta, tri_shade, materials, textures, spectra, mis, lights, lnodes, trails, infinite;
    DevBuf envmaps;
    DevBuf media;
    DScene d{};
    uint32_t kinds_mask = 0;
    int n_materials = 0;
    int bvh_nodes = 0, bvh_leaf_tris = 0, bvh_depth = 0;
    hk::LightBVH lbvh;
    // ---- in-place edits (hk_scene_set_transform, hk_scene_set_vertices, hk_scene_update_materials, hk_scene_update_lights, hk_scene_update_envmap, hk_scene_update_medium) ----
    std::vector<hk_material> h_materials;   // the records as created / last updated: what an update is checked against
    std::vector<hk_light> h_lights;         // likewise; the light BVH is rebuilt from these
    std::vector<DEnvMap> h_envmaps;         // the device records as uploaded (sizes and table pointers; marg_func_int and rot may be stale)
    int n_textures = 0, n_spectra = 0;
    std::vector<int> level_start;           // breadth-first node levels: level L is [level_start[L], level_start[L + 1])
    DevBuf base_pos, base_nrm, base_tan, slot_of_prim;   // base geometry (as created / last hk_scene_set_vertices) and the leaf slot of every triangle (first transform or new vertices)
    int tri_geo = 0;                        // DScene::tri_geo as created (upload_attributes): where the geometry table's rows are
    DevBuf vertex_stage;                    // hk_scene_set_vertices: the uploaded range and its interval table, read by k_set_tris (grows with the largest range)
    DevBuf cost_partial;                    // hk_scene_bvh_cost: the per-block sums of k_bvh_cost (first call)
    double cost_created = 0.0;              // the tree cost of the tree as built (hk_scene_bvh_cost)
    DevBuf rebuilt_cost;                    // hk_scene_rebuild_bvh: k_bvh_cost's sums over the tree it built, then that tree's root node
    int rebuilt_cost_blocks = 0;            // > 0: rebuilt_cost holds that many sums the host has not yet made cost_created of
    bool have_base = false;
    bool qnodes_built = false;              // s->qnodes holds a quantised tree (D.qnodes is null while no grid is known to contain it)
    enum { XF_BLOCK = 1024 };
    std::vector<float> block_box;           // deep trees: lo[3] hi[3] (or a superset) of the base positions of every XF_BLOCK triangles
    struct Xf {
        int end;
        bool identity;
        float m[12];
    };
    std::map<int, Xf> xf;                   // transform of every triangle interval [key, end): the grid of the quantised nodes
    struct Staging {                        // pinned upload buffers of the edits' records and tables, reused once their copies have run
        void* host = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
    };
    std::vector<Staging> staging;
    // ---- hk_scene_refit_lights: what a refit of the light BVH needs besides lnodes, filled from `lbvh` at the scene's FIRST refit
    // (a scene that is never refit pays nothing).  While `ready`, the tree lives on the device: `lbvh` keeps the topology and the
    // trails, its bounds are those of the last build (hk_scene_light_bvh_copy reads `raw` back).  hk_scene_update_lights rebuilds
    // and clears `ready`; the buffers are sized by the light count and stay.
    struct LightRefit {
        bool ready = false;
        hk::LightRefitLayout lay;
        DevBuf raw, parent, leaf_entry, level_entries, stamps;   // per entry: the node as built (bmin bmax w phi cos_o cos_e bits), its parent, its stamp; per light its leaf entry; the inner entries by depth
        DevBuf stage;                                            // one call's records, leaves and slots (sized for an edit of every light)
        uint32_t stamp = 0;
    } lrefit;
    // ---- hk_scene_update_medium: per medium, the record as created / last updated (what an update is checked against; its pointers
    // only say which arrays were given and are never followed), the device record as uploaded, and the buffers (in `owned`) it points into
    struct Medium {
        hk_medium rec{};
        DMedium d{};
        DevBuf *majorant = nullptr, *maj_zero = nullptr, *density = nullptr, *rgb[3] = {nullptr, nullptr, nullptr};
        DevBuf *nvdb = nullptr, *blocks = nullptr, *bricks = nullptr;   // NanoVDB: these grow with the tree (bricks: empty while they do not fit HK_NVDB_DENSE_MB)
    };
    std::vector<Medium> h_media;
    // hk_scene_update_medium_dense: the field as uploaded (a host source only) and the build's working set — control record, flags,
    // slots, lists and tile sums of the three levels; both grow with the largest field
    DevBuf dense_field, dense_work;
    // the arrays the records above point into (texels, spectra, envmap tables, medium grids): freed with the scene, after the staging
    // events below have been waited for (the destructor's body runs before the members go)
    std::vector<std::unique_ptr<DevBuf>> owned;
    DevBuf& own() {
        owned.emplace_back(new DevBuf());
        return *owned.back();
    }
    ~hk_scene() {
        for (auto& st : staging) {
            if (st.ev) (void)hipEventSynchronize(st.ev), (void)hipEventDestroy(st.ev);
            if (st.host) (void)hipHostFree(st.host);
        }
    }
};
// hk_scene.cpp; hk_scene_update_materials bakes and classifies with the same two, hk_scene_update_lights bakes with the third
void bake_material(const hk::RGB2Spec& t, const hk_material& m, DMaterial& o);
bool material_alpha_tested(const hk_material& m);
void bake_light(const hk::RGB2Spec& r2s, const hk_light& l, DLight& o);   // o: zeroed
// hk_scene.cpp; hk_scene_update_medium checks, bakes, plans and classifies with the code hk_scene_create runs
std::string check_medium_record(const hk_medium& m);
void bake_medium_fields(const hk::RGB2Spec& r2s, const hk_medium& m, DMedium& o);
struct NvdbPlan {   // what the device holds of a NanoVDB tree besides its bytes
    int nvb_min[3] = {0, 0, 0}, nvb_dim[3] = {0, 0, 0};   // DMedium::nvb_min / nvb_dim
    float background = 0.0f;
    long long total = 0;          // blocks of the table
    std::vector<uint2> table;     // DMedium::nv_blocks
    bool bricks = false;          // the halo bricks fit HK_NVDB_DENSE_MB
    void fill(DMedium& o) const;
};
int plan_nanovdb(const hk_medium& m, NvdbPlan& p);   // HK_OK, or the refusal of the tree (fail())
// the part of it that follows from the extent (p.nvb_min / p.nvb_dim as scanned) and the size alone: the table's dimensions and limits,
// the brick budget.  hk_scene_update_medium_dense, whose table is built on the device, plans with this.
int plan_nanovdb_shape(long long nvdb_size, NvdbPlan& p);
struct MediaClasses {
    int media_mask = 0, all_grey = 0, grey_pool = 0, grey_bricks = 0;
};
MediaClasses classify_media(const std::vector<DMedium>& dmed, int n_media);
// entries of the trails / infinite arrays of a scene of n lights (the node array has twice as many: hk::LightTables)
inline size_t light_table_capacity(int n_lights) { return n_lights > 0 ? (size_t)n_lights : 1; }

struct hk_film {
    hk_ctx* ctx = nullptr;
    int width = 0, height = 0;
    bool f64 = false;
    DevBuf own;
    void* accum = nullptr;  // device
    bool external = false;  // the caller owns `accum` (and may read it behind stream / event ordering of its own)
    bool exposed = false;   // hk_film_accum_device_ptr handed the accumulators out: the caller may keep the pointer, so calls into this film are never only noted
    DevBuf readback;
    // hk_film_read_rgb / _async: the finalized frame lands in PINNED host memory (two buffers in turn), or straight in the caller's
    // buffer when the caller named it with hk_film_pin_host (HK_READBACK_PIN=1: also a pointer that has come twice in a row)
    float* staging[2] = {nullptr, nullptr};
    int staging_next = 0, staging_last = -1;   // which buffer the next async read fills / the last one filled
    bool read_in_flight = false;
    hipEvent_t ev_read = nullptr;
    void* last_out = nullptr;       // the caller's buffer of the previous synchronous read
    void* pinned_user = nullptr;    // ... registered with the driver (hipHostRegister) — the copy goes there directly
    bool pinned_explicit = false;   // registered by hk_film_pin_host (stays until hk_film_unpin_host / hk_film_destroy)
    void* pin_failed = nullptr;     // HK_READBACK_PIN=1: the pointer whose registration the driver refused (not retried every frame)
    // hk_film_update_aux / hk_film_present: the display chain's device buffers, packed one float4 per pixel in Julia [h,w] order.  Sized
    // once per film (aux on the first update, the rest on the first present) and reused: a steady-state present allocates nothing.
    // The chain's 3-float output frame is `readback`.
    DevBuf guides, albedo;          // (nx, ny, nz, depth) and film.albedo (3 floats per pixel)
    DevBuf frame[2], variance;      // (r, g, b, lum) ping and pong, 3x3 luminance variance of the pass-0 frame
    bool have_aux = false;          // hk_film_update_aux has run
};

struct hk_integrator {
    hk_ctx* ctx = nullptr;
    hk_integrator_params p{};
    DFilter filter{};
    DevBuf f_func, f_mcdf, f_mfunc, f_ccdf;
    // path state (the reference's VolPathState, volpath-state.jl:29-181)
    DPathState st{};
    std::vector<std::unique_ptr<DevBuf>> bufs;
    int st_capacity = 0, st_depth = 0, st_media = -1;   // what the retained path state was allocated for
    // VIEW CACHE (hk_render.cpp).  cam_gen: the camera generation of this set — ray_o, ray_d and a 4-byte meta word per entry, written by
    // k_camera alone (null: none wanted, or cam_unfit: it did not fit beside the rest).  view_key: what the camera records, the depth-0
    // ray counts and the zeroed L that the set holds were generated from; empty unless the last pass on the set kept them and ran to its film.
    DPathGen cam_gen{};
    bool cam_unfit = false;
    std::string view_key;
    bool mid_pass = false;                              // the current pass is a mid-size one of a closed scene (ensure_state): static stride, one stream
    int slab_mode = 0;         // 0: one allocation per array; 1: measuring the slab; 2: carving it
    void* slab_base = nullptr;
    size_t slab_off = 0;
    DevBuf sobol_table;  // DSobol::hi_table
    int sobol_rows = 0, sobol_stride = 0, sobol_log2 = -1, sobol_digits = -1, sobol_x0 = -1, sobol_y0 = -1, sobol_tiles_x = -1;
    DevBuf sobol_lo;     // DSobol::lo_table
    int lo_rows = 0, lo_base = -1, lo_sample_stride = -1, lo_count = 0;
    // the path-state sets of the context's lanes (pipelined small passes); a render on lane l swaps set l in for the duration of the call
    struct StateSet {
        DPathState st{};
        std::vector<std::unique_ptr<DevBuf>> bufs;
        int st_capacity = 0, st_depth = 0, st_media = -1;
        DPathGen cam_gen{};
        bool cam_unfit = false;
        std::string view_key;
    };
    std::vector<StateSet> lane_sets;
    void swap_set(StateSet& o) {
        std::swap(st, o.st);
        std::swap(bufs, o.bufs);
        std::swap(st_capacity, o.st_capacity);
        std::swap(st_depth, o.st_depth);
        std::swap(st_media, o.st_media);
        std::swap(cam_gen, o.cam_gen);
        std::swap(cam_unfit, o.cam_unfit);
        std::swap(view_key, o.view_key);
    }
};
// hk_render.cpp (the sampler parameters of a film; hk_test_sobol / hk_test_camera build the same)
int ceil_log2(long v);
DSobol make_sobol(const hk_integrator_params& p, int w, int h);

struct hk_comm {
    std::vector<hk_ctx*> ctxs;     // local ranks of this process (1 in the one-process-per-GPU layout)
    std::vector<void*> comms;      // ncclComm_t per local rank
    int world = 1;
};

#pragma GCC visibility pop
