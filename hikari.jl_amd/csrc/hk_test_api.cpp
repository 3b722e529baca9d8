// hk_test_api.cpp — the sub-kernel entry points of the parity tests (hk_trace_closest, hk_test_*): arrays up, one launch, arrays down.
#include "hk_host.h"

namespace {
struct Tmp {
    std::vector<void*> ptrs;
    ~Tmp() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class T>
    T* up(const T* src, size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (src && n) (void)hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
        return (T*)p;
    }
};
}  // namespace

extern "C" int32_t hk_trace_closest(hk_ctx* c, hk_scene* sc, int32_t n, const float* o3, const float* d3, const float* tmax, float* out_t, int32_t* out_prim,
                                    float* out_uv2) {
    if (!c || !sc || n < 0) return fail(HK_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    Tmp t;
    float *o = t.up(o3, 3 * (size_t)n), *d = t.up(d3, 3 * (size_t)n), *tm = t.up(tmax, n);
    float* ot = t.up<float>(nullptr, n);
    int* op = t.up<int>(nullptr, n);
    float* ouv = t.up<float>(nullptr, 2 * (size_t)n);
    if (!o || !d || !tm || !ot || !op || !ouv) return fail(HK_ERR_DEVICE, "hipMalloc failed");
    hk::launch_test_trace(c->stream, sc->d, n, o, d, tm, ot, op, ouv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_t, ot, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_prim, op, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_uv2, ouv, 2 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_sobol(hk_ctx* c, int32_t width, int32_t height, int32_t spp, uint32_t seed, int32_t n, const int32_t* px, const int32_t* py,
                                 const int32_t* sample_idx, const int32_t* dim, float* out_1d, float* out_2d) {
    if (!c || !c->have_tables) return fail(HK_ERR_INVALID, "tables not set");
    HIP_TRY(hipSetDevice(c->device));
    hk_integrator_params p{};
    p.samples_per_pixel = spp;
    p.sampler_seed = seed;
    DSobol sob;
    sob.log2_spp = ceil_log2(spp < 1 ? 1 : spp);
    sob.n_base4_digits = ceil_log2(width > height ? width : height) + (sob.log2_spp + 1) / 2;
    sob.seed = seed;
    sob.width = width;
    Tmp t;
    int *a = t.up(px, n), *b = t.up(py, n), *s = t.up(sample_idx, n), *dm = t.up(dim, n);
    float *o1 = t.up<float>(nullptr, n), *o2 = t.up<float>(nullptr, 2 * (size_t)n);
    hk::launch_test_sobol(c->stream, c->tables, sob, n, a, b, s, dm, o1, o2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_1d, o1, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_2d, o2, 2 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_camera(hk_ctx* c, hk_integrator* I, const hk_camera* cam, int32_t width, int32_t height, int32_t n, const int32_t* px, const int32_t* py,
                                  const int32_t* sample_idx, float* out15) {
    if (!c || !I || !cam) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    DSobol sob = make_sobol(I->p, width, height);
    DCamera dc = make_camera(*cam);
    Tmp t;
    int *a = t.up(px, n), *b = t.up(py, n), *s = t.up(sample_idx, n);
    float* o = t.up<float>(nullptr, 15 * (size_t)n);
    hk::launch_test_camera(c->stream, c->tables, I->filter, dc, sob, height, n, a, b, s, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out15, o, 15 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_uplift(hk_ctx* c, int32_t mode, int32_t n, const float* rgb, const float* lambda, float* out) {
    if (!c || !c->have_tables) return fail(HK_ERR_INVALID, "tables not set");
    HIP_TRY(hipSetDevice(c->device));
    Tmp t;
    float *r = t.up(rgb, 3 * (size_t)n), *l = t.up(lambda, 4 * (size_t)n), *o = t.up<float>(nullptr, 4 * (size_t)n);
    hk::launch_test_uplift(c->stream, c->tables, mode, n, r, l, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, o, 4 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_light(hk_ctx* c, hk_scene* sc, int32_t mode, int32_t light_idx_1based, int32_t n, const float* p3, const float* in3, const float* lambda,
                                 float* out) {
    if (!c || !sc || !p3 || !in3 || !lambda || !out) return fail(HK_ERR_INVALID, "null argument");
    if (mode == 0 && (light_idx_1based < 1 || light_idx_1based > sc->d.n_lights)) return fail(HK_ERR_INVALID, "light index out of range");
    HIP_TRY(hipSetDevice(c->device));
    Tmp t;
    float *dp = t.up(p3, 3 * (size_t)n), *di = t.up(in3, 3 * (size_t)n), *dl = t.up(lambda, 4 * (size_t)n), *o = t.up<float>(nullptr, 12 * (size_t)n);
    hk::launch_test_light(c->stream, sc->d, c->tables, mode, light_idx_1based, n, dp, di, dl, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, o, 12 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_bsdf(hk_ctx* c, hk_scene* sc, int32_t mode, int32_t mat_idx, int32_t regularize, int32_t n, const float* wo, const float* wi, const float* ns,
                                const float* lambda, const float* u, const float* uc, float* out) {
    if (!c || !sc || !wo || !wi || !ns || !lambda || !u || !uc || !out) return fail(HK_ERR_INVALID, "null argument");
    if (mat_idx < 0 || mat_idx >= sc->n_materials) return fail(HK_ERR_INVALID, "material index out of range");
    HIP_TRY(hipSetDevice(c->device));
    Tmp t;
    float *dwo = t.up(wo, 3 * (size_t)n), *dwi = t.up(wi, 3 * (size_t)n), *dns = t.up(ns, 3 * (size_t)n), *dl = t.up(lambda, 4 * (size_t)n);
    float *du = t.up(u, 2 * (size_t)n), *duc = t.up(uc, (size_t)n), *o = t.up<float>(nullptr, 10 * (size_t)n);
    hk::launch_test_bsdf(c->stream, sc->d, c->tables, mode, mat_idx, regularize, n, dwo, dwi, dns, dl, du, duc, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, o, 10 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_light_bvh(hk_ctx* c, hk_scene* sc, int32_t n, const float* p3, const float* n3, const float* u, int32_t* out_light, float* out_pmf,
                                     const int32_t* query_light, float* out_query_pmf) {
    if (!c || !sc) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    Tmp t;
    float *p = t.up(p3, 3 * (size_t)n), *nn = t.up(n3, 3 * (size_t)n), *uu = t.up(u, n);
    int* ol = t.up<int>(nullptr, n);
    float* op = t.up<float>(nullptr, n);
    int* q = query_light ? t.up(query_light, n) : nullptr;
    float* oq = t.up<float>(nullptr, n);
    hk::launch_test_light_bvh(c->stream, sc->d, n, p, nn, uu, ol, op, q, oq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_light, ol, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_pmf, op, n * 4, hipMemcpyDeviceToHost));
    if (query_light && out_query_pmf) HIP_TRY(hipMemcpy(out_query_pmf, oq, n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}

// The host twin of hk_scene_refit_lights (hk::refit_light_bvh) on a tree built from `lights`: no device, no context.  The calls are
// applied in turn; call k takes the next call_n[k] entries of index / records.
extern "C" int32_t hk_test_light_refit_host(const hk_light* lights, int32_t n_lights, int32_t n_calls, const int32_t* call_n, const int32_t* index, const hk_light* records,
                                            int32_t* n_nodes, float* nodes_out, uint32_t* bit_trails, uint32_t* table_out) {
    if (!lights || n_lights < 1 || n_calls < 0 || (n_calls > 0 && (!call_n || !index || !records)) || !n_nodes) return fail(HK_ERR_INVALID, "hk_test_light_refit_host: bad argument");
    std::vector<hk_light> all(lights, lights + n_lights);
    hk::LightBVH bvh;
    hk::LightTables t;
    hk::derive_light_tables(all.data(), n_lights, bvh, t);
    hk::LightRefitLayout lay;
    hk::light_refit_layout(bvh, lay);
    size_t at = 0;
    for (int k = 0; k < n_calls; ++k) {
        for (int j = 0; j < call_n[k]; ++j) {
            const int idx = index[at + (size_t)j];
            hk::LightBVHNodeH leaf;
            if (idx < 0 || idx >= n_lights || records[at + (size_t)j].kind != all[(size_t)idx].kind ||
                (hk::light_leaf(records[at + (size_t)j], idx + 1, leaf) == 2) != (bvh.bit_trails[(size_t)idx] != 0xFFFFFFFFu))
                return fail(HK_ERR_INVALID, "hk_test_light_refit_host: an edit hk_scene_refit_lights refuses");
        }
        hk::refit_light_bvh(bvh, t, lay, call_n[k], index + at, records + at);
        for (int j = 0; j < call_n[k]; ++j) all[(size_t)index[at + (size_t)j]] = records[at + (size_t)j];
        at += (size_t)call_n[k];
    }
    *n_nodes = (int32_t)bvh.nodes.size();
    if (nodes_out)
        for (size_t i = 0; i < bvh.nodes.size(); ++i) {   // hk_scene_light_bvh_copy's record
            const hk::LightBVHNodeH& n = bvh.nodes[i];
            float* o = nodes_out + 16 * i;
            std::memcpy(o, n.bmin, 12), std::memcpy(o + 3, n.bmax, 12), std::memcpy(o + 6, n.w, 12);
            o[9] = n.phi, o[10] = n.cos_o, o[11] = n.cos_e;
            o[12] = (n.bits & 1u) ? 1.0f : 0.0f, o[13] = (float)n.child1_or_light, o[14] = (n.bits & 2u) ? 1.0f : 0.0f, o[15] = 0.0f;
        }
    if (bit_trails) std::memcpy(bit_trails, bvh.bit_trails.data(), bvh.bit_trails.size() * 4);
    if (table_out) {   // the walked table at the capacity of the scene: 2 n_lights entries, the rest zero
        std::memset(table_out, 0, 2 * (size_t)n_lights * sizeof(hk::LightNodeRec));
        std::memcpy(table_out, t.nodes.data(), t.nodes.size() * sizeof(hk::LightNodeRec));
    }
    return HK_OK;
}
// the table the light sampler walks, as the device holds it now: 16 words per entry, 2 max(n_lights, 1) entries (waits for the stream)
extern "C" int32_t hk_test_light_table_copy(hk_scene* sc, uint32_t* table_out) {
    if (!sc || !table_out) return fail(HK_ERR_INVALID, "null argument");
    hk_ctx* c = sc->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(table_out, sc->lnodes.p, 2 * light_table_capacity((int)sc->h_lights.size()) * sizeof(DLightNode), hipMemcpyDeviceToHost));
    return HK_OK;
}

extern "C" int32_t hk_test_mix(hk_ctx* c, hk_scene* sc, int32_t mat_idx, int32_t n, const float* p3, const float* wo3, const float* uv2, int32_t* out_mat) {
    if (!c || !sc || !p3 || !wo3 || !uv2 || !out_mat) return fail(HK_ERR_INVALID, "null argument");
    if (mat_idx < 0 || mat_idx >= sc->n_materials) return fail(HK_ERR_INVALID, "material index out of range");
    HIP_TRY(hipSetDevice(c->device));
    Tmp t;
    float *dp = t.up(p3, 3 * (size_t)n), *dw = t.up(wo3, 3 * (size_t)n), *du = t.up(uv2, 2 * (size_t)n);
    int* o = t.up<int>(nullptr, (size_t)n);
    hk::launch_test_mix(c->stream, sc->d, mat_idx, n, dp, dw, du, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_mat, o, (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_medium(hk_ctx* c, hk_scene* sc, int32_t mode, int32_t medium_idx, int32_t n, const float* a3, const float* b3, const float* tmax,
                                  const float* lambda, float* out) {
    if (!c || !sc || !a3 || !lambda || !out || (mode >= 1 && (!b3 || !tmax))) return fail(HK_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 2) return fail(HK_ERR_INVALID, "mode must be 0 (sample_point), 1 (majorant segments) or 2 (majorant segments with the zero-cell fast-forward)");
    if (medium_idx < 0 || medium_idx >= sc->d.n_media) return fail(HK_ERR_INVALID, "medium index out of range");
    HIP_TRY(hipSetDevice(c->device));
    const size_t stride = mode == 0 ? 13 : (size_t)hk::test_majorant_stride();
    Tmp t;
    float *da = t.up(a3, 3 * (size_t)n), *db = b3 ? t.up(b3, 3 * (size_t)n) : nullptr, *dt = tmax ? t.up(tmax, (size_t)n) : nullptr, *dl = t.up(lambda, 4 * (size_t)n);
    float* o = t.up<float>(nullptr, stride * (size_t)n);
    hk::launch_test_medium(c->stream, sc->d, c->tables, mode, medium_idx, n, da, db, dt, dl, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, o, stride * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}
extern "C" int32_t hk_test_trace_lean(hk_ctx* c, hk_scene* sc, int32_t anyhit, int32_t n, const float* o3, const float* d3, const float* tmax, float* out_t, int32_t* out_prim,
                                      float* out_uv2) {
    if (!c || !sc || !o3 || !d3 || !tmax || !out_t || !out_prim || !out_uv2) return fail(HK_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    Tmp t;
    float *o = t.up(o3, 3 * (size_t)n), *d = t.up(d3, 3 * (size_t)n), *tm = t.up(tmax, (size_t)n);
    float *ot = t.up<float>(nullptr, (size_t)n), *ouv = t.up<float>(nullptr, 2 * (size_t)n);
    int* op = t.up<int>(nullptr, (size_t)n);
    hk::launch_test_trace_lean(c->stream, c->n_cu, sc->d, anyhit, n, o, d, tm, ot, op, ouv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_t, ot, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_prim, op, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_uv2, ouv, 2 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}

extern "C" int32_t hk_test_medium_bricks(hk_scene* s, int32_t idx, int32_t* dims, float* out) {
    if (!s || !dims) return fail(HK_ERR_INVALID, "hk_test_medium_bricks: null argument");
    if (idx < 0 || idx >= (int)s->h_media.size()) return fail(HK_ERR_INVALID, "hk_test_medium_bricks: medium index out of range");
    const DMedium& d = s->h_media[idx].d;
    for (int k = 0; k < 3; ++k) dims[k] = d.nv_bricks ? d.nvb_dim[k] : 0;
    if (!d.nv_bricks || !out) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, d.nv_bricks, (size_t)d.nvb_dim[0] * d.nvb_dim[1] * d.nvb_dim[2] * 729 * sizeof(float), hipMemcpyDeviceToHost));
    return HK_OK;
}

extern "C" int32_t hk_test_queue_counts(hk_integrator* I, int32_t depth, int32_t kind, int32_t* n_segments, int32_t* counts, int32_t* flagged) {
    if (!I || !n_segments) return fail(HK_ERR_INVALID, "hk_test_queue_counts: null argument");
    if (kind < -2 || kind >= HK_MAX_KINDS || depth < 0 || depth >= I->st_depth + 2) return fail(HK_ERR_INVALID, "hk_test_queue_counts: kind or depth out of range");
    if (kind < 0 && flagged) return fail(HK_ERR_INVALID, "hk_test_queue_counts: only a kind's queue has flagged entries");
    const int queue = kind == -1 ? Q_RAY : (kind == -2 ? Q_ESCAPED : Q_MAT0 + kind);   // -1: the generation's rays, -2: those that escaped
    if (!I->st.counters) return fail(HK_ERR_INVALID, "hk_test_queue_counts: no pass has been rendered");
    *n_segments = I->st.n_waves;
    if (!counts) return HK_OK;
    hk_ctx* c = I->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(counts, I->st.counters + (size_t)(depth * Q_COUNT + queue) * I->st.n_waves, (size_t)I->st.n_waves * sizeof(int), hipMemcpyDeviceToHost));
    if (!flagged) return HK_OK;
    // the entries themselves (the kind's queue is overwritten by every bounce: they are those of the bounce traced last)
    const size_t Q = (size_t)I->st.n_waves * I->st.wave_cap;
    std::vector<uint32_t> q(Q);
    HIP_TRY(hipMemcpy(q.data(), I->st.mat_q + (size_t)kind * Q, Q * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int w = 0; w < I->st.n_waves; ++w) {
        int n = 0;
        for (int i = 0; i < counts[w] && i < I->st.wave_cap; ++i) n += (q[(size_t)w * I->st.wave_cap + i] & HK_MATQ_EMISSIVE) != 0u;
        flagged[w] = n;
    }
    return HK_OK;
}

extern "C" int32_t hk_test_tri_geo(hk_scene* s, int32_t recompute, int32_t* n_tris, int32_t* has_table, float* out4) {
    if (!s || !n_tris) return fail(HK_ERR_INVALID, "hk_test_tri_geo: null argument");
    const int T = s->d.n_tris;
    *n_tris = T;
    if (has_table) *has_table = s->d.tri_geo != 0 ? 1 : 0;
    if (!out4 || T == 0) return HK_OK;
    if (!recompute && s->d.tri_geo == 0) return fail(HK_ERR_INVALID, "hk_test_tri_geo: the scene has no geometry table");
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    Tmp t;
    float* o = t.up<float>(nullptr, 4 * (size_t)T);
    hk::launch_test_tri_geo(c->stream, s->d, recompute ? 1 : 0, reinterpret_cast<float4*>(o));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out4, o, 4 * (size_t)T * sizeof(float), hipMemcpyDeviceToHost));
    return HK_OK;
}
