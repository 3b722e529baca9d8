// hk_scene.cpp — scene upload: hk_scene_create checks a description, then runs the builders below in order (surface classes, BVH and
// its quantised copy, attributes, textures, spectra, materials, lights and the light BVH, environment maps, media, the device record,
// the tables of the in-place edits).  Each builder takes what it reads and fills what it writes; hk_scene_edit.cpp reuses bake_material,
// material_alpha_tested and bake_light.
#include "hk_host.h"

// ---- constant-colour baking (host float32 arithmetic identical to the device/run-time path) ----------
namespace {
inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline float max3(float a, float b, float c) {
    float m = a > b ? a : b;
    return m > c ? m : c;
}
void bake_bounded(const hk::RGB2Spec& t, float r, float g, float b, float out[4]) {
    hk::rgb_to_coeffs(t, r, g, b, out);
    out[3] = 1.0f;
}
void bake_unbounded(const hk::RGB2Spec& t, float r, float g, float b, float out[4]) {  // uplift_rgb_unbounded (uplift.jl:286-308)
    float m = max3(r, g, b);
    if (m <= 0.0f) {
        out[0] = out[1] = out[2] = out[3] = 0.0f;
        return;
    }
    hk::rgb_to_coeffs(t, r / m, g / m, b / m, out);
    out[3] = m / hk::poly_max(out);
}
void bake_illuminant(const hk::RGB2Spec& t, float r, float g, float b, float out[4]) {  // uplift.jl:514-538
    float m = max3(r, g, b);
    if (m <= 0.0f) {
        out[0] = out[1] = out[2] = out[3] = 0.0f;
        return;
    }
    float scale = 2.0f * m;
    hk::rgb_to_coeffs(t, r / scale, g / scale, b / scale, out);
    out[3] = scale;
}
enum { BAKE_BOUNDED, BAKE_BOUNDED_CLAMP, BAKE_UNBOUNDED };
int bake_mode(int kind, int slot) {
    if (kind == HK_MAT_MATTE && slot == 0) return BAKE_BOUNDED_CLAMP;  // clamp(kd_rgb) then uplift_rgb
    if ((kind == HK_MAT_CONDUCTOR || kind == HK_MAT_COATED_CONDUCTOR) && slot < 2) return BAKE_UNBOUNDED;
    return BAKE_BOUNDED;
}
void node_boxes(const hk::BVHNode& n, float lo[2][3], float hi[2][3]) {
    for (int k = 0; k < 3; ++k) lo[0][k] = n.lo0[k], hi[0][k] = n.hi0[k], lo[1][k] = n.lo1[k], hi[1][k] = n.hi1[k];
}
}  // namespace
// The device record of a material: constant colours baked into sigmoid coefficients (hk_scene_create, hk_scene_update_materials).
void bake_material(const hk::RGB2Spec& t, const hk_material& m, DMaterial& o) {
    std::memset(&o, 0, sizeof o);
    o.kind = (m.kind >= 0 && m.kind <= HK_MAT_FALLBACK) ? m.kind : HK_MAT_FALLBACK;
    o.flags = m.flags;
    std::memcpy(o.i, m.i, sizeof o.i);
    std::memcpy(o.spectrum, m.spectrum, sizeof o.spectrum);
    std::memcpy(o.mix_key, m.mix_key, sizeof o.mix_key);
    for (int k = 0; k < 4; ++k) {
        DSpectrumParam& sp = o.rgb[k];
        sp.tex = m.rgb[k].tex;
        std::memcpy(sp.rgba, m.rgb[k].c, 16);
        float cf[4] = {0, 0, 0, 0};
        if (sp.tex < 0) {
            float r = m.rgb[k].c[0], g = m.rgb[k].c[1], b = m.rgb[k].c[2];
            if (o.kind == HK_MAT_DIFFUSE_TRANSMISSION && k < 2) {  // clamp(rgb * scale, 0, 1) (spectral-eval.jl:2098-2103)
                const float sc = m.f[0].v;
                r = clampf(r * sc, 0.0f, 1.0f), g = clampf(g * sc, 0.0f, 1.0f), b = clampf(b * sc, 0.0f, 1.0f);
            }
            if (o.kind == HK_MAT_COATED_CONDUCTOR && k == 2)  // reflectance mode: clamp(r, 0, 0.9999) (:2924-2928)
                r = clampf(r, 0.0f, 0.9999f), g = clampf(g, 0.0f, 0.9999f), b = clampf(b, 0.0f, 0.9999f);
            switch (bake_mode(o.kind, k)) {
                case BAKE_BOUNDED_CLAMP:
                    r = clampf(r, 0.0f, INFINITY);
                    g = clampf(g, 0.0f, INFINITY);
                    b = clampf(b, 0.0f, INFINITY);
                    bake_bounded(t, r, g, b, cf);
                    break;
                case BAKE_UNBOUNDED: bake_unbounded(t, r, g, b, cf); break;
                default: bake_bounded(t, r, g, b, cf); break;
            }
        }
        sp.coef = make_float4(cf[0], cf[1], cf[2], cf[3]);
    }
    for (int k = 0; k < 8; ++k) {
        o.f[k] = m.f[k].v;
        o.ftex[k] = m.f[k].tex;
    }
}
// Alpha-tested surface (Matte with an alpha texture or alpha < 1).  This class decides DScene::all_opaque, the HK_TRI_OPAQUE bits and so
// which kernel variants run: hk_scene_create classifies with it, and hk_scene_update_materials refuses a record whose class differs.
bool material_alpha_tested(const hk_material& m) { return m.kind == HK_MAT_MATTE && (m.rgb[0].tex >= 0 || m.rgb[0].c[3] < 1.0f); }

// what a medium record must satisfy on its own, whoever hands it in (hk_scene_create; hk_scene_update_medium, which builds the majorant itself)
std::string check_medium_record(const hk_medium& m) {
    if (m.kind < HK_MEDIUM_HOMOGENEOUS || m.kind > HK_MEDIUM_NANOVDB) return "unknown medium kind";
    if (m.kind == HK_MEDIUM_RGB_GRID && ((!m.sigma_a_grid && !m.sigma_s_grid) || (m.Le_grid && !m.sigma_a_grid)))   // media.jl:1073-1079
        return "RGBGridMedium needs sigma_a_grid or sigma_s_grid (and sigma_a_grid when Le_grid is given)";
    return std::string();
}

namespace {
// Checks of a scene description: the arrays, and texture / spectrum / Mix child / area-light / medium / envmap indices.
// Nothing is allocated before a description has passed.
std::string validate_desc(const hk_scene_desc& d) {
    if (d.n_envmaps > 0 && !d.envmaps) return "n_envmaps > 0 but envmaps is null";
    for (int i = 0; i < d.n_lights; ++i)
        if (d.lights && d.lights[i].kind == HK_LIGHT_ENVIRONMENT && (d.lights[i].envmap < 0 || d.lights[i].envmap >= d.n_envmaps)) return "environment light refers to a missing envmap";
    if (d.n_triangles < 0 || (d.n_triangles > 0 && (!d.positions || !d.meta))) return "bad triangle arrays";
    auto need = [](int n, const void* p) { return n <= 0 || p != nullptr; };
    if (d.n_materials < 0 || d.n_textures < 0 || d.n_media_interfaces < 0 || d.n_lights < 0 || d.n_envmaps < 0 || d.n_media < 0 || d.n_spectra < 0) return "negative count";
    if (!need(d.n_materials, d.materials) || !need(d.n_textures, d.textures) || !need(d.n_media_interfaces, d.media_interfaces) || !need(d.n_lights, d.lights) ||
        !need(d.n_media, d.media) || !need(d.n_spectra, d.spectra))
        return "count > 0 with a null array";
    auto tex_ok = [&](int t, int channels) { return t < 0 || (t < d.n_textures && (channels == 0 || d.textures[t].channels == channels || d.textures[t].kind == 1)); };
    for (int i = 0; i < d.n_textures; ++i) {
        const hk_texture& t = d.textures[i];
        if (!t.data || t.width <= 0 || t.height <= 0 || (t.channels != 1 && t.channels != 4) || (t.kind != 0 && t.kind != 1)) return "bad texture record " + std::to_string(i);
        if (t.kind == 1 && (t.height != 3 || t.channels != 4)) return "vertex-colour texture must be face_colors[3, n_faces] RGBA";
    }
    for (int i = 0; i < d.n_spectra; ++i)
        if (d.spectra[i].n < 1 || !d.spectra[i].lambdas || !d.spectra[i].values) return "bad spectrum record " + std::to_string(i);
    for (int i = 0; i < d.n_materials; ++i) {
        const hk_material& m = d.materials[i];
        for (int k = 0; k < 4; ++k)
            if (!tex_ok(m.rgb[k].tex, 0)) return "material " + std::to_string(i) + ": rgb texture index out of range";
        for (int k = 0; k < 8; ++k)
            if (!tex_ok(m.f[k].tex, 0)) return "material " + std::to_string(i) + ": float texture index out of range";
        const bool reads_spectra = m.kind == HK_MAT_CONDUCTOR || m.kind == HK_MAT_COATED_CONDUCTOR;
        for (int k = 0; k < 2; ++k)
            if (reads_spectra && m.spectrum[k] >= d.n_spectra) return "material " + std::to_string(i) + ": spectrum index out of range";
        if (m.kind == HK_MAT_MIX && (m.i[0] < 0 || m.i[0] >= d.n_materials || m.i[1] < 0 || m.i[1] >= d.n_materials))
            return "MixMaterial " + std::to_string(i) + ": child material index out of range";
    }
    for (int i = 0; i < d.n_media_interfaces; ++i) {
        const hk_medium_interface& mi = d.media_interfaces[i];
        if (mi.material < 0 || mi.material >= d.n_materials) return "medium interface references a missing material";
        if (mi.inside < -1 || mi.inside >= d.n_media || mi.outside < -1 || mi.outside >= d.n_media) return "medium interface references a missing medium";
    }
    for (int i = 0; i < d.n_lights; ++i) {
        const hk_light& l = d.lights[i];
        if (l.kind < HK_LIGHT_POINT || l.kind > HK_LIGHT_DIFFUSE_AREA) return "unknown light kind";
        if (l.kind == HK_LIGHT_DIFFUSE_AREA && !tex_ok(l.Le.tex, 0)) return "area light: Le texture index out of range";
    }
    for (int t = 0; t < d.n_triangles; ++t) {
        const hk_tri_meta& m = d.meta[t];
        if ((int64_t)m.medium_interface_idx >= d.n_media_interfaces) return "triangle references a missing medium interface";
        if ((int64_t)m.arealight_flat_idx_1based > d.n_lights) return "triangle references a missing area light";
        // Q34: the index is the light COUNT at push time (scene-mesh.jl:127-128) while the flat order groups the lights by type
        // (light-sampler.jl:289-329): a light of an already-seen type pushed later shifts the area lights and the triangle then names
        // another DiffuseAreaLight — or a light of another kind, for which arealight_Le is black (diffuse-area.jl:81).  Accepted as is.
    }
    for (int i = 0; i < d.n_envmaps; ++i) {
        const hk_envmap& e = d.envmaps[i];
        if (e.width <= 0 || e.height <= 0 || e.nu <= 0 || e.nv <= 0 || !e.data || !e.conditional_func || !e.conditional_cdf || !e.conditional_func_int || !e.marginal_func ||
            !e.marginal_cdf)
            return "incomplete hk_envmap record";
    }
    for (int i = 0; i < d.n_media; ++i) {
        const hk_medium& m = d.media[i];
        std::string bad = check_medium_record(m);
        if (!bad.empty()) return bad;
        if (m.kind != HK_MEDIUM_HOMOGENEOUS && !m.majorant) return "heterogeneous medium without a majorant grid";
    }
    return std::string();
}

// ---- surfaces: opaque = no medium transition and no alpha test possible ----
struct SurfaceClasses {
    std::vector<uint8_t> mi_opaque;   // per medium interface
    bool all_opaque = true;
};
SurfaceClasses classify_surfaces(const hk_scene_desc* d) {
    SurfaceClasses out;
    out.mi_opaque.assign(d->n_media_interfaces > 0 ? d->n_media_interfaces : 1, 1);
    for (int i = 0; i < d->n_media_interfaces; ++i) {
        const hk_medium_interface& mi = d->media_interfaces[i];
        const bool op = mi.inside == mi.outside && !material_alpha_tested(d->materials[mi.material]);
        out.mi_opaque[i] = op;
        if (!op) out.all_opaque = false;
    }
    return out;
}

// ---- BVH ----
struct BvhUpload {
    int root_ref = 0;
    bool have_qnodes = false;   // s->qnodes holds the quantised copy, on the grid below
    float q_base[3] = {0, 0, 0}, q_cell[3] = {1, 1, 1};
};
std::vector<DNode> pack_nodes(const hk::BVH& bvh) {
    std::vector<DNode> dn(bvh.nodes.size() ? bvh.nodes.size() : 1);
    for (size_t i = 0; i < bvh.nodes.size(); ++i) {
        const hk::BVHNode& n = bvh.nodes[i];
        float lo[2][3], hi[2][3];
        node_boxes(n, lo, hi);
        hk_pack_node_boxes(dn[i], lo, hi);
        dn[i].c0 = n.c0;
        dn[i].c1 = n.c1;
        dn[i].pad0 = dn[i].pad1 = 0;
    }
    return dn;
}
std::vector<float4> pack_leaf_tris(const hk::BVH& bvh, const hk_scene_desc* d, const std::vector<uint8_t>& mi_opaque) {
    std::vector<float4> lt(3 * (bvh.leaf_prims.size() ? bvh.leaf_prims.size() : 1));
    for (size_t i = 0; i < bvh.leaf_prims.size(); ++i) {
        int prim = bvh.leaf_prims[i];
        const float* p = d->positions + 9 * (size_t)prim;
        uint32_t flags = 0;
        uint32_t mi = d->meta[prim].medium_interface_idx;
        if (mi_opaque[mi]) flags |= HK_TRI_OPAQUE;
        float pw, fw;
        std::memcpy(&pw, &prim, 4);
        std::memcpy(&fw, &flags, 4);
        hk_pack_leaf_tri(&lt[3 * i], p, pw, fw, 0.0f);
    }
    return lt;
}
// The quantised copy of a tree (DQNode, hk_types.h): 16-bit planes on a grid over the root box, lo rounded down and hi rounded up with one
// more cell of margin.  false: the grid does not contain some box with its margin (the float nodes are used).
bool quantise_nodes(const hk::BVH& bvh, float q_base[3], float q_cell[3], std::vector<DQNode>& qn) {
    for (int k = 0; k < 3; ++k) {
        const double ext = (double)bvh.hi[k] - (double)bvh.lo[k];
        q_cell[k] = (float)std::max(ext / 65527.0, 1e-30);
        q_base[k] = (float)((double)bvh.lo[k] - 3.0 * (double)q_cell[k]);
    }
    qn.resize(bvh.nodes.size());
    bool ok = true;
    for (size_t i = 0; i < bvh.nodes.size(); ++i) {
        const hk::BVHNode& n = bvh.nodes[i];
        float lo[2][3], hi[2][3];
        node_boxes(n, lo, hi);
        hk_quant_node(qn[i], lo, hi, q_base, q_cell);   // (an empty box stays empty: lo > hi)
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 3; ++k) {
                const uint32_t ql = qn[i].w[3 * c + k] & 0xffffu, qh = qn[i].w[3 * c + k] >> 16;
                // the grid must contain the box with its margin (a box outside the root's bounds would be clipped: never for a child of the root)
                if (std::isfinite(lo[c][k]) && std::isfinite(hi[c][k]) &&
                    ((double)q_base[k] + ql * (double)q_cell[k] > lo[c][k] || (double)q_base[k] + qh * (double)q_cell[k] < hi[c][k]))
                    ok = false;
            }
        qn[i].c0 = n.c0;
        qn[i].c1 = n.c1;
    }
    return ok;
}
int upload_bvh(hk_scene* s, const hk_scene_desc* d, const std::vector<uint8_t>& mi_opaque, const hk::BVH& bvh, BvhUpload& out) {
    s->bvh_nodes = (int)bvh.nodes.size();
    s->bvh_leaf_tris = (int)bvh.leaf_prims.size();
    s->bvh_depth = bvh.max_depth;
    out.root_ref = bvh.root_ref;
    const std::vector<DNode> dn = pack_nodes(bvh);
    const std::vector<float4> lt = pack_leaf_tris(bvh, d, mi_opaque);
    HIP_TRY(s->nodes.upload(dn.data(), dn.size() * sizeof(DNode)));
    s->cost_created = hk::tree_cost(bvh.nodes.size(), [&](size_t i, float lo[2][3], float hi[2][3], int& c0, int& c1) {   // hk_scene_bvh_cost: of the float boxes as uploaded
        hk_unpack_node_boxes(dn[i], lo, hi);
        c0 = dn[i].c0, c1 = dn[i].c1;
    });
    // a deep tree gets the quantised copy, read by the lean traversal kernels' deep-tree instantiations (HK_QNODES=0: off)
    // (shallow trees gain nothing: their any-hit kernel with the nodes beyond its LDS cache read from a quantised array — measured,
    //  Cornell shadow class + 1.7 %, two-spheres + 0.7 % — is bound by instruction issue, and the conversions are instructions)
    if (bvh.max_depth > 16 && !bvh.nodes.empty() && hk::knob_on("HK_QNODES")) {
        std::vector<DQNode> qn;
        if (quantise_nodes(bvh, out.q_base, out.q_cell, qn)) {
            HIP_TRY(s->qnodes.upload(qn.data(), qn.size() * sizeof(DQNode)));
            out.have_qnodes = true;
        }
    }
    HIP_TRY(s->leaf_tris.upload(lt.data(), lt.size() * sizeof(float4)));
    return HK_OK;
}

int upload_attributes(hk_scene* s, const hk_scene_desc* d) {
    const int T = d->n_triangles;
    // the geometry table (DScene::tri_geo) lives behind the positions, in their allocation: 16 B per triangle, filled on the device by
    // hk_scene_create (a scene with packed records keeps the rows in the records and needs no room here)
    bool tri_pack = T >= 32768;
    if (const char* e = hk::knob("HK_TRI_PACK")) tri_pack = T > 0 && std::atoi(e) != 0;
    s->tri_geo = hk::tri_geo_word(T, tri_pack);
    HIP_TRY(s->positions.alloc(T > 0 ? hk::positions_floats(T, s->tri_geo, tri_pack) * 4 : 4));
    if (T > 0) HIP_TRY(hipMemcpy(s->positions.p, d->positions, (size_t)T * 9 * 4, hipMemcpyHostToDevice));
    if (d->normals) HIP_TRY(s->normals.upload(d->normals, (size_t)T * 9 * 4));
    if (d->uvs) HIP_TRY(s->uvs.upload(d->uvs, (size_t)T * 6 * 4));
    if (d->tangents) HIP_TRY(s->tangents.upload(d->tangents, (size_t)T * 9 * 4));
    static_assert(sizeof(DTriMeta) == sizeof(hk_tri_meta), "meta layout");
    HIP_TRY(s->meta.upload(d->meta, (size_t)T * sizeof(hk_tri_meta)));
    // scenes whose attribute arrays (108 B per triangle) fit in an XCD's L2 gain nothing and pay the second address path (cloud config,
    // 24 triangles: shade + 4 %): records from 32 768 triangles up.  HK_TRI_PACK=0: never, 1: always (A/B switch and tests; films bit-identical)
    if (tri_pack) {   // packed shading records (DScene::tri_shade): p[9] n[9] uv[6] meta[3] pad[1] geo[4] per triangle, one 128-byte line
        std::vector<float> rec((size_t)T * 32, 0.0f);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        static const float default_uv[6] = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f};   // (0,0), (1,0), (1,1): uv_at's defaults
        for (int t = 0; t < T; ++t) {
            float* r = rec.data() + (size_t)t * 32;
            std::memcpy(r, d->positions + 9 * (size_t)t, 36);
            if (d->normals) std::memcpy(r + 9, d->normals + 9 * (size_t)t, 36);
            else for (int k = 0; k < 9; ++k) r[9 + k] = nan;
            std::memcpy(r + 18, d->uvs ? d->uvs + 6 * (size_t)t : default_uv, 24);
            std::memcpy(r + 24, &d->meta[t], 12);
        }
        HIP_TRY(s->tri_shade.upload(rec.data(), rec.size() * sizeof(float)));
    }
    return HK_OK;
}

int upload_textures(hk_scene* s, const hk_scene_desc* d) {
    std::vector<DTexture> dt(d->n_textures > 0 ? d->n_textures : 1);
    for (int i = 0; i < d->n_textures; ++i) {
        const hk_texture& t = d->textures[i];
        DevBuf* b = &s->own();
        HIP_TRY(b->upload(t.data, (size_t)t.width * t.height * t.channels * 4));
        dt[i].data = b->as<float>();
        dt[i].width = t.width;
        dt[i].height = t.height;
        dt[i].channels = t.channels;
        dt[i].pad = t.kind;  // 0 image, 1 vertex colours
    }
    HIP_TRY(s->textures.upload(dt.data(), dt.size() * sizeof(DTexture)));
    return HK_OK;
}
int upload_spectra(hk_scene* s, const hk_scene_desc* d) {
    std::vector<DPLSpectrum> dsp(d->n_spectra > 0 ? d->n_spectra : 1);
    for (int i = 0; i < d->n_spectra; ++i) {
        const hk_pl_spectrum& sp = d->spectra[i];
        DevBuf* b = &s->own();
        std::vector<float> both(2 * (size_t)sp.n);
        std::memcpy(both.data(), sp.lambdas, sp.n * 4);
        std::memcpy(both.data() + sp.n, sp.values, sp.n * 4);
        HIP_TRY(b->upload(both.data(), both.size() * 4));
        dsp[i].lambdas = b->as<float>();
        dsp[i].values = b->as<float>() + sp.n;
        dsp[i].n = sp.n;
        dsp[i].pad = 0;
    }
    HIP_TRY(s->spectra.upload(dsp.data(), dsp.size() * sizeof(DPLSpectrum)));
    return HK_OK;
}
// materials: constant colours baked into sigmoid coefficients
int upload_materials(hk_scene* s, const hk_scene_desc* d, const hk::RGB2Spec& r2s) {
    std::vector<DMaterial> dm(d->n_materials > 0 ? d->n_materials : 1);
    std::memset(dm.data(), 0, dm.size() * sizeof(DMaterial));
    for (int i = 0; i < d->n_materials; ++i) {
        bake_material(r2s, d->materials[i], dm[i]);
        if (dm[i].kind != HK_MAT_MIX) s->kinds_mask |= 1u << dm[i].kind;
    }
    s->d.has_mix = hk::materials_have_kind(d->materials, (size_t)d->n_materials, HK_MAT_MIX);
    s->d.single_kind = hk::single_material_kind(s->kinds_mask, s->d.has_mix, HK_MAX_KINDS);
    s->n_materials = d->n_materials;
    HIP_TRY(s->materials.upload(dm.data(), dm.size() * sizeof(DMaterial)));
    return HK_OK;
}
int upload_medium_interfaces(hk_scene* s, const hk_scene_desc* d) {
    static_assert(sizeof(DMediumInterface) == 16, "mi layout");
    std::vector<DMediumInterface> dmi(d->n_media_interfaces > 0 ? d->n_media_interfaces : 1);
    for (int i = 0; i < d->n_media_interfaces; ++i) dmi[i] = DMediumInterface{d->media_interfaces[i].material, d->media_interfaces[i].inside, d->media_interfaces[i].outside, 0};
    HIP_TRY(s->mis.upload(dmi.data(), dmi.size() * sizeof(DMediumInterface)));
    return HK_OK;
}

}  // namespace
// ---- lights ----
void bake_light(const hk::RGB2Spec& r2s, const hk_light& l, DLight& o) {   // o: zeroed
    o.kind = l.kind;
    o.flags = (l.two_sided ? 1 : 0) | (l.spectrum_kind == HK_SPEC_ILLUMINANT ? 2 : 0);
    o.scale = l.scale;
    o.area = l.area;
    o.Le_tex = -1;
    float cf[4] = {0, 0, 0, 0};
    if (l.kind == HK_LIGHT_DIFFUSE_AREA) {
        o.Le_tex = l.Le.tex;
        std::memcpy(o.Le_rgba, l.Le.c, 16);
        if (l.Le.tex < 0) bake_bounded(r2s, l.Le.c[0] * l.scale, l.Le.c[1] * l.scale, l.Le.c[2] * l.scale, cf);  // uplift_rgb(Le*scale): Q3
        std::memcpy(o.v, l.v, sizeof o.v);
        std::memcpy(o.normal, l.normal, sizeof o.normal);
        std::memcpy(o.uv, l.uv, sizeof o.uv);
    } else {
        if (l.spectrum_kind == HK_SPEC_ILLUMINANT) {
            cf[0] = l.poly[0];
            cf[1] = l.poly[1];
            cf[2] = l.poly[2];
            cf[3] = l.illum_scale;
        } else
            bake_illuminant(r2s, l.i_rgb[0], l.i_rgb[1], l.i_rgb[2], cf);
        if (l.kind == HK_LIGHT_POINT || l.kind == HK_LIGHT_SPOT) std::memcpy(o.p, l.position, 12);
        if (l.kind == HK_LIGHT_DIRECTIONAL || l.kind == HK_LIGHT_SUN) std::memcpy(o.p, l.direction, 12);
        if (l.kind == HK_LIGHT_SPOT) {
            const float* m = l.world_to_light;
            float rows[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
            std::memcpy(o.v, rows, sizeof rows);
            o.cos_total_width = l.cos_total_width;
            o.cos_falloff_start = l.cos_falloff_start;
        }
        if (l.kind == HK_LIGHT_ENVIRONMENT) {  // scale::RGBSpectrum rides in Le_rgba, the map index in Le_tex
            std::memcpy(o.Le_rgba, l.i_rgb, 16);
            o.Le_tex = l.envmap;
        }
    }
    o.coef = make_float4(cf[0], cf[1], cf[2], cf[3]);
}
namespace {
// The light records, the light BVH and its lists.  has_escape: an ambient or environment light is among them.
// (The parent of this code also kept a `textured_emitters` flag for DScene::simple_lights; it was set only in the branch of the lights
// that are NOT DiffuseAreaLights, under the condition that the light is one, i.e. never.  simple_lights is what has always run:
// no escape light and no texture in the scene — see fill_dscene.  Not "fixed" here: that would change which kernels run.)
int upload_lights(hk_scene* s, const hk_scene_desc* d, const hk::RGB2Spec& r2s, int& has_escape) {
    std::vector<DLight> dl(d->n_lights > 0 ? d->n_lights : 1);
    std::memset(dl.data(), 0, dl.size() * sizeof(DLight));
    has_escape = 0;
    for (int i = 0; i < d->n_lights; ++i) {
        bake_light(r2s, d->lights[i], dl[i]);
        if (d->lights[i].kind == HK_LIGHT_AMBIENT || d->lights[i].kind == HK_LIGHT_ENVIRONMENT) has_escape = 1;
    }
    HIP_TRY(s->lights.upload(dl.data(), dl.size() * sizeof(DLight)));
    static_assert(sizeof(DLightNode) == 64 && sizeof(hk::LightNodeRec) == sizeof(DLightNode), "light node layout");
    static_assert(offsetof(hk::LightNodeRec, half_diag) == offsetof(DLightNode, half_diag) && offsetof(hk::LightNodeRec, w) == offsetof(DLightNode, w) &&
                      offsetof(hk::LightNodeRec, sin_o) == offsetof(DLightNode, sin_o) && offsetof(hk::LightNodeRec, child1_or_light) == offsetof(DLightNode, child1_or_light),
                  "light node layout");
    hk::LightTables t;
    hk::derive_light_tables(d->lights, d->n_lights, s->lbvh, t);
    // each array at the capacity the light count allows (light_table_capacity), the rest zeroed: hk_scene_update_lights rewrites them in
    // place when lights enter or leave the tree, and only the counts of DScene change
    auto put = [](DevBuf& b, const void* src, size_t bytes, size_t cap) -> hipError_t {
        hipError_t e = b.alloc(cap);
        if (e == hipSuccess) e = hipMemset(b.p, 0, cap);
        if (e == hipSuccess) e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    const size_t cap = light_table_capacity(d->n_lights);
    HIP_TRY(put(s->lnodes, t.nodes.data(), t.nodes.size() * sizeof(DLightNode), 2 * cap * sizeof(DLightNode)));
    HIP_TRY(put(s->trails, t.trails.data(), t.trails.size() * 4, cap * 4));
    HIP_TRY(put(s->infinite, t.infinite.data(), t.infinite.size() * 4, cap * 4));
    return HK_OK;
}

// ---- environment maps: texels + Distribution2D tables, layouts as the reference holds them ----
int upload_envmaps(hk_scene* s, const hk_scene_desc* d) {
    std::vector<DEnvMap> de(d->n_envmaps > 0 ? d->n_envmaps : 1);
    std::memset(de.data(), 0, de.size() * sizeof(DEnvMap));
    for (int i = 0; i < d->n_envmaps; ++i) {
        const hk_envmap& e = d->envmaps[i];
        auto up = [&](const float* src, size_t n, const float** dst) -> hipError_t {
            DevBuf* b = &s->own();
            hipError_t err = b->upload(src, n * 4);
            *dst = b->as<float>();
            return err;
        };
        DEnvMap& o = de[i];
        const float* texels = nullptr;
        HIP_TRY(up(e.data, (size_t)e.width * e.height * 4, &texels));
        o.data = reinterpret_cast<const float4*>(texels);
        HIP_TRY(up(e.conditional_func, (size_t)e.nu * e.nv, &o.cond_func));
        HIP_TRY(up(e.conditional_cdf, (size_t)(e.nu + 1) * e.nv, &o.cond_cdf));
        HIP_TRY(up(e.conditional_func_int, (size_t)e.nv, &o.cond_func_int));
        HIP_TRY(up(e.marginal_func, (size_t)e.nv, &o.marg_func));
        HIP_TRY(up(e.marginal_cdf, (size_t)e.nv + 1, &o.marg_cdf));
        o.marg_func_int = e.marginal_func_int;
        o.width = e.width, o.height = e.height, o.nu = e.nu, o.nv = e.nv;
        std::memcpy(o.rot, e.rotation, sizeof o.rot);
    }
    HIP_TRY(s->envmaps.upload(de.data(), de.size() * sizeof(DEnvMap)));
    s->h_envmaps.assign(de.begin(), de.begin() + (d->n_envmaps > 0 ? d->n_envmaps : 0));
    return HK_OK;
}

// ---- media: sigma_a / sigma_s / Le baked with uplift_rgb_unbounded, grids / NanoVDB bytes uploaded ----
// The extent of the block table of a NanoVDB tree = every 8^3 block that is a leaf or lies in a non-background tile (the node tables are
// scanned, so nothing the walk could return differently is left outside), united with the record's index bbox, +1 block of margin for
// the trilinear +1 taps.  Blocks further out hold the root background `bg_probe`.  false: a non-background root tile (not tabulated).
bool nvdb_block_extent(const hk_medium& m, float& bg_probe, int nvb_min[3], int nvb_dim[3]) {
    const unsigned char* B = m.nvdb_bytes;
    bg_probe = hknv::f32(B, m.root_offset_1based + 28);
    int lo[3] = {m.index_bbox_min[0] >> 3, m.index_bbox_min[1] >> 3, m.index_bbox_min[2] >> 3};
    int hi[3] = {m.index_bbox_max[0] >> 3, m.index_bbox_max[1] >> 3, m.index_bbox_max[2] >> 3};
    auto include = [&](long long x0, long long y0, long long z0, long long nblk) {  // voxel origin, extent in blocks
        long long o[3] = {x0 >> 3, y0 >> 3, z0 >> 3};
        for (int k = 0; k < 3; ++k) {
            if (o[k] < lo[k]) lo[k] = (int)o[k];
            if (o[k] + nblk - 1 > hi[k]) hi[k] = (int)(o[k] + nblk - 1);
        }
    };
    auto sext21 = [](unsigned long long v) { return (long long)((v & 0x100000ull) ? (v | ~0x1fffffull) : v); };
    bool unbounded = false;
    for (int i = 0; i < m.root_table_size; ++i) {
        long long tile = m.root_offset_1based + 64 + (long long)i * 32;
        unsigned long long key = (unsigned long long)hknv::i64(B, tile);
        long long tz = sext21(key & 0x1fffffull) << 12, ty = sext21((key >> 21) & 0x1fffffull) << 12, tx = sext21((key >> 42) & 0x1fffffull) << 12;
        long long child = hknv::i64(B, tile + 8);
        if (child == 0) {
            if (hknv::f32(B, tile + 20) != bg_probe) unbounded = true;  // a 4096^3 constant tile: not tabulated
            continue;
        }
        long long upper = m.root_offset_1based + child;
        for (int nu = 0; nu < 32768; ++nu) {
            long long ux = tx + (((nu >> 10) & 31) << 7), uy = ty + (((nu >> 5) & 31) << 7), uz = tz + ((nu & 31) << 7);
            if (!hknv::mask(B, upper + 4128, nu)) {
                if (hknv::f32(B, upper + 8256 + (long long)nu * 8) != bg_probe) include(ux, uy, uz, 16);
                continue;
            }
            long long lower = upper + hknv::i64(B, upper + 8256 + (long long)nu * 8);
            for (int nl = 0; nl < 4096; ++nl) {
                long long lx = ux + (((nl >> 8) & 15) << 3), ly = uy + (((nl >> 4) & 15) << 3), lz = uz + ((nl & 15) << 3);
                if (hknv::mask(B, lower + 544, nl) || hknv::f32(B, lower + 1088 + (long long)nl * 8) != bg_probe) include(lx, ly, lz, 1);
            }
        }
    }
    if (unbounded) return false;
    for (int k = 0; k < 3; ++k) {
        nvb_min[k] = lo[k] - 1;
        nvb_dim[k] = hi[k] - lo[k] + 3;
    }
    return true;
}
// the tree flattened into (leaf offset, constant value bits) per block; false: non-background data on the margin
bool nvdb_block_table(const hk_medium& m, const int nvb_min[3], const long long dim[3], float bg_probe, std::vector<uint2>& table) {
    table.resize((size_t)(dim[0] * dim[1] * dim[2]));
    bool margin_ok = true;
    for (long long bx = 0; bx < dim[0]; ++bx)
        for (long long by = 0; by < dim[1]; ++by)
            for (long long bz = 0; bz < dim[2]; ++bz) {
                float value;
                long long leaf = hknv::find_block(m.nvdb_bytes, m.root_offset_1based, m.root_table_size, (int)((nvb_min[0] + bx) * 8), (int)((nvb_min[1] + by) * 8),
                                                  (int)((nvb_min[2] + bz) * 8), value);
                uint32_t bits;
                std::memcpy(&bits, &value, 4);
                table[(size_t)bz + (size_t)dim[2] * ((size_t)by + (size_t)dim[1] * (size_t)bx)] = make_uint2((uint32_t)leaf, bits);
                const bool on_margin = bx == 0 || by == 0 || bz == 0 || bx == dim[0] - 1 || by == dim[1] - 1 || bz == dim[2] - 1;
                if (on_margin && (leaf != 0 || value != bg_probe)) margin_ok = false;  // cannot happen after the scan above
            }
    return margin_ok;
}
// dense bricks: every block of the table materialised (leaf values copied, constant blocks filled) WITH the first voxel
// plane of its +x / +y / +z neighbours (9^3 floats per block, z fastest), so that the device fetches the eight taps of a
// lookup from one brick at one computed address.  2.9 KB per block: taken when it fits HK_NVDB_DENSE_MB (default 4096 MB —
// 288 GB of HBM are there to be used; the bench cloud needs 67 MB), else the table + leaves path stays.
std::vector<float> nvdb_dense_bricks(const hk_medium& m, const std::vector<uint2>& table, const long long dim[3], float bg_probe) {
    const long long total = dim[0] * dim[1] * dim[2];
    std::vector<float> plain((size_t)total * 512);
    for (size_t b = 0; b < (size_t)total; ++b) {
        const uint2 e = table[b];
        float* dst = plain.data() + b * 512;
        if (e.x == 0u) {
            float v;
            std::memcpy(&v, &e.y, 4);
            for (int n = 0; n < 512; ++n) dst[n] = v;
        } else
            for (int n = 0; n < 512; ++n) dst[n] = hknv::f32(m.nvdb_bytes, (long long)e.x + 96 + (long long)n * 4);
    }
    auto voxel = [&](long long bx, long long by, long long bz, int x, int y, int z) -> float {   // (x, y, z) in 0 .. 8 relative to block (bx, by, bz)
        bx += x >> 3, by += y >> 3, bz += z >> 3;
        if (bx >= dim[0] || by >= dim[1] || bz >= dim[2]) return bg_probe;   // beyond the (background) margin
        return plain[((size_t)bz + (size_t)dim[2] * ((size_t)by + (size_t)dim[1] * (size_t)bx)) * 512 + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7))];
    };
    std::vector<float> bricks((size_t)total * 729);
    for (long long bx = 0; bx < dim[0]; ++bx)
        for (long long by = 0; by < dim[1]; ++by)
            for (long long bz = 0; bz < dim[2]; ++bz) {
                float* dst = bricks.data() + ((size_t)bz + (size_t)dim[2] * ((size_t)by + (size_t)dim[1] * (size_t)bx)) * 729;
                for (int x = 0; x < 9; ++x)
                    for (int y = 0; y < 9; ++y)
                        for (int z = 0; z < 9; ++z) dst[x * 81 + y * 9 + z] = voxel(bx, by, bz, x, y, z);
            }
    return bricks;
}
}  // namespace
// What the device holds of a NanoVDB tree besides its bytes: extent and background of the block table, the table, and whether the halo
// bricks fit HK_NVDB_DENSE_MB.  Every refusal of a tree is here, for hk_scene_create and hk_scene_update_medium alike; the limits and the
// budget, which follow from the extent alone, also for hk_scene_update_medium_dense (plan_nanovdb_shape).
int plan_nanovdb_shape(long long nvdb_size, NvdbPlan& p) {
    p.total = 1;
    for (int k = 0; k < 3; ++k) {
        if (p.nvb_dim[k] < 3) p.nvb_dim[k] = 3;
        p.total *= (long long)p.nvb_dim[k];
    }
    if (p.total > (1ll << 27) || nvdb_size >= (1ll << 32)) {
        return fail(HK_ERR_UNSUPPORTED, "NanoVDB grid too large for the device block table (index bbox > 2^27 blocks or buffer >= 4 GiB)");
    }
    size_t budget_mb = 4096;
    if (const char* e = hk::knob("HK_NVDB_DENSE_MB")) budget_mb = (size_t)std::atol(e);
    p.bricks = (size_t)p.total * 729 * sizeof(float) <= budget_mb * (size_t)(1 << 20);
    return HK_OK;
}
int plan_nanovdb(const hk_medium& m, NvdbPlan& p) {
    if (!m.nvdb_bytes || m.nvdb_size <= 0) return fail(HK_ERR_INVALID, "NanoVDB medium without tree bytes");
    if (!nvdb_block_extent(m, p.background, p.nvb_min, p.nvb_dim)) return fail(HK_ERR_UNSUPPORTED, "NanoVDB grid with a non-background root tile (4096^3 constant region) is not supported");
    if (int e = plan_nanovdb_shape(m.nvdb_size, p)) return e;
    const long long dim[3] = {p.nvb_dim[0], p.nvb_dim[1], p.nvb_dim[2]};
    if (!nvdb_block_table(m, p.nvb_min, dim, p.background, p.table)) return fail(HK_ERR_INVALID, "NanoVDB block table: non-background data on the margin (corrupt tree?)");
    return HK_OK;
}
void NvdbPlan::fill(DMedium& o) const {
    for (int k = 0; k < 3; ++k) o.nvb_min[k] = nvb_min[k], o.nvb_dim[k] = nvb_dim[k];
    o.nv_background = background;
}
namespace {
int upload_nanovdb(hk_scene* s, const hk_medium& m, DMedium& o, hk_scene::Medium& hm) {
    NvdbPlan p;
    if (int e = plan_nanovdb(m, p)) return e;
    DevBuf* nb = hm.nvdb = &s->own();
    HIP_TRY(nb->upload(m.nvdb_bytes, (size_t)m.nvdb_size));
    o.nvdb = nb->as<unsigned char>();
    p.fill(o);
    DevBuf* tb = hm.blocks = &s->own();
    HIP_TRY(tb->upload(p.table.data(), p.table.size() * sizeof(uint2)));
    o.nv_blocks = tb->as<uint2>();
    DevBuf* bb = hm.bricks = &s->own();   // (empty while the bricks do not fit: hk_scene_update_medium sizes it when a later tree's do)
    if (p.bricks) {
        const long long dim[3] = {p.nvb_dim[0], p.nvb_dim[1], p.nvb_dim[2]};
        const std::vector<float> bricks = nvdb_dense_bricks(m, p.table, dim, p.background);
        HIP_TRY(bb->upload(bricks.data(), bricks.size() * sizeof(float)));
        o.nv_bricks = bb->as<float>();
    }
    return HK_OK;
}
}  // namespace
// the part of a DMedium that is no pointer into device memory (hk_scene_update_medium bakes with the same)
void bake_medium_fields(const hk::RGB2Spec& r2s, const hk_medium& m, DMedium& o) {
    o.kind = m.kind;
    o.g = m.g;
    float cf[4];
    bake_unbounded(r2s, m.sigma_a[0], m.sigma_a[1], m.sigma_a[2], cf);
    o.sigma_a = make_float4(cf[0], cf[1], cf[2], cf[3]);
    bake_unbounded(r2s, m.sigma_s[0], m.sigma_s[1], m.sigma_s[2], cf);
    o.sigma_s = make_float4(cf[0], cf[1], cf[2], cf[3]);
    bake_unbounded(r2s, m.Le[0], m.Le[1], m.Le[2], cf);
    o.Le = make_float4(cf[0], cf[1], cf[2], cf[3]);
    std::memcpy(o.bmin, m.bounds_min, 12);
    std::memcpy(o.bmax, m.bounds_max, 12);
    std::memcpy(o.r2m, m.render_to_medium, 48);
    std::memcpy(o.res, m.res, 12);
    std::memcpy(o.mres, m.majorant_res, 12);
    std::memcpy(o.inv_mat, m.inv_mat, 36);
    std::memcpy(o.vec, m.vec, 12);
    o.root_off = m.root_offset_1based;
    o.root_table_size = m.root_table_size;
    if (m.kind == HK_MEDIUM_RGB_GRID) {
        o.sigma_scale = m.sigma_scale;
        o.Le_scale = m.Le_scale;
    }
}
namespace {
int bake_medium(hk_scene* s, const hk::RGB2Spec& r2s, const hk_medium& m, DMedium& o, hk_scene::Medium& hm) {
    bake_medium_fields(r2s, m, o);
    if (m.kind != HK_MEDIUM_HOMOGENEOUS) {
        DevBuf* mb = hm.majorant = &s->own();
        HIP_TRY(mb->upload(m.majorant, (size_t)m.majorant_res[0] * m.majorant_res[1] * m.majorant_res[2] * 4));
        o.majorant = mb->as<float>();
        // one bit per majorant cell: value exactly 0 (DMedium::maj_zero, majorant_skip_zero)
        const size_t ncell = (size_t)m.majorant_res[0] * m.majorant_res[1] * m.majorant_res[2];
        std::vector<uint32_t> zero((ncell + 31) / 32, 0u);
        for (size_t i = 0; i < ncell; ++i)
            if (m.majorant[i] == 0.0f) zero[i >> 5] |= 1u << (i & 31);
        DevBuf* zb = hm.maj_zero = &s->own();
        HIP_TRY(zb->upload(zero.data(), zero.size() * 4));
        o.maj_zero = zb->as<uint32_t>();
    }
    if (m.kind == HK_MEDIUM_GRID) {
        DevBuf* db = hm.density = &s->own();
        HIP_TRY(db->upload(m.density, (size_t)m.res[0] * m.res[1] * m.res[2] * 4));
        o.density = db->as<float>();
    }
    if (m.kind == HK_MEDIUM_RGB_GRID) {
        const size_t nvox = (size_t)m.res[0] * m.res[1] * m.res[2];
        const float* src[3] = {m.sigma_a_grid, m.sigma_s_grid, m.Le_grid};
        const float4** dst[3] = {&o.rgb_a, &o.rgb_s, &o.rgb_Le};
        for (int g = 0; g < 3; ++g) {
            if (!src[g]) continue;
            DevBuf* gb = hm.rgb[g] = &s->own();
            HIP_TRY(gb->upload(src[g], nvox * 16));
            *dst[g] = gb->as<float4>();
        }
    }
    if (m.kind == HK_MEDIUM_NANOVDB) return upload_nanovdb(s, m, o, hm);
    return HK_OK;
}
int upload_media(hk_scene* s, const hk_scene_desc* d, const hk::RGB2Spec& r2s, std::vector<DMedium>& dmed) {
    dmed.resize(d->n_media > 0 ? d->n_media : 1);
    std::memset(dmed.data(), 0, dmed.size() * sizeof(DMedium));
    s->h_media.resize(d->n_media > 0 ? d->n_media : 0);
    for (int i = 0; i < d->n_media; ++i) {
        if (int e = bake_medium(s, r2s, d->media[i], dmed[i], s->h_media[i])) return e;
        s->h_media[i].rec = d->media[i];
        s->h_media[i].d = dmed[i];
    }
    HIP_TRY(s->media.upload(dmed.data(), dmed.size() * sizeof(DMedium)));
    return HK_OK;
}
}  // namespace
// The classes of a scene's media: they select kernel instantiations and size the integrator's path state, so hk_scene_update_medium
// refuses an edit that changes one.
MediaClasses classify_media(const std::vector<DMedium>& dmed, int n_media) {
    MediaClasses D;
    for (int i = 0; i < n_media; ++i) D.media_mask |= 1 << dmed[i].kind;
    D.all_grey = n_media == 1 ? 1 : 0;   // the GREY kernels read ONE medium record
    for (int i = 0; i < n_media; ++i) {
        const DMedium& dm = dmed[i];
        const bool flat_a = dm.sigma_a.w == 0.0f || (dm.sigma_a.x == 0.0f && dm.sigma_a.y == 0.0f);
        const bool flat_s = dm.sigma_s.w == 0.0f || (dm.sigma_s.x == 0.0f && dm.sigma_s.y == 0.0f);
        if (!(flat_a && flat_s && (dm.kind == HK_MEDIUM_GRID || dm.kind == HK_MEDIUM_NANOVDB))) D.all_grey = 0;
    }
    D.grey_pool = (D.all_grey && n_media == 1 && dmed[0].mres[0] <= 1024 && dmed[0].mres[1] <= 1024 && dmed[0].mres[2] <= 1024) ? 1 : 0;
    D.grey_bricks = (D.all_grey && dmed[0].kind == HK_MEDIUM_NANOVDB && dmed[0].nv_bricks != nullptr) ? 1 : 0;
    return D;
}
namespace {

void fill_dscene(hk_scene* s, const hk_scene_desc* d, const BvhUpload& bvh, bool all_opaque, int has_escape, const MediaClasses& mc) {
    DScene& D = s->d;
    D.media = s->media.as<DMedium>();
    D.n_media = d->n_media;
    D.media_mask = mc.media_mask, D.all_grey = mc.all_grey, D.grey_pool = mc.grey_pool, D.grey_bricks = mc.grey_bricks;
    D.nodes = s->nodes.as<DNode>();
    D.qnodes = bvh.have_qnodes ? s->qnodes.as<DQNode>() : nullptr;
    for (int k = 0; k < 3; ++k) D.q_base[k] = bvh.q_base[k], D.q_cell[k] = bvh.q_cell[k];
    D.leaf_tris = s->leaf_tris.as<float4>();
    D.root_ref = bvh.root_ref;
    D.n_tris = d->n_triangles;
    D.n_nodes = s->bvh_nodes;
    D.tri_geo = s->tri_geo;
    D.positions = s->positions.as<float>();
    D.normals = d->normals ? s->normals.as<float>() : nullptr;
    D.uvs = d->uvs ? s->uvs.as<float>() : nullptr;
    D.tangents = d->tangents ? s->tangents.as<float>() : nullptr;
    D.meta = s->meta.as<DTriMeta>();
    D.tri_shade = s->tri_shade.p ? s->tri_shade.as<float>() : nullptr;
    D.materials = s->materials.as<DMaterial>();
    D.textures = s->textures.as<DTexture>();
    D.spectra = s->spectra.as<DPLSpectrum>();
    D.mis = s->mis.as<DMediumInterface>();
    D.lights = s->lights.as<DLight>();
    D.n_lights = d->n_lights;
    D.n_materials = d->n_materials;
    D.lnodes = s->lnodes.as<DLightNode>();
    D.bit_trails = s->trails.as<uint32_t>();
    D.infinite_lights = s->infinite.as<int>();
    D.num_bvh_lights = s->lbvh.num_bvh;
    D.num_infinite_lights = (int)s->lbvh.infinite.size();
    D.envmaps = s->envmaps.as<DEnvMap>();
    D.n_envmaps = d->n_envmaps;
    D.has_escape_lights = has_escape;
    D.simple_lights = (!has_escape && d->n_textures == 0) ? 1 : 0;
    D.all_opaque = all_opaque ? 1 : 0;
    D.bvh_depth = s->bvh_depth;
}
// what the in-place edits need: the material records, the node levels, the base bounds per triangle block of a quantised tree
void note_edit_tables(hk_scene* s, const hk_scene_desc* d, const hk::BVH& bvh, bool have_qnodes) {
    const int T = d->n_triangles;
    s->h_materials.assign(d->materials, d->materials + d->n_materials);
    s->h_lights.assign(d->lights, d->lights + d->n_lights);
    s->n_textures = d->n_textures;
    s->n_spectra = d->n_spectra;
    if (!bvh.nodes.empty()) {   // breadth-first order: a level is a contiguous range (bvh_build.cpp)
        std::vector<int> depth(bvh.nodes.size(), 0);
        s->level_start.push_back(0);
        for (size_t i = 0; i < bvh.nodes.size(); ++i) {
            if (bvh.nodes[i].c0 >= 0) depth[bvh.nodes[i].c0] = depth[i] + 1;
            if (bvh.nodes[i].c1 >= 0) depth[bvh.nodes[i].c1] = depth[i] + 1;
            if (i > 0 && depth[i] != depth[i - 1]) s->level_start.push_back((int)i);
        }
        s->level_start.push_back((int)bvh.nodes.size());
    }
    s->qnodes_built = have_qnodes;
    if (have_qnodes) {
        const int nb = (T + hk_scene::XF_BLOCK - 1) / hk_scene::XF_BLOCK;
        s->block_box.resize(6 * (size_t)nb);
        for (int b = 0; b < nb; ++b) {
            float* bb = s->block_box.data() + 6 * (size_t)b;
            for (int k = 0; k < 3; ++k) bb[k] = INFINITY, bb[3 + k] = -INFINITY;
            for (int t = b * hk_scene::XF_BLOCK; t < std::min(T, (b + 1) * hk_scene::XF_BLOCK); ++t)
                for (int v = 0; v < 9; ++v) {
                    const float x = d->positions[9 * (size_t)t + v];
                    bb[v % 3] = std::min(bb[v % 3], x);
                    bb[3 + v % 3] = std::max(bb[3 + v % 3], x);
                }
        }
    }
    if (T > 0) s->xf[0] = hk_scene::Xf{T, true, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
}
}  // namespace

extern "C" int32_t hk_scene_create(hk_ctx* c, const hk_scene_desc* d, hk_scene** out) {
    if (!c || !d || !out) return fail(HK_ERR_INVALID, "null argument");
    if (!c->have_tables) return fail(HK_ERR_INVALID, "hk_ctx_set_tables must be called first");
    KnobScope knobs(&c->knobs);
    {   // every index the device will follow is checked here: a malformed description is an error, never an out-of-bounds read
        std::string bad = validate_desc(*d);
        if (!bad.empty()) return fail(HK_ERR_INVALID, bad);
    }
    HIP_TRY(hipSetDevice(c->device));
    // the scene is owned by `guard` until it is handed to the caller: every error return below frees what was built so far
    std::unique_ptr<hk_scene> guard(new hk_scene());
    hk_scene* s = guard.get();
    s->ctx = c;
    const SurfaceClasses surf = classify_surfaces(d);
    hk::BVH bvh;
    hk::build_bvh(d->positions, d->n_triangles, bvh, hk::knob_int("HK_BVH_LEAF", 4), hk::knob_int("HK_BVH_BINS", 32));
    BvhUpload bu;
    if (int e = upload_bvh(s, d, surf.mi_opaque, bvh, bu)) return e;
    if (int e = upload_attributes(s, d)) return e;
    if (int e = upload_textures(s, d)) return e;
    if (int e = upload_spectra(s, d)) return e;
    if (int e = upload_materials(s, d, c->r2s_host)) return e;
    if (int e = upload_medium_interfaces(s, d)) return e;
    int has_escape = 0;
    if (int e = upload_lights(s, d, c->r2s_host, has_escape)) return e;
    if (int e = upload_envmaps(s, d)) return e;
    std::vector<DMedium> dmed;
    if (int e = upload_media(s, d, c->r2s_host, dmed)) return e;
    fill_dscene(s, d, bu, surf.all_opaque, has_escape, classify_media(dmed, d->n_media));
    if (s->d.tri_geo) {   // the geometry rows of every triangle, by the function surface_at would call (finished before the scene is handed out)
        hk::launch_tri_geo(c->stream, s->positions.as<float>(), d->n_triangles, s->d.tri_geo, s->tri_shade.p ? s->tri_shade.as<float>() : nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    note_edit_tables(s, d, bvh, bu.have_qnodes);
    *out = guard.release();
    return HK_OK;
}
extern "C" int32_t hk_scene_destroy(hk_scene* s) {
    int status = HK_OK;   // the object goes either way; a device error of a pass that was still noted / in flight is reported (hk_last_error)
    if (s) {
        (void)hipSetDevice(s->ctx->device);
        status = join_lanes(s->ctx);
        if (hipStreamSynchronize(s->ctx->stream) != hipSuccess && status == HK_OK) status = fail(HK_ERR_DEVICE, "hk_scene_destroy: the context's stream reports an error");
        delete s;
    }
    return status;
}
extern "C" int32_t hk_scene_bvh_info(hk_scene* s, int32_t* n_nodes, int32_t* n_leaf_tris, int32_t* max_depth) {
    if (!s) return fail(HK_ERR_INVALID, "null scene");
    if (n_nodes) *n_nodes = s->bvh_nodes;
    if (n_leaf_tris) *n_leaf_tris = s->bvh_leaf_tris;
    if (max_depth) *max_depth = s->bvh_depth;
    return HK_OK;
}
extern "C" int32_t hk_scene_light_bvh_copy(hk_scene* s, int32_t* n_nodes, float* nodes_out, uint32_t* bit_trails) {
    if (!s || !n_nodes) return fail(HK_ERR_INVALID, "null argument");
    *n_nodes = (int32_t)s->lbvh.nodes.size();
    // after hk_scene_refit_lights the bounds live on the device: read them back (this waits for the context's stream) and hand them
    // out in the host order, with the topology words of the tree as built
    std::vector<hk::LightBVHNodeH> refit;
    if (nodes_out && s->lrefit.ready && !s->lbvh.nodes.empty()) {
        hk_ctx* c = s->ctx;
        HIP_TRY(hipSetDevice(c->device));
        std::vector<hk::LightBVHNodeH> raw((size_t)s->lrefit.lay.n_entries);
        HIP_TRY(hipMemcpyAsync(raw.data(), s->lrefit.raw.p, raw.size() * sizeof(hk::LightBVHNodeH), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        refit.resize(s->lbvh.nodes.size());
        for (size_t i = 0; i < refit.size(); ++i) {
            refit[i] = raw[(size_t)s->lrefit.lay.entry_of_host[i]];
            refit[i].bits = (refit[i].bits & 1u) | (s->lbvh.nodes[i].bits & 2u);
            refit[i].child1_or_light = s->lbvh.nodes[i].child1_or_light;
        }
    }
    if (nodes_out)
        for (size_t i = 0; i < s->lbvh.nodes.size(); ++i) {
            const hk::LightBVHNodeH& n = refit.empty() ? s->lbvh.nodes[i] : refit[i];
            float* o = nodes_out + 16 * i;
            std::memcpy(o, n.bmin, 12);
            std::memcpy(o + 3, n.bmax, 12);
            std::memcpy(o + 6, n.w, 12);
            o[9] = n.phi;
            o[10] = n.cos_o;
            o[11] = n.cos_e;
            o[12] = (n.bits & 1u) ? 1.0f : 0.0f;
            o[13] = (float)n.child1_or_light;
            o[14] = (n.bits & 2u) ? 1.0f : 0.0f;
            o[15] = 0.0f;
        }
    if (bit_trails)
        for (size_t i = 0; i < s->lbvh.bit_trails.size(); ++i) bit_trails[i] = s->lbvh.bit_trails[i];
    return HK_OK;
}
