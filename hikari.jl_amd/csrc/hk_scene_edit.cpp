// hk_scene_edit.cpp — in-place scene edits: hk_scene_set_transform (device transform + BVH refit), hk_scene_set_vertices (new base
// geometry of a triangle range in one device pass + BVH refit), hk_scene_update_materials, hk_scene_update_lights (records + host
// rebuild of the light BVH), hk_scene_update_envmap (rotation, texels + device table build), hk_scene_update_envmap_sky (the texels of
// a Hosek-Wilkie sky evaluated on the device; hk_scene_envmap_copy reads a map back) and hk_scene_update_medium (record, volume
// data + device build of majorant grid, zero-cell mask and NanoVDB bricks), hk_scene_update_medium_dense (the NanoVDB tree of a dense
// field and its block table built on the device as well) and hk_scene_rebuild_bvh (a new BVH topology built on the
// device); hk_scene_bvh_cost / hk_scene_bvh_copy / hk_scene_bvh_leaves read the tree back, hk_scene_medium_tree_copy a NanoVDB tree.
#include "hk_host.h"
#include "hk_bvh_decide.h"
#include "hk_light_bounds.h"

// ---- in-place scene edits -----------------------------------------------------------------------------------------------------
// Only hk_scene_rebuild_bvh and hk_scene_update_medium_dense wait for the device, once each and for a small record.  For every
// entry point the noted calls are rendered first (against the scene as it was), the lanes are joined, and the work is enqueued on the context's stream behind everything already there.  Every argument is checked
// before anything changes.  (hk_scene_rebuild_bvh waits once, for the size of the tree it built; it is also the one edit that changes
// bvh_depth and n_nodes — what follows from that is argued at its entry point.)
// Caches keyed by the scene that an edit must not invalidate, and why it does not: DScene::all_opaque and the HK_TRI_OPAQUE bits (opacity
// class of every material and the medium interfaces are unchanged), kinds_mask (a record changes its kind only to or from a Mix of kinds the mask has: check_material_update), simple_lights / has_escape_lights
// (lights and textures unchanged), bvh_depth and n_nodes (topology unchanged), the light BVH (built from the base geometry, Q18),
// the context's noted call (flushed) and lanes (joined); the integrator's path state is sized from those flags only.
// hk_scene_update_lights changes the light set, so it re-derives what is derived from it, through hk_scene_create's own code path
// (hk::derive_light_tables): the host tree hk_scene::lbvh (hk_scene_light_bvh_copy), the node / trail tables and the two counts
// DScene::num_bvh_lights / num_infinite_lights.  What else reads the light set, and why it needs nothing more: has_escape_lights and
// simple_lights depend on the lights' KINDS and on the texture count (both fixed: a changed kind is refused, Le.tex must name a texture
// the scene has), n_lights is fixed; hk::preselect_lights and small_pass_class (k_small_pass's instantiation) compare num_bvh_lights
// with HK_PRESELECT_MIN, but per render call and from the DScene of that call, which is passed to every kernel by value at launch — a
// tree that grows past the threshold is preselected from the next call on, as a fresh scene's would be (the path state carries sel_light
// whenever the scene has no media, whatever the count); k_light_select_pool's LDS copy of the top of the tree is filled per launch from
// num_bvh_lights.  The infinite list is a function of the kinds alone and stays as uploaded.
// hk_scene_update_envmap changes texels, tables and rotation of a map of unchanged size: nothing on the host is derived from those
// (hk_scene_update_envmap_sky: texels and tables only).
// hk_scene_update_medium changes one medium's record and the data behind it; what it leaves valid is said at the entry point below.
namespace {
// the transform of the header's arithmetic: m as given, its normal matrix in double, identity => copy
std::string make_xform(const float* m34, DXform& X) {
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(m34[j])) return "hk_scene_set_transform: non-finite matrix entry";
    std::memcpy(X.m, m34, sizeof X.m);
    static const float id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    X.copy = 1;
    for (int j = 0; j < 12; ++j)
        if (m34[j] != id[j]) X.copy = 0;
    double A[3][3], Cf[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = m34[4 * i + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            Cf[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1];
        }
    const double det = (A[0][0] * Cf[0][0] + A[0][1] * Cf[0][1]) + A[0][2] * Cf[0][2];
    if (!(det != 0.0) || !std::isfinite(det)) return "hk_scene_set_transform: singular matrix";
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            X.nm[3 * i + j] = (float)(Cf[i][j] / det);
            if (!std::isfinite(X.nm[3 * i + j])) return "hk_scene_set_transform: the normal matrix overflows";
        }
    return std::string();
}
// A grid for the quantised nodes that contains every node after the edit, without reading the device: the union over the transform
// intervals of (identity) the base bounds of their triangle blocks, (otherwise) the 8 corners of that box through the point formula in
// double, widened by a bound on the binary32 rounding; then one cell of margin.  false: no finite grid (the float nodes are used).
bool quant_grid(const hk_scene* s, DQGrid& g) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int B = hk_scene::XF_BLOCK;
    for (const auto& kv : s->xf) {
        const int a = kv.first, e = kv.second.end;
        double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int b = a / B; b <= (e - 1) / B; ++b)   // whole blocks: a superset of the interval
            for (int k = 0; k < 3; ++k) blo[k] = std::min(blo[k], (double)s->block_box[6 * (size_t)b + k]), bhi[k] = std::max(bhi[k], (double)s->block_box[6 * (size_t)b + 3 + k]);
        if (kv.second.identity) {
            for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], blo[k]), hi[k] = std::max(hi[k], bhi[k]);
            continue;
        }
        const float* m = kv.second.m;
        for (int k = 0; k < 3; ++k) {
            double mag = std::fabs((double)m[4 * k + 3]);
            for (int j = 0; j < 3; ++j) mag += std::fabs((double)m[4 * k + j]) * std::max(std::fabs(blo[j]), std::fabs(bhi[j]));
            const double err = mag * std::ldexp(1.0, -20);   // >= the rounding of three products and three sums in binary32
            for (int corner = 0; corner < 8; ++corner) {
                double v = m[4 * k + 3];
                for (int j = 0; j < 3; ++j) v += (double)m[4 * k + j] * ((corner >> j) & 1 ? bhi[j] : blo[j]);
                lo[k] = std::min(lo[k], v - err), hi[k] = std::max(hi[k], v + err);
            }
        }
    }
    for (int k = 0; k < 3; ++k) {
        const double cell = (hi[k] - lo[k]) / 65527.0;
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !std::isfinite(cell)) return false;
        const double l = lo[k] - cell, h = hi[k] + cell;   // one cell of margin; then the grid as hk_scene_create lays it over a box
        g.cell[k] = (float)std::max((h - l) / 65527.0, 1e-30);
        g.base[k] = (float)(l - 3.0 * (double)g.cell[k]);
        if (!std::isfinite(g.base[k]) || !std::isfinite(g.cell[k])) return false;
    }
    return true;
}
// the base copies of the geometry and the leaf slot of every triangle (first edit of the geometry only: an unedited scene pays nothing)
int ensure_base(hk_scene* s) {
    if (s->have_base) return HK_OK;
    hk_ctx* c = s->ctx;
    DScene& D = s->d;
    const int T = D.n_tris;
    HIP_TRY(s->base_pos.alloc((size_t)T * 36));
    HIP_TRY(hipMemcpyAsync(s->base_pos.p, D.positions, (size_t)T * 36, hipMemcpyDeviceToDevice, c->stream));
    if (D.normals) {
        HIP_TRY(s->base_nrm.alloc((size_t)T * 36));
        HIP_TRY(hipMemcpyAsync(s->base_nrm.p, D.normals, (size_t)T * 36, hipMemcpyDeviceToDevice, c->stream));
    }
    if (D.tangents) {
        HIP_TRY(s->base_tan.alloc((size_t)T * 36));
        HIP_TRY(hipMemcpyAsync(s->base_tan.p, D.tangents, (size_t)T * 36, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(s->slot_of_prim.alloc((size_t)T * 4));
    hk::launch_slot_of_prim(c->stream, D.leaf_tris, s->bvh_leaf_tris, s->slot_of_prim.as<int>());
    HIP_TRY(hipGetLastError());
    s->have_base = true;
    return HK_OK;
}
// every box of the unchanged topology from D.positions, deepest level first; the quantised copy on a grid that holds the edited tree,
// or the float nodes when none is known to
int refit_levels(hk_ctx* c, const std::vector<int>& level_start, DNode* nodes, DQNode* qn, const DQGrid& grid, const float4* leaf, const float* pos) {
    for (int L = (int)level_start.size() - 2; L >= 0; --L) {   // nothing to do when the root is a leaf
        hk::launch_refit_level(c->stream, level_start[L], level_start[L + 1], nodes, qn, grid, leaf, pos);
        HIP_TRY(hipGetLastError());
    }
    return HK_OK;
}
int refit_tree(hk_scene* s) {
    DScene& D = s->d;
    DQGrid grid{};
    DQNode* qn = nullptr;
    if (s->qnodes_built) {
        if (quant_grid(s, grid)) {
            qn = s->qnodes.as<DQNode>();
            for (int k = 0; k < 3; ++k) D.q_base[k] = grid.base[k], D.q_cell[k] = grid.cell[k];
        }
        D.qnodes = qn;   // null: no grid is known to hold the moved tree, the traversal reads the float nodes (same hits)
    }
    return refit_levels(s->ctx, s->level_start, s->nodes.as<DNode>(), qn, grid, D.leaf_tris, D.positions);
}
}  // namespace

extern "C" int32_t hk_scene_set_transform(hk_scene* s, int32_t first_tri, int32_t n_tris, const float* m34) {
    if (!s || !m34) return fail(HK_ERR_INVALID, "hk_scene_set_transform: null argument");
    const int T = s->d.n_tris;
    if (T <= 0) return fail(HK_ERR_INVALID, "hk_scene_set_transform: the scene has no triangles");
    if (first_tri < 0 || n_tris < 1 || (int64_t)first_tri + n_tris > T) return fail(HK_ERR_INVALID, "hk_scene_set_transform: triangle range outside the scene");
    DXform X{};
    {
        std::string bad = make_xform(m34, X);
        if (!bad.empty()) return fail(HK_ERR_INVALID, bad);
    }
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;   // noted calls render the scene as it was; the lanes finish before the stream rewrites it
    DScene& D = s->d;
    if (int e = ensure_base(s)) return e;
    hk::launch_xform_tris(c->stream, X, first_tri, n_tris, s->base_pos.as<float>(), D.normals ? s->base_nrm.as<float>() : nullptr, D.tangents ? s->base_tan.as<float>() : nullptr,
                          s->slot_of_prim.as<int>(), s->positions.as<float>(), D.normals ? s->normals.as<float>() : nullptr, D.tangents ? s->tangents.as<float>() : nullptr,
                          D.tri_shade ? s->tri_shade.as<float>() : nullptr, tri_geo_rows(s->positions.as<float>(), D.tri_geo), s->leaf_tris.as<float4>());
    HIP_TRY(hipGetLastError());
    {   // the transform of every triangle interval (the quantised grid's bookkeeping)
        const int a = first_tri, e = first_tri + n_tris;
        auto split = [&](int at) {
            if (at >= T) return;
            auto it = std::prev(s->xf.upper_bound(at));
            if (it->first == at) return;
            hk_scene::Xf right = it->second;
            it->second.end = at;
            s->xf[at] = right;
        };
        split(a);
        split(e);
        s->xf.erase(s->xf.lower_bound(a), s->xf.lower_bound(e));
        hk_scene::Xf x{e, X.copy != 0, {}};
        std::memcpy(x.m, m34, sizeof x.m);
        s->xf[a] = x;
    }
    if (int e = refit_tree(s)) return e;
    return HK_OK;
}

namespace {
// a pinned staging buffer whose previous copies have run (at most four; the oldest is waited for only when all four are in flight)
int acquire_staging(hk_scene* s, size_t bytes, hk_scene::Staging*& st) {
    st = nullptr;
    for (auto& b : s->staging)
        if (b.bytes >= bytes && hipEventQuery(b.ev) == hipSuccess) {
            st = &b;
            break;
        }
    if (!st) {
        if (s->staging.size() < 4) {
            s->staging.emplace_back();
            st = &s->staging.back();
            HIP_TRY(hipEventCreateWithFlags(&st->ev, hipEventDisableTiming));
        } else {
            st = &s->staging.front();
            HIP_TRY(hipEventSynchronize(st->ev));
        }
        if (st->bytes < bytes) {
            if (st->host) HIP_TRY(hipHostFree(st->host));
            st->host = nullptr, st->bytes = 0;
            HIP_TRY(hipHostMalloc(&st->host, bytes, hipHostMallocDefault));
            st->bytes = bytes;
        }
    }
    return HK_OK;
}
// what an update may change: everything but the kind, a Mix's children, and the opacity class; indices must stay in range.  The one
// change of kind: a record may BECOME a MixMaterial of two materials of the scene, and a MixMaterial may become a material of a kind
// the scene already shades (hk_scene::kinds_mask: the kinds of the non-Mix records at creation, which never shrinks) — a Mix resolves
// to records of the scene, so neither direction brings a kind the scene's kernels and queues were not chosen for.
std::string check_material_update(const hk_scene* s, int idx, const hk_material& old, const hk_material& m) {
    const std::string at = "hk_scene_update_materials: material " + std::to_string(idx) + ": ";
    if (m.kind != old.kind) {
        if (m.kind == HK_MAT_MIX) {
            if (m.i[0] < 0 || m.i[0] >= s->n_materials || m.i[1] < 0 || m.i[1] >= s->n_materials) return at + "MixMaterial child material index out of range";
        } else if (old.kind != HK_MAT_MIX || m.kind < 0 || m.kind >= 32 || !(s->kinds_mask & (1u << m.kind)))
            return at + "the kind differs from the record it replaces";
    } else if (m.kind == HK_MAT_MIX && (m.i[0] != old.i[0] || m.i[1] != old.i[1] || std::memcmp(m.mix_key, old.mix_key, sizeof m.mix_key) != 0))
        return at + "a MixMaterial's children (i[], mix_key) cannot change";
    for (int k = 0; k < 4; ++k)
        if (m.rgb[k].tex >= s->n_textures) return at + "rgb texture index out of range";
    for (int k = 0; k < 8; ++k)
        if (m.f[k].tex >= s->n_textures) return at + "float texture index out of range";
    if (m.kind == HK_MAT_CONDUCTOR || m.kind == HK_MAT_COATED_CONDUCTOR)
        for (int k = 0; k < 2; ++k)
            if (m.spectrum[k] >= s->n_spectra) return at + "spectrum index out of range";
    if (material_alpha_tested(m) != material_alpha_tested(old)) return at + "the opacity class (Matte alpha texture / alpha < 1) cannot change";
    return std::string();
}
}  // namespace

extern "C" int32_t hk_scene_update_materials(hk_scene* s, int32_t first, int32_t n, const hk_material* materials) {
    if (!s || !materials) return fail(HK_ERR_INVALID, "hk_scene_update_materials: null argument");
    if (first < 0 || n < 1 || (int64_t)first + n > s->n_materials) return fail(HK_ERR_INVALID, "hk_scene_update_materials: material range outside the scene");
    for (int j = 0; j < n; ++j) {
        std::string bad = check_material_update(s, first + j, s->h_materials[first + j], materials[j]);
        if (!bad.empty()) return fail(HK_ERR_INVALID, bad);
    }
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    const size_t bytes = (size_t)n * sizeof(DMaterial);
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, bytes, st)) return e;
    if (int e = join_lanes(c)) return e;   // noted calls render the old materials; the lanes finish before the stream rewrites them
    DMaterial* rec = static_cast<DMaterial*>(st->host);
    for (int j = 0; j < n; ++j) bake_material(c->r2s_host, materials[j], rec[j]);
    HIP_TRY(hipMemcpyAsync(s->materials.as<DMaterial>() + first, rec, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    for (int j = 0; j < n; ++j) s->h_materials[first + j] = materials[j];
    s->d.has_mix = hk::materials_have_kind(s->h_materials.data(), s->h_materials.size(), HK_MAT_MIX);   // which k_trace_lean the next call launches
    s->d.single_kind = hk::single_material_kind(s->kinds_mask, s->d.has_mix, HK_MAX_KINDS);
    return HK_OK;
}

extern "C" int32_t hk_scene_update_lights(hk_scene* s, int32_t first, int32_t n, const hk_light* lights) {
    if (!s || !lights) return fail(HK_ERR_INVALID, "hk_scene_update_lights: null argument");
    const int NL = (int)s->h_lights.size();
    if (first < 0 || n < 1 || (int64_t)first + n > NL) return fail(HK_ERR_INVALID, "hk_scene_update_lights: light range outside the scene");
    for (int j = 0; j < n; ++j) {   // what an update may change: everything but the kind; indices must stay in range (hk_scene_create's checks)
        const hk_light& l = lights[j];
        const std::string at = "hk_scene_update_lights: light " + std::to_string(first + j) + ": ";
        if (l.kind != s->h_lights[first + j].kind) return fail(HK_ERR_INVALID, at + "the kind differs from the record it replaces");
        if (l.kind == HK_LIGHT_ENVIRONMENT && (l.envmap < 0 || l.envmap >= (int)s->h_envmaps.size())) return fail(HK_ERR_INVALID, at + "environment light refers to a missing envmap");
        if (l.kind == HK_LIGHT_DIFFUSE_AREA && l.Le.tex >= s->n_textures) return fail(HK_ERR_INVALID, at + "area light: Le texture index out of range");
    }
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    // the tables of the edited light set, by hk_scene_create's code path; the scene is untouched until everything is enqueued
    std::vector<hk_light> all = s->h_lights;
    std::copy(lights, lights + n, all.begin() + first);
    hk::LightBVH lbvh;
    hk::LightTables t;
    hk::derive_light_tables(all.data(), NL, lbvh, t);
    // one staging block: the n baked records, then the node and trail tables (the capacities of hk_scene_create hold them: LightTables)
    const size_t b_rec = (size_t)n * sizeof(DLight), b_nodes = t.nodes.size() * sizeof(DLightNode), b_trails = t.trails.size() * 4;
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, b_rec + b_nodes + b_trails, st)) return e;
    if (int e = join_lanes(c)) return e;   // noted calls render the old lights; the lanes finish before the stream rewrites them
    char* h = static_cast<char*>(st->host);
    DLight* rec = reinterpret_cast<DLight*>(h);
    std::memset(rec, 0, b_rec);
    for (int j = 0; j < n; ++j) bake_light(c->r2s_host, lights[j], rec[j]);
    std::memcpy(h + b_rec, t.nodes.data(), b_nodes);
    std::memcpy(h + b_rec + b_nodes, t.trails.data(), b_trails);
    HIP_TRY(hipMemcpyAsync(s->lights.as<DLight>() + first, rec, b_rec, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->lnodes.p, h + b_rec, b_nodes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->trails.p, h + b_rec + b_nodes, b_trails, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    s->h_lights.swap(all);
    s->lbvh = std::move(lbvh);
    s->lrefit.ready = false;   // the refit arrays described the tree that was: the next refit fills them from the new one
    s->d.num_bvh_lights = t.num_bvh;
    s->d.num_infinite_lights = t.num_infinite;
    return HK_OK;
}

// ---- hk_scene_refit_lights: new records for a SET of lights, the light BVH refit on the device (the header states the contract) ----
// What the edit leaves valid, beyond what hk_scene_update_lights argues at the head of this file: the topology, so the bit trails, the
// child entries of lnodes, num_bvh_lights, num_infinite_lights and the infinite list — a light may not enter or leave the tree.  The
// readers of lnodes (bvh_sample_light / bvh_pmf of hk_device.h, k_light_select and k_light_select_pool with its LDS copy of the top of
// the tree, k_shade, k_small_pass, hk_test_light_bvh) take every node from the table at launch and hold nothing across calls.
namespace {
// the refit arrays of a scene, from the tree as built (first refit, and the first after a rebuild)
int ensure_light_refit(hk_scene* s) {
    hk_scene::LightRefit& R = s->lrefit;
    if (R.ready) return HK_OK;
    hk_ctx* c = s->ctx;
    hk::light_refit_layout(s->lbvh, R.lay);
    const size_t NL = s->h_lights.size(), cap = light_table_capacity((int)NL), E = (size_t)R.lay.n_entries, n_inner = R.lay.level_entries.size();
    if (E > 2 * cap || n_inner > cap) return fail(HK_ERR_UNSUPPORTED, "hk_scene_refit_lights: the light tree exceeds the scene's capacity");
    if (!R.raw.p) {   // sized by the light count, as lnodes is: a rebuild changes the tree, never the capacity
        HIP_TRY(R.raw.alloc(2 * cap * sizeof(HkLightRaw)));
        HIP_TRY(R.parent.alloc(2 * cap * 4));
        HIP_TRY(R.stamps.alloc(2 * cap * 4));
        HIP_TRY(R.leaf_entry.alloc(cap * 4));
        HIP_TRY(R.level_entries.alloc(cap * 4));
        HIP_TRY(R.stage.alloc(cap * (sizeof(DLight) + sizeof(HkLightRaw) + sizeof(int2))));   // the largest edit: no call ever grows it (growing would wait for the device)
    }
    const size_t b_raw = E * sizeof(HkLightRaw), b_par = E * 4, b_leaf = NL * 4, b_lev = n_inner * 4;
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, b_raw + b_par + b_leaf + b_lev + 16, st)) return e;
    char* h = static_cast<char*>(st->host);
    std::memset(h, 0, b_raw);
    for (size_t e = 0; e < E; ++e)
        if (R.lay.host_of_entry[e] >= 0) std::memcpy(h + e * sizeof(HkLightRaw), &s->lbvh.nodes[(size_t)R.lay.host_of_entry[e]], sizeof(HkLightRaw));
    std::memcpy(h + b_raw, R.lay.parent.data(), b_par);
    std::memcpy(h + b_raw + b_par, R.lay.leaf_entry.data(), b_leaf);
    std::memcpy(h + b_raw + b_par + b_leaf, R.lay.level_entries.data(), b_lev);
    if (b_raw) HIP_TRY(hipMemcpyAsync(R.raw.p, h, b_raw, hipMemcpyHostToDevice, c->stream));
    if (b_par) HIP_TRY(hipMemcpyAsync(R.parent.p, h + b_raw, b_par, hipMemcpyHostToDevice, c->stream));
    if (b_leaf) HIP_TRY(hipMemcpyAsync(R.leaf_entry.p, h + b_raw + b_par, b_leaf, hipMemcpyHostToDevice, c->stream));
    if (b_lev) HIP_TRY(hipMemcpyAsync(R.level_entries.p, h + b_raw + b_par + b_leaf, b_lev, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(R.stamps.p, 0, 2 * cap * 4, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    R.stamp = 0;
    R.ready = true;
    return HK_OK;
}
bool floats_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}
}  // namespace

extern "C" int32_t hk_scene_refit_lights(hk_scene* s, int32_t n, const int32_t* index, const hk_light* lights) {
    static_assert(sizeof(HkLightRaw) == sizeof(hk::LightBVHNodeH), "a raw node is the builder's node");
    if (!s || !index || !lights) return fail(HK_ERR_INVALID, "hk_scene_refit_lights: null argument");
    const int NL = (int)s->h_lights.size();
    if (n < 1 || n > NL) return fail(HK_ERR_INVALID, "hk_scene_refit_lights: the number of lights is outside the scene");
    std::vector<char> seen((size_t)NL, 0);
    std::vector<hk::LightBVHNodeH> leaves;
    std::vector<int2> slot((size_t)n);
    for (int j = 0; j < n; ++j) {   // hk_scene_update_lights' checks, and what keeps the topology valid
        const int idx = index[j];
        auto at = [idx]() { return "hk_scene_refit_lights: light " + std::to_string(idx) + ": "; };   // (built only for a refusal)
        if (idx < 0 || idx >= NL) return fail(HK_ERR_INVALID, at() + "index outside the scene");
        if (seen[(size_t)idx]) return fail(HK_ERR_INVALID, at() + "the index is given twice");
        seen[(size_t)idx] = 1;
        const hk_light& l = lights[j];
        if (l.kind != s->h_lights[(size_t)idx].kind) return fail(HK_ERR_INVALID, at() + "the kind differs from the record it replaces");
        if (l.kind == HK_LIGHT_ENVIRONMENT && (l.envmap < 0 || l.envmap >= (int)s->h_envmaps.size())) return fail(HK_ERR_INVALID, at() + "environment light refers to a missing envmap");
        if (l.kind == HK_LIGHT_DIFFUSE_AREA && l.Le.tex >= s->n_textures) return fail(HK_ERR_INVALID, at() + "area light: Le texture index out of range");
        if ((l.kind == HK_LIGHT_POINT || l.kind == HK_LIGHT_SPOT) && !floats_finite(l.position, 3)) return fail(HK_ERR_INVALID, at() + "non-finite position");
        if (l.kind == HK_LIGHT_DIFFUSE_AREA && !(floats_finite(l.v, 9) && floats_finite(l.normal, 3) && std::isfinite(l.area))) return fail(HK_ERR_INVALID, at() + "non-finite vertex, normal or area");
        hk::LightBVHNodeH leaf;
        const bool in_tree = hk::light_leaf(l, idx + 1, leaf) == 2, was = s->lbvh.bit_trails[(size_t)idx] != 0xFFFFFFFFu;
        if (in_tree != was)
            return fail(HK_ERR_INVALID, at() + (in_tree ? "the light would enter the light tree" : "the light would leave the light tree") +
                                            " (bounded lights of positive power are in it): a refit keeps the topology, send this edit with hk_scene_update_lights");
        slot[(size_t)j] = make_int2(idx, in_tree ? (int)leaves.size() : -1);
        if (in_tree) {
            if (!(floats_finite(leaf.bmin, 3) && floats_finite(leaf.bmax, 3) && floats_finite(leaf.w, 3) && std::isfinite(leaf.phi) && std::isfinite(leaf.cos_o) && std::isfinite(leaf.cos_e)))
                return fail(HK_ERR_INVALID, at() + "non-finite light bounds (direction, cone or power)");
            leaves.push_back(leaf);
        }
    }
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    hk_scene::LightRefit& R = s->lrefit;
    // one staging block, proportional to the edit: the n baked records, the raw leaves, the slots
    const size_t b_rec = (size_t)n * sizeof(DLight), b_leaf = leaves.size() * sizeof(HkLightRaw), b_slot = (size_t)n * sizeof(int2), total = b_rec + b_leaf + b_slot;
    if (int e = ensure_light_refit(s)) return e;                // new arrays only: the scene's tables are as they were
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, total, st)) return e;
    if (int e = join_lanes(c)) return e;   // noted calls render the old lights; the lanes finish before the stream rewrites them
    char* h = static_cast<char*>(st->host);
    DLight* rec = reinterpret_cast<DLight*>(h);
    std::memset(rec, 0, b_rec);
    for (int j = 0; j < n; ++j) bake_light(c->r2s_host, lights[j], rec[j]);
    if (b_leaf) std::memcpy(h + b_rec, leaves.data(), b_leaf);
    std::memcpy(h + b_rec + b_leaf, slot.data(), b_slot);
    char* dv = R.stage.as<char>();
    HIP_TRY(hipMemcpyAsync(dv, h, total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    if (++R.stamp == 0) {   // the stamps have gone round: none may look like this call's
        HIP_TRY(hipMemsetAsync(R.stamps.p, 0, R.stamps.bytes, c->stream));
        R.stamp = 1;
    }
    DLightRefit A{};
    A.n = n, A.stamp = R.stamp;
    A.rec = reinterpret_cast<const uint4*>(dv);
    A.leaf = reinterpret_cast<const HkLightRaw*>(dv + b_rec);
    A.slot = reinterpret_cast<const int2*>(dv + b_rec + b_leaf);
    A.lights = s->lights.as<DLight>();
    A.raw = R.raw.as<HkLightRaw>();
    A.lnodes = s->lnodes.as<DLightNode>();
    A.parent = R.parent.as<int>(), A.leaf_entry = R.leaf_entry.as<int>(), A.stamps = R.stamps.as<uint32_t>();
    hk::launch_light_refit_leaves(c->stream, A);
    HIP_TRY(hipGetLastError());
    if (!leaves.empty())
        for (int d = (int)R.lay.level_start.size() - 2; d >= 0; --d) {   // nothing to do when the root is a leaf
            const int begin = R.lay.level_start[(size_t)d], count = R.lay.level_start[(size_t)d + 1] - begin;
            hk::launch_light_refit_level(c->stream, R.level_entries.as<int>() + begin, count, A);
            HIP_TRY(hipGetLastError());
        }
    for (int j = 0; j < n; ++j) s->h_lights[(size_t)index[j]] = lights[j];
    return HK_OK;
}

extern "C" int32_t hk_scene_update_envmap(hk_scene* s, int32_t idx, const float* data, const float* rotation) {
    if (!s) return fail(HK_ERR_INVALID, "hk_scene_update_envmap: null scene");
    if (!data && !rotation) return fail(HK_ERR_INVALID, "hk_scene_update_envmap: neither texels nor a rotation given");
    if (idx < 0 || idx >= (int)s->h_envmaps.size()) return fail(HK_ERR_INVALID, "hk_scene_update_envmap: map index out of range");
    if (rotation)
        for (int j = 0; j < 9; ++j)
            if (!std::isfinite(rotation[j])) return fail(HK_ERR_INVALID, "hk_scene_update_envmap: non-finite rotation entry");
    DEnvMap& e = s->h_envmaps[idx];
    if (data && (e.nu != e.width || e.nv != e.height)) return fail(HK_ERR_INVALID, "hk_scene_update_envmap: the map's tables are not of its texels' resolution (nu != width or nv != height)");
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    const size_t b_rot = 9 * sizeof(float), b_data = data ? (size_t)e.width * e.height * 16 : 0;
    hk_scene::Staging* st = nullptr;
    if (int err = acquire_staging(s, b_rot + b_data, st)) return err;
    if (int err = join_lanes(c)) return err;   // noted calls render the old sky; the lanes finish before the stream rewrites it
    char* h = static_cast<char*>(st->host);
    DEnvMap* record = s->envmaps.as<DEnvMap>() + idx;
    if (rotation) {   // the nine floats of the record and nothing else (marg_func_int lives there too, and only the device knows it)
        std::memcpy(h, rotation, b_rot);
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(record) + offsetof(DEnvMap, rot), h, b_rot, hipMemcpyHostToDevice, c->stream));
        std::memcpy(e.rot, rotation, b_rot);
    }
    if (data) {   // the texels into their buffer, the tables from them into theirs (sizes unchanged)
        std::memcpy(h + b_rot, data, b_data);
        HIP_TRY(hipMemcpyAsync(const_cast<float4*>(e.data), h + b_rot, b_data, hipMemcpyHostToDevice, c->stream));
        hk::launch_envmap_tables(c->stream, e, record);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    return HK_OK;
}

// The texels of map `idx` from a sky record, on the device (k_sky_texels), then the tables from them as above.  The record is a kernel
// argument, so nothing is staged and nothing of the caller's is read after the call returns.
extern "C" int32_t hk_scene_update_envmap_sky(hk_scene* s, int32_t idx, const hk_sky_params* sky) {
    if (!sky) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: null params");
    if (!s) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: null scene");
    if (idx < 0 || idx >= (int)s->h_envmaps.size()) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: map index out of range");
    const DEnvMap& e = s->h_envmaps[idx];
    if (e.width != e.height) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: the map is not square");
    if (e.nu != e.width || e.nv != e.height) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: the map's tables are not of its texels' resolution (nu != width or nv != height)");
    if (sky->reserved != 0) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: reserved is not 0");
    bool finite = true;
    for (int j = 0; j < 3; ++j) finite = finite && std::isfinite(sky->sun_dir[j]) && std::isfinite(sky->ground_rgb[j]);
    const double* d = &sky->config[0][0];
    for (int j = 0; j < 11 * 9; ++j) finite = finite && std::isfinite(d[j]);
    for (int j = 0; j < 11; ++j) finite = finite && std::isfinite(sky->radiance[j]);
    d = &sky->xyz_weight[0][0];
    for (int j = 0; j < 3 * 13; ++j) finite = finite && std::isfinite(d[j]);
    if (!finite) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: non-finite entry in the record");
    const double len2 = ((double)sky->sun_dir[0] * sky->sun_dir[0] + (double)sky->sun_dir[1] * sky->sun_dir[1]) + (double)sky->sun_dir[2] * sky->sun_dir[2];
    if (!(len2 >= 1.0 - 1e-3 && len2 <= 1.0 + 1e-3)) return fail(HK_ERR_INVALID, "hk_scene_update_envmap_sky: sun_dir is not a unit vector (squared length outside 1 +- 1e-3)");
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int err = join_lanes(c)) return err;   // noted calls render the old sky; the lanes finish before the stream rewrites it
    hk::launch_sky_texels(c->stream, *sky, e.width, const_cast<float4*>(e.data));
    hk::launch_envmap_tables(c->stream, e, s->envmaps.as<DEnvMap>() + idx);
    HIP_TRY(hipGetLastError());
    return HK_OK;
}

extern "C" int32_t hk_scene_envmap_copy(hk_scene* s, int32_t idx, int32_t* width, int32_t* height, float* texels, float* conditional_func, float* conditional_cdf, float* marginal_func,
                                        float* marginal_cdf, float* marginal_func_int) {
    if (!s) return fail(HK_ERR_INVALID, "hk_scene_envmap_copy: null scene");
    if (idx < 0 || idx >= (int)s->h_envmaps.size()) return fail(HK_ERR_INVALID, "hk_scene_envmap_copy: map index out of range");
    const DEnvMap& e = s->h_envmaps[idx];
    if ((conditional_func || conditional_cdf || marginal_func || marginal_cdf) && (e.nu != e.width || e.nv != e.height))   // a caller sizes its buffers from width and height
        return fail(HK_ERR_INVALID, "hk_scene_envmap_copy: the map's tables are not of its texels' resolution (nu != width or nv != height): only sizes, texels and marginal_func_int can be read");
    if (width) *width = e.width;
    if (height) *height = e.height;
    if (!texels && !conditional_func && !conditional_cdf && !marginal_func && !marginal_cdf && !marginal_func_int) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int err = join_lanes(c)) return err;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t nu = (size_t)e.nu, nv = (size_t)e.nv;
    if (texels) HIP_TRY(hipMemcpy(texels, e.data, (size_t)e.width * e.height * 16, hipMemcpyDeviceToHost));
    if (conditional_func) HIP_TRY(hipMemcpy(conditional_func, e.cond_func, nu * nv * 4, hipMemcpyDeviceToHost));
    if (conditional_cdf) HIP_TRY(hipMemcpy(conditional_cdf, e.cond_cdf, (nu + 1) * nv * 4, hipMemcpyDeviceToHost));
    if (marginal_func) HIP_TRY(hipMemcpy(marginal_func, e.marg_func, nv * 4, hipMemcpyDeviceToHost));
    if (marginal_cdf) HIP_TRY(hipMemcpy(marginal_cdf, e.marg_cdf, (nv + 1) * 4, hipMemcpyDeviceToHost));
    if (marginal_func_int)   // the device record's own copy: only the device knows it after a table build
        HIP_TRY(hipMemcpy(marginal_func_int, reinterpret_cast<const char*>(s->envmaps.as<DEnvMap>() + idx) + offsetof(DEnvMap, marg_func_int), 4, hipMemcpyDeviceToHost));
    return HK_OK;
}

namespace {
bool all_finite(const float* p, int n) {
    for (int j = 0; j < n; ++j)
        if (!std::isfinite(p[j])) return false;
    return true;
}
// what an update may change: everything but the kind, the voxel and majorant resolutions and which RGB grids there are
std::string check_medium_update(const hk_medium& old, const hk_medium& m) {
    if (m.kind != old.kind) return "the kind differs from the record it replaces";
    std::string bad = check_medium_record(m);   // hk_scene_create's own check of a record
    if (!bad.empty()) return bad;
    if (!all_finite(&m.g, 1)) return "non-finite g";
    if (m.kind == HK_MEDIUM_HOMOGENEOUS) return std::string();
    if (!all_finite(m.bounds_min, 3) || !all_finite(m.bounds_max, 3)) return "non-finite bounds";
    if (!all_finite(m.render_to_medium, 16) || !all_finite(m.medium_to_render, 16)) return "non-finite transform";
    if (std::memcmp(m.majorant_res, old.majorant_res, sizeof m.majorant_res) != 0) return "majorant_res cannot change";
    if (m.kind == HK_MEDIUM_NANOVDB) {
        if (!all_finite(m.inv_mat, 9) || !all_finite(m.vec, 3)) return "non-finite inv_mat / vec";
        return std::string();
    }
    if (std::memcmp(m.res, old.res, sizeof m.res) != 0) return "res cannot change";
    if (m.kind == HK_MEDIUM_GRID) return m.density ? std::string() : std::string("GridMedium without density");
    if (!all_finite(&m.sigma_scale, 1) || !all_finite(&m.Le_scale, 1)) return "non-finite sigma_scale / Le_scale";
    if (!m.sigma_a_grid != !old.sigma_a_grid || !m.sigma_s_grid != !old.sigma_s_grid || !m.Le_grid != !old.Le_grid)
        return "an RGB grid cannot appear or disappear (sigma_a_grid / sigma_s_grid / Le_grid)";
    return std::string();
}
void swap_buffers(DevBuf& a, DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.slab_dev, b.slab_dev);
}
size_t staged(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // every block of a staging buffer starts on a 256-byte boundary
// the classes of the scene with `o` as medium idx, by hk_scene_create's code: empty, or the refusal of an edit that would change one
std::string media_class_refusal(const hk_scene* s, int idx, const DMedium& o) {
    const int NM = (int)s->h_media.size();
    std::vector<DMedium> all(NM);
    for (int i = 0; i < NM; ++i) all[i] = s->h_media[i].d;
    all[idx] = o;
    const MediaClasses mc = classify_media(all, NM);
    const DScene& D = s->d;
    if (mc.media_mask == D.media_mask && mc.all_grey == D.all_grey && mc.grey_pool == D.grey_pool && mc.grey_bricks == D.grey_bricks) return std::string();
    return mc.grey_bricks != D.grey_bricks ? "the class of the scene's media would change (halo bricks against HK_NVDB_DENSE_MB: grey_bricks)"
                                           : "the class of the scene's media would change (a grey medium turning coloured or the reverse: all_grey / grey_pool)";
}
// a tree that needs more than the NanoVDB buffers hold (tree bytes, block table, bricks) gets new ones: all are allocated before any is
// exchanged, and the stream is waited for before the old ones go (passes already enqueued read them)
int fit_nanovdb_buffers(hk_ctx* c, hk_scene::Medium& hm, const size_t need[3]) {
    DevBuf fresh[3];
    DevBuf* const have[3] = {hm.nvdb, hm.blocks, hm.bricks};
    bool grow = false;
    for (int k = 0; k < 3; ++k)
        if (have[k]->bytes < need[k]) {
            HIP_TRY(fresh[k].alloc(need[k]));
            grow = true;
        }
    if (grow) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; ++k)
            if (fresh[k].p) swap_buffers(*have[k], fresh[k]);
    }
    return HK_OK;
}
}  // namespace

// Medium `idx` becomes *mp.  What this leaves valid, and why: the view cache (hk_render.cpp) is off in scenes with media, so no camera
// record outlives the edit; the medium the camera sits in is found on the device in every pass (k_detect_camera_medium), from the
// record of that pass; DScene — the media pointer, n_media and the four classes — is passed to every kernel by value at launch and is
// not touched: the record array keeps its place, and an edit that would change media_mask / all_grey / grey_pool / grey_bricks (they
// select kernel instantiations and size the path state: classify_media) is refused, as hk_scene_update_materials refuses a change of
// opacity class.  Everything derived from the volume data — majorant grid, zero-cell mask, halo bricks — is rebuilt from it on the
// device, to the bits hk_scene_create would be handed or build; the block table is hk_scene_create's host build, uploaded.
extern "C" int32_t hk_scene_update_medium(hk_scene* s, int32_t idx, const hk_medium* mp) {
    if (!s || !mp) return fail(HK_ERR_INVALID, "hk_scene_update_medium: null argument");
    const int NM = (int)s->h_media.size();
    if (idx < 0 || idx >= NM) return fail(HK_ERR_INVALID, "hk_scene_update_medium: medium index out of range");
    const hk_medium& m = *mp;
    hk_scene::Medium& hm = s->h_media[idx];
    const std::string at = "hk_scene_update_medium: medium " + std::to_string(idx) + ": ";
    {
        std::string bad = check_medium_update(hm.rec, m);
        if (!bad.empty()) return fail(HK_ERR_INVALID, at + bad);
    }
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    DMedium o = hm.d;   // the pointers stay (a NanoVDB tree's are set below), everything else is baked as hk_scene_create bakes it
    bake_medium_fields(c->r2s_host, m, o);
    NvdbPlan plan;
    if (m.kind == HK_MEDIUM_NANOVDB) {
        if (plan_nanovdb(m, plan) != HK_OK) return fail(HK_ERR_INVALID, at + g_err);
        for (const uint2& e : plan.table)   // a leaf the kernels below (and the tracking kernels) read lies inside the bytes given
            if (e.x != 0u && (long long)e.x - 1 + 96 + 2048 > (long long)m.nvdb_size) return fail(HK_ERR_INVALID, at + "NanoVDB block table: a leaf lies outside nvdb_size (corrupt tree?)");
        plan.fill(o);
        o.nv_bricks = plan.bricks ? reinterpret_cast<const float*>(&plan) : nullptr;   // (for the class check; the buffer's address follows)
    }
    {
        std::string bad = media_class_refusal(s, idx, o);
        if (!bad.empty()) return fail(HK_ERR_INVALID, at + bad);
    }
    // one staging block: the record, then the data that crosses to the device (voxel grids, or tree bytes and block table)
    const size_t nvox = (size_t)m.res[0] * m.res[1] * m.res[2];
    const float* rgb_src[3] = {m.sigma_a_grid, m.sigma_s_grid, m.Le_grid};
    const size_t b_tree = m.kind == HK_MEDIUM_NANOVDB ? (size_t)m.nvdb_size : 0, b_table = plan.table.size() * sizeof(uint2), b_bricks = plan.bricks ? (size_t)plan.total * 729 * sizeof(float) : 0;
    size_t total = staged(sizeof(DMedium));
    if (m.kind == HK_MEDIUM_GRID) total += staged(nvox * 4);
    if (m.kind == HK_MEDIUM_RGB_GRID)
        for (int g = 0; g < 3; ++g) total += rgb_src[g] ? staged(nvox * 16) : 0;
    if (m.kind == HK_MEDIUM_NANOVDB) total += staged(b_tree) + staged(b_table);
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, total, st)) return e;
    if (int e = join_lanes(c)) return e;   // noted calls render the old medium; the lanes finish before the stream rewrites it
    if (m.kind == HK_MEDIUM_NANOVDB) {
        const size_t need[3] = {b_tree, b_table, b_bricks};
        if (int e = fit_nanovdb_buffers(c, hm, need)) return e;
        o.nvdb = hm.nvdb->as<unsigned char>();
        o.nv_blocks = hm.blocks->as<uint2>();
        o.nv_bricks = plan.bricks ? hm.bricks->as<float>() : nullptr;
    }
    char* h = static_cast<char*>(st->host);
    size_t off = staged(sizeof(DMedium));
    auto upload = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        std::memcpy(h + off, src, bytes);
        const hipError_t e = hipMemcpyAsync(dst, h + off, bytes, hipMemcpyHostToDevice, c->stream);
        off += staged(bytes);
        return e;
    };
    if (m.kind == HK_MEDIUM_GRID) HIP_TRY(upload(hm.density->p, m.density, nvox * 4));
    if (m.kind == HK_MEDIUM_RGB_GRID)
        for (int g = 0; g < 3; ++g)
            if (rgb_src[g]) HIP_TRY(upload(hm.rgb[g]->p, rgb_src[g], nvox * 16));
    if (m.kind == HK_MEDIUM_NANOVDB) {
        HIP_TRY(upload(hm.nvdb->p, m.nvdb_bytes, b_tree));
        HIP_TRY(upload(hm.blocks->p, plan.table.data(), b_table));
    }
    // the tables derived from the data, behind its copies; then the record that points to them
    if (m.kind == HK_MEDIUM_GRID || m.kind == HK_MEDIUM_RGB_GRID) hk::launch_majorant_grid(c->stream, o);
    if (m.kind == HK_MEDIUM_NANOVDB) {
        DIndexBox ib;
        for (int k = 0; k < 3; ++k) ib.lo[k] = m.index_bbox_min[k], ib.hi[k] = m.index_bbox_max[k];
        hk::launch_majorant_nanovdb(c->stream, o, ib);
        if (plan.bricks) hk::launch_nvdb_bricks(c->stream, o, (size_t)plan.total);
    }
    HIP_TRY(hipGetLastError());
    std::memcpy(h, &o, sizeof o);
    HIP_TRY(hipMemcpyAsync(s->media.as<DMedium>() + idx, h, sizeof o, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    hm.rec = m;
    hm.d = o;
    return HK_OK;
}

// NanoVDB medium `idx` becomes the tree of a dense field, built on the device (hk_nvdb_build.h).  The scene is left as
// hk_scene_update_medium leaves it for the host-built tree of the same field, and what that call leaves valid stays valid for the same
// reasons.  Everything before the one wait writes the scene's working buffers only; every refusal comes before the first write to a
// buffer a record points to, so a refused call leaves the scene as it was.  hk_scene::Medium::rec gets no pointer to tree bytes: there
// are none on the host (its pointers are never followed — check_medium_update and hk_scene_medium_tree_copy read its plain fields).
extern "C" int32_t hk_scene_update_medium_dense(hk_scene* s, int32_t idx, const hk_medium* mp, const hk_dense_field* fp) {
    if (!s || !mp || !fp || !fp->data) return fail(HK_ERR_INVALID, "hk_scene_update_medium_dense: null argument");
    const int NM = (int)s->h_media.size();
    if (idx < 0 || idx >= NM) return fail(HK_ERR_INVALID, "hk_scene_update_medium_dense: medium index out of range");
    hk_scene::Medium& hm = s->h_media[idx];
    const hk_dense_field& F = *fp;
    const std::string at = "hk_scene_update_medium_dense: medium " + std::to_string(idx) + ": ";
    if (hm.rec.kind != HK_MEDIUM_NANOVDB) return fail(HK_ERR_INVALID, at + "not a NanoVDB medium");
    if (F.res[0] < 1 || F.res[1] < 1 || F.res[2] < 1) return fail(HK_ERR_INVALID, at + "res below 1");
    if (F.layout != HK_DENSE_X_FASTEST && F.layout != HK_DENSE_Z_FASTEST) return fail(HK_ERR_INVALID, at + "unknown layout");
    hk_medium m = *mp;   // the record hk_scene_update_medium would be given: the map as build_nanovdb_from_dense derives it, in binary32
    std::memset(m.inv_mat, 0, sizeof m.inv_mat);
    for (int k = 0; k < 3; ++k) {
        const float d = (m.bounds_max[k] - m.bounds_min[k]) / (float)F.res[k];
        m.inv_mat[4 * k] = 1.0f / d;
        m.vec[k] = m.bounds_min[k] + d / 2.0f;
    }
    m.nvdb_bytes = nullptr, m.majorant = nullptr, m.max_density = 0.0f;
    {
        std::string bad = check_medium_update(hm.rec, m);
        if (!bad.empty()) return fail(HK_ERR_INVALID, at + bad);
    }
    // the three levels over the field's extent: 8^3 blocks, lower nodes of 16^3 blocks, upper nodes of 32^3 lower nodes
    DDense D{};
    long long n_lev[3];
    for (int k = 0; k < 3; ++k) {
        D.res[k] = F.res[k];
        D.lev[0].dim[k] = (int)(((long long)F.res[k] + 7) / 8);
        D.lev[1].dim[k] = (D.lev[0].dim[k] + 15) / 16;
        D.lev[2].dim[k] = (D.lev[1].dim[k] + 31) / 32;
    }
    for (int L = 0; L < 3; ++L) n_lev[L] = (long long)D.lev[L].dim[0] * D.lev[L].dim[1] * D.lev[L].dim[2];
    if (n_lev[0] > (1ll << 27)) return fail(HK_ERR_INVALID, at + "a field of more than 2^27 blocks of 8^3 voxels");
    const size_t nx = (size_t)F.res[0], ny = (size_t)F.res[1], b_field = nx * ny * (size_t)F.res[2] * sizeof(float);
    D.fast = F.layout == HK_DENSE_X_FASTEST ? 0 : 2;
    if (D.fast == 0) D.stride[0] = 1, D.stride[1] = (long long)nx, D.stride[2] = (long long)(nx * ny);
    else D.stride[0] = (long long)(ny * (size_t)F.res[2]), D.stride[1] = F.res[2], D.stride[2] = 1;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    // the working set: control record, then per level flags, slots, list and tile sums
    size_t work = staged(sizeof(DDenseCtl)), o_flags[3], o_slot[3], o_list[3], o_sums[3];
    for (int L = 0; L < 3; ++L) {
        DDenseLevel& V = D.lev[L];
        V.n = (uint32_t)n_lev[L];
        V.tiles = (V.n + (uint32_t)HK_DENSE_SCAN_TILE - 1u) / (uint32_t)HK_DENSE_SCAN_TILE;
        o_flags[L] = work, work += staged(V.n);
        o_slot[L] = work, work += staged((size_t)V.n * 4);
        o_list[L] = work, work += staged((size_t)V.n * 4);
        o_sums[L] = work, work += staged((size_t)V.tiles * 4);
    }
    if (s->dense_work.bytes < work) HIP_TRY(s->dense_work.alloc(work));
    if (!F.on_device && s->dense_field.bytes < b_field) HIP_TRY(s->dense_field.alloc(b_field));
    char* wk = s->dense_work.as<char>();
    D.ctl = reinterpret_cast<DDenseCtl*>(wk);
    for (int L = 0; L < 3; ++L) {
        D.lev[L].flags = reinterpret_cast<unsigned char*>(wk + o_flags[L]);
        D.lev[L].slot = reinterpret_cast<uint32_t*>(wk + o_slot[L]);
        D.lev[L].list = reinterpret_cast<uint32_t*>(wk + o_list[L]);
        D.lev[L].sums = reinterpret_cast<uint32_t*>(wk + o_sums[L]);
    }
    // one staging block: the record, the control record coming back, then a host field on its way to the device
    const size_t o_ctl = staged(sizeof(DMedium)), o_field = o_ctl + staged(sizeof(DDenseCtl));
    hk_scene::Staging* st = nullptr;
    if (int e = acquire_staging(s, o_field + (F.on_device ? 0 : staged(b_field)), st)) return e;
    if (int e = join_lanes(c)) return e;   // noted calls render the old medium; the lanes finish before the stream rewrites it
    char* h = static_cast<char*>(st->host);
    D.data = F.data;
    if (!F.on_device) {
        std::memcpy(h + o_field, F.data, b_field);
        HIP_TRY(hipMemcpyAsync(s->dense_field.p, h + o_field, b_field, hipMemcpyHostToDevice, c->stream));
        D.data = s->dense_field.as<float>();
    }
    hk::launch_dense_count(c->stream, D);
    HIP_TRY(hipGetLastError());
    // the one wait: node counts, the leaves' bounds and the non-finite flag
    DDenseCtl& ctl = *reinterpret_cast<DDenseCtl*>(h + o_ctl);
    HIP_TRY(hipMemcpyAsync(&ctl, D.ctl, sizeof ctl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ctl.nonfinite) return fail(HK_ERR_INVALID, at + "non-finite voxel");
    for (int L = 0; L < 3; ++L)
        if ((long long)ctl.count[L] > n_lev[L] || (ctl.count[L] == 0u) != (ctl.count[0] == 0u))
            return fail(HK_ERR_DEVICE, at + "the device builder reported inconsistent node counts (the scene is unchanged)");
    // the tree's sections as build_nanovdb_from_dense lays them out, and the record of such a tree
    const long long n_leaf = ctl.count[0], n_lower = ctl.count[1], n_upper = ctl.count[2];
    D.section[2] = hknv::ROOT_HEADER + n_upper * hknv::ROOT_TILE;
    D.section[1] = D.section[2] + n_upper * hknv::UPPER_SIZE;
    D.section[0] = D.section[1] + n_lower * hknv::LOWER_SIZE;
    m.nvdb_size = D.section[0] + n_leaf * hknv::LEAF_SIZE;
    m.root_offset_1based = 1, m.upper_offset_1based = D.section[2] + 1, m.lower_offset_1based = D.section[1] + 1;
    m.leaf_offset_1based = n_leaf ? D.section[0] + 1 : 1;
    m.upper_count = (int)n_upper, m.lower_count = (int)n_lower, m.leaf_count = (int)n_leaf, m.root_table_size = (int)n_upper;
    NvdbPlan plan;
    for (int k = 0; k < 3; ++k) {
        m.index_bbox_min[k] = D.index_min[k] = n_leaf ? (0x7fffffff - ctl.lo_enc[k]) * 8 : 0;
        m.index_bbox_max[k] = D.index_max[k] = n_leaf ? ctl.hi1[k] * 8 : 0;   // the largest leaf origin + 8
        // nvdb_block_extent of this tree: its leaves lie inside the index bounding box, every tile holds the background
        const int lo = m.index_bbox_min[k] >> 3, hi = m.index_bbox_max[k] >> 3;
        plan.nvb_min[k] = lo - 1, plan.nvb_dim[k] = hi - lo + 3;
    }
    plan.background = 0.0f;
    if (plan_nanovdb_shape(m.nvdb_size, plan) != HK_OK) return fail(HK_ERR_INVALID, at + g_err);
    DMedium o = hm.d;
    bake_medium_fields(c->r2s_host, m, o);
    plan.fill(o);
    o.nv_bricks = plan.bricks ? reinterpret_cast<const float*>(&plan) : nullptr;   // (for the class check; the buffer's address follows)
    {
        std::string bad = media_class_refusal(s, idx, o);
        if (!bad.empty()) return fail(HK_ERR_INVALID, at + bad);
    }
    const size_t need[3] = {(size_t)m.nvdb_size, (size_t)plan.total * sizeof(uint2), plan.bricks ? (size_t)plan.total * 729 * sizeof(float) : 0};
    if (int e = fit_nanovdb_buffers(c, hm, need)) return e;
    o.nvdb = hm.nvdb->as<unsigned char>();
    o.nv_blocks = hm.blocks->as<uint2>();
    o.nv_bricks = plan.bricks ? hm.bricks->as<float>() : nullptr;
    D.tree = hm.nvdb->as<unsigned char>();
    D.table = hm.blocks->as<uint2>();
    for (int k = 0; k < 3; ++k) D.nvb_min[k] = plan.nvb_min[k], D.nvb_dim[k] = plan.nvb_dim[k];
    hk::launch_dense_emit(c->stream, D, ctl.count, (size_t)m.nvdb_size);
    DIndexBox ib;
    for (int k = 0; k < 3; ++k) ib.lo[k] = m.index_bbox_min[k], ib.hi[k] = m.index_bbox_max[k];
    hk::launch_majorant_nanovdb(c->stream, o, ib);
    if (plan.bricks) hk::launch_nvdb_bricks(c->stream, o, (size_t)plan.total);
    HIP_TRY(hipGetLastError());
    std::memcpy(h, &o, sizeof o);
    HIP_TRY(hipMemcpyAsync(s->media.as<DMedium>() + idx, h, sizeof o, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    hm.rec = m;
    hm.d = o;
    return HK_OK;
}

extern "C" int32_t hk_scene_medium_tree_copy(hk_scene* s, int32_t idx, hk_medium* record_out, int64_t* n_bytes, uint8_t* bytes, int32_t* table_dims, int32_t* table_min, uint32_t* table) {
    if (!s || !n_bytes) return fail(HK_ERR_INVALID, "hk_scene_medium_tree_copy: null argument");
    if (idx < 0 || idx >= (int)s->h_media.size()) return fail(HK_ERR_INVALID, "hk_scene_medium_tree_copy: medium index out of range");
    const hk_scene::Medium& hm = s->h_media[idx];
    if (hm.rec.kind != HK_MEDIUM_NANOVDB) return fail(HK_ERR_INVALID, "hk_scene_medium_tree_copy: not a NanoVDB medium");
    if (record_out) {
        *record_out = hm.rec;
        record_out->density = record_out->sigma_a_grid = record_out->sigma_s_grid = record_out->Le_grid = record_out->majorant = nullptr;
        record_out->nvdb_bytes = nullptr;
    }
    *n_bytes = hm.rec.nvdb_size;
    for (int k = 0; k < 3; ++k) {
        if (table_dims) table_dims[k] = hm.d.nvb_dim[k];
        if (table_min) table_min[k] = hm.d.nvb_min[k];
    }
    if (!bytes && !table) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bytes) HIP_TRY(hipMemcpy(bytes, hm.d.nvdb, (size_t)hm.rec.nvdb_size, hipMemcpyDeviceToHost));
    if (table) HIP_TRY(hipMemcpy(table, hm.d.nv_blocks, (size_t)hm.d.nvb_dim[0] * hm.d.nvb_dim[1] * hm.d.nvb_dim[2] * sizeof(uint2), hipMemcpyDeviceToHost));
    return HK_OK;
}

extern "C" int32_t hk_scene_medium_copy(hk_scene* s, int32_t idx, int32_t* n_cells, float* majorant, uint32_t* zero_mask) {
    if (!s || !n_cells) return fail(HK_ERR_INVALID, "hk_scene_medium_copy: null argument");
    if (idx < 0 || idx >= (int)s->h_media.size()) return fail(HK_ERR_INVALID, "hk_scene_medium_copy: medium index out of range");
    const DMedium& d = s->h_media[idx].d;
    const size_t ncell = d.majorant ? (size_t)d.mres[0] * d.mres[1] * d.mres[2] : 0;   // (a homogeneous medium has no grid)
    *n_cells = (int32_t)ncell;
    if (!ncell || (!majorant && !zero_mask)) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (majorant) HIP_TRY(hipMemcpy(majorant, d.majorant, ncell * 4, hipMemcpyDeviceToHost));
    if (zero_mask) HIP_TRY(hipMemcpy(zero_mask, d.maj_zero, (ncell + 31) / 32 * 4, hipMemcpyDeviceToHost));
    return HK_OK;
}

// New base geometry for triangles [first_tri, first_tri + n_tris).  What this leaves valid: everything hk_scene_set_transform leaves
// valid (the header of this file: topology, opacity bits, kinds and the light set are untouched), and the transform intervals
// hk_scene::xf — the new base is put under the transform each triangle is under.  hk_scene::block_box follows the new positions (a
// superset where the range covers a block partly), so quant_grid still proves its grid.  The one wait for the device: a range larger
// than any before grows the device-side staging block, and hipFree of the old one waits for the kernels that read it.
extern "C" int32_t hk_scene_set_vertices(hk_scene* s, int32_t first_tri, int32_t n_tris, const float* positions, const float* normals, const float* tangents, const float* uvs) {
    if (!s || !positions) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: null argument");
    const int T = s->d.n_tris;
    if (T <= 0) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: the scene has no triangles");
    if (first_tri < 0 || n_tris < 1 || (int64_t)first_tri + n_tris > T) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: triangle range outside the scene");
    DScene& D = s->d;
    if (normals && !D.normals) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: normals for a scene created without normals");
    if (tangents && !D.tangents) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: tangents for a scene created without tangents");
    if (uvs && !D.uvs) return fail(HK_ERR_INVALID, "hk_scene_set_vertices: uvs for a scene created without uvs");
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    // the transforms in force on the range, with the normal matrices k_set_tris applies
    const int a = first_tri, e = first_tri + n_tris;
    std::vector<int> iv_start;
    std::vector<DXform> iv_xf;
    for (auto it = std::prev(s->xf.upper_bound(a)); it != s->xf.end() && it->first < e; ++it) {
        DXform X{};
        const std::string bad = make_xform(it->second.m, X);   // (accepted once by hk_scene_set_transform)
        if (!bad.empty()) return fail(HK_ERR_INVALID, bad);
        iv_start.push_back(it->first);
        iv_xf.push_back(X);
    }
    // one staging block: interval starts, transforms, then the arrays given
    const size_t n = (size_t)n_tris;
    const size_t o_start = 0, o_xf = o_start + staged(iv_start.size() * sizeof(int)), o_pos = o_xf + staged(iv_xf.size() * sizeof(DXform));
    const size_t o_nrm = o_pos + staged(n * 36), o_tan = o_nrm + (normals ? staged(n * 36) : 0), o_uv = o_tan + (tangents ? staged(n * 36) : 0);
    const size_t total = o_uv + (uvs ? staged(n * 24) : 0);
    hk_scene::Staging* st = nullptr;
    if (int err = acquire_staging(s, total, st)) return err;
    char* h = static_cast<char*>(st->host);
    std::vector<float> fresh;   // bounds of the new positions per XF_BLOCK triangles (scenes with quantised nodes)
    if (!hk::stage_positions(positions, first_tri, n_tris, reinterpret_cast<float*>(h + o_pos), s->block_box.empty() ? 0 : hk_scene::XF_BLOCK, fresh))
        return fail(HK_ERR_INVALID, "hk_scene_set_vertices: non-finite position");
    if (s->vertex_stage.bytes < total) HIP_TRY(s->vertex_stage.alloc(total));   // (before anything of the scene changes)
    if (int err = join_lanes(c)) return err;   // noted calls render the mesh as it was; the lanes finish before the stream rewrites it
    if (int err = ensure_base(s)) return err;
    std::memcpy(h + o_start, iv_start.data(), iv_start.size() * sizeof(int));
    std::memcpy(h + o_xf, iv_xf.data(), iv_xf.size() * sizeof(DXform));
    if (normals) std::memcpy(h + o_nrm, normals, n * 36);
    if (tangents) std::memcpy(h + o_tan, tangents, n * 36);
    if (uvs) std::memcpy(h + o_uv, uvs, n * 24);
    char* dv = s->vertex_stage.as<char>();
    HIP_TRY(hipMemcpyAsync(dv, h, total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev, c->stream));
    DSetTris A{};
    A.first = first_tri, A.n = n_tris, A.n_iv = (int)iv_start.size();
    A.iv_start = reinterpret_cast<const int*>(dv + o_start);
    A.iv_xf = reinterpret_cast<const DXform*>(dv + o_xf);
    A.in_pos = reinterpret_cast<const float*>(dv + o_pos);
    A.in_nrm = normals ? reinterpret_cast<const float*>(dv + o_nrm) : nullptr;
    A.in_tan = tangents ? reinterpret_cast<const float*>(dv + o_tan) : nullptr;
    A.in_uv = uvs ? reinterpret_cast<const float*>(dv + o_uv) : nullptr;
    A.base_pos = s->base_pos.as<float>();
    A.base_nrm = D.normals ? s->base_nrm.as<float>() : nullptr;
    A.base_tan = D.tangents ? s->base_tan.as<float>() : nullptr;
    A.pos = s->positions.as<float>();
    A.nrm = D.normals ? s->normals.as<float>() : nullptr;
    A.tan = D.tangents ? s->tangents.as<float>() : nullptr;
    A.uvs = D.uvs ? s->uvs.as<float>() : nullptr;
    A.shade = D.tri_shade ? s->tri_shade.as<float>() : nullptr;
    A.geo = tri_geo_rows(s->positions.as<float>(), D.tri_geo);
    A.slot_of_prim = s->slot_of_prim.as<int>();
    A.leaf = s->leaf_tris.as<float4>();
    hk::launch_set_tris(c->stream, A);
    HIP_TRY(hipGetLastError());
    hk::merge_block_boxes(s->block_box, T, first_tri, n_tris, hk_scene::XF_BLOCK, fresh);
    return refit_tree(s);
}

namespace {
// the root node's boxes as the device holds them (the stream has been waited for)
int root_area(hk_scene* s, double& area) {
    DNode root;
    HIP_TRY(hipMemcpy(&root, s->nodes.p, sizeof root, hipMemcpyDeviceToHost));
    float lo[2][3], hi[2][3];
    hk_unpack_node_boxes(root, lo, hi);
    area = hk_root_area(lo, hi);
    return HK_OK;
}
// the cost of the tree hk_scene_rebuild_bvh built: its k_bvh_cost sums and its root node were left in rebuilt_cost on the stream (the
// stream has been waited for)
int take_rebuilt_cost(hk_scene* s) {
    const int nb = s->rebuilt_cost_blocks;
    std::vector<double> part((size_t)nb);
    DNode root;
    HIP_TRY(hipMemcpy(part.data(), s->rebuilt_cost.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&root, s->rebuilt_cost.as<char>() + part.size() * sizeof(double), sizeof root, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (double v : part) sum += v;   // in block order, as hk_scene_bvh_cost adds them
    float lo[2][3], hi[2][3];
    hk_unpack_node_boxes(root, lo, hi);
    const double area = hk_root_area(lo, hi);
    s->cost_created = area > 0.0 ? sum / area : 0.0;
    s->rebuilt_cost_blocks = 0;
    return HK_OK;
}
}  // namespace

extern "C" int32_t hk_scene_bvh_cost(hk_scene* s, double* cost_now, double* cost_created) {
    if (!s) return fail(HK_ERR_INVALID, "hk_scene_bvh_cost: null scene");
    const int N = s->bvh_nodes;
    hk_ctx* c = s->ctx;
    if (s->rebuilt_cost_blocks > 0) {   // a rebuild since the last call: the cost of its tree is on the device
        HIP_TRY(hipSetDevice(c->device));
        KnobScope knobs(&c->knobs);
        if (int e = join_lanes(c)) return e;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int e = take_rebuilt_cost(s)) return e;
    }
    if (cost_created) *cost_created = s->cost_created;
    if (!cost_now) return HK_OK;
    *cost_now = 0.0;
    if (N <= 0) return HK_OK;   // the root is a leaf (or there is no triangle): no inner node, no cost
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    const int nb = hk::bvh_cost_blocks(N);
    if (s->cost_partial.bytes < (size_t)nb * sizeof(double)) HIP_TRY(s->cost_partial.alloc((size_t)nb * sizeof(double)));   // (first call, or a rebuilt tree with more nodes)
    hk::launch_bvh_cost(c->stream, s->nodes.as<DNode>(), N, s->cost_partial.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<double> part((size_t)nb);
    HIP_TRY(hipMemcpy(part.data(), s->cost_partial.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    double sum = 0.0, area = 0.0;
    for (double v : part) sum += v;   // in block order
    if (int e = root_area(s, area)) return e;
    *cost_now = area > 0.0 ? sum / area : 0.0;
    return HK_OK;
}

extern "C" int32_t hk_scene_bvh_copy(hk_scene* s, int32_t* n_nodes, float* boxes, int32_t* refs) {
    if (!s || !n_nodes) return fail(HK_ERR_INVALID, "hk_scene_bvh_copy: null argument");
    const int N = s->bvh_nodes;
    *n_nodes = N;
    if (N <= 0 || (!boxes && !refs)) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<DNode> dn((size_t)N);
    HIP_TRY(hipMemcpy(dn.data(), s->nodes.p, dn.size() * sizeof(DNode), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) {
        if (boxes) {
            float lo[2][3], hi[2][3];
            hk_unpack_node_boxes(dn[i], lo, hi);
            for (int ch = 0; ch < 2; ++ch)
                for (int k = 0; k < 3; ++k) boxes[12 * (size_t)i + 6 * ch + k] = lo[ch][k], boxes[12 * (size_t)i + 6 * ch + 3 + k] = hi[ch][k];
        }
        if (refs) refs[2 * (size_t)i] = dn[i].c0, refs[2 * (size_t)i + 1] = dn[i].c1;
    }
    return HK_OK;
}

extern "C" int32_t hk_scene_bvh_leaves(hk_scene* s, int32_t* n, int32_t* prims) {
    if (!s || !n) return fail(HK_ERR_INVALID, "hk_scene_bvh_leaves: null argument");
    const int T = s->bvh_leaf_tris;
    *n = T;
    if (T <= 0 || !prims) return HK_OK;
    hk_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    KnobScope knobs(&c->knobs);
    if (int e = join_lanes(c)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float4> lt(3 * (size_t)T);
    HIP_TRY(hipMemcpy(lt.data(), s->leaf_tris.p, lt.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (int i = 0; i < T; ++i) std::memcpy(&prims[i], &lt[3 * (size_t)i].w, 4);
    return HK_OK;
}

// A new tree over D.positions.  What this changes, and what follows from it: nodes, quantised nodes, leaf records and the slot table
// get new buffers (built on the stream, boxes and cost included, and exchanged at the end, after the last call that can fail: an error return leaves the scene as it was);
// bvh_nodes / D.n_nodes, bvh_depth / D.bvh_depth and level_start follow the new tree.  Who reads the depth, and why nothing else has
// to be invalidated: the path state's shape (pass_traits / ensure_state, hk_render.cpp: `small_scene`, grey_compact_ok) and the shadow
// stream (`want_overlap`) are decided per render call from the DScene of that call, and ensure_state lays the state out anew — dropping
// its view key, as for any reallocation — when the segment count it wants differs from the one it has; the view key itself holds the
// layout (n_waves, wave_cap, compact, dynamic_segments) and the camera records do not depend on the scene, so a rebuild that keeps the
// layout keeps the cached view.  The kernel instantiations (lean_dispatch, launch_shadow_walk, small_pass_class: hk_launch_impl.h) are
// chosen per launch from DScene::bvh_depth, passed by value.  A scene created shallow has no block_box and no quantised copy: grown past
// 16 levels it runs the deep instantiations on its float nodes (D.qnodes == nullptr: same hits).  A deep scene grown shallow keeps its
// quantised copy up to date (refit_tree) and the 16-entry instantiations do not read it.  Opacity bits and prim words travel with the
// triangles (k_build_leaves copies them from the old slot); transforms (hk_scene::xf), block_box and the base copies are indexed by
// triangle, not by slot, and stay.
extern "C" int32_t hk_scene_rebuild_bvh(hk_scene* s) {
    if (!s) return fail(HK_ERR_INVALID, "hk_scene_rebuild_bvh: null scene");
    hk_ctx* c = s->ctx;
    DScene& D = s->d;
    const int T = D.n_tris;
    KnobScope knobs(&c->knobs);
    const int leaf = hk_bvh_leaf_size(hk::knob_int("HK_BVH_LEAF", 4)), nbins = hk_bvh_bin_count(hk::knob_int("HK_BVH_BINS", 32));
    if (s->bvh_nodes <= 0 || T <= leaf) return HK_OK;   // the root is a leaf (or would be one under the leaf size of now): nothing to build
    HIP_TRY(hipSetDevice(c->device));
    const int small_max = hk::knob_int_in("HK_BVH_BUILD_SMALL", 0, INT_MAX, 1024);
    const int large_cap = (int)((long long)T / ((long long)std::max(small_max, leaf) + 1)) + 1;   // large segments are disjoint and hold more than small_max triangles each
    const size_t n = (size_t)T, cap_nodes = (size_t)std::max(T - 1, 1);
    const size_t cap_seg = n / ((size_t)leaf + 1) + 1;   // a level's inner nodes are disjoint and hold more than `leaf` triangles each
    DevBuf nodes, qnodes, leaf_tris, slots, old_slots, tbox, idx, seg, large, large_cb, large_bins, n_left, order, ctl, cost;
    HIP_TRY(nodes.alloc(cap_nodes * sizeof(DNode)));
    if (s->qnodes_built) HIP_TRY(qnodes.alloc(cap_nodes * sizeof(DQNode)));
    HIP_TRY(leaf_tris.alloc(3 * n * sizeof(float4)));
    if (s->have_base) HIP_TRY(slots.alloc(n * 4));
    else HIP_TRY(old_slots.alloc(n * 4));
    HIP_TRY(tbox.alloc(n * 24));
    HIP_TRY(idx.alloc(2 * n * 4));
    HIP_TRY(seg.alloc(2 * cap_seg * sizeof(DBuildSeg)));
    HIP_TRY(large.alloc(2 * (size_t)large_cap * 4));
    HIP_TRY(large_cb.alloc((size_t)large_cap * 6 * 4));
    HIP_TRY(large_bins.alloc((size_t)large_cap * HK_BUILD_BIN_WORDS * 4));
    HIP_TRY(n_left.alloc(cap_seg * 4));
    HIP_TRY(order.alloc(n * 4));
    HIP_TRY(ctl.alloc(sizeof(DBuildCtl)));
    const int cost_blocks = hk::bvh_cost_blocks((int)cap_nodes);
    HIP_TRY(cost.alloc((size_t)cost_blocks * sizeof(double) + sizeof(DNode)));
    if (int e = join_lanes(c)) return e;   // noted calls render the tree as it was; the lanes finish before the stream builds beside it
    DBuild B{};
    B.n_tris = T, B.leaf = leaf, B.nbins = nbins, B.small_max = small_max, B.large_cap = large_cap;
    B.pos = D.positions;
    B.tbox = tbox.as<float>();
    B.idx[0] = idx.as<int>(), B.idx[1] = idx.as<int>() + n;
    B.seg[0] = seg.as<DBuildSeg>(), B.seg[1] = seg.as<DBuildSeg>() + cap_seg;
    B.large[0] = large.as<int>(), B.large[1] = large.as<int>() + large_cap;
    B.large_cb = large_cb.as<int>(), B.large_bins = large_bins.as<int>();
    B.n_left = n_left.as<int>(), B.order = order.as<int>();
    B.nodes = nodes.as<DNode>();
    B.qnodes = s->qnodes_built ? qnodes.as<DQNode>() : nullptr;
    B.ctl = ctl.as<DBuildCtl>();
    hk::launch_bvh_build(c->stream, B);
    HIP_TRY(hipGetLastError());
    DBuildLeaves A{};
    A.n_tris = T, A.order = B.order, A.pos = D.positions, A.old_leaf = D.leaf_tris, A.leaf = leaf_tris.as<float4>();
    if (s->have_base) A.old_slot_of_prim = s->slot_of_prim.as<int>(), A.slot_of_prim = slots.as<int>();
    else {
        hk::launch_slot_of_prim(c->stream, D.leaf_tris, T, old_slots.as<int>());
        A.old_slot_of_prim = old_slots.as<int>(), A.slot_of_prim = nullptr;
    }
    hk::launch_bvh_build_leaves(c->stream, A);
    HIP_TRY(hipGetLastError());
    // the one wait: node count, depth and level table of the tree just built
    DBuildCtl h{};
    HIP_TRY(hipMemcpyAsync(&h, ctl.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bool sane = h.depth >= 1 && h.depth <= HK_BVH_DEPTH_BUDGET && h.n_nodes >= 1 && (size_t)h.n_nodes <= cap_nodes && h.level_start[0] == 0 && h.level_start[h.depth] == h.n_nodes;
    for (int L = 0; sane && L < h.depth; ++L) sane = h.level_start[L + 1] > h.level_start[L];
    if (!sane) return fail(HK_ERR_DEVICE, "hk_scene_rebuild_bvh: the device builder reported an inconsistent tree (the scene is unchanged)");
    // boxes of the new tree (the quantised copy on a proved grid, or none) and its cost, still into the new buffers: every launch that
    // can be refused has been accepted before anything of the scene changes
    const std::vector<int> levels(h.level_start, h.level_start + h.depth + 1);
    DQGrid grid{};
    DQNode* qn = nullptr;
    if (s->qnodes_built && quant_grid(s, grid)) qn = qnodes.as<DQNode>();
    if (int e = refit_levels(c, levels, nodes.as<DNode>(), qn, grid, leaf_tris.as<float4>(), D.positions)) return e;
    // the cost of this tree (the new cost_created) stays on the device until somebody asks: no second wait here
    const int blocks = hk::bvh_cost_blocks(h.n_nodes);
    hk::launch_bvh_cost(c->stream, nodes.as<DNode>(), h.n_nodes, cost.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cost.as<char>() + (size_t)blocks * sizeof(double), nodes.p, sizeof(DNode), hipMemcpyDeviceToDevice, c->stream));
    // the exchange: nothing below can fail (the old buffers go when this function returns: the stream was waited for before the
    // refit was enqueued, and nothing enqueued since reads them)
    swap_buffers(s->nodes, nodes);
    if (s->qnodes_built) swap_buffers(s->qnodes, qnodes);
    swap_buffers(s->leaf_tris, leaf_tris);
    if (s->have_base) swap_buffers(s->slot_of_prim, slots);
    swap_buffers(s->rebuilt_cost, cost);
    s->rebuilt_cost_blocks = blocks;
    s->bvh_nodes = h.n_nodes, s->bvh_depth = h.depth;
    s->level_start = levels;
    D.nodes = s->nodes.as<DNode>();
    D.leaf_tris = s->leaf_tris.as<float4>();
    D.n_nodes = h.n_nodes, D.bvh_depth = h.depth;
    if (s->qnodes_built) {   // as refit_tree leaves them: the copy on its grid, or null (the float nodes are read: same hits)
        if (qn)
            for (int k = 0; k < 3; ++k) D.q_base[k] = grid.base[k], D.q_cell[k] = grid.cell[k];
        D.qnodes = qn ? s->qnodes.as<DQNode>() : nullptr;
    }
    return HK_OK;
}
