// Host-only check of the light-BVH refit (hikari.jl_amd/csrc/hk_light_bounds.h and hk::refit_light_bvh of light_bvh.cpp, the host twin of
// hk_scene_refit_lights), built by tests/test_light_refit_host.py with g++ -ffp-contract=off, plain and with -fsanitize=address,undefined.
// Over random light sets of mixed kinds and random edit sequences that keep every light's kind and its membership in the tree:
//   - the invariants of a refit tree, in double from the stored binary32 nodes: box = union of the child boxes, phi = the binary32 sum,
//     cos_e = the min, two_sided = the or, and the cone holds both child cones up to a MEASURED slack — the worst residual of
//     angle(w, w_c) + theta_c - theta over the libm-built trees of the same run, times 4 (plus 1e-6 rad where the built tree has none);
//   - a refit with unchanged records keeps boxes, phi, cos_e and bits of the built tree, and its cones within that bound;
//   - nodes off the dirty paths keep their bytes, edited leaves are the leaves of a tree built from the edited records;
//   - the edits one call at a time and all in one call (in another order) end in the same bytes;
//   - asin, acos, sin, cos of the header against libm in double (worst error in binary32 ulps, printed).
// usage: light_refit_check <sequences> <seed>      prints "ok ..." with the measured figures
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "bvh_build.h"
#include "hk_light_bounds.h"

static unsigned rng_state;
static unsigned urand() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static float frand() { return (float)urand() * (1.0f / 16777216.0f); }
#define CHECK(c)                                                                      \
    if (!(c)) {                                                                       \
        std::printf("FAILED %s (line %d, sequence %d, edit %d)\n", #c, __LINE__, seq, edit); \
        return 1;                                                                     \
    }

// a random record of `kind` (the generator of light_rebuild_check.cpp); dark: zero power, outside the tree
static hk_light random_light(int kind, bool dark) {
    hk_light l;
    std::memset(&l, 0, sizeof l);
    l.kind = kind;
    l.envmap = kind == HK_LIGHT_ENVIRONMENT ? 0 : -1;
    l.Le.tex = -1;
    l.spectrum_kind = (urand() & 3) == 0 ? HK_SPEC_ILLUMINANT : HK_SPEC_RGB;
    for (int k = 0; k < 3; ++k) l.i_rgb[k] = dark ? 0.0f : 0.1f + 20.0f * frand();
    l.poly[0] = -1e-5f * frand(), l.poly[1] = 0.01f * frand(), l.poly[2] = frand() - 0.5f;
    l.illum_scale = dark ? 0.0f : 0.5f + frand();
    l.scale = (urand() & 7) == 0 ? 1.0f / 10567.0f : 0.25f + 2.0f * frand();
    const bool clustered = (urand() & 1) != 0;
    for (int k = 0; k < 3; ++k) l.position[k] = clustered ? (float)(urand() % 3) : 20.0f * frand() - 10.0f;
    float d[3] = {frand() - 0.5f, frand() - 0.5f, frand() - 0.5f + 1e-3f};
    if ((urand() & 7) == 0) d[0] = 0.0f, d[1] = 0.0f, d[2] = (urand() & 1) ? 1.0f : -1.0f;   // equal and opposite axes: the union's two sphere branches
    const float dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int k = 0; k < 3; ++k) l.direction[k] = d[k] / dn;
    for (int k = 0; k < 4; ++k) l.world_to_light[5 * k] = l.light_to_world[5 * k] = 1.0f;
    l.light_to_world[2] = d[0] / dn, l.light_to_world[6] = d[1] / dn, l.light_to_world[10] = d[2] / dn;
    l.cos_falloff_start = 0.5f + 0.5f * frand();
    l.cos_total_width = l.cos_falloff_start * frand();
    if ((urand() & 7) == 0) l.cos_total_width = l.cos_falloff_start;
    if (kind == HK_LIGHT_DIFFUSE_AREA) {
        const float size = (urand() & 15) == 0 ? 5.0f : 0.2f;
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) l.v[3 * v + k] = l.position[k] + size * (frand() - 0.5f);
        if ((urand() & 7) == 0) {   // an axis-aligned face: normals that are exactly equal or opposite between lights
            l.v[2] = l.v[5] = l.v[8] = l.position[2];
        }
        float e1[3] = {l.v[3] - l.v[0], l.v[4] - l.v[1], l.v[5] - l.v[2]}, e2[3] = {l.v[6] - l.v[0], l.v[7] - l.v[1], l.v[8] - l.v[2]};
        const float cp[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float twice = std::sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]);
        for (int k = 0; k < 3; ++k) l.normal[k] = twice > 0.0f ? cp[k] / twice : (k == 2 ? 1.0f : 0.0f);
        l.area = dark ? 0.0f : 0.5f * twice;
        for (int k = 0; k < 3; ++k) l.Le.c[k] = dark ? 0.0f : 0.1f + 8.0f * frand();
        l.Le.c[3] = 1.0f;
        l.two_sided = (int)(urand() & 1);
    }
    return l;
}

static double angle_of(const float* a, const float* b) {   // of two (nearly) unit vectors, in double
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
}
static double theta_of(float c) { return std::acos(std::min(1.0, std::max(-1.0, (double)c))); }

// the worst residual of "the cone holds both child cones" over the inner nodes of a tree in host order (<= 0: every cone holds)
static double cone_residual(const hk::LightBVH& t) {
    double worst = 0.0;
    for (size_t i = 0; i < t.nodes.size(); ++i) {
        const hk::LightBVHNodeH& n = t.nodes[i];
        if (n.bits & 2u) continue;
        if (n.cos_o <= -1.0f) continue;   // the whole sphere
        const hk::LightBVHNodeH* ch[2] = {&t.nodes[i + 1], &t.nodes[n.child1_or_light - 1]};
        for (int c = 0; c < 2; ++c) worst = std::max(worst, angle_of(n.w, ch[c]->w) + theta_of(ch[c]->cos_o) - theta_of(n.cos_o));
    }
    return worst;
}
// box, phi, cos_e, two_sided of every inner node against its children
static bool exact_invariants(const hk::LightBVH& t) {
    for (size_t i = 0; i < t.nodes.size(); ++i) {
        const hk::LightBVHNodeH& n = t.nodes[i];
        if (n.bits & 2u) continue;
        const hk::LightBVHNodeH &a = t.nodes[i + 1], &b = t.nodes[n.child1_or_light - 1];
        for (int k = 0; k < 3; ++k)
            if (n.bmin[k] != std::min(a.bmin[k], b.bmin[k]) || n.bmax[k] != std::max(a.bmax[k], b.bmax[k])) return false;
        const volatile float phi = a.phi + b.phi;
        if (n.phi != phi || n.cos_e != std::min(a.cos_e, b.cos_e) || (n.bits & 1u) != ((a.bits | b.bits) & 1u)) return false;
        const double wl = std::sqrt((double)n.w[0] * n.w[0] + (double)n.w[1] * n.w[1] + (double)n.w[2] * n.w[2]);
        if (!(std::fabs(wl - 1.0) < 1e-5) || !(n.cos_o >= -1.0f && n.cos_o <= 1.0f)) return false;
    }
    return true;
}
static double ulps(float got, double want) {
    const float w = (float)want;
    const double ulp = (double)std::nextafter(std::fabs(w) > 0 ? std::fabs(w) : 1e-30f, INFINITY) - (double)(std::fabs(w) > 0 ? std::fabs(w) : 1e-30f);
    return std::fabs((double)got - want) / ulp;
}

int main(int argc, char** argv) {
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 300;
    rng_state = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    int seq = -1, edit = -1;
    // ---- the four functions against libm in double ----
    double e_asin = 0, e_acos = 0, e_sin = 0, e_cos = 0, a_cos = 0;
    for (int i = 0; i <= 2000000; ++i) {
        const float x = (float)i / 2000000.0f;
        e_asin = std::max(e_asin, ulps(hk_lb_asin(x), std::asin((double)x)));
        e_acos = std::max(e_acos, std::max(ulps(hk_lb_acos(x), std::acos((double)x)), ulps(hk_lb_acos(-x), std::acos(-(double)x))));
        const float t = x * HK_LB_PI;
        e_sin = std::max(e_sin, std::fabs((double)hk_lb_sin(t) - std::sin((double)t)));   // absolute: what the rotation of an axis sees
        a_cos = std::max(a_cos, std::fabs((double)hk_lb_cos(t) - std::cos((double)t)));
        if (std::fabs(std::cos((double)t)) > 0.01) e_cos = std::max(e_cos, ulps(hk_lb_cos(t), std::cos((double)t)));
    }
    const double ulp1 = std::ldexp(1.0, -24);   // one ulp of a binary32 value in [0.5, 1)
    std::printf("functions: ulp_asin %.3f ulp_acos %.3f abs_sin_ulp1 %.3f abs_cos_ulp1 %.3f ulp_cos %.3f\n", e_asin, e_acos, e_sin / ulp1, a_cos / ulp1, e_cos);
    CHECK(e_asin <= 4.0&& e_acos <= 4.0 && e_sin <= 2.0 * ulp1 && a_cos <= 2.0 * ulp1 && e_cos <= 4.0);
    CHECK(hk_lb_acos(1.0f) == 0.0f && hk_lb_asin(0.0f) == 0.0f && hk_lb_sin(0.0f) == 0.0f && hk_lb_cos(0.0f) == 1.0f);

    static const int kinds[7] = {HK_LIGHT_POINT, HK_LIGHT_SPOT, HK_LIGHT_DIRECTIONAL, HK_LIGHT_SUN, HK_LIGHT_AMBIENT, HK_LIGHT_ENVIRONMENT, HK_LIGHT_DIFFUSE_AREA};
    double worst_libm = 0.0, worst_refit = 0.0, worst_ratio = 0.0;
    long edits_done = 0, trees = 0, spheres = 0;
    std::vector<std::pair<double, double>> cones;   // (residual of a refit tree, residual of the libm-built tree of the same lights)
    for (seq = 0; seq < sequences; ++seq) {
        edit = -1;
        const int n = seq < 8 ? seq + 1 : 1 + (int)(urand() % 200);
        const int flavour = (int)(urand() % 4);   // 0: every kind, 1: tree lights only, 2: area lights only, 3: points only
        std::vector<hk_light> desc((size_t)n);
        for (int i = 0; i < n; ++i) {
            const int kind = flavour == 1 ? kinds[(urand() & 1) ? 0 : (urand() & 1) ? 1 : 6] : flavour == 2 ? HK_LIGHT_DIFFUSE_AREA : flavour == 3 ? HK_LIGHT_POINT : kinds[urand() % 7];
            desc[(size_t)i] = random_light(kind, (urand() & 7) == 0);
        }
        hk::LightBVH built;
        hk::LightTables tb;
        hk::derive_light_tables(desc.data(), n, built, tb);
        hk::LightRefitLayout lay;
        hk::light_refit_layout(built, lay);
        const double slack_of_built = cone_residual(built);
        worst_libm = std::max(worst_libm, slack_of_built);
        CHECK(exact_invariants(built));
        ++trees;
        // the layout: every node has one entry, every light of the tree a leaf entry
        CHECK(lay.n_entries == (built.nodes.empty() ? 0 : 2 * built.num_bvh));
        for (int i = 0; i < n; ++i) CHECK((lay.leaf_entry[(size_t)i] >= 0) == (built.bit_trails[(size_t)i] != 0xFFFFFFFFu));
        // ---- unchanged records, every light: what has no transcendental in it keeps its bits ----
        {
            std::vector<int32_t> idx((size_t)n);
            for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
            hk::LightBVH same = built;
            hk::LightTables ts = tb;
            hk::refit_light_bvh(same, ts, lay, n, idx.data(), desc.data());
            CHECK(same.nodes.size() == built.nodes.size());
            for (size_t i = 0; i < built.nodes.size(); ++i) {
                const hk::LightBVHNodeH &a = same.nodes[i], &b = built.nodes[i];
                CHECK(std::memcmp(a.bmin, b.bmin, 24) == 0 && a.phi == b.phi && a.cos_e == b.cos_e && a.bits == b.bits && a.child1_or_light == b.child1_or_light);
                if (a.bits & 2u) CHECK(std::memcmp(&a, &b, sizeof a) == 0);
                CHECK(std::memcmp(&ts.nodes[(size_t)lay.entry_of_host[i]].bits, &tb.nodes[(size_t)lay.entry_of_host[i]].bits, 8) == 0);   // bits and child entry of the walked table
                if (a.bits & 2u) CHECK(std::memcmp(&ts.nodes[(size_t)lay.entry_of_host[i]], &tb.nodes[(size_t)lay.entry_of_host[i]], 64) == 0);
                spheres += !(a.bits & 2u) && a.cos_o == -1.0f;
            }
            const double r = cone_residual(same);
            worst_refit = std::max(worst_refit, r);
            if (slack_of_built > 0.0) worst_ratio = std::max(worst_ratio, r / slack_of_built);
            cones.emplace_back(r, slack_of_built);
            CHECK(exact_invariants(same));
        }
        // ---- edit sequences ----
        hk::LightBVH seq_tree = built;
        hk::LightTables seq_tab = tb;
        std::vector<hk_light> now = desc;
        std::vector<int32_t> all_idx;
        std::vector<char> touched((size_t)n, 0);
        const int n_edits = 1 + (int)(urand() % 4);
        for (edit = 0; edit < n_edits; ++edit) {
            std::vector<int32_t> idx;
            std::vector<hk_light> rec;
            const int mode = (int)(urand() % 3);   // 0: one light, 1: a scattered third, 2: all
            for (int i = 0; i < n; ++i) {
                if (mode == 1 && urand() % 3) continue;
                const bool in_tree = built.bit_trails[(size_t)i] != 0xFFFFFFFFu;
                hk_light l;
                hk::LightBVHNodeH leaf;
                int tries = 0;
                do l = random_light(desc[(size_t)i].kind, !in_tree);
                while ((hk::light_leaf(l, i + 1, leaf) == 2) != in_tree && ++tries < 16);
                if ((hk::light_leaf(l, i + 1, leaf) == 2) != in_tree) continue;
                idx.push_back(i), rec.push_back(l);
            }
            if (mode == 0 && !idx.empty()) {
                const size_t k = urand() % idx.size();
                idx = {idx[k]}, rec = {rec[k]};
            }
            if (idx.empty()) continue;
            if (urand() & 1) std::reverse(idx.begin(), idx.end()), std::reverse(rec.begin(), rec.end());
            const hk::LightBVH before = seq_tree;
            hk::refit_light_bvh(seq_tree, seq_tab, lay, (int)idx.size(), idx.data(), rec.data());
            for (size_t j = 0; j < idx.size(); ++j) now[(size_t)idx[j]] = rec[j], touched[(size_t)idx[j]] = 1;
            // off the dirty paths nothing moved
            std::vector<char> dirty((size_t)std::max(lay.n_entries, 1), 0);
            for (int32_t i : idx)
                for (int32_t e = lay.leaf_entry[(size_t)i]; e >= 0; e = lay.parent[(size_t)e]) dirty[(size_t)e] = 1;
            for (size_t h = 0; h < seq_tree.nodes.size(); ++h)
                if (!dirty[(size_t)lay.entry_of_host[h]]) CHECK(std::memcmp(&seq_tree.nodes[h], &before.nodes[h], 64) == 0);
            CHECK(exact_invariants(seq_tree));
            // the measured slack of a tree BUILT from the records as they are now
            hk::LightBVH fresh;
            hk::LightTables tf;
            hk::derive_light_tables(now.data(), n, fresh, tf);
            CHECK(fresh.bit_trails.size() == seq_tree.bit_trails.size() && fresh.num_bvh == built.num_bvh);
            const double slack = cone_residual(fresh), r = cone_residual(seq_tree);
            worst_libm = std::max(worst_libm, slack), worst_refit = std::max(worst_refit, r);
            if (slack > 0.0) worst_ratio = std::max(worst_ratio, r / slack);
            cones.emplace_back(r, slack);
            // edited leaves are the fresh tree's leaves of those lights
            for (int32_t i : idx) {
                if (lay.leaf_entry[(size_t)i] < 0) continue;
                const hk::LightBVHNodeH& mine = seq_tree.nodes[(size_t)lay.host_of_entry[(size_t)lay.leaf_entry[(size_t)i]]];
                bool found = false;
                for (const auto& f : fresh.nodes)
                    if ((f.bits & 2u) && f.child1_or_light == (uint32_t)(i + 1)) found = std::memcmp(&f, &mine, 64) == 0;
                CHECK(found);
            }
            // the walked table is the header's record of every node
            for (size_t h = 0; h < seq_tree.nodes.size(); ++h) {
                if (!dirty[(size_t)lay.entry_of_host[h]]) continue;
                HkLightRaw raw;
                std::memcpy(&raw, &seq_tree.nodes[h], 64);
                const hk::LightNodeRec& got = seq_tab.nodes[(size_t)lay.entry_of_host[h]];
                const HkLightWalk w = hk_lb_walk_record(raw, got.child1_or_light);
                CHECK(std::memcmp(&w, &got, 64) == 0);
            }
            ++edits_done;
        }
        edit = -2;
        // ---- the same edits in ONE call, in another order ----
        for (int i = n - 1; i >= 0; --i)
            if (touched[(size_t)i]) all_idx.push_back(i);
        if (!all_idx.empty()) {
            std::vector<hk_light> rec;
            for (int32_t i : all_idx) rec.push_back(now[(size_t)i]);
            hk::LightBVH one = built;
            hk::LightTables to = tb;
            hk::refit_light_bvh(one, to, lay, (int)all_idx.size(), all_idx.data(), rec.data());
            // (a node dirtied by the sequence but not by its last edits was still computed from the same final children)
            CHECK(one.nodes.size() == seq_tree.nodes.size() && (one.nodes.empty() || std::memcmp(one.nodes.data(), seq_tree.nodes.data(), one.nodes.size() * 64) == 0));
            CHECK(std::memcmp(to.nodes.data(), seq_tab.nodes.data(), to.nodes.size() * 64) == 0);
            CHECK(one.bit_trails == built.bit_trails);
        }
    }
    // the cone bound, once the slack is measured: 4 x the worst residual of the libm-built trees of this run, plus 1e-6 rad for the
    // lights whose own built tree has none.  (Tree by tree the ratio is printed, not bounded: a built tree of few cones is often
    // exact by luck, and the refit of the same lights is not.)
    seq = edit = -3;
    for (const auto& c : cones) CHECK(c.first <= 4.0 * worst_libm + (c.second > 0.0 ? 0.0 : 1e-6));
    std::printf("ok sequences %d trees %ld edits %ld sphere-nodes %ld libm_residual %.9g refit_residual %.9g worst_ratio %.4g ulp_asin %.3f ulp_acos %.3f abs_sin_ulp1 %.3f abs_cos_ulp1 %.3f ulp_cos %.3f\n",
                sequences, trees, edits_done, spheres, worst_libm, worst_refit, worst_ratio, e_asin, e_acos, e_sin / ulp1, a_cos / ulp1, e_cos);
    return 0;
}
