// Host-only check of hk::derive_light_tables (hikari.jl_amd/csrc/light_bvh.cpp), the one code path from hk_light records to the device's
// light tables, driven the way hk_scene_update_lights drives it (built by tests/test_light_edits_host.py with g++, once more with
// -fsanitize=address,undefined).  A "scene" keeps its light records and three arrays allocated ONCE at the capacity of its light
// count (2 n node entries, n trails, n infinite lights); every edit of a random sequence replaces a range of records — kinds kept,
// powers switched to zero and back, lights moved, re-coloured, re-aimed — derives the tables from the whole array and copies them over
// what the arrays held.  After every edit: the tables fit the capacities, and the live part of the arrays, the counts and the host tree
// equal, byte for byte, what a scene created from scratch from the edited records holds.
// usage: light_rebuild_check <sequences> <seed>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh_build.h"

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

// a random record of `kind`; dark: zero power (a point / spot / area light then stays out of the tree)
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
    const bool clustered = (urand() & 1) != 0;   // some lights share a spot: centroid ties, the builder's median fallback
    for (int k = 0; k < 3; ++k) l.position[k] = clustered ? (float)(urand() % 3) : 20.0f * frand() - 10.0f;
    float d[3] = {frand() - 0.5f, frand() - 0.5f, frand() - 0.5f + 1e-3f};
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
        const float e1[3] = {l.v[3] - l.v[0], l.v[4] - l.v[1], l.v[5] - l.v[2]}, e2[3] = {l.v[6] - l.v[0], l.v[7] - l.v[1], l.v[8] - l.v[2]};
        const float cp[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float twice = std::sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]);
        for (int k = 0; k < 3; ++k) l.normal[k] = twice > 0.0f ? cp[k] / twice : (k == 2 ? 1.0f : 0.0f);
        l.area = dark && (urand() & 1) ? 0.0f : 0.5f * twice;   // a degenerate moved face: area 0
        for (int k = 0; k < 3; ++k) l.Le.c[k] = dark ? 0.0f : 0.1f + 8.0f * frand();
        l.Le.c[3] = 1.0f;
        l.two_sided = (int)(urand() & 1);
    }
    return l;
}

struct Scene {   // what hk_scene keeps of its lights: the records, the host tree, the arrays at capacity, the counts
    std::vector<hk_light> lights;
    hk::LightBVH lbvh;
    std::vector<hk::LightNodeRec> nodes;
    std::vector<uint32_t> trails;
    std::vector<int32_t> infinite;
    int num_bvh = 0, num_infinite = 0;
    bool fits = true;
    void create(const std::vector<hk_light>& l) {
        lights = l;
        const size_t cap = l.empty() ? 1 : l.size();
        nodes.assign(2 * cap, hk::LightNodeRec{});
        trails.assign(cap, 0u);
        infinite.assign(cap, 0);
        derive();
    }
    void derive() {
        hk::LightTables t;
        hk::derive_light_tables(lights.data(), (int)lights.size(), lbvh, t);
        fits = t.nodes.size() <= nodes.size() && t.trails.size() <= trails.size() && t.infinite.size() <= infinite.size() && !t.nodes.empty() && !t.trails.empty() &&
               !t.infinite.empty();
        if (!fits) return;   // (never copy past a capacity, not even in a failing check)
        std::memcpy(nodes.data(), t.nodes.data(), t.nodes.size() * sizeof(hk::LightNodeRec));
        std::memcpy(trails.data(), t.trails.data(), t.trails.size() * 4);
        std::memcpy(infinite.data(), t.infinite.data(), t.infinite.size() * 4);
        num_bvh = t.num_bvh, num_infinite = t.num_infinite;
    }
    void update(int first, int n, const hk_light* l) {
        for (int j = 0; j < n; ++j) lights[first + j] = l[j];
        derive();
    }
};

int main(int argc, char** argv) {
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 300;
    rng_state = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    static const int kinds[7] = {HK_LIGHT_POINT, HK_LIGHT_SPOT, HK_LIGHT_DIRECTIONAL, HK_LIGHT_SUN, HK_LIGHT_AMBIENT, HK_LIGHT_ENVIRONMENT, HK_LIGHT_DIFFUSE_AREA};
    static_assert(sizeof(hk::LightNodeRec) == 64, "node record");
    long edits_done = 0, emptied = 0, deepest = 0;
    for (int seq = 0; seq < sequences; ++seq) {
        int edit = -1;
        const int n = seq < 8 ? seq + 1 : 1 + (int)(urand() % 200);
        const int flavour = (int)(urand() % 4);   // 0: every kind, 1: tree lights only, 2: area lights only, 3: mostly infinite lights
        std::vector<hk_light> desc(n);
        for (int i = 0; i < n; ++i) {
            const int kind = flavour == 1 ? kinds[(urand() & 1) ? 0 : (urand() & 1) ? 1 : 6] : flavour == 2 ? HK_LIGHT_DIFFUSE_AREA : flavour == 3 && (urand() & 3) ? kinds[2 + urand() % 4] : kinds[urand() % 7];
            desc[i] = random_light(kind, (urand() & 7) == 0);
        }
        Scene edited;
        edited.create(desc);
        CHECK(edited.fits);
        const int n_edits = 1 + (int)(urand() % 6);
        for (edit = 0; edit < n_edits; ++edit) {
            int first = (int)(urand() % n), count = 1 + (int)(urand() % (n - first));
            const int mode = (int)(urand() % 4);   // 0: new values, 1: the range goes dark, 2: the WHOLE scene goes dark (empty tree), 3: one light
            if (mode == 2) first = 0, count = n;
            if (mode == 3) count = 1;
            std::vector<hk_light> repl(count);
            for (int j = 0; j < count; ++j) repl[j] = random_light(desc[first + j].kind, mode == 1 || mode == 2);
            edited.update(first, count, repl.data());
            CHECK(edited.fits);
            for (int j = 0; j < count; ++j) desc[first + j] = repl[j];
            Scene fresh;
            fresh.create(desc);
            CHECK(fresh.fits);
            CHECK(edited.num_bvh == fresh.num_bvh && edited.num_infinite == fresh.num_infinite);
            CHECK(fresh.num_bvh <= n && fresh.num_infinite <= n);
            const size_t live_nodes = fresh.num_bvh > 0 ? 2 * (size_t)fresh.num_bvh : 1;   // what a descent or k_light_select's LDS fill can read
            CHECK(live_nodes <= edited.nodes.size());
            CHECK(std::memcmp(edited.nodes.data(), fresh.nodes.data(), live_nodes * sizeof(hk::LightNodeRec)) == 0);
            CHECK(std::memcmp(edited.trails.data(), fresh.trails.data(), (size_t)n * 4) == 0);
            CHECK(std::memcmp(edited.infinite.data(), fresh.infinite.data(), (size_t)fresh.num_infinite * 4) == 0);
            CHECK(edited.lbvh.nodes.size() == fresh.lbvh.nodes.size() && edited.lbvh.bit_trails == fresh.lbvh.bit_trails && edited.lbvh.infinite == fresh.lbvh.infinite);
            CHECK(edited.lbvh.nodes.empty() || std::memcmp(edited.lbvh.nodes.data(), fresh.lbvh.nodes.data(), fresh.lbvh.nodes.size() * sizeof(hk::LightBVHNodeH)) == 0);
            // every child entry an inner node names, and every light a leaf names, is inside the live part
            if (fresh.num_bvh > 0)
                for (size_t e = 0; e < live_nodes; ++e) {
                    if (e == 1) continue;
                    const hk::LightNodeRec& nd = edited.nodes[e];
                    if (nd.bits & 2u) {
                        CHECK(nd.child1_or_light >= 1 && nd.child1_or_light <= (uint32_t)n);
                    } else {
                        CHECK(nd.child1_or_light >= 2 && nd.child1_or_light + 1 < live_nodes && nd.child1_or_light % 2 == 0);
                    }
                }
            ++edits_done;
            emptied += fresh.num_bvh == 0;
            if ((long)fresh.lbvh.nodes.size() > deepest) deepest = (long)fresh.lbvh.nodes.size();
        }
    }
    std::printf("ok sequences %d edits %ld empty-tree states %ld largest tree %ld nodes\n", sequences, edits_done, emptied, deepest);
    return 0;
}
