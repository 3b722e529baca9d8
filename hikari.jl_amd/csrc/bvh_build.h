// bvh_build.h — host-side acceleration-structure builders of the HIP library.
#pragma once
#include <cstdint>
#include <vector>

#include "hikari_mi355x.h"

namespace hk {

struct BVHNode {
    float lo0[3], hi0[3], lo1[3], hi1[3];
    int c0, c1;
};
struct BVH {
    std::vector<BVHNode> nodes;
    std::vector<int> leaf_prims;  // original triangle index per leaf slot
    int root_ref = 0;
    int max_depth = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    int median_splits = 0;        // nodes cut at count / 2 instead of a SAH boundary (coincident centroids, or the depth budget)
};
#define HK_BVH_COUNTS_MEDIANS 1
void build_bvh(const float* positions, int n_tris, BVH& out, int leaf_size = 4, int bins = 32);   // leaf_size: triangles per leaf, 1 .. 8; bins: SAH bins per axis, 4 .. 64
// (32 bins since round 5: the 10^6-triangle scene's traversal - 1.7 %, its any-hit casts - 1.5 % against 16, 64 no better, 8 + 1 %; the small scenes unchanged)

// Light BVH (lights/bvh-light-sampler.jl:283-466).  Node = 16 floats/uints as uploaded to the device.
struct LightBVHNodeH {
    float bmin[3], bmax[3], w[3];
    float phi, cos_o, cos_e;
    uint32_t bits;             // bit0 two_sided, bit1 leaf
    uint32_t child1_or_light;  // 1-based
    uint32_t pad[2];
};
struct LightBVH {
    std::vector<LightBVHNodeH> nodes;
    std::vector<uint32_t> bit_trails;   // per light, 0xFFFFFFFF = not in the BVH
    std::vector<int32_t> infinite;      // 1-based flat indices
    int num_bvh = 0;
};
// max_poly[i]: max_value of light i's sigmoid polynomial (needed for RGBIlluminantSpectrum luminance)
void build_light_bvh(const hk_light* lights, int n, LightBVH& out);
// A light-BVH node as the device walks it: the layout of DLightNode (hk_types.h, which says what the fields are; hk_scene.cpp asserts
// that the two agree), declared here so that the host-only builder can fill it.
struct LightNodeRec {
    float centre[3];
    float half_diag;
    float r2;
    float w[3];
    float phi, cos_o, cos_e, sin_o;
    uint32_t bits;
    uint32_t child1_or_light;
    uint32_t pad[2];
};
// What the device holds of a light set besides the baked records: the nodes in sibling-pair order, the bit trail of every light, the
// infinite lights (1-based) and the two counts of DScene.  No array is empty (one zeroed entry stands in).  A set of n lights gives at
// most 2 n node entries, n trails and n infinite lights: the capacities hk_scene_create allocates.
struct LightTables {
    std::vector<LightNodeRec> nodes;
    std::vector<uint32_t> trails;
    std::vector<int32_t> infinite;
    int num_bvh = 0, num_infinite = 0;
};
void derive_light_tables(const hk_light* lights, int n, LightBVH& bvh, LightTables& out);

// ---- the light-BVH refit (hk_scene_refit_lights; the arithmetic of inner nodes is hk_light_bounds.h) ----
// The builder's own bounds of one light.  0: an infinite kind, 1: bounded but outside the tree (phi is not > 0), 2: in the tree, and
// `leaf` is the leaf node build_light_bvh makes of it (light_1based in child1_or_light).
int light_leaf(const hk_light& l, int light_1based, LightBVHNodeH& leaf);
// Where the nodes of a built tree lie on the device (sibling-pair order) and what a refit needs to climb it.
struct LightRefitLayout {
    int n_entries = 0;                    // device entries: 2 per light of the tree, entry 1 unused; 0: empty tree
    std::vector<int32_t> entry_of_host;   // per host node
    std::vector<int32_t> host_of_entry;   // per entry (-1: entry 1)
    std::vector<int32_t> parent;          // per entry (-1: the root, entry 1)
    std::vector<int32_t> leaf_entry;      // per light of the scene, 0-based (-1: not in the tree)
    std::vector<int32_t> level_entries;   // the inner entries grouped by depth: depth d is [level_start[d], level_start[d + 1])
    std::vector<int32_t> level_start;
};
void light_refit_layout(const LightBVH& bvh, LightRefitLayout& out);
// the host twin of the device refit: n distinct 0-based light indices and their new records (kinds and tree membership unchanged)
void refit_light_bvh(LightBVH& bvh, LightTables& t, const LightRefitLayout& lay, int n, const int32_t* index, const hk_light* lights);

// sigmoid-polynomial helpers shared by the host-side bakers (spectral/rgb2spec.jl:17-53, 85-167)
struct RGB2Spec {
    int res = 0;
    const float* scale = nullptr;
    const float* coeffs = nullptr;
};
void rgb_to_coeffs(const RGB2Spec& t, float r, float g, float b, float out[3]);
float poly_eval(const float c[3], float lambda);
float poly_max(const float c[3]);

}  // namespace hk
