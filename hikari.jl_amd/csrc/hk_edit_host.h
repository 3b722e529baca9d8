// hk_edit_host.h — the host arithmetic of hk_scene_set_vertices and hk_scene_bvh_cost that needs no device: staging a range of new
// positions (finite check, copy, bounds per block of triangles in one pass), folding those bounds into hk_scene::block_box, and the
// cost of a tree from its float child boxes; and whether the material records hold a MixMaterial.  Plain C++ (tests/native/vertex_edit_check.cpp builds it alone, under the sanitizers);
// hk_node_cost is also what the device reduction (k_bvh_cost) evaluates per node, so both sides round alike.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define HK_EDIT_HD __host__ __device__
#else
#define HK_EDIT_HD
#endif

// Surface area 2(dx*dy + dx*dz + dy*dz) of a box in double from its float planes; an empty box (some lo > hi, or a NaN plane) has none.
HK_EDIT_HD inline double hk_box_area(const float lo[3], const float hi[3]) {
    if (!(lo[0] <= hi[0]) || !(lo[1] <= hi[1]) || !(lo[2] <= hi[2])) return 0.0;
    const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
    return 2.0 * ((dx * dy + dx * dz) + dy * dz);
}
// One node's share of the tree cost before the division by the root's area: A(child) * w over both children, w = 1 for an inner
// child (ref >= 0) and the triangle count for a leaf child (ref = ~(first << 3 | count - 1)).
HK_EDIT_HD inline double hk_node_cost(const float lo[2][3], const float hi[2][3], int c0, int c1) {
    const double w0 = c0 >= 0 ? 1.0 : (double)(((~c0) & 7) + 1), w1 = c1 >= 0 ? 1.0 : (double)(((~c1) & 7) + 1);
    return hk_box_area(lo[0], hi[0]) * w0 + hk_box_area(lo[1], hi[1]) * w1;
}
// Area of the root box: the union of the root node's two child boxes (an empty child adds nothing).
HK_EDIT_HD inline double hk_root_area(const float lo[2][3], const float hi[2][3]) {
    float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int c = 0; c < 2; ++c) {
        if (!(lo[c][0] <= hi[c][0]) || !(lo[c][1] <= hi[c][1]) || !(lo[c][2] <= hi[c][2])) continue;
        for (int k = 0; k < 3; ++k) l[k] = lo[c][k] < l[k] ? lo[c][k] : l[k], h[k] = h[k] < hi[c][k] ? hi[c][k] : h[k];
    }
    return hk_box_area(l, h);
}

namespace hk {

// DScene::has_mix from the material records as created / last updated (hk_material: `kind`); hk_scene_create and
// hk_scene_update_materials both ask this, over ALL records, so the flag cannot drift from them.
template <class Material>
inline int materials_have_kind(const Material* m, size_t n, int kind) {
    for (size_t i = 0; i < n; ++i)
        if (m[i].kind == kind) return 1;
    return 0;
}
// DScene::single_kind: the one material kind of a scene without a MixMaterial whose non-Mix records (kinds_mask: bit k = a record of
// kind k) are all of that kind and which has a queue (kind < max_kinds); -1 otherwise.
inline int single_material_kind(unsigned kinds_mask, int has_mix, int max_kinds) {
    if (has_mix || kinds_mask == 0u || (kinds_mask & (kinds_mask - 1u)) != 0u) return -1;
    int k = 0;
    while (!((kinds_mask >> k) & 1u)) ++k;
    return k < max_kinds ? k : -1;
}
// DPathState::shade_slot_walk from the knobs (ensure_state): HK_SHADE_SLOT_WALK, unless the emissive pre-scan is asked for
// (HK_SHADE_PRESCAN=1: a pass over the kind queue) or the LEAN k_shade is off (HK_SHADE_LEAN=0) — both mean the queue walk.
inline bool shade_slot_walk_wanted(bool slot_walk_knob, bool prescan, bool lean_knob) { return slot_walk_knob && !prescan && lean_knob; }
// ... and per launch (launch_shade, for the LEAN k_shade of kind `kind`): the scene is of that one kind and the trace launch of this
// bounce ran k_trace_lean's single-kind flush (launch_trace: not the counting instantiation), which marks escaped entries in mat_id.
inline bool shade_slot_walk_launch(int wanted, int single_kind, int kind, bool single_flush) { return wanted != 0 && single_kind >= 0 && single_kind == kind && single_flush; }

// Copies the 9 * n floats of triangles [first, first + n) to `dst` and, when `block` > 0, notes lo[3] hi[3] of every block of `block`
// triangles the range touches in `fresh` (block first / block comes first).  false: a position is not finite (dst and fresh are then
// unspecified; nothing else was written).
inline bool stage_positions(const float* src, int first, int n, float* dst, int block, std::vector<float>& fresh) {
    fresh.clear();
    const int b0 = block > 0 ? first / block : 0;
    if (block > 0) {
        const int nb = (first + n - 1) / block - b0 + 1;
        fresh.resize(6 * (size_t)nb);
        for (int b = 0; b < nb; ++b)
            for (int k = 0; k < 3; ++k) fresh[6 * (size_t)b + k] = INFINITY, fresh[6 * (size_t)b + 3 + k] = -INFINITY;
    }
    bool finite = true;
    for (int i = 0; i < n; ++i) {
        const float* p = src + 9 * (size_t)i;
        std::memcpy(dst + 9 * (size_t)i, p, 36);
        for (int v = 0; v < 9; ++v) finite = finite && std::isfinite(p[v]);
        if (block > 0) {
            float* bb = fresh.data() + 6 * (size_t)((first + i) / block - b0);
            for (int v = 0; v < 9; ++v) {
                bb[v % 3] = std::min(bb[v % 3], p[v]);
                bb[3 + v % 3] = std::max(bb[3 + v % 3], p[v]);
            }
        }
    }
    return finite;
}

// Folds the bounds stage_positions noted into block_box (lo[3] hi[3] per `block` triangles of a scene of n_tris): a block the range
// covers whole gets the new box, a block it covers partly the union with what it had (a superset of the block's true bounds).
inline void merge_block_boxes(std::vector<float>& block_box, int n_tris, int first, int n, int block, const std::vector<float>& fresh) {
    if (block_box.empty() || block <= 0) return;
    const int b0 = first / block, b1 = (first + n - 1) / block;
    for (int b = b0; b <= b1; ++b) {
        float* bb = block_box.data() + 6 * (size_t)b;
        const float* nb = fresh.data() + 6 * (size_t)(b - b0);
        const int begin = b * block, end = std::min(n_tris, begin + block);
        const bool whole = first <= begin && first + n >= end;
        for (int k = 0; k < 3; ++k) {
            bb[k] = whole ? nb[k] : std::min(bb[k], nb[k]);
            bb[3 + k] = whole ? nb[3 + k] : std::max(bb[3 + k], nb[3 + k]);
        }
    }
}

// THE GEOMETRY TABLE (DScene::tri_geo, hk_types.h).  tri_geo_word: the value of that word for a scene as created — 0 no table (no
// triangles, or rows that an int offset cannot reach), 1 the rows are words 28 .. 31 of the packed records, else the offset in floats of
// the float4 rows from the start of the positions: the first 16-byte boundary behind the 9 n_tris floats.  positions_floats: what the
// positions' allocation holds then.
inline int tri_geo_word(int n_tris, bool packed) {
    if (n_tris <= 0) return 0;
    if (packed) return 1;
    const long long off = (9LL * n_tris + 3) & ~3LL;
    return off <= 0x7fffffffLL ? (int)off : 0;
}
inline size_t positions_floats(int n_tris, int word, bool packed) {
    const size_t T = n_tris > 0 ? (size_t)n_tris : 0;
    return (!packed && word != 0) ? (size_t)word + 4 * T : 9 * T;
}
// K12 per launch (launch_film): the grouped fold is the arm of passes of 64 k samples per pixel (HK_FILM_FOLD=0: never)
inline bool film_fold_launch(bool knob, int samples_in_pass) { return knob && samples_in_pass >= 64 && (samples_in_pass & 63) == 0; }

// hk_scene_bvh_cost's formula over a whole tree on the host: node(i, lo, hi, c0, c1) hands out node i (node 0 is the root); the terms
// are added in node order.  0 for a tree without inner nodes or a root without area.
template <class Node>
inline double tree_cost(size_t n_nodes, Node&& node) {
    double sum = 0.0, root = 0.0;
    for (size_t i = 0; i < n_nodes; ++i) {
        float lo[2][3], hi[2][3];
        int c0 = 0, c1 = 0;
        node(i, lo, hi, c0, c1);
        if (i == 0) root = hk_root_area(lo, hi);
        sum += hk_node_cost(lo, hi, c0, c1);
    }
    return root > 0.0 ? sum / root : 0.0;
}
// ... over hk_scene_bvh_copy's arrays: boxes = 12 floats per node (lo0 hi0 lo1 hi1), refs = 2 per node
inline double tree_cost(const float* boxes, const int* refs, size_t n_nodes) {
    return tree_cost(n_nodes, [&](size_t i, float lo[2][3], float hi[2][3], int& c0, int& c1) {
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 3; ++k) lo[c][k] = boxes[12 * i + 6 * c + k], hi[c][k] = boxes[12 * i + 6 * c + 3 + k];
        c0 = refs[2 * i], c1 = refs[2 * i + 1];
    });
}

}  // namespace hk
