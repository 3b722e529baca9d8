// hk_bvh_decide.h — the per-node decision of the binned-SAH BVH builder, shared by the host builder (bvh_build.cpp, hk_scene_create)
// and the device builder (k_build_split, hk_scene_rebuild_bvh), so that both take the same decision from the same bins and a rebuilt
// scene gets the tree a fresh scene would get.  Plain C++ (tests/native/bvh_decide_check.cpp builds it alone, under the sanitizers);
// binary32 without contraction on both sides (the library's build flags), division the correctly rounded one.
//
// The inputs of a decision are order-free: the box of the node's centroids, and per axis and bin the union of the triangle boxes that
// fall into the bin (minima and maxima) and their number (an integer).  Whatever order the triangles arrive in — sequentially on the
// host, through integer-keyed atomic min / max on the device — the bins hold the same values (a zero may differ in sign; no
// comparison or product below tells the two apart), and so does the decision.
//
// MEDIAN FALLBACK.  When no bin boundary separates the centroids (all coincide) or the depth budget refuses the SAH split, the node is
// cut at first + count / 2.  The two builders agree on the SIZES of the two sides of that node (so the depth budget holds exactly as
// on the host), not on which triangles land on which side: the host takes the count / 2 smallest centroids of the widest axis
// (std::nth_element), the device cuts the segment in the order it has.  Below a node of coincident centroids everything is split by
// count, so the references still agree; below a node the budget cut, the subtrees may differ.  Either is a valid tree (same hits); a
// test that compares trees checks first that the scene takes no fallback.
#pragma once

#if defined(__HIPCC__)
#define HK_BVH_HD __host__ __device__
#else
#define HK_BVH_HD
#endif

#define HK_BVH_MAX_BINS 64
#define HK_BVH_DEPTH_BUDGET 30   // < HK_LDS_STACK: a per-lane stack of that many entries never overflows
#define HK_BVH_MAX_LEVELS 31     // inner nodes live on levels 0 .. HK_BVH_DEPTH_BUDGET - 1; the device builder launches this many

// the knobs as both builders resolve them (HK_BVH_LEAF, HK_BVH_BINS)
HK_BVH_HD inline int hk_bvh_leaf_size(int leaf) { return leaf >= 1 && leaf <= 8 ? leaf : 4; }
HK_BVH_HD inline int hk_bvh_bin_count(int bins) { return bins < 4 ? 4 : (bins > HK_BVH_MAX_BINS ? HK_BVH_MAX_BINS : bins); }

// levels a median-split subtree of `count` triangles still needs (leaves of at most `leaf`)
HK_BVH_HD inline int hk_bvh_levels_needed(int count, int leaf) {
    if (count <= leaf) return 0;
    const int v = (count + leaf - 1) / leaf;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
// bins per unit of centroid extent along an axis, and the bin of a centroid (lo: the centroid box's lower plane)
HK_BVH_HD inline float hk_bvh_bin_scale(float ext, int nbins) { return nbins / ext; }
HK_BVH_HD inline int hk_bvh_bin_of(float centroid, float lo, float scale, int nbins) {
    int b = (int)((centroid - lo) * scale);
    b = b < 0 ? 0 : b;
    return b > nbins - 1 ? nbins - 1 : b;
}
// half the surface area of a box; an empty one (lo = +inf, hi = -inf: the difference is not >= 0) has none
HK_BVH_HD inline float hk_bvh_half_area(const float lo[3], const float hi[3]) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0)) return 0.0f;
    return dx * dy + dy * dz + dz * dx;
}

// One axis' bins: lo / hi[b][k] the union of the triangle boxes of bin b (+inf / -inf where empty), cnt[b] their number.
struct HkBvhBins {
    float lo[HK_BVH_MAX_BINS][3], hi[HK_BVH_MAX_BINS][3];
    int cnt[HK_BVH_MAX_BINS];
};
// axis < 0: no SAH candidate at all (every centroid extent is zero).  Otherwise the cheapest boundary (axis, then bin order, strict <):
// the triangles of bins <= split go left, n_left of them.  median: cut at count / 2 instead (no candidate, or the depth budget).
struct HkBvhSplit {
    int axis, split, n_left, median;
};

HK_BVH_HD inline void hk_bvh_grow(float lo[3], float hi[3], const float blo[3], const float bhi[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = blo[k] < lo[k] ? blo[k] : lo[k];   // std::min(lo, blo)
        hi[k] = hi[k] < bhi[k] ? bhi[k] : hi[k];   // std::max(hi, bhi)
    }
}

// The decision for a node of `count` > leaf triangles at `depth`.  bins[axis] is read only where the centroid extent of that axis
// is > 0 (an axis without extent offers no candidate and need not be binned).
HK_BVH_HD inline HkBvhSplit hk_bvh_decide(const float cb_lo[3], const float cb_hi[3], const HkBvhBins* bins, int count, int depth, int leaf, int nbins) {
    HkBvhSplit s;
    s.axis = -1, s.split = -1, s.n_left = 0, s.median = 1;
    float best_cost = __builtin_inff();
    for (int axis = 0; axis < 3; ++axis) {
        const float ext = cb_hi[axis] - cb_lo[axis];
        if (!(ext > 0)) continue;
        const HkBvhBins& B = bins[axis];
        float right_area[HK_BVH_MAX_BINS];
        int right_cnt[HK_BVH_MAX_BINS];
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) lo[k] = __builtin_inff(), hi[k] = -__builtin_inff();
        int c = 0;
        for (int b = nbins - 1; b >= 1; --b) {
            hk_bvh_grow(lo, hi, B.lo[b], B.hi[b]);
            c += B.cnt[b];
            right_area[b] = hk_bvh_half_area(lo, hi);
            right_cnt[b] = c;
        }
        for (int k = 0; k < 3; ++k) lo[k] = __builtin_inff(), hi[k] = -__builtin_inff();
        c = 0;
        for (int b = 0; b < nbins - 1; ++b) {
            hk_bvh_grow(lo, hi, B.lo[b], B.hi[b]);
            c += B.cnt[b];
            if (c == 0 || right_cnt[b + 1] == 0) continue;   // the empty-side rule
            const float cost = hk_bvh_half_area(lo, hi) * (float)c + right_area[b + 1] * (float)right_cnt[b + 1];
            if (cost < best_cost) {
                best_cost = cost;
                s.axis = axis;
                s.split = b;
                s.n_left = c;
            }
        }
    }
    if (s.axis < 0) return s;
    // depth budget: both sides must still fit with median splits
    const int nl = s.n_left, nr = count - nl, big = nl > nr ? nl : nr;
    s.median = (nl == 0 || nr == 0 || depth + 1 + hk_bvh_levels_needed(big, leaf) > HK_BVH_DEPTH_BUDGET) ? 1 : 0;
    return s;
}
