// Host-only check of hikari.jl_amd/csrc/hk_bvh_decide.h (built by tests/test_bvh_rebuild_host.py with g++, plain and under
// AddressSanitizer + UBSan): the device builder's algorithm written sequentially — level by level over segments of an index array, bins
// accumulated in REVERSE triangle order (the decision must not depend on the order), hk_bvh_decide per segment, a stable partition,
// children numbered breadth-first by a running count, a median fallback that cuts the segment where it is — and held to the host
// builder (bvh_build.cpp, linked in): where neither takes a median split, the same node count, depth, child references and the same
// triangles in every leaf; otherwise every triangle in one leaf, the depth inside the budget, and whether the references agree is
// reported (they do when every median split is one of coincident centroids: both sides of such a node are split by count alone).  Prints the order-free topology digest of tests/native/bvh_tree_digest.cpp for the caller to compare
// with the recorded one.   usage: bvh_decide_check <positions.f32> <leaf size> <bins>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "bvh_build.h"
#include "hk_bvh_decide.h"

#define CHECK(c)                                            \
    if (!(c)) {                                             \
        std::printf("FAILED %s (line %d)\n", #c, __LINE__); \
        return 1;                                           \
    }

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
struct Seg {
    int first, count;
};
struct Node {
    int c0, c1;
};

static uint64_t topology(const std::vector<Node>& nodes, const std::vector<int>& prims) {
    uint64_t h = 14695981039346656037ull;
    for (const Node& nd : nodes)
        for (int ref : {nd.c0, nd.c1}) {
            h = fnv(h, &ref, sizeof ref);
            if (ref >= 0) continue;
            const int first = (~ref) >> 3, count = ((~ref) & 7) + 1;
            std::vector<int> p(prims.begin() + first, prims.begin() + first + count);
            std::sort(p.begin(), p.end());
            h = fnv(h, p.data(), p.size() * sizeof(int));
        }
    return h;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> pos;
    float buf[4096];
    for (size_t got; (got = std::fread(buf, sizeof(float), 4096, f)) > 0;) pos.insert(pos.end(), buf, buf + got);
    std::fclose(f);
    CHECK(pos.size() % 9 == 0);
    const int T = (int)(pos.size() / 9), leaf = hk_bvh_leaf_size(std::atoi(argv[2])), nbins = hk_bvh_bin_count(std::atoi(argv[3]));
    CHECK(T > leaf);
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> tbox(6 * (size_t)T);
    for (int t = 0; t < T; ++t) {
        float* b = &tbox[6 * (size_t)t];
        for (int k = 0; k < 3; ++k) b[k] = inf, b[3 + k] = -inf;
        for (int v = 0; v < 9; ++v) b[v % 3] = std::min(b[v % 3], pos[9 * (size_t)t + v]), b[3 + v % 3] = std::max(b[3 + v % 3], pos[9 * (size_t)t + v]);
    }
    std::vector<int> idx[2] = {std::vector<int>(T), std::vector<int>(T)}, order(T, -1);
    for (int t = 0; t < T; ++t) idx[0][t] = t;
    std::vector<Seg> segs{{0, T}};
    std::vector<Node> nodes;
    int depth = 0, medians = 0, node0 = 0;
    for (int L = 0; L < HK_BVH_MAX_LEVELS && !segs.empty(); ++L) {
        const std::vector<int>& in = idx[L & 1];
        std::vector<int>& out = idx[(L + 1) & 1];
        std::vector<Seg> next;
        const int child0 = node0 + (int)segs.size();
        depth = L + 1;
        for (const Seg& s : segs) {
            float cb_lo[3] = {inf, inf, inf}, cb_hi[3] = {-inf, -inf, -inf};
            auto cent = [&](int t, int a) { return 0.5f * (tbox[6 * (size_t)t + a] + tbox[6 * (size_t)t + 3 + a]); };
            for (int i = s.count - 1; i >= 0; --i)
                for (int a = 0; a < 3; ++a) cb_lo[a] = std::min(cb_lo[a], cent(in[s.first + i], a)), cb_hi[a] = std::max(cb_hi[a], cent(in[s.first + i], a));
            static HkBvhBins bins[3];
            for (int a = 0; a < 3; ++a) {
                const float ext = cb_hi[a] - cb_lo[a];
                if (!(ext > 0)) continue;
                for (int b = 0; b < nbins; ++b) {
                    for (int k = 0; k < 3; ++k) bins[a].lo[b][k] = inf, bins[a].hi[b][k] = -inf;
                    bins[a].cnt[b] = 0;
                }
                const float scale = hk_bvh_bin_scale(ext, nbins);
                for (int i = s.count - 1; i >= 0; --i) {
                    const int t = in[s.first + i], b = hk_bvh_bin_of(cent(t, a), cb_lo[a], scale, nbins);
                    CHECK(b >= 0 && b < nbins);
                    hk_bvh_grow(bins[a].lo[b], bins[a].hi[b], &tbox[6 * (size_t)t], &tbox[6 * (size_t)t + 3]);
                    bins[a].cnt[b]++;
                }
            }
            const HkBvhSplit sp = hk_bvh_decide(cb_lo, cb_hi, bins, s.count, L, leaf, nbins);
            int nl;
            if (sp.median) {
                ++medians;
                nl = s.count / 2;
                for (int i = 0; i < s.count; ++i) out[s.first + i] = in[s.first + i];
            } else {
                CHECK(sp.axis >= 0 && sp.axis < 3 && sp.split >= 0 && sp.split < nbins - 1);
                nl = sp.n_left;
                const float scale = hk_bvh_bin_scale(cb_hi[sp.axis] - cb_lo[sp.axis], nbins);
                int l = 0, r = 0;
                for (int i = 0; i < s.count; ++i) {
                    const int t = in[s.first + i];
                    if (hk_bvh_bin_of(cent(t, sp.axis), cb_lo[sp.axis], scale, nbins) <= sp.split) out[s.first + l++] = t;
                    else {
                        CHECK(nl + r < s.count);
                        out[s.first + nl + r++] = t;
                    }
                }
                CHECK(l == nl && l + r == s.count);   // the bin counts are the partition's sizes
            }
            CHECK(nl >= 1 && s.count - nl >= 1);
            CHECK(L + 1 + hk_bvh_levels_needed(std::max(nl, s.count - nl), leaf) <= HK_BVH_DEPTH_BUDGET);
            Node nd;
            for (int c = 0; c < 2; ++c) {
                const int cf = c ? s.first + nl : s.first, cn = c ? s.count - nl : nl;
                int ref;
                if (cn > leaf) {
                    ref = child0 + (int)next.size();
                    next.push_back({cf, cn});
                } else {
                    ref = ~((cf << 3) | (cn - 1));
                    for (int i = 0; i < cn; ++i) order[cf + i] = out[cf + i];
                }
                (c ? nd.c1 : nd.c0) = ref;
            }
            nodes.push_back(nd);
        }
        node0 = child0;
        segs.swap(next);
    }
    CHECK(segs.empty());
    std::vector<int> seen(T, 0);
    for (int i = 0; i < T; ++i) {
        CHECK(order[i] >= 0 && order[i] < T);
        ++seen[order[i]];
    }
    for (int t = 0; t < T; ++t) CHECK(seen[t] == 1);
    // against the host builder
    hk::BVH bvh;
    hk::build_bvh(pos.data(), T, bvh, leaf, nbins);
    CHECK(depth <= HK_BVH_DEPTH_BUDGET && bvh.max_depth <= HK_BVH_DEPTH_BUDGET);
    CHECK((bvh.median_splits == 0) == (medians == 0));   // (the first median split of either builder is taken at the same node)
    bool refs_equal = bvh.nodes.size() == nodes.size() && bvh.max_depth == depth;
    for (size_t i = 0; refs_equal && i < nodes.size(); ++i) refs_equal = bvh.nodes[i].c0 == nodes[i].c0 && bvh.nodes[i].c1 == nodes[i].c1;
    std::vector<Node> host_nodes(bvh.nodes.size());
    for (size_t i = 0; i < bvh.nodes.size(); ++i) host_nodes[i] = {bvh.nodes[i].c0, bvh.nodes[i].c1};
    const uint64_t mine = topology(nodes, order), host = topology(host_nodes, bvh.leaf_prims);
    if (medians == 0) CHECK(refs_equal && mine == host);
    std::printf("{\"triangles\": %d, \"nodes\": %zu, \"depth\": %d, \"topology_fnv\": \"%016llx\", \"host_topology_fnv\": \"%016llx\", \"medians\": %d, \"host_medians\": %d, \"refs_equal\": %s}\n", T,
                nodes.size(), depth, (unsigned long long)mine, (unsigned long long)host, medians, bvh.median_splits, refs_equal ? "true" : "false");
    return 0;
}
