// Digest of the host builder's tree (hikari.jl_amd/csrc/bvh_build.cpp), built with g++ by tools/bvh_tree_digest.py and by
// tests/test_bvh_rebuild_host.py: FNV-1a 64 of the node array as build_bvh leaves it (boxes and child references, byte for byte) and of
// leaf_prims, plus an order-free digest of the topology (child references, and the SORTED triangle indices of every leaf) that a
// builder with another order inside a leaf can be held to.   usage: bvh_tree_digest <positions.f32> <leaf size> <bins>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bvh_build.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
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
    if (pos.size() % 9 != 0) return 2;
    const int n = (int)(pos.size() / 9);
    hk::BVH bvh;
    hk::build_bvh(pos.data(), n, bvh, std::atoi(argv[2]), std::atoi(argv[3]));
    static_assert(sizeof(hk::BVHNode) == 56, "BVHNode has no padding: its bytes are its fields");
    const uint64_t seed = 14695981039346656037ull;
    const uint64_t h_nodes = fnv(seed, bvh.nodes.data(), bvh.nodes.size() * sizeof(hk::BVHNode));
    const uint64_t h_prims = fnv(seed, bvh.leaf_prims.data(), bvh.leaf_prims.size() * sizeof(int));
    uint64_t h_topo = seed;
    for (const hk::BVHNode& nd : bvh.nodes)
        for (int ref : {nd.c0, nd.c1}) {
            h_topo = fnv(h_topo, &ref, sizeof ref);
            if (ref >= 0) continue;
            const int first = (~ref) >> 3, count = ((~ref) & 7) + 1;
            std::vector<int> prims(bvh.leaf_prims.begin() + first, bvh.leaf_prims.begin() + first + count);
            std::sort(prims.begin(), prims.end());
            h_topo = fnv(h_topo, prims.data(), prims.size() * sizeof(int));
        }
    int medians = -1;
#ifdef HK_BVH_COUNTS_MEDIANS
    medians = bvh.median_splits;
#endif
    std::printf("{\"triangles\": %d, \"nodes\": %zu, \"depth\": %d, \"nodes_fnv\": \"%016llx\", \"prims_fnv\": \"%016llx\", \"topology_fnv\": \"%016llx\", \"medians\": %d}\n", n, bvh.nodes.size(),
                bvh.max_depth, (unsigned long long)h_nodes, (unsigned long long)h_prims, (unsigned long long)h_topo, medians);
    return 0;
}
