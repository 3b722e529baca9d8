// hk_nvdb_build.h — the NanoVDB tree of a dense field, built on the device (hk_scene_update_medium_dense): the bytes
// build_nanovdb_from_dense (media.py; nanovdb.jl:602-858) writes on the host, and the block table plan_nanovdb (hk_scene.cpp) derives
// from them.  Part of the hk_kernels.hip translation unit.  Everything is integer bookkeeping plus `!=`, min and max of binary32
// values: there is no float arithmetic, no float atomic, and nothing depends on the order in which lanes or blocks arrive.
//
//   k_dense_flags      one wave per 8 x 8 rows of 64 voxels along the field's fastest axis (coalesced for either layout): per 8^3 block
//                      "any voxel != 0.0f" (-0.0f is background), the blocks' bounds, the non-finite flag
//   k_dense_group      a lower node per 16^3 blocks, then an upper node per 32^3 lower nodes: any child set
//   k_dense_tile_sums, k_dense_scan_sums, k_dense_slots
//                      per level, the exclusive prefix sum of the flags in [x][y][z] order (z fastest) — the lexicographic order in
//                      which the host builder numbers leaves, lower and upper nodes — and the list of the set ones; the counts
//   ---- the host reads the counts, the bounds and the flag (the one wait), sizes the tree, and zeroes it ----
//   k_dense_leaves     one wave per leaf: origin, 7 7 7, value mask, min, max, 512 values (through LDS: lz-fastest on the way out,
//                      the field's fastest axis on the way in)
//   k_dense_nodes      one block per lower / upper node: bbox, child and value mask, child offsets; the root tiles and header
//   k_dense_table      one lane per block-table entry: the 1-based leaf offset, or 0 and the background's bits
#pragma once

__device__ __forceinline__ long long dense_index(const int dim[3], int x, int y, int z) { return (long long)z + (long long)dim[2] * ((long long)y + (long long)dim[1] * (long long)x); }

__global__ void __launch_bounds__(64) k_dense_flags(DDense D, unsigned n_chunk) {
    const int f = D.fast, a = f == 0 ? 1 : 0, b = f == 0 ? 2 : 1;   // the lanes' axis and the two axes of the 8 x 8 rows
    const int* nb = D.lev[0].dim;
    const unsigned w = blockIdx.x, chunk = w % n_chunk, r = w / n_chunk;
    const int qa = (int)(r % (unsigned)nb[a]), qb = (int)(r / (unsigned)nb[a]), lane = threadIdx.x;
    const long long c = (long long)chunk * 64 + lane;
    const bool in = c < D.res[f];
    const float* src = D.data + c * D.stride[f];
    bool any = false, bad = false;
#pragma unroll 8
    for (int row = 0; row < 64; ++row) {
        const int ia = qa * 8 + (row & 7), ib = qb * 8 + (row >> 3);
        if (in && ia < D.res[a] && ib < D.res[b]) {   // a block that sticks out of the field is padded with 0
            const float v = src[(long long)ia * D.stride[a] + (long long)ib * D.stride[b]];
            any |= v != 0.0f;
            bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        }
    }
    const unsigned long long set = __ballot(any);
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&D.ctl->nonfinite, 1);
    const int qf = (int)(c >> 3);
    if ((lane & 7) == 0 && qf < nb[f]) {
        int q[3];
        q[f] = qf, q[a] = qa, q[b] = qb;
        D.lev[0].flags[dense_index(nb, q[0], q[1], q[2])] = ((set >> lane) & 0xffull) != 0ull ? 1 : 0;
    }
    if (lane == 0 && set != 0ull) {   // integer maxima: the same whatever the order
        int lo[3], hi[3];
        lo[f] = (int)(chunk * 8u) + (__ffsll((long long)set) - 1) / 8, hi[f] = (int)(chunk * 8u) + (63 - __clzll((long long)set)) / 8;
        lo[a] = hi[a] = qa, lo[b] = hi[b] = qb;
        for (int k = 0; k < 3; ++k) atomicMax(&D.ctl->lo_enc[k], 0x7fffffff - lo[k]), atomicMax(&D.ctl->hi1[k], hi[k] + 1);
    }
}

// level `to` (1: lower nodes of 16^3 blocks, 2: upper nodes of 32^3 lower nodes) from the level below it; one wave per node
__global__ void __launch_bounds__(64) k_dense_group(DDense D, int to) {
    const DDenseLevel& P = D.lev[to];
    const DDenseLevel& C = D.lev[to - 1];
    const int S = to == 1 ? 4 : 5, lane = threadIdx.x;
    for (unsigned p = blockIdx.x; p < P.n; p += gridDim.x) {
        const int pz = (int)(p % (unsigned)P.dim[2]), py = (int)((p / (unsigned)P.dim[2]) % (unsigned)P.dim[1]), px = (int)((p / (unsigned)P.dim[2]) / (unsigned)P.dim[1]);
        bool any = false;
        for (int i = lane; i < (1 << (3 * S)); i += 64) {
            const int cx = (px << S) + (i >> (2 * S)), cy = (py << S) + ((i >> S) & ((1 << S) - 1)), cz = (pz << S) + (i & ((1 << S) - 1));
            if (cx < C.dim[0] && cy < C.dim[1] && cz < C.dim[2]) any |= C.flags[dense_index(C.dim, cx, cy, cz)] != 0;
        }
        const unsigned long long set = __ballot(any);
        if (lane == 0) P.flags[p] = set != 0ull ? 1 : 0;
    }
}

// exclusive prefix sum of one value per lane over a block of 256 (wave scans by shuffle, the four wave totals through LDS)
__device__ __forceinline__ uint32_t dense_block_scan(uint32_t v, uint32_t* wave_total, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    __syncthreads();   // (wave_total is the caller's to reuse)
    return before + incl - v;
}
// the tile of HK_DENSE_SCAN_TILE flags this block has: its level and the tile's index there (the grid is the three levels' tiles in turn)
__device__ __forceinline__ int dense_tile_level(const DDense& D, unsigned& tile) {
    int L = 0;
    tile = blockIdx.x;
    while (L < 2 && tile >= D.lev[L].tiles) tile -= D.lev[L].tiles, ++L;
    return L;
}
__device__ __forceinline__ uint32_t dense_lane_flags(const DDenseLevel& V, unsigned tile, uint32_t& first) {   // this lane's 16 flags as bits
    first = tile * (uint32_t)HK_DENSE_SCAN_TILE + threadIdx.x * 16u;
    uint32_t bits = 0;
    for (uint32_t j = 0; j < 16u; ++j)
        if (first + j < V.n && V.flags[first + j] != 0) bits |= 1u << j;
    return bits;
}
__global__ void __launch_bounds__(256) k_dense_tile_sums(DDense D) {
    __shared__ uint32_t wave_total[4];
    unsigned tile;
    const DDenseLevel& V = D.lev[dense_tile_level(D, tile)];
    uint32_t first, total;
    const uint32_t bits = dense_lane_flags(V, tile, first);
    (void)dense_block_scan((uint32_t)__popc(bits), wave_total, total);
    if (threadIdx.x == 0) V.sums[tile] = total;
}
// one block per level: the tile sums become their exclusive prefix sums, the total the level's node count
__global__ void __launch_bounds__(256) k_dense_scan_sums(DDense D) {
    __shared__ uint32_t wave_total[4];
    const DDenseLevel& V = D.lev[blockIdx.x];
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < V.tiles; t0 += 256u) {   // (every lane of the block takes every round)
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t v = t < V.tiles ? V.sums[t] : 0u;
        uint32_t total;
        const uint32_t before = dense_block_scan(v, wave_total, total);
        if (t < V.tiles) V.sums[t] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) D.ctl->count[blockIdx.x] = carry;
}
__global__ void __launch_bounds__(256) k_dense_slots(DDense D) {
    __shared__ uint32_t wave_total[4];
    unsigned tile;
    const DDenseLevel& V = D.lev[dense_tile_level(D, tile)];
    uint32_t first, total;
    const uint32_t bits = dense_lane_flags(V, tile, first);
    uint32_t slot = V.sums[tile] + dense_block_scan((uint32_t)__popc(bits), wave_total, total);
    for (uint32_t j = 0; j < 16u && first + j < V.n; ++j) {
        V.slot[first + j] = slot;
        if ((bits >> j) & 1u) V.list[slot++] = first + j;   // (slot < the level's count <= n: the list has n entries)
    }
}

// binary32 -> an integer that orders as the value does, -0.0f below +0.0f (finite values): minimum and maximum by it are exact and the
// same in any order
__device__ __forceinline__ int dense_order_key(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);   // a negative value: the magnitude bits reversed in order
}
__device__ __forceinline__ float dense_order_value(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// One wave per leaf, slot = blockIdx.x (the list is in slot order).  The 512 voxels go through LDS at (lx * 65 + ly * 8 + lz): the
// loads run along the field's fastest axis (8 voxels of 8 rows per instruction when that is z, 8 x 8 when it is x), the stores to the
// leaf are 256 contiguous bytes; the pad of one word per lx keeps both sides of the transpose off shared banks (a write of lane t
// lands on bank t mod 32 either way, a read on bank (j + t) mod 64).
__global__ void __launch_bounds__(64) k_dense_leaves(DDense D) {
    __shared__ float tile[8 * 65];
    const int* nb = D.lev[0].dim;
    const uint32_t blk = D.lev[0].list[blockIdx.x];
    const int bz = (int)(blk % (unsigned)nb[2]), by = (int)((blk / (unsigned)nb[2]) % (unsigned)nb[1]), bx = (int)((blk / (unsigned)nb[2]) / (unsigned)nb[1]);
    const int t = threadIdx.x;
    for (int j = 0; j < 8; ++j) {
        const int lx = D.fast == 0 ? (t & 7) : j, ly = t >> 3, lz = D.fast == 0 ? j : (t & 7);
        const int x = bx * 8 + lx, y = by * 8 + ly, z = bz * 8 + lz;
        float v = 0.0f;   // beyond the field: padded with the background
        if (x < D.res[0] && y < D.res[1] && z < D.res[2]) v = D.data[(long long)x * D.stride[0] + (long long)y * D.stride[1] + (long long)z * D.stride[2]];
        tile[lx * 65 + ly * 8 + lz] = v;
    }
    __syncthreads();
    unsigned char* leaf = D.tree + D.section[0] + (long long)blockIdx.x * hknv::LEAF_SIZE;
    float* values = reinterpret_cast<float*>(leaf + hknv::LEAF_VALUES);
    uint32_t* mask = reinterpret_cast<uint32_t*>(leaf + hknv::LEAF_MASK);
    int kmin = 0x7fffffff, kmax = -0x7fffffff - 1;
    for (int j = 0; j < 8; ++j) {
        const float v = tile[j * 65 + t];   // value n = j * 64 + t = (lx << 6) | (ly << 3) | lz
        values[j * 64 + t] = v;
        const unsigned long long active = __ballot(v != 0.0f);   // bits n .. n + 63 of the value mask, little-endian bytes
        if (t == 0) mask[2 * j] = (uint32_t)active, mask[2 * j + 1] = (uint32_t)(active >> 32);
        const int k = dense_order_key(v);
        kmin = k < kmin ? k : kmin, kmax = k > kmax ? k : kmax;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(kmin, d), b = __shfl_xor(kmax, d);
        kmin = a < kmin ? a : kmin, kmax = b > kmax ? b : kmax;
    }
    if (t < 3) reinterpret_cast<int*>(leaf)[t] = (t == 0 ? bx : (t == 1 ? by : bz)) * 8;
    if (t == 3) *reinterpret_cast<uint32_t*>(leaf + hknv::LEAF_FLAGS) = 0x00070707u;
    if (t == 4) *reinterpret_cast<float*>(leaf + hknv::LEAF_MIN) = dense_order_value(kmin);
    if (t == 5) *reinterpret_cast<float*>(leaf + hknv::LEAF_MIN + 4) = dense_order_value(kmax);
}

// One block per node of level LEVEL (1 lower, 2 upper), slot = blockIdx.x: the bbox, a bit of the child mask and of the value mask and
// the offset from this node for every child there is; entries without a child stay 0 (tile value 0 = the background, inactive).  An
// upper node also writes its root tile, and the first one the root header.
template <int LEVEL>
__global__ void __launch_bounds__(256) k_dense_nodes(DDense D) {
    constexpr int S = LEVEL == 1 ? 4 : 5, SPAN = LEVEL == 1 ? 128 : 4096;   // children per axis (log2), voxels per axis
    constexpr long long SIZE = LEVEL == 1 ? hknv::LOWER_SIZE : hknv::UPPER_SIZE, CHILD_SIZE = LEVEL == 1 ? hknv::LEAF_SIZE : hknv::LOWER_SIZE;
    constexpr long long TABLE = LEVEL == 1 ? hknv::LOWER_TABLE : hknv::UPPER_TABLE, CHILDMASK = LEVEL == 1 ? hknv::LOWER_CHILDMASK : hknv::UPPER_CHILDMASK;
    constexpr long long VALUEMASK = LEVEL == 1 ? hknv::LOWER_VALUEMASK : hknv::UPPER_VALUEMASK;
    const DDenseLevel& P = D.lev[LEVEL];
    const DDenseLevel& C = D.lev[LEVEL - 1];
    const uint32_t p = P.list[blockIdx.x];
    const int pz = (int)(p % (unsigned)P.dim[2]), py = (int)((p / (unsigned)P.dim[2]) % (unsigned)P.dim[1]), px = (int)((p / (unsigned)P.dim[2]) / (unsigned)P.dim[1]);
    const long long at = D.section[LEVEL] + (long long)blockIdx.x * SIZE;   // this node's position in the tree
    unsigned char* node = D.tree + at;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 6) reinterpret_cast<int*>(node)[tid] = (tid % 3 == 0 ? px : (tid % 3 == 1 ? py : pz)) * SPAN + (tid < 3 ? 0 : SPAN - 1);
    for (int n = tid; n < (1 << (3 * S)); n += 256) {   // entry n = (cx << 2S) | (cy << S) | cz; a wave has 64 consecutive entries: one mask word
        const int cx = (px << S) + (n >> (2 * S)), cy = (py << S) + ((n >> S) & ((1 << S) - 1)), cz = (pz << S) + (n & ((1 << S) - 1));
        bool child = false;
        long long ci = 0;
        if (cx < C.dim[0] && cy < C.dim[1] && cz < C.dim[2]) ci = dense_index(C.dim, cx, cy, cz), child = C.flags[ci] != 0;
        const unsigned long long set = __ballot(child);
        if (lane == 0 && set != 0ull) {
            uint32_t* cm = reinterpret_cast<uint32_t*>(node + CHILDMASK) + 2 * (n >> 6);
            uint32_t* vm = reinterpret_cast<uint32_t*>(node + VALUEMASK) + 2 * (n >> 6);
            cm[0] = vm[0] = (uint32_t)set, cm[1] = vm[1] = (uint32_t)(set >> 32);
        }
        if (child) reinterpret_cast<long long*>(node + TABLE)[n] = D.section[LEVEL - 1] + (long long)C.slot[ci] * CHILD_SIZE - at;
    }
    if (LEVEL == 2 && tid == 0) {
        unsigned char* tile = D.tree + hknv::ROOT_HEADER + (long long)blockIdx.x * hknv::ROOT_TILE;
        // the key of nanovdb.jl's coord_to_key for the node's origin (px, py, pz) * 4096: 21 bits per axis, z lowest
        *reinterpret_cast<unsigned long long*>(tile) = ((unsigned long long)pz & 0x1fffffull) | (((unsigned long long)py & 0x1fffffull) << 21) | (((unsigned long long)px & 0x1fffffull) << 42);
        *reinterpret_cast<long long*>(tile + 8) = at;   // from the root, which is at 0
        *reinterpret_cast<uint32_t*>(tile + 16) = 1u;
        if (blockIdx.x == 0) {
            int* head = reinterpret_cast<int*>(D.tree);
            for (int k = 0; k < 3; ++k) head[k] = D.index_min[k], head[3 + k] = D.index_max[k];
            reinterpret_cast<uint32_t*>(D.tree)[6] = gridDim.x;   // the table size = the number of upper nodes; the background (0.0f) is the zeroed word after it
        }
    }
}

// the block table of plan_nanovdb for this tree: entry (bx, by, bz) of the extent, bz fastest, = {1-based leaf offset, 0} for a block
// that is a leaf, {0, bits of the background 0.0f} for every other one
__global__ void __launch_bounds__(256) k_dense_table(DDense D, unsigned long long n) {
    const int* nb = D.lev[0].dim;
    const unsigned long long d1 = (unsigned long long)D.nvb_dim[1], d2 = (unsigned long long)D.nvb_dim[2];
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (unsigned long long)gridDim.x * 256) {
        const long long bz = D.nvb_min[2] + (long long)(e % d2), by = D.nvb_min[1] + (long long)((e / d2) % d1), bx = D.nvb_min[0] + (long long)((e / d2) / d1);
        uint32_t leaf = 0u;
        if (bx >= 0 && by >= 0 && bz >= 0 && bx < nb[0] && by < nb[1] && bz < nb[2]) {
            const long long i = dense_index(nb, (int)bx, (int)by, (int)bz);
            if (D.lev[0].flags[i] != 0) leaf = (uint32_t)(D.section[0] + (long long)D.lev[0].slot[i] * hknv::LEAF_SIZE + 1);
        }
        D.table[e] = make_uint2(leaf, 0u);
    }
}
