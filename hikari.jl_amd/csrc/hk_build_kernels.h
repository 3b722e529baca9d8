// hk_build_kernels.h — the device BVH builder: build_key, k_build_init, k_build_large_bounds / k_build_large_bins, k_build_split, k_build_emit, k_build_leaves.
// Part of the hk_kernels.hip translation unit (needs hk_bvh_decide.h, the host builder's own split decision, hk_edit_host.h: hk_pack_leaf_tri; hk_edit_kernels.h: grow_lo / grow_hi).
#pragma once

// ---------------------------------------------------------------------------------------------------
// BVH REBUILD (hk_scene_rebuild_bvh): the topology hk_scene_create's host builder (bvh_build.cpp) would give the world positions the
// device holds, built level by level, top-down.  A level's inner nodes are SEGMENTS of an index array (DBuildSeg); per level:
//   k_build_large_bounds / k_build_large_bins   the centroid box and the SAH bins of the segments larger than HK_BVH_BUILD_SMALL, by
//                                               every block whose positions they cover: reduced in LDS, combined across blocks with
//                                               integer atomics on ordered keys (min / max) and integer adds
//   k_build_split                               one block per segment: smaller segments are bounded and binned entirely in LDS; the
//                                               decision (hk_bvh_decide, the host builder's own); the stable partition by ballots
//                                               and a block scan into the other index array
//   k_build_emit                                ONE block: prefix sums over the level give the children their breadth-first numbers
//                                               (the host's renumbering order: left child first), the child references, the next
//                                               level's segments and the final slots of the leaves
// Minima, maxima and counts do not depend on arrival order and nothing is compacted with atomics: two builds give the same bits.
// The host launches all HK_BUILD_MAX_LEVELS levels without looking (a level without segments returns at once) and reads DBuildCtl
// back once.  Boxes are not written here: k_refit_level computes them from the topology and the leaf order.
// A segment of 10^6 triangles is partitioned by ONE block (tile after tile); spreading it over several is future work.
// ---------------------------------------------------------------------------------------------------
static_assert(HK_BUILD_MAX_LEVELS == HK_BVH_MAX_LEVELS && HK_BUILD_BIN_WORDS == 3 * HK_BVH_MAX_BINS * 7 && HK_BVH_MAX_BINS == 64,
              "hk_types.h and hk_bvh_decide.h describe one builder: the bin words are indexed (axis * 64 + bin) * 7 below");
#define HK_KEY_PINF 0x7f800000          // build_key(+inf)
#define HK_KEY_NINF ((int)0x807fffff)   // build_key(-inf)
// a monotone map binary32 -> int (its own inverse): integer min / max of keys is min / max of the floats (-0 sorts below +0)
__device__ inline int build_key(float f) {
    const int k = __float_as_int(f);
    return k >= 0 ? k : k ^ 0x7fffffff;
}
__device__ inline float build_val(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ void __launch_bounds__(256) k_build_init(DBuild B) {
    const int T = B.n_tris;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < T; i += gridDim.x * blockDim.x) {
        const float* p = B.pos + 9 * (size_t)i;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int v = 0; v < 9; ++v) lo[v % 3] = grow_lo(lo[v % 3], p[v]), hi[v % 3] = grow_hi(hi[v % 3], p[v]);
        for (int k = 0; k < 3; ++k) B.tbox[6 * (size_t)i + k] = lo[k], B.tbox[6 * (size_t)i + 3 + k] = hi[k];
        B.idx[0][i] = i, B.idx[1][i] = i, B.order[i] = i;   // (every entry a triangle index from the start)
    }
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < (long long)B.large_cap * HK_BUILD_BIN_WORDS; w += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(w % 7);
        B.large_bins[w] = f < 3 ? HK_KEY_PINF : (f < 6 ? HK_KEY_NINF : 0);
    }
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < B.large_cap * 6; w += gridDim.x * blockDim.x) B.large_cb[w] = w % 6 < 3 ? HK_KEY_PINF : HK_KEY_NINF;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // level 0: the root (the host does not build a scene whose root is a leaf)
        DBuildCtl& C = *B.ctl;
        for (int L = 0; L <= HK_BUILD_MAX_LEVELS; ++L) C.n_seg[L] = 0, C.n_large[L] = 0;
        for (int L = 0; L <= HK_BUILD_MAX_LEVELS + 1; ++L) C.level_start[L] = 0;
        const bool large = T > B.small_max && B.large_cap > 0;
        C.n_seg[0] = 1, C.n_large[0] = large ? 1 : 0, C.level_start[1] = 1, C.n_nodes = 0, C.depth = 0;
        DBuildSeg root;
        root.first = 0, root.count = T, root.large = large ? 0 : -1, root.pad = 0;
        B.seg[0][0] = root;
        B.large[0][0] = 0;
    }
}

// the large segment of level L that holds position i of the index array (its slot in the bin storage), or -1
__device__ inline int build_find_large(const DBuild& B, int L, int n_large, int i) {
    const DBuildSeg* segs = B.seg[L & 1];
    const int* large = B.large[L & 1];
    int lo = 0, hi = n_large - 1;
    if (hi < 0 || segs[large[0]].first > i) return -1;
    while (lo < hi) {   // the last one that starts at or before i
        const int mid = (lo + hi + 1) >> 1;
        if (segs[large[mid]].first <= i) lo = mid;
        else hi = mid - 1;
    }
    const DBuildSeg s = segs[large[lo]];
    return i < s.first + s.count ? lo : -1;
}
__device__ inline void build_centroid(const float* tb, float c[3]) {
    for (int k = 0; k < 3; ++k) c[k] = 0.5f * (tb[k] + tb[3 + k]);   // the host's expression
}

// Centroid boxes of the large segments.  A block's 256 positions mostly lie in one segment (that of its first position): those are
// reduced in LDS and leave the block as six atomics; positions of another segment go to memory directly.
__global__ void __launch_bounds__(256) k_build_large_bounds(DBuild B, int L) {
    __shared__ int acc[6];
    __shared__ int k0;
    const int n_large = B.ctl->n_large[L];
    if (n_large == 0) return;
    const int* in = B.idx[L & 1];
    for (int base = blockIdx.x * 256; base < B.n_tris; base += gridDim.x * 256) {
        const int i = base + (int)threadIdx.x;
        const int k = i < B.n_tris ? build_find_large(B, L, n_large, i) : -1;
        if (threadIdx.x == 0) k0 = k;
        if (threadIdx.x < 6) acc[threadIdx.x] = threadIdx.x < 3 ? HK_KEY_PINF : HK_KEY_NINF;
        __syncthreads();
        if (k >= 0) {
            float c[3];
            build_centroid(B.tbox + 6 * (size_t)in[i], c);
            int* dst = k == k0 ? acc : B.large_cb + 6 * (size_t)k;
            for (int a = 0; a < 3; ++a) atomicMin(dst + a, build_key(c[a])), atomicMax(dst + 3 + a, build_key(c[a]));
        }
        __syncthreads();
        if (threadIdx.x < 6 && k0 >= 0) {
            if (threadIdx.x < 3) atomicMin(B.large_cb + 6 * (size_t)k0 + threadIdx.x, acc[threadIdx.x]);
            else atomicMax(B.large_cb + 6 * (size_t)k0 + threadIdx.x, acc[threadIdx.x]);
        }
        __syncthreads();
    }
}

// one triangle into the bins of every axis with extent: words (axis * 64 + bin) * 7 + (lo[3], hi[3], count)
__device__ inline void build_bin_tri(int* bins, const float* tb, const float cb_lo[3], const float cb_hi[3], int nbins) {
    float c[3];
    build_centroid(tb, c);
    for (int a = 0; a < 3; ++a) {
        const float ext = cb_hi[a] - cb_lo[a];
        if (!(ext > 0)) continue;
        const int b = hk_bvh_bin_of(c[a], cb_lo[a], hk_bvh_bin_scale(ext, nbins), nbins);
        int* w = bins + (a * 64 + b) * 7;
        for (int k = 0; k < 3; ++k) atomicMin(w + k, build_key(tb[k])), atomicMax(w + 3 + k, build_key(tb[3 + k]));
        atomicAdd(w + 6, 1);
    }
}

__global__ void __launch_bounds__(256) k_build_large_bins(DBuild B, int L) {
    __shared__ int acc[HK_BUILD_BIN_WORDS];
    __shared__ int k0;
    const int n_large = B.ctl->n_large[L];
    if (n_large == 0) return;
    const int* in = B.idx[L & 1];
    for (int base = blockIdx.x * 256; base < B.n_tris; base += gridDim.x * 256) {
        const int i = base + (int)threadIdx.x;
        const int k = i < B.n_tris ? build_find_large(B, L, n_large, i) : -1;
        if (threadIdx.x == 0) k0 = k;
        for (int w = threadIdx.x; w < HK_BUILD_BIN_WORDS; w += 256) acc[w] = w % 7 < 3 ? HK_KEY_PINF : (w % 7 < 6 ? HK_KEY_NINF : 0);
        __syncthreads();
        if (k >= 0) {
            float lo[3], hi[3];
            for (int a = 0; a < 3; ++a) lo[a] = build_val(B.large_cb[6 * (size_t)k + a]), hi[a] = build_val(B.large_cb[6 * (size_t)k + 3 + a]);
            build_bin_tri(k == k0 ? acc : B.large_bins + (size_t)k * HK_BUILD_BIN_WORDS, B.tbox + 6 * (size_t)in[i], lo, hi, B.nbins);
        }
        __syncthreads();
        if (k0 >= 0) {
            int* dst = B.large_bins + (size_t)k0 * HK_BUILD_BIN_WORDS;
            for (int w = threadIdx.x; w < HK_BUILD_BIN_WORDS; w += 256) {
                const int f = w % 7, v = acc[w];
                if (f < 3) { if (v != HK_KEY_PINF) atomicMin(dst + w, v); }
                else if (f < 6) { if (v != HK_KEY_NINF) atomicMax(dst + w, v); }
                else if (v != 0) atomicAdd(dst + w, v);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_build_split(DBuild B, int L) {
    __shared__ int bins_i[HK_BUILD_BIN_WORDS];
    __shared__ HkBvhBins bins[3];
    __shared__ int cb_i[6];
    __shared__ float cb[6];
    __shared__ HkBvhSplit sp;
    __shared__ int wave_n[2][4];
    const int n_seg = B.ctl->n_seg[L];
    const int* in = B.idx[L & 1];
    int* out = B.idx[(L + 1) & 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nbins = B.nbins;
    for (int j = blockIdx.x; j < n_seg; j += gridDim.x) {   // (j is the block's: every barrier below is taken by all of it)
        const DBuildSeg seg = B.seg[L & 1][j];
        const int first = seg.first, count = seg.count;
        if (seg.large < 0) {
            for (int w = tid; w < HK_BUILD_BIN_WORDS; w += 256) bins_i[w] = w % 7 < 3 ? HK_KEY_PINF : (w % 7 < 6 ? HK_KEY_NINF : 0);
            if (tid < 6) cb_i[tid] = tid < 3 ? HK_KEY_PINF : HK_KEY_NINF;
            __syncthreads();
            for (int i = tid; i < count; i += 256) {
                float c[3];
                build_centroid(B.tbox + 6 * (size_t)in[first + i], c);
                for (int a = 0; a < 3; ++a) atomicMin(cb_i + a, build_key(c[a])), atomicMax(cb_i + 3 + a, build_key(c[a]));
            }
            __syncthreads();
            if (tid < 6) cb[tid] = build_val(cb_i[tid]);
            __syncthreads();
            for (int i = tid; i < count; i += 256) build_bin_tri(bins_i, B.tbox + 6 * (size_t)in[first + i], cb, cb + 3, nbins);
        } else {   // binned by the two kernels before this one; the storage is handed back as it was found
            int* g_cb = B.large_cb + 6 * (size_t)seg.large;
            int* g_bins = B.large_bins + (size_t)seg.large * HK_BUILD_BIN_WORDS;
            if (tid < 6) {
                cb[tid] = build_val(g_cb[tid]);
                g_cb[tid] = tid < 3 ? HK_KEY_PINF : HK_KEY_NINF;
            }
            for (int w = tid; w < HK_BUILD_BIN_WORDS; w += 256) {
                bins_i[w] = g_bins[w];
                g_bins[w] = w % 7 < 3 ? HK_KEY_PINF : (w % 7 < 6 ? HK_KEY_NINF : 0);
            }
        }
        __syncthreads();
        for (int w = tid; w < 3 * 64; w += 256) {
            const int a = w >> 6, b = w & 63;
            const int* src = bins_i + w * 7;
            for (int k = 0; k < 3; ++k) bins[a].lo[b][k] = build_val(src[k]), bins[a].hi[b][k] = build_val(src[3 + k]);
            bins[a].cnt[b] = src[6];
        }
        __syncthreads();
        if (tid == 0) sp = hk_bvh_decide(cb, cb + 3, bins, count, L, B.leaf, nbins);
        __syncthreads();
        const bool median = sp.median != 0;
        const int n_left = median ? count / 2 : sp.n_left;
        if (median) {   // the segment as it is, cut at count / 2 (hk_bvh_decide.h: MEDIAN FALLBACK)
            for (int i = tid; i < count; i += 256) out[first + i] = in[first + i];
        } else {
            const int axis = sp.axis;
            const float lo = cb[axis], scale = hk_bvh_bin_scale(cb[3 + axis] - cb[axis], nbins);
            int done_l = 0, done_r = 0;
            for (int i0 = 0; i0 < count; i0 += 256) {
                const int i = i0 + tid;
                const bool valid = i < count;
                int t = 0;
                bool left = false;
                if (valid) {
                    t = in[first + i];
                    const float* tb = B.tbox + 6 * (size_t)t;
                    left = hk_bvh_bin_of(0.5f * (tb[axis] + tb[3 + axis]), lo, scale, nbins) <= sp.split;
                }
                const unsigned long long ml = __ballot(valid && left), mr = __ballot(valid && !left);
                const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
                if (lane == 0) wave_n[0][wave] = __popcll(ml), wave_n[1][wave] = __popcll(mr);
                __syncthreads();
                int pre_l = 0, pre_r = 0, tot_l = 0, tot_r = 0;
                for (int w = 0; w < 4; ++w) {
                    if (w < wave) pre_l += wave_n[0][w], pre_r += wave_n[1][w];
                    tot_l += wave_n[0][w], tot_r += wave_n[1][w];
                }
                if (valid) {   // (the bin counts and this predicate are one expression: the slot is inside the segment; checked all the same)
                    const int slot = left ? done_l + pre_l + __popcll(ml & below) : n_left + done_r + pre_r + __popcll(mr & below);
                    if (slot >= 0 && slot < count) out[first + slot] = t;
                }
                done_l += tot_l, done_r += tot_r;
                __syncthreads();
            }
        }
        if (tid == 0) B.n_left[j] = n_left;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(1024) k_build_emit(DBuild B, int L) {
    __shared__ int wave_n[2][16];
    __shared__ int carry[2];
    DBuildCtl& C = *B.ctl;
    const int n_seg = C.n_seg[L];
    if (n_seg == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node0 = C.level_start[L], child0 = C.level_start[L + 1];
    const DBuildSeg* segs = B.seg[L & 1];
    DBuildSeg* next = B.seg[(L + 1) & 1];
    int* next_large = B.large[(L + 1) & 1];
    const int* order_src = B.idx[(L + 1) & 1];
    if (tid == 0) carry[0] = 0, carry[1] = 0;
    __syncthreads();
    for (int j0 = 0; j0 < n_seg; j0 += 1024) {
        const int j = j0 + tid;
        const bool valid = j < n_seg;
        DBuildSeg s{};
        int nl = 0, nr = 0;
        if (valid) s = segs[j], nl = B.n_left[j], nr = s.count - nl;
        const bool in_l = valid && nl > B.leaf, in_r = valid && nr > B.leaf;
        const bool big_l = in_l && nl > B.small_max, big_r = in_r && nr > B.small_max;
        // exclusive prefix over the level, left child before right: inner children (their node numbers), large ones (their bin slots)
        int mine_n = (in_l ? 1 : 0) + (in_r ? 1 : 0), mine_b = (big_l ? 1 : 0) + (big_r ? 1 : 0);
        int scan_n = mine_n, scan_b = mine_b;
        for (int d = 1; d < 64; d <<= 1) {
            const int un = __shfl_up(scan_n, d), ub = __shfl_up(scan_b, d);
            if (lane >= d) scan_n += un, scan_b += ub;
        }
        if (lane == 63) wave_n[0][wave] = scan_n, wave_n[1][wave] = scan_b;
        __syncthreads();
        int pre_n = carry[0], pre_b = carry[1], tot_n = 0, tot_b = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) pre_n += wave_n[0][w], pre_b += wave_n[1][w];
            tot_n += wave_n[0][w], tot_b += wave_n[1][w];
        }
        pre_n += scan_n - mine_n, pre_b += scan_b - mine_b;
        if (valid) {
            int ref[2];
            for (int c = 0; c < 2; ++c) {
                const int cf = c ? s.first + nl : s.first, cn = c ? nr : nl;
                const bool inner = c ? in_r : in_l, big = c ? big_r : big_l;
                if (inner) {
                    const int r = pre_n + (c && in_l ? 1 : 0);
                    int slot = big ? pre_b + (c && big_l ? 1 : 0) : -1;
                    if (slot >= B.large_cap) slot = -1;   // (cannot happen: large segments are disjoint and larger than small_max; such a one would be binned in LDS)
                    DBuildSeg ns;
                    ns.first = cf, ns.count = cn, ns.large = slot, ns.pad = 0;
                    next[r] = ns;
                    if (slot >= 0) next_large[slot] = r;
                    ref[c] = child0 + r;
                } else {   // a leaf: its slots are its place in the index array (the host's leaf_prims grows in the same order)
                    ref[c] = ~((cf << 3) | (cn - 1));
                    for (int i = 0; i < cn; ++i) B.order[cf + i] = order_src[cf + i];
                }
            }
            DNode* nd = B.nodes + node0 + j;
            nd->c0 = ref[0], nd->c1 = ref[1], nd->pad0 = 0, nd->pad1 = 0;
            if (B.qnodes) B.qnodes[node0 + j].c0 = ref[0], B.qnodes[node0 + j].c1 = ref[1];
        }
        __syncthreads();
        if (tid == 0) carry[0] += tot_n, carry[1] += tot_b;
        __syncthreads();
    }
    if (tid == 0) {
        C.n_seg[L + 1] = carry[0];
        C.n_large[L + 1] = carry[1] < B.large_cap ? carry[1] : B.large_cap;
        C.level_start[L + 2] = child0 + carry[0];
        C.n_nodes = child0;
        C.depth = L + 1;
    }
}

// the new leaf records from the positions, in the new order; prim and flag words from the triangle's old slot
__global__ void __launch_bounds__(256) k_build_leaves(DBuildLeaves A) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n_tris; i += gridDim.x * blockDim.x) {
        const int prim = A.order[i];
        const float4* O = A.old_leaf + 3 * (size_t)A.old_slot_of_prim[prim];
        float p[9];
        for (int v = 0; v < 9; ++v) p[v] = A.pos[9 * (size_t)prim + v];
        hk_pack_leaf_tri(A.leaf + 3 * (size_t)i, p, O[0].w, O[1].w, O[2].w);
        if (A.slot_of_prim) A.slot_of_prim[prim] = i;
    }
}
