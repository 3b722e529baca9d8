// hk_edit_kernels.h — the scene edits: k_slot_of_prim, k_tri_geo, k_xform_tris, k_refit_level, k_set_tris, the light-BVH refit
// k_light_refit_leaves / k_light_refit_level and the tree cost k_bvh_cost.
// Part of the hk_kernels.hip translation unit (needs hk_device.h, hk_edit_host.h and hk_light_bounds.h: the arithmetic the host applies to the same arrays).
#pragma once

// ---------------------------------------------------------------------------------------------------
// SCENE EDITS (hk_scene_set_transform).  k_xform_tris rewrites the geometry of a triangle range from the base copies (the arrays as
// created), k_refit_level recomputes the child boxes of one breadth-first level of the unchanged topology — launched deepest level first,
// so the kernel boundary makes the level below visible to every CU.  Binary32 without contraction, the order of the header.
// ---------------------------------------------------------------------------------------------------
__global__ void k_slot_of_prim(const float4* __restrict__ leaf_tris, int n, int* __restrict__ slot_of_prim) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) slot_of_prim[__float_as_int(leaf_tris[3 * (size_t)i].w)] = i;
}

// n' = (N[k][0]*x + N[k][1]*y) + N[k][2]*z, then n' / sqrt((x*x + y*y) + z*z); a NaN vector (no normal) is copied
__device__ inline void xform_dir(const float* M, int stride, const float* in, float* out) {
    const float x = in[0], y = in[1], z = in[2];
    if (x != x || y != y || z != z) {
        out[0] = x, out[1] = y, out[2] = z;
        return;
    }
    float r[3];
    for (int k = 0; k < 3; ++k) r[k] = (M[stride * k] * x + M[stride * k + 1] * y) + M[stride * k + 2] * z;
    const float len = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    for (int k = 0; k < 3; ++k) out[k] = r[k] / len;
}

// THE PER-TRIANGLE GEOMETRY TABLE (DScene::tri_geo): a row is written by whoever writes the triangle's positions — k_tri_geo for a
// whole scene at hk_scene_create, k_xform_tris and k_set_tris for the rows they rewrite — through tri_geo_of, the function surface_at
// itself calls in a scene without the table.  geo: the float4 array behind the positions; a scene with packed records (shade) keeps
// the row in words 28 .. 31 of the record.  A BVH refit or rebuild moves no vertex and writes no row.
__device__ inline void tri_geo_store(const float* p, size_t t, float4* __restrict__ geo, float* __restrict__ shade) {
    const float4 g = tri_geo_of(mk3(p[0], p[1], p[2]), mk3(p[3], p[4], p[5]), mk3(p[6], p[7], p[8]));
    if (shade) *reinterpret_cast<float4*>(shade + 32 * t + 28) = g;
    else if (geo) geo[t] = g;
}
__global__ void __launch_bounds__(256) k_tri_geo(const float* __restrict__ pos, int n, float4* __restrict__ geo, float* __restrict__ shade) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float p[9];
        for (int j = 0; j < 9; ++j) p[j] = pos[9 * (size_t)i + j];
        tri_geo_store(p, (size_t)i, geo, shade);
    }
}

__global__ void __launch_bounds__(256) k_xform_tris(DXform X, int first, int n, const float* __restrict__ bp, const float* __restrict__ bn, const float* __restrict__ bt,
                                                    const int* __restrict__ slot_of_prim, float* __restrict__ pos, float* __restrict__ nrm, float* __restrict__ tan,
                                                    float* __restrict__ shade, float4* __restrict__ geo, float4* __restrict__ leaf) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const size_t t = (size_t)first + i;
        float p[9];
        for (int v = 0; v < 3; ++v) {
            const float x = bp[9 * t + 3 * v], y = bp[9 * t + 3 * v + 1], z = bp[9 * t + 3 * v + 2];
            for (int k = 0; k < 3; ++k)
                p[3 * v + k] = X.copy ? bp[9 * t + 3 * v + k] : ((X.m[4 * k] * x + X.m[4 * k + 1] * y) + X.m[4 * k + 2] * z) + X.m[4 * k + 3];
        }
        for (int j = 0; j < 9; ++j) pos[9 * t + j] = p[j];
        if (shade)
            for (int j = 0; j < 9; ++j) shade[32 * t + j] = p[j];
        tri_geo_store(p, t, geo, shade);
        if (nrm) {
            float q[9];
            for (int v = 0; v < 3; ++v) {
                if (X.copy)
                    for (int k = 0; k < 3; ++k) q[3 * v + k] = bn[9 * t + 3 * v + k];
                else
                    xform_dir(X.nm, 3, bn + 9 * t + 3 * v, q + 3 * v);
            }
            for (int j = 0; j < 9; ++j) nrm[9 * t + j] = q[j];
            if (shade)
                for (int j = 0; j < 9; ++j) shade[32 * t + 9 + j] = q[j];
        }
        if (tan) {
            for (int v = 0; v < 3; ++v) {
                float q[3];
                if (X.copy)
                    for (int k = 0; k < 3; ++k) q[k] = bt[9 * t + 3 * v + k];
                else
                    xform_dir(X.m, 4, bt + 9 * t + 3 * v, q);
                for (int k = 0; k < 3; ++k) tan[9 * t + 3 * v + k] = q[k];
            }
        }
        float4* L = leaf + 3 * (size_t)slot_of_prim[t];
        hk_pack_leaf_tri(L, p, L[0].w, L[1].w, L[2].w);
    }
}

// min / max as the builder's Box::grow (std::min / std::max)
__device__ inline float grow_lo(float lo, float v) { return v < lo ? v : lo; }
__device__ inline float grow_hi(float hi, float v) { return hi < v ? v : hi; }

__global__ void __launch_bounds__(256) k_refit_level(int begin, int end, DNode* __restrict__ nodes, DQNode* __restrict__ qnodes, DQGrid grid,
                                                     const float4* __restrict__ leaf, const float* __restrict__ pos) {
    for (int i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
        DNode nd = nodes[i];
        float lo[2][3], hi[2][3];
        for (int c = 0; c < 2; ++c) {
            const int ref = c ? nd.c1 : nd.c0;
            for (int k = 0; k < 3; ++k) lo[c][k] = INFINITY, hi[c][k] = -INFINITY;
            if (ref >= 0) {   // inner child: the union of its two boxes (written by the previous launch)
                float cl[2][3], ch[2][3];
                hk_unpack_node_boxes(nodes[ref], cl, ch);
                for (int s = 0; s < 2; ++s)
                    for (int k = 0; k < 3; ++k) lo[c][k] = grow_lo(lo[c][k], cl[s][k]), hi[c][k] = grow_hi(hi[c][k], ch[s][k]);
            } else {          // leaf child: its triangles' world vertices, by prim
                const int first = (~ref) >> 3, count = ((~ref) & 7) + 1;
                for (int j = 0; j < count; ++j) {
                    const float* p = pos + 9 * (size_t)__float_as_int(leaf[3 * (size_t)(first + j)].w);
                    for (int v = 0; v < 9; ++v) lo[c][v % 3] = grow_lo(lo[c][v % 3], p[v]), hi[c][v % 3] = grow_hi(hi[c][v % 3], p[v]);
                }
            }
        }
        hk_pack_node_boxes(nd, lo, hi);
        nodes[i].a = nd.a, nodes[i].b = nd.b, nodes[i].c = nd.c;
        if (qnodes) {
            DQNode q = qnodes[i];
            hk_quant_node(q, lo, hi, grid.base, grid.cell);
            for (int w = 0; w < 6; ++w) qnodes[i].w[w] = q.w[w];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// NEW VERTICES (hk_scene_set_vertices).  k_set_tris gives every triangle of the range to one lane, which reads the uploaded values once,
// keeps them as the new base, puts them under the transform in force on its triangle (k_xform_tris' arithmetic) and writes every copy of
// the geometry the kernels read.  The arrays are [T][9] / [T][6] floats: the 64 rows of a wave are 2304 / 1536 contiguous bytes, which
// the wave moves as 9 / 6 instructions of 256 contiguous bytes each through a transposing LDS tile (rows 9 words apart: no bank
// conflict) — a lane walking its own 36-byte row would touch 18 lines per instruction.  The 128-byte shading record is written by its
// lane as 16-byte stores (p and n fill the first 72 bytes; the meta words are not touched), the leaf slot is a scatter by nature.
// ---------------------------------------------------------------------------------------------------
template <int K>
__device__ inline void wave_rows_load(const float* __restrict__ src, int rows, float* lds, int lane, float* __restrict__ copy_to, float* v) {
    for (int j = 0; j < K; ++j) {
        const int w = lane + 64 * j;
        if (w < rows * K) {
            const float x = src[w];
            lds[w] = x;
            if (copy_to) copy_to[w] = x;
        }
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) v[j] = lane < rows ? lds[K * lane + j] : 0.0f;
    __syncthreads();
}
template <int K>
__device__ inline void wave_rows_store(float* __restrict__ dst, int rows, float* lds, int lane, const float* v) {
    for (int j = 0; j < K; ++j) lds[K * lane + j] = v[j];
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        const int w = lane + 64 * j;
        if (w < rows * K) dst[w] = lds[w];
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) k_set_tris(DSetTris A) {
    __shared__ float lds_all[4 * 64 * 9];
    const int lane = threadIdx.x & 63;
    float* lds = lds_all + 64 * 9 * (threadIdx.x >> 6);   // one tile per wave
    // every thread of the block takes every turn of this loop (the tile helpers hold block barriers)
    for (long long blk = (long long)blockIdx.x * 256; blk < A.n; blk += (long long)gridDim.x * 256) {
        const long long w0 = blk + (threadIdx.x & ~63u);   // the wave's first triangle, counted from the range's
        const int rows = (int)(A.n - w0 < 0 ? 0 : (A.n - w0 < 64 ? A.n - w0 : 64));
        const bool live = lane < rows;
        const size_t r0 = (size_t)w0, t0 = (size_t)A.first + r0, t = t0 + lane;
        int iv = 0;
        if (live) {   // the last interval that starts at or before t
            int lo = 0, hi = A.n_iv - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (A.iv_start[mid] <= (int)t) lo = mid;
                else hi = mid - 1;
            }
            iv = lo;
        }
        const DXform X = A.iv_xf[iv];
        float bp[9], p[9];
        wave_rows_load<9>(A.in_pos + 9 * r0, rows, lds, lane, A.base_pos + 9 * t0, bp);
        for (int v = 0; v < 3; ++v) {
            const float x = bp[3 * v], y = bp[3 * v + 1], z = bp[3 * v + 2];
            for (int k = 0; k < 3; ++k) p[3 * v + k] = X.copy ? bp[3 * v + k] : ((X.m[4 * k] * x + X.m[4 * k + 1] * y) + X.m[4 * k + 2] * z) + X.m[4 * k + 3];
        }
        wave_rows_store<9>(A.pos + 9 * t0, rows, lds, lane, p);
        float q[9];
        if (A.nrm) {
            float bn[9];
            if (A.in_nrm) wave_rows_load<9>(A.in_nrm + 9 * r0, rows, lds, lane, A.base_nrm + 9 * t0, bn);
            else wave_rows_load<9>(A.base_nrm + 9 * t0, rows, lds, lane, nullptr, bn);
            for (int v = 0; v < 3; ++v) {
                if (X.copy)
                    for (int k = 0; k < 3; ++k) q[3 * v + k] = bn[3 * v + k];
                else
                    xform_dir(X.nm, 3, bn + 3 * v, q + 3 * v);
            }
            wave_rows_store<9>(A.nrm + 9 * t0, rows, lds, lane, q);
        }
        if (A.tan) {
            float bt[9], tq[9];
            if (A.in_tan) wave_rows_load<9>(A.in_tan + 9 * r0, rows, lds, lane, A.base_tan + 9 * t0, bt);
            else wave_rows_load<9>(A.base_tan + 9 * t0, rows, lds, lane, nullptr, bt);
            for (int v = 0; v < 3; ++v) {
                if (X.copy)
                    for (int k = 0; k < 3; ++k) tq[3 * v + k] = bt[3 * v + k];
                else
                    xform_dir(X.m, 4, bt + 3 * v, tq + 3 * v);
            }
            wave_rows_store<9>(A.tan + 9 * t0, rows, lds, lane, tq);
        }
        float uv[6];
        if (A.in_uv) wave_rows_load<6>(A.in_uv + 6 * r0, rows, lds, lane, A.uvs + 6 * t0, uv);   // not transformed: the copy is the array
        if (!live) continue;
        if (A.shade) {   // p[9] n[9] uv[6] meta[3] pad[1] geo[4] (the geometry row: tri_geo_store below)
            float* S = A.shade + 32 * t;
            float4* S4 = reinterpret_cast<float4*>(S);
            S4[0] = make_float4(p[0], p[1], p[2], p[3]);
            S4[1] = make_float4(p[4], p[5], p[6], p[7]);
            if (A.nrm) {
                S4[2] = make_float4(p[8], q[0], q[1], q[2]);
                S4[3] = make_float4(q[3], q[4], q[5], q[6]);
                *reinterpret_cast<float2*>(S + 16) = make_float2(q[7], q[8]);
            } else
                S[8] = p[8];
            if (A.in_uv)
                for (int j = 0; j < 3; ++j) *reinterpret_cast<float2*>(S + 18 + 2 * j) = make_float2(uv[2 * j], uv[2 * j + 1]);
        }
        tri_geo_store(p, t, A.geo, A.shade);
        float4* L = A.leaf + 3 * (size_t)A.slot_of_prim[t];
        hk_pack_leaf_tri(L, p, L[0].w, L[1].w, L[2].w);
    }
}

// ---------------------------------------------------------------------------------------------------
// LIGHT-BVH REFIT (hk_scene_refit_lights): the topology stays, the bounds on the paths from the edited leaves to the root are
// recomputed with the arithmetic of hk_light_bounds.h.  k_light_refit_leaves gives every edited light to one lane: it puts the baked
// record in its place, and for a light of the tree writes the raw leaf (the builder's bounds, from the host) and the record the walk
// reads, then climbs the parent chain storing this call's stamp until it meets it — lanes that meet on a node store the same word, so plain
// stores do, and the lane that stored first goes on to the root (the kernel boundary before the first level launch publishes every stamp).
// k_light_refit_level then takes the inner entries of ONE depth, deepest first (the kernel boundary publishes the level below, as
// for k_refit_level): a stamped entry reads its two children — one 128-byte pair — and writes their union and its walked record.
// Which lane computes a node never changes what it computes: the result is a function of the tree and the edit alone.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_light_refit_leaves(DLightRefit A) {
    static_assert(sizeof(DLight) % 16 == 0 && sizeof(HkLightRaw) == 64 && sizeof(HkLightWalk) == sizeof(DLightNode), "record sizes");
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
        const int2 sl = A.slot[i];
        const uint4* src = A.rec + (size_t)i * (sizeof(DLight) / 16);
        uint4* dst = reinterpret_cast<uint4*>(A.lights + sl.x);
        for (int k = 0; k < (int)(sizeof(DLight) / 16); ++k) dst[k] = src[k];
        if (sl.y < 0) continue;
        const int e = A.leaf_entry[sl.x];
        if (e < 0) continue;   // (the host refuses an edit that would put a light into the tree)
        const HkLightRaw leaf = A.leaf[sl.y];
        A.raw[e] = leaf;
        *reinterpret_cast<HkLightWalk*>(A.lnodes + e) = hk_lb_walk_record(leaf, leaf.child1_or_light);
        // an entry that carries this call's stamp has a lane above it that climbs, or has climbed, the rest: N lanes store about 2 N words, not N x depth
        for (int p = A.parent[e]; p >= 0 && A.stamps[p] != A.stamp; p = A.parent[p]) A.stamps[p] = A.stamp;
    }
}
__global__ void __launch_bounds__(256) k_light_refit_level(const int* __restrict__ entries, int count, DLightRefit A) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const int e = entries[i];
        if (A.stamps[e] != A.stamp) continue;
        const uint32_t c = A.lnodes[e].child1_or_light;   // the entry of child 0; child 1 is the next one
        const HkLightRaw u = hk_lb_union(A.raw[c], A.raw[c + 1]);
        A.raw[e] = u;
        *reinterpret_cast<HkLightWalk*>(A.lnodes + e) = hk_lb_walk_record(u, c);
    }
}

// TREE COST (hk_scene_bvh_cost): hk_node_cost of one node per lane, added in the block by a fixed tree of 8 steps; the host adds the
// per-block sums in index order.  No atomics: the same tree gives the same bits.
__global__ void __launch_bounds__(256) k_bvh_cost(const DNode* __restrict__ nodes, int n, double* __restrict__ partial) {
    __shared__ double red[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const DNode nd = nodes[i];
        float lo[2][3], hi[2][3];
        hk_unpack_node_boxes(nd, lo, hi);
        v = hk_node_cost(lo, hi, nd.c0, nd.c1);
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
