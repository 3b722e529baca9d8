// hk_table_kernels.h — tables rebuilt on the device after an edit: the environment map's distribution (k_envmap_*), a medium's
// majorant grid (k_majorant_*) and the NanoVDB brick cache (k_nvdb_bricks).
// Part of the hk_kernels.hip translation unit (needs hk_device.h; nothing of the render stages).
#pragma once

// ---------------------------------------------------------------------------------------------------
// ENVIRONMENT-MAP TABLES (hk_scene_update_envmap with new texels): Distribution2D(to_Y.(data)) on the device (sampler/sampling.jl:179-262,
// textures/environment_map.jl:24-45), in the header's arithmetic.  The order of the binary32 additions IS the result, so nothing is
// scanned in parallel: k_envmap_rows gives every row v of the map to one lane, which walks its nu texels left to right — texel (v, u)
// is data[v + height * u], so the lanes of a wave read adjacent texels; their table stores are nu floats apart (a sky changes rarely,
// the table is written once) — and k_envmap_marginal is ONE lane adding the nv row integrals.  Division is the correctly rounded one
// (the library is built without -fno-hip-fp32-correctly-rounded-divide-sqrt) and nothing is contracted.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_envmap_rows(const float4* __restrict__ data, int nu, int nv, float* __restrict__ cond_func, float* __restrict__ cond_cdf,
                                                    float* __restrict__ cond_func_int, float* __restrict__ marg_func) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float fnu = (float)nu;
    float* func = cond_func + (size_t)nu * v;
    float* cdf = cond_cdf + (size_t)(nu + 1) * v;
    float sum = 0.0f;
    cdf[0] = 0.0f;
    for (int u = 0; u < nu; ++u) {
        const float4 t = data[(size_t)v + (size_t)nv * u];
        const float y = (0.212671f * t.x + 0.715160f * t.y) + 0.072169f * t.z;   // to_Y
        func[u] = y;
        sum = sum + y / fnu;
        cdf[u + 1] = sum;
    }
    cond_func_int[v] = sum;
    marg_func[v] = sum;
    if (sum == 0.0f)   // isapprox(x, 0f0): exact zero only
        for (int u = 1; u <= nu; ++u) cdf[u] = (float)u / fnu;
    else
        for (int u = 1; u <= nu; ++u) cdf[u] = cdf[u] / sum;
}
__global__ void __launch_bounds__(64) k_envmap_marginal(int nv, const float* __restrict__ marg_func, float* __restrict__ marg_cdf, DEnvMap* __restrict__ record) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float fnv = (float)nv;
    float sum = 0.0f;
    marg_cdf[0] = 0.0f;
    for (int v = 0; v < nv; ++v) {
        sum = sum + marg_func[v] / fnv;
        marg_cdf[v + 1] = sum;
    }
    record->marg_func_int = sum;   // the record's own copy: the host never reads it back
    if (sum == 0.0f)
        for (int v = 1; v <= nv; ++v) marg_cdf[v] = (float)v / fnv;
    else
        for (int v = 1; v <= nv; ++v) marg_cdf[v] = marg_cdf[v] / sum;
}

// ---------------------------------------------------------------------------------------------------
// MEDIUM TABLES (hk_scene_update_medium): what hk_scene_create takes from the caller (majorant grid) or builds on the host (zero-cell
// mask, NanoVDB halo bricks), built here from the volume data already on the device.  Each is a pure function of that data — a maximum
// over an index box, a comparison, a gather — so no order of evaluation changes a bit of it: the lanes of a wave stride through a cell's
// box with the grid's contiguous axis fastest, keep a running maximum each, and a butterfly of shuffles combines the 64 of them (no
// atomics).  A cell is given to ONE WAVE (four cells per block), or to the whole block when the boxes are large (the launcher decides
// from the mean box size; the four wave maxima then meet in LDS).  Run per edit, not per pass.
// ---------------------------------------------------------------------------------------------------
__device__ inline float box_max(float m, float v) { return m < v ? v : m; }   // the host builders' max(m, v): m stays on a tie (+0 against -0) and against NaN
__device__ inline float wave_max(float m) {
    for (int off = 32; off > 0; off >>= 1) m = box_max(m, __shfl_xor(m, off));
    return m;
}
// Voxels of majorant cell i along an axis of n voxels and r cells (media.jl:1459-1493, 1-based there): start = max(1, floor(i*n/r) + 1),
// end = min(n, ceil((i+1)*n/r)).  The reference forms i*n/r as a Float64 quotient of two integers; its floor / ceil are those of the exact
// rational whenever i*n < 2^53 and r < 2^23 (the quotient is below 2^31, so its rounding error is under 2^-23 <= 1/r, the least distance
// of a non-integer a/r from an integer; an integer quotient is exact) — which holds for every grid that fits the device.  So they are
// taken in 64-bit integer arithmetic: floor = a / r, ceil = (b + r - 1) / r.  -> 0-based first voxel and the count (never below 1 for n >= 1).
__device__ inline void majorant_axis_box(int i, int n, int r, int& lo, int& len) {
    const long long a = (long long)i * n, b = (long long)(i + 1) * n;
    int start = (int)(a / r) + 1, end = (int)((b + r - 1) / r);
    start = start < 1 ? 1 : start;
    end = end > n ? n : end;
    lo = start - 1;
    len = end >= start ? end - start + 1 : 0;
}
// the cell of a wave / block and its share of the cell's box: elements first, first + stride, ...
struct CellLanes {
    int cell, first, stride;
    bool live;
};
__device__ inline CellLanes cell_lanes(int ncell, int block_per_cell) {
    CellLanes c;
    const long long id = block_per_cell ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    c.live = id < ncell;
    c.cell = c.live ? (int)id : 0;
    c.first = block_per_cell ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    c.stride = block_per_cell ? 256 : 64;
    return c;
}
// the maximum of `m` over the lanes that share a cell; true on the one lane that writes the cell (red: 4 floats of LDS per value)
__device__ inline bool cell_max(float& m, float* red, int block_per_cell) {
    m = wave_max(m);
    if (!block_per_cell) return (threadIdx.x & 63) == 0;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) m = box_max(box_max(red[0], red[1]), box_max(red[2], red[3]));
    return threadIdx.x == 0;
}

// GridMedium: max(0, max over the box) (media.jl:1459-1493).  RGBGridMedium: sigma_scale * (ma + ms), ma / ms the box maxima of the largest
// RGB component clamped at 0, an absent grid counting as 1 (media.jl:1122-1183).  Voxel (x, y, z) is at x + nx * (y + ny * z): a wave reads
// runs of the box's x extent.
template <bool RGB>
__global__ void __launch_bounds__(256) k_majorant_grid(DMedium m, int ncell, int block_per_cell, float* __restrict__ majorant) {
    __shared__ float red[2][4];
    const CellLanes c = cell_lanes(ncell, block_per_cell);
    const int rx = m.mres[0], ry = m.mres[1], rz = m.mres[2], nx = m.res[0], ny = m.res[1], nz = m.res[2];
    const int ix = c.cell % rx, iy = (c.cell / rx) % ry, iz = (c.cell / rx) / ry;
    int x0, xl, y0, yl, z0, zl;
    majorant_axis_box(ix, nx, rx, x0, xl);
    majorant_axis_box(iy, ny, ry, y0, yl);
    majorant_axis_box(iz, nz, rz, z0, zl);
    const long long total = c.live ? (long long)xl * yl * zl : 0;
    float ma = 0.0f, ms = 0.0f;
    for (long long t = c.first; t < total; t += c.stride) {
        const long long row = t / xl;
        const int x = x0 + (int)(t - row * xl), y = y0 + (int)(row % yl), z = z0 + (int)(row / yl);
        const size_t v = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * (size_t)z);
        if (RGB) {
            if (m.rgb_a) {
                const float4 a = m.rgb_a[v];
                ma = box_max(ma, box_max(box_max(a.x, a.y), a.z));
            }
            if (m.rgb_s) {
                const float4 s = m.rgb_s[v];
                ms = box_max(ms, box_max(box_max(s.x, s.y), s.z));
            }
        } else
            ma = box_max(ma, m.density[v]);
    }
    bool writer = cell_max(ma, red[0], block_per_cell);
    if (RGB) {
        if (block_per_cell) __syncthreads();
        writer = cell_max(ms, red[1], block_per_cell);
    }
    if (writer && c.live) majorant[c.cell] = RGB ? m.sigma_scale * ((m.rgb_a ? ma : 1.0f) + (m.rgb_s ? ms : 1.0f)) : ma;
}

// NanoVDBMedium (nanovdb.jl:1174-1235): the cell's two corners bmin + diag * i / r and bmin + diag * (i + 1) / r in binary32, both through
// world_to_index_f_raw (the full 3x3 inv_mat), the integer range [floor(min - 1), ceil(max + 1)] clipped to the index bounding box, and
// max(0, the voxel values in the range) — read as the tracking kernels read a voxel (nv_find_block: table entry -> leaf value; a block
// outside the table holds the background).  Leaf values are z-fastest, so z is the lanes' axis.
__device__ inline int majorant_index_bound(float f) {   // float -> int, saturating (the clip to the bounding box follows)
    return f < -2147483648.0f ? -2147483647 - 1 : (f >= 2147483648.0f ? 2147483647 : (int)f);
}
__global__ void __launch_bounds__(256) k_majorant_nanovdb(DMedium m, DIndexBox ib, int ncell, int block_per_cell, float* __restrict__ majorant) {
    __shared__ float red[4];
    const CellLanes c = cell_lanes(ncell, block_per_cell);
    const int rx = m.mres[0], ry = m.mres[1];
    const int i[3] = {c.cell % rx, (c.cell / rx) % ry, (c.cell / rx) / ry};
    float p0[3], p1[3];
    for (int k = 0; k < 3; ++k) {
        const float diag = m.bmax[k] - m.bmin[k], r = (float)m.mres[k];
        p0[k] = m.bmin[k] + diag * (float)i[k] / r;
        p1[k] = m.bmin[k] + diag * (float)(i[k] + 1) / r;
    }
    const float q0[3] = {p0[0] - m.vec[0], p0[1] - m.vec[1], p0[2] - m.vec[2]}, q1[3] = {p1[0] - m.vec[0], p1[1] - m.vec[1], p1[2] - m.vec[2]};
    int lo[3], len[3];
    bool empty = !c.live;
    for (int k = 0; k < 3; ++k) {
        const float a = (m.inv_mat[3 * k] * q0[0] + m.inv_mat[3 * k + 1] * q0[1]) + m.inv_mat[3 * k + 2] * q0[2];
        const float b = (m.inv_mat[3 * k] * q1[0] + m.inv_mat[3 * k + 1] * q1[1]) + m.inv_mat[3 * k + 2] * q1[2];
        const float fl = floorf(fminf(a, b) - 1.0f), fh = ceilf(fmaxf(a, b) + 1.0f);
        if (!(fl == fl) || !(fh == fh)) empty = true;   // an overflowed corner: no range
        int l = majorant_index_bound(fl), h = majorant_index_bound(fh);
        l = l < ib.lo[k] ? ib.lo[k] : l;
        h = h > ib.hi[k] ? ib.hi[k] : h;
        if (l > h) empty = true;
        lo[k] = l;
        len[k] = empty ? 0 : h - l + 1;   // at most the bounding box's extent, which the host has bounded (the block table covers it)
    }
    const long long total = empty ? 0 : (long long)len[0] * len[1] * len[2];
    float mx = 0.0f;
    for (long long t = c.first; t < total; t += c.stride) {
        const long long row = t / len[2];
        const int z = lo[2] + (int)(t - row * len[2]), y = lo[1] + (int)(row % len[1]), x = lo[0] + (int)(row / len[1]);
        const NvBlock blk = nv_find_block(m, x >> 3, y >> 3, z >> 3);
        mx = box_max(mx, blk.leaf_off == 0u ? blk.value : nv_leaf_value(m, blk.leaf_off, ((x & 7) << 6) | ((y & 7) << 3) | (z & 7)));
    }
    const bool writer = cell_max(mx, red, block_per_cell);
    if (writer && c.live) majorant[c.cell] = mx;
}

// DMedium::maj_zero: bit c of the mask <=> majorant[c] == 0.  One lane per cell; a wave's ballot is two words of the mask, written by
// lanes 0 and 32.  Lanes past the last cell vote 0, so the unused bits of the last word are 0; a word past the mask is not written.
__global__ void __launch_bounds__(256) k_majorant_zero_mask(const float* __restrict__ majorant, int ncell, uint32_t* __restrict__ mask) {
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long zero = __ballot(cell < ncell && majorant[cell < ncell ? cell : 0] == 0.0f);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && cell < ncell) mask[cell >> 5] = (uint32_t)(zero >> lane);
}

// DMedium::nv_bricks (nvdb_dense_bricks of hk_scene.cpp): brick b of the block table is its block's 8^3 voxels and the first plane of the
// +x / +y / +z neighbours, dst[x * 81 + y * 9 + z]; a neighbour beyond the table holds the background.  One lane per float, consecutive
// lanes consecutive in z: the stores are contiguous, the leaf loads runs of 8 or 9.
__global__ void __launch_bounds__(256) k_nvdb_bricks(DMedium m, unsigned long long n_out, float* __restrict__ bricks) {
    const unsigned long long d1 = (unsigned long long)m.nvb_dim[1], d2 = (unsigned long long)m.nvb_dim[2];
    for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < n_out; g += (unsigned long long)gridDim.x * 256) {
        const unsigned long long b = g / 729u;
        const int e = (int)(g - b * 729u), x = e / 81, y = (e / 9) % 9, z = e % 9;
        const unsigned long long bz = b % d2 + (unsigned)(z >> 3), by = (b / d2) % d1 + (unsigned)(y >> 3), bx = (b / d2) / d1 + (unsigned)(x >> 3);
        float v = m.nv_background;
        if (bx < (unsigned long long)m.nvb_dim[0] && by < d1 && bz < d2) {
            const uint2 ent = m.nv_blocks[bz + d2 * (by + d1 * bx)];
            v = ent.x == 0u ? __uint_as_float(ent.y) : nv_leaf_value(m, ent.x, ((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
        }
        bricks[g] = v;
    }
}
