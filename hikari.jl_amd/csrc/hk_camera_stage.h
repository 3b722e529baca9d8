// hk_camera_stage.h — K1 and its tables: k_sobol_table, k_segment_lists, k_sobol_lo_table, camera_body and k_camera.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h).
#pragma once

// Pixel-digit table of the ZSobol index (DSobol::hi_table): entry (row, pixel slot) = the permuted base-4 digits above the
// sample bits, for the dimension of that row.  Built once per film size / sampler seed.
__global__ void __launch_bounds__(256) k_sobol_table(DSobol sob, DFrame fr, uint2* table, int rows) {
    const long total = (long)rows * fr.n_pixels_padded;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int row = (int)(i / fr.n_pixels_padded), pix = (int)(i - (long)row * fr.n_pixels_padded);
        int px, py;
        bool inside;
        slot_to_pixel(fr, pix, px, py, inside);
        const int dim = sobol_row_dim(row);
        uint64_t m = (left_shift2((uint64_t)(uint32_t)(py + 1)) << 1) | left_shift2((uint64_t)(uint32_t)(px + 1));
        uint64_t morton = m << sob.log2_spp;
        const int pow2 = sob.log2_spp & 1;
        const uint64_t dmix = 0x55555555ull * (uint64_t)(int64_t)dim;
        uint64_t hi = zsobol_digits(morton, dmix, pow2, sob.n_base4_digits - 1, zsobol_first_pixel_digit(sob.log2_spp));
        table[i] = make_uint2((uint32_t)(hi >> sob.log2_spp), zsobol_top_perms(morton, dmix, sob.log2_spp));
    }
}

// Work lists (see SegTickets): the non-empty segments of a queue and their number.
struct SegQueues {
    int n;
    int depth[HK_MAX_KINDS + 6], q[HK_MAX_KINDS + 6];
};
// grid (queues, HK_LIST_SPLIT): block y writes the non-empty segments of its contiguous share, ascending, behind those of the shares
// before it — whose number it counts itself (a few dozen loads per thread), so the list is globally ascending (dense queues give
// the identity, which keeps the static stride's segment -> wave -> XCD assignment) and no block waits for another.
#define HK_LIST_SPLIT 8
__global__ void __launch_bounds__(1024) k_segment_lists(DPathState st, SegQueues qs) {
    __shared__ int wave_total[16];
    const int d = qs.depth[blockIdx.x], q = qs.q[blockIdx.x];
    const int* __restrict__ cnt = st.counters + (size_t)(d * Q_COUNT + q) * st.n_waves;
    int* __restrict__ out = st.seg_list + (size_t)(d * Q_COUNT + q) * st.n_waves;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int share = (st.n_waves + HK_LIST_SPLIT - 1) / HK_LIST_SPLIT;
    // both clamped: for small segment counts ceil(n / 8) * 7 can exceed n (n = 12: share 2, block 7 would start at 14 and count the NEXT
    // queue's words into its prefix)
    const int begin = (int)blockIdx.y * share < st.n_waves ? (int)blockIdx.y * share : st.n_waves, end = begin + share < st.n_waves ? begin + share : st.n_waves;
    // the non-empty segments before this block's share
    int mine = 0;
    for (int i = (int)threadIdx.x; i < begin; i += 1024) mine += cnt[i] != 0 ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane == 0) wave_total[wave] = mine;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < 16; ++w) base += wave_total[w];
    for (int start = begin; start < end; start += 1024) {
        const int i = start + (int)threadIdx.x;
        const bool nz = i < end && cnt[i] != 0;
        const unsigned long long m = __ballot(nz);
        __syncthreads();
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (nz) out[base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
    }
    if (blockIdx.y == HK_LIST_SPLIT - 1 && threadIdx.x == 0) st.seg_list_n[d * Q_COUNT + q] = base;
}

// Sample-bit table (DSobol::lo_table): the low log2_spp bits of the permuted index for sample indices base + j * stride, j < count.
// One thread per 16 entries.  With stride 1 and base a multiple of 16 the sixteen share every digit above the last two, the
// permutation of the second-to-last digit is chosen by the digits above it (one hash for all sixteen) and that of the last digit by
// the digits above IT (one hash per four): 9 hashes per 16 entries instead of 4 per entry (Cornell 800^2, 49 rows, 256 spp: 16 GB).
__global__ void __launch_bounds__(256) k_sobol_lo_table(DSobol sob, DFrame fr, uint16_t* table, int rows, int base, int stride, int count) {
    const long groups = count >> 4;
    const long total = (long)rows * fr.n_pixels_padded * groups;
    const uint32_t mask = (1u << sob.log2_spp) - 1u;
    const int pow2 = sob.log2_spp & 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long rp = i / groups;
        const int q = (int)(i - rp * groups);
        const int row = (int)(rp / fr.n_pixels_padded), pix = (int)(rp - (long)row * fr.n_pixels_padded);
        int px, py;
        bool inside;
        slot_to_pixel(fr, pix, px, py, inside);
        const int dim = sobol_row_dim(row);
        const uint64_t dmix = 0x55555555ull * (uint64_t)(int64_t)dim;
        const uint64_t m = ((left_shift2((uint64_t)(uint32_t)(py + 1)) << 1) | left_shift2((uint64_t)(uint32_t)(px + 1))) << sob.log2_spp;
        const uint2 e = sob.hi_table[(size_t)row * sob.hi_stride + pix];
        uint32_t v[16];
        const int s0 = base + 16 * q * stride;
        if (stride == 1 && pow2 == 0 && (s0 & 15) == 0 && sob.log2_spp >= 4) {
            const uint64_t morton = m | (uint64_t)(uint32_t)s0;
            const uint32_t upper = (uint32_t)zsobol_sample_index_cached(morton, dim, sob.log2_spp, e.x, e.y) & mask & ~15u;
            const int p1 = zsobol_perm_index(morton >> 4, dmix);
            for (int d1 = 0; d1 < 4; ++d1) {
                const uint32_t hi = upper | ((uint32_t)zsobol_permute_digit(p1, d1) << 2);
                const int p0 = zsobol_perm_index((morton | ((uint64_t)d1 << 2)) >> 2, dmix);
                for (int d0 = 0; d0 < 4; ++d0) v[4 * d1 + d0] = hi | (uint32_t)zsobol_permute_digit(p0, d0);
            }
        } else {
            for (int t = 0; t < 16; ++t) v[t] = (uint32_t)zsobol_sample_index_cached(m | (uint64_t)(uint32_t)(s0 + t * stride), dim, sob.log2_spp, e.x, e.y) & mask;
        }
        uint4* out = reinterpret_cast<uint4*>(table) + 2 * i;
        out[0] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        out[1] = make_uint4(v[8] | (v[9] << 16), v[10] | (v[11] << 16), v[12] | (v[13] << 16), v[14] | (v[15] << 16));
    }
}

// ---------------------------------------------------------------------------------------------------
// K1: camera rays (volpath.jl:125-205).  One thread per path slot of the pass.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void camera_body(const DPathState& st, const DFrame& fr, const DTables& T, const DFilter& flt, const DCamera& cam, const DSobol& sob, const SegTickets& src) {
    const int total = fr.n_pixels_padded * fr.samples_in_pass;
    const int n_chunks = total >> 6;
    const DPathGen g0 = st.gen_cam;
    HK_FOR_EACH_SEGMENT_FROM(gw, st, src) {
    WavePos out{0};
    const size_t seg = (size_t)gw * st.wave_cap;
    // wave w generates chunks w, w+W, w+2W, ... (64 consecutive slots = samples of one pixel, or of 64 / S pixels; interleaved across waves for load balance)
    for (int chunk = gw; chunk < n_chunks; chunk += st.n_waves) {
        int slot = chunk * 64 + lane_id();
        int pix, k;
        split_slot(fr, (uint32_t)slot, pix, k);
        int px, py;
        bool active;
        slot_to_pixel(fr, pix, px, py, active);
        const size_t p = seg + (size_t)wp_push(out, active);   // generation 0 holds the pass's paths in camera order, film padding squeezed out
        if (active) {
            int sample_idx = fr.first_sample + k * fr.sample_stride;
            int x = px + 1, y = py + 1;  // 1-based pixel coordinates (Q1)
            SobolCtx sc = sobol_ctx(sob, T.sobol, x, y, sample_idx, pix, k);
            float wavelength_u = sobol_1d(sc, 1);
            v2 jit = sobol_2d(sc, 3);
            // dims 4 (time) and 6 (lens) only matter with a finite aperture: ray.time is carried by the reference
            // but never read on this path (no motion blur in VolPath), and the lens sample is unused when
            // lens_radius == 0 (perspective.jl:103-112).  Both draws are pure functions, so skipping them is exact.
            float time_u = 0.0f;
            v2 lens = mk2(0.0f, 0.0f);
            if (cam.lens_radius > 0) {
                time_u = sobol_1d(sc, 4);
                lens = sobol_2d(sc, 6);
            }
            float fx, fy, fw;
            filter_sample(flt, jit, fx, fy, fw);
            S4 lambda, pdf;
            sample_wavelengths_visible(wavelength_u, lambda, pdf);
            v2 pfilm = mk2((float)x + 0.5f + fx, (float)fr.height - (float)y + 1.0f + 0.5f + fy);  // Q2
            v3 ro, rd;
            float time;
            generate_ray(cam, pfilm, lens, time_u, ro, rd, time);
            if (!st.const_origin || p == seg) stream_st(&g0.ray_o[p], make_float4(ro.x, ro.y, ro.z, INF_F));   // (a pinhole camera's rays all start at one point: ld_ray_o)
            // beta = r_u = r_l = 1 at depth 0 (volpath.jl:190-197): in scenes without media nothing changes them before the first
            // shading event, so they are not stored and the depth-0 readers substitute the constant (ld_throughput); the compact
            // records of a grey medium keep r_l = 1 beside the direction
            stream_st(&g0.ray_d[p], make_float4(rd.x, rd.y, rd.z, (st.compact && !fr.implicit_ones) ? 1.0f : 0.0f));
            st_lambda(g0, p, lambda);
            if (!fr.implicit_ones) {
                st4(&g0.beta[p], s4(1.0f));
                st_ru_rl(g0, p, s4(1.0f), s4(1.0f), st.compact != 0);
            }
            st_meta(st, g0, p, (uint32_t)(*st.initial_medium + 1) << 16, (uint32_t)slot);
            stream_st(&st.lambda_s[slot], lambda);
            stream_st(&st.L[slot], s4(0.0f));
            stream_st(&st.filter_w[slot], fw);
        }
    }
    if (lane_id() == 0) *count_ptr(st, 0, Q_RAY, gw) = out.count;
    }
}
__global__ void __launch_bounds__(256) k_camera(DPathState st, DFrame fr, DTables T, DFilter flt, DCamera cam, DSobol sob, int initial_medium) {
    camera_body(st, fr, T, flt, cam, sob, seg_open(st, ticket_ptr(st, st.ticket_rows - 1, TK_CAMERA), st.dynamic_segments != 0, -1, 0));
}
