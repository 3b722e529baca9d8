// hk_display.h — the display chain: K13 (film -> frame), the first-hit guides, the 3x3 luminance variance, the a-trous passes and the
// postprocess.  Part of the hk_kernels.hip translation unit (traverse, generate_ray, geometric_normal and lane_id are defined above it).
// Every stage is ONE device function of one pixel that knows no memory layout, and one kernel template over a layout (hk_types.h):
//   PlanarPixels   three floats per pixel and planar guides — the host-array entry points hk_film_read_rgb, hk_film_fill_aux, hk_denoise,
//                  hk_postprocess, hk_film_postprocess (pinned to the oracle by the parity tests);
//   PackedPixels   one float4 (r, g, b, lum) and one float4 (nx, ny, nz, depth) per pixel, buffers of the film — hk_film_update_aux and
//                  hk_film_present: a tap is two 16-byte loads and no luminance.
// Both instantiations run the same expressions in the same order (strict binary32, no contraction), so hk_film_present returns, bit for
// bit, what hk_film_read_rgb -> hk_denoise -> hk_postprocess return (tests/test_film_present.py).
// All images are Julia [h,w] column-major: linear index i = col * h + row, exactly the reference's idx -> (row, col) mapping.
#pragma once

HKD long pixel_index(int row, int col, int h) { return (long)col * h + row; }
HKD void pixel_row_col(long i, int h, int& row, int& col) { row = (int)(i % h), col = (int)(i / h); }

// K13 (volpath.jl:384-417): rgb / weight of film pixel p, 0 where no sample landed
template <typename ACC>
HKD void finalize_pixel(const ACC* __restrict__ accum, size_t N, size_t p, float& r, float& g, float& b) {
    ACC w = accum[3 * N + p];
    r = 0.0f, g = 0.0f, b = 0.0f;
    if (w > (ACC)0) {
        ACC inv = (ACC)1 / w;
        r = (float)(accum[3 * p] * inv);
        g = (float)(accum[3 * p + 1] * inv);
        b = (float)(accum[3 * p + 2] * inv);
    }
}
// out = Julia Matrix{RGB{Float32}}[height,width]: the film's row-major pixel (px, py) lands at py + height * px
template <typename ACC, class Layout>
__global__ void __launch_bounds__(256) k_finalize(const ACC* __restrict__ accum, Layout out, int width, int height) {
    size_t N = (size_t)width * height;
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
        int px = (int)(p % width), py = (int)(p / width);
        float r, g, b;
        finalize_pixel(accum, N, p, r, g, b);
        out.store_color((size_t)py + (size_t)height * px, r, g, b);
    }
}

// aux_buffer_kernel! (src/film.jl:435-483): first hit of the ray through the centre of pixel (row, col), 1-based -> (normal, distance), albedo
HKD float4 first_hit_guides(const DScene& sc, const DCamera& cam, int row, int col, float miss_depth, int* stack, int lane, unsigned& a, unsigned& b, float& alb) {
    v2 pixel = mk2(((float)col - 1.0f) + 0.5f, ((float)row - 1.0f) + 0.5f);
    v3 ro, rd;
    float time;
    generate_ray(cam, pixel, mk2(0.5f, 0.5f), 0.0f, ro, rd, time);
    bool opaque;
    HitRec hr = traverse<0, false>(sc, ro, rd, INF_F, stack, lane, a, b, opaque);
    float d = miss_depth;
    v3 nn = mk3(0, 0, 0);
    alb = 0.0f;
    if (hr.prim >= 0) {
        nn = geometric_normal(sc, hr.prim);
        v3 hp = ro + rd * hr.t;
        v3 dd = hp - ro;
        d = sqrtf(dd.x * dd.x + dd.y * dd.y + dd.z * dd.z);
        alb = 0.8f;
    }
    return make_float4(nn.x, nn.y, nn.z, d);
}
template <class Layout>
__global__ void __launch_bounds__(HK_TRACE_BLOCK) k_aux(DScene sc, DCamera cam, int h, int w, float miss_depth, float* __restrict__ albedo, Layout out) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * HK_LDS_STACK * 64];
    int* stack = lds_stack + (threadIdx.x >> 6) * (HK_LDS_STACK * 64);
    const int lane = lane_id();
    unsigned a = 0, b = 0;
    const long n = (long)h * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int row, col;
        pixel_row_col(i, h, row, col);
        float alb;
        float4 g = first_hit_guides(sc, cam, row + 1, col + 1, miss_depth, stack, lane, a, b, alb);
        albedo[3 * i] = albedo[3 * i + 1] = albedo[3 * i + 2] = alb;
        out.store_guide(i, g);
    }
}

// ---------------------------------------------------------------------------------------------------
// denoise! (src/denoise.jl): 3x3 luminance variance (:236-286) and one a-trous pass (:136-229)
// ---------------------------------------------------------------------------------------------------
template <class Layout>
HKD float variance_pixel(const Layout& src, int row, int col, int h, int w) {
    float sum = 0.0f, sum_sq = 0.0f;
    int count = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            int qr = row + dy, qc = col + dx;
            if (qr >= 0 && qr < h && qc >= 0 && qc < w) {
                float lum = src.color(pixel_index(qr, qc, h)).w;
                sum += lum;
                sum_sq += lum * lum;
                ++count;
            }
        }
    float mean = sum / (float)count, mean_sq = sum_sq / (float)count;
    return maxf(0.0f, mean_sq - mean * mean);
}
template <class Layout>
__global__ void __launch_bounds__(256) k_variance(Layout src, float* __restrict__ variance, int h, int w) {
    const long n = (long)h * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int row, col;
        pixel_row_col(i, h, row, col);
        variance[i] = variance_pixel(src, row, col, h, w);
    }
}
// One pixel of an a-trous pass: cp / gp the centre's records (colour + luminance, normal + depth), var_p its variance,
// fetch(dyi, dxi, cq, gq) the records of tap (dyi, dxi), clamped to the edge; UNROLL: the layout's tap_unroll
template <int UNROLL, class Fetch>
HKD void atrous_pixel(const hk_denoise_params& P, int step, float4 cp, float4 gp, float var_p, Fetch fetch, float& r, float& g, float& b) {
    const float K1D[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float r_p = cp.x, g_p = cp.y, b_p = cp.z;
    float lum_p = cp.w;
    float nx = gp.x, ny = gp.y, nz = gp.z;
    float d_p = gp.w;
    // weight_color's sigma (:76-88) depends on the centre pixel only
    float sigma_c = var_p > 0.0f ? P.sigma_color * sqrtf(var_p) + 1.0e-4f : P.sigma_color;
    float sigma_d = P.sigma_depth * (float)step + 1.0e-4f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll UNROLL
    for (int dyi = 0; dyi < 5; ++dyi)
#pragma unroll UNROLL
        for (int dxi = 0; dxi < 5; ++dxi) {
            float4 cq, gq;
            fetch(dyi, dxi, cq, gq);
            float r_q = cq.x, g_q = cq.y, b_q = cq.z;
            float lum_q = cq.w;
            float w_spatial = K1D[dxi] * K1D[dyi];
            float w_color = expf(-fabsf(lum_p - lum_q) / sigma_c);
            float dotv = nx * gq.x + ny * gq.y + nz * gq.z;
            float w_norm = powf(maxf(0.0f, dotv), P.sigma_normal);
            float w_depth = expf(-fabsf(d_p - gq.w) / sigma_d);
            float weight = w_spatial * w_color * w_norm * w_depth;
            sr += r_q * weight;
            sg += g_q * weight;
            sb += b_q * weight;
            sw += weight;
        }
    r = r_p, g = g_p, b = b_p;
    if (sw > 1.0e-6f) {   // false for NaN (centre depth +Inf against +Inf neighbours): the pixel is kept
        float inv = 1.0f / sw;
        r = sr * inv, g = sg * inv, b = sb * inv;
    }
}

// ---------------------------------------------------------------------------------------------------
// postprocess_kernel! (src/postprocess.jl:185-250): exposure, white balance, imaging ratio, tone curve, gamma, escaped-ray mask.
// ---------------------------------------------------------------------------------------------------
HKD float pp_unch2(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}
HKD float pp_filmic(float x) {
    x = maxf(0.0f, x - 0.004f);
    return (x * (6.2f * x + 0.5f)) / (x * (6.2f * x + 1.7f) + 0.06f);
}
// r, g, b: the linear colour of pixel i; the depths of the escaped mask come through the layout
template <class Layout>
HKD void postprocess_pixel(const hk_postprocess_params& P, float& r, float& g, float& b, long i, const Layout& px, int h, int w) {
    r = r * P.exposure, g = g * P.exposure, b = b * P.exposure;
    if (P.apply_wb) {
        float ro = P.wb[0] * r + P.wb[1] * g + P.wb[2] * b, go = P.wb[3] * r + P.wb[4] * g + P.wb[5] * b, bo = P.wb[6] * r + P.wb[7] * g + P.wb[8] * b;
        r = maxf(0.0f, ro), g = maxf(0.0f, go), b = maxf(0.0f, bo);
    }
    r = r * P.imaging_ratio, g = g * P.imaging_ratio, b = b * P.imaging_ratio;
    switch (P.tonemap) {
        case HK_TONEMAP_REINHARD: {
            float lum = luminance709(r, g, b);
            float sc = lum > 0.0f ? 1.0f / (1.0f + lum) : 1.0f;
            r = clampf(r * sc, 0.0f, 1.0f), g = clampf(g * sc, 0.0f, 1.0f), b = clampf(b * sc, 0.0f, 1.0f);
        } break;
        case HK_TONEMAP_REINHARD_EXT: {
            float lum = luminance709(r, g, b);
            float lw2 = P.white_point * P.white_point;
            float sc = lum > 0.0f ? (1.0f + lum / lw2) / (1.0f + lum) : 1.0f;
            r = clampf(r * sc, 0.0f, 1.0f), g = clampf(g * sc, 0.0f, 1.0f), b = clampf(b * sc, 0.0f, 1.0f);
        } break;
        case HK_TONEMAP_ACES: {
            const float a = 2.51f, bc = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
            r = clampf((r * (a * r + bc)) / (r * (c * r + d) + e), 0.0f, 1.0f);
            g = clampf((g * (a * g + bc)) / (g * (c * g + d) + e), 0.0f, 1.0f);
            b = clampf((b * (a * b + bc)) / (b * (c * b + d) + e), 0.0f, 1.0f);
        } break;
        case HK_TONEMAP_UNCHARTED2: {
            float ws = 1.0f / pp_unch2(11.2f);
            r = clampf(pp_unch2(r * 2.0f) * ws, 0.0f, 1.0f), g = clampf(pp_unch2(g * 2.0f) * ws, 0.0f, 1.0f), b = clampf(pp_unch2(b * 2.0f) * ws, 0.0f, 1.0f);
        } break;
        case HK_TONEMAP_FILMIC: r = pp_filmic(r), g = pp_filmic(g), b = pp_filmic(b); break;
        default: r = clampf(r, 0.0f, 1.0f), g = clampf(g, 0.0f, 1.0f), b = clampf(b, 0.0f, 1.0f); break;
    }
    if (P.apply_gamma) r = powf(r, P.inv_gamma), g = powf(g, P.inv_gamma), b = powf(b, P.inv_gamma);
    if (P.mask_escaped && px.has_depth()) {
        int row, col;
        pixel_row_col(i, h, row, col);
        row += 1, col += 1;
        int d_row = h - row + 1;  // Y flip
        int escaped = 0, total = 0;
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                int nr = d_row + dr, nc = col + dc;
                if (nr >= 1 && nr <= h && nc >= 1 && nc <= w) {
                    escaped += isinf(px.depth_at(pixel_index(nr - 1, nc - 1, h))) ? 1 : 0;
                    total += 1;
                }
            }
        float alpha = (float)escaped / (float)total;
        r = r * (1.0f - alpha) + P.bg[0] * alpha, g = g * (1.0f - alpha) + P.bg[1] * alpha, b = b * (1.0f - alpha) + P.bg[2] * alpha;
    }
}
// the frame a caller sees is always three floats per pixel
template <class Layout>
__global__ void __launch_bounds__(256) k_postprocess(hk_postprocess_params P, Layout src, float* __restrict__ out, int h, int w) {
    const long n = (long)h * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float4 c = src.color(i);
        float r = c.x, g = c.y, b = c.z;
        postprocess_pixel(P, r, g, b, i, src, h, w);
        PlanarPixels{out, nullptr, nullptr}.store_color(i, r, g, b);
    }
}
// One a-trous pass, one thread per pixel along the contiguous dimension, the taps from global memory at every step (an LDS tile of
// 32 x 8 pixels + halo for steps 1 and 2 of the packed layout was built and measured: no gain outside the spread, LAB_NOTEBOOK — not kept).
// FINAL (hk_film_present): the last pass applies the postprocess (apply_pp) to its own result and writes the 3-float frame `out`.
template <class Layout, bool FINAL>
__global__ void __launch_bounds__(256) k_atrous(hk_denoise_params P, hk_postprocess_params PP, int apply_pp, int step, Layout src, const float* __restrict__ variance, Layout dst,
                                                float* __restrict__ out, int h, int w) {
    const long n = (long)h * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int row, col;
        pixel_row_col(i, h, row, col);
        auto fetch = [&](int dyi, int dxi, float4& cq, float4& gq) {
            int qr = row + (dyi - 2) * step, qc = col + (dxi - 2) * step;
            qr = qr < 0 ? 0 : (qr > h - 1 ? h - 1 : qr);
            qc = qc < 0 ? 0 : (qc > w - 1 ? w - 1 : qc);
            long q = pixel_index(qr, qc, h);
            cq = src.color(q);
            gq = src.guide(q);
        };
        float r, g, b;
        atrous_pixel<Layout::tap_unroll>(P, step, src.color(i), src.guide(i), P.use_variance ? variance[i] : 0.0f, fetch, r, g, b);
        if (FINAL) {
            if (apply_pp) postprocess_pixel(PP, r, g, b, i, src, h, w);
            PlanarPixels{out, nullptr, nullptr}.store_color(i, r, g, b);
        } else
            dst.store_color(i, r, g, b);
    }
}
