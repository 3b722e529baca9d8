// hk_film_kernels.h — K12: the fold of a pixel's samples into the film accumulators (film_tile) and k_film.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h; hk_small_pass.h above it declares film_tile ahead).
#pragma once

// ---------------------------------------------------------------------------------------------------
// K12: spectral -> RGB, firefly clamp, filter-weighted accumulation (volpath.jl:326-375).  The S samples of
// a pixel are folded in sample order, so the fp32 sums equal the reference's sample-by-sample sums.
// ---------------------------------------------------------------------------------------------------
// The wavelength pdfs are a function of the wavelengths alone (sample_wavelengths_visible: pdf = visible_wavelengths_pdf(lambda), the
// same expression on the same bits): the film kernel recomputes them instead of reading 16 B per sample that k_camera had to write.
HKD S4 pdf_of(S4 l) { return s4(visible_wavelengths_pdf(l.x), visible_wavelengths_pdf(l.y), visible_wavelengths_pdf(l.z), visible_wavelengths_pdf(l.w)); }
// One 8x8 pixel tile = a contiguous run of 64 * S path slots, by one wave.  The run is read 64 slots at a time (coalesced; the colour
// conversion — twelve IEEE divisions and table reads per sample, the bulk of this kernel — runs on all lanes), the weighted
// colours go through LDS (`mine`: 256 floats of the wave), and the entries of a pixel are added one after the other IN SAMPLE ORDER, as
// the reference adds them (so the film does not depend on the pass size): lanes 4p .. 4p+3 own the four channels of the p-th pixel met
// in the step.
// G > 1 (k_film under HK_FILM_FOLD, passes of S = 64 k samples): the fold of ONE pixel keeps four lanes busy for 64 dependent additions
// per step while sixty wait.  The wave converts the steps of G consecutive pixels of the tile instead (all lanes, as before), each into a
// row of its own, and 4 G lanes — lane 4 p + c: pixel p of the group, channel c — add their rows together: per pixel and channel the same
// additions in the same order, the accumulator carried over the pixel's S / 64 steps.  A row is 64 * 4 + 4 words: without the four
// words of padding every row starts on bank 0 and the lanes of one t collide.
constexpr int HK_FILM_ROW = 64 * 4 + 4;
#ifndef HK_FILM_FOLD_G
#define HK_FILM_FOLD_G 4   // pixels per group: 4, 8 and 16 were measured (LAB_NOTEBOOK "tri_geo and the film fold"); 4 keeps eight waves per SIMD
#endif
template <typename ACC, int G>
__device__ __forceinline__ void film_tile(const DPathState& st, const DFrame& fr, const DTables& T, ACC* __restrict__ accum, float* __restrict__ mine, int tile) {
    const int lane = lane_id();
    const int S = fr.samples_in_pass;
    const size_t N = (size_t)fr.width * fr.height;
        const size_t base = (size_t)tile * 64 * S;
        // pass sizes that tile the 64-slot steps (S a multiple of 64, or 4 / 8 / 16 / 32): whole pixels per step, one quad per pixel;
        // any other S: one lane per pixel walks the steps.  Both add in sample order.
        const int ch = lane & 3, quad = lane >> 2;
        if constexpr (G > 1) {
            if (S >= 64 && (S & 63) == 0) {
                const int steps_per_pix = S / 64;
                for (int p0 = 0; p0 < 64; p0 += G) {
                    ACC acc = 0;
                    bool inside = false;
                    size_t fp = 0;
                    if (quad < G) {
                        int px, py;
                        slot_to_pixel(fr, tile * 64 + p0 + quad, px, py, inside);
                        fp = inside ? (size_t)py * fr.width + px : 0;
                        if (inside) acc = ch < 3 ? accum[3 * fp + ch] : accum[3 * N + fp];
                    }
                    for (int stp = 0; stp < steps_per_pix; ++stp) {
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                        for (int g = 0; g < G; ++g) {
                            const size_t slot = base + (size_t)(p0 + g) * S + (size_t)stp * 64 + lane;
                            const S4 lam_ = ld4(&st.lambda_s[slot]);
                            const v3 rgb = spectral_to_rgb_clamped(T, ld4(&st.L[slot]), lam_, pdf_of(lam_), fr.max_component_value);
                            if (st.view_cache == 1) stream_st(&st.L[slot], s4(0.0f));
                            const float fw = st.filter_w[slot];
                            float* row = mine + g * HK_FILM_ROW + 4 * lane;
                            row[0] = fw * rgb.x;
                            row[1] = fw * rgb.y;
                            row[2] = fw * rgb.z;
                            row[3] = fw;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                        if (quad < G && inside) {
                            const float* row = mine + quad * HK_FILM_ROW + ch;
                            for (int t = 0; t < 64; ++t) acc += (ACC)row[4 * t];
                        }
                    }
                    if (quad < G && inside) {
                        if (ch < 3)
                            accum[3 * fp + ch] = acc;
                        else
                            accum[3 * N + fp] = acc;
                    }
                }
                return;
            }
        }
        if (S >= 64 ? (S & 63) == 0 : (S >= 4 && (64 % S) == 0)) {
            const int pix_per_step = S >= 64 ? 1 : 64 / S;        // pixels wholly inside one step (S < 64), or one pixel over S / 64 steps
            const int steps_per_pix = S >= 64 ? S / 64 : 1;
            for (int p0 = 0; p0 < 64; p0 += pix_per_step) {       // first pixel of the group handled together
                ACC acc = 0;
                bool inside = false;
                size_t fp = 0;
                if (quad < pix_per_step) {
                    int px, py;
                    slot_to_pixel(fr, tile * 64 + p0 + quad, px, py, inside);
                    fp = inside ? (size_t)py * fr.width + px : 0;
                    if (inside) acc = ch < 3 ? accum[3 * fp + ch] : accum[3 * N + fp];
                }
                for (int stp = 0; stp < steps_per_pix; ++stp) {
                    const size_t slot = base + (size_t)p0 * S + (size_t)stp * 64 + lane;
                    // slots of film padding were never written by k_camera: whatever they hold is converted but never added
                    const S4 lam_ = ld4(&st.lambda_s[slot]);
                    const v3 rgb = spectral_to_rgb_clamped(T, ld4(&st.L[slot]), lam_, pdf_of(lam_), fr.max_component_value);
                    if (st.view_cache == 1) stream_st(&st.L[slot], s4(0.0f));   // the next pass may keep this one's camera records: its L starts at zero without k_camera
                    const float fw = st.filter_w[slot];
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    mine[4 * lane + 0] = fw * rgb.x;
                    mine[4 * lane + 1] = fw * rgb.y;
                    mine[4 * lane + 2] = fw * rgb.z;
                    mine[4 * lane + 3] = fw;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    if (quad < pix_per_step && inside) {
                        const int first = S >= 64 ? 0 : quad * S, cnt = S >= 64 ? 64 : S;
                        for (int t = 0; t < cnt; ++t) acc += (ACC)mine[4 * (first + t) + ch];
                    }
                }
                if (quad < pix_per_step && inside) {
                    if (ch < 3)
                        accum[3 * fp + ch] = acc;
                    else
                        accum[3 * N + fp] = acc;
                }
            }
        } else {
            // general S: lane = pixel, every 64-slot step's entries of a pixel added by its lane (four channels in turn)
            int px, py;
            bool inside;
            slot_to_pixel(fr, tile * 64 + lane, px, py, inside);
            const size_t p = inside ? (size_t)py * fr.width + px : 0;
            ACC r = 0, g = 0, b = 0, w = 0;
            if (inside) r = accum[3 * p], g = accum[3 * p + 1], b = accum[3 * p + 2], w = accum[3 * N + p];
            const int lo = lane * S, hi = lo + S;
            for (int j = 0; j < 64 * S; j += 64) {
                const size_t slot = base + j + lane;
                const S4 lam_ = ld4(&st.lambda_s[slot]);
                const v3 rgb = spectral_to_rgb_clamped(T, ld4(&st.L[slot]), lam_, pdf_of(lam_), fr.max_component_value);
                if (st.view_cache == 1) stream_st(&st.L[slot], s4(0.0f));
                const float fw = st.filter_w[slot];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                mine[4 * lane + 0] = fw * rgb.x;
                mine[4 * lane + 1] = fw * rgb.y;
                mine[4 * lane + 2] = fw * rgb.z;
                mine[4 * lane + 3] = fw;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                const int a = lo > j ? lo : j, e = hi < j + 64 ? hi : j + 64;
                if (inside)
                    for (int t = a; t < e; ++t) {
                        r += (ACC)mine[4 * (t - j) + 0];
                        g += (ACC)mine[4 * (t - j) + 1];
                        b += (ACC)mine[4 * (t - j) + 2];
                        w += (ACC)mine[4 * (t - j) + 3];
                    }
            }
            if (inside) {
                accum[3 * p] = r;
                accum[3 * p + 1] = g;
                accum[3 * p + 2] = b;
                accum[3 * N + p] = w;
            }
        }
}
template <typename ACC, int G>
__global__ void __launch_bounds__(256) k_film(DPathState st, DFrame fr, DTables T, ACC* __restrict__ accum) {
    __shared__ float buf[4][G > 1 ? G * HK_FILM_ROW : 64 * 4];
    float* mine = buf[threadIdx.x >> 6];
    const int n_tiles = fr.n_pixels_padded >> 6;
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int tile = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); tile < n_tiles; tile += n_waves) film_tile<ACC, G>(st, fr, T, accum, mine, tile);
}
