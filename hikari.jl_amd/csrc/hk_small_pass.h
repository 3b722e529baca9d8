// hk_small_pass.h — k_small_pass: a small pass as ONE launch, every stage of a segment run by the wave that owns it.
// Part of the hk_kernels.hip translation unit (needs the stage bodies of hk_camera_stage.h, hk_traverse.h, hk_shade.h and hk_shadow.h;
// film_tile, declared here, is defined in hk_film_kernels.h).
#pragma once

// ---------------------------------------------------------------------------------------------------
// A SMALL pass as ONE launch (the reference's interactive call: one sample of every pixel, volpath.jl:445-450).  A path never leaves the
// segment that generated its camera ray, so K1 and every bounce's K2 / K8 - K9 / K10 of a segment depend on nothing outside it: the wave
// that owns the segment runs all of them, stage after stage, without waiting for any other wave.  As launches, the 26 kernels of such a
// call each ran at the latency of one wave's chunks PLUS the wait for the slowest wave of the stage; here a wave's stages follow each
// other directly.  The stage bodies are the standalone kernels' (camera_body, trace_lean_body, shade_body, shadow_body: same arithmetic,
// same order, same queues — films bit-identical), the block is k_trace_lean's (16 waves: the stacks and the top of the tree in LDS).
// Hand-over between stages goes through the segment's global arrays: written and read by the SAME wave, so completing the stores
// (workgroup-scope release / acquire: s_waitcnt; a CU's vector L1 is write-through and coherent with its own stores) is all it takes.
// For: all-opaque scenes without media, escape lights or light preselection whose only material kind is Matte under simple lights
// (launch_small_pass says which; everything else keeps the launches).
// ---------------------------------------------------------------------------------------------------
template <typename ACC, int G = 1>   // (G = 1: the wave's 256 staging floats, all a stack has to spare)
__device__ __forceinline__ void film_tile(const DPathState& st, const DFrame& fr, const DTables& T, ACC* __restrict__ accum, float* __restrict__ mine, int tile);
__device__ __forceinline__ void stage_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// GENERAL: the kinds with a light-weight shade body — Matte (under any lights), Mirror, Glass, Conductor — whichever the scene has, and K7 for
// escape lights (escaped_body); two waves per SIMD (512-thread blocks and below), where the union of their registers fits.
// STACK = 32: trees deeper than 16 levels (the 10^6-triangle scene; its next-event light comes from the shade body's own descent of the
// light BVH — what k_light_select would have chosen, test_light_preselection_is_result_neutral).
template <int NC, int BLOCK, bool GENERAL = false, int STACK = 16>
__global__ void __attribute__((amdgpu_flat_work_group_size(BLOCK, BLOCK), amdgpu_waves_per_eu(BLOCK / 256))) k_small_pass(DPathState st, DScene sc, DTables T, DFrame fr, DFilter flt, DCamera cam, DSobol sob,
                                                                                                                            int max_depth, int shadows, int merged, void* accum, int film_mode, uint32_t kinds_mask, DStats* stats) {
    __shared__ int lds_stack[(BLOCK / 64) * STACK * 64];
    __shared__ float4 lds_box[3 * NC];
    __shared__ int2 lds_child[NC];
    __shared__ uint32_t emit_list[(BLOCK / 64) * 128];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    uint32_t* elist = emit_list + (threadIdx.x >> 6) * 128;
    const NodeCache cache = node_cache_fill<NC, BLOCK>(sc, lds_box, lds_child);
#ifdef HK_DEBUG_UTIL   // cycles per wave and stage (probes 10 - 13: camera, trace, shade, shadow — "x of y": average cycles of a wave's stage calls / 64)
    unsigned long long t_stage[4] = {0, 0, 0, 0}, n_stage[4] = {0, 0, 0, 0};
#define HK_STAGE_T(i, call) do { const unsigned long long t0_ = __builtin_readcyclecounter(); call; t_stage[i] += __builtin_readcyclecounter() - t0_; n_stage[i] += 64; } while (0)
#else
#define HK_STAGE_T(i, call) call
#endif
    for (int g = global_wave(); g < st.n_waves; g += physical_waves()) {
        HK_STAGE_T(0, camera_body(st, fr, T, flt, cam, sob, seg_single(st, g)));
        stage_fence();
        HK_STAGE_T(1, (trace_lean_body<false, NC>(st, sc, 0, stats, seg_single(st, g), stack, cache)));
        for (int depth = 0; depth < max_depth; ++depth) {
            stage_fence();
            if (!GENERAL)
                HK_STAGE_T(2, (shade_body<HK_MAT_MATTE, true, false, false>(st, sc, T, fr, sob, depth, 1, stats, seg_single(st, g), elist)));
            else {
                if (sc.has_escape_lights) escaped_body<1>(st, sc, T, depth, fr.implicit_ones, seg_single(st, g));
                int first_kind = 1;   // the kinds in ascending order, each continuing the shadow / next-ray queues of the one before (as the launches do)
#define HK_SMALL_KIND(K, S)                                                                                                                   \
    if (kinds_mask & (1u << K)) {                                                                                                             \
        if (!first_kind) stage_fence();                                                                                                       \
        HK_STAGE_T(2, (shade_body<K, S, false, false>(st, sc, T, fr, sob, depth, first_kind, stats, seg_single(st, g), elist)));            \
        first_kind = 0;                                                                                                                       \
    }
                if (sc.simple_lights) {
                    HK_SMALL_KIND(HK_MAT_MATTE, true)
                } else {
                    HK_SMALL_KIND(HK_MAT_MATTE, false)
                }
                HK_SMALL_KIND(HK_MAT_MIRROR, false)
                HK_SMALL_KIND(HK_MAT_GLASS, false)
                HK_SMALL_KIND(HK_MAT_CONDUCTOR, false)
#undef HK_SMALL_KIND
            }
            stage_fence();
            // the shadow rays of this bounce and the rays of the next one, together (trace_shadow_body)
            if (depth + 1 < max_depth) {
                if (shadows && merged)
                    HK_STAGE_T(3, (trace_shadow_body<NC>(st, sc, depth, stats, g, stack, cache)));
                else {
                    if (shadows) HK_STAGE_T(3, (shadow_body<false, NC>(st, sc, depth, stats, seg_single(st, g), stack, cache)));
                    HK_STAGE_T(1, (trace_lean_body<false, NC>(st, sc, depth + 1, stats, seg_single(st, g), stack, cache)));
                }
            } else if (shadows)
                HK_STAGE_T(3, (shadow_body<false, NC>(st, sc, depth, stats, seg_single(st, g), stack, cache)));
        }
        // K12 for a one-sample pass: chunk c of the camera IS tile c, and this segment's chunks are g, g + W, ... — the wave adds its own
        // paths to the film (film_tile: k_film's arithmetic; the traversal stacks are free now: 256 of their floats stage the colours)
        if (film_mode) {
            stage_fence();
            const int n_tiles = fr.n_pixels_padded >> 6;
            for (int tile = g; tile < n_tiles; tile += st.n_waves) {
                if (film_mode == 2)
                    film_tile<double>(st, fr, T, (double*)accum, reinterpret_cast<float*>(stack), tile);
                else
                    film_tile<float>(st, fr, T, (float*)accum, reinterpret_cast<float*>(stack), tile);
            }
        }
    }
#ifdef HK_DEBUG_UTIL
    if (lane_id() == 0)
        for (int i = 0; i < 4; ++i) {
            (stats + global_wave())->dbg[20 + 2 * i] += n_stage[i];
            (stats + global_wave())->dbg[21 + 2 * i] += t_stage[i];
        }
#endif
#undef HK_STAGE_T
}
