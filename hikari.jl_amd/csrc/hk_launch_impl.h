// hk_launch_impl.h — the launch layer (hk_launch.h): part of the hk_kernels.hip translation unit, included after the kernels.
// Every resident-grid launch goes through launch_resident; a run-time bool or small integer class that selects a template argument goes
// through with_bool / with_int.  A new kernel instantiation is one more call of those — the compiler checks its arguments.
#pragma once
#include "hk_launch.h"

namespace hk {

template <bool V>
using bool_c = std::bool_constant<V>;
template <int V>
using int_c = std::integral_constant<int, V>;
// f(bool_c<b>{}): a run-time bool as a template argument (decltype(arg)::value inside a generic lambda)
template <class F>
static void with_bool(bool b, F&& f) {
    if (b) f(bool_c<true>{});
    else f(bool_c<false>{});
}
// f(int_c<V>{}) for the V of the list that equals v; the LAST one when none does (the list's default case)
template <int V0, int... Vs, class F>
static void with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(int_c<V0>{});
    else if (v == V0) f(int_c<V0>{});
    else with_int<Vs...>(v, f);
}

#ifndef HK_OCC_SCALE_DEFAULT
#define HK_OCC_SCALE_DEFAULT 1.0f
#endif
static inline int grid_for(int n, int block, int cap) {
    long g = ((long)n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// blocks per CU that are actually resident for a kernel (occupancy API, capped): the wave-segment loop makes any
// grid size correct, so the grid is sized to residency instead of oversubscribing and paying a tail round.
template <class K>
static int resident_blocks(K kernel, int block) {   // blocks per CU as the occupancy API reports them (uncapped)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    return per_cu;
}
// HK_OCC_SCALE (round 6): the occupancy API of this ROCm answers HALF of what the register file admits for the 256-thread kernels here
// (k_camera, 52 VGPRs: 4 blocks per CU where 512 / 56 registers give 8 waves per SIMD = 8 blocks; MI355X_MICROARCH.md "Register files").
// Grids are sized by `answer x scale`, capped at the caller's cap (8 blocks = 32 waves per CU, the hardware's own limit) — a block the
// CU cannot hold simply starts later, and the ticketed / strided segment loops make any grid size correct.
static float occ_scale() {
    const char* e = hk::knob("HK_OCC_SCALE");
    const float v = e ? (float)std::atof(e) : HK_OCC_SCALE_DEFAULT;
    return v >= 0.25f && v <= 8.0f ? v : 1.0f;
}
// Residency is a property of (kernel, device): cached per kernel instantiation AND per device, so one process can drive several
// GPUs (the in-library multi-device path) without one device's answer leaking to another.
#define HK_MAX_DEVICES 64
template <auto Kernel>
static int cached_blocks(int block, int n_cu, int cap_per_cu) {
    static int cache[HK_MAX_DEVICES];
    int dev = 0, per_cu;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= HK_MAX_DEVICES)
        per_cu = resident_blocks(Kernel, block);
    else {
        if (cache[dev] == 0) {
            cache[dev] = resident_blocks(Kernel, block);
            if (hk::knob("HK_DEBUG_ALLOC")) std::fprintf(stderr, "HK_DEBUG_ALLOC occupancy API: %d blocks of %d per CU for %s\n", cache[dev], block, __PRETTY_FUNCTION__);
        }
        per_cu = cache[dev];
    }
    per_cu = (int)((float)per_cu * occ_scale() + 0.5f);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > cap_per_cu) per_cu = cap_per_cu;
    return per_cu * n_cu;
}
// Segments are walked with a static stride, so the number of physical waves must DIVIDE W or the last round runs with a
// fraction of the waves (shade at W = 16/CU with 12 resident: 12 % slower than at W = 24): the largest divisor of the
// 4-wave block count that is resident.
static int clamp_blocks(int blocks, const DPathState& st, int waves_per_block = 4) {
    const int units = st.n_waves / waves_per_block;
    if (blocks >= units) return units;
    if (st.dynamic_segments) return blocks;
    int best = 1;
    for (int b = blocks; b >= 1; --b)
        if (units % b == 0) {
            best = b;
            break;
        }
    // a divisor far below residency wastes more than the tail round it avoids
    return best * 4 >= blocks * 3 ? best : blocks;
}
// K(st, args...) over the wave segments of st: as many blocks as are resident (at most cap_per_cu per CU), clamped to the segment count.
template <auto K, class... A>
static void launch_resident(hipStream_t s, int n_cu, const DPathState& st, int block, int cap_per_cu, A&&... args) {
    const int blocks = cached_blocks<K>(block, n_cu, cap_per_cu);
    hipLaunchKernelGGL(K, dim3(clamp_blocks(blocks, st, block / 64)), dim3(block), 0, s, st, args...);
}

// ---- the A/B switches of the launch layer, looked up per launch in the context's knob table ----
static bool node_cache_on() { return knob_on("HK_NODE_CACHE"); }           // 0: the lean kernels read every node from global memory
static int grey_mode() { return knob_int("HK_GREY", 1); }                   // 0: flat-spectrum media run through the general tracking kernels
static int grey_flat_mode() { return knob_int("HK_GREY_FLAT", 1); }         // 0: grey media run through the round-3 GREY instantiations of k_track / k_shadow_walk
static int walk_pool_mode() { return knob_int("HK_WALK_POOL", 1); }         // 0: k_shadow_walk<.., GREY> instead of k_walk_pool; 1: 8-entry stacks where the tree allows; other: 16
static int track_pool_mode() { return knob_int("HK_TRACK_POOL", 1); }       // 0: k_track_flat instead of k_track_pool
// both sampler tables hold every draw of this bounce (rows up to 9 + 5 depth: sobol_row) for every path of the pass: the table-only
// instantiations (HK_SOBOL_TABLE_ONLY=0: always the general ones)
static bool sobol_tables_cover(const DSobol& sob, int depth) {
    return sob.hi_table != nullptr && sob.lo_table != nullptr && 9 + 5 * depth < sob.lo_rows && 9 + 5 * depth < sob.hi_rows && knob_on("HK_SOBOL_TABLE_ONLY");
}
// media kernels are instantiated for a single medium kind or for all four (15)
static int media_mask_class(const DScene& sc) {
    int m = sc.media_mask;
    return (m == 1 || m == 2 || m == 4 || m == 8) ? m : 15;
}

void launch_camera(hipStream_t s, int n_cu, const DPathState& st, const DFrame& fr, const DTables& T, const DFilter& flt, const DCamera& cam, const DSobol& sob, int initial_medium) {
    launch_resident<k_camera>(s, n_cu, st, 256, 8, fr, T, flt, cam, sob, initial_medium);
}

// k_trace_lean over a BVH of depth <= 16: ONE 1024-thread block per CU (the 4 waves per SIMD its registers allow anyway) whose LDS
// holds the 16 stacks (64 KB) and the top 1536 nodes of the tree (84 KB) — all of the Cornell box, the upper levels of the others.
// Measured (HK_NODE_CACHE=0 switches it off): trace -11 % in the Cornell box and the sky scene; with the 32-entry stacks of the
// 10^6-triangle scene 512 nodes are a small part of the visits (+-1 %: no cache there).
// The any-hit kernel lives on residency (7 waves per SIMD on 16 KB of stacks; the big cache cost it three of them: +3 %), so it
// gets the cache that FITS beside them.  Round 6 (two-spheres Cornell box, A B | B A): what counts is nodes per WAVE-SLOT — a cache is shared by the
// waves of its block, so bigger blocks buy more of the tree for the same LDS.  12-wave blocks with the top 560 nodes (48 KB of stacks + 31 KB of
// nodes, two blocks per CU = 6 waves per SIMD): k_shadow 17.55 -> 16.4 ms per Cornell frame, sky 2.6 -> 2.5.  On the way: 4-wave blocks with
// 112 nodes (rounds 3-5, seven blocks per CU) 17.55, 176 nodes (six blocks) 17.0, 192 / 240 / 320 nodes (five, five, four blocks) 18.5 / 18.3 /
// 20.3; 8-wave blocks with 384 nodes 20.2 and 14-wave blocks with 432 nodes 22.5 (one block short of the plan each); 16-wave blocks with the
// whole tree (four waves per SIMD) 17.0.
#ifndef HK_SHADOW_NC16
#define HK_SHADOW_NC16 560
#endif
#ifndef HK_SHADOW_BLOCK16   // threads per block of the any-hit kernel over trees <= 16 deep
#define HK_SHADOW_BLOCK16 768
#endif
#ifndef HK_SHADOW_NC32
#define HK_SHADOW_NC32 0
#endif
#ifndef HK_TRACE_SINGLE_KIND   // 0: scenes of one material kind run k_trace_lean's Mix-free flush instead of the single-kind one (A/B builds)
#define HK_TRACE_SINGLE_KIND 1
#endif
#ifndef HK_TRACE_NC32
#define HK_TRACE_NC32 128   // 10^6-triangle scene: trace -1.3 % (256 nodes cost a block per CU: +15 %)
#endif
// The instantiation of a lean kernel (k_trace_lean / k_shadow: <COUNT, STACK, BLOCK, NC, QN>) for this tree: launch(COUNT, STACK, BLOCK, NC, QN).
// A tree at most 16 deep: 16-entry stacks, blocks of B16 threads that cache its top NC16 nodes; a deeper one: HK_LDS_STACK entries, NC32
// nodes, and its quantised nodes (DScene::qnodes) where the scene has them.  HK_NODE_CACHE=0: no cache (honoured for the quantised tree too,
// ADVICE r5), and then the plain block.
template <int B16, int NC16, int NC32, class F>
static void lean_dispatch(const DScene& sc, const DFrame& fr, F&& launch) {
    with_bool(fr.count_nodes != 0, [&](auto COUNT) {
        with_bool(node_cache_on(), [&](auto CACHE) {
            constexpr bool cache = decltype(CACHE)::value;
            if (sc.bvh_depth <= 16) launch(COUNT, int_c<16>{}, int_c<cache ? B16 : HK_TRACE_BLOCK>{}, int_c<cache ? NC16 : 0>{}, bool_c<false>{});
            else with_bool(sc.qnodes != nullptr, [&](auto QN) { launch(COUNT, int_c<HK_LDS_STACK>{}, int_c<HK_TRACE_BLOCK>{}, int_c<cache ? NC32 : 0>{}, QN); });
        });
    });
}
// The flush of k_trace_lean's instantiation follows the scene's materials (DScene::has_mix / single_kind, kept current by
// hk_scene_update_materials): 0 with the MixMaterial resolve, 1 without it, 2 without it and for ONE material kind.  The counting
// instantiations (count_nodes, a diagnostic) are not multiplied: they keep the general flush.
static int lean_flush(const DScene& sc, const DFrame& fr) { return (sc.has_mix || fr.count_nodes) ? 0 : (HK_TRACE_SINGLE_KIND && sc.single_kind >= 0 ? 2 : 1); }
void launch_trace(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth, DStats* stats) {
    if (lean_scene(sc)) {
        const int flush = lean_flush(sc, fr);
        lean_dispatch<1024, 1536, HK_TRACE_NC32>(sc, fr, [&](auto COUNT, auto STACK, auto BLOCK, auto NC, auto QN) {
            constexpr int block = decltype(BLOCK)::value;
            constexpr bool count = decltype(COUNT)::value;
            with_int<2, 1, 0>(flush, [&](auto FLUSH) {
                constexpr int f = count ? 0 : decltype(FLUSH)::value;
                launch_resident<k_trace_lean<count, decltype(STACK)::value, block, decltype(NC)::value, decltype(QN)::value, f == 0, f == 2>>(s, n_cu, st, block, 8, sc, depth, stats);
            });
        });
        return;
    }
    with_bool(fr.count_nodes != 0, [&](auto COUNT) { launch_resident<k_trace<decltype(COUNT)::value>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, T, fr, depth, stats); });
}
template <bool C, int MM>
static void launch_walk_split(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DFrame& fr, int depth, DStats* stats) {
    const int cb = clamp_blocks(cached_blocks<k_walk_cast<C, MM, 16>>(HK_TRACE_BLOCK, n_cu, 8), st);
    const int tb = clamp_blocks(cached_blocks<k_walk_track<MM>>(256, n_cu, 8), st);
    for (int round = 0; round < HK_WALK_ROUNDS; ++round) {
        hipLaunchKernelGGL((k_walk_cast<C, MM, 16>), dim3(cb), dim3(HK_TRACE_BLOCK), 0, s, st, sc, depth, round, stats, sc.media);
        hipLaunchKernelGGL((k_walk_track<MM>), dim3(tb), dim3(256), 0, s, st, sc, depth, round, fr.walk_tune, stats, sc.media);
    }
}
// The compact records (r_u == 1 not stored, r_l one float: DPathState::compact) also hold in a scene whose one medium is grey AND runs
// through the pool kernels (k_track_pool / k_walk_pool, the only media kernels that know the compact layout): r_u is never touched
// there and every factor of r_l is a scalar.  HK_GREY_COMPACT=0: the full records.
bool grey_compact_ok(const DScene& sc) {
    if (!knob_on("HK_GREY_COMPACT")) return false;
    const int mc = sc.n_media > 0 ? media_mask_class(sc) : 0;
    return sc.n_media == 1 && sc.all_grey && sc.grey_pool && (mc == 2 || mc == 8) && sc.bvh_depth <= 16 && grey_mode() && grey_flat_mode() && track_pool_mode() && walk_pool_mode() &&
           !walk_split_mode();
}
// the shadow walk through surfaces that let rays pass and through media of class MM (0: no medium)
template <bool C, int MM>
static void launch_shadow_walk(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth, DStats* stats) {
    constexpr bool grey_kind = MM == 2 || MM == 8;   // the media kinds with GREY / pool instantiations
    constexpr int M2 = grey_kind ? MM : 8;
    const bool shallow = sc.bvh_depth <= 16;   // 16-entry stacks: 16 KB per block
    const int pool = walk_pool_mode();
    if (shallow && grey_kind && sc.grey_pool && grey_mode() && grey_flat_mode() && pool) {
        if (M2 == 8 && sc.grey_bricks && sc.bvh_depth <= 8 && pool == 1)
            launch_resident<k_walk_pool<C, 8, true, 8, 64>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, depth, fr.walk_tune, fr.track_gate, stats, sc.media);
        else if (M2 == 8 && sc.grey_bricks)
            launch_resident<k_walk_pool<C, 8, true, 16, 56>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, depth, fr.walk_tune, fr.track_gate, stats, sc.media);
        else
            launch_resident<k_walk_pool<C, M2, false, 16, 56>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, depth, fr.walk_tune, fr.track_gate, stats, sc.media);
    } else if (shallow && grey_kind && sc.all_grey && grey_mode())
        launch_resident<k_shadow_walk<C, M2, 16, true>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, T, depth, fr.walk_tune, stats, sc.media);
    else if (shallow)
        launch_resident<k_shadow_walk<C, MM, 16>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, T, depth, fr.walk_tune, stats, sc.media);
    else
        launch_resident<k_shadow_walk<C, MM>>(s, n_cu, st, HK_TRACE_BLOCK, 8, sc, T, depth, fr.walk_tune, stats, sc.media);
}
void launch_shadow(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth, DStats* stats) {
    if (lean_scene(sc)) {
        lean_dispatch<HK_SHADOW_BLOCK16, HK_SHADOW_NC16, HK_SHADOW_NC32>(sc, fr, [&](auto COUNT, auto STACK, auto BLOCK, auto NC, auto QN) {
            constexpr int block = decltype(BLOCK)::value;
            launch_resident<k_shadow<decltype(COUNT)::value, decltype(STACK)::value, block, decltype(NC)::value, decltype(QN)::value>>(s, n_cu, st, block, 8, sc, depth, stats);
        });
        return;
    }
    const int mc = sc.n_media > 0 ? media_mask_class(sc) : 0;
    const bool split = sc.all_grey && grey_mode() && walk_split_mode() && sc.bvh_depth <= 16 && st.wq_a != nullptr;
    with_bool(fr.count_nodes != 0, [&](auto COUNT) {
        constexpr bool c = decltype(COUNT)::value;
        if (split && mc == 8) launch_walk_split<c, 8>(s, n_cu, st, sc, fr, depth, stats);
        else if (split && mc == 2) launch_walk_split<c, 2>(s, n_cu, st, sc, fr, depth, stats);
        else with_int<0, 1, 2, 4, 8, 15>(mc, [&](auto MM) { launch_shadow_walk<c, decltype(MM)::value>(s, n_cu, st, sc, T, fr, depth, stats); });
    });
}
// work lists of up to HK_MAX_KINDS + 6 queues (pairs depth, queue id) in one launch
void launch_segment_lists(hipStream_t s, const DPathState& st, int n, const int* depths, const int* queues) {
    if (n <= 0) return;
    SegQueues qs;
    qs.n = n;
    for (int i = 0; i < n; ++i) {
        qs.depth[i] = depths[i];
        qs.q[i] = queues[i];
    }
    hipLaunchKernelGGL(k_segment_lists, dim3(n, HK_LIST_SPLIT), dim3(1024), 0, s, st, qs);
}
// The lean k_shade reads the geometric normal and the area of the hit triangle from the scene's table (DScene::tri_geo) where there is
// one; HK_TRI_GEO=0 (A/B switch; films bit-identical): it computes them from the positions, as every other caller of surface_at does.
static bool tri_geo_on(const DScene& sc) { return sc.tri_geo != 0 && knob_on("HK_TRI_GEO"); }
void launch_medium(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, DStats* stats) {
    {
        const int d = depth, q = Q_MEDIUM;
        launch_segment_lists(s, st, 1, &d, &q);
    }
    const bool grey = sc.all_grey && grey_mode();
    const bool flat = grey && grey_flat_mode();
    const bool pool = flat && track_pool_mode() && sc.grey_pool;
    auto track = [&](auto MM, auto GREY) { launch_resident<k_track<decltype(MM)::value, decltype(GREY)::value>>(s, n_cu, st, 256, 8, sc, T, fr, depth, stats, sc.media); };
    auto track_flat = [&](auto MM, auto BRICKS) {
        constexpr int mm = decltype(MM)::value;
        constexpr bool bricks = decltype(BRICKS)::value;
        if (pool) launch_resident<k_track_pool<mm, bricks>>(s, n_cu, st, 256, 8, sc, fr, depth, stats, sc.media);
        else launch_resident<k_track_flat<mm, bricks>>(s, n_cu, st, 256, 8, sc, fr, depth, stats, sc.media);
    };
    switch (media_mask_class(sc)) {   // (only homogeneous (2) and grid (8) media have grey instantiations, only grids have bricks)
        case 1: track(int_c<1>{}, bool_c<false>{}); break;
        case 2:
            if (flat) track_flat(int_c<2>{}, bool_c<false>{});
            else with_bool(grey, [&](auto GREY) { track(int_c<2>{}, GREY); });
            break;
        case 4: track(int_c<4>{}, bool_c<false>{}); break;
        case 8:
            if (flat) with_bool(sc.grey_bricks != 0, [&](auto BRICKS) { track_flat(int_c<8>{}, BRICKS); });
            else with_bool(grey, [&](auto GREY) { track(int_c<8>{}, GREY); });
            break;
        default: track(int_c<15>{}, bool_c<false>{}); break;
    }
    {
        const int d = depth, q = Q_SCATTER;
        launch_segment_lists(s, st, 1, &d, &q);
    }
    with_bool(sobol_tables_cover(sob, depth), [&](auto FT) { launch_resident<k_scatter<decltype(FT)::value>>(s, n_cu, st, 256, 8, sc, T, fr, sob, depth, stats); });
}
void launch_detect_camera_medium(hipStream_t s, const DPathState& st, const DScene& sc, float x, float y, float z, DStats* stats) {
    hipLaunchKernelGGL(k_detect_camera_medium, dim3(1), dim3(64), 0, s, st, sc, x, y, z, stats);
}
void launch_escaped(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth) {
    // HK_ESCAPED_UNROLL=2: two queue entries per lane and iteration (A/B switch; films bit-identical).  Measured, sky: 8.9 -> 10.4 ms per
    // frame — its registers cost the kernel a block per CU (3 instead of 4); off.  (One wave per segment instead of the resident stride: +-0, sky)
    with_bool(knob_int("HK_ESCAPED_UNROLL", 1) != 2, [&](auto ONE) { launch_resident<k_escaped<decltype(ONE)::value ? 1 : 2>>(s, n_cu, st, 256, 8, sc, T, depth, fr.implicit_ones); });
}
// scenes whose next-event light is chosen by k_light_select before the shade kernels run (HK_PRESELECT=0: never)
bool preselect_lights(const DScene& sc, const DPathState& st) {
    return sc.n_media == 0 && sc.num_bvh_lights >= HK_PRESELECT_MIN && st.sel_light != nullptr && knob_on("HK_PRESELECT");
}
void launch_light_select(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, uint32_t kinds_mask, DStats* stats) {
    const int min_idle = knob_int_in("HK_SELECT_MIN_IDLE", 1, 64, HK_SELECT_MIN_IDLE);
    const bool pool = knob_on("HK_SELECT_POOL");   // 0: the per-lane-refill kernel of round 4 (A/B switch; films bit-identical)
    with_bool(sobol_tables_cover(sob, depth), [&](auto FT) {
        constexpr bool ft = decltype(FT)::value;
        if (pool) launch_resident<k_light_select_pool<ft>>(s, n_cu, st, HK_SELECT_BLOCK, 8, sc, T, fr, sob, depth, kinds_mask, stats);
        else launch_resident<k_light_select<ft>>(s, n_cu, st, 256, 8, sc, T, fr, sob, depth, kinds_mask, min_idle, stats);
    });
}
void launch_shade(hipStream_t s, int n_cu, int kind, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, int first_kind, DStats* stats) {
    auto shade = [&](auto KIND, auto SIMPLE, auto FT, auto PRE) {
        launch_resident<k_shade<decltype(KIND)::value, decltype(SIMPLE)::value, decltype(FT)::value, decltype(PRE)::value>>(s, n_cu, st, 256, 8, sc, T, fr, sob, depth, first_kind, stats);
    };
    const bool ft = sobol_tables_cover(sob, depth);
    // Matte under simple lights in a lean scene whose state holds the lean records (compact, 32-bit meta words, the slim shadow record):
    // the LEAN instantiation — those facts at compile time, the second half's values handed over through LDS, five waves per SIMD
    // (HK_SHADE_LEAN=0: the general instantiation; A/B switch, films bit-identical)
    if (kind == HK_MAT_MATTE && sc.simple_lights && lean_scene(sc) && st.compact && st.meta32 && st.sh_final && !preselect_lights(sc, st) && knob_on("HK_SHADE_LEAN")) {
        // ... and by slot instead of through the kind queue where the scene is all Matte and this bounce's trace launch marked the escaped
        // entries (the single-kind flush); decided per launch: hk_scene_update_materials changes single_kind (HK_SHADE_SLOT_WALK=0: never)
        const bool slots = shade_slot_walk_launch(st.shade_slot_walk, sc.single_kind, kind, lean_flush(sc, fr) == 2);
        with_bool(ft, [&](auto FT) {
            with_bool(slots, [&](auto SLOTS) {
                with_bool(tri_geo_on(sc), [&](auto GEO) {   // the geometric normal and the area from the scene's table (HK_TRI_GEO=0: from the positions)
                    launch_resident<k_shade<HK_MAT_MATTE, true, decltype(FT)::value, false, true, decltype(SLOTS)::value, decltype(GEO)::value>>(s, n_cu, st, 256, 8, sc, T, fr, sob, depth, first_kind, stats);
                });
            });
        });
        return;
    }
    // the kinds with next-event instantiations of their own (table-only draws, a light chosen beforehand); the others run k_shade<KIND>
    const bool light_kind = kind == HK_MAT_MATTE || kind == HK_MAT_MIRROR || kind == HK_MAT_GLASS || kind == HK_MAT_CONDUCTOR;
    if (light_kind && preselect_lights(sc, st))   // k_light_select has run for this depth: the instantiations without the light-BVH descent
        with_int<HK_MAT_MATTE, HK_MAT_MIRROR, HK_MAT_GLASS, HK_MAT_CONDUCTOR>(kind, [&](auto KIND) { with_bool(ft, [&](auto FT) { shade(KIND, bool_c<false>{}, FT, bool_c<true>{}); }); });
    else if (kind == HK_MAT_MATTE && sc.simple_lights)
        with_bool(ft, [&](auto FT) { shade(int_c<HK_MAT_MATTE>{}, bool_c<true>{}, FT, bool_c<false>{}); });
    else if (light_kind && ft)
        with_int<HK_MAT_MATTE, HK_MAT_MIRROR, HK_MAT_GLASS, HK_MAT_CONDUCTOR>(kind, [&](auto KIND) { shade(KIND, bool_c<false>{}, bool_c<true>{}, bool_c<false>{}); });
    else
        with_int<HK_MAT_MATTE, HK_MAT_MIRROR, HK_MAT_GLASS, HK_MAT_CONDUCTOR, HK_MAT_COATED_DIFFUSE, HK_MAT_THIN_DIELECTRIC, HK_MAT_DIFFUSE_TRANSMISSION, HK_MAT_COATED_DIFFUSE_TRANSMISSION,
                 HK_MAT_COATED_CONDUCTOR, HK_MAT_FALLBACK>(kind, [&](auto KIND) { shade(KIND, bool_c<false>{}, bool_c<false>{}, bool_c<false>{}); });
}
// k_small_pass: the whole pass of a small call in one launch.
#ifndef HK_SMALL_PASS_NC
#define HK_SMALL_PASS_NC 1536
#endif
// the scenes k_small_pass is instantiated for (the pass itself must be a small one: launch_small_pass): -> 0 none, 1 the all-matte closed
// scene under simple lights, 2 the general instantiation (Matte / Mirror / Glass / Conductor, escape lights)
static int small_pass_class(const DScene& sc, uint32_t kinds_mask) {
    const int mode = knob_int("HK_SMALL_PASS_FUSED", 2);   // 0: the stages as launches, 1: only the all-matte instantiation (A/B switch; films bit-identical)
    if (mode == 0) return 0;
    if (!(lean_scene(sc) && sc.bvh_depth <= HK_LDS_STACK && node_cache_on())) return 0;
    if (kinds_mask == (1u << HK_MAT_MATTE) && sc.simple_lights && !sc.has_escape_lights && sc.bvh_depth <= 16 && sc.num_bvh_lights < HK_PRESELECT_MIN) return 1;
    const uint32_t light_kinds = (1u << HK_MAT_MATTE) | (1u << HK_MAT_MIRROR) | (1u << HK_MAT_GLASS) | (1u << HK_MAT_CONDUCTOR);
    return (mode >= 2 && kinds_mask != 0 && (kinds_mask & ~light_kinds) == 0) ? 2 : 0;
}
bool small_pass_fusable(const DScene& sc, uint32_t kinds_mask) { return small_pass_class(sc, kinds_mask) != 0; }
// one block per CU (its LDS: 16-entry stacks, the top of the tree, the emission lists) of as many waves as the pass has segments per CU;
// -> false when the pass has fewer segments than one block's waves
template <int BLOCK, bool GENERAL, int STACK, class... A>
static bool small_pass_blocks(hipStream_t s, int n_cu, const DPathState& st, bool dry, A&&... args) {
    constexpr auto kernel = k_small_pass<HK_SMALL_PASS_NC, BLOCK, GENERAL, STACK>;
    int blocks = cached_blocks<kernel>(BLOCK, n_cu, 1);
    if (blocks * (BLOCK / 64) > st.n_waves) blocks = st.n_waves / (BLOCK / 64);
    if (blocks < 1) return false;
    if (!dry) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), 0, s, st, args...);
    return true;
}
bool launch_small_pass(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DFilter& flt, const DCamera& cam, const DSobol& sob, int max_depth,
                       uint32_t kinds_mask, DStats* stats, bool dry, void* accum, int film_mode) {
    const int cls = small_pass_class(sc, kinds_mask);
    if (cls == 0 || !st.small_pass || st.dynamic_segments || fr.count_nodes) return false;
    // a SMALL pass in ensure_state's sense (at most 16 chunks for each of 4 waves per CU), not the mid-size pass that shares its static
    // segments: with 25 chunks per stage the launches' higher residency wins (800^2 x 32 spp without sampler tables: 14.8 ms as launches, 17.2 here)
    if (((long)st.capacity + 63) / 64 / 16 > 4L * n_cu) return false;
    for (int depth = 0; depth < max_depth; ++depth)
        if (sobol_tables_cover(sob, depth)) return false;
    const int merged = knob_on("HK_SMALL_PASS_MERGED") ? 1 : 0;   // 0: shadow rays and the next bounce's rays as two stages (A/B switch; films bit-identical)
    // (Cornell 800^2, one sample per call: 1.42 / 1.05 / 1.14 ms at 4 / 8 / 16 segments per CU — 256- / 512- / 1024-thread blocks; a 768-thread
    // block for 12: 1.55.  Eight waves per CU hold 312 paths each: chunks stay fuller down the bounces than with 156, and at two waves per
    // SIMD nothing spills.)
    // two waves per SIMD at most: at 16 segments per CU (1 024-thread blocks, 128 registers) the matte instantiation spilled 372 B per lane
    // and lost to 8 (1.14 ms against 1.05), the general one does not fit at all — such a pass keeps the launches
    if (st.n_waves > 8 * n_cu) return false;
    bool launched = false;
    auto pass = [&](auto GENERAL, auto STACK) {   // 512-thread blocks for 8 segments per CU, 256-thread blocks for 4
        with_bool(st.n_waves > 4 * n_cu, [&](auto WIDE) {
            launched = small_pass_blocks<decltype(WIDE)::value ? 512 : 256, decltype(GENERAL)::value, decltype(STACK)::value>(s, n_cu, st, dry, sc, T, fr, flt, cam, sob, max_depth, sc.n_lights > 0 ? 1 : 0, merged,
                                                                                                                       accum, film_mode, kinds_mask, stats);
        });
    };
    if (cls == 2 && sc.bvh_depth > 16) pass(bool_c<true>{}, int_c<HK_LDS_STACK>{});
    else if (cls == 2) pass(bool_c<true>{}, int_c<16>{});
    else pass(bool_c<false>{}, int_c<16>{});
    return launched;
}
void launch_film(hipStream_t s, const DPathState& st, const DFrame& fr, const DTables& T, void* accum, bool f64) {
    int g = grid_for(fr.n_pixels_padded >> 6, 4, 4096);   // one wave per 8x8 tile
    // the grouped fold's arm is that of passes of 64 k samples; every other pass keeps the one-pixel kernel and its 4 KB of LDS
    // (HK_FILM_FOLD=0: always the one-pixel kernel; A/B switch, films bit-identical)
    const bool fold = film_fold_launch(knob_on("HK_FILM_FOLD"), fr.samples_in_pass);
    if (f64) {   // (double accumulators keep the one-pixel kernel: grouped it takes 70 registers and loses a wave per SIMD)
        hipLaunchKernelGGL((k_film<double, 1>), dim3(g), dim3(256), 0, s, st, fr, T, (double*)accum);
    } else {
        if (fold) hipLaunchKernelGGL((k_film<float, HK_FILM_FOLD_G>), dim3(g), dim3(256), 0, s, st, fr, T, (float*)accum);
        else hipLaunchKernelGGL((k_film<float, 1>), dim3(g), dim3(256), 0, s, st, fr, T, (float*)accum);
    }
}
void launch_sobol_table(hipStream_t s, const DSobol& sob, const DFrame& fr, uint2* table, int rows) {
    hipLaunchKernelGGL(k_sobol_table, dim3(grid_for((long)rows * fr.n_pixels_padded > 0x3fffffff ? 0x3fffffff : rows * fr.n_pixels_padded, 256, 8192)), dim3(256), 0, s, sob, fr, table, rows);
}
void launch_sobol_lo_table(hipStream_t s, const DSobol& sob, const DFrame& fr, uint16_t* table, int rows, int base, int stride, int count) {
    hipLaunchKernelGGL(k_sobol_lo_table, dim3(65536), dim3(256), 0, s, sob, fr, table, rows, base, stride, count);
}
// ---- the display chain (hk_display.h): one launcher per stage, instantiated for both pixel layouts ----
template <class Layout>
void launch_finalize(hipStream_t s, const void* accum, bool f64, Layout out, int w, int h) {
    int g = grid_for(w * h, 256, 4096);
    if (f64)
        hipLaunchKernelGGL((k_finalize<double, Layout>), dim3(g), dim3(256), 0, s, (const double*)accum, out, w, h);
    else
        hipLaunchKernelGGL((k_finalize<float, Layout>), dim3(g), dim3(256), 0, s, (const float*)accum, out, w, h);
}
template <class Layout>
void launch_aux(hipStream_t s, const DScene& sc, const DCamera& cam, int h, int w, float miss_depth, float* albedo, Layout out) {
    hipLaunchKernelGGL(k_aux<Layout>, dim3(grid_for(h * w, HK_TRACE_BLOCK, 2048)), dim3(HK_TRACE_BLOCK), 0, s, sc, cam, h, w, miss_depth, albedo, out);
}
template <class Layout>
void launch_variance(hipStream_t s, Layout src, float* variance, int h, int w) {
    hipLaunchKernelGGL(k_variance<Layout>, dim3(grid_for(h * w, 256, 8192)), dim3(256), 0, s, src, variance, h, w);
}
template <class Layout>
void launch_postprocess(hipStream_t s, const hk_postprocess_params& P, Layout src, float* out, int h, int w) {
    hipLaunchKernelGGL(k_postprocess<Layout>, dim3(grid_for(h * w, 256, 8192)), dim3(256), 0, s, P, src, out, h, w);
}
// the host files call these two instantiations of each
template void launch_finalize<PlanarPixels>(hipStream_t, const void*, bool, PlanarPixels, int, int);
template void launch_aux<PlanarPixels>(hipStream_t, const DScene&, const DCamera&, int, int, float, float*, PlanarPixels);
template void launch_variance<PlanarPixels>(hipStream_t, PlanarPixels, float*, int, int);
template void launch_postprocess<PlanarPixels>(hipStream_t, const hk_postprocess_params&, PlanarPixels, float*, int, int);
template void launch_finalize<PackedPixels>(hipStream_t, const void*, bool, PackedPixels, int, int);
template void launch_aux<PackedPixels>(hipStream_t, const DScene&, const DCamera&, int, int, float, float*, PackedPixels);
template void launch_variance<PackedPixels>(hipStream_t, PackedPixels, float*, int, int);
template void launch_postprocess<PackedPixels>(hipStream_t, const hk_postprocess_params&, PackedPixels, float*, int, int);
template <class Layout, bool FINAL>
static void atrous(hipStream_t s, const hk_denoise_params& P, int step, Layout src, const float* variance, Layout dst, float* out, const hk_postprocess_params* pp, int h, int w) {
    const hk_postprocess_params PP = pp ? *pp : hk_postprocess_params{};
    hipLaunchKernelGGL((k_atrous<Layout, FINAL>), dim3(grid_for(h * w, 256, 8192)), dim3(256), 0, s, P, PP, pp ? 1 : 0, step, src, variance, dst, out, h, w);
}
void launch_atrous(hipStream_t s, const hk_denoise_params& P, int step, PlanarPixels src, const float* variance, PlanarPixels dst, int h, int w) {
    atrous<PlanarPixels, false>(s, P, step, src, variance, dst, nullptr, nullptr, h, w);
}
void launch_atrous(hipStream_t s, const hk_denoise_params& P, int step, PackedPixels src, const float* variance, PackedPixels dst, float* out, const hk_postprocess_params* pp, int h, int w) {
    with_bool(out != nullptr, [&](auto FINAL) { atrous<PackedPixels, decltype(FINAL)::value>(s, P, step, src, variance, dst, out, pp, h, w); });
}
void launch_slot_of_prim(hipStream_t s, const float4* leaf, int n, int* slot_of_prim) {
    hipLaunchKernelGGL(k_slot_of_prim, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, leaf, n, slot_of_prim);
}
void launch_tri_geo(hipStream_t s, float* pos, int n, int tri_geo, float* shade) {
    if (n > 0) hipLaunchKernelGGL(k_tri_geo, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, pos, n, tri_geo_rows(pos, tri_geo), shade);
}
void launch_xform_tris(hipStream_t s, const DXform& X, int first, int n, const float* bp, const float* bn, const float* bt, const int* slot_of_prim, float* pos, float* nrm,
                       float* tan, float* shade, float4* geo, float4* leaf) {
    hipLaunchKernelGGL(k_xform_tris, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, X, first, n, bp, bn, bt, slot_of_prim, pos, nrm, tan, shade, geo, leaf);
}
void launch_refit_level(hipStream_t s, int begin, int end, DNode* nodes, DQNode* qnodes, const DQGrid& grid, const float4* leaf, const float* pos) {
    hipLaunchKernelGGL(k_refit_level, dim3(grid_for(end - begin, 256, 8192)), dim3(256), 0, s, begin, end, nodes, qnodes, grid, leaf, pos);
}
void launch_set_tris(hipStream_t s, const DSetTris& A) { hipLaunchKernelGGL(k_set_tris, dim3(grid_for(A.n, 256, 8192)), dim3(256), 0, s, A); }
void launch_light_refit_leaves(hipStream_t s, const DLightRefit& A) { hipLaunchKernelGGL(k_light_refit_leaves, dim3(grid_for(A.n, 256, 8192)), dim3(256), 0, s, A); }
void launch_light_refit_level(hipStream_t s, const int* entries, int count, const DLightRefit& A) {
    hipLaunchKernelGGL(k_light_refit_level, dim3(grid_for(count, 256, 8192)), dim3(256), 0, s, entries, count, A);
}
void launch_bvh_cost(hipStream_t s, const DNode* nodes, int n, double* partial) {
    hipLaunchKernelGGL(k_bvh_cost, dim3((unsigned)bvh_cost_blocks(n)), dim3(256), 0, s, nodes, n, partial);
}
// hk_scene_rebuild_bvh: every launch of the device builder (k_build_*), top level first; nothing is read back in between
void launch_bvh_build(hipStream_t s, const DBuild& B) {
    const int T = B.n_tris;
    hipLaunchKernelGGL(k_build_init, dim3(grid_for(T, 256, 8192)), dim3(256), 0, s, B);
    const int position_blocks = grid_for(T, 256, 2048), segment_blocks = std::min(T / (B.leaf + 1) + 1, 4096);
    for (int L = 0; L < HK_BUILD_MAX_LEVELS; ++L) {
        if (B.large_cap > 0) {
            hipLaunchKernelGGL(k_build_large_bounds, dim3(position_blocks), dim3(256), 0, s, B, L);
            hipLaunchKernelGGL(k_build_large_bins, dim3(position_blocks), dim3(256), 0, s, B, L);
        }
        hipLaunchKernelGGL(k_build_split, dim3(segment_blocks), dim3(256), 0, s, B, L);
        hipLaunchKernelGGL(k_build_emit, dim3(1), dim3(1024), 0, s, B, L);
    }
}
void launch_bvh_build_leaves(hipStream_t s, const DBuildLeaves& A) { hipLaunchKernelGGL(k_build_leaves, dim3(grid_for(A.n_tris, 256, 8192)), dim3(256), 0, s, A); }
// the Distribution2D tables of map `e` (a host copy of the record: sizes and table pointers) from its texels; `record` is the device record
void launch_envmap_tables(hipStream_t s, const DEnvMap& e, DEnvMap* record) {
    hipLaunchKernelGGL(k_envmap_rows, dim3((e.nv + 63) / 64), dim3(64), 0, s, e.data, e.nu, e.nv, const_cast<float*>(e.cond_func), const_cast<float*>(e.cond_cdf),
                       const_cast<float*>(e.cond_func_int), const_cast<float*>(e.marg_func));
    hipLaunchKernelGGL(k_envmap_marginal, dim3(1), dim3(64), 0, s, e.nv, e.marg_func, const_cast<float*>(e.marg_cdf), record);
}
void launch_sky_texels(hipStream_t s, const hk_sky_params& sky, int res, float4* data) {
    hipLaunchKernelGGL(k_sky_texels, dim3((unsigned)(((long long)res * res + 255) / 256)), dim3(256), 0, s, sky, res, data);
}

// The tables hk_scene_update_medium derives from the volume data of `m` (a host copy of the record the device will hold: sizes and the
// pointers to data already enqueued on `s`): the majorant grid into m.majorant, then its zero-cell mask into m.maj_zero.  A cell goes to
// one wave, or to a block when the mean box holds more than HK_MAJORANT_BLOCK_VOXELS (8192) voxels: 128 per lane and more.
static int majorant_block_per_cell(double box_voxels) { return box_voxels > (double)knob_int("HK_MAJORANT_BLOCK_VOXELS", 8192) ? 1 : 0; }
static void majorant_zero_mask(hipStream_t s, const DMedium& m, int ncell) {
    hipLaunchKernelGGL(k_majorant_zero_mask, dim3((unsigned)(((long long)ncell + 255) / 256)), dim3(256), 0, s, m.majorant, ncell, const_cast<uint32_t*>(m.maj_zero));
}
void launch_majorant_grid(hipStream_t s, const DMedium& m) {
    const int ncell = m.mres[0] * m.mres[1] * m.mres[2];
    const int per_block = majorant_block_per_cell((double)m.res[0] * m.res[1] * m.res[2] / ncell);
    const dim3 grid((unsigned)(per_block ? ncell : ((long long)ncell + 3) / 4));
    with_bool(m.kind == HK_MEDIUM_RGB_GRID, [&](auto RGB) {
        hipLaunchKernelGGL((k_majorant_grid<decltype(RGB)::value>), grid, dim3(256), 0, s, m, ncell, per_block, const_cast<float*>(m.majorant));
    });
    majorant_zero_mask(s, m, ncell);
}
void launch_majorant_nanovdb(hipStream_t s, const DMedium& m, const DIndexBox& ib) {
    const int ncell = m.mres[0] * m.mres[1] * m.mres[2];
    double box = 1.0;
    for (int k = 0; k < 3; ++k) box *= ((double)ib.hi[k] - ib.lo[k] + 1.0) / m.mres[k] + 3.0;   // the cell's share of the bounding box and the slop of 1 on both sides
    const int per_block = majorant_block_per_cell(box);
    hipLaunchKernelGGL(k_majorant_nanovdb, dim3((unsigned)(per_block ? ncell : ((long long)ncell + 3) / 4)), dim3(256), 0, s, m, ib, ncell, per_block, const_cast<float*>(m.majorant));
    majorant_zero_mask(s, m, ncell);
}
// the halo bricks of every block of m.nv_blocks into m.nv_bricks (n_blocks = the product of m.nvb_dim)
void launch_nvdb_bricks(hipStream_t s, const DMedium& m, size_t n_blocks) {
    const unsigned long long n_out = (unsigned long long)n_blocks * 729u;
    hipLaunchKernelGGL(k_nvdb_bricks, dim3((unsigned)std::min<unsigned long long>((n_out + 255) / 256, 1u << 20)), dim3(256), 0, s, m, n_out, const_cast<float*>(m.nv_bricks));
}

// hk_scene_update_medium_dense, before its one wait: flags of the three levels, their prefix sums and lists, and D.ctl (zeroed here)
void launch_dense_count(hipStream_t s, const DDense& D) {
    (void)hipMemsetAsync(D.ctl, 0, sizeof(DDenseCtl), s);
    const int f = D.fast, a = f == 0 ? 1 : 0, b = f == 0 ? 2 : 1;
    const unsigned n_chunk = (unsigned)(((long long)D.res[f] + 63) / 64);   // (n_chunk * blocks of the two other axes <= the field's blocks <= 2^27)
    hipLaunchKernelGGL(k_dense_flags, dim3(n_chunk * (unsigned)D.lev[0].dim[a] * (unsigned)D.lev[0].dim[b]), dim3(64), 0, s, D, n_chunk);
    for (int to = 1; to <= 2; ++to) hipLaunchKernelGGL(k_dense_group, dim3(std::min(D.lev[to].n, 1u << 16)), dim3(64), 0, s, D, to);
    const unsigned tiles = D.lev[0].tiles + D.lev[1].tiles + D.lev[2].tiles;
    hipLaunchKernelGGL(k_dense_tile_sums, dim3(tiles), dim3(256), 0, s, D);
    hipLaunchKernelGGL(k_dense_scan_sums, dim3(3), dim3(256), 0, s, D);
    hipLaunchKernelGGL(k_dense_slots, dim3(tiles), dim3(256), 0, s, D);
}
// ... and after it: the tree of n_bytes (zeroed here; count[] as read back) and the block table of the extent in D
void launch_dense_emit(hipStream_t s, const DDense& D, const uint32_t count[3], size_t n_bytes) {
    (void)hipMemsetAsync(D.tree, 0, n_bytes, s);
    if (count[0]) hipLaunchKernelGGL(k_dense_leaves, dim3(count[0]), dim3(64), 0, s, D);
    if (count[1]) hipLaunchKernelGGL(k_dense_nodes<1>, dim3(count[1]), dim3(256), 0, s, D);
    if (count[2]) hipLaunchKernelGGL(k_dense_nodes<2>, dim3(count[2]), dim3(256), 0, s, D);
    const unsigned long long n = (unsigned long long)D.nvb_dim[0] * D.nvb_dim[1] * D.nvb_dim[2];
    hipLaunchKernelGGL(k_dense_table, dim3((unsigned)std::min<unsigned long long>((n + 255) / 256, 1u << 20)), dim3(256), 0, s, D, n);
}

}  // namespace hk
