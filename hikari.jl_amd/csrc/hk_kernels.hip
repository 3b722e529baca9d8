// hk_kernels.hip — the device code of the library for gfx950 (wave64): ONE translation unit (DESIGN.md §4 describes the pass).
// The headers are slices of it, not modules: each uses what stands above it, and the order of the kernels in the code object is the
// order of this file.  Keep the order; a new kernel goes with its stage.  Tracking, the shadow walk and the scene edits are sections
// of this file, between the includes:
//     hk_wave_queues.h     lane_id, WaveQ, segment tickets and loops, streaming loads / stores, record loaders, HK_DBG*
//     hk_camera_stage.h    k_sobol_table, k_segment_lists, k_sobol_lo_table, k_camera                                      [K1]
//     hk_traverse.h        LDS cache fills, k_trace, the per-lane ray state machine, k_trace_lean                          [K3]
//     section K4           k_track, k_track_flat, k_track_pool, k_scatter, k_detect_camera_medium                         [K4-K6]
//     hk_shade.h           k_escaped, k_light_select, k_light_select_pool, k_shade                               [K7, K2,K8,K9,K11]
//     hk_shadow.h          shadow_contribute*, k_shadow, trace_shadow_body                                                 [K10]
//     hk_small_pass.h      k_small_pass: all stages of a small pass in one launch
//     section walk         k_shadow_walk, k_walk_pool, k_walk_cast, k_walk_track                                           [K10]
//     hk_film_kernels.h, hk_display.h    the film fold and k_film; the display chain                                   [K12, K13]
//     section SCENE EDITS  transform, refit, set, tree cost, device BVH build
//     hk_table_kernels.h, hk_nvdb_build.h    k_envmap_*, k_majorant_*, k_nvdb_bricks; a NanoVDB tree from a dense field
//     hk_launch_impl.h, hk_test_kernels.h    the launch layer (hk_launch.h), which names every kernel; the parity tests' entry points
#include <hip/hip_runtime.h>
#include <type_traits>
#include <cstdlib>
#include <cstdio>

#include "hikari_mi355x.h"
#include "hk_device.h"
#include "hk_edit_host.h"
#include "hk_bvh_decide.h"

using namespace hkd;

namespace {
#include "hk_wave_queues.h"
}  // namespace
#include "hk_camera_stage.h"
#include "hk_traverse.h"

// ---------------------------------------------------------------------------------------------------
// K4: delta tracking with null collisions (delta-tracking.jl:79-453), after k_trace, for the paths that travel inside a
// medium.  The collision count per path is wildly uneven (0 .. 1000s), so the wave does not walk its queue 64 entries at
// a time: every lane is a little state machine that takes ONE step per iteration (next majorant segment, or one tentative
// collision) and, when its path is finished, waits for the next refill, where finished paths are routed with
// ballot/popcount pushes (scatter queue -> k_scatter, escaped queue, material-kind queues with Mix resolved) and idle lanes
// pull the next entries of the wave's own queue segment.  Still no atomics: queue, cursor and counts are wave-private.
// Arithmetic and RNG consumption per path are exactly those of the sequential loop.
// ---------------------------------------------------------------------------------------------------
#ifndef HK_REFILL_MIN_IDLE
#define HK_REFILL_MIN_IDLE 8
#endif
// the tracking loops wait on dependent loads (NanoVDB tree, majorant cells) ~60 % of the time at 2 waves/SIMD: trade a few
// spilled registers for a third wave
#ifndef HK_MEDIA_WAVES
#define HK_MEDIA_WAVES 2
#endif
#ifndef HK_TRACK_ADVANCE
#define HK_TRACK_ADVANCE 4
#endif
#ifndef HK_DELTA_ADVANCE
#define HK_DELTA_ADVANCE 6   // k_track's own advance-loop length (the shadow walk keeps HK_TRACK_ADVANCE)
#endif
#ifndef HK_SKIP_ZERO
#define HK_SKIP_ZERO 0
#endif
#ifndef HK_GREY_TRACK_WAVES
#define HK_GREY_TRACK_WAVES 4
#endif
enum { TR_BUSY = -101, TR_EMPTY = -100, TR_SCATTER = -3, TR_ESCAPED = -2 };  // >= 0: reached its surface hit of that material kind

// A path that survived tracking to t_max on the ray (o, d) is handed the hit k_trace stored for it: TR_ESCAPED where there is none, else
// the final material kind, a MixMaterial resolved here (mat_id rewritten, its emissive bit kept).  For k_track and k_track_flat;
// k_track_pool, which has to reload the ray, keeps its own copy in `route`.
HKD int classify_survivor(const DPathState& st, const DScene& sc, uint32_t slot, v3 o, v3 d) {
    float4 H = st.hit[slot];
    const int prim = __float_as_int(H.y);
    if (prim < 0) return TR_ESCAPED;
    const int mat_word = st.mat_id[slot];
    int mat = mat_word & ~HK_MAT_EMISSIVE_BIT;
    if (sc.materials[mat].kind == HK_MAT_MIX) {
        float w = 1.0f - H.z - H.w;
        mat = resolve_mix_material(sc, mat, o + d * H.x, -d, uv_at(sc, prim, w, H.z, H.w));
        st.mat_id[slot] = mat | (mat_word & HK_MAT_EMISSIVE_BIT);
    }
    int kind = sc.materials[mat].kind;
    return kind == HK_MAT_MIX ? HK_MAT_FALLBACK : kind;
}

// One open output segment of k_track: the wave owns its count words while it is open.
struct TrackSeg {
    int gw;                       // segment index, -1 = slot free
    int esc, sca;                 // entries in the segment's escaped / scatter queues
    int kind_count[HK_MAX_KINDS]; // entries in its per-kind queues
};
// GREY (scenes whose media are all Grid / NanoVDB with flat sigma_a and sigma_s spectra — DScene::all_grey; the BOMEX example's cloud is
// RGBSpectrum(0) / RGBSpectrum(1)): every ratio the tracker multiplies into beta and r_u is then a spectrum of four EQUAL components
// divided by its own first component, i.e. 1 up to rounding — the general code multiplies by (1 +- 3 ulp) per collision, this
// instantiation leaves beta and r_u alone (they stay in memory, not in registers), carries r_l's rescaling as one float, needs no
// wavelengths and no exp at a cell boundary.  Every DECISION (free-flight distance, absorb / scatter / null, termination) is taken on
// the same first-component arithmetic as in the general code, so the collision sequence of a path is identical.
template <int MM, bool GREY = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(GREY ? HK_GREY_TRACK_WAVES : HK_MEDIA_WAVES))) k_track(DPathState st, DScene sc, DTables T, DFrame fr, int depth, DStats* stats, const DMedium* __restrict__ media) {
    // `media` == sc.media: a restrict-qualified kernel argument, so the record of a wave-uniform medium index is read with scalar loads
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_coll = 0, n_dda = 0;
    const DPathGen g = gen_at(st, depth);   // throughput / scattering vertex are updated IN PLACE in the current generation
    const bool ones = depth == 0 && fr.implicit_ones;
    // The wave streams segment after segment (SegStream) WITHOUT draining its lanes in between: the collision count per path is so
    // uneven that a third of the lane-slots of a segment-at-a-time walk sat empty in the segment's tail.  A finished path must be
    // pushed into the queues of ITS segment, so two segments are open at any time — `cur` (tag cur_tag) feeds the refill, the other
    // slot holds the previous segment until its last lane has finished — and every lane carries the tag of its segment.
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_TRACK), true, depth, Q_MEDIUM);
    TrackSeg seg[2];
    seg[0].gw = seg[1].gw = -1;
    int cur_tag = 0;
    const uint32_t* __restrict__ queue = st.medium_q;
    int n = 0, cursor = 0;
    bool more = true;
    auto open_seg = [&](TrackSeg& s, int gw) {
        s.gw = gw;
        s.esc = *count_ptr(st, depth, Q_ESCAPED, gw);
        s.sca = 0;
#pragma unroll
        for (int k = 0; k < HK_MAX_KINDS; ++k) s.kind_count[k] = *count_ptr(st, depth, Q_MAT0 + k, gw);
    };
    auto close_seg = [&](TrackSeg& s) {
        if (s.gw >= 0 && lane == 0) {
            *count_ptr(st, depth, Q_SCATTER, s.gw) = s.sca;
            *count_ptr(st, depth, Q_ESCAPED, s.gw) = s.esc;
#pragma unroll
            for (int k = 0; k < HK_MAX_KINDS; ++k) *count_ptr(st, depth, Q_MAT0 + k, s.gw) = s.kind_count[k];
        }
        s.gw = -1;
    };
    {
        int state = TR_EMPTY, tag = 0;
        uint32_t slot = 0, pslot = 0;   // generation index of the lane's path; its path slot (pixel-sample id: where L lives)
        v3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1), cur_o = mk3(0, 0, 0);
        S4 lambda = s4(0.0f), beta = s4(0.0f), r_u = s4(0.0f), r_l = s4(0.0f), base_a = s4(0.0f), base_s = s4(0.0f), base_Le = s4(0.0f), sm = s4(0.0f);
        float a0 = 0.0f, s0 = 0.0f, rl_f = 1.0f;   // GREY: the flat sigma_a / sigma_s values, the factor r_l has picked up so far
        bool dead_null = false;                    // GREY: beta or r_u is black (the general code notices at the first null collision / at the end)
        uint64_t rng = 0;
        MajorantIter it = exhausted_iter();
        float seg1 = 0.0f, sm0 = 0.0f, t = 0.0f;
        bool in_seg = false, pending = false;
        float pend_dt = 0.0f;
        int k_in_seg = 0, segi = 0, medium_idx = 0;
        for (;;) {
            const unsigned long long busy_m = __ballot(state == TR_BUSY);
            if (busy_m == 0ull || (64 - __popcll(busy_m) >= fr.refill_idle && (cursor < n || more))) {
                // ---- route the finished paths into the queues of their own segment ----
#pragma unroll
                for (int tg = 0; tg < 2; ++tg) {
                    TrackSeg& S = seg[tg];
                    const bool sel = tag == tg && state != TR_BUSY && state != TR_EMPTY;
                    if (__ballot(sel) == 0ull) continue;
                    const size_t base = (size_t)S.gw * st.wave_cap;
                    {
                        const unsigned long long m = __ballot(sel && state == TR_SCATTER);
                        if (sel && state == TR_SCATTER) st.scatter_q[base + S.sca + __popcll(m & lt_mask)] = slot;
                        S.sca += __popcll(m);
                    }
                    {
                        const unsigned long long m = __ballot(sel && state == TR_ESCAPED);
                        if (sel && state == TR_ESCAPED) st.escaped_q[base + S.esc + __popcll(m & lt_mask)] = slot;
                        S.esc += __popcll(m);
                    }
                    unsigned long long todo_k = __ballot(sel && state >= 0);
                    while (todo_k) {
                        int src = __ffsll((long long)todo_k) - 1;
                        const int k = __builtin_amdgcn_readlane(state, src);   // wave-uniform: counts stay in scalar registers
                        bool mine = sel && state == k;
                        unsigned long long m = __ballot(mine);
                        int cnt = 0;
#pragma unroll
                        for (int kk = 0; kk < HK_MAX_KINDS; ++kk) cnt = (kk == k) ? S.kind_count[kk] : cnt;
                        if (mine) st.mat_q[((size_t)k * st.n_waves + S.gw) * st.wave_cap + cnt + __popcll(m & lt_mask)] = matq_entry(st, slot);
                        int add = __popcll(m);
#pragma unroll
                        for (int kk = 0; kk < HK_MAX_KINDS; ++kk) S.kind_count[kk] += (kk == k) ? add : 0;
                        todo_k &= ~m;
                    }
                }
                if (state != TR_BUSY) state = TR_EMPTY;
                // ---- the current segment is used up: open the next one in the other slot as soon as that slot's last lane is done ----
                while (more && cursor >= n) {
                    const int other = cur_tag ^ 1;
                    const bool other_busy = __ballot(state == TR_BUSY && tag == other) != 0ull;
                    if (other_busy) break;   // both slots hold lanes in flight: no third segment, the refill waits
                    if (other == 0) close_seg(seg[0]); else close_seg(seg[1]);
                    const int gw = stream_next(stream, st.n_waves);
                    if (gw >= st.n_waves) {
                        more = false;
                        break;
                    }
                    if (other == 0) open_seg(seg[0], gw); else open_seg(seg[1], gw);
                    cur_tag = other;
                    queue = st.medium_q + (size_t)gw * st.wave_cap;
                    n = *count_ptr(st, depth, Q_MEDIUM, gw);
                    cursor = 0;
                }
                // ---- refill idle lanes from the current segment's queue ----
                const unsigned long long want = __ballot(state == TR_EMPTY);
                const int avail = n - cursor;
                const int rank = __popcll(want & lt_mask);
                if (state == TR_EMPTY && rank < avail) {
                    slot = queue[cursor + rank];
                    tag = cur_tag;
                    float4 O = g.ray_o[slot], D = g.ray_d[slot];
                    ro = mk3(O.x, O.y, O.z);
                    rd = mk3(D.x, D.y, D.z);
                    const float t_max = st.hit[slot].x;
                    const uint2 meta = g.meta[slot];
                    medium_idx = (int)(meta.x >> 16) - 1;
                    pslot = meta.y;
                    const DMedium& med = sc.n_media == 1 ? media[0] : media[medium_idx];
                    if constexpr (GREY) {
                        a0 = eval_flat(med.sigma_a);
                        s0 = eval_flat(med.sigma_s);
                        base_a = s4(a0);
                        base_s = s4(s0);
                        rl_f = 1.0f;
                        dead_null = is_black(ld_throughput(g.beta, slot, ones)) || is_black(ld_throughput(g.r_u, slot, ones));
                    } else {
                        lambda = ld_lambda(st, g, slot, pslot);
                        beta = ld_throughput(g.beta, slot, ones);
                        r_u = ld_throughput(g.r_u, slot, ones);
                        r_l = ld_throughput(g.r_l, slot, ones);
                        base_a = eval_scaled(med.sigma_a, lambda);
                        base_s = eval_scaled(med.sigma_s, lambda);
                        if (HK_HAS_MEDIUM(MM, HK_MEDIUM_HOMOGENEOUS)) base_Le = eval_scaled(med.Le, lambda);
                    }
                    rng = lcg_init(ro, rd, t_max);
                    it = create_majorant_iterator<MM>(med, ro, rd, t_max);
                    in_seg = false;
                    pending = false;
                    segi = 0;
                    state = TR_BUSY;
                }
                const int want_n = __popcll(want);
                cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
                if (__ballot(state == TR_BUSY) == 0ull) {
                    if (cursor >= n && !more) break;
                    continue;
                }
            }
            // The medium record is read through a wave-uniform index (scalar loads into SGPRs): lanes are served medium by medium
            // ("waterfall"), which is a single trip for the usual one-medium scene.
            bool survived = false;
            unsigned long long todo = __ballot(state == TR_BUSY);
            while (todo) {
                const int m_uniform = __builtin_amdgcn_readlane(medium_idx, __ffsll((long long)todo) - 1);
                const bool mine = state == TR_BUSY && medium_idx == m_uniform;
                const DMedium& med = media[m_uniform];
                // ---- phase A: cheap steps (next majorant cell, free-flight sample, cell-boundary crossing) until every busy lane
                //      either holds a tentative collision or has run out of segments ----
    #pragma unroll 1
                for (int adv = 0; adv < fr.delta_advance; ++adv) {
                    const bool need = mine && state == TR_BUSY && !pending && !survived;
                    if (__ballot(need) == 0ull) break;
                    if (!need) continue;
                    if (!in_seg) {
                        float seg0;
                        if (segi >= 256 || !majorant_next<MM>(it, med, base_a + base_s, seg0, seg1, sm))
                            survived = true;  // ran out of segments with the path still alive
                        else {
                            ++segi;
                            ++n_dda;
                            sm0 = sm.x;
                            if (sm0 >= 1e-10f) {
                                t = seg0;
                                cur_o = ro + rd * t;
                                in_seg = true;
                                k_in_seg = 0;
                            }
                        }
                    }
                    // a lane that has just entered a cell draws its first free flight in the same round (same operations per path
                    // in the same order; one round less per cell entered)
                    if (!in_seg || survived) {
                    } else if (k_in_seg >= 1024) {
                        in_seg = false;
                    } else {
                        ++k_in_seg;
                        float u = lcg_next(rng);
                        pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                        float ts = t + pend_dt;
                        if (ts >= seg1) {
                            if constexpr (!GREY) {   // GREY: T_maj / T_maj[1] = 1, nothing changes
                                float dr = seg1 - t;
                                S4 Tm = s4exp((-dr) * sm);
                                float T0 = Tm.x;
                                if (T0 > 1e-10f) {
                                    beta = div4(beta * Tm, T0);
                                    r_u = div4(r_u * Tm, T0);
                                    r_l = div4(r_l * Tm, T0);
                                }
                            }
                            in_seg = false;
                        } else
                            pending = true;
                    }
                }
                // ---- phase B: the tentative collisions (medium lookup, absorb / scatter / null) ----
                if (GREY && mine && state == TR_BUSY && pending) {
                    pending = false;
                    const float dt = pend_dt;
                    const float Tm0 = media_expf((-dt) * sm0);
                    const v3 p = cur_o + rd * dt;
                    ++n_coll;
                    const float d = sample_density<MM>(med, p);
                    const float sa = a0 * d, ss = s0 * d;
                    const float p_absorb = sa / sm0, p_scatter = ss / sm0;
                    const float ue = lcg_next(rng);
                    if (ue < p_absorb) {
                        state = TR_EMPTY;  // absorbed
                    } else if (ue < p_absorb + p_scatter) {
                        if (depth >= fr.max_depth)
                            state = TR_EMPTY;
                        else {   // beta and r_u are rescaled by sigma_s T_maj / (sigma_s T_maj)[1] = 1: they stay as they are in the record
                            g.ray_o[slot] = make_float4(p.x, p.y, p.z, INF_F);  // the scattering vertex: k_scatter continues from here
                            state = TR_SCATTER;
                        }
                    } else {
                        const float sn0 = maxf(sm0 - sa - ss, 0.0f);
                        const float pdf = Tm0 * sn0;
                        if (pdf > 1e-10f) {
                            rl_f = ((rl_f * Tm0) * sm0) * (1.0f / pdf);
                            t = t + dt;
                            cur_o = p;
                            if (dead_null) state = TR_EMPTY;
                        } else
                            state = TR_EMPTY;
                    }
                }
                if (!GREY && mine && state == TR_BUSY && pending) {
                    pending = false;
                    const float dt = pend_dt;
                    const float ts = t + dt;
                    S4 Tm = s4exp((-dt) * sm);
                    v3 p = cur_o + rd * dt;
                    ++n_coll;
                    MediumProps mp = sample_point<MM>(T, lambda, med, base_a, base_s, base_Le, p);
                    if ((HK_HAS_MEDIUM(MM, HK_MEDIUM_HOMOGENEOUS) || HK_HAS_MEDIUM(MM, HK_MEDIUM_RGB_GRID)) && !is_black(mp.Le) && depth < fr.max_depth) {
                        float pr = sm0 * Tm.x;
                        if (pr > 1e-10f) {
                            S4 r_e = r_u * sm * Tm / pr;
                            if (!is_black(r_e)) st4(&st.L[pslot], ld4(&st.L[pslot]) + beta * mp.sigma_a * Tm * mp.Le / (pr * average(r_e)));
                        }
                    }
                    float p_absorb = mp.sigma_a.x / sm0, p_scatter = mp.sigma_s.x / sm0;
                    float ue = lcg_next(rng);
                    if (ue < p_absorb) {
                        state = TR_EMPTY;  // absorbed
                    } else if (ue < p_absorb + p_scatter) {
                        if (depth >= fr.max_depth)
                            state = TR_EMPTY;
                        else {
                            float pdf = Tm.x * mp.sigma_s.x;
                            if (pdf > 1e-10f) {
                                beta = div4(beta * Tm * mp.sigma_s, pdf);
                                r_u = div4(r_u * Tm * mp.sigma_s, pdf);
                            }
                            st4(&g.beta[slot], beta);
                            st4(&g.r_u[slot], r_u);
                            g.ray_o[slot] = make_float4(p.x, p.y, p.z, INF_F);  // the scattering vertex: k_scatter continues from here
                            state = TR_SCATTER;
                        }
                    } else {
                        S4 sn = s4max0(sm - mp.sigma_a - mp.sigma_s);
                        float pdf = Tm.x * sn.x;
                        if (pdf > 1e-10f) {
                            beta = div4(beta * Tm * sn, pdf);
                            r_u = div4(r_u * Tm * sn, pdf);
                            r_l = div4(r_l * Tm * sm, pdf);
                            t = ts;
                            cur_o = p;
                            if (is_black(beta) || is_black(r_u)) state = TR_EMPTY;
                        } else
                            state = TR_EMPTY;
                    }
                }
                todo &= ~__ballot(mine);
            }
            if (survived) {
                state = TR_EMPTY;
                if (!((GREY ? dead_null : (is_black(beta) || is_black(r_u))) || depth >= fr.max_depth)) {
                    // survived to t_max: hand the stored surface hit / the escape over with the updated throughput
                    if constexpr (GREY) {
                        st4(&g.r_l[slot], ld_throughput(g.r_l, slot, ones) * rl_f);
                    } else {
                        st4(&g.beta[slot], beta);
                        st4(&g.r_u[slot], r_u);
                        st4(&g.r_l[slot], r_l);
                    }
                    state = classify_survivor(st, sc, slot, ro, rd);
                }
            }
        }
    }
    close_seg(seg[0]);
    close_seg(seg[1]);
    stats += global_wave();
    wave_add(&stats->collisions, n_coll);
    wave_add(&stats->nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);   // (priced per scene: SURVEY 8d charges the NanoVDB tree walk)
    wave_add(&stats->dda_steps, n_dda);
}

// ---------------------------------------------------------------------------------------------------
// k_track_flat: K4 of a scene whose ONE medium is GREY (k_track<MM, true> above) — the same per-lane state machine, the same
// arithmetic and RNG consumption per path (films bit-identical: tests + tools/ab_bitwise.py, HK_GREY_FLAT=0 runs the older kernel),
// re-shaped for INSTRUCTION ISSUE.  On this chip a scalar instruction costs a SIMD about what a vector one does (tools/valu_rate.hip:
// v_fma + s_add pair 6.4 cycles at 4 waves against 2.9 + 4.2 alone), and k_track issued as many scalar exec-mask instructions as
// vector ones: every loop-carried `bool` (in_seg, pending, survived, dead_null, the iterator's liveness ...) lived in an SGPR pair
// and every divergent assignment to it cost an andn2 / and / or triple PER NESTING LEVEL it crossed.  Here
//   * the lane's flags are bits of ONE VGPR: a write under a divergent exec mask merges for free, a test is v_and + v_cmp;
//   * the majorant iterator's mode / axis signs are three more bits of that word, its DDA step is straight-line code;
//   * there is one medium (all_grey): no waterfall loop, its record's fields are read once into scalar registers before the loop;
//   * BRICKS: the medium is a NanoVDB grid with dense halo bricks (DScene::grey_bricks) — the tree-walk paths of the lookup are
//     not in the kernel;
//   * the collision round can WAIT (fr.track_gate): when fewer than N lanes hold a tentative collision and others can still advance,
//     the cheap-step loop goes on for a few more iterations (the rule of k_shadow's waiting leaf phases).
// ---------------------------------------------------------------------------------------------------
#ifndef HK_FLAT_TRACK_WAVES
#define HK_FLAT_TRACK_WAVES 4
#endif
enum { TF_IN_SEG = 1, TF_PENDING = 2, TF_SURVIVED = 4, TF_DEAD_NULL = 8, TF_TAG = 16, TF_IT_LIVE = 32, TF_NEG0 = 0x100, TF_NEG1 = 0x200, TF_NEG2 = 0x400 };
template <int MM, bool BRICKS>
__global__ void __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(HK_FLAT_TRACK_WAVES))) k_track_flat(DPathState st, DScene sc, DFrame fr, int depth, DStats* stats, const DMedium* __restrict__ media) {
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_coll = 0, n_dda = 0;
    HK_DBG_DECL
    const DPathGen g = gen_at(st, depth);
    const bool ones = depth == 0 && fr.implicit_ones;
    const DMedium& med = media[0];
    const float a0 = eval_flat(med.sigma_a), s0 = eval_flat(med.sigma_s);
    const float sig_t = a0 + s0;   // (base_a + base_s).x of the general code
    const int mrx = med.mres[0], mry = med.mres[1], mrz = med.mres[2];
    const float* __restrict__ maj = med.majorant;
    const bool last_depth = depth >= fr.max_depth;
    const int gate_min = fr.track_gate & 0xff, gate_cap = fr.delta_advance + ((fr.track_gate >> 8) & 0xff);
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_TRACK), true, depth, Q_MEDIUM);
    TrackSeg seg[2];
    seg[0].gw = seg[1].gw = -1;
    int cur_tag = 0;
    const uint32_t* __restrict__ queue = st.medium_q;
    int n = 0, cursor = 0;
    bool more = true;
    auto open_seg = [&](TrackSeg& s, int gw) {
        s.gw = gw;
        s.esc = *count_ptr(st, depth, Q_ESCAPED, gw);
        s.sca = 0;
#pragma unroll
        for (int k = 0; k < HK_MAX_KINDS; ++k) s.kind_count[k] = *count_ptr(st, depth, Q_MAT0 + k, gw);
    };
    auto close_seg = [&](TrackSeg& s) {
        if (s.gw >= 0 && lane == 0) {
            *count_ptr(st, depth, Q_SCATTER, s.gw) = s.sca;
            *count_ptr(st, depth, Q_ESCAPED, s.gw) = s.esc;
#pragma unroll
            for (int k = 0; k < HK_MAX_KINDS; ++k) *count_ptr(st, depth, Q_MAT0 + k, s.gw) = s.kind_count[k];
        }
        s.gw = -1;
    };
    int state = TR_EMPTY, fl = 0;
    uint32_t slot = 0;
    v3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1), cur_o = mk3(0, 0, 0);
    float rl_f = 1.0f;
    uint64_t rng = 0;
    float it_tmin = 0.0f, it_tmax = 0.0f, nt0 = 0.0f, nt1 = 0.0f, nt2 = 0.0f, dl0 = 0.0f, dl1 = 0.0f, dl2 = 0.0f;
    int vx = 0, vy = 0, vz = 0;
    float seg1 = 0.0f, sm0 = 0.0f, t = 0.0f, pend_dt = 0.0f;
    int k_in_seg = 0, segi = 0;
    for (;;) {
        const unsigned long long busy_m = __ballot(state == TR_BUSY);
        if (busy_m == 0ull || (64 - __popcll(busy_m) >= fr.refill_idle && (cursor < n || more))) {
            // ---- route the finished paths into the queues of their own segment ----
            const int tag = (fl & TF_TAG) ? 1 : 0;
#pragma unroll
            for (int tg = 0; tg < 2; ++tg) {
                TrackSeg& S = seg[tg];
                const bool sel = tag == tg && state != TR_BUSY && state != TR_EMPTY;
                if (__ballot(sel) == 0ull) continue;
                const size_t base = (size_t)S.gw * st.wave_cap;
                {
                    const unsigned long long m = __ballot(sel && state == TR_SCATTER);
                    if (sel && state == TR_SCATTER) st.scatter_q[base + S.sca + __popcll(m & lt_mask)] = slot;
                    S.sca += __popcll(m);
                }
                {
                    const unsigned long long m = __ballot(sel && state == TR_ESCAPED);
                    if (sel && state == TR_ESCAPED) st.escaped_q[base + S.esc + __popcll(m & lt_mask)] = slot;
                    S.esc += __popcll(m);
                }
                unsigned long long todo_k = __ballot(sel && state >= 0);
                while (todo_k) {
                    int src = __ffsll((long long)todo_k) - 1;
                    const int k = __builtin_amdgcn_readlane(state, src);   // wave-uniform: counts stay in scalar registers
                    bool mine = sel && state == k;
                    unsigned long long m = __ballot(mine);
                    int cnt = 0;
#pragma unroll
                    for (int kk = 0; kk < HK_MAX_KINDS; ++kk) cnt = (kk == k) ? S.kind_count[kk] : cnt;
                    if (mine) st.mat_q[((size_t)k * st.n_waves + S.gw) * st.wave_cap + cnt + __popcll(m & lt_mask)] = matq_entry(st, slot);
                    int add = __popcll(m);
#pragma unroll
                    for (int kk = 0; kk < HK_MAX_KINDS; ++kk) S.kind_count[kk] += (kk == k) ? add : 0;
                    todo_k &= ~m;
                }
            }
            if (state != TR_BUSY) state = TR_EMPTY;
            // ---- the current segment is used up: open the next one in the other slot as soon as that slot's last lane is done ----
            while (more && cursor >= n) {
                const int other = cur_tag ^ 1;
                const bool other_busy = __ballot(state == TR_BUSY && ((fl & TF_TAG) ? 1 : 0) == other) != 0ull;
                if (other_busy) break;   // both slots hold lanes in flight: no third segment, the refill waits
                if (other == 0) close_seg(seg[0]); else close_seg(seg[1]);
                const int gw = stream_next(stream, st.n_waves);
                if (gw >= st.n_waves) {
                    more = false;
                    break;
                }
                if (other == 0) open_seg(seg[0], gw); else open_seg(seg[1], gw);
                cur_tag = other;
                queue = st.medium_q + (size_t)gw * st.wave_cap;
                n = *count_ptr(st, depth, Q_MEDIUM, gw);
                cursor = 0;
            }
            // ---- refill idle lanes from the current segment's queue ----
            const unsigned long long want = __ballot(state == TR_EMPTY);
            const int avail = n - cursor;
            const int rank = __popcll(want & lt_mask);
            HK_DBG(5, state == TR_EMPTY && rank < avail);
            if (state == TR_EMPTY && rank < avail) {
                slot = queue[cursor + rank];
                float4 O = g.ray_o[slot], D = g.ray_d[slot];
                ro = mk3(O.x, O.y, O.z);
                rd = mk3(D.x, D.y, D.z);
                const float t_max = st.hit[slot].x;
                const bool dead = is_black(ld_throughput(g.beta, slot, ones)) || is_black(ld_throughput(g.r_u, slot, ones));
                rl_f = 1.0f;
                rng = lcg_init(ro, rd, t_max);
                const MajorantIter it = create_majorant_iterator<MM>(med, ro, rd, t_max);
                it_tmin = it.t_min;
                it_tmax = it.t_max;
                nt0 = it.next_t[0], nt1 = it.next_t[1], nt2 = it.next_t[2];
                dl0 = it.delta_t[0], dl1 = it.delta_t[1], dl2 = it.delta_t[2];
                vx = it.voxel[0], vy = it.voxel[1], vz = it.voxel[2];
                fl = (cur_tag ? TF_TAG : 0) | (dead ? TF_DEAD_NULL : 0) | ((it.mode & 0xff) == 2 ? TF_IT_LIVE : 0) | (it.mode & 0x700);
                segi = 0;
                state = TR_BUSY;
            }
            const int want_n = __popcll(want);
            cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
            if (__ballot(state == TR_BUSY) == 0ull) {
                if (cursor >= n && !more) break;
                continue;
            }
        }
        // ---- phase A: cheap steps (next majorant cell, free-flight sample) until the busy lanes hold a tentative collision or have
        //      run out of cells.  fr.delta_advance iterations; then, while fewer than gate_min lanes hold a collision, up to gate_cap ----
#pragma unroll 1
        for (int adv = 0;; ++adv) {
            const bool need = state == TR_BUSY && (fl & (TF_PENDING | TF_SURVIVED)) == 0;
            if (__ballot(need) == 0ull) break;
            if (adv >= fr.delta_advance) {
                if (adv >= gate_cap) break;
                if (__popcll(__ballot(state == TR_BUSY && (fl & TF_PENDING) != 0)) >= gate_min) break;
            }
            HK_DBG(0, need);
            if (need) {
                if ((fl & TF_IN_SEG) == 0) {
                    HK_DBG(1, true);
                    // majorant_next (media.jl:625-729) of a DDA iterator, straight-line
                    if ((fl & TF_IT_LIVE) == 0 || segi >= 256 || it_tmin >= it_tmax)
                        fl |= TF_SURVIVED;   // ran out of segments with the path still alive
                    else {
                        const bool lxy = nt0 < nt1, lxz = nt0 < nt2, lyz = nt1 < nt2;
                        const bool ax0 = lxy & lxz, ax1 = (!lxy) & lyz;   // axis 0, axis 1, else axis 2
                        const float nt = ax0 ? nt0 : (ax1 ? nt1 : nt2);
                        const float stm = minf(nt, it_tmax);
                        const float rho = maj[vx + mrx * (vy + mry * vz)];
                        const float seg0 = it_tmin;
                        seg1 = stm;
                        const bool neg = (fl & (ax0 ? TF_NEG0 : (ax1 ? TF_NEG1 : TF_NEG2))) != 0;
                        const int v = (ax0 ? vx : (ax1 ? vy : vz)) + (neg ? -1 : 1);
                        const int lim = neg ? -1 : (ax0 ? mrx : (ax1 ? mry : mrz));
                        const float s = nt + (ax0 ? dl0 : (ax1 ? dl1 : dl2));
                        vx = ax0 ? v : vx;
                        vy = ax1 ? v : vy;
                        vz = (ax0 | ax1) ? vz : v;
                        nt0 = ax0 ? s : nt0;
                        nt1 = ax1 ? s : nt1;
                        nt2 = (ax0 | ax1) ? nt2 : s;
                        const bool out = v == lim;
                        fl = out ? (fl & ~TF_IT_LIVE) : fl;
                        it_tmin = out ? it_tmax : stm;
                        ++segi;
                        ++n_dda;
                        sm0 = sig_t * rho;
                        if (sm0 >= 1e-10f) {
                            t = seg0;
                            cur_o = ro + rd * t;
                            fl |= TF_IN_SEG;
                            k_in_seg = 0;
                        }
                    }
                }
                // a lane that has just entered a cell draws its first free flight in the same round
                if ((fl & (TF_IN_SEG | TF_SURVIVED)) == TF_IN_SEG) {
                    HK_DBG(2, true);
                    if (k_in_seg >= 1024)
                        fl &= ~TF_IN_SEG;
                    else {
                        ++k_in_seg;
                        const float u = lcg_next(rng);
                        pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                        const float ts = t + pend_dt;
                        fl = ts >= seg1 ? (fl & ~TF_IN_SEG) : (fl | TF_PENDING);   // leaves the cell (T_maj / T_maj[1] = 1: nothing else changes) / tentative collision
                    }
                }
            }
        }
        // ---- phase B: the tentative collisions (medium lookup, absorb / scatter / null) ----
        HK_DBG(3, state == TR_BUSY && (fl & TF_PENDING) != 0);
        HK_DBG(4, state == TR_BUSY);
        if (state == TR_BUSY && (fl & TF_PENDING) != 0) {
            fl &= ~TF_PENDING;
            const float dt = pend_dt;
            const float Tm0 = media_expf((-dt) * sm0);
            const v3 p = cur_o + rd * dt;
            ++n_coll;
            const float d = sample_density<MM, BRICKS>(med, p);
            const float sa = a0 * d, ss = s0 * d;
            const float p_absorb = sa / sm0, p_scatter = ss / sm0;
            const float ue = lcg_next(rng);
            if (ue < p_absorb) {
                state = TR_EMPTY;  // absorbed
            } else if (ue < p_absorb + p_scatter) {
                if (last_depth)
                    state = TR_EMPTY;
                else {   // beta and r_u are rescaled by sigma_s T_maj / (sigma_s T_maj)[1] = 1: they stay as they are in the record
                    g.ray_o[slot] = make_float4(p.x, p.y, p.z, INF_F);  // the scattering vertex: k_scatter continues from here
                    state = TR_SCATTER;
                }
            } else {
                const float sn0 = maxf(sm0 - sa - ss, 0.0f);
                const float pdf = Tm0 * sn0;
                if (pdf > 1e-10f) {
                    rl_f = ((rl_f * Tm0) * sm0) * (1.0f / pdf);
                    t = t + dt;
                    cur_o = p;
                    if (fl & TF_DEAD_NULL) state = TR_EMPTY;
                } else
                    state = TR_EMPTY;
            }
        }
        if (state == TR_BUSY && (fl & TF_SURVIVED) != 0) {
            state = TR_EMPTY;
            if (!((fl & TF_DEAD_NULL) != 0 || last_depth)) {
                // survived to t_max: hand the stored surface hit / the escape over with the updated throughput
                st4(&g.r_l[slot], ld_throughput(g.r_l, slot, ones) * rl_f);
                state = classify_survivor(st, sc, slot, ro, rd);
            }
        }
    }
    close_seg(seg[0]);
    close_seg(seg[1]);
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->collisions, n_coll);
    wave_add(&stats->nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);   // (priced per scene: SURVEY 8d charges the NanoVDB tree walk)
    wave_add(&stats->dda_steps, n_dda);
}

// ---------------------------------------------------------------------------------------------------
// k_track_pool: k_track_flat with DENSE set-up and DENSE routing through a per-wave pool in LDS.  A camera / bounce ray lives 2.7
// collisions and 7.7 majorant cells, so half of k_track's instructions were the per-ray set-up (queue entry, ray record, LCG seed,
// majorant iterator: 18 IEEE divisions) and the routing of the finished paths — both executed for the ~25 idle lanes that triggered a
// refill, with every instruction paid for 64.  Here
//   * SET-UP runs for 64 queue entries at once, whenever the pool is empty and a lane is free, and writes 64 ready-to-track states
//     (19 words each) to the wave's pool;
//   * a lane whose path ends takes the next state from the pool IN THE SAME ROUND (19 LDS reads) — no lane waits for a refill round;
//   * a finished path leaves (slot, destination key, r_l factor) in a 128-entry ring in LDS; the ring is ROUTED 64 entries at a time:
//     the r_l update, the hit / material classification of the survivors (Mix resolve included) and the ballot compaction into the
//     segment's queues all run on full waves;
//   * the two open segments' count words live in LDS, not in 28 scalar registers.
// Same arithmetic and RNG consumption per path as k_track<MM, true> (films bit-identical: tools/ab_bitwise.py; HK_TRACK_POOL=0 runs
// k_track_flat).  Only the ORDER of a segment's queue entries differs, which no result depends on (test_scheduling_is_result_neutral).
// ---------------------------------------------------------------------------------------------------
enum { TP_SLOT = 0, TP_RO = 1, TP_RD = 4, TP_RNG = 7, TP_TMIN = 9, TP_TMAX = 10, TP_NT = 11, TP_DL = 14, TP_VOX = 17, TP_FL = 18, TP_FIELDS = 19, TP_RING = 128,
       TP_TAGS = 4, TP_TAG_SHIFT = 12, TP_WAVE_INTS = TP_FIELDS * 64 + 3 * TP_RING + 16 * TP_TAGS, TP_SURVIVED = 14 };
HKD void wave_lds_fence() {   // orders this wave's LDS writes before its later LDS reads by OTHER lanes (the hardware executes a wave's LDS instructions in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int MM, bool BRICKS>
__global__ void __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(HK_FLAT_TRACK_WAVES))) k_track_pool(DPathState st, DScene sc, DFrame fr, int depth, DStats* stats, const DMedium* __restrict__ media) {
    __shared__ int lds_all[4 * TP_WAVE_INTS];
    int* const pool = lds_all + (threadIdx.x >> 6) * TP_WAVE_INTS;   // [field][64]
    int* const ring = pool + TP_FIELDS * 64;                          // [slot | key | r_l factor][TP_RING]
    int* const segc = ring + 3 * TP_RING;                             // [tag][16]: entries in the segment's escaped, scatter and per-kind queues; [15] = the segment
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_coll = 0, n_dda = 0;
    HK_DBG_DECL
    const DPathGen g = gen_at(st, depth);
    const bool ones = depth == 0 && fr.implicit_ones;
    const DMedium& med = media[0];
    const float a0 = eval_flat(med.sigma_a), s0 = eval_flat(med.sigma_s);
    const float sig_t = a0 + s0;   // (base_a + base_s).x of the general code
    const int mrx = med.mres[0], mry = med.mres[1], mrz = med.mres[2];
    const float* __restrict__ maj = med.majorant;
    const bool last_depth = depth >= fr.max_depth;
    const int gate_min = fr.track_gate & 0xff, gate_cap = fr.delta_advance + ((fr.track_gate >> 8) & 0xff);
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_TRACK), true, depth, Q_MEDIUM);
    int cur_tag = 0;          // up to TP_TAGS segments are open at a time (a path's tag: bits TP_TAG_SHIFT.. of its flag word): the wave goes on
                              // with the next segment while the last paths of the previous ones are still in flight
    if (lane < TP_TAGS) segc[lane * 16 + 15] = -1;
    const uint32_t* __restrict__ queue = st.medium_q;
    int n = 0, cursor = 0;
    bool more = true;
    int pool_n = 0, res_head = 0, res_n = 0;   // wave-uniform
    bool drain = false;                         // route the whole ring, not only full chunks
    auto open_seg = [&](int tag, int gw) {
        if (lane < 2 + HK_MAX_KINDS) segc[tag * 16 + lane] = lane == 1 ? 0 : *count_ptr(st, depth, lane == 0 ? Q_ESCAPED : Q_MAT0 + lane - 2, gw);
        if (lane == 15) segc[tag * 16 + 15] = gw;
    };
    auto close_seg = [&](int tag) {
        const int gw = __builtin_amdgcn_readfirstlane(segc[tag * 16 + 15]);
        if (gw >= 0 && lane < 2 + HK_MAX_KINDS) *count_ptr(st, depth, lane == 0 ? Q_ESCAPED : (lane == 1 ? Q_SCATTER : Q_MAT0 + lane - 2), gw) = segc[tag * 16 + lane];
        if (lane == 15) segc[tag * 16 + 15] = -1;
    };
    // route the first cnt (<= 64) entries of the ring: r_l update and classification of the survivors, then ballot compaction per destination
    auto route = [&](int cnt) {
        wave_lds_fence();
        const bool have = lane < cnt;
        const int p = (res_head + lane) & (TP_RING - 1);
        uint32_t rslot = 0, eflag = 0u;
        int key = -1;
        if (have) {
            rslot = (uint32_t)ring[p];
            key = ring[TP_RING + p];
        }
        HK_DBG(6, have);
        if (have && (key & 15) == TP_SURVIVED) {
            // survived to t_max: hand the stored surface hit / the escape over with the updated throughput
            const float rl = __int_as_float(ring[2 * TP_RING + p]);
            mul_rl(g, rslot, ones, rl, st.compact != 0);
            const float4 H = st.hit[rslot];
            const int prim = __float_as_int(H.y);
            int cls = 0;
            if (prim >= 0) {
                const int mat_word = st.mat_id[rslot];
                eflag = (mat_word & HK_MAT_EMISSIVE_BIT) != 0 ? HK_MATQ_EMISSIVE : 0u;   // (a surface hit: its destination below is a kind queue)
                int mat = mat_word & ~HK_MAT_EMISSIVE_BIT;
                if (sc.materials[mat].kind == HK_MAT_MIX) {
                    const float4 O = g.ray_o[rslot], D = g.ray_d[rslot];
                    const v3 o = mk3(O.x, O.y, O.z), d = mk3(D.x, D.y, D.z);
                    const float w = 1.0f - H.z - H.w;
                    mat = resolve_mix_material(sc, mat, o + d * H.x, -d, uv_at(sc, prim, w, H.z, H.w));
                    st.mat_id[rslot] = mat | (mat_word & HK_MAT_EMISSIVE_BIT);
                }
                const int kind = sc.materials[mat].kind;
                cls = 2 + (kind == HK_MAT_MIX ? HK_MAT_FALLBACK : kind);
            }
            key = (key & ~15) | cls;
        }
        res_head = (res_head + cnt) & (TP_RING - 1);
        res_n -= cnt;
        unsigned long long todo = __ballot(have);
        while (todo) {
            const int k = __builtin_amdgcn_readlane(key, __ffsll((long long)todo) - 1);   // wave-uniform destination
            const unsigned long long m = __ballot(key == k);
            const int base = __builtin_amdgcn_readfirstlane(segc[k]);
            const int gw = __builtin_amdgcn_readfirstlane(segc[(k & ~15) + 15]), cls = k & 15;
            uint32_t* __restrict__ q = cls == 0 ? st.escaped_q + (size_t)gw * st.wave_cap
                                     : cls == 1 ? st.scatter_q + (size_t)gw * st.wave_cap
                                                : st.mat_q + ((size_t)(cls - 2) * st.n_waves + gw) * st.wave_cap;
            if (key == k) q[base + __popcll(m & lt_mask)] = rslot | eflag;
            if (lane == 0) segc[k] = base + __popcll(m);
            todo &= ~m;
        }
        wave_lds_fence();
    };
    int state = TR_EMPTY, fl = 0;
    uint32_t slot = 0;
    v3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1), cur_o = mk3(0, 0, 0);
    float rl_f = 1.0f;
    uint64_t rng = 0;
    float it_tmin = 0.0f, it_tmax = 0.0f, nt0 = 0.0f, nt1 = 0.0f, nt2 = 0.0f, dl0 = 0.0f, dl1 = 0.0f, dl2 = 0.0f;
    int vx = 0, vy = 0, vz = 0;
    float seg1 = 0.0f, sm0 = 0.0f, t = 0.0f, pend_dt = 0.0f;
    int k_in_seg = 0, segi = 0;
    for (;;) {
        // ---- finished paths leave their result in the ring ----
        {
            const bool fin = state != TR_BUSY && state != TR_EMPTY;
            const unsigned long long m = __ballot(fin);
            if (m != 0ull) {
                if (fin) {
                    const int p = (res_head + res_n + __popcll(m & lt_mask)) & (TP_RING - 1);
                    ring[p] = (int)slot;
                    ring[TP_RING + p] = (((fl >> TP_TAG_SHIFT) & (TP_TAGS - 1)) << 4) | (state == TR_SCATTER ? 1 : TP_SURVIVED);   // (survivors are classified when routed)
                    ring[2 * TP_RING + p] = __float_as_int(rl_f);
                    state = TR_EMPTY;
                }
                res_n += __popcll(m);
            }
        }
        // full chunks of the ring are routed at once; all of it before a segment is retired and at the end (ONE call site: the routing
        // code with its Mix resolve is long)
        while (res_n >= (drain ? 1 : 64)) route(res_n < 64 ? res_n : 64);
        drain = false;
        unsigned long long free_m = __ballot(state == TR_EMPTY);
        // ---- the pool is empty and a lane is free: set up the next 64 entries of the segment's queue ----
        if (free_m != 0ull && pool_n == 0 && (cursor < n || more)) {
            while (more && cursor >= n) {
                // the current segment is used up: open the next one in the oldest slot as soon as that slot's last lane is done
                const int other = (cur_tag + 1) & (TP_TAGS - 1);
                const bool other_busy = __ballot(state == TR_BUSY && ((fl >> TP_TAG_SHIFT) & (TP_TAGS - 1)) == other) != 0ull;
                if (other_busy) break;   // every slot holds lanes in flight: the set-up waits
                if (res_n > 0) {         // its last results are still in the ring
                    drain = true;
                    break;
                }
                close_seg(other);
                const int gw = stream_next(stream, st.n_waves);
                if (gw >= st.n_waves) {
                    more = false;
                    break;
                }
                open_seg(other, gw);
                cur_tag = other;
                queue = st.medium_q + (size_t)gw * st.wave_cap;
                n = *count_ptr(st, depth, Q_MEDIUM, gw);
                cursor = 0;
            }
            if (drain) continue;
            const int avail = n - cursor;
            const int take = avail < 64 ? avail : 64;
            if (take > 0) HK_DBG(5, lane < take);
            if (lane < take) {
                const uint32_t s_new = queue[cursor + lane];
                const float4 O = g.ray_o[s_new], D = g.ray_d[s_new];
                const v3 o = mk3(O.x, O.y, O.z), d = mk3(D.x, D.y, D.z);
                const float t_max = st.hit[s_new].x;
                const bool dead = is_black(ld_throughput(g.beta, s_new, ones)) || is_black(ld_ru(g, s_new, ones, st.compact != 0));
                const uint64_t r = lcg_init(o, d, t_max);
                const MajorantIter it = create_majorant_iterator<MM>(med, o, d, t_max);
                int* e = pool + lane;
                e[TP_SLOT * 64] = (int)s_new;
                e[(TP_RO + 0) * 64] = __float_as_int(o.x);
                e[(TP_RO + 1) * 64] = __float_as_int(o.y);
                e[(TP_RO + 2) * 64] = __float_as_int(o.z);
                e[(TP_RD + 0) * 64] = __float_as_int(d.x);
                e[(TP_RD + 1) * 64] = __float_as_int(d.y);
                e[(TP_RD + 2) * 64] = __float_as_int(d.z);
                e[(TP_RNG + 0) * 64] = (int)(uint32_t)r;
                e[(TP_RNG + 1) * 64] = (int)(uint32_t)(r >> 32);
                e[TP_TMIN * 64] = __float_as_int(it.t_min);
                e[TP_TMAX * 64] = __float_as_int(it.t_max);
                e[(TP_NT + 0) * 64] = __float_as_int(it.next_t[0]);
                e[(TP_NT + 1) * 64] = __float_as_int(it.next_t[1]);
                e[(TP_NT + 2) * 64] = __float_as_int(it.next_t[2]);
                e[(TP_DL + 0) * 64] = __float_as_int(it.delta_t[0]);
                e[(TP_DL + 1) * 64] = __float_as_int(it.delta_t[1]);
                e[(TP_DL + 2) * 64] = __float_as_int(it.delta_t[2]);
                e[TP_VOX * 64] = (it.mode & 0xff) == 2 ? (it.voxel[0] | (it.voxel[1] << 10) | (it.voxel[2] << 20)) : 0;
                e[TP_FL * 64] = (cur_tag << TP_TAG_SHIFT) | (dead ? TF_DEAD_NULL : 0) | ((it.mode & 0xff) == 2 ? TF_IT_LIVE : 0) | (it.mode & 0x700);
            }
            pool_n = take > 0 ? take : 0;
            cursor += pool_n;
            wave_lds_fence();
        }
        // ---- free lanes take a ready state from the pool ----
        if (free_m != 0ull && pool_n > 0) {
            const int rank = __popcll(free_m & lt_mask);
            if (state == TR_EMPTY && rank < pool_n) {
                const int* e = pool + (pool_n - 1 - rank);
                slot = (uint32_t)e[TP_SLOT * 64];
                ro = mk3(__int_as_float(e[(TP_RO + 0) * 64]), __int_as_float(e[(TP_RO + 1) * 64]), __int_as_float(e[(TP_RO + 2) * 64]));
                rd = mk3(__int_as_float(e[(TP_RD + 0) * 64]), __int_as_float(e[(TP_RD + 1) * 64]), __int_as_float(e[(TP_RD + 2) * 64]));
                rng = (uint64_t)(uint32_t)e[(TP_RNG + 0) * 64] | ((uint64_t)(uint32_t)e[(TP_RNG + 1) * 64] << 32);
                it_tmin = __int_as_float(e[TP_TMIN * 64]);
                it_tmax = __int_as_float(e[TP_TMAX * 64]);
                nt0 = __int_as_float(e[(TP_NT + 0) * 64]), nt1 = __int_as_float(e[(TP_NT + 1) * 64]), nt2 = __int_as_float(e[(TP_NT + 2) * 64]);
                dl0 = __int_as_float(e[(TP_DL + 0) * 64]), dl1 = __int_as_float(e[(TP_DL + 1) * 64]), dl2 = __int_as_float(e[(TP_DL + 2) * 64]);
                const int vox = e[TP_VOX * 64];
                vx = vox & 1023, vy = (vox >> 10) & 1023, vz = vox >> 20;
                fl = e[TP_FL * 64];
                rl_f = 1.0f;
                segi = 0;
                state = TR_BUSY;
            }
            const int free_n = __popcll(free_m);
            pool_n -= free_n < pool_n ? free_n : pool_n;
            wave_lds_fence();
        }
        if (__ballot(state == TR_BUSY) == 0ull) {
            if (pool_n == 0 && cursor >= n && !more) {
                if (res_n == 0) break;
                drain = true;
            }
            continue;
        }
        // ---- phase A: cheap steps (next majorant cell, free-flight sample) until the busy lanes hold a tentative collision or have
        //      run out of cells ----
#pragma unroll 1
        for (int adv = 0;; ++adv) {
            const bool need = state == TR_BUSY && (fl & (TF_PENDING | TF_SURVIVED)) == 0;
            if (__ballot(need) == 0ull) break;
            if (adv >= fr.delta_advance) {
                if (adv >= gate_cap) break;
                if (__popcll(__ballot(state == TR_BUSY && (fl & TF_PENDING) != 0)) >= gate_min) break;
            }
            HK_DBG(0, need);
            if (need) {
                if ((fl & TF_IN_SEG) == 0) {
                    HK_DBG(1, true);
                    // majorant_next (media.jl:625-729) of a DDA iterator, straight-line
                    if ((fl & TF_IT_LIVE) == 0 || segi >= 256 || it_tmin >= it_tmax)
                        fl |= TF_SURVIVED;   // ran out of segments with the path still alive
                    else {
                        const bool lxy = nt0 < nt1, lxz = nt0 < nt2, lyz = nt1 < nt2;
                        const bool ax0 = lxy & lxz, ax1 = (!lxy) & lyz;   // axis 0, axis 1, else axis 2
                        const float nt = ax0 ? nt0 : (ax1 ? nt1 : nt2);
                        const float stm = minf(nt, it_tmax);
                        const float rho = maj[vx + mrx * (vy + mry * vz)];
                        const float seg0 = it_tmin;
                        seg1 = stm;
                        const bool neg = (fl & (ax0 ? TF_NEG0 : (ax1 ? TF_NEG1 : TF_NEG2))) != 0;
                        const int v = (ax0 ? vx : (ax1 ? vy : vz)) + (neg ? -1 : 1);
                        const int lim = neg ? -1 : (ax0 ? mrx : (ax1 ? mry : mrz));
                        const float s = nt + (ax0 ? dl0 : (ax1 ? dl1 : dl2));
                        vx = ax0 ? v : vx;
                        vy = ax1 ? v : vy;
                        vz = (ax0 | ax1) ? vz : v;
                        nt0 = ax0 ? s : nt0;
                        nt1 = ax1 ? s : nt1;
                        nt2 = (ax0 | ax1) ? nt2 : s;
                        const bool out = v == lim;
                        fl = out ? (fl & ~TF_IT_LIVE) : fl;
                        it_tmin = out ? it_tmax : stm;
                        ++segi;
                        ++n_dda;
                        sm0 = sig_t * rho;
                        if (sm0 >= 1e-10f) {
                            t = seg0;
                            cur_o = ro + rd * t;
                            fl |= TF_IN_SEG;
                            k_in_seg = 0;
                        }
                    }
                }
                // a lane that has just entered a cell draws its first free flight in the same round
                if ((fl & (TF_IN_SEG | TF_SURVIVED)) == TF_IN_SEG) {
                    HK_DBG(2, true);
                    if (k_in_seg >= 1024)
                        fl &= ~TF_IN_SEG;
                    else {
                        ++k_in_seg;
                        const float u = lcg_next(rng);
                        pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                        const float ts = t + pend_dt;
                        fl = ts >= seg1 ? (fl & ~TF_IN_SEG) : (fl | TF_PENDING);   // leaves the cell (T_maj / T_maj[1] = 1: nothing else changes) / tentative collision
                    }
                }
            }
        }
        // ---- phase B: the tentative collisions (medium lookup, absorb / scatter / null) ----
        HK_DBG(3, state == TR_BUSY && (fl & TF_PENDING) != 0);
        HK_DBG(4, state == TR_BUSY);
        if (state == TR_BUSY && (fl & TF_PENDING) != 0) {
            fl &= ~TF_PENDING;
            const float dt = pend_dt;
            const float Tm0 = media_expf((-dt) * sm0);
            const v3 p = cur_o + rd * dt;
            ++n_coll;
            const float d = sample_density<MM, BRICKS>(med, p);
            const float sa = a0 * d, ss = s0 * d;
            const float p_absorb = sa / sm0, p_scatter = ss / sm0;
            const float ue = lcg_next(rng);
            if (ue < p_absorb) {
                state = TR_EMPTY;  // absorbed
            } else if (ue < p_absorb + p_scatter) {
                if (last_depth)
                    state = TR_EMPTY;
                else {   // beta and r_u are rescaled by sigma_s T_maj / (sigma_s T_maj)[1] = 1: they stay as they are in the record
                    g.ray_o[slot] = make_float4(p.x, p.y, p.z, INF_F);  // the scattering vertex: k_scatter continues from here
                    state = TR_SCATTER;
                }
            } else {
                const float sn0 = maxf(sm0 - sa - ss, 0.0f);
                const float pdf = Tm0 * sn0;
                if (pdf > 1e-10f) {
                    rl_f = ((rl_f * Tm0) * sm0) * (1.0f / pdf);
                    t = t + dt;
                    cur_o = p;
                    if (fl & TF_DEAD_NULL) state = TR_EMPTY;
                } else
                    state = TR_EMPTY;
            }
        }
        if (state == TR_BUSY && (fl & TF_SURVIVED) != 0) state = ((fl & TF_DEAD_NULL) != 0 || last_depth) ? TR_EMPTY : TP_SURVIVED;
    }
#pragma unroll
    for (int tg = 0; tg < TP_TAGS; ++tg) close_seg(tg);
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->collisions, n_coll);
    wave_add(&stats->nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);   // (priced per scene: SURVEY 8d charges the NanoVDB tree walk)
    wave_add(&stats->dda_steps, n_dda);
}

// ---------------------------------------------------------------------------------------------------
// K5 + K6: direct lighting at a medium scattering vertex (light-BVH NEE with n = 0, HG evaluated with cos = wo.wi,
// medium-scatter.jl:15-138) and phase-function sampling (medium-scatter.jl:148-216).  First writer of this depth's shadow /
// next-ray segments.
// ---------------------------------------------------------------------------------------------------
template <bool FT>   // FT: this bounce's Sobol draws are table loads for every path (see k_shade)
__global__ void __launch_bounds__(256) k_scatter(DPathState st, DScene sc, DTables T, DFrame fr, DSobol sob, int depth, DStats* stats) {
    unsigned n_lnodes = 0, n_sv = 0;
    HK_FOR_EACH_WAVE_SEGMENT(gw, st, ticket_ptr(st, depth, TK_SCATTER), depth, Q_SCATTER) {
        const uint32_t* __restrict__ queue = st.scatter_q + (size_t)gw * st.wave_cap;
        const int n = *count_ptr(st, depth, Q_SCATTER, gw);
        const DPathGen g = gen_at(st, depth), gn = st.gen[(depth + 1) & 1];
        const size_t seg = (size_t)gw * st.wave_cap;
        WavePos q_shadow{0}, q_next{0};   // first writer of this depth's shadow records and of the next generation
        for (int base = 0; base < n; base += 64) {
            int i = base + lane_id();
            bool active = i < n;
            uint32_t slot = active ? queue[i] : 0u;
            bool push_shadow = false, push_ray = false;
            // records of the two pushes (written after the wave-wide position is known)
            float4 shO = make_float4(0, 0, 0, 0), shD = shO, nD = shO, O = shO;
            S4 shLd = s4(0.0f), shRu = s4(0.0f), shRl = s4(0.0f), lambda = s4(0.0f), beta = s4(0.0f), r_u = s4(0.0f), n_rl = s4(0.0f);
            uint32_t pslot = 0, nflags = 0;
            if (active) {
                ++n_sv;
                O = g.ray_o[slot];
                const float4 D = g.ray_d[slot];
                v3 sp = mk3(O.x, O.y, O.z), wo = mk3(-D.x, -D.y, -D.z);
                const uint2 meta = g.meta[slot];
                pslot = meta.y;
                const int medium_idx = (int)(meta.x >> 16) - 1;
                const float sg = sc.media[medium_idx].g;
                lambda = ld_lambda(st, g, slot, pslot);
                beta = ld4(&g.beta[slot]);
                r_u = ld_ru(g, slot, false, st.compact != 0);
                int pix, k;
                split_slot(fr, pslot, pix, k);
                SobolCtx sctx = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix, k, fr.first_sample + k * fr.sample_stride);
                const int base_dim = 6 + 7 * depth;
                if (sc.n_lights > 0) {
                    float light_select = sobol_1d<FT>(sctx, base_dim + 1);
                    float light_pmf;
                    int light_idx = bvh_sample_light(sc, sp, mk3(0, 0, 0), light_select, light_pmf, n_lnodes);
                    if (light_idx >= 1 && light_idx <= sc.n_lights && light_pmf > 0.0f) {
                        const DLight& sel = sc.lights[light_idx - 1];
                        v2 u_light = mk2(0.0f, 0.0f);
                        if (sel.kind >= HK_LIGHT_AMBIENT) u_light = sobol_2d<FT>(sctx, base_dim + 3);
                        LightSample ls = sample_light(sc, T, sel, sp, lambda, u_light);
                        if (ls.pdf > 0.0f && !is_black(ls.Li)) {
                            float phase_val = hg_p(sg, dot(wo, ls.wi));
                            if (phase_val > 0.0f) {
                                float light_pdf = ls.pdf * light_pmf;
                                float phase_pdf = ls.is_delta ? 0.0f : phase_val;
                                float tmx = ls.is_delta ? norm(ls.p_light - sp) - 0.001f : 1.0e6f;
                                shO = make_float4(sp.x, sp.y, sp.z, tmx);
                                shD = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, __int_as_float(medium_idx));
                                shLd = beta * phase_val * ls.Li;
                                shRu = r_u * phase_pdf;
                                shRl = r_u * light_pdf;
                                push_shadow = true;
                            }
                        }
                    }
                }
                int new_depth = depth + 1;
                if (new_depth < fr.max_depth) {
                    v2 u = sobol_2d<FT>(sctx, base_dim + 6);
                    float ppdf;
                    v3 wi = sample_hg(sg, wo, u, ppdf);
                    if (ppdf > 0.0f) {
                        nD = make_float4(wi.x, wi.y, wi.z, D.w);  // ray_o already holds the vertex, t_max = Inf
                        n_rl = r_u / ppdf;
                        nflags = (uint32_t)new_depth | (1u << 9) | ((uint32_t)(medium_idx + 1) << 16);  // specular = false, any_non_specular = true
                        push_ray = true;
                    }
                }
            }
            const size_t ps = seg + (size_t)wp_push(q_shadow, push_shadow);
            if (push_shadow) {
                st.sh_o[ps] = shO;
                st.sh_d[ps] = shD;
                st4(&st.sh_Ld[ps], shLd);
                st_shadow_weights(st, ps, shRu, shRl);
                st.sh_slot[ps] = pslot;
            }
            const size_t pn = seg + (size_t)wp_push(q_next, push_ray);
            if (push_ray) {   // the continuing path's record, whole, at its position in the next generation
                gn.ray_o[pn] = O;
                if (st.compact) nD.w = n_rl.x;
                gn.ray_d[pn] = nD;
                st4(&gn.beta[pn], beta);
                st_ru_rl(gn, pn, r_u, n_rl, st.compact != 0);
                st_lambda(gn, pn, lambda);
                gn.meta[pn] = make_uint2(nflags, pslot);
            }
        }
        if (lane_id() == 0) {
            *count_ptr(st, depth, Q_SHADOW, gw) = q_shadow.count;
            *count_ptr(st, depth + 1, Q_RAY, gw) = q_next.count;
        }
    }
    stats += global_wave();
    wave_add(&stats->sc_light_nodes, n_lnodes);
    wave_add(&stats->scatter_vertices, n_sv);
}

// K14: which medium is the camera in?  (intersection.jl:690-747)  One lane, result stays on the device.
__global__ void __launch_bounds__(64) k_detect_camera_medium(DPathState st, DScene sc, float cx, float cy, float cz, DStats* stats) {
    __shared__ int lds_stack[HK_LDS_STACK * 64];
    if (threadIdx.x != 0) return;
    v3 d = mk3(0.57735027f, 0.57735027f, 0.57735027f);
    v3 o = mk3(cx, cy, cz);
    int result = -1;
    unsigned a = 0, b = 0, casts = 0;
    for (int it = 0; it < 16; ++it) {
        bool dummy;
        ++casts;
        HitRec h = traverse<0, false>(sc, o, d, INF_F, lds_stack, 0, a, b, dummy);
        if (h.prim < 0) break;
        DMediumInterface mi = sc.mis[sc.meta[h.prim].mi];
        v3 n = geometric_normal(sc, h.prim);
        if (mi.inside != mi.outside) {
            result = dot(-d, n) > 0.0f ? mi.outside : mi.inside;
            break;
        }
        v3 off = dot(d, n) > 0.0f ? n : -n;
        o = (o + d * h.t) + off * 1e-4f;
    }
    *st.initial_medium = result;
    stats->rays_closest += casts;
}

#include "hk_shade.h"

#include "hk_shadow.h"

#include "hk_small_pass.h"

#ifndef HK_GREY_WALK_WAVES
#define HK_GREY_WALK_WAVES 4
#endif
enum { SH_EMPTY = 0, SH_CAST = 1, SH_TRACK = 2 };
#ifndef HK_SHADOW_FEED_ROUNDS
#define HK_SHADOW_FEED_ROUNDS 3
#endif
#ifndef HK_SHADOW_TRACK_BATCH
#define HK_SHADOW_TRACK_BATCH 4
#endif

// GREY: see k_track — the transmittance ratios of a flat-spectrum medium have four equal components, so T_ray, r_u, r_l and the
// per-segment ratio-tracking state are one float each (same operations, in the same order, as the general code performs on the
// first component), no wavelengths are fetched, and a cell boundary costs nothing.
template <bool COUNT, int MM, int STACK = HK_LDS_STACK, bool GREY = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(HK_TRACE_BLOCK, HK_TRACE_BLOCK), amdgpu_waves_per_eu(MM == 0 ? 4 : GREY ? HK_GREY_WALK_WAVES : (MM == 8 || MM == 2 || MM == 1) ? 3 : HK_MEDIA_WAVES))) k_shadow_walk(DPathState st, DScene sc, DTables T, int depth, int tune, DStats* stats, const DMedium* __restrict__ media) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * STACK * 64];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0, n_coll = 0, n_dda = 0;
    HK_DBG_DECL
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_SHADOW), true, depth, Q_SHADOW);
    uint32_t rec0 = 0;   // current segment's shadow records: entries rec0 .. rec0 + n - 1 (the wave streams segment after segment)
    int n = 0, cursor = 0;
    bool more = true;
    int state = SH_EMPTY;
    uint32_t slot = 0;
    v3 ro = mk3(0, 0, 0), dir = mk3(0, 0, 1);
    float t_remaining = 0.0f, hit_t = 0.0f;
    int medium = -1, next_medium = -1, seg = 0;
    bool miss_case = false, transition = false;
    using W = typename std::conditional<GREY, float, S4>::type;   // a spectral weight: four wavelengths, or one value for all four
    W T_ray = wone<W>(), tr_u = wone<W>(), tr_l = wone<W>();
    S4 lambda = s4(0.0f);
    // ratio-tracking state of the current medium segment
    W sT = wone<W>(), su = wone<W>(), sl = wone<W>();
    S4 base_a = s4(0.0f), base_s = s4(0.0f), base_Le = s4(0.0f), sm = s4(0.0f);
    float a0 = 0.0f, s0 = 0.0f;   // GREY: the flat sigma_a / sigma_s values
    MajorantIter it = exhausted_iter();
    PCG32 rng = PCG32{0ull, 0ull};
    float seg1 = 0.0f, sm0 = 0.0f, t = 0.0f;
    bool in_seg = false, after_inner = false, pending = false;
    float pend_dt = 0.0f;
    int k_in_seg = 0, segi = 0;
    int feed_rounds = 0;
    for (;;) {
        // ---- refill ----
        const unsigned long long busy_m = __ballot(state != SH_EMPTY);
        if (busy_m == 0ull || (64 - __popcll(busy_m) >= (tune >> 24) && (cursor < n || more))) {
            while (more && cursor >= n) {   // this segment is used up: go on with the next one, the lanes in flight keep running
                const int gw = stream_next(stream, st.n_waves);
                if (gw >= st.n_waves) {
                    more = false;
                    break;
                }
                rec0 = (uint32_t)gw * (uint32_t)st.wave_cap;
                n = *count_ptr(st, depth, Q_SHADOW, gw);
                cursor = 0;
            }
            const unsigned long long want = ~busy_m;
            const int avail = n - cursor;
            const int rank = __popcll(want & lt_mask);
            if (state == SH_EMPTY && rank < avail) {
                slot = rec0 + (uint32_t)(cursor + rank);
                float4 O = st.sh_o[slot], D = st.sh_d[slot];
                ro = mk3(O.x, O.y, O.z);
                dir = mk3(D.x, D.y, D.z);
                t_remaining = O.w;
                medium = __float_as_int(D.w);
                T_ray = wone<W>();
                tr_u = wone<W>();
                tr_l = wone<W>();
                if (MM != 0 && !GREY) lambda = ld4(&st.lambda_s[st.sh_slot[slot]]);
                seg = 0;
                state = t_remaining < 1e-6f ? SH_EMPTY : SH_CAST;  // a degenerate ray is simply not visible
            }
            const int want_n = __popcll(want);
            cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
            if (__ballot(state != SH_EMPTY) == 0ull) {
                if (cursor >= n && !more) break;
                continue;  // every fetched ray was degenerate (or the segment was empty): fetch again
            }
        }
        // ---- casts, for all lanes that need one (when enough of them wait, or nothing else can run) ----
        {
            const unsigned long long cast_m = __ballot(state == SH_CAST);
            const unsigned long long track_m = __ballot(state == SH_TRACK);
            if (cast_m != 0ull && (track_m == 0ull || __popcll(cast_m) >= ((tune >> 24) < 8 ? (tune >> 24) : 8))) {
                HK_DBG(0, state == SH_CAST);
                if (state == SH_CAST) {
                    bool opaque;
                    ++n_casts;
                    HitRec h = traverse<1, COUNT>(sc, ro, dir, t_remaining, stack, lane, n_nodes, n_tris, opaque);
                    bool alive = true;
                    if (h.prim < 0) {
                        miss_case = true;
                        hit_t = t_remaining;
                    } else {
                        ++n_hits;
                        miss_case = false;
                        hit_t = h.t;
                        if (opaque)
                            alive = false;
                        else {
                            DTriMeta meta = sc.meta[h.prim];
                            DMediumInterface mi = sc.mis[meta.mi];
                            v3 ng = geometric_normal(sc, h.prim);
                            bool entering = dot(dir, ng) < 0.0f;
                            transition = mi.inside != mi.outside;
                            next_medium = transition ? (entering ? mi.inside : mi.outside) : medium;
                            if (!transition) {
                                float w = 1.0f - h.u - h.v;
                                float alpha = surface_alpha(sc, mi.material, uv_at(sc, h.prim, w, h.u, h.v));
                                bool pass = false;
                                if (alpha < 1.0f) {
                                    PCG32 arng = pcg32_init(pbrt_hash(ro), pbrt_hash(dir));
                                    pass = pcg32_f32(arng) > alpha;
                                }
                                alive = pass;
                            }
                        }
                    }
                    if (!alive)
                        state = SH_EMPTY;  // blocked
                    else if (MM != 0 && medium >= 0) {
                        // ratio tracking over [0, hit_t] of this segment (intersection.jl:326-336, 376-386)
                        const DMedium& m = sc.n_media == 1 ? media[0] : media[medium];
                        sT = wone<W>();
                        su = wone<W>();
                        sl = wone<W>();
                        if constexpr (GREY) {
                            a0 = eval_flat(m.sigma_a);
                            s0 = eval_flat(m.sigma_s);
                            base_a = s4(a0);
                            base_s = s4(s0);
                        } else {
                            base_a = eval_scaled(m.sigma_a, lambda);
                            base_s = eval_scaled(m.sigma_s, lambda);
                            if (HK_HAS_MEDIUM(MM, HK_MEDIUM_HOMOGENEOUS)) base_Le = eval_scaled(m.Le, lambda);
                        }
                        it = create_majorant_iterator<MM>(m, ro, dir, hit_t);
                        rng = pcg32_init(pbrt_hash(ro), pbrt_hash(dir));
                        in_seg = false;
                        after_inner = false;
                        pending = false;
                        segi = 0;
                        state = SH_TRACK;
                    } else if (miss_case) {
                        shadow_contribute<MM == 0>(st, slot, wide(T_ray), wide(tr_u), wide(tr_l));
                        state = SH_EMPTY;
                    } else {
                        // step over the surface (no medium on this side)
                        bool stop = false;
                        if (transition) {
                            if (is_black(T_ray)) stop = true;
                            medium = next_medium;
                        }
                        ro = ro + dir * (hit_t + 1e-4f);
                        t_remaining = t_remaining - hit_t - 1e-4f;
                        ++seg;
                        state = (stop || seg >= 10 || t_remaining < 1e-6f) ? SH_EMPTY : SH_CAST;
                    }
                }
            }
        }
        // ---- short rays (one cast and done: shadow rays that start outside the medium, blocked ones) leave their lanes empty for the
        //      whole tracking batch below, which is where the time goes: fetch and cast again, a few times, until the wave is mostly
        //      tracking (the cloud's walk ran its collision rounds with 28 % of the lanes EMPTY although work was waiting) ----
        if (MM != 0 && feed_rounds < ((tune >> 16) & 0xff)) {
            const int waiting = __popcll(__ballot(state == SH_EMPTY)) + __popcll(__ballot(state == SH_CAST));
            if (waiting >= (tune >> 24) && (cursor < n || more)) {
                ++feed_rounds;
                continue;
            }
        }
        feed_rounds = 0;
        // ---- a few ratio-tracking rounds: cheap steps until a tentative collision is pending, then the collisions.  Lanes are
        //      served medium by medium so that the medium record is read through a wave-uniform index (scalar loads) ----
        if (MM != 0) {
            unsigned long long todo = __ballot(state == SH_TRACK);
            while (todo) {
                const int m_uniform = __builtin_amdgcn_readlane(medium, __ffsll((long long)todo) - 1);
                const bool mine = state == SH_TRACK && medium == m_uniform;
                const DMedium& med = media[m_uniform];
#pragma unroll 1
                for (int batch = 0; batch < (tune & 0xff); ++batch) {
                    if (__ballot(mine && state == SH_TRACK) == 0ull) break;
                    bool track_done = false;
#pragma unroll 1
                    for (int adv = 0; adv < ((tune >> 8) & 0xff); ++adv) {
                        const bool need = mine && state == SH_TRACK && !pending && !track_done;
                        if (__ballot(need) == 0ull) break;
                        HK_DBG(1, need);
                        if (!need) continue;
                        if (!in_seg) {
                            float seg0;
                            if (after_inner && is_black(sT))
                                track_done = true;
                            else if (segi >= 256 || !majorant_next<MM>(it, med, base_a + base_s, seg0, seg1, sm))
                                track_done = true;
                            else {
                                ++segi;
                                ++n_dda;
                                sm0 = sm.x;
                                if (sm0 >= 1e-10f) {
                                    t = seg0;
                                    in_seg = true;
                                    k_in_seg = 0;
                                }
                            }
                            after_inner = false;
                        }
                        if (!in_seg || track_done) {   // (a lane that has just entered a cell goes on in the same round: see k_track)
                        } else if (k_in_seg >= 100) {
                            in_seg = false;
                            after_inner = true;
                        } else {
                            ++k_in_seg;
                            float u = pcg32_f32(rng);
                            pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                            float ts = t + pend_dt;
                            if (ts >= seg1) {
                                if constexpr (!GREY) {   // GREY: T_maj / T_maj[1] = 1, nothing changes
                                    float dr = seg1 - t;
                                    S4 Tm = s4exp((-dr) * sm);
                                    float T0 = Tm.x;
                                    if (T0 > 1e-10f) {
                                        sT = div4(sT * Tm, T0);
                                        sl = div4(sl * Tm, T0);
                                        su = div4(su * Tm, T0);
                                    }
                                }
                                in_seg = false;
                                after_inner = true;
                            } else
                                pending = true;
                        }
                    }
                    HK_DBG(2, mine && state == SH_TRACK && pending);
                    HK_DBG(3, state == SH_TRACK);
                    HK_DBG(4, state == SH_CAST);
                    HK_DBG(5, state == SH_EMPTY);
                    if (GREY && mine && state == SH_TRACK && pending) {
                        if constexpr (GREY) {
                            pending = false;
                            const float dt = pend_dt;
                            const float ts = t + dt;
                            ++n_coll;
                            const float d = sample_density<MM>(med, ro + dir * ts);
                            const float sn0 = maxf(sm0 - a0 * d - s0 * d, 0.0f);
                            const float Tm0 = media_expf((-dt) * sm0);
                            const float pr = Tm0 * sm0;
                            if (pr > 1e-10f) {
                                const float inv = 1.0f / pr;
                                sT = ((sT * Tm0) * sn0) * inv;
                                sl = ((sl * Tm0) * sm0) * inv;
                                su = ((su * Tm0) * sn0) * inv;
                                const float est = sT * (1.0f / maxf(1e-10f, average_flat(sl + su)));
                                if (est < 0.05f) {
                                    float rr = pcg32_f32(rng);
                                    if (rr < 0.75f) {
                                        sT = 0.0f;
                                        track_done = true;
                                    } else
                                        sT = sT / (1.0f - 0.75f);
                                }
                                if (sT == 0.0f) track_done = true;
                                t = ts;
                            } else {
                                sT = 0.0f;
                                track_done = true;
                            }
                        }
                    }
                    if (!GREY && mine && state == SH_TRACK && pending) {
                      if constexpr (!GREY) {
                        pending = false;
                        const float dt = pend_dt;
                        const float ts = t + dt;
                        ++n_coll;
                        MediumProps mp = sample_point<MM>(T, lambda, med, base_a, base_s, base_Le, ro + dir * ts);
                        S4 sn = s4max0(sm - mp.sigma_a - mp.sigma_s);
                        S4 Tm = s4exp((-dt) * sm);
                        float pr = Tm.x * sm0;
                        if (pr > 1e-10f) {
                            sT = div4(sT * Tm * sn, pr);
                            sl = div4(sl * Tm * sm, pr);
                            su = div4(su * Tm * sn, pr);
                            S4 est = div4(sT, maxf(1e-10f, average(sl + su)));
                            if (max_component(est) < 0.05f) {
                                float rr = pcg32_f32(rng);
                                if (rr < 0.75f) {
                                    sT = s4(0.0f);
                                    track_done = true;
                                } else
                                    sT = sT / (1.0f - 0.75f);
                            }
                            if (is_black(sT)) track_done = true;
                            t = ts;
                        } else {
                            sT = s4(0.0f);
                            track_done = true;
                        }
                    }
                    }
                    if (track_done) {
                        T_ray = T_ray * sT;
                        tr_u = tr_u * su;
                        tr_l = tr_l * sl;
                        if (miss_case) {
                            shadow_contribute<MM == 0>(st, slot, wide(T_ray), wide(tr_u), wide(tr_l));
                            state = SH_EMPTY;
                        } else {
                            bool stop = false;
                            if (transition) {
                                if (is_black(T_ray)) stop = true;
                                medium = next_medium;
                            }
                            ro = ro + dir * (hit_t + 1e-4f);
                            t_remaining = t_remaining - hit_t - 1e-4f;
                            ++seg;
                            state = (stop || seg >= 10 || t_remaining < 1e-6f) ? SH_EMPTY : SH_CAST;
                        }
                    }
                }
                todo &= ~__ballot(mine);
            }
        }
    }
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->sh_collisions, n_coll);
    wave_add(&stats->sh_nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);
    wave_add(&stats->sh_dda_steps, n_dda);
    wave_add(&stats->rays_shadow, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->sh_nodes, n_nodes);
        wave_add(&stats->sh_tris, n_tris);
    }
}

// ---------------------------------------------------------------------------------------------------
// k_walk_pool: K10 of a scene whose ONE medium is GREY (k_shadow_walk<.., GREY = true> above; same arithmetic and RNG consumption per
// shadow ray, films bit-identical: tools/ab_bitwise.py, HK_WALK_POOL=0 runs the older kernel), with the two halves of a walk taken apart
// INSIDE the wave (the split into two kernels lost to the traffic and the random order of its hand-over queues):
//   * CAST PHASE, dense: whenever the wave's pool is empty and a lane is free, ALL 64 lanes cast — lanes that hold a ray waiting for its
//     next segment cast that one, every other lane (tracking or idle) the next shadow record of the stream — then run the surface logic
//     of intersection.jl:316-406 and, for the rays that have a stretch of medium in front of them, the set-up of the ratio tracker
//     (majorant iterator: 18 IEEE divisions; PCG seed: two 64-bit Murmur hashes).  What goes on is written to the POOL in LDS
//     (26 words per ray, CAP entries; a phase takes no more rays than the pool has room for).  In k_shadow_walk this code ran for
//     the 16 - 25 lanes that happened to be idle, and the tracking rounds ran with 46 % of the lanes waiting for it.
//     STACK / CAP: 16-entry traversal stacks and 48 pool entries are 36 KB of LDS per 4-wave block, four blocks per CU (8-entry stacks
//     and 64 pool entries for the example's shallow BVH measured the same: 0.305 against 0.308 s).
//   * TRACKING ROUNDS: a lane whose stretch ends takes the next ready ray from the pool in the same round (26 LDS reads); lane
//     flags in one VGPR, straight-line DDA step (see k_track_flat).
// ---------------------------------------------------------------------------------------------------
enum { WP_SLOT = 0, WP_RO = 1, WP_DIR = 4, WP_TREM = 7, WP_HIT = 8, WP_T = 9, WP_U = 10, WP_L = 11, WP_TMIN = 12, WP_TMAX = 13, WP_NT = 14, WP_DL = 17, WP_VOX = 20, WP_RNG = 21,
       WP_FL = 25, WP_FIELDS = 26 };
enum { WF_IN_SEG = 1, WF_PENDING = 2, WF_DONE = 4, WF_AFTER_INNER = 8, WF_IT_LIVE = 32, WF_NEG0 = 0x100, WF_NEG1 = 0x200, WF_NEG2 = 0x400, WF_MISS = 0x1000, WF_TRANSITION = 0x2000,
       WF_NEXT_MEDIUM = 0x4000, WF_MEDIUM = 0x8000, WF_SEG_SHIFT = 16, WF_SEG_MASK = 0xf0000, WF_CAST = 0x100000 };
#ifndef HK_WALK_POOL_WAVES
#define HK_WALK_POOL_WAVES 4
#endif
#ifndef HK_WALK_POOL_NC
#define HK_WALK_POOL_NC 16
#define HK_WALK_POOL_NT 32
#endif
template <bool COUNT, int MM, bool BRICKS, int STACK, int CAP>
__global__ void __attribute__((amdgpu_flat_work_group_size(HK_TRACE_BLOCK, HK_TRACE_BLOCK), amdgpu_waves_per_eu(HK_WALK_POOL_WAVES))) k_walk_pool(DPathState st, DScene sc, int depth, int tune, int gate, DStats* stats, const DMedium* __restrict__ media) {
    constexpr int WAVE_INTS = WP_FIELDS * CAP + STACK * 64;
    __shared__ int lds_all[(HK_TRACE_BLOCK / 64) * WAVE_INTS];
    int* const pool = lds_all + (threadIdx.x >> 6) * WAVE_INTS;   // [field][CAP]
    int* const stack = pool + WP_FIELDS * CAP;
    // the shallow-BVH instantiation (a cloud in a box: a few dozen triangles) casts from LDS: nodes and leaf triangles, 2.5 KB per block
    constexpr int NC = STACK <= 8 ? HK_WALK_POOL_NC : 0, NT = STACK <= 8 ? HK_WALK_POOL_NT : 0;
    __shared__ float4 lds_box[NC > 0 ? 3 * NC : 1];
    __shared__ int2 lds_child[NC > 0 ? NC : 1];
    __shared__ float4 lds_tri[NT > 0 ? 3 * NT : 1];
    const NodeCache cache = NC > 0 ? scene_cache_fill<NC, NT, HK_TRACE_BLOCK>(sc, lds_box, lds_child, lds_tri) : NodeCache();
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0, n_coll = 0, n_dda = 0;
    HK_DBG_DECL
    const DMedium& med = media[0];
    const float a0 = eval_flat(med.sigma_a), s0 = eval_flat(med.sigma_s);
    const float sig_t = a0 + s0;
    const int mrx = med.mres[0], mry = med.mres[1], mrz = med.mres[2];
    const float* __restrict__ maj = med.majorant;
    const int adv_n = (tune >> 8) & 0xff;
    const int gate_min = gate & 0xff, gate_cap = adv_n + ((gate >> 8) & 0xff);   // a collision round waits for gate_min pending lanes, for at most gate_cap cheap steps
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_SHADOW), true, depth, Q_SHADOW);
    uint32_t rec0 = 0;   // current segment's shadow records: entries rec0 .. rec0 + n - 1 (the wave streams segment after segment)
    int n = 0, cursor = 0;
    bool more = true;
    int track_n = 0, cast_n = 0;   // wave-uniform: ready rays at pool[0 .. track_n), rays waiting for a cast at pool[CAP - cast_n .. CAP)
    int state = SH_EMPTY, fl = 0;
    uint32_t slot = 0;
    v3 ro = mk3(0, 0, 0), dir = mk3(0, 0, 1);
    float t_remaining = 0.0f, hit_t = 0.0f;
    float T_ray = 1.0f, tr_u = 1.0f, tr_l = 1.0f, sT = 1.0f, su = 1.0f, sl = 1.0f;
    float it_tmin = 0.0f, it_tmax = 0.0f, nt0 = 0.0f, nt1 = 0.0f, nt2 = 0.0f, dl0 = 0.0f, dl1 = 0.0f, dl2 = 0.0f;
    int vx = 0, vy = 0, vz = 0;
    PCG32 rng = PCG32{0ull, 0ull};
    float seg1 = 0.0f, sm0 = 0.0f, t = 0.0f, pend_dt = 0.0f;
    int k_in_seg = 0, segi = 0;
    for (;;) {
        const unsigned long long track_m = __ballot(state == SH_TRACK);
        // ---- cast phase: no ready ray is left in the pool and a lane is not tracking (or every lane holds a waiting ray) ----
        const bool own = state == SH_CAST;   // (a lane keeps a waiting ray itself only when the pool had no room for it)
        const unsigned long long own_m = __ballot(own);
        if (~track_m != 0ull && (track_n == 0 || own_m == ~0ull)) {
            // the rays of the phase: the lanes' own waiting ones, then the pool's waiting ones, then the next records of the stream — as
            // many of those as the pool could take back (every ray leaves at most one entry behind); the records may come from several
            // segments (the deep bounces' segments hold a few dozen records each)
            const int n_other = 64 - __popcll(own_m);
            const int c_take = cast_n < n_other ? cast_n : n_other;
            const int rank = __popcll(~own_m & lt_mask);
            const bool from_pool = !own && rank < c_take;
            bool fresh = false;
            uint32_t c_slot = slot;
            int f_take = 0;
            {
                int want = n_other - c_take < CAP - track_n - cast_n ? n_other - c_take : CAP - track_n - cast_n;
                while (want > 0) {
                    while (more && cursor >= n) {   // this segment is used up: go on with the next one
                        const int gw = stream_next(stream, st.n_waves);
                        if (gw >= st.n_waves) {
                            more = false;
                            break;
                        }
                        rec0 = (uint32_t)gw * (uint32_t)st.wave_cap;
                        n = *count_ptr(st, depth, Q_SHADOW, gw);
                        cursor = 0;
                    }
                    const int avail = n - cursor;
                    if (avail <= 0) break;
                    const int take = avail < want ? avail : want;
                    const int r = rank - c_take - f_take;
                    if (!own && r >= 0 && r < take) {
                        fresh = true;
                        c_slot = rec0 + (uint32_t)(cursor + r);
                    }
                    cursor += take;
                    f_take += take;
                    want -= take;
                }
            }
            if (own_m == 0ull && c_take == 0 && f_take == 0) {
                if (track_m == 0ull) break;   // nothing in flight, nothing left
            } else {
                v3 c_ro = ro, c_dir = dir;
                float c_trem = t_remaining, c_T = T_ray, c_u = tr_u, c_l = tr_l;
                int c_fl = fl & (WF_MEDIUM | WF_SEG_MASK);
                if (from_pool) {
                    const int* e = pool + (CAP - cast_n + rank);
                    c_slot = (uint32_t)e[WP_SLOT * CAP];
                    c_ro = mk3(__int_as_float(e[(WP_RO + 0) * CAP]), __int_as_float(e[(WP_RO + 1) * CAP]), __int_as_float(e[(WP_RO + 2) * CAP]));
                    c_dir = mk3(__int_as_float(e[(WP_DIR + 0) * CAP]), __int_as_float(e[(WP_DIR + 1) * CAP]), __int_as_float(e[(WP_DIR + 2) * CAP]));
                    c_trem = __int_as_float(e[WP_TREM * CAP]);
                    c_T = __int_as_float(e[WP_T * CAP]);
                    c_u = __int_as_float(e[WP_U * CAP]);
                    c_l = __int_as_float(e[WP_L * CAP]);
                    c_fl = e[WP_FL * CAP] & (WF_MEDIUM | WF_SEG_MASK);
                }
                if (fresh) {
                    const float4 O = st.sh_o[c_slot], D = st.sh_d[c_slot];
                    c_ro = mk3(O.x, O.y, O.z);
                    c_dir = mk3(D.x, D.y, D.z);
                    c_trem = O.w;
                    c_T = c_u = c_l = 1.0f;
                    c_fl = __float_as_int(D.w) >= 0 ? WF_MEDIUM : 0;
                }
                cast_n -= c_take;
                wave_lds_fence();
                const bool active = own || from_pool || (fresh && !(c_trem < 1e-6f));   // a degenerate ray is simply not visible
                int out = 0;   // 0: the ray ended here, 1: ready to track, 2: waits for another cast
                float c_hit = 0.0f;
                MajorantIter it = exhausted_iter();
                PCG32 c_rng = PCG32{0ull, 0ull};
                HK_DBG(8, active);
                if (active) {
                    bool opaque;
                    ++n_casts;
                    const HitRec h = traverse<1, COUNT, NC, NT>(sc, c_ro, c_dir, c_trem, stack, lane, n_nodes, n_tris, opaque, cache);
                    bool alive = true, miss_case = true, transition = false;
                    int next_medium = -1;
                    c_hit = c_trem;
                    if (h.prim >= 0) {
                        ++n_hits;
                        miss_case = false;
                        c_hit = h.t;
                        if (opaque)
                            alive = false;
                        else {
                            const DTriMeta meta = sc.meta[h.prim];
                            const DMediumInterface mi = sc.mis[meta.mi];
                            const v3 ng = geometric_normal(sc, h.prim);
                            const bool entering = dot(c_dir, ng) < 0.0f;
                            transition = mi.inside != mi.outside;
                            next_medium = transition ? (entering ? mi.inside : mi.outside) : ((c_fl & WF_MEDIUM) ? 0 : -1);
                            if (!transition) {
                                const float w = 1.0f - h.u - h.v;
                                const float alpha = surface_alpha(sc, mi.material, uv_at(sc, h.prim, w, h.u, h.v));
                                bool pass = false;
                                if (alpha < 1.0f) {
                                    PCG32 arng = pcg32_init(pbrt_hash(c_ro), pbrt_hash(c_dir));
                                    pass = pcg32_f32(arng) > alpha;
                                }
                                alive = pass;
                            }
                        }
                    }
                    if (!alive) {
                        // blocked
                    } else if (c_fl & WF_MEDIUM) {
                        // ratio tracking over [0, c_hit] of this segment (intersection.jl:326-336, 376-386): set up here, run in the tracking rounds
                        it = create_majorant_iterator<MM>(med, c_ro, c_dir, c_hit);
                        c_rng = pcg32_init(pbrt_hash(c_ro), pbrt_hash(c_dir));
                        c_fl |= (miss_case ? WF_MISS : 0) | (transition ? WF_TRANSITION : 0) | (next_medium >= 0 ? WF_NEXT_MEDIUM : 0) | ((it.mode & 0xff) == 2 ? WF_IT_LIVE : 0) | (it.mode & 0x700);
                        out = 1;
                    } else if (miss_case) {
                        shadow_contribute_rt(st, c_slot, s4(c_T), s4(c_u), s4(c_l));
                    } else {
                        // step over the surface (no medium on this side)
                        const bool stop = transition && c_T == 0.0f;
                        if (transition) c_fl = (c_fl & ~WF_MEDIUM) | (next_medium >= 0 ? WF_MEDIUM : 0);
                        c_ro = c_ro + c_dir * (c_hit + 1e-4f);
                        c_trem = c_trem - c_hit - 1e-4f;
                        const int seg = ((c_fl & WF_SEG_MASK) >> WF_SEG_SHIFT) + 1;
                        c_fl = (c_fl & ~WF_SEG_MASK) | (seg << WF_SEG_SHIFT);
                        out = (stop || seg >= 10 || c_trem < 1e-6f) ? 0 : 2;
                    }
                }
                HK_DBG(9, out == 1);
                const int c_vox = (c_fl & WF_IT_LIVE) ? (it.voxel[0] | (it.voxel[1] << 10) | (it.voxel[2] << 20)) : 0;
                // ---- a lane's own ray stays with the lane ----
                if (own) {
                    slot = c_slot;
                    ro = c_ro, dir = c_dir;
                    t_remaining = c_trem, hit_t = c_hit;
                    T_ray = c_T, tr_u = c_u, tr_l = c_l;
                    it_tmin = it.t_min, it_tmax = it.t_max;
                    nt0 = it.next_t[0], nt1 = it.next_t[1], nt2 = it.next_t[2];
                    dl0 = it.delta_t[0], dl1 = it.delta_t[1], dl2 = it.delta_t[2];
                    vx = c_vox & 1023, vy = (c_vox >> 10) & 1023, vz = c_vox >> 20;
                    rng = c_rng;
                    fl = c_fl;
                    sT = su = sl = 1.0f;
                    segi = 0;
                    state = out == 1 ? SH_TRACK : (out == 2 ? SH_CAST : SH_EMPTY);
                }
                // ---- the others' rays go to the pool: ready ones from the bottom, waiting ones from the top ----
                const unsigned long long ready_m = __ballot(!own && out == 1), wait_m = __ballot(!own && out == 2);
                if (!own && out != 0) {
                    int* e = pool + (out == 1 ? track_n + __popcll(ready_m & lt_mask) : CAP - 1 - cast_n - __popcll(wait_m & lt_mask));
                    e[WP_SLOT * CAP] = (int)c_slot;
                    e[(WP_RO + 0) * CAP] = __float_as_int(c_ro.x);
                    e[(WP_RO + 1) * CAP] = __float_as_int(c_ro.y);
                    e[(WP_RO + 2) * CAP] = __float_as_int(c_ro.z);
                    e[(WP_DIR + 0) * CAP] = __float_as_int(c_dir.x);
                    e[(WP_DIR + 1) * CAP] = __float_as_int(c_dir.y);
                    e[(WP_DIR + 2) * CAP] = __float_as_int(c_dir.z);
                    e[WP_TREM * CAP] = __float_as_int(c_trem);
                    e[WP_T * CAP] = __float_as_int(c_T);
                    e[WP_U * CAP] = __float_as_int(c_u);
                    e[WP_L * CAP] = __float_as_int(c_l);
                    e[WP_FL * CAP] = c_fl;
                    if (out == 1) {
                        e[WP_HIT * CAP] = __float_as_int(c_hit);
                        e[WP_TMIN * CAP] = __float_as_int(it.t_min);
                        e[WP_TMAX * CAP] = __float_as_int(it.t_max);
                        e[(WP_NT + 0) * CAP] = __float_as_int(it.next_t[0]);
                        e[(WP_NT + 1) * CAP] = __float_as_int(it.next_t[1]);
                        e[(WP_NT + 2) * CAP] = __float_as_int(it.next_t[2]);
                        e[(WP_DL + 0) * CAP] = __float_as_int(it.delta_t[0]);
                        e[(WP_DL + 1) * CAP] = __float_as_int(it.delta_t[1]);
                        e[(WP_DL + 2) * CAP] = __float_as_int(it.delta_t[2]);
                        e[WP_VOX * CAP] = c_vox;
                        e[(WP_RNG + 0) * CAP] = (int)(uint32_t)c_rng.state;
                        e[(WP_RNG + 1) * CAP] = (int)(uint32_t)(c_rng.state >> 32);
                        e[(WP_RNG + 2) * CAP] = (int)(uint32_t)c_rng.inc;
                        e[(WP_RNG + 3) * CAP] = (int)(uint32_t)(c_rng.inc >> 32);
                    }
                }
                track_n += __popcll(ready_m);
                cast_n += __popcll(wait_m);
                wave_lds_fence();
            }
        }
        // ---- free lanes take a ready ray from the pool ----
        {
            const unsigned long long free_m = __ballot(state == SH_EMPTY);
            if (free_m != 0ull && track_n > 0) {
                const int rank = __popcll(free_m & lt_mask);
                if (state == SH_EMPTY && rank < track_n) {
                    const int* e = pool + (track_n - 1 - rank);
                    slot = (uint32_t)e[WP_SLOT * CAP];
                    ro = mk3(__int_as_float(e[(WP_RO + 0) * CAP]), __int_as_float(e[(WP_RO + 1) * CAP]), __int_as_float(e[(WP_RO + 2) * CAP]));
                    dir = mk3(__int_as_float(e[(WP_DIR + 0) * CAP]), __int_as_float(e[(WP_DIR + 1) * CAP]), __int_as_float(e[(WP_DIR + 2) * CAP]));
                    t_remaining = __int_as_float(e[WP_TREM * CAP]);
                    hit_t = __int_as_float(e[WP_HIT * CAP]);
                    T_ray = __int_as_float(e[WP_T * CAP]);
                    tr_u = __int_as_float(e[WP_U * CAP]);
                    tr_l = __int_as_float(e[WP_L * CAP]);
                    it_tmin = __int_as_float(e[WP_TMIN * CAP]);
                    it_tmax = __int_as_float(e[WP_TMAX * CAP]);
                    nt0 = __int_as_float(e[(WP_NT + 0) * CAP]), nt1 = __int_as_float(e[(WP_NT + 1) * CAP]), nt2 = __int_as_float(e[(WP_NT + 2) * CAP]);
                    dl0 = __int_as_float(e[(WP_DL + 0) * CAP]), dl1 = __int_as_float(e[(WP_DL + 1) * CAP]), dl2 = __int_as_float(e[(WP_DL + 2) * CAP]);
                    const int vox = e[WP_VOX * CAP];
                    vx = vox & 1023, vy = (vox >> 10) & 1023, vz = vox >> 20;
                    rng.state = (uint64_t)(uint32_t)e[(WP_RNG + 0) * CAP] | ((uint64_t)(uint32_t)e[(WP_RNG + 1) * CAP] << 32);
                    rng.inc = (uint64_t)(uint32_t)e[(WP_RNG + 2) * CAP] | ((uint64_t)(uint32_t)e[(WP_RNG + 3) * CAP] << 32);
                    fl = e[WP_FL * CAP];
                    sT = su = sl = 1.0f;
                    segi = 0;
                    state = SH_TRACK;
                }
                const int free_n = __popcll(free_m);
                track_n -= free_n < track_n ? free_n : track_n;
                wave_lds_fence();
            }
        }
        if (__ballot(state == SH_TRACK) == 0ull) continue;   // (the cast phase above ends the kernel when nothing is left)
        // ---- phase A: cheap steps (next majorant cell, free-flight sample) ----
#pragma unroll 1
        for (int adv = 0;; ++adv) {
            const bool need = state == SH_TRACK && (fl & (WF_PENDING | WF_DONE)) == 0;
            if (__ballot(need) == 0ull) break;
            if (adv >= adv_n) {
                if (adv >= gate_cap) break;
                if (__popcll(__ballot(state == SH_TRACK && (fl & WF_PENDING) != 0)) >= gate_min) break;
            }
            HK_DBG(10, need);
            if (need) {
                if ((fl & WF_IN_SEG) == 0) {
                    if (((fl & WF_AFTER_INNER) != 0 && sT == 0.0f) || segi >= 256 || (fl & WF_IT_LIVE) == 0 || it_tmin >= it_tmax)
                        fl |= WF_DONE;
                    else {
                        // majorant_next (media.jl:625-729) of a DDA iterator, straight-line
                        const bool lxy = nt0 < nt1, lxz = nt0 < nt2, lyz = nt1 < nt2;
                        const bool ax0 = lxy & lxz, ax1 = (!lxy) & lyz;   // axis 0, axis 1, else axis 2
                        const float nt = ax0 ? nt0 : (ax1 ? nt1 : nt2);
                        const float stm = minf(nt, it_tmax);
                        const float rho = maj[vx + mrx * (vy + mry * vz)];
                        const float seg0 = it_tmin;
                        seg1 = stm;
                        const bool neg = (fl & (ax0 ? WF_NEG0 : (ax1 ? WF_NEG1 : WF_NEG2))) != 0;
                        const int v = (ax0 ? vx : (ax1 ? vy : vz)) + (neg ? -1 : 1);
                        const int lim = neg ? -1 : (ax0 ? mrx : (ax1 ? mry : mrz));
                        const float s = nt + (ax0 ? dl0 : (ax1 ? dl1 : dl2));
                        vx = ax0 ? v : vx;
                        vy = ax1 ? v : vy;
                        vz = (ax0 | ax1) ? vz : v;
                        nt0 = ax0 ? s : nt0;
                        nt1 = ax1 ? s : nt1;
                        nt2 = (ax0 | ax1) ? nt2 : s;
                        const bool out_of_grid = v == lim;
                        fl = out_of_grid ? (fl & ~WF_IT_LIVE) : fl;
                        it_tmin = out_of_grid ? it_tmax : stm;
                        ++segi;
                        ++n_dda;
                        sm0 = sig_t * rho;
                        if (sm0 >= 1e-10f) {
                            t = seg0;
                            fl |= WF_IN_SEG;
                            k_in_seg = 0;
                        }
                    }
                    fl &= ~WF_AFTER_INNER;
                }
                // a lane that has just entered a cell draws its first free flight in the same round
                if ((fl & (WF_IN_SEG | WF_DONE)) == WF_IN_SEG) {
                    if (k_in_seg >= 100)
                        fl = (fl & ~WF_IN_SEG) | WF_AFTER_INNER;
                    else {
                        ++k_in_seg;
                        const float u = pcg32_f32(rng);
                        pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                        const float ts = t + pend_dt;
                        fl = ts >= seg1 ? ((fl & ~WF_IN_SEG) | WF_AFTER_INNER) : (fl | WF_PENDING);   // leaves the cell (T_maj / T_maj[1] = 1: nothing else changes) / tentative collision
                    }
                }
            }
        }
        // ---- phase B: the tentative collisions ----
        HK_DBG(11, state == SH_TRACK && (fl & WF_PENDING) != 0);
        HK_DBG(12, state == SH_TRACK);
        HK_DBG(13, state == SH_CAST);
        if (state == SH_TRACK && (fl & WF_PENDING) != 0) {
            fl &= ~WF_PENDING;
            const float dt = pend_dt;
            const float ts = t + dt;
            ++n_coll;
            const float d = sample_density<MM, BRICKS>(med, ro + dir * ts);
            const float sn0 = maxf(sm0 - a0 * d - s0 * d, 0.0f);
            const float Tm0 = media_expf((-dt) * sm0);
            const float pr = Tm0 * sm0;
            if (pr > 1e-10f) {
                const float inv = 1.0f / pr;
                sT = ((sT * Tm0) * sn0) * inv;
                sl = ((sl * Tm0) * sm0) * inv;
                su = ((su * Tm0) * sn0) * inv;
                const float est = sT * (1.0f / maxf(1e-10f, average_flat(sl + su)));
                if (est < 0.05f) {
                    const float rr = pcg32_f32(rng);
                    if (rr < 0.75f) {
                        sT = 0.0f;
                        fl |= WF_DONE;
                    } else
                        sT = sT / (1.0f - 0.75f);
                }
                if (sT == 0.0f) fl |= WF_DONE;
                t = ts;
            } else {
                sT = 0.0f;
                fl |= WF_DONE;
            }
        }
        // ---- the end of a stretch of medium: contribute (the ray reached its light), or leave the ray in the pool for the cast behind the surface ----
        {
            const bool fin = state == SH_TRACK && (fl & WF_DONE) != 0;
            const unsigned long long fin_m = __ballot(fin);
            if (fin_m != 0ull) {
                bool goes_on = false;
                if (fin) {
                    T_ray = T_ray * sT;
                    tr_u = tr_u * su;
                    tr_l = tr_l * sl;
                    state = SH_EMPTY;
                    if (fl & WF_MISS)
                        shadow_contribute_rt(st, slot, s4(T_ray), s4(tr_u), s4(tr_l));
                    else {
                        const bool stop = (fl & WF_TRANSITION) != 0 && T_ray == 0.0f;
                        const int medium_bit = (fl & WF_TRANSITION) ? ((fl & WF_NEXT_MEDIUM) ? WF_MEDIUM : 0) : WF_MEDIUM;
                        ro = ro + dir * (hit_t + 1e-4f);
                        t_remaining = t_remaining - hit_t - 1e-4f;
                        const int seg = ((fl & WF_SEG_MASK) >> WF_SEG_SHIFT) + 1;
                        fl = medium_bit | (seg << WF_SEG_SHIFT);
                        goes_on = !(stop || seg >= 10 || t_remaining < 1e-6f);
                    }
                }
                const unsigned long long on_m = __ballot(goes_on);
                if (on_m != 0ull) {
                    const int room = CAP - track_n - cast_n;
                    const int r = __popcll(on_m & lt_mask);
                    if (goes_on && r < room) {
                        int* e = pool + (CAP - 1 - cast_n - r);
                        e[WP_SLOT * CAP] = (int)slot;
                        e[(WP_RO + 0) * CAP] = __float_as_int(ro.x);
                        e[(WP_RO + 1) * CAP] = __float_as_int(ro.y);
                        e[(WP_RO + 2) * CAP] = __float_as_int(ro.z);
                        e[(WP_DIR + 0) * CAP] = __float_as_int(dir.x);
                        e[(WP_DIR + 1) * CAP] = __float_as_int(dir.y);
                        e[(WP_DIR + 2) * CAP] = __float_as_int(dir.z);
                        e[WP_TREM * CAP] = __float_as_int(t_remaining);
                        e[WP_T * CAP] = __float_as_int(T_ray);
                        e[WP_U * CAP] = __float_as_int(tr_u);
                        e[WP_L * CAP] = __float_as_int(tr_l);
                        e[WP_FL * CAP] = fl;
                    } else if (goes_on)
                        state = SH_CAST;   // no room: the lane keeps the ray until the next cast phase
                    const int pushed = __popcll(on_m);
                    cast_n += pushed < room ? pushed : room;
                    wave_lds_fence();
                }
            }
        }
    }
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->sh_collisions, n_coll);
    wave_add(&stats->sh_nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);
    wave_add(&stats->sh_dda_steps, n_dda);
    wave_add(&stats->rays_shadow, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->sh_nodes, n_nodes);
        wave_add(&stats->sh_tris, n_tris);
    }
}

// ---------------------------------------------------------------------------------------------------
// K10 of a scene whose (single) medium is GREY, SPLIT in two kernels.  k_shadow_walk carries the registers of the
// BVH traversal and of the ratio tracker together (128 VGPRs with spills at 4 waves per SIMD) and these loops are bound by instruction
// issue at low residency; the two halves never need each other's state:
//   k_walk_cast   one any-hit-style cast per record (LDS stacks + the scene's nodes and triangles in LDS, like k_trace), the surface
//                 logic of intersection.jl:316-406; a ray that has to cross a medium is parked in its record and queued for
//   k_walk_track  ratio tracking through the medium up to the surface found by the cast (intersection.jl:422-542): a flat state
//                 machine without traversal state; a ray that goes on behind the surface is queued for the next cast round.
// Rounds alternate cast(0), track(0), cast(1), ... on the host side (HK_WALK_ROUNDS casts: the reference walks <= 10 segments).
// Round 0 streams the shadow records of the wave segments like k_shadow_walk; later rounds read GLOBAL index queues filled with one
// atomic per wave and push: the order of the queue does not matter to the result, because a path slot receives at most one shadow
// contribution per depth (one NEE sample per vertex) — no two records of a launch add to the same L.
// In-flight state of a record: sh_o = (origin, t_remaining), sh_d = (direction, medium), sh_T = (T_ray, r_u, r_l, hit_t),
// sh_aux = segments | miss << 8 | transition << 9 | (next medium + 1) << 16.
// Same arithmetic per ray as k_shadow_walk<.., GREY = true>: films are bit-identical (tests: HK_WALK_SPLIT=0 against 1).
// ---------------------------------------------------------------------------------------------------
#define HK_WALK_ROUNDS 10
HKD int* walk_ctl(const DPathState& st, int depth, int round) { return st.wq_ctl + (size_t)(depth * (HK_WALK_ROUNDS + 1) + round) * 4; }   // {count A, cursor A, count B, cursor B}
// A global queue is written and read in wave-private CHUNKS: one atomic on the queue's count / cursor per chunk, not per push
// (the first version paid one atomic per refill round and push — 90 M same-address atomics per frame: the tracking half alone took
// longer than the whole unsplit walk).  A writer reserves HK_GQ_CHUNK entries at a time and pads what it leaves unused with
// HK_GQ_NONE, which readers skip; a reader takes chunks sized to the queue (n / (8 x waves), 64 ... 4096 entries).
#define HK_GQ_CHUNK 256
#define HK_GQ_NONE 0xffffffffu
struct GQOut {
    uint32_t* q;
    int* count;
    int base, used, cap;
};
HKD GQOut gq_out_open(uint32_t* q, int* count) { return GQOut{q, count, 0, 0, 0}; }
HKD void gq_out_pad(GQOut& o) {
    for (int i = o.used + lane_id(); i < o.cap; i += 64) o.q[o.base + i] = HK_GQ_NONE;
}
HKD void gq_out_push(GQOut& o, uint32_t value, bool active) {   // called by the whole wave
    const unsigned long long m = __ballot(active);
    const int k = __popcll(m);
    if (k == 0) return;
    if (o.used + k > o.cap) {
        gq_out_pad(o);
        int b = 0;
        if (lane_id() == 0) b = atomicAdd(o.count, HK_GQ_CHUNK);
        o.base = __builtin_amdgcn_readfirstlane(b);
        o.used = 0;
        o.cap = HK_GQ_CHUNK;
    }
    if (active) o.q[o.base + o.used + __popcll(m & ((1ull << lane_id()) - 1ull))] = value;
    o.used += k;
}
struct GQIn {
    const uint32_t* q;
    int* cursor;
    int n, lo, hi, chunk;
    bool more;
};
HKD GQIn gq_in_open(const uint32_t* q, int* cursor, int n) {
    int chunk = (n / (8 * physical_waves()) + 63) & ~63;
    chunk = chunk < 64 ? 64 : (chunk > 4096 ? 4096 : chunk);
    return GQIn{q, cursor, n, 0, 0, chunk, n > 0};
}
// the next entries of the wave's chunk for the lanes with `want` (lane rank r gets entry lo + r); -> false once the queue is used up
HKD bool gq_in_take(GQIn& in, bool want, uint32_t& value, bool& got) {
    got = false;
    while (in.lo >= in.hi && in.more) {
        int b = 0;
        if (lane_id() == 0) b = atomicAdd(in.cursor, in.chunk);
        b = __builtin_amdgcn_readfirstlane(b);
        if (b >= in.n)
            in.more = false;
        else {
            in.lo = b;
            in.hi = b + in.chunk < in.n ? b + in.chunk : in.n;
        }
    }
    if (in.lo >= in.hi) return false;
    const unsigned long long m = __ballot(want);
    const int rank = __popcll(m & ((1ull << lane_id()) - 1ull));
    const int avail = in.hi - in.lo, k = __popcll(m);
    if (want && rank < avail) {
        value = in.q[in.lo + rank];
        got = value != HK_GQ_NONE;
    }
    in.lo += k < avail ? k : avail;
    return true;
}

template <bool COUNT, int MM, int STACK>
__global__ void __launch_bounds__(HK_TRACE_BLOCK) k_walk_cast(DPathState st, DScene sc, int depth, int round, DStats* stats, const DMedium* __restrict__ media) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * STACK * 64];
    __shared__ float4 lds_box[3 * HK_MEDIA_NC];
    __shared__ int2 lds_child[HK_MEDIA_NC];
    __shared__ float4 lds_tri[3 * HK_MEDIA_NT];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    int* ctl = walk_ctl(st, depth, round);
    if (round > 0 && ctl[0] == 0) return;   // nothing was queued for this round (uniform: before the block's barrier)
    const NodeCache cache = scene_cache_fill<HK_MEDIA_NC, HK_MEDIA_NT, HK_TRACE_BLOCK>(sc, lds_box, lds_child, lds_tri);
    const int lane = lane_id();
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0;
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_SHADOW), true, depth, Q_SHADOW);
    uint32_t rec0 = 0;
    int n = 0, cursor = 0;
    GQIn in = gq_in_open(st.wq_a, &ctl[1], round > 0 ? ctl[0] : 0);
    GQOut out = gq_out_open(st.wq_b, &ctl[2]);
    for (;;) {
        // ---- the next 64 records ----
        uint32_t rec = 0;
        bool have = false;
        if (round == 0) {
            if (cursor >= n) {
                const int gw = stream_next(stream, st.n_waves);
                if (gw >= st.n_waves) break;
                rec0 = (uint32_t)gw * (uint32_t)st.wave_cap;
                n = *count_ptr(st, depth, Q_SHADOW, gw);
                cursor = 0;
                continue;
            }
            have = cursor + lane < n;
            rec = rec0 + (uint32_t)(cursor + lane);
            cursor += 64;
        } else if (!gq_in_take(in, true, rec, have))
            break;
        v3 ro = mk3(0, 0, 0), dir = mk3(0, 0, 1);
        float t_remaining = 0.0f, T_ray = 1.0f, tr_u = 1.0f, tr_l = 1.0f;
        int medium = -1, seg = 0;
        if (have) {
            const float4 O = st.sh_o[rec], D = st.sh_d[rec];
            ro = mk3(O.x, O.y, O.z);
            dir = mk3(D.x, D.y, D.z);
            t_remaining = O.w;
            medium = __float_as_int(D.w);
            if (round > 0) {
                const float4 Tq = st.sh_T[rec];
                T_ray = Tq.x, tr_u = Tq.y, tr_l = Tq.z;
                seg = (int)(st.sh_aux[rec] & 0xffu);
            }
        }
        bool active = have && !(t_remaining < 1e-6f);   // a degenerate ray is simply not visible
        // ---- casts; a ray that meets a surface outside every medium steps over it and casts again right here ----
        while (__ballot(active) != 0ull) {
            bool park = false;
            if (active) {
                bool opaque;
                ++n_casts;
                HitRec h = traverse<1, COUNT, HK_MEDIA_NC, HK_MEDIA_NT>(sc, ro, dir, t_remaining, stack, lane, n_nodes, n_tris, opaque, cache);
                bool alive = true, miss_case = true, transition = false;
                int next_medium = medium;
                float hit_t = t_remaining;
                if (h.prim >= 0) {
                    ++n_hits;
                    miss_case = false;
                    hit_t = h.t;
                    if (opaque)
                        alive = false;
                    else {
                        DTriMeta meta = sc.meta[h.prim];
                        DMediumInterface mi = sc.mis[meta.mi];
                        v3 ng = geometric_normal(sc, h.prim);
                        bool entering = dot(dir, ng) < 0.0f;
                        transition = mi.inside != mi.outside;
                        next_medium = transition ? (entering ? mi.inside : mi.outside) : medium;
                        if (!transition) {
                            float w = 1.0f - h.u - h.v;
                            float alpha = surface_alpha(sc, mi.material, uv_at(sc, h.prim, w, h.u, h.v));
                            bool pass = false;
                            if (alpha < 1.0f) {
                                PCG32 arng = pcg32_init(pbrt_hash(ro), pbrt_hash(dir));
                                pass = pcg32_f32(arng) > alpha;
                            }
                            alive = pass;
                        }
                    }
                }
                if (!alive)
                    active = false;  // blocked
                else if (medium >= 0) {
                    // ratio tracking over [0, hit_t] comes next: park the ray in its record
                    st.sh_o[rec] = make_float4(ro.x, ro.y, ro.z, t_remaining);
                    st.sh_d[rec] = make_float4(dir.x, dir.y, dir.z, __int_as_float(medium));
                    st.sh_T[rec] = make_float4(T_ray, tr_u, tr_l, hit_t);
                    st.sh_aux[rec] = (uint32_t)seg | (miss_case ? 0x100u : 0u) | (transition ? 0x200u : 0u) | ((uint32_t)(next_medium + 1) << 16);
                    // the tracker's per-ray set-up (majorant iterator: three divisions per axis; two 64-bit hashes for the PCG32 seed) is
                    // done HERE, where every lane of the wave has a ray, and handed over in the record: inside the tracking state
                    // machine it ran on the ~25 lanes of a refill round and cost as much as five collisions
                    const MajorantIter it = create_majorant_iterator<MM>(media[0], ro, dir, hit_t);
                    const PCG32 rng = pcg32_init(pbrt_hash(ro), pbrt_hash(dir));
                    float4* itp = st.sh_it + 4 * (size_t)rec;
                    itp[0] = make_float4(it.next_t[0], it.next_t[1], it.next_t[2], it.t_min);
                    itp[1] = make_float4(it.delta_t[0], it.delta_t[1], it.delta_t[2], it.t_max);
                    itp[2] = make_float4(__int_as_float(it.voxel[0]), __int_as_float(it.voxel[1]), __int_as_float(it.voxel[2]), __int_as_float(it.mode));
                    itp[3] = make_float4(__uint_as_float((uint32_t)rng.state), __uint_as_float((uint32_t)(rng.state >> 32)), __uint_as_float((uint32_t)rng.inc),
                                         __uint_as_float((uint32_t)(rng.inc >> 32)));
                    park = true;
                    active = false;
                } else if (miss_case) {
                    shadow_contribute<false>(st, rec, s4(T_ray), s4(tr_u), s4(tr_l));
                    active = false;
                } else {
                    // step over the surface (no medium on this side)
                    bool stop = false;
                    if (transition) {
                        if (T_ray == 0.0f) stop = true;
                        medium = next_medium;
                    }
                    ro = ro + dir * (hit_t + 1e-4f);
                    t_remaining = t_remaining - hit_t - 1e-4f;
                    ++seg;
                    active = !(stop || seg >= 10 || t_remaining < 1e-6f);
                }
            }
            gq_out_push(out, rec, park);
        }
    }
    gq_out_pad(out);
    stats += global_wave();
    wave_add(&stats->rays_shadow, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->sh_nodes, n_nodes);
        wave_add(&stats->sh_tris, n_tris);
    }
}

#ifndef HK_WALK_TRACK_WAVES
#define HK_WALK_TRACK_WAVES 5
#endif
template <int MM>
__global__ void __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(HK_WALK_TRACK_WAVES))) k_walk_track(DPathState st, DScene sc, int depth, int round, int tune, DStats* stats,
                                                                                                                               const DMedium* __restrict__ media) {
    int* ctl = walk_ctl(st, depth, round);
    int* ctl_next = walk_ctl(st, depth, round + 1);
    const int n = ctl[2];
    if (n == 0) return;
    const DMedium& med = media[0];   // GREY scenes hold one medium
    const float a0 = eval_flat(med.sigma_a), s0 = eval_flat(med.sigma_s);
    const S4 sigma_t = s4(a0 + s0);
    const int refill_idle = tune >> 24, adv_rounds = (tune >> 8) & 0xff, batches = tune & 0xff;
    unsigned n_coll = 0, n_dda = 0;
    HK_DBG_DECL
    GQIn in = gq_in_open(st.wq_b, &ctl[3], n);
    GQOut out = gq_out_open(st.wq_a, &ctl_next[0]);
    // per-lane state
    bool busy = false, in_seg = false, pending = false;
    uint32_t rec = 0;
    v3 ro = mk3(0, 0, 0), dir = mk3(0, 0, 1);
    float T_ray = 1.0f, tr_u = 1.0f, tr_l = 1.0f, hit_t = 0.0f, t_remaining = 0.0f;
    float sT = 1.0f, su = 1.0f, sl = 1.0f, sm0 = 0.0f, seg1 = 0.0f, t = 0.0f, pend_dt = 0.0f;
    uint32_t aux = 0;
    int k_in_seg = 0, segi = 0;
    MajorantIter it = exhausted_iter();
    PCG32 rng = PCG32{0ull, 0ull};
    for (;;) {
        // ---- refill ----
        const unsigned long long busy_m = __ballot(busy);
        const bool can_refill = in.more || in.lo < in.hi;
        if (busy_m == 0ull || (can_refill && 64 - __popcll(busy_m) >= refill_idle)) {
            if (!can_refill) break;
            uint32_t r_new = 0;
            bool got = false;
            gq_in_take(in, !busy, r_new, got);
            HK_DBG(5, got);
            if (got) {
                rec = r_new;
                const float4 O = st.sh_o[rec], D = st.sh_d[rec], Tq = st.sh_T[rec];
                aux = st.sh_aux[rec];
                ro = mk3(O.x, O.y, O.z);
                dir = mk3(D.x, D.y, D.z);
                t_remaining = O.w;
                T_ray = Tq.x, tr_u = Tq.y, tr_l = Tq.z, hit_t = Tq.w;
                sT = su = sl = 1.0f;
                {   // iterator and RNG as k_walk_cast set them up
                    const float4* itp = st.sh_it + 4 * (size_t)rec;
                    const float4 I0 = itp[0], I1 = itp[1], I2 = itp[2], I3 = itp[3];
                    it.next_t[0] = I0.x, it.next_t[1] = I0.y, it.next_t[2] = I0.z, it.t_min = I0.w;
                    it.delta_t[0] = I1.x, it.delta_t[1] = I1.y, it.delta_t[2] = I1.z, it.t_max = I1.w;
                    it.voxel[0] = __float_as_int(I2.x), it.voxel[1] = __float_as_int(I2.y), it.voxel[2] = __float_as_int(I2.z), it.mode = __float_as_int(I2.w);
                    rng.state = (uint64_t)__float_as_uint(I3.x) | ((uint64_t)__float_as_uint(I3.y) << 32);
                    rng.inc = (uint64_t)__float_as_uint(I3.z) | ((uint64_t)__float_as_uint(I3.w) << 32);
                }
                in_seg = false;
                pending = false;
                segi = 0;
                busy = true;
            }
            if (__ballot(busy) == 0ull) {
                if (!(in.more || in.lo < in.hi)) break;
                continue;
            }
        }
#pragma unroll 1
        for (int batch = 0; batch < batches; ++batch) {
            bool done = false;
            // ---- cheap steps until a tentative collision is pending: next majorant cell; free-flight sample inside a cell ----
#pragma unroll 1
            for (int adv = 0; adv < adv_rounds; ++adv) {
                const bool need = busy && !pending && !done;
                if (__ballot(need) == 0ull) break;
                HK_DBG(0, need);
                HK_DBG(1, need && !in_seg);
                HK_DBG(2, need && in_seg);
                if (need && !in_seg) {
                    float seg0;
                    S4 sm;
                    if (segi >= 256 || !majorant_next<MM>(it, med, sigma_t, seg0, seg1, sm))
                        done = true;
                    else {
                        ++segi;
                        ++n_dda;
                        sm0 = sm.x;
                        const bool enter = sm0 >= 1e-10f;
                        t = enter ? seg0 : t;
                        in_seg = enter;
                        k_in_seg = enter ? 0 : k_in_seg;
                    }
                }
                if (need && in_seg && !done) {   // in a cell with a non-zero majorant (also: just entered): the next tentative collision, or out through the cell's far side
                    const bool over = k_in_seg >= 100;
                    PCG32 r2 = rng;
                    const float u = pcg32_f32(r2);
                    rng = over ? rng : r2;
                    k_in_seg += over ? 0 : 1;
                    pend_dt = -media_logf(maxf(1e-10f, 1.0f - u)) / sm0;
                    const bool leave = over || (t + pend_dt >= seg1);   // T_maj / T_maj[1] = 1 at the boundary: nothing else changes
                    in_seg = !leave;
                    pending = !leave;
                }
            }
            // ---- the tentative collisions ----
            HK_DBG(3, busy && pending);
            HK_DBG(4, busy);
            if (busy && pending) {
                pending = false;
                const float dt = pend_dt;
                const float ts = t + dt;
                ++n_coll;
                const float d = sample_density<MM>(med, ro + dir * ts);
                const float sn0 = maxf(sm0 - a0 * d - s0 * d, 0.0f);
                const float Tm0 = media_expf((-dt) * sm0);
                const float pr = Tm0 * sm0;
                if (pr > 1e-10f) {
                    const float inv = 1.0f / pr;
                    sT = ((sT * Tm0) * sn0) * inv;
                    sl = ((sl * Tm0) * sm0) * inv;
                    su = ((su * Tm0) * sn0) * inv;
                    const float est = sT * (1.0f / maxf(1e-10f, average_flat(sl + su)));
                    if (est < 0.05f) {
                        const float rr = pcg32_f32(rng);
                        if (rr < 0.75f) {
                            sT = 0.0f;
                            done = true;
                        } else
                            sT = sT / (1.0f - 0.75f);
                    }
                    if (sT == 0.0f) done = true;
                    t = ts;
                } else {
                    sT = 0.0f;
                    done = true;
                }
            }
            // ---- the end of this medium segment ----
            bool requeue = false;
            if (busy && done) {
                busy = false;
                T_ray = T_ray * sT;
                tr_u = tr_u * su;
                tr_l = tr_l * sl;
                if (aux & 0x100u)   // the cast ended at the light: deliver
                    shadow_contribute<false>(st, rec, s4(T_ray), s4(tr_u), s4(tr_l));
                else {
                    int seg = (int)(aux & 0xffu);
                    int medium = 0;   // the ray was in the (only) medium
                    bool stop = false;
                    if (aux & 0x200u) {
                        if (T_ray == 0.0f) stop = true;
                        medium = (int)(aux >> 16) - 1;
                    }
                    ro = ro + dir * (hit_t + 1e-4f);
                    t_remaining = t_remaining - hit_t - 1e-4f;
                    ++seg;
                    if (!(stop || seg >= 10 || t_remaining < 1e-6f)) {
                        st.sh_o[rec] = make_float4(ro.x, ro.y, ro.z, t_remaining);
                        st.sh_d[rec] = make_float4(dir.x, dir.y, dir.z, __int_as_float(medium));
                        st.sh_T[rec] = make_float4(T_ray, tr_u, tr_l, 0.0f);
                        st.sh_aux[rec] = (uint32_t)seg;
                        requeue = true;
                    }
                }
            }
            gq_out_push(out, rec, requeue);
            if (__ballot(busy) == 0ull) break;
        }
    }
    gq_out_pad(out);
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->sh_collisions, n_coll);
    wave_add(&stats->sh_nvdb_collisions, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1 ? n_coll : 0u);
    wave_add(&stats->sh_dda_steps, n_dda);
}

#include "hk_film_kernels.h"

#include "hk_display.h"

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

#include "hk_table_kernels.h"

#include "hk_nvdb_build.h"
#include "hk_launch_impl.h"
#include "hk_test_kernels.h"
