// hk_track.h — K4-K6, the paths inside a medium: classify_survivor and TrackSeg, the delta-tracking state machines k_track, k_track_flat and
// k_track_pool with their knobs, k_scatter and k_detect_camera_medium.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h and hk_traverse.h: SegStream, the segment tickets, trace_closest).
#pragma once

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
    // open_seg / close_seg, the routing loop and the next-segment loop below are k_track's, kept as copies: as TrackSeg members and functions of (st, seg[2], state, tag, ...) every k_track and k_track_flat gets another register allocation
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
        // phases A and B are k_track_flat's, kept as copies: with the lane state in a struct, or phase B as a function of references to these locals, both kernels get another register allocation
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
