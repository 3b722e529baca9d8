// hk_shadow_walk.h — K10 of scenes with media or non-opaque surfaces: k_shadow_walk, its LDS-pool form k_walk_pool, and the two-kernel
// form k_walk_cast / k_walk_track, with their knobs.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h, hk_traverse.h, hk_track.h: HK_MEDIA_WAVES, HK_TRACK_ADVANCE; hk_shadow.h: wone, wide, shadow_contribute*).
#pragma once

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

// the statistics of a wave that casts and tracks (k_shadow_walk, k_walk_pool), into its row
template <bool COUNT>
HKD void walk_stats_add(DStats* stats, bool nvdb, unsigned n_coll, unsigned n_dda, unsigned n_casts, unsigned n_hits, unsigned n_nodes, unsigned n_tris) {
    wave_add(&stats->sh_collisions, n_coll);
    wave_add(&stats->sh_nvdb_collisions, nvdb ? n_coll : 0u);
    wave_add(&stats->sh_dda_steps, n_dda);
    wave_add(&stats->rays_shadow, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->sh_nodes, n_nodes);
        wave_add(&stats->sh_tris, n_tris);
    }
}

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
                        } else {   // the step over the surface, as after a cast above; kept as a copy: as a lambda or a function all 28 instantiations change
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
    walk_stats_add<COUNT>(stats, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1, n_coll, n_dda, n_casts, n_hits, n_nodes, n_tris);
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
            // the grey collision of k_shadow_walk<.., GREY> and k_walk_track, kept as a copy: one function for the three changes the register numbering of all of them
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
    walk_stats_add<COUNT>(stats, (sc.media_mask >> HK_MEDIUM_NANOVDB) & 1, n_coll, n_dda, n_casts, n_hits, n_nodes, n_tris);
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
                // what the hit means is k_shadow_walk's block, kept as a copy: as one function (returning alive, or with out-references) every k_shadow_walk with media and every k_walk_cast changes
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
                // the grey collision of k_shadow_walk<.., GREY> and k_walk_pool, kept as a copy (see k_walk_pool)
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
