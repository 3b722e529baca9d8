// hk_shadow.h — K10 of all-opaque scenes without media: shadow_contribute*, shadow_body and k_shadow (one any-hit cast per ray), and
// trace_shadow_body, which casts the shadow rays of a bounce and the closest hits of the next in one launch.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h and hk_traverse.h: lane_ray_start / lane_ray_round, node_cache_fill).
#pragma once

// ---------------------------------------------------------------------------------------------------
// K10: shadow rays (intersection.jl:302-406, 565-600).
//   k_shadow       scenes without media whose surfaces are all opaque: one any-hit cast per ray.
//   k_shadow_walk  the general walk through medium-transition / alpha surfaces (<= 10 segments) with ratio tracking
//                  (intersection.jl:422-542) in the medium segments.  Like k_track it is a per-lane state machine with
//                  wave-private refill: a lane alternates between "needs a cast" and "tracking steps", casts are done
//                  together for all lanes that need one, and finished lanes pull the next shadow ray of the wave's queue.
// ---------------------------------------------------------------------------------------------------
// rec: index of the shadow record (segment * wave_cap + position in the segment's shadow queue)
template <class W> HKD W wone();
template <> HKD float wone<float>() { return 1.0f; }
template <> HKD S4 wone<S4>() { return s4(1.0f); }
HKD S4 wide(S4 v) { return v; }
HKD S4 wide(float v) { return s4(v); }
HKD bool is_black(float v) { return v == 0.0f; }
template <bool COMPACT>
HKD void shadow_contribute(const DPathState& st, uint32_t rec, S4 T_ray, S4 tr_u, S4 tr_l) {
    if (is_black(T_ray)) return;
    S4 w_u, w_l;
    ld_shadow_weights<COMPACT>(st, rec, w_u, w_l);
    S4 mis = w_u * tr_u + w_l * tr_l;
    float den = average(mis);
    if (den > 1e-10f) {
        S4 fin = ld4(&st.sh_Ld[rec]) * T_ray / den;
        if (!is_black(fin)) {
            // (this read-modify-write of one path's 16 B costs k_shadow a quarter of its time in the Cornell box — 15.4 -> 11.4 ms per
            // frame without it; float atomics: 47 ms; non-temporal loads of the records around it, or the path slot read with the ray and
            // weights / Ld / L loaded together (one memory round trip instead of four): +-0 — it is the traffic, not the latency)
            const uint32_t pslot = st.sh_slot[rec];
            st4(&st.L[pslot], ld4(&st.L[pslot]) + fin);
        }
    }
}

// SLIM SHADOW RECORDS (round 6; DPathState::sh_final, opaque scenes without media).  Without media a shadow ray's transmittance and its two
// track weights are 1, so the denominator of what an unoccluded ray adds — average(w_u * 1 + w_l * 1) — is known when the record is
// written: k_shade forms it (shadow_contribute's operations in its order: the same bits) and stores it in the unused fourth word of sh_d;
// the two weights (8 B) are neither written nor read — a 56-byte record instead of 60 and one stream less in k_shadow, which still does
// the division.  (First version: the DIVISION in k_shade too and the path slot beside the direction, 48 B — k_shadow -9 %, but the four
// correctly rounded divisions cost k_shade<Matte> +0.8 ms per Cornell frame, as much as the bytes returned: LAB_NOTEBOOK.md round 6.)
HKD void shadow_contribute_final(const DPathState& st, uint32_t rec, float den) {
    if (den > 1e-10f) {
        const S4 fin = ld4(&st.sh_Ld[rec]) * s4(1.0f) / den;
        if (!is_black(fin)) {
            const uint32_t pslot = st.sh_slot[rec];
            st4(&st.L[pslot], ld4(&st.L[pslot]) + fin);
        }
    }
}
// the layout of the shadow weights is a run-time fact where grey media may or may not use the compact records (k_walk_pool)
HKD void shadow_contribute_rt(const DPathState& st, uint32_t rec, S4 T_ray, S4 tr_u, S4 tr_l) {
    if (st.compact)
        shadow_contribute<true>(st, rec, T_ray, tr_u, tr_l);
    else
        shadow_contribute<false>(st, rec, T_ray, tr_u, tr_l);
}

template <bool COUNT, int NC, bool QN = false>
__device__ __forceinline__ void shadow_body(const DPathState& st, const DScene& sc, int depth, DStats* stats, SegStream stream, int* __restrict__ stack, const NodeCache& cache) {
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int DONE = (int)0x80000000;
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0;
    HK_DBG_DECL
    uint32_t seg = 0;   // current segment's shadow records: entries seg .. seg + n - 1, streamed in order
    int n = 0, cursor = 0;
    bool more = true;
    bool have = false;
    uint32_t slot = 0;
    float rec_den = 0.0f;
    LaneRay r;
    r.cur = r.pend = DONE;
    for (;;) {
        const unsigned long long run_m = __ballot(have && r.cur != DONE);
        if (run_m == 0ull || (64 - __popcll(run_m) >= HK_TRACE_MIN_IDLE && (cursor < n || more))) {
            if (have && r.cur == DONE) {   // finished: an unoccluded shadow ray delivers its contribution
                if (r.best.prim < 0) {
                    if (st.sh_final)
                        shadow_contribute_final(st, slot, rec_den);
                    else
                        shadow_contribute<true>(st, slot, s4(1.0f), s4(1.0f), s4(1.0f));
                } else
                    ++n_hits;
                have = false;
            }
            while (more && cursor >= n) {   // this segment is used up: go on with the next one, the lanes in flight keep running
                const int gw = stream_next(stream, st.n_waves);
                if (gw >= st.n_waves) {
                    more = false;
                    break;
                }
                seg = (uint32_t)gw * (uint32_t)st.wave_cap;
                n = *count_ptr(st, depth, Q_SHADOW, gw);
                cursor = 0;
            }
            const unsigned long long want = __ballot(!have);
            const int avail = n - cursor;
            const int rank = __popcll(want & lt_mask);
            if (!have && rank < avail) {
                slot = seg + (uint32_t)(cursor + rank);
                float4 O = stream_ld(&st.sh_o[slot]), D = stream_ld(&st.sh_d[slot]);
                rec_den = D.w;   // (slim records: the denominator travels beside the direction)
                if (O.w >= 1e-6f) {   // a degenerate shadow ray is simply not visible
                    ++n_casts;
                    lane_ray_start<QN>(r, sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), O.w);
                    have = true;
                }
            }
            const int want_n = __popcll(want);
            cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
            if (__ballot(have) == 0ull) {
                if (cursor >= n && !more) break;
                continue;
            }
        }
#ifdef HK_DEBUG_UTIL
        HK_DBG(5, have && r.cur != DONE);      // rounds: lanes with a shadow ray in flight (probes 3 / 4: its node steps / leaf phases)
        lane_ray_round<true, COUNT, NC, HK_POSTPONE_ANYHIT != 0, false, QN>(r, have && r.cur != DONE, sc, stack, lane, n_nodes, n_tris, cache, cursor < n || more, dbg_ + 6);
#else
        lane_ray_round<true, COUNT, NC, HK_POSTPONE_ANYHIT != 0, false, QN>(r, have && r.cur != DONE, sc, stack, lane, n_nodes, n_tris, cache, cursor < n || more);
#endif
    }
    stats += global_wave();
    HK_DBG_FLUSH(stats);
    wave_add(&stats->rays_shadow, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->sh_nodes, n_nodes);
        wave_add(&stats->sh_tris, n_tris);
    }
}
template <bool COUNT, int STACK, int BLOCK = HK_TRACE_BLOCK, int NC = 0, bool QN = false>
__global__ void __launch_bounds__(BLOCK) k_shadow(DPathState st, DScene sc, int depth, DStats* stats) {
    __shared__ int lds_stack[(BLOCK / 64) * STACK * 64];
    __shared__ float4 lds_box[NC > 0 ? 3 * NC : 1];
    __shared__ int2 lds_child[NC > 0 ? NC : 1];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    const NodeCache cache = node_cache_fill<NC, BLOCK, QN>(sc, lds_box, lds_child);
    shadow_body<COUNT, NC, QN>(st, sc, depth, stats, stream_open(st, ticket_ptr(st, depth, TK_SHADOW), false, depth, Q_SHADOW), stack, cache);
}

// K10 of bounce `depth` and K2 of bounce `depth + 1` of ONE segment in one per-lane-refill loop (k_small_pass): after the shade stage
// the segment's shadow rays and its next generation of rays are both there and depend on nothing but it, so idle lanes take whichever is
// left (shadow records first) and the wave keeps twice the rays in flight — one drain instead of two, fuller rounds.  Per ray nothing
// changes: an any-hit ray ends at its first accepted triangle and delivers its contribution (shadow_body), a closest-hit ray is routed
// as trace_lean_body routes it; a path's L sees the same additions in the same order (its shadow ray of this bounce, then whatever
// bounce depth + 1 adds in the NEXT stage).
template <int NC>
__device__ __forceinline__ void trace_shadow_body(const DPathState& st, const DScene& sc, int depth, DStats* stats, int gw, int* __restrict__ stack, const NodeCache& cache) {
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int DONE = (int)0x80000000;
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0, n_sh_casts = 0;
    const int dt = depth + 1;
    const DPathGen g = gen_at(st, dt);
    const uint32_t seg = (uint32_t)gw * (uint32_t)st.wave_cap;
    const int n_ray = *count_ptr(st, dt, Q_RAY, gw), n_sh = *count_ptr(st, depth, Q_SHADOW, gw);
    WaveQ q_escaped = wq_open(st.escaped_q, st, gw);
    int kind_count[HK_MAX_KINDS];
#pragma unroll
    for (int k = 0; k < HK_MAX_KINDS; ++k) kind_count[k] = 0;
    int cur_ray = 0, cur_sh = 0;
    int state = LR_EMPTY;
    uint32_t slot = 0;
    float rec_den = 0.0f;
    LaneRay r;
    r.cur = r.pend = DONE;
    r.any = false;
    for (;;) {
        const unsigned long long run_m = __ballot(state == LR_ACTIVE && r.cur != DONE);
        if (run_m == 0ull || (64 - __popcll(run_m) >= HK_TRACE_MIN_IDLE && (cur_ray < n_ray || cur_sh < n_sh))) {
            int kind = -1;
            uint32_t eflag = 0u;   // HK_MATQ_EMISSIVE when the hit triangle carries an area light: travels in the kind-queue entry
            if (state == LR_ACTIVE && r.cur == DONE) {
                if (r.any) {   // a shadow ray: unoccluded, it delivers its contribution
                    if (r.best.prim < 0) {
                        if (st.sh_final)
                            shadow_contribute_final(st, slot, rec_den);
                        else
                            shadow_contribute<true>(st, slot, s4(1.0f), s4(1.0f), s4(1.0f));
                    } else
                        ++n_hits;
                } else if (r.best.prim < 0)
                    kind = -2;
                else {
                    ++n_hits;
                    const DTriMeta hm = sc.meta[r.best.prim];
                    eflag = hm.arealight > 0 ? HK_MATQ_EMISSIVE : 0u;
                    kind = classify_hit<true, false, true>(st, sc, slot, r.best, r.o, r.d, sc.mis[hm.mi].material, hm.arealight > 0);
                }
                state = LR_EMPTY;
            }
            wq_push(q_escaped, slot, kind == -2);
            kind_queues_push<true>(st, gw, kind, slot | eflag, __ballot(kind >= 0), lt_mask, kind_count);
            // ---- refill: the shadow records first, then the rays of the next bounce ----
            const unsigned long long want = __ballot(state == LR_EMPTY);
            const int avail_sh = n_sh - cur_sh, avail_ray = n_ray - cur_ray;
            const int rank = __popcll(want & lt_mask);
            if (state == LR_EMPTY) {
                if (rank < avail_sh) {
                    slot = seg + (uint32_t)(cur_sh + rank);
                    float4 O = stream_ld(&st.sh_o[slot]), D = stream_ld(&st.sh_d[slot]);
                    rec_den = D.w;
                    if (O.w >= 1e-6f) {   // a degenerate shadow ray is simply not visible
                        ++n_sh_casts;
                        lane_ray_start(r, sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), O.w);
                        r.any = true;
                        state = LR_ACTIVE;
                    }
                } else if (rank - avail_sh < avail_ray) {
                    slot = seg + (uint32_t)(cur_ray + rank - avail_sh);
                    float4 O = stream_ld(&g.ray_o[slot]), D = stream_ld(&g.ray_d[slot]);
                    ++n_casts;
                    lane_ray_start(r, sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), O.w);
                    state = LR_ACTIVE;
                }
            }
            const int want_n = __popcll(want);
            const int take_sh = want_n < avail_sh ? want_n : avail_sh;
            const int rest = want_n - take_sh;
            cur_sh += take_sh;
            cur_ray += rest < avail_ray ? rest : avail_ray;
            if (__ballot(state == LR_ACTIVE) == 0ull) {
                if (cur_ray >= n_ray && cur_sh >= n_sh) break;
                continue;   // (only degenerate shadow rays were drawn: draw again)
            }
        }
        lane_ray_round<false, false, NC, false, true>(r, state == LR_ACTIVE && r.cur != DONE, sc, stack, lane, n_nodes, n_tris, cache, cur_ray < n_ray || cur_sh < n_sh);
    }
    wq_close(q_escaped, count_ptr(st, dt, Q_ESCAPED, gw));
    if (lane == 0) {
        *count_ptr(st, dt, Q_MEDIUM, gw) = 0;
#pragma unroll
        for (int k = 0; k < HK_MAX_KINDS; ++k) *count_ptr(st, dt, Q_MAT0 + k, gw) = kind_count[k];
    }
    stats += global_wave();
    wave_add(&stats->rays_closest, n_casts);
    wave_add(&stats->rays_shadow, n_sh_casts);
    wave_add(&stats->hits, n_hits);
}
