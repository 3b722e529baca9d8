// hk_traverse.h — K3, closest-hit traversal and classification: the LDS cache fills, k_trace (scenes with media), the per-lane ray
// state machine (lane_ray_start / lane_ray_round), trace_lean_body and k_trace_lean.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h).
#pragma once

// Copies the first min(NC, sc.n_nodes) nodes into the block's LDS (see NodeCache) and waits for the whole block.
template <int NC, int BLOCK, bool QN = false>
HKD NodeCache node_cache_fill(const DScene& sc, float4* __restrict__ box, int2* __restrict__ child) {
    NodeCache c;
    c.box = (const lds_float4*)box, c.child = (const lds_int2*)child;
    c.tri = nullptr, c.nt = 0;
    c.nc = sc.n_nodes < NC ? sc.n_nodes : NC;
    if (NC > 0) {
        for (int i = threadIdx.x; i < c.nc; i += BLOCK) {
            if (QN) {   // quantised tree: the LDS copy holds the grid coordinates as floats (node_step's arithmetic is the same for both arms)
                const uint4* qp = reinterpret_cast<const uint4*>(sc.qnodes) + 2 * (size_t)i;
                const uint4 P = qp[0], Q = qp[1];
                box[i] = make_float4((float)(P.x & 0xffffu), (float)(P.x >> 16), (float)(P.y & 0xffffu), (float)(P.y >> 16));
                box[NC + i] = make_float4((float)(P.z & 0xffffu), (float)(P.z >> 16), (float)(P.w & 0xffffu), (float)(P.w >> 16));
                box[2 * NC + i] = make_float4((float)(Q.x & 0xffffu), (float)(Q.x >> 16), (float)(Q.y & 0xffffu), (float)(Q.y >> 16));
                child[i] = make_int2((int)Q.z, (int)Q.w);
                continue;
            }
            const float4* np = reinterpret_cast<const float4*>(sc.nodes) + 4 * (size_t)i;
            const float4 D = np[3];
            box[i] = np[0], box[NC + i] = np[1], box[2 * NC + i] = np[2];
            child[i] = make_int2(__float_as_int(D.x), __float_as_int(D.y));
        }
        __syncthreads();
    }
    return c;
}

// The scenes of the media kernels are often a handful of boxes (the cloud config: 24 triangles, 7 nodes): k_trace keeps the first NC
// nodes AND the first NT leaf triangles in LDS, so such a cast touches no global memory at all (cloud trace 87 -> 65 ms).  Not the
// shadow walk: the same cache inside k_shadow_walk cost it 28 % (its registers are full: 168 at 3 waves per SIMD).
#define HK_MEDIA_NC 64
#define HK_MEDIA_NT 80    // 32 KB of stacks + 7.25 KB of cache: 4 blocks per CU, as without it
template <int NC, int NT, int BLOCK>
HKD NodeCache scene_cache_fill(const DScene& sc, float4* __restrict__ box, int2* __restrict__ child, float4* __restrict__ tri) {
    NodeCache c = node_cache_fill<NC, BLOCK>(sc, box, child);
    c.tri = (const lds_float4*)tri;
    c.nt = sc.n_tris < NT ? sc.n_tris : NT;
    for (int i = threadIdx.x; i < c.nt; i += BLOCK) {
        const float4* tp = sc.leaf_tris + 3 * (size_t)i;
        tri[i] = tp[0], tri[NT + i] = tp[1], tri[2 * NT + i] = tp[2];
    }
    __syncthreads();
    return c;
}

// A kind-queue entry (DPathState::mat_q) for a hit whose mat_id word was stored earlier (the media kernels route hits that k_trace
// recorded): the generation index, with the emissive flag of mat_id in its top bit.
HKD uint32_t matq_entry(const DPathState& st, uint32_t slot) { return slot | ((st.mat_id[slot] & HK_MAT_EMISSIVE_BIT) != 0 ? HK_MATQ_EMISSIVE : 0u); }

// Classifies a fresh closest hit `h` of the ray (o, d) on a triangle of material `mat`: the final material kind, and the path's hit and
// mat_id records (STREAM: with streaming stores, as the lean kernels write them).  MixMaterial is resolved here so the queue is sorted by
// the *final* material kind.  MIX = false: the scene has no MixMaterial, and neither the resolve nor its tests are compiled in; SINGLE
// (with MIX = false): the kind is the scene's one kind, and the material record is not loaded for it.  For k_trace, trace_lean_body
// and trace_shadow_body.  (Hit and ray are passed BY VALUE: with `const HitRec&` the lean kernels came out with other registers.)
template <bool MIX, bool SINGLE, bool STREAM>
HKD int classify_hit(const DPathState& st, const DScene& sc, uint32_t slot, HitRec h, v3 o, v3 d, int mat, bool emissive) {
    if (MIX && sc.materials[mat].kind == HK_MAT_MIX) {
        float w = 1.0f - h.u - h.v;
        mat = resolve_mix_material(sc, mat, o + d * h.t, -d, uv_at(sc, h.prim, w, h.u, h.v));
    }
    int kind = SINGLE ? sc.single_kind : sc.materials[mat].kind;
    if (MIX && kind == HK_MAT_MIX) kind = HK_MAT_FALLBACK;
    if constexpr (STREAM) {
        stream_st(&st.hit[slot], make_float4(h.t, __int_as_float(h.prim), h.u, h.v));
        stream_st(reinterpret_cast<uint32_t*>(st.mat_id) + slot, (uint32_t)(mat | (emissive ? HK_MAT_EMISSIVE_BIT : 0)));
    } else {
        st.hit[slot] = make_float4(h.t, __int_as_float(h.prim), h.u, h.v);
        st.mat_id[slot] = mat | (emissive ? HK_MAT_EMISSIVE_BIT : 0);
    }
    return kind;
}
// Ballot-compacts the lanes with a hit (kind >= 0; `pending` is their ballot) into the segment's per-kind queues, one kind per turn:
// `entry` goes to queue `kind` behind the kind_count[kind] entries already there.  For k_trace (plain stores) and trace_shadow_body;
// trace_lean_body keeps the loop itself (see there).
template <bool STREAM>
HKD void kind_queues_push(const DPathState& st, int gw, int kind, uint32_t entry, unsigned long long pending, unsigned long long lt_mask, int (&kind_count)[HK_MAX_KINDS]) {
    while (pending) {
        int src = __ffsll((long long)pending) - 1;
        const int k = __builtin_amdgcn_readlane(kind, src);   // src is wave-uniform: the kind and every count below stay in scalar registers
        bool mine = kind == k;
        unsigned long long m = __ballot(mine);
        int cnt = 0;
#pragma unroll
        for (int kk = 0; kk < HK_MAX_KINDS; ++kk) cnt = (kk == k) ? kind_count[kk] : cnt;
        if (mine) {
            uint32_t* dst = &st.mat_q[((size_t)k * st.n_waves + gw) * st.wave_cap + cnt + __popcll(m & lt_mask)];
            if constexpr (STREAM)
                stream_st(dst, entry);
            else
                *dst = entry;
        }
        int add = __popcll(m);
#pragma unroll
        for (int kk = 0; kk < HK_MAX_KINDS; ++kk) kind_count[kk] += (kk == k) ? add : 0;
        pending &= ~m;
    }
}

// ---------------------------------------------------------------------------------------------------
// K3: closest-hit traversal + classification (intersection.jl:188-269).
// ---------------------------------------------------------------------------------------------------
template <bool COUNT>
__global__ void __launch_bounds__(HK_TRACE_BLOCK) k_trace(DPathState st, DScene sc, DTables T, DFrame fr, int depth, DStats* stats) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * HK_LDS_STACK * 64];
    __shared__ float4 lds_box[3 * HK_MEDIA_NC];
    __shared__ int2 lds_child[HK_MEDIA_NC];
    __shared__ float4 lds_tri[3 * HK_MEDIA_NT];
    int* stack = lds_stack + (threadIdx.x >> 6) * (HK_LDS_STACK * 64);
    const NodeCache cache = scene_cache_fill<HK_MEDIA_NC, HK_MEDIA_NT, HK_TRACE_BLOCK>(sc, lds_box, lds_child, lds_tri);
    const int lane = lane_id();
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0;
    HK_FOR_EACH_WAVE_SEGMENT(gw, st, ticket_ptr(st, depth, TK_TRACE), depth, Q_RAY) {
    const DPathGen g = gen_at(st, depth);
    const uint32_t seg = (uint32_t)gw * (uint32_t)st.wave_cap;   // the segment's live rays are entries seg .. seg + n - 1 of this generation
    const int n = *count_ptr(st, depth, Q_RAY, gw);
    WaveQ q_escaped = wq_open(st.escaped_q, st, gw);
    WaveQ q_medium = wq_open(st.medium_q, st, gw);
    int kind_count[HK_MAX_KINDS];
#pragma unroll
    for (int k = 0; k < HK_MAX_KINDS; ++k) kind_count[k] = 0;
    for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        bool active = i < n;
        uint32_t slot = seg + (uint32_t)(active ? i : 0);   // generation index of the path
        int kind = -1;  // -1 none, -2 escaped, >= 0 material kind
        bool in_medium = false;
        if (active && sc.n_media > 0 && (g.meta[slot].x >> 16) != 0u) {
            // ray travels inside a medium: one cast (no alpha test, intersection.jl:198-221), then delta tracking
            // (k_medium) decides whether the stored surface hit is ever reached
            in_medium = true;
            float4 O = g.ray_o[slot], D = g.ray_d[slot];
            bool dummy;
            ++n_casts;
            HitRec h = traverse<0, COUNT, HK_MEDIA_NC, HK_MEDIA_NT>(sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), O.w, stack, lane, n_nodes, n_tris, dummy, cache);
            if (h.prim >= 0) {
                ++n_hits;
                st.hit[slot] = make_float4(h.t, __int_as_float(h.prim), h.u, h.v);
                const DTriMeta hm = sc.meta[h.prim];
                st.mat_id[slot] = sc.mis[hm.mi].material | (hm.arealight > 0 ? HK_MAT_EMISSIVE_BIT : 0);
            } else
                st.hit[slot] = make_float4(INF_F, __int_as_float(-1), 0.0f, 0.0f);
        }
        wq_push(q_medium, slot, in_medium);
        if (active && !in_medium) {
            float4 O = g.ray_o[slot], D = g.ray_d[slot];
            v3 ro = mk3(O.x, O.y, O.z), rd = mk3(D.x, D.y, D.z);
            float tmax = O.w;
            // alpha-test loop: alpha-killed surfaces are skipped without consuming depth (<= 16 casts)
            for (int it = 0; it < 16; ++it) {
                bool dummy;
                ++n_casts;
                HitRec h = traverse<0, COUNT, HK_MEDIA_NC, HK_MEDIA_NT>(sc, ro, rd, it == 0 ? tmax : INF_F, stack, lane, n_nodes, n_tris, dummy, cache);
                if (h.prim < 0) {
                    kind = -2;
                    break;
                }
                ++n_hits;
                DTriMeta meta = sc.meta[h.prim];
                int mat = sc.mis[meta.mi].material;
                if (!sc.all_opaque) {
                    float w = 1.0f - h.u - h.v;
                    v2 uv = uv_at(sc, h.prim, w, h.u, h.v);
                    float alpha = surface_alpha(sc, mat, uv);
                    if (alpha < 1.0f) {
                        PCG32 rng = pcg32_init(pbrt_hash(ro), pbrt_hash(rd));
                        if (pcg32_f32(rng) > alpha) {
                            v3 pi = ro + rd * h.t;
                            v3 ng = geometric_normal(sc, h.prim);
                            v3 off = dot(rd, ng) > 0.0f ? ng : -ng;
                            ro = pi + off * 1e-4f;
                            continue;
                        }
                    }
                }
                kind = classify_hit<true, false, false>(st, sc, slot, h, ro, rd, mat, meta.arealight > 0);
                if (it > 0) g.ray_o[slot] = make_float4(ro.x, ro.y, ro.z, INF_F);  // origin after alpha skips
                if (meta.arealight > 0) slot |= HK_MATQ_EMISSIVE;   // the flag travels in the kind-queue entry (in `slot` itself: a register more costs this kernel its fourth wave; from here on `slot` is a queue ENTRY — it feeds the two pushes below and must not index anything)
                break;
            }
        }
        // ballot-compact into this wave's per-kind queue segments
        wq_push(q_escaped, slot, kind == -2);
        kind_queues_push<false>(st, gw, kind, slot, __ballot(kind >= 0), (1ull << lane) - 1ull, kind_count);
    }
    wq_close(q_escaped, count_ptr(st, depth, Q_ESCAPED, gw));
    wq_close(q_medium, count_ptr(st, depth, Q_MEDIUM, gw));
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < HK_MAX_KINDS; ++k) *count_ptr(st, depth, Q_MAT0 + k, gw) = kind_count[k];
    }
    }
    stats += global_wave();
    wave_add(&stats->rays_closest, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->nodes, n_nodes);
        wave_add(&stats->tris, n_tris);
    }
}

// ---------------------------------------------------------------------------------------------------
// K3 / K10 for scenes without media whose surfaces are all opaque (the common case): while-while traversal with wave-private
// dynamic fetch.  The step count per ray varies by 3-4x inside a wave of incoherent rays; instead of letting finished lanes
// idle until the slowest ray of the batch is done, a lane whose ray is finished keeps its result until the next flush, where
// results are classified / pushed with ballots and idle lanes pull the next rays of the wave's own queue segment.
// Same arithmetic and same per-ray result as traverse<>() (closest hit: min (t, prim); shadow: any hit).
// ---------------------------------------------------------------------------------------------------
// refill once this many lanes are idle: 12 was the optimum with pixel-tile waves; since a wave holds the samples of a few neighbouring
// pixels (rays that finish together more often) 24 - 32 is (many-light trace -4 %, shadow -3 %; flat from 24 to 40)
#ifndef HK_TRACE_MIN_IDLE
#define HK_TRACE_MIN_IDLE 24
#endif
// the closest-hit KERNEL of scenes whose tree sits in the 16-wave block's LDS cache (Cornell, sky: BVHs <= 16 deep) refills at 32 idle lanes —
// round 6, A B | B A on one box: k_trace_lean 34.45 -> 33.6 ms per Cornell frame (40: 34.15, 48: 35.4), sky 19.95 -> 19.65; the deep-tree
// instantiation of the 10^6-triangle scene keeps 24 (32: +1.2 %, 40: +2.6 %), and so do the any-hit kernel (32: +-0) and the small pass
#ifndef HK_CLOSEST_MIN_IDLE_LDS
#define HK_CLOSEST_MIN_IDLE_LDS 32
#endif
// leaf phases wait until this many lanes hold a leaf (0: never wait), as long as the kernel can still refill its idle lanes
#ifndef HK_ANYHIT_LEAF_MIN
#define HK_ANYHIT_LEAF_MIN 16
#endif
#ifndef HK_CLOSEST_LEAF_MIN
#define HK_CLOSEST_LEAF_MIN 0
#endif
// closest hit with the whole tree in LDS: the node loop of a round ends once A * (lanes still descending) < lanes waiting with a leaf
#ifndef HK_LEAF_BREAK_A
#define HK_LEAF_BREAK_A 2
#endif
// POSTPONED LEAVES (round 5; Aila & Laine's "speculative traversal").  A lane that reaches a leaf while its stack still holds nodes does
// not wait for the wave's next leaf phase: it keeps the leaf in `pend` and goes on descending from the popped node; only a lane that
// reaches a SECOND leaf (or has nothing left to descend) waits.  Node steps and leaf phases both run fuller; the price is one leaf's
// worth of stale t_best (a few more nodes visited).  The hit does not depend on the order in which leaves are tested (closest hit:
// minimum of (t, prim); any hit: whether one exists), so films are bit-identical (test_lean_traversal_parity, ab_bitwise.py).
// MEASURED AND SWITCHED OFF (interleaved on one box, films bit-identical): the stale t_best costs more node visits than the fuller phases
// return — Cornell trace +1.5 %, shadow +5 %; 10^6 triangles trace +7 %, shadow +4 %; sky trace +10 %.
#ifndef HK_POSTPONE_CLOSEST
#define HK_POSTPONE_CLOSEST 0
#endif
#ifndef HK_POSTPONE_ANYHIT
#define HK_POSTPONE_ANYHIT 0
#endif
#ifndef HK_NODE_UNROLL
#define HK_NODE_UNROLL 3   // node steps per evaluation of the node loop's exit rule (ballots, popcounts, the branch): 1 / 2 / 3 steps — Cornell trace 32.8 / 32.0 / 31.6 ms,
#endif                     // 10^6 triangles 0.531 / 0.518 / 0.517 s (interleaved on one box, films bit-identical); lanes that reach a leaf sit out the rest of the group
struct LaneRay {   // per-lane traversal state
    v3 o, d;
    RaySlab rs;
    float t_max;
    HitRec best;
    int cur, sp;
    int pend;   // a postponed leaf reference, or DONE (0x80000000) for none; cur == DONE implies pend == DONE
    bool any;   // lane_ray_round<.., MIXED>: this lane's ray is an any-hit (shadow) ray among closest-hit rays (trace_shadow_body)
};
template <bool QN = false>
HKD void lane_ray_start(LaneRay& r, const DScene& sc, v3 o, v3 d, float t_max) {
    r.o = o;
    r.d = d;
    r.t_max = t_max;
    r.best.t = t_max;
    r.best.prim = -1;
    r.best.u = r.best.v = 0.0f;
    r.rs = QN ? ray_slab_grid(sc, o, d) : ray_slab(o, d);
    r.sp = 0;
    r.cur = sc.n_tris == 0 ? (int)0x80000000 : sc.root_ref;
    r.pend = (int)0x80000000;
    r.any = false;
}
// one while-while round for the lanes with `active`: inner nodes until every such lane holds a leaf (or is done), then the leaves.
// ANYHIT: the first accepted triangle ends the ray (cur = DONE, best.prim >= 0).
// MIXED (with ANYHIT = false): closest-hit and any-hit rays share the wave, LaneRay::any says which a lane holds; the round's rules are the
// closest-hit kernel's, a lane's leaf test is its own kind's.
template <bool ANYHIT, bool COUNT, int NC = 0, bool POSTPONE = (ANYHIT ? HK_POSTPONE_ANYHIT != 0 : HK_POSTPONE_CLOSEST != 0), bool MIXED = false, bool QN = false>
HKD void lane_ray_round(LaneRay& r, bool active, const DScene& sc, int* __restrict__ stack, int lane, unsigned& n_nodes, unsigned& n_tris, const NodeCache& cache = NodeCache(),
                        bool may_wait = false
#ifdef HK_DEBUG_UTIL
                        , unsigned long long* dbg_ = nullptr
#endif
                        ) {
    const int DONE = (int)0x80000000;
    // ballots of ONE comparison each, combined as scalar masks: the ballot of a compound condition costs two VALU instructions
    // (v_cndmask + v_cmp) on top of the comparisons, and this loop is bound by instruction issue
    const unsigned long long act_m = __builtin_amdgcn_ballot_w64(active);
    // The rule that ends the node loop weighs what a leaf costs against a node step.  With the WHOLE tree in LDS (closest hit in the
    // Cornell box) a node step is cheap and the leaf phase — 46 % of the lanes under the 1 : 1 rule, up to four triangles each — is
    // where the lane-slots go: the nodes run on until they are outnumbered 2 : 1 (trace -5 %, frame +1.7 %).  Trees that reach into
    // global memory keep 1 : 1 (sky scene at 2 : 1: trace +1 %; 10^6 triangles: +3 %), and so does the any-hit kernel (+-0 either way).
    const int break_a = (!ANYHIT && NC > 0 && sc.n_nodes <= NC) ? HK_LEAF_BREAK_A : 1;
    for (;;) {
        const unsigned long long in_nodes = act_m & __builtin_amdgcn_ballot_w64(r.cur >= 0);
        if (in_nodes == 0ull) break;
        // stragglers: once fewer lanes are still descending than are waiting with a leaf, test the leaves first — the descending
        // lanes keep their state and go on in the next round.  (Running the node loop until the LAST lane holds a leaf cost
        // half of the traversal time in the 10^6-triangle scene: trace 0.94 -> 0.46 s, shadow 0.30 -> 0.19 s.)
        const int n_desc = __builtin_popcountll(in_nodes), n_leaf = __builtin_popcountll(act_m & __builtin_amdgcn_ballot_w64((unsigned)r.cur > 0x80000000u));   // cur < 0 and not DONE
        if (break_a * n_desc < n_leaf) break;
        // (ending the round here as soon as the caller's refill threshold is reached — rays that finish inside the node loop leave idle
        // lanes behind — fills the node steps better, 67 -> 72 % in the any-hit kernel, and still loses: the flush / refill it triggers
        // more often costs more than the lanes it feeds.  Cornell trace +7 %, shadow +9 %, 10^6 triangles +3 %.)
#ifdef HK_DEBUG_UTIL
        if (dbg_) HK_DBG(0, active && r.cur >= 0);          // node steps: lanes that descend
#endif
#pragma unroll
        for (int rep = 1; rep < HK_NODE_UNROLL; ++rep)
            if (active && r.cur >= 0) {
                if (COUNT) ++n_nodes;
                node_step<NC, QN>(sc, r.rs, r.best.t, stack, lane, r.cur, r.sp, cache);
            }
        if (active && r.cur >= 0) {
            if (COUNT) ++n_nodes;
            node_step<NC, QN>(sc, r.rs, r.best.t, stack, lane, r.cur, r.sp, cache);
            if (POSTPONE) {
                if (r.cur == DONE) {   // nothing left to descend: the postponed leaf (if any) is what is left of this ray
                    r.cur = r.pend;
                    r.pend = DONE;
                } else if (r.cur < 0 && r.pend == DONE && r.sp > 0) {   // a first leaf, and more to descend: postpone it
                    r.pend = r.cur;
                    --r.sp;
                    r.cur = stack[r.sp * 64 + lane];
                }
            }
        }
    }
    // The leaf phase is the expensive half of a round (up to four triangles), and it used to run for however few lanes held a leaf: in the
    // any-hit kernel, where most rays finish in the node loop without ever reaching one, 14 % of its lane-slots did work (HK_DEBUG_UTIL).
    // While the caller can still refill (`may_wait`), the few leaf holders now keep their leaf and wait: the caller's refill brings new
    // rays, and the leaves are tested once LEAF_MIN lanes hold one (Cornell: leaf phases 14 % -> 32 % full and 57 % fewer of them, k_shadow -5 %;
    // 8 or 20 instead of 16: no better).  (After the node loop either nothing descends or fewer lanes descend
    // than hold leaves: with fewer than LEAF_MIN <= 20 leaf holders at least 24 lanes are idle, so the refill is certain to happen.)
    constexpr int LEAF_MIN = ANYHIT ? (NC > 0 ? HK_ANYHIT_LEAF_MIN : 0) : HK_CLOSEST_LEAF_MIN;   // the deep-tree instantiations (NC == 0: 10^6 triangles) lose 1 % by waiting
    static_assert(LEAF_MIN == 0 || 64 - 2 * LEAF_MIN >= HK_TRACE_MIN_IDLE, "waiting leaf holders must leave enough idle lanes for the caller's refill to trigger");
    // (with postponed leaves the wait only looks at the lanes that are STUCK with a leaf in `cur`: the descending ones take their
    // postponed leaf along)
    if (LEAF_MIN > 0 && may_wait && __builtin_popcountll(act_m & __builtin_amdgcn_ballot_w64((unsigned)r.cur > 0x80000000u)) < LEAF_MIN) return;
    const bool has_pend = POSTPONE && r.pend != DONE;
#ifdef HK_DEBUG_UTIL
    if (dbg_) HK_DBG(1, active && (has_pend || (r.cur < 0 && r.cur != DONE)));   // leaf phase: lanes that hold a leaf
#endif
#ifdef HK_DEBUG_UTIL
    if (dbg_) {   // triangle iterations of the leaf phase: the wave runs max(count) of them, sum(count) lane-slots work (probe 6: closest hit, 7: any hit — an upper bound there)
        const bool holds = active && (has_pend || (r.cur < 0 && r.cur != DONE));
        int c = holds ? ((~(has_pend ? r.pend : r.cur)) & 7) + 1 : 0, mx = c, sm = c;
        for (int off = 32; off > 0; off >>= 1) {
            mx = max(mx, __shfl_xor(mx, off));
            sm += __shfl_xor(sm, off);
        }
        dbg_[ANYHIT ? 8 : 12] += 64ull * (unsigned)mx;
        dbg_[ANYHIT ? 9 : 13] += (unsigned)sm;
    }
#endif
    if (active && (has_pend || (r.cur < 0 && r.cur != DONE))) {
        int ref = ~(has_pend ? r.pend : r.cur);
        int first = ref >> 3, count = (ref & 7) + 1;
        bool stop = false;
        if (!ANYHIT && !MIXED) {
            // closest hit tests every triangle of the leaf, so the next one is fetched while this one is tested (trace -4 % in the
            // Cornell box, -2 % elsewhere); the any-hit loop below usually stops early and is better off without (shadow +1 %)
            const float4* tp = sc.leaf_tris + 3 * (size_t)first;
            float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
            for (int i = 0; i < count; ++i) {
                float4 N0 = T0, N1 = T1, N2 = T2;
                if (i + 1 < count) N0 = tp[3 * i + 3], N1 = tp[3 * i + 4], N2 = tp[3 * i + 5];
                asm volatile("" ::"v"(T0.x), "v"(T0.y), "v"(T0.z), "v"(T0.w));
                if (COUNT) ++n_tris;
                float t, u, v;
                if (intersect_triangle(r.o, r.d, r.t_max, mk3(T0.x, T0.y, T0.z), mk3(T1.x, T1.y, T1.z), mk3(T2.x, T2.y, T2.z), t, u, v)) {
                    int prim = __float_as_int(T0.w);
                    if (r.best.prim < 0 || t < r.best.t || (t == r.best.t && prim < r.best.prim)) {
                        r.best.t = t;
                        r.best.prim = prim;
                        r.best.u = u;
                        r.best.v = v;
                    }
                }
                T0 = N0, T1 = N1, T2 = N2;
            }
        } else
        for (int i = 0; i < count && !stop; ++i) {
            const float4* tp = sc.leaf_tris + 3 * (size_t)(first + i);
            float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
            // all three loads are issued here: left alone, the compiler sinks the v0 load behind the det != 0 test and
            // every triangle pays a second memory round trip
            asm volatile("" ::"v"(T0.x), "v"(T0.y), "v"(T0.z), "v"(T0.w));
            if (COUNT) ++n_tris;
            float t, u, v;
            if (intersect_triangle(r.o, r.d, r.t_max, mk3(T0.x, T0.y, T0.z), mk3(T1.x, T1.y, T1.z), mk3(T2.x, T2.y, T2.z), t, u, v)) {
                int prim = __float_as_int(T0.w);
                if (MIXED ? r.any : ANYHIT) {
                    r.best.t = t;
                    r.best.prim = prim;
                    stop = true;
                } else if (r.best.prim < 0 || t < r.best.t || (t == r.best.t && prim < r.best.prim)) {
                    r.best.t = t;
                    r.best.prim = prim;
                    r.best.u = u;
                    r.best.v = v;
                }
            }
        }
        if (stop) {
            r.cur = DONE;
            if (POSTPONE) r.pend = DONE;
        } else if (has_pend)
            r.pend = DONE;   // (cur — a node to descend, or a second leaf for the next phase — stays)
        else if (r.sp > 0) {
            --r.sp;
            r.cur = stack[r.sp * 64 + lane];
        } else
            r.cur = DONE;
    }
}

enum { LR_EMPTY = 0, LR_ACTIVE = 1 };

// STACK: LDS stack entries per lane.  The stack holds at most one entry per inner level, so a BVH of depth <= 16 (every scene
// but the 10^6-triangle one) runs with half the LDS: 16 KB per block instead of 32, and LDS stops limiting residency.
// MIX = false: the scene has no MixMaterial (DScene::has_mix), and the flush carries neither the resolve (texture lookup, hashes, uv
// interpolation) nor its tests — registers and scheduling of a branch never taken.
// SINGLE (with MIX = false): every material of the scene is of ONE kind (DScene::single_kind, uniform): the flush does not load the
// material record for its kind and pushes to that kind's queue in one step, with one count; hit, mat_id and the queue entries
// (order, emissive flag) are written as by the general flush.
template <bool COUNT, int NC, bool QN = false, int MIN_IDLE = HK_TRACE_MIN_IDLE, bool MIX = true, bool SINGLE = false>
__device__ __forceinline__ void trace_lean_body(const DPathState& st, const DScene& sc, int depth, DStats* stats, const SegTickets& src, int* __restrict__ stack, const NodeCache& cache) {
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int DONE = (int)0x80000000;
    unsigned n_nodes = 0, n_tris = 0, n_casts = 0, n_hits = 0;
    HK_DBG_DECL
    HK_FOR_EACH_SEGMENT_FROM(gw, st, src) {
    const DPathGen g = gen_at(st, depth);
    const uint32_t seg = (uint32_t)gw * (uint32_t)st.wave_cap;   // the rays of this segment: entries seg .. seg + n - 1, read in order (no index queue)
    const int n = *count_ptr(st, depth, Q_RAY, gw);
    WaveQ q_escaped = wq_open(st.escaped_q, st, gw);
    static_assert(!(SINGLE && MIX), "a scene with a MixMaterial is not a single-kind scene");
    int kind_count[HK_MAX_KINDS];
#pragma unroll
    for (int k = 0; k < HK_MAX_KINDS; ++k) kind_count[k] = 0;
    int one_count = 0;   // SINGLE: the entries of the one kind's queue
    int cursor = 0;
    int state = LR_EMPTY;
    uint32_t slot = 0;
    LaneRay r;
    r.cur = r.pend = DONE;
    for (;;) {
        const unsigned long long run_m = __ballot(state == LR_ACTIVE && r.cur != DONE);
        if (run_m == 0ull || (64 - __popcll(run_m) >= MIN_IDLE && cursor < n)) {
            // ---- flush: classify the finished rays, push them to the escaped / material-kind queues ----
            HK_DBG(8, state == LR_ACTIVE && r.cur == DONE);   // flushes: lanes that deliver a finished ray
            int kind = -1;
            uint32_t eflag = 0u;   // HK_MATQ_EMISSIVE when the hit triangle carries an area light: travels in the kind-queue entry
            if (state == LR_ACTIVE && r.cur == DONE) {
                if (r.best.prim < 0) {
                    kind = -2;
                    // SINGLE: k_shade may walk the generation by slot instead of through the kind queue — the entry says that it holds no hit
                    if constexpr (SINGLE) stream_st(reinterpret_cast<uint32_t*>(st.mat_id) + slot, HK_MAT_ESCAPED);
                } else {
                    ++n_hits;
                    const DTriMeta hm = sc.meta[r.best.prim];
                    eflag = hm.arealight > 0 ? HK_MATQ_EMISSIVE : 0u;
                    kind = classify_hit<MIX, SINGLE, true>(st, sc, slot, r.best, r.o, r.d, sc.mis[hm.mi].material, hm.arealight > 0);
                }
                state = LR_EMPTY;
            }
            wq_push(q_escaped, slot, kind == -2);
            unsigned long long pending = __ballot(kind >= 0);
            if (SINGLE) {   // what the loop below does in its one turn when every hit is of the same kind
                if (kind >= 0) stream_st(&st.mat_q[((size_t)sc.single_kind * st.n_waves + gw) * st.wave_cap + one_count + __popcll(pending & lt_mask)], slot | eflag);
                one_count += __popcll(pending);
                pending = 0ull;
            }
            while (pending) {   // kind_queues_push<true>, kept as a copy: with the call the HK_DEBUG_UTIL build of this body allocates its registers differently
                int src = __ffsll((long long)pending) - 1;
                const int k = __builtin_amdgcn_readlane(kind, src);   // src is wave-uniform: the kind and every count below stay in scalar registers
                bool mine = kind == k;
                unsigned long long m = __ballot(mine);
                int cnt = 0;
#pragma unroll
                for (int kk = 0; kk < HK_MAX_KINDS; ++kk) cnt = (kk == k) ? kind_count[kk] : cnt;
                if (mine) stream_st(&st.mat_q[((size_t)k * st.n_waves + gw) * st.wave_cap + cnt + __popcll(m & lt_mask)], slot | eflag);
                int add = __popcll(m);
#pragma unroll
                for (int kk = 0; kk < HK_MAX_KINDS; ++kk) kind_count[kk] += (kk == k) ? add : 0;
                pending &= ~m;
            }
            // ---- refill ----
            const unsigned long long want = __ballot(state == LR_EMPTY);
            const int avail = n - cursor;
            const int rank = __popcll(want & lt_mask);
            if (state == LR_EMPTY && rank < avail) {
                slot = seg + (uint32_t)(cursor + rank);
                float4 O = ld_ray_o(st, g, slot, depth, seg), D = stream_ld(&g.ray_d[slot]);
                ++n_casts;
                lane_ray_start<QN>(r, sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), O.w);
                state = LR_ACTIVE;
            }
            const int want_n = __popcll(want);
            cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
            if (__ballot(state == LR_ACTIVE) == 0ull) break;
        }
#ifdef HK_DEBUG_UTIL
        HK_DBG(2, state == LR_ACTIVE && r.cur != DONE);      // rounds: lanes with a ray in flight
        lane_ray_round<false, COUNT, NC, HK_POSTPONE_CLOSEST != 0, false, QN>(r, state == LR_ACTIVE && r.cur != DONE, sc, stack, lane, n_nodes, n_tris, cache, cursor < n, dbg_);
#else
        lane_ray_round<false, COUNT, NC, HK_POSTPONE_CLOSEST != 0, false, QN>(r, state == LR_ACTIVE && r.cur != DONE, sc, stack, lane, n_nodes, n_tris, cache, cursor < n);
#endif
    }
    wq_close(q_escaped, count_ptr(st, depth, Q_ESCAPED, gw));
    if (lane == 0) {
        *count_ptr(st, depth, Q_MEDIUM, gw) = 0;
#pragma unroll
        for (int k = 0; k < HK_MAX_KINDS; ++k) *count_ptr(st, depth, Q_MAT0 + k, gw) = SINGLE ? (k == sc.single_kind ? one_count : 0) : kind_count[k];
    }
    }
    stats += global_wave();
    wave_add(&stats->rays_closest, n_casts);
    wave_add(&stats->hits, n_hits);
    if (COUNT) {
        wave_add(&stats->nodes, n_nodes);
        wave_add(&stats->tris, n_tris);
    }
    HK_DBG_FLUSH(stats);
}
template <bool COUNT, int STACK, int BLOCK = HK_TRACE_BLOCK, int NC = 0, bool QN = false, bool MIX = true, bool SINGLE = false>
__global__ void __launch_bounds__(BLOCK) k_trace_lean(DPathState st, DScene sc, int depth, DStats* stats) {
    __shared__ int lds_stack[(BLOCK / 64) * STACK * 64];
    __shared__ float4 lds_box[NC > 0 ? 3 * NC : 1];
    __shared__ int2 lds_child[NC > 0 ? NC : 1];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    const NodeCache cache = node_cache_fill<NC, BLOCK, QN>(sc, lds_box, lds_child);
    trace_lean_body<COUNT, NC, QN, (NC >= 1024 ? HK_CLOSEST_MIN_IDLE_LDS : HK_TRACE_MIN_IDLE), MIX, SINGLE>(st, sc, depth, stats, seg_open(st, ticket_ptr(st, depth, TK_TRACE), st.dynamic_segments != 0, depth, Q_RAY), stack, cache);
}
