// hk_shade.h — K7 and K8 + K9 + K11: k_escaped, the light preselection (k_light_select, k_light_select_pool), shade_body and k_shade.
// Part of the hk_kernels.hip translation unit (needs hk_wave_queues.h).
#pragma once

// ---------------------------------------------------------------------------------------------------
// K7: escaped rays (intersection.jl:622-678; lights.jl:408-467).  MIS uses 1/num_lights (Q6).
// ---------------------------------------------------------------------------------------------------
// one escaped path: what it adds to its L (false: nothing)
__device__ __forceinline__ bool escaped_one(const DPathState& st, const DScene& sc, const DTables& T, const DPathGen& g, bool ones, uint32_t slot, S4& fin, uint32_t& pslot, int depth) {
    const uint2 meta = ld_meta(st, g, slot, depth);
    pslot = meta.y;
    S4 lambda = ld_lambda(st, g, slot, meta.y);
    S4 Le = s4(0.0f);
    v3 rd = mk3(0, 0, 1);
    bool have_dir = false;
    for (int li = 0; li < sc.n_lights; ++li) {
        const DLight& l = sc.lights[li];
        if (l.kind == HK_LIGHT_AMBIENT) Le = Le + l.scale * light_spectrum(l, lambda);
        if (l.kind == HK_LIGHT_ENVIRONMENT) {  // bilinear env(dir) * scale, illuminant uplift (lights.jl:408-419)
            if (!have_dir) {
                float4 D = g.ray_d[slot];
                rd = mk3(D.x, D.y, D.z);
                have_dir = true;
            }
            float4 t = env_eval(sc.envmaps[l.Le_tex], rd);
            Le = Le + eval_illuminant(coef_illuminant(T, t.x * l.Le_rgba[0], t.y * l.Le_rgba[1], t.z * l.Le_rgba[2]), lambda);
        }
    }
    S4 beta = ld_throughput(g.beta, slot, ones);
    S4 contribution = beta * Le;
    if (is_black(contribution)) return false;
    uint32_t fl = meta.x;
    int pdepth = (int)(fl & 0xff);
    bool specular = (fl >> 8) & 1u;
    S4 r_u = ld_ru(g, slot, ones, st.compact != 0);
    if (pdepth == 0 || specular)
        fin = contribution / average(r_u);
    else {
        float choice = sc.n_lights > 0 ? 1.0f / (float)sc.n_lights : 0.0f;
        float light_pdf = 0.0f;  // only EnvironmentLight has a pdf (lights.jl:445-467)
        if (sc.n_envmaps > 0)
            for (int li = 0; li < sc.n_lights; ++li) {
                const DLight& l = sc.lights[li];
                light_pdf = light_pdf + (l.kind == HK_LIGHT_ENVIRONMENT ? env_pdf_li(sc.envmaps[l.Le_tex], rd) : 0.0f);
            }
        S4 rl = ld_rl(g, slot, ones, st.compact != 0) * choice * light_pdf;
        float den = average(r_u + rl);
        fin = den > 1e-10f ? contribution / den : contribution / average(r_u);
    }
    return true;
}
// UNROLL = 2 (round 6): a lane carries TWO queue entries through the chain of dependent loads (queue entry -> record -> environment texels ->
// spectrum table -> L) at once.  The kernel spends 0.81 of its wave time parked at s_waitcnt (profiles/r05_wavestate_sky.txt) with one
// entry per lane in flight; the two are different paths, so their additions to L do not meet and the film is the same bit for bit.
template <int UNROLL>
__device__ __forceinline__ void escaped_body(const DPathState& st, const DScene& sc, const DTables& T, int depth, int implicit_ones, const SegTickets& src) {
    HK_FOR_EACH_SEGMENT_FROM(gw, st, src) {
    const uint32_t* __restrict__ queue = st.escaped_q + (size_t)gw * st.wave_cap;
    const int n = *count_ptr(st, depth, Q_ESCAPED, gw);
    const DPathGen g = gen_at(st, depth);
    const bool ones = depth == 0 && implicit_ones;
    int i = lane_id();
    if (UNROLL == 2) {
        for (; i + 64 < n; i += 128) {
            const uint32_t slot0 = queue[i], slot1 = queue[i + 64];
            S4 fin0, fin1;
            uint32_t p0, p1;
            const bool a0 = escaped_one(st, sc, T, g, ones, slot0, fin0, p0, depth);
            const bool a1 = escaped_one(st, sc, T, g, ones, slot1, fin1, p1, depth);
            S4 L0 = s4(0.0f), L1 = s4(0.0f);
            if (a0) L0 = ld4(&st.L[p0]);
            if (a1) L1 = ld4(&st.L[p1]);
            if (a0) st4(&st.L[p0], L0 + fin0);
            if (a1) st4(&st.L[p1], L1 + fin1);
        }
    }
    for (; i < n; i += 64) {
        S4 fin;
        uint32_t pslot;
        if (escaped_one(st, sc, T, g, ones, queue[i], fin, pslot, depth)) st4(&st.L[pslot], ld4(&st.L[pslot]) + fin);
    }
    }
}
template <int UNROLL>
__global__ void __launch_bounds__(256) k_escaped(DPathState st, DScene sc, DTables T, int depth, int implicit_ones) {
    escaped_body<UNROLL>(st, sc, T, depth, implicit_ones, seg_open(st, ticket_ptr(st, depth, TK_ESCAPED), st.dynamic_segments != 0, depth, Q_ESCAPED));
}

// ---------------------------------------------------------------------------------------------------
// K8 + K9 + K11 fused per material kind (surface-eval.jl:147-220, 250-341, 396-512).
// ---------------------------------------------------------------------------------------------------
// Register budget: 512 VGPRs per SIMD lane => 3 waves/SIMD need <= 168, 4 need <= 128.  The simple kinds sit a few registers
// above 168 without a hint; asking for 3 waves costs a handful of scratch spills and buys a third more latency hiding.
// The walk kinds (coated diffuse / transmission) are far above: they keep the default.
// ---------------------------------------------------------------------------------------------------
// Light selection of K9 as its own kernel, for scenes with a deep light BVH (DScene::num_bvh_lights >= HK_PRESELECT_MIN, no media).
// A descent of bvh_sample_light (bvh-light-sampler.jl:105-170) takes as many levels as the chosen light's leaf is deep — 12 to 25 in
// the 5*10^4-light scene — and inside k_shade every lane of a wave waits for the deepest: 49 % of the lanes active.  Here each
// lane is a little state machine (like the traversal kernels'): one level per round for the lanes that descend, finished lanes keep
// their result until enough of them wait (HK_SELECT_MIN_IDLE = 24: 8 / 16 / 24 / 32 idle lanes give 0.78 / 0.72 / 0.69 / 0.70 s of shading per
// 512-spp frame; computing the inputs in a dense pre-pass changed nothing), then write it and pull the next shading vertices of the segment — the
// entries of its per-kind queues, one kind after the other.  Same arithmetic per vertex as the fused form: position and shading normal
// from surface_at, the sample from dimension base + 1, node_importance in the same order; the result (light, pmf) goes to sel_light[entry].
// ---------------------------------------------------------------------------------------------------
#define HK_PRESELECT_MIN 64
#ifndef HK_SELECT_MIN_IDLE
#define HK_SELECT_MIN_IDLE 24
#endif
template <bool FT>
__global__ void __launch_bounds__(256) k_light_select(DPathState st, DScene sc, DTables T, DFrame fr, DSobol sob, int depth, uint32_t kinds_mask, int min_idle, DStats* stats) {
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_lnodes = 0;
    const DPathGen g = gen_at(st, depth);
    const int base_dim = 6 + 7 * depth;
    const int ninf = sc.num_infinite_lights, nbvh = sc.num_bvh_lights;
    const bool has_bvh = nbvh > 0;
    const float p_inf = (float)ninf / (float)(ninf + (has_bvh ? 1 : 0));
    HK_FOR_EACH_WAVE_SEGMENT(gw, st, ticket_ptr(st, depth, TK_SELECT), depth, Q_RAY) {
        int kind = -1, n = 0, cursor = 0;
        const uint32_t* __restrict__ queue = st.mat_q;
        bool more = true;
        // per-lane descent state
        bool busy = false, done = false;
        uint32_t slot = 0, bits = 0, child = 0;
        int ni = 1, res_light = 0, lvl = 0;
        float ub = 0.0f, pmf = 0.0f, res_pmf = 0.0f;
        v3 p = mk3(0, 0, 0), nn = mk3(0, 0, 1);
        for (;;) {
            const unsigned long long run_m = __ballot(busy && !done);
            if (run_m == 0ull || (64 - __popcll(run_m) >= min_idle && (cursor < n || more))) {
                if (busy && done) {
                    st.sel_light[slot] = make_uint2((uint32_t)res_light, __float_as_uint(res_pmf));
                    busy = false;
                }
                while (more && cursor >= n) {   // the next kind present in the scene that has entries in this segment
                    ++kind;
                    while (kind < HK_MAX_KINDS && !(kinds_mask & (1u << kind))) ++kind;
                    if (kind >= HK_MAX_KINDS) {
                        more = false;
                        break;
                    }
                    queue = st.mat_q + ((size_t)kind * st.n_waves + gw) * st.wave_cap;
                    n = *count_ptr(st, depth, Q_MAT0 + kind, gw);
                    cursor = 0;
                }
                const unsigned long long want = __ballot(!busy);
                const int avail = n - cursor;
                const int rank = __popcll(want & lt_mask);
                if (!busy && rank < avail) {
                    slot = queue[cursor + rank] & ~HK_MATQ_EMISSIVE;
                    const float4 H = st.hit[slot], O = ld_ray_o(st, g, slot, depth, (size_t)gw * st.wave_cap), D = g.ray_d[slot];
                    const Surface sf = surface_at(sc, __float_as_int(H.y), H.z, H.w, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), H.x);
                    p = sf.pi;
                    nn = sf.ns;
                    int pix, k;
                    split_slot(fr, ld_meta(st, g, slot, depth).y, pix, k);
                    const SobolCtx sctx = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix, k, fr.first_sample + k * fr.sample_stride);
                    const float u = sobol_1d<FT>(sctx, base_dim + 1);
                    // bvh_sample_light's prologue: the infinite lights, then the root
                    busy = true;
                    done = true;
                    res_light = 0;
                    res_pmf = 0.0f;
                    if (ninf + nbvh > 0) {
                        if (ninf > 0 && u < p_inf) {
                            const float ur = u / p_inf;
                            int idx = (int)floorf(ur * (float)ninf);
                            idx = (idx < ninf - 1 ? idx : ninf - 1) + 1;
                            res_pmf = p_inf / (float)ninf;
                            res_light = sc.infinite_lights[idx - 1];
                        } else if (has_bvh) {
                            ub = ninf > 0 ? minf((u - p_inf) / (1.0f - p_inf), 0.99999994f) : minf(u, 0.99999994f);
                            pmf = 1.0f - p_inf;
                            ni = 1;
                            const DLightNode root = load_light_node(sc.lnodes, 0);
                            bits = root.bits, child = root.child1_or_light;
                            lvl = 0;
                            done = false;
                        }
                    }
                }
                const int want_n = __popcll(want);
                cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
                if (__ballot(busy) == 0ull) {
                    if (cursor >= n && !more) break;
                    continue;
                }
            }
            // ---- one level of the descent for the lanes that are on their way ----
            if (busy && !done) {
                if (lvl >= 64) {   // the reference gives up after 64 levels (bvh-light-sampler.jl:126)
                    res_light = 0;
                    res_pmf = 0.0f;
                    done = true;
                } else if (bits & 2u) {
                    res_pmf = pmf;
                    res_light = (int)child;
                    done = true;
                } else {
                    ++lvl;
                    const DLightNode n0 = load_light_node(sc.lnodes, (int)child), n1 = load_light_node(sc.lnodes, (int)child + 1);
                    const float c0 = node_importance(n0, p, nn);
                    const float c1 = node_importance(n1, p, nn);
                    n_lnodes += 2;
                    if (c0 == 0.0f && c1 == 0.0f) {
                        res_light = 0;
                        res_pmf = 0.0f;
                        done = true;
                    } else {
                        const float p0 = c0 / (c0 + c1);
                        if (ub < p0) {
                            pmf *= p0;
                            ub = ub / p0;
                            bits = n0.bits, child = n0.child1_or_light;
                        } else {
                            pmf *= (1.0f - p0);
                            ub = (ub - p0) / (1.0f - p0);
                            bits = n1.bits, child = n1.child1_or_light;
                        }
                    }
                }
            }
        }
    }
    stats += global_wave();
    wave_add(&stats->light_nodes, n_lnodes);
}

// ---------------------------------------------------------------------------------------------------
// k_light_select re-shaped around a per-wave POOL in LDS (round 5; the round-4 re-shape of the cloud's tracking kernels carried over).
// The per-lane-refill kernel above ran its descent rounds 70 % full: finished lanes waited for 24 of their kind, and the per-vertex
// SET-UP (hit record, surface_at, the Sobol draw, the infinite-light prologue) ran for those ~25 lanes only.  Here
//   * the set-up runs for 64 queue entries AT ONCE whenever the pool is empty and a lane is free; vertices that need a descent leave
//     (entry, p, n, u_bvh) — 8 words — in the pool, the others (an infinite light chosen, no tree) are answered on the spot;
//   * a lane whose descent reaches its leaf writes sel_light[entry] and takes the next vertex from the pool IN THE SAME ROUND;
//   * results are indexed by entry, nothing is left behind in a segment: the wave streams segment after segment and kind after kind
//     (SegStream) and drains its lanes once, at the end of the launch.
// Arithmetic per vertex is that of bvh_sample_light, operation for operation (test_light_bvh_parity: pmf at 0 ulp;
// test_light_preselection_is_result_neutral: film bit-identical with the fused form and with the kernel above, HK_SELECT_POOL=0).
// ---------------------------------------------------------------------------------------------------
//   * desynchronised lanes each fetch their own 128-B pair every round — 64 different lines per load instruction, where the batches of
//     the kernel above still shared the top of the tree: the first pooled version issued 20 % fewer VALU instructions at 84 % lane
//     utilisation (67 %) and was SLOWER, waiting 51 % of its wave-cycles for memory (16 %).  So the top NTOP entries of the tree — the
//     first 9 levels in the pair order, half of an average descent — live in the block's LDS (one array per 16-byte part of a node, as
//     in NodeCache).
#ifndef HK_SELECT_NTOP
#define HK_SELECT_NTOP 512
#endif
#ifndef HK_SELECT_BLOCK
#define HK_SELECT_BLOCK 256
#endif
template <int NTOP>
HKD DLightNode lds_light_node(const lds_float4* top, int i) {
    const hk_f4v a = top[i], b = top[NTOP + i], c = top[2 * NTOP + i], d = top[3 * NTOP + i];
    DLightNode n;
    n.centre[0] = a.x, n.centre[1] = a.y, n.centre[2] = a.z, n.half_diag = a.w;
    n.r2 = b.x, n.w[0] = b.y, n.w[1] = b.z, n.w[2] = b.w;
    n.phi = c.x, n.cos_o = c.y, n.cos_e = c.z, n.sin_o = c.w;
    n.bits = __float_as_uint(d.x), n.child1_or_light = __float_as_uint(d.y);
    n.pad[0] = n.pad[1] = 0u;
    return n;
}
#ifndef HK_SELECT_WAVES
#define HK_SELECT_WAVES 4   // 40 KB of LDS per 4-wave block: four blocks per CU.  Measured (many-light frame, shade class, interleaved on one box):
#endif                      // per-lane refill 0.680 s; pool without the top cache 0.759; 256 / 512 / 4 waves 0.613; 512 / 512 / 6 waves (80 VGPRs, spills) 0.650;
                            // 512 / 512 / 4 waves 0.617; one 1024-thread block with the top 1024 entries 0.610
template <bool FT, int BLOCK = HK_SELECT_BLOCK, int NTOP = HK_SELECT_NTOP>
__global__ void __attribute__((amdgpu_flat_work_group_size(BLOCK, BLOCK), amdgpu_waves_per_eu(HK_SELECT_WAVES))) k_light_select_pool(DPathState st, DScene sc, DTables T, DFrame fr, DSobol sob, int depth, uint32_t kinds_mask, DStats* stats) {
    __shared__ uint32_t lds_pool[BLOCK / 64][8][64];   // [wave of the block][field][entry] (bit patterns): lane i reads entry head + rank(i) — consecutive words, no bank conflict
    __shared__ float4 lds_top[NTOP > 0 ? 4 * NTOP : 1];
    uint32_t (*pool)[64] = lds_pool[threadIdx.x >> 6];
    const lds_float4* top = (const lds_float4*)lds_top;
    const int n_top = NTOP > 0 ? (2 * sc.num_bvh_lights < NTOP ? 2 * sc.num_bvh_lights : NTOP) : 0;   // the tree of n lights has 2 n entries (entry 1 unused)
    if (NTOP > 0) {
        for (int i = threadIdx.x; i < n_top; i += BLOCK) {
            const float4* q = reinterpret_cast<const float4*>(sc.lnodes + i);
            lds_top[i] = q[0], lds_top[NTOP + i] = q[1], lds_top[2 * NTOP + i] = q[2], lds_top[3 * NTOP + i] = q[3];
        }
        __syncthreads();
    }
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned n_lnodes = 0;
    const DPathGen g = gen_at(st, depth);
    const int base_dim = 6 + 7 * depth;
    const int ninf = sc.num_infinite_lights, nbvh = sc.num_bvh_lights;
    const bool has_bvh = nbvh > 0;
    const float p_inf = (float)ninf / (float)(ninf + (has_bvh ? 1 : 0));
    uint32_t root_bits = 2u, root_child = 0u;
    if (has_bvh) {
        const DLightNode root = load_light_node(sc.lnodes, 0);
        root_bits = __builtin_amdgcn_readfirstlane(root.bits), root_child = __builtin_amdgcn_readfirstlane(root.child1_or_light);
    }
    SegStream stream = stream_open(st, ticket_ptr(st, depth, TK_SELECT), false, depth, Q_RAY);
    int gw = -1, kind = HK_MAX_KINDS, n = 0, cursor = 0;   // the input: entries cursor .. n - 1 of `queue`, the per-kind queue of segment gw
    const uint32_t* __restrict__ queue = st.mat_q;
    bool more = true;
    int pool_n = 0, pool_head = 0;
    // per-lane descent
    bool busy = false;
    uint32_t slot = 0, bits = 0, child = 0;
    int lvl = 0;
    float ub = 0.0f, pmf = 0.0f;
    v3 p = mk3(0, 0, 0), nn = mk3(0, 0, 1);
    for (;;) {
        const unsigned long long free_m = __ballot(!busy);
        if (free_m != 0ull) {
            if (pool_head == pool_n && more) {
                // ---- the next (up to 64) entries of the input ----
                while (more && cursor >= n) {
                    ++kind;
                    while (kind < HK_MAX_KINDS && !(kinds_mask & (1u << kind))) ++kind;
                    if (kind >= HK_MAX_KINDS) {   // this segment's kinds are used up: the next segment
                        gw = stream_next(stream, st.n_waves);
                        if (gw >= st.n_waves) {
                            more = false;
                            break;
                        }
                        kind = -1;
                        continue;
                    }
                    queue = st.mat_q + ((size_t)kind * st.n_waves + gw) * st.wave_cap;
                    n = *count_ptr(st, depth, Q_MAT0 + kind, gw);
                    cursor = 0;
                }
                pool_n = pool_head = 0;
                if (more) {
                    const int take = n - cursor < 64 ? n - cursor : 64;
                    bool descend = false;
                    uint32_t e = 0;
                    float u_b = 0.0f;
                    v3 sp = mk3(0, 0, 0), sn = mk3(0, 0, 1);
                    if (lane < take) {
                        e = queue[cursor + lane] & ~HK_MATQ_EMISSIVE;
                        const float4 H = st.hit[e], O = ld_ray_o(st, g, e, depth, (size_t)gw * st.wave_cap), D = g.ray_d[e];
                        const Surface sf = surface_at(sc, __float_as_int(H.y), H.z, H.w, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), H.x);
                        sp = sf.pi;
                        sn = sf.ns;
                        int pix, k;
                        split_slot(fr, ld_meta(st, g, e, depth).y, pix, k);
                        const SobolCtx sctx = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix, k, fr.first_sample + k * fr.sample_stride);
                        const float u = sobol_1d<FT>(sctx, base_dim + 1);
                        // bvh_sample_light's prologue: the infinite lights, then the root
                        int res_light = 0;
                        float res_pmf = 0.0f;
                        if (ninf + nbvh > 0) {
                            if (ninf > 0 && u < p_inf) {
                                const float ur = u / p_inf;
                                int idx = (int)floorf(ur * (float)ninf);
                                idx = (idx < ninf - 1 ? idx : ninf - 1) + 1;
                                res_pmf = p_inf / (float)ninf;
                                res_light = sc.infinite_lights[idx - 1];
                            } else if (has_bvh) {
                                u_b = ninf > 0 ? minf((u - p_inf) / (1.0f - p_inf), 0.99999994f) : minf(u, 0.99999994f);
                                if (root_bits & 2u) {   // a tree of one light
                                    res_pmf = 1.0f - p_inf;
                                    res_light = (int)root_child;
                                } else
                                    descend = true;
                            }
                        }
                        if (!descend) st.sel_light[e] = make_uint2((uint32_t)res_light, __float_as_uint(res_pmf));
                    }
                    cursor += take;
                    const unsigned long long dm = __ballot(descend);
                    if (descend) {
                        const int at = __popcll(dm & lt_mask);
                        pool[0][at] = e;
                        pool[1][at] = __float_as_uint(sp.x), pool[2][at] = __float_as_uint(sp.y), pool[3][at] = __float_as_uint(sp.z);
                        pool[4][at] = __float_as_uint(sn.x), pool[5][at] = __float_as_uint(sn.y), pool[6][at] = __float_as_uint(sn.z);
                        pool[7][at] = __float_as_uint(u_b);
                    }
                    pool_n = __popcll(dm);
                    __builtin_amdgcn_wave_barrier();   // (the pool belongs to this wave alone: LDS operations of one wave complete in order)
                }
            }
            const int avail = pool_n - pool_head;
            if (avail > 0) {
                const int rank = __popcll(free_m & lt_mask);
                if (!busy && rank < avail) {
                    const int at = pool_head + rank;
                    slot = pool[0][at];
                    p = mk3(__uint_as_float(pool[1][at]), __uint_as_float(pool[2][at]), __uint_as_float(pool[3][at]));
                    nn = mk3(__uint_as_float(pool[4][at]), __uint_as_float(pool[5][at]), __uint_as_float(pool[6][at]));
                    ub = __uint_as_float(pool[7][at]);
                    pmf = 1.0f - p_inf;
                    bits = root_bits, child = root_child;
                    lvl = 0;
                    busy = true;
                }
                const int free_n = __popcll(free_m);
                pool_head += free_n < avail ? free_n : avail;
            }
            if (__ballot(busy) == 0ull) {
                if (!more && pool_head == pool_n) break;
                continue;
            }
        }
        // ---- one level of the descent for every lane that is on its way (a lane that took a vertex above starts at once) ----
        if (busy) {
            int res_light = -1;
            float res_pmf = 0.0f;
            if (lvl >= 64) {   // the reference gives up after 64 levels (bvh-light-sampler.jl:126)
                res_light = 0;
            } else {
                ++lvl;
                DLightNode n0, n1;
                if (NTOP > 0 && (int)child + 1 < n_top) {
                    n0 = lds_light_node<NTOP>(top, (int)child), n1 = lds_light_node<NTOP>(top, (int)child + 1);
                    asm volatile("" : "+v"(n0.bits));   // (keeps the two arms apart: a select of generic pointers would become one flat load)
                } else
                    n0 = load_light_node(sc.lnodes, (int)child), n1 = load_light_node(sc.lnodes, (int)child + 1);
                const float c0 = node_importance(n0, p, nn);
                const float c1 = node_importance(n1, p, nn);
                n_lnodes += 2;
                if (c0 == 0.0f && c1 == 0.0f) {
                    res_light = 0;
                } else {
                    const float p0 = c0 / (c0 + c1);
                    if (ub < p0) {
                        pmf *= p0;
                        ub = ub / p0;
                        bits = n0.bits, child = n0.child1_or_light;
                    } else {
                        pmf *= (1.0f - p0);
                        ub = (ub - p0) / (1.0f - p0);
                        bits = n1.bits, child = n1.child1_or_light;
                    }
                    if ((bits & 2u) && lvl < 64) {   // the chosen child is a leaf: its light, with the pmf of the way down (a leaf 64 levels down is never looked at: bvh-light-sampler.jl:126)
                        res_light = (int)child;
                        res_pmf = pmf;
                    }
                }
            }
            if (res_light >= 0) {
                st.sel_light[slot] = make_uint2((uint32_t)res_light, __float_as_uint(res_pmf));
                busy = false;
            }
        }
    }
    stats += global_wave();
    wave_add(&stats->light_nodes, n_lnodes);
}

#ifndef HK_SHADE_WAVES_MATTE
#define HK_SHADE_WAVES_MATTE 4
#endif
#ifndef HK_SHADE_WAVES
#define HK_SHADE_WAVES 3
#endif
#ifndef HK_SHADE_WAVES_LEAN   // the LEAN Matte instantiation (shade_body) whose draws are table loads
#define HK_SHADE_WAVES_LEAN 5
#endif
#ifndef HK_SHADE_WAVES_LEAN_HASH   // the LEAN instantiation with the digit-hashing fallback in it
#define HK_SHADE_WAVES_LEAN_HASH 5
#endif
// K8 for one flagged vertex (surface-eval.jl:147-220): L += beta * Le / MIS denominator.
// LEAN (shade_body): the generation records are compact with 32-bit meta words and r_u == 1 — the weights are one float each, the
// same additions in the same order (the four equal components of the general form are summed one by one: 3a + a is not 4a in binary32)
template <bool TWO_PLANES, bool SIMPLE, bool LEAN = false>
HKD void shade_emission(const DPathState& st, const DPathGen& g, bool ones, const DScene& sc, const DTables& T, uint32_t slot, unsigned& n_lnodes, int depth, size_t seg) {
    const float4 H = st.hit[slot];
    const float4 O = ld_ray_o(st, g, slot, depth, seg), D = g.ray_d[slot];
    const v3 ro = mk3(O.x, O.y, O.z), rd = mk3(D.x, D.y, D.z);
    const float t_hit = H.x;
    const int prim = __float_as_int(H.y);
    const DTriMeta meta = tri_meta(sc, prim);
    if (meta.arealight <= 0) return;
    const Surface sf = surface_at(sc, prim, H.z, H.w, ro, rd, t_hit);
    const v3 wo = -rd;
    uint2 pmeta;
    if constexpr (LEAN) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(g.meta)[slot];
        pmeta = make_uint2((uint32_t)depth | (((w >> 30) & 1u) << 8), w & 0x3fffffffu);
    } else
        pmeta = ld_meta(st, g, slot, depth);
    const S4 lambda = ld_lambda(st, g, slot, pmeta.y);
    const DLight& light = sc.lights[meta.arealight - 1];
    S4 Le = arealight_Le<TWO_PLANES, SIMPLE>(sc, T, light, wo, sf.n, sf.uv, lambda);
    if (is_black(Le)) return;
    const S4 beta = ld_throughput(g.beta, slot, ones);
    const uint32_t fl = pmeta.x;
    const int pdepth = (int)(fl & 0xff);
    const bool specular_bounce = (fl >> 8) & 1u;
    S4 contribution = beta * Le;
    S4 fin;
    if constexpr (LEAN) {
        // average(r_u) == (((1 + 1) + 1) + 1) / 4 == 1 and x / 1 == x
        fin = contribution;
        if (!(pdepth == 0 || specular_bounce)) {
            const float r_l = ones ? 1.0f : D.w;   // (compact: r_l travels in the fourth word of ray_d)
            float choice = bvh_pmf(sc, sf.pi, sf.n, (int)meta.arealight, n_lnodes);
            float ct = fabsf(dot(sf.n, normalize(rd)));
            float light_pdf = 0.0f;
            if (ct > 0.0f && sf.area > 0.0f) light_pdf = choice * ((t_hit * t_hit) / (ct * sf.area));
            const float a = 1.0f + r_l * light_pdf;
            const float den = (((a + a) + a) + a) / 4.0f;
            if (den > 1e-10f) fin = contribution / den;
        }
    } else {
        const S4 r_u = ld_ru(g, slot, ones, st.compact != 0), r_l = ld_rl(g, slot, ones, st.compact != 0);
        if (pdepth == 0 || specular_bounce)
            fin = contribution / average(r_u);
        else {
            float choice = bvh_pmf(sc, sf.pi, sf.n, (int)meta.arealight, n_lnodes);
            float ct = fabsf(dot(sf.n, normalize(rd)));
            float light_pdf = 0.0f;
            if (ct > 0.0f && sf.area > 0.0f) light_pdf = choice * ((t_hit * t_hit) / (ct * sf.area));
            S4 rl = r_l * light_pdf;
            float den = average(r_u + rl);
            fin = den > 1e-10f ? contribution / den : contribution / average(r_u);
        }
    }
    st4(&st.L[pmeta.y], ld4(&st.L[pmeta.y]) + fin);
}

template <int KIND>
struct ShadeWaves {
    // Matte runs faster at 4 waves per SIMD with some scratch than at 3 without (Cornell: the scratch-free three-wave build of
    // k_shade<Matte, SIMPLE, FT> is 19 % slower, 42.6 -> 50.6 ms per frame).  By the compiler's listing k_shade<Matte, SIMPLE, FT> holds
    // 128 VGPRs + 28 B of scratch per lane at 4 waves (96 + 156 B at 5), k_shade<Matte, SIMPLE, !FT> 128 + 76 B (96 + 220 B at 5): the
    // fifth wave is the LEAN instantiation's (shade_body), which fits 96 registers.  The kinds with larger BSDFs lose more to the
    // spills than the fourth wave returns (sky: conductor + glass +7 %)
    static constexpr int value = (KIND == HK_MAT_COATED_DIFFUSE || KIND == HK_MAT_COATED_DIFFUSE_TRANSMISSION) ? 1 : (KIND == HK_MAT_MATTE ? HK_SHADE_WAVES_MATTE : HK_SHADE_WAVES);
};
#ifndef HK_SHADE_MIN_WAVES
#define HK_SHADE_MIN_WAVES 1
#endif
// SIMPLE (instantiated for Matte): the scene has no ambient / environment light and no texture of any kind (DScene::simple_lights)
// FT ("full tables"; Matte, Mirror, Glass, Conductor): every Sobol draw of this bounce is in the sampler's two tables for every path of the launch (the host
// checks DSobol::lo_rows against the rows of this depth): the draws are two loads each and the digit-hashing fallback — three 64-bit
// hash loops inlined at each of the five draw sites — is not in the kernel at all.
// PRE: the light of this vertex's next-event estimation was chosen by k_light_select (scenes with a deep light BVH): the descent —
// three quarters of this kernel's time in the 5*10^4-light scene, run at 49 % lane utilisation because leaf depths differ — is not here.
// LEAN (Matte; the launcher: compact && meta32 && sh_final state in a lean_scene): what those run-time facts fix is fixed at compile
// time.  r_u is the constant 1 (neither loaded nor kept), the MIS weights are one float each, there is no medium and no interface
// record, the meta word is the 32-bit one, the slim shadow record the only one.  Only exact folds (1 * x, x / 1, component .x): the
// films are those of the general instantiation bit for bit.  The values that only the second half of a vertex reads (K11 and the
// BSDF evaluation at the end of K9) wait in `stash` — HK_SHADE_STASH dwords per lane of LDS, [dword][thread of the block] — while the
// light is chosen and sampled: with them out of the register file the kernel fits 96 registers, five waves per SIMD.
#define HK_SHADE_STASH 16
// LEAN, HK_SHADE_PREFETCH: the next chunk's records wait in LDS, fetched by global->LDS loads (no register holds anything across the
// loop body).  [part][thread of the block]; a wave's 64 lanes own 64 consecutive entries of every part: the LDS base of a load is
// wave-uniform, the hardware adds lane * size.  entry[chunk & 1]: the queue entry, requested two chunks ahead at the top of a chunk;
// hit / ray_d / meta: requested one chunk ahead from the middle of a chunk, where the registers are at their lowest, through that entry.
// 2 * 1 KB + 4 KB + 4 KB + 1 KB = 11 KB beside the 18 KB of list and stash: five blocks per CU still fit (beta, the next in line,
// would not: 15 KB + 18 KB).
struct ShadeStage {
    uint32_t* entry;   // [2][256]
    float4* hit;       // [256]
    float4* ray_d;     // [256]
    uint32_t* meta;    // [256]
};
// this lane's 4 / 16 bytes at src -> lds_wave_base[lane]
__device__ __forceinline__ void lds_fetch4(const uint32_t* src, uint32_t* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
__device__ __forceinline__ void lds_fetch16(const float4* src, float4* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// SLOTS (LEAN, a scene of ONE material kind whose trace launch ran the single-kind flush: launch_shade): the kind queue sorts nothing, so
// the wave walks the segment's generation itself — slot = seg + i for i below the segment's RAY count — and every record load is a
// contiguous 64-lane load.  An entry whose ray escaped holds HK_MAT_ESCAPED in mat_id and its lane sits the chunk out; the emissive flag is
// mat_id's own bit.  The fetch-ahead needs no queue entry: the next chunk's slots are this chunk's + 64, requested near the top of a chunk,
// behind the emission block (all lanes, escaped ones too: their successors may hold hits), the mat_id word with them in stage.entry[0 .. 255].  Shadow and continuing
// records are appended in walk order, so every generation of a segment stays in ascending path-slot order down the bounces.
// GEO (LEAN): surface_at reads the hit triangle's geometric normal and area from the scene's table (DScene::tri_geo) instead of the positions.
template <int KIND, bool SIMPLE, bool FT, bool PRE, bool LEAN = false, bool SLOTS = false, bool GEO = false>
__device__ __forceinline__ void shade_body(const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, int first_kind, DStats* stats, const SegTickets& src,
                                           uint32_t* __restrict__ elist,   // elist: this wave's 128 LDS words (slots of flagged — emissive-hit — vertices waiting for the dense K8 pass)
                                           float* stash = nullptr,         // LEAN: the block's HK_SHADE_STASH * 256 LDS words
                                           ShadeStage stage = ShadeStage{}) {   // LEAN: the block's staging area of the fetch-ahead (null pointers: none)
    static_assert(!LEAN || (KIND == HK_MAT_MATTE && HK_LAMBDA_BY_SLOT), "the lean body is Matte's");
    static_assert(!SLOTS || LEAN, "the slot walk is the lean body's");
    static_assert(!GEO || LEAN, "the geometry table is read by the lean body");
    const int lane = lane_id();
    unsigned n_vertices = 0, n_lnodes = 0;
    unsigned nv_wave = 0;   // LEAN: the vertices of the whole wave
    // LEAN: the per-lane count of light-BVH nodes lives in the last stash word between the chunks
    unsigned* const nl_stash = LEAN ? reinterpret_cast<unsigned*>(stash) + (HK_SHADE_STASH - 1) * 256 + threadIdx.x : nullptr;
    auto nl_flush = [&]() {
        if constexpr (LEAN) {
            if (n_lnodes) *nl_stash += n_lnodes;
            n_lnodes = 0;
        }
    };
    if constexpr (LEAN) *nl_stash = 0u;
    // LEAN: what is the same for the whole wave (segment, counts) is said to be (readfirstlane): it lives in scalar registers
    auto uni = [](int v) { return LEAN ? __builtin_amdgcn_readfirstlane(v) : v; };
    HK_FOR_EACH_SEGMENT_FROM(gw_v, st, src) {
    const int gw = uni(gw_v);
    const uint32_t* __restrict__ queue = st.mat_q + ((size_t)KIND * st.n_waves + gw) * st.wave_cap;
    const int n = uni(*count_ptr(st, depth, SLOTS ? Q_RAY : Q_MAT0 + KIND, gw));   // SLOTS: every entry of the generation, hit or escaped
    const DPathGen g = gen_at(st, depth), gn = st.gen[(depth + 1) & 1];
    const size_t seg = (size_t)gw * st.wave_cap;
    const bool ones = depth == 0 && fr.implicit_ones;
    // several kinds append to the same shadow-record / next-generation segments: continue from the counts left by the kinds before
    WavePos q_shadow{0}, q_next{0};
    if (!first_kind) {
        q_shadow.count = uni(*count_ptr(st, depth, Q_SHADOW, gw));
        q_next.count = uni(*count_ptr(st, depth + 1, Q_RAY, gw));
    }
    // ---- K8, densely: emission from area-light hits, MIS against the light-BVH pmf (surface-eval.jl:147-220).  The trace kernels
    //      flag such hits in the kind-queue entry (HK_MATQ_EMISSIVE); the flagged entries are gathered in a wave-private LDS list and
    //      handled 64 at a time.  Done inline for every vertex, a wave walks the light BVH (bvh_pmf, ~2 log2 n node evaluations)
    //      whenever ANY of its 64 vertices sits on an emitter: with 5 % emissive faces that is 96 % of the waves at 5 % lane
    //      utilisation.  The list is fed by the main pass's own queue load and emptied whenever 64 entries wait, and once more after
    //      the segment's last chunk: an emission add touches L of its own path alone, which nothing else in this kernel reads or
    //      writes, so where in the launch it happens is free. ----
    int n_emit = 0;
    // the first `take` (<= 64) entries of the list; the rest moves to the front
    auto emit_pass = [&](int take) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < take) shade_emission<KIND == HK_MAT_MATTE, SIMPLE, LEAN>(st, g, ones, sc, T, elist[lane], n_lnodes, depth, seg);
        nl_flush();
        const int rest = n_emit - take;
        const uint32_t moved = lane < rest ? elist[64 + lane] : 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < rest) elist[lane] = moved;
        n_emit = rest;
    };
    const bool prescan = !SLOTS && uni(st.shade_prescan) != 0;
    if (prescan) {
        // HK_SHADE_PRESCAN=1 (A/B switch; films bit-identical): the flag is looked up in mat_id by a pass of its own over the whole
        // queue before the first vertex is shaded — two dependent round trips per chunk that the default does not make
        for (int base = 0; base < n || n_emit > 0; base += 64) {
            if (base < n) {
                const int i = base + lane;
                const uint32_t cand = i < n ? queue[i] & ~HK_MATQ_EMISSIVE : 0u;
                const bool em = i < n && (st.mat_id[cand] & HK_MAT_EMISSIVE_BIT) != 0;
                const unsigned long long m = __ballot(em);
                if (em) elist[n_emit + __popcll(m & ((1ull << lane) - 1ull))] = cand;
                n_emit += __popcll(m);
                if (n_emit < 64 && base + 64 < n) continue;
            }
            emit_pass(n_emit < 64 ? n_emit : 64);
        }
    }
    // LEAN fetch-ahead: this wave's 64 entries of every staging part; the entry of chunk 1 is requested before chunk 0 starts
    const bool prefetch = LEAN && stage.entry != nullptr;
    const int wave0 = LEAN ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) : 0;
    if constexpr (LEAN && !SLOTS) {
        if (prefetch && 64 + lane < n) lds_fetch4(&queue[64 + lane], stage.entry + 256 + wave0);
    }
    for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        bool active = i < n;
        if constexpr (LEAN && !SLOTS) {   // the entry of chunk k + 2 (never one at or past n): its address depends on nothing
            if (prefetch && i + 128 < n) lds_fetch4(&queue[i + 128], stage.entry + ((base >> 6) & 1) * 256 + wave0);
        }
        const bool staged = prefetch && base > 0;   // this chunk's hit, ray_d and meta word were requested from the middle of the chunk before (SLOTS: from its top)
        float4 H_staged = make_float4(0, 0, 0, 0), D_staged = H_staged;   // SLOTS: what the top of a staged chunk reads from the staging area
        uint32_t meta_staged = 0;
        uint32_t slot;
        bool em_slot = false;
        uint32_t mat_w = HK_MAT_ESCAPED;   // SLOTS: the path's mat_id word (the vertex takes its material index from it)
        if constexpr (SLOTS) {
            slot = (uint32_t)seg + (uint32_t)i;   // generation index of the path: the segment's entries in order
            if (staged) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the staged records have landed
                const uint32_t w = stage.entry[(int)threadIdx.x];
                if (active) mat_w = w;
            } else if (active)
                mat_w = reinterpret_cast<const uint32_t*>(st.mat_id)[slot];
            active = mat_w != HK_MAT_ESCAPED;
            em_slot = active && (mat_w & HK_MAT_EMISSIVE_BIT) != 0u;
        } else
            slot = active ? queue[i] : 0u;   // generation index of the path (the kind queue is a sorted subset of the segment)
        {   // the entry's flag: an emissive hit waits in the list for the dense K8 pass (at most 63 waiting + 64 new of its 128 words)
            const bool em = SLOTS ? em_slot : !prescan && (slot & HK_MATQ_EMISSIVE) != 0u;
            if constexpr (!SLOTS) slot &= ~HK_MATQ_EMISSIVE;
            const unsigned long long m = __ballot(em);
            if (m != 0ull) {
                if (em) elist[n_emit + __popcll(m & ((1ull << lane) - 1ull))] = slot;
                n_emit += __popcll(m);
                if (n_emit >= 64) emit_pass(64);
            }
        }
        if constexpr (SLOTS) {   // (behind the emission pass: nothing but the slot lives across it)
            if (staged) {
                const int t = (int)threadIdx.x;
                H_staged = stage.hit[t], D_staged = stage.ray_d[t], meta_staged = stage.meta[t];
                // the values are in registers before the staging area is handed to the next chunk's loads
                asm volatile("" : "+v"(H_staged.x), "+v"(H_staged.y), "+v"(H_staged.z), "+v"(H_staged.w), "+v"(D_staged.x), "+v"(D_staged.y), "+v"(D_staged.z), "+v"(D_staged.w), "+v"(meta_staged) : : "memory");
            }
            if (prefetch && i + 64 < n) {   // the records of chunk k + 1 (never one at or past n), whatever became of this lane's own ray
                const uint32_t ns = slot + 64u;
                lds_fetch4(reinterpret_cast<const uint32_t*>(st.mat_id) + ns, stage.entry + wave0);
                lds_fetch16(&st.hit[ns], stage.hit + wave0);
                lds_fetch16(&g.ray_d[ns], stage.ray_d + wave0);
                lds_fetch4(reinterpret_cast<const uint32_t*>(g.meta) + ns, stage.meta + wave0);
            }
        }
        bool push_shadow = false, push_ray = false;
        // state shared by the two halves of the vertex (NEE, then BSDF sampling): loaded once
        float4 H = make_float4(0, 0, 0, 0);
        if constexpr (SLOTS) H = H_staged;
        Surface sf;
        v3 wo = mk3(0, 0, 1);
        DTriMeta meta{0u, 0u, 0u};
        S4 lambda = s4(0.0f), beta = s4(0.0f), r_u = s4(0.0f), kd_matte = s4(0.0f);
        uint32_t fl = 0, pslot = 0;
        int pdepth = 0, medium = -1;
        bool any_non_specular = false;
        SobolCtx sctx;
        using W = std::conditional_t<LEAN, float, S4>;   // a MIS weight
        // LEAN: this lane's column of the stash, [dword][thread]; stash_at launders the index so that no store is forwarded to a load
        auto stash_at = [&]() {
            int i = (int)threadIdx.x;
            asm volatile("" : "+v"(i));
            return stash + i;
        };
        // every path in the depth-d queues has work.depth == d, so the dimension (and its scramble hashes) is
        // wave-uniform: derived from the kernel argument it stays in scalar registers
        const int base_dim = 6 + 7 * depth;
        float4 shO = make_float4(0, 0, 0, 0), shD = shO;
        S4 shLd = s4(0.0f);
        W shRu{}, shRl{};
        if constexpr (SLOTS) nv_wave += (unsigned)__popcll(__ballot(active));   // (the entries that hold a hit)
        else if constexpr (LEAN) nv_wave += (unsigned)(n - base < 64 ? n - base : 64);   // (wave-uniform: a scalar register)
        if (active) {
            if constexpr (!LEAN) ++n_vertices;
            float4 D;
            uint32_t meta_w = 0;   // LEAN: the record's 32-bit meta word (path slot, specular and any-non-specular bits)
            // the vertex's material record: mat_id read ONCE for this half (SLOTS: not at all — the chunk holds the word); the second half
            // reads it again rather than keep a register across the light's choice and sample
            const int mat_idx = (SLOTS ? (int)mat_w : st.mat_id[slot]) & ~HK_MAT_EMISSIVE_BIT;
            if (SLOTS && staged)
                D = D_staged, meta_w = meta_staged;   // (and H: read at the top of the chunk)
            else if (LEAN && staged) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the staged records have landed
                const int t = (int)threadIdx.x;
                H = stage.hit[t], D = stage.ray_d[t], meta_w = stage.meta[t];
            } else {
                H = stream_ld(&st.hit[slot]);
                D = stream_ld(&g.ray_d[slot]);
                if constexpr (LEAN) meta_w = reinterpret_cast<const uint32_t*>(g.meta)[slot];
            }
            float4 O = ld_ray_o(st, g, slot, depth, seg);
            v3 ro = mk3(O.x, O.y, O.z), rd = mk3(D.x, D.y, D.z);
            float t_hit = H.x;
            int prim = __float_as_int(H.y);
            sf = surface_at<GEO>(sc, prim, H.z, H.w, ro, rd, t_hit);
            wo = -rd;
            meta = tri_meta(sc, prim);
            if constexpr (LEAN) {
                pslot = meta_w & 0x3fffffffu;
                pdepth = depth;   // (what ld_meta returns for a 32-bit word: every path of the depth-d queues is at depth d)
                any_non_specular = (meta_w >> 31) != 0u;
            } else {
                const uint2 pmeta = ld_meta(st, g, slot, depth);
                fl = pmeta.x;
                pslot = pmeta.y;
                pdepth = (int)(fl & 0xff);
                any_non_specular = (fl >> 9) & 1u;
                medium = (int)(fl >> 16) - 1;
                r_u = ld_ru(g, slot, ones, st.compact != 0);
            }
            lambda = ld_lambda(st, g, slot, pslot);
            if (ones)
                beta = s4(1.0f);
            else {
                const float4 bv = stream_ld(&g.beta[slot]);
                beta = s4(bv.x, bv.y, bv.z, bv.w);
            }

            // pixel coordinates for the Sobol dimensions of this bounce (volpath.jl:252-262, Q19)
            int pix, k;
            split_slot(fr, pslot, pix, k);
            sctx = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix, k, fr.first_sample + k * fr.sample_stride);

            if (KIND == HK_MAT_MATTE) kd_matte = matte_kd<SIMPLE>(sc, T, sc.materials[mat_idx], TexCtx(sf.uv, meta.prim_index, H.z, H.w), lambda);
#ifdef HK_ABLATE
            // cost attribution by duplication (tools/ablate.md): stage HK_ABLATE runs a second time on laundered inputs, its result is
            // kept alive but unused; the k_shade time delta against the plain build is that stage's cost.  Never defined in the product.
            {
                float sink = 0.0f;
                if (HK_ABLATE == 1) {   // every Sobol draw of a matte vertex
                    uint32_t ps2 = pslot;
                    int d2 = base_dim;
                    asm volatile("" : "+v"(ps2));
                    asm volatile("" : "+s"(d2));
                    int pix2, k2;
                    split_slot(fr, ps2, pix2, k2);
                    SobolCtx c2 = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix2, k2, fr.first_sample + k2 * fr.sample_stride);
                    v2 a = sobol_2d(c2, d2 + 3), b = sobol_2d(c2, d2 + 6);
                    sink = sobol_1d(c2, d2 + 1) + a.x + a.y + b.x + b.y + sobol_1d(c2, d2 + 7);
                }
                if (HK_ABLATE == 2 && sc.n_lights > 0) {   // light-BVH descent
                    float u2 = H.z, pmf2;
                    asm volatile("" : "+v"(u2));
                    unsigned dummy = 0;
                    sink = (float)bvh_sample_light(sc, sf.pi, sf.ns, u2, pmf2, dummy) + pmf2;
                }
                if (HK_ABLATE == 3 && sc.n_lights > 0) {   // sample_light on a pseudo-random light
                    uint32_t li = pslot;
                    asm volatile("" : "+v"(li));
                    LightSample l2 = sample_light(sc, T, sc.lights[li % (uint32_t)sc.n_lights], sf.pi, lambda, mk2(H.z, H.w));
                    sink = l2.pdf + l2.Li.x + l2.Li.w + l2.wi.x + l2.p_light.z;
                }
                if (HK_ABLATE == 4) {   // matte_kd (spectral reflectance at four wavelengths)
                    S4 l2 = lambda;
                    asm volatile("" : "+v"(l2.x), "+v"(l2.y), "+v"(l2.z), "+v"(l2.w));
                    S4 k2 = matte_kd(sc, T, sc.materials[mat_idx], TexCtx(sf.uv, meta.prim_index, H.z, H.w), l2);
                    sink = k2.x + k2.y + k2.z + k2.w;
                }
                if (HK_ABLATE == 5) {   // surface_at
                    float b2 = H.z;
                    asm volatile("" : "+v"(b2));
                    Surface s2 = surface_at<GEO>(sc, prim, b2, H.w, ro, rd, t_hit);
                    sink = s2.pi.x + s2.n.y + s2.ns.z + s2.uv.x + s2.area;
                }
                if (HK_ABLATE == 6) {   // eval_matte_kd + sample_matte_kd on laundered directions
                    v3 w2 = wo;
                    asm volatile("" : "+v"(w2.x), "+v"(w2.y), "+v"(w2.z));
                    float p2;
                    S4 f2 = eval_matte_kd(kd_matte, w2, sf.n, sf.ns, p2);
                    BSDFSample s2 = sample_matte_kd(sc, sc.materials[mat_idx], kd_matte, w2, sf.ns, TexCtx(sf.uv, meta.prim_index, H.z, H.w), mk2(H.z, H.w));
                    sink = f2.x + f2.w + p2 + s2.pdf + s2.wi.x + s2.f.y;
                }
                if (HK_ABLATE == 7) {   // the mat_id -> material record fetches of a matte vertex (Kd's coefficients, sigma) on a laundered slot
                    uint32_t s2 = slot;
                    asm volatile("" : "+v"(s2));
                    const DMaterial& m2 = sc.materials[st.mat_id[s2] & ~HK_MAT_EMISSIVE_BIT];
                    const float4 c2 = m2.rgb[0].coef;
                    sink = c2.x + c2.y + c2.z + c2.w + eval_f32<SIMPLE>(sc, m2, 0, TexCtx(sf.uv, meta.prim_index, H.z, H.w));
                }
                asm volatile("" : : "v"(sink));
            }
#endif

            if constexpr (LEAN) {   // out of the registers while the light is chosen and sampled
                float* sp = stash + threadIdx.x;
                sp[0 * 256] = sf.n.x, sp[1 * 256] = sf.n.y, sp[2 * 256] = sf.n.z;
                sp[3 * 256] = wo.x, sp[4 * 256] = wo.y, sp[5 * 256] = wo.z;
                sp[6 * 256] = kd_matte.x, sp[7 * 256] = kd_matte.y, sp[8 * 256] = kd_matte.z, sp[9 * 256] = kd_matte.w;
                sp[10 * 256] = beta.x, sp[11 * 256] = beta.y, sp[12 * 256] = beta.z, sp[13 * 256] = beta.w;
                sp[14 * 256] = __uint_as_float(meta_w);
                // the registers are at their lowest here: the next chunk's entry (requested a chunk ago) names the records to stage
                if (!SLOTS && prefetch && i + 64 < n) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the entry has landed
                    const uint32_t ns = stage.entry[(((base >> 6) + 1) & 1) * 256 + (int)threadIdx.x] & ~HK_MATQ_EMISSIVE;
                    lds_fetch16(&st.hit[ns], stage.hit + wave0);
                    lds_fetch16(&g.ray_d[ns], stage.ray_d + wave0);
                    lds_fetch4(reinterpret_cast<const uint32_t*>(g.meta) + ns, stage.meta + wave0);
                }
            }
            // ---- K9: next-event estimation through the light BVH ----
            if (sc.n_lights > 0) {
                const DMaterial& mat = sc.materials[mat_idx];
                float light_pmf;
                int light_idx;
                if constexpr (PRE) {
                    const uint2 pre = st.sel_light[slot];
                    light_idx = (int)pre.x;
                    light_pmf = __uint_as_float(pre.y);
                } else {
                    float light_select = sobol_1d<FT>(sctx, base_dim + 1);
                    light_idx = bvh_sample_light(sc, sf.pi, sf.ns, light_select, light_pmf, n_lnodes);
                }
                if (light_idx >= 1 && light_idx <= sc.n_lights && light_pmf > 0.0f) {
                    const DLight& sel = sc.lights[light_idx - 1];
                    // delta lights ignore the 2-D sample (lights.jl:39-131): draw it only for lights that use it
                    v2 u_light = mk2(0.0f, 0.0f);
                    if (sel.kind >= HK_LIGHT_AMBIENT) u_light = sobol_2d<FT>(sctx, base_dim + 3);
                    LightSample ls = sample_light<KIND == HK_MAT_MATTE, SIMPLE>(sc, T, sel, sf.pi, lambda, u_light);
                    if (ls.pdf > 0.0f && !is_black(ls.Li)) {
                        float bsdf_pdf;
                        if constexpr (LEAN) {
                            const float* sp = stash_at();
                            wo = mk3(sp[3 * 256], sp[4 * 256], sp[5 * 256]);
                            kd_matte = s4(sp[6 * 256], sp[7 * 256], sp[8 * 256], sp[9 * 256]);
                            beta = s4(sp[10 * 256], sp[11 * 256], sp[12 * 256], sp[13 * 256]);
                        }
                        S4 f = KIND == HK_MAT_MATTE ? eval_matte_kd(kd_matte, wo, ls.wi, sf.ns, bsdf_pdf)
                                                    : eval_bsdf<KIND>(sc, T, mat, wo, ls.wi, sf.ns, TexCtx(sf.uv, meta.prim_index, H.z, H.w), lambda, bsdf_pdf);
                        if (!is_black(f)) {
                            float ct = fabsf(dot(ls.wi, sf.ns));
                            S4 Ld = beta * f * ls.Li * ct;
                            if (!is_black(Ld)) {
                                v3 off = 1e-4f * sf.ns;  // NB: shading normal (Q9)
                                v3 so = dot(ls.wi, sf.ns) > 0.0f ? sf.pi + off : sf.pi - off;
                                v3 tl = ls.p_light - so;
                                float tmax = sqrtf(dot(tl, tl)) - 1e-3f;
                                float nbp = ls.is_delta ? 0.0f : bsdf_pdf;
                                shO = make_float4(so.x, so.y, so.z, tmax);
                                shD = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, __int_as_float(medium));
                                shLd = Ld;
                                if constexpr (LEAN) {   // r_u == 1
                                    shRu = nbp;
                                    shRl = ls.pdf * light_pmf;
                                } else {
                                    shRu = r_u * nbp;
                                    shRl = (r_u * ls.pdf) * light_pmf;
                                }
                                push_shadow = true;
                            }
                        }
                    }
                }
            }
        }
        nl_flush();
        // the shadow record goes to its position in the segment's shadow queue: k_shadow streams the records
        {
            const size_t ps = seg + (size_t)wp_push(q_shadow, push_shadow);
            if constexpr (LEAN) {   // the slim record is the only one; its denominator by the general form's additions, in their order
                if (push_shadow) {
                    const float m = shRu + shRl;
                    shD.w = (((m + m) + m) + m) / 4.0f;
                    stream_st(&st.sh_o[ps], shO);
                    stream_st(&st.sh_d[ps], shD);
                    stream_st(&st.sh_Ld[ps], shLd);
                    stream_st(&st.sh_slot[ps], pslot);
                }
            } else if (push_shadow && st.sh_final) {   // slim record (shadow_contribute_final): the denominator beside the direction instead of two weights
                const S4 mis = s4(shRu.x) * s4(1.0f) + s4(shRl.x) * s4(1.0f);
                shD.w = average(mis);
                stream_st(&st.sh_o[ps], shO);
                stream_st(&st.sh_d[ps], shD);
                stream_st(&st.sh_Ld[ps], shLd);
                stream_st(&st.sh_slot[ps], pslot);
            } else if (push_shadow) {
                stream_st(&st.sh_o[ps], shO);
                stream_st(&st.sh_d[ps], shD);
                stream_st(&st.sh_Ld[ps], shLd);
                if (st.compact) {
#if HK_NT
                    __builtin_nontemporal_store((hk_f2){shRu.x, shRl.x}, (hk_f2*)(reinterpret_cast<float2*>(st.sh_ru) + ps));
#else
                    reinterpret_cast<float2*>(st.sh_ru)[ps] = make_float2(shRu.x, shRl.x);
#endif
                } else
                    st_shadow_weights(st, ps, shRu, shRl);
                stream_st(&st.sh_slot[ps], pslot);
            }
        }
        // ---- K11: BSDF sampling, throughput, Russian roulette, continuation ray ----
        float4 nO = make_float4(0, 0, 0, 0), nD = nO;
        S4 nb = s4(0.0f);
        W nrl{};
        uint32_t nflags = 0;
        if (active) {
            int new_depth = pdepth + 1;
            if (new_depth < fr.max_depth) {
                const DMaterial& mat = sc.materials[st.mat_id[slot] & ~HK_MAT_EMISSIVE_BIT];
                DMediumInterface mi{};
                if constexpr (LEAN) {   // back from the stash; the sampler context is derived again from the path slot (the same values)
                    const float* sp = stash_at();
                    sf.n = mk3(sp[0 * 256], sp[1 * 256], sp[2 * 256]);
                    wo = mk3(sp[3 * 256], sp[4 * 256], sp[5 * 256]);
                    kd_matte = s4(sp[6 * 256], sp[7 * 256], sp[8 * 256], sp[9 * 256]);
                    beta = s4(sp[10 * 256], sp[11 * 256], sp[12 * 256], sp[13 * 256]);
                    const uint32_t meta_w = __float_as_uint(sp[14 * 256]);
                    pslot = meta_w & 0x3fffffffu;
                    any_non_specular = (meta_w >> 31) != 0u;
                    int pix, k;
                    split_slot(fr, pslot, pix, k);
                    sctx = sobol_ctx_slot(sob, T.sobol, fr.x0, fr.y0, fr.tiles_x, pix, k, fr.first_sample + k * fr.sample_stride);
                } else
                    mi = sc.mis[meta.mi];
                // the 1-D component sample is read only by BSDFs that choose a lobe (Glass and the layered kinds)
                float uc = (KIND == HK_MAT_GLASS || KIND > HK_MAT_CONDUCTOR) && KIND != HK_MAT_FALLBACK ? sobol_1d<FT>(sctx, base_dim + 4) : 0.0f;
                v2 u = (KIND == HK_MAT_MIRROR || KIND == HK_MAT_GLASS || KIND == HK_MAT_THIN_DIELECTRIC) ? mk2(0.0f, 0.0f) : sobol_2d<FT>(sctx, base_dim + 6);
                bool regularize = fr.regularize && any_non_specular;
                BSDFSample s = KIND == HK_MAT_MATTE ? sample_matte_kd<SIMPLE>(sc, mat, kd_matte, wo, sf.ns, TexCtx(sf.uv, meta.prim_index, H.z, H.w), u)
                                                    : sample_bsdf<KIND>(sc, T, mat, wo, sf.ns, TexCtx(sf.uv, meta.prim_index, H.z, H.w), lambda, u, uc, regularize);
                if (s.pdf > 0.0f && !is_black(s.f)) {
                    float ct = fabsf(dot(s.wi, sf.ns));
                    nb = s.is_specular ? beta * s.f : beta * s.f * ct / s.pdf;
                    if constexpr (LEAN) nrl = s.is_specular ? 1.0f : 1.0f / s.pdf;   // r_u == 1
                    else nrl = s.is_specular ? r_u : r_u / s.pdf;
                    bool cont = true;
                    if (new_depth > 3) {  // russian_roulette_spectral, min_depth fixed at 3 (Q7)
                        float rr = sobol_1d<FT>(sctx, base_dim + 7);
                        float q = maxf(0.05f, 1.0f - max_component(nb));
                        if (rr < q)
                            cont = false;
                        else
                            nb = nb * (1.0f / (1.0f - q));
                    }
                    if (cont) {
                        int new_medium = -1;   // LEAN: no interface changes the medium, and -1 + 1 leaves the flag word's medium field 0
                        if constexpr (!LEAN) new_medium = (mi.inside != mi.outside) ? (dot(s.wi, sf.n) > 0.0f ? mi.outside : mi.inside) : medium;
                        v3 off = dot(s.wi, sf.n) > 0.0f ? sf.n : -sf.n;
                        v3 no = sf.pi + off * 0.0001f;
                        nO = make_float4(no.x, no.y, no.z, INF_F);
                        nD = make_float4(s.wi.x, s.wi.y, s.wi.z, 0.0f);  // time = 0 (Q17)
                        bool ans = any_non_specular || !s.is_specular;
                        nflags = (uint32_t)new_depth | ((s.is_specular ? 1u : 0u) << 8) | ((ans ? 1u : 0u) << 9) | ((uint32_t)(new_medium + 1) << 16);
                        push_ray = true;
                    }
                }
            }
        }
        {   // the continuing path's record, whole, at its position in the next generation (r_u is unchanged by a surface event)
            const size_t pn = seg + (size_t)wp_push(q_next, push_ray);
            if constexpr (LEAN) {   // the compact record with its 32-bit meta word
                if (push_ray) {
                    stream_st(&gn.ray_o[pn], nO);
                    nD.w = nrl;
                    stream_st(&gn.ray_d[pn], nD);
                    stream_st(&gn.beta[pn], nb);
                    stream_st(reinterpret_cast<uint32_t*>(gn.meta) + pn, pslot | (((nflags >> 8) & 1u) << 30) | (((nflags >> 9) & 1u) << 31));
                }
            } else if (push_ray) {
                stream_st(&gn.ray_o[pn], nO);
                if (st.compact) nD.w = nrl.x;   // (compact: r_l travels beside the direction)
                stream_st(&gn.ray_d[pn], nD);
                stream_st(&gn.beta[pn], nb);
                st_ru_rl(gn, pn, r_u, nrl, st.compact != 0);
                st_lambda(gn, pn, lambda);
                st_meta(st, gn, pn, nflags, pslot);
            }
        }
    }
    if (n_emit > 0) emit_pass(n_emit);   // the flagged entries still waiting (fewer than 64)
    if (lane == 0) {
        *count_ptr(st, depth, Q_SHADOW, gw) = q_shadow.count;
        *count_ptr(st, depth + 1, Q_RAY, gw) = q_next.count;
    }
    }
    if constexpr (LEAN) {
        n_vertices = lane == 0 ? nv_wave : 0u;   // (the statistics are sums over the lanes)
        n_lnodes = *nl_stash;
    }
    stats += global_wave();
    wave_add(&stats->vertices, n_vertices);
    wave_add(&stats->light_nodes, n_lnodes);
}
template <int KIND, bool SIMPLE = false, bool FT = false, bool PRE = false, bool LEAN = false, bool SLOTS = false, bool GEO = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(LEAN ? (FT ? HK_SHADE_WAVES_LEAN : HK_SHADE_WAVES_LEAN_HASH) : ShadeWaves<KIND>::value))) k_shade(DPathState st, DScene sc, DTables T, DFrame fr, DSobol sob, int depth, int first_kind, DStats* stats) {
    __shared__ uint32_t emit_list[4 * 128];
    SegTickets src = seg_open(st, ticket_ptr(st, depth, TK_SHADE0 + KIND), st.dynamic_segments != 0, depth, Q_MAT0 + KIND);
    if constexpr (LEAN) {
        src.pos = __builtin_amdgcn_readfirstlane(src.pos), src.k0 = __builtin_amdgcn_readfirstlane(src.k0);   // (wave-uniform: the wave's index)
        __shared__ float stash[HK_SHADE_STASH * 256];   // five blocks per CU: 5 x (2 KB + 16 KB + 11 KB) of the CU's 160 KB
        // the staging area of the fetch-ahead: objects of their own, so that the compiler can tell its reads from the stash's
        __shared__ uint32_t stage_entry[2 * 256];
        __shared__ float4 stage_hit[256];
        __shared__ float4 stage_ray_d[256];
        __shared__ uint32_t stage_meta[256];
        ShadeStage stage{};
        if (st.shade_prefetch) stage.entry = stage_entry, stage.hit = stage_hit, stage.ray_d = stage_ray_d, stage.meta = stage_meta;
        shade_body<KIND, SIMPLE, FT, PRE, true, SLOTS, GEO>(st, sc, T, fr, sob, depth, first_kind, stats, src, emit_list + (threadIdx.x >> 6) * 128, stash, stage);
    } else
        shade_body<KIND, SIMPLE, FT, PRE>(st, sc, T, fr, sob, depth, first_kind, stats, src, emit_list + (threadIdx.x >> 6) * 128);
}
