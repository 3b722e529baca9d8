// hk_wave_queues.h — what every stage shares: lane_id, the wave-private segmented queues (WaveQ), the segment tickets and the segment loops,
// the streaming loads / stores, the record loaders of a path generation, the HK_DBG* probes and the slot <-> pixel mapping.
// Part of the hk_kernels.hip translation unit, inside its anonymous namespace; the first of its headers (needs hk_device.h only).
#pragma once

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// Wave-private segmented queues: wave segment w owns entries [w*wave_cap, (w+1)*wave_cap) of every queue and the count word
// counts[..][w].  A path never leaves the segment that generated its camera ray, so compaction is pure ballot/popcount
// arithmetic: no atomics, no cursors, deterministic order.  (A single global queue counter serialises at ~88 atomics/us on this
// chip: 40 k wave-pushes per launch cost ~0.45 ms per kernel.)
struct WaveQ {
    uint32_t* base;
    int count;  // wave-uniform
};
// Wave index of the launch.  Everything that ties data to an XCD (static segment strides, ticket counters) assumes 4-wave blocks dealt
// round-robin over the 8 XCDs: wave g runs on XCD (g / 4) % 8.  A 16-wave block (k_trace_lean with its node cache) numbers its
// waves so that this still holds: it stands for the four 4-wave blocks vb = ((b / 8) * 4 + w / 4) * 8 + b % 8 (a bijection when
// the grid is a multiple of 8 blocks, which one block per CU is).
__device__ __forceinline__ int global_wave() {
    const int w = (int)(threadIdx.x >> 6), b = (int)blockIdx.x;
    if (blockDim.x == 1024 && (gridDim.x & 7) == 0) return ((((b >> 3) * 4 + (w >> 2)) * 8 + (b & 7)) << 2) + (w & 3);
    if (blockDim.x == 512 && (gridDim.x & 7) == 0) return ((((b >> 3) * 2 + (w >> 2)) * 8 + (b & 7)) << 2) + (w & 3);   // an 8-wave block (k_light_select_pool): two such 4-wave blocks
    return b * (int)(blockDim.x >> 6) + w;
}
__device__ __forceinline__ int physical_waves() { return (int)(gridDim.x * (blockDim.x >> 6)); }
// A kernel is launched with as many physical waves as are resident for ITS register/LDS budget; each physical wave walks the
// virtual wave segments.  Surface scenes walk them with a static stride (the grid is clamped to a divisor of W, see
// clamp_blocks: residency differs per kernel — 12 .. 28 waves per CU — and a stride that does not divide W leaves a tail round
// with a fraction of the waves busy).  Scenes with media, whose work per segment is wildly uneven (a tile that looks into a
// cloud vs one that sees the sky), hand the segments out through tickets: +9 % on the cloud config, -16 % on the sky config.
// One ticket = one atomic, and ONE WORD takes ~88 atomics/us on this chip: with a single ticket word a launch over W = 24 k
// segments cost 0.3 ms even when every segment was empty — the launch floor of the deep bounces of the cloud config in round 1
// (k_escaped / k_scatter / k_shade min 316 - 328 us).  Handing out several segments per ticket is no way out (4 per ticket made the
// shadow walk 48 % slower: tail).  The ticket is therefore split HK_TICKET_WAYS = 64 ways: counter k, in its own 256-byte line
// (so another memory channel), hands out the segments k, k + K, k + 2K, ...; a wave starts at counter (wave mod K) and moves on
// to the next live counter when one is exhausted, never to come back.  Same one-segment granularity and the same stealing
// behaviour, 1/K of the serialisation.
// WORK LISTS.  At the deep bounces most segments of a queue are empty (an open scene loses half of its paths per bounce), and a
// launch that visits all W segments pays a count-word round trip (plus a ticket) per empty one.  After every producer the host
// launches k_segment_lists, which writes, per queue, the ascending list of its non-empty segments and their number; consumers
// iterate over the list — statically (entry w, w + waves, ...) or by ticket — and never see an empty segment.
#ifndef HK_TICKET_REFRESH
#define HK_TICKET_REFRESH 0   // see seg_next
#endif
#ifndef HK_TICKET_OPEN_SHARED
#define HK_TICKET_OPEN_SHARED 1
#endif
struct SegTickets {
    int* cnt;                   // HK_TICKET_WAYS (= 64: one per lane) counters, HK_TICKET_STRIDE ints apart
    unsigned long long alive;   // counters not yet seen exhausted (wave-uniform)
    int k0;                     // where this wave starts looking
    const int* list;            // non-empty segments of the consumed queue, ascending (null: every segment 0 .. n - 1)
    int n;                      // entries to hand out
    int pos, step;              // static mode: next entry of this wave, stride (step == 0: ticket mode)
    unsigned long long own;     // ticket mode: the counters whose segments the static stride would give to this wave's XCD
    bool share;                 // ticket mode: exhausted counters are published in one shared word (seg_next)
};
// Static stride: block b runs on XCD b % 8 and its wave w takes the list entries 4b + w, 4b + w + waves, ...: the records one kernel
// writes are read by the next kernel from the SAME XCD's L2 while they are still there (the per-XCD L2s do not share).  Tickets keep
// that affinity: counter k hands out entries k, k + 64, ..., all congruent to k mod 32, so counter k "belongs" to XCD (k / 4) % 8; a wave
// draws from the eight counters of its own XCD first and steals from the others only when those are exhausted (sky scene: the
// deep, sparse bounces fit in L2 — shade +12 % slower with XCD-blind tickets).
__device__ __forceinline__ unsigned long long xcd_counters() {
    int x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    x &= 7;
    return (0xfull << (4 * x)) | (0xfull << (4 * x + 32));
}
__device__ __forceinline__ int seg_per_way(int n_segments, int k) { return (n_segments - k + HK_TICKET_WAYS - 1) / HK_TICKET_WAYS; }
__device__ __forceinline__ const int* seg_list_ptr(const DPathState& st, int depth, int q) { return st.seg_list + (size_t)(depth * Q_COUNT + q) * st.n_waves; }
// dynamic: all 64 counters are inspected with ONE parallel load (lane k reads counter k): an exhausted launch costs a wave one
// memory round trip and no atomic at all.  depth < 0: no list, every segment (the camera kernel).
__device__ __forceinline__ SegTickets seg_open(const DPathState& st, int* cnt, bool dynamic, int depth, int q) {
    SegTickets it;
    it.cnt = cnt;
    const bool lists = depth >= 0 && st.small_pass == 0;
    it.list = lists ? seg_list_ptr(st, depth, q) : nullptr;
    it.n = lists ? st.seg_list_n[depth * Q_COUNT + q] : st.n_waves;
    if (st.small_pass) dynamic = false;
    it.k0 = global_wave() & (HK_TICKET_WAYS - 1);
    it.pos = global_wave();
    it.step = dynamic ? 0 : physical_waves();
    it.alive = 0ull;
    it.own = 0ull;
    it.share = st.ticket_share != 0;
    if (dynamic) {
        it.own = xcd_counters();
        const int lane = lane_id();
#if HK_TICKET_OPEN_SHARED
        if (it.share) {   // the shared word says which counters are used up: one 8-byte read instead of 64 lines per wave and launch
            const unsigned long long m = __hip_atomic_load(reinterpret_cast<unsigned long long*>(cnt + 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
            it.alive = __ballot(0 < seg_per_way(it.n, lane)) & ~(((unsigned long long)hi << 32) | lo);
        } else
#endif
        {
            const int v = __hip_atomic_load(cnt + lane * HK_TICKET_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            it.alive = __ballot(v < seg_per_way(it.n, lane));
        }
    }
    return it;
}
__device__ __forceinline__ int seg_entry(const SegTickets& it, int i) { return it.list ? it.list[i] : i; }
__device__ __forceinline__ int seg_next(SegTickets& it, int n_segments) {   // -> segment index, or n_segments when none is left
    if (it.step != 0) {
        const int i = it.pos;
        if (i >= it.n) return n_segments;
        it.pos = i + it.step;
        return seg_entry(it, i);
    }
    while (it.alive != 0ull) {
        // first live counter at or after k0 (cyclically)
        const unsigned long long cand = (it.alive & it.own) != 0ull ? (it.alive & it.own) : it.alive;
        const unsigned long long rot = it.k0 == 0 ? cand : ((cand >> it.k0) | (cand << (64 - it.k0)));
        const int k = (it.k0 + __ffsll((long long)rot) - 1) & (HK_TICKET_WAYS - 1);
        const int per_k = seg_per_way(it.n, k);
        int t = 0;
        if (lane_id() == 0) t = atomicAdd(it.cnt + k * HK_TICKET_STRIDE, 1);
        t = __builtin_amdgcn_readfirstlane(t);
        it.k0 = k;
        if (t < per_k) return seg_entry(it, k + t * HK_TICKET_WAYS);
        // counters only grow: exhausted once, exhausted for good.  At the end of a launch every wave finds that out one failed atomic at
        // a time (up to 63 serial round trips).  HK_TICKET_REFRESH=1 re-reads all 64 counters with one parallel load after a failure
        // instead: the deep bounces of a 32-spp Cornell frame lose 20 - 30 us per launch, the 256-spp frame and the many-light frame gain
        // 0.5 %, but the 64 extra line reads per wave get in the way of the remaining atomics where launches are short and many — the
        // cloud frame +3.6 %, Cornell at 64 spp +3 % — so it stays off (round 4, interleaved on one box).  What does pay where launches are
        // short and many is ONE shared word of "exhausted" bits per ticket (DPathState::ticket_share): cloud frame -1.8 % (644 -> 633 ms,
        // three interleaved pairs); with seg_open reading that word instead of the 64 counters another -0.4 %, Cornell -0.5 %,
        // many-light -0.3 %.
#if HK_TICKET_REFRESH
        const int v = __hip_atomic_load(it.cnt + lane_id() * HK_TICKET_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        it.alive &= __ballot(v < seg_per_way(it.n, lane_id()));
#endif
        if (it.share) {   // one shared word per ticket (the unused second 128-B half of counter 0's 256 bytes): a wave that finds counter k
                          // exhausted says so and learns, with the same atomic, what the others have found
            unsigned long long m = 0ull;
            if (lane_id() == 0) m = __hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(it.cnt + 32), 1ull << k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
            it.alive &= ~(((unsigned long long)hi << 32) | lo);
        }
        it.alive &= ~(1ull << k);
    }
    return n_segments;
}
// depth / q: the queue the kernel consumes (its work list); depth < 0: all segments
#define HK_FOR_EACH_WAVE_SEGMENT(gw, st, ticket, depth, q)                                                        \
    for (SegTickets gw##_t = seg_open(st, ticket, (st).dynamic_segments != 0, depth, q); gw##_t.cnt; gw##_t.cnt = nullptr) \
        for (int gw = seg_next(gw##_t, (st).n_waves); gw < (st).n_waves; gw = seg_next(gw##_t, (st).n_waves))
// the same loop over a prepared source (seg_open's result, or seg_single: the stage bodies are shared with k_small_pass)
#define HK_FOR_EACH_SEGMENT_FROM(gw, st, tickets)                                                                  \
    for (SegTickets gw##_t = (tickets); gw##_t.cnt; gw##_t.cnt = nullptr)                                         \
        for (int gw = seg_next(gw##_t, (st).n_waves); gw < (st).n_waves; gw = seg_next(gw##_t, (st).n_waves))
// exactly the segment g (static mode: the counter pointer only says "open")
__device__ __forceinline__ SegTickets seg_single(const DPathState& st, int g) {
    SegTickets it;
    it.cnt = st.tickets;
    it.alive = 0ull;
    it.k0 = 0;
    it.list = nullptr;
    it.n = g + 1;
    it.pos = g;
    it.step = 1 << 30;
    it.own = 0ull;
    it.share = false;
    return it;
}
// A kernel whose lanes leave nothing behind in their segment (the shadow kernels: results go to L[slot]) does not have to drain its
// lanes at the end of every segment: it asks for one segment after another and the per-lane refill simply continues with the next
// segment's entries.  The only drain left is the one at the end of the launch (the shadow walk of the cloud config ran a third of
// its lane-slots empty in the tails of its ~1000-entry segments).
typedef SegTickets SegStream;
__device__ __forceinline__ SegStream stream_open(const DPathState& st, int* ticket, bool force_dynamic, int depth, int q) {
    return seg_open(st, ticket, force_dynamic || st.dynamic_segments != 0, depth, q);
}
__device__ __forceinline__ int stream_next(SegStream& s, int n_segments) { return seg_next(s, n_segments); }
// ticket words: row = bounce depth (row max_depth + 1: camera / film), column = kernel
enum { TK_TRACE = 0, TK_TRACK = 1, TK_SHADOW = 2, TK_ESCAPED = 3, TK_SCATTER = 4, TK_SHADE0 = 5, TK_SELECT = 1, TK_CAMERA = 0, TK_FILM = 1 };   // TK_SELECT shares TK_TRACK's column: k_light_select only runs in scenes without media
__device__ __forceinline__ int* ticket_ptr(const DPathState& st, int row, int col) { return st.tickets + (size_t)(row * HK_TICKET_COLS + col) * (HK_TICKET_WAYS * HK_TICKET_STRIDE); }
__device__ __forceinline__ WaveQ wq_open(uint32_t* q, const DPathState& st, int gw) { return WaveQ{q + (size_t)gw * st.wave_cap, 0}; }
__device__ __forceinline__ void wq_push(WaveQ& q, uint32_t value, bool active) {
    unsigned long long mask = __ballot(active);
    if (active) q.base[q.count + __popcll(mask & ((1ull << lane_id()) - 1ull))] = value;
    q.count += __popcll(mask);
}
// beta / r_u / r_l of generation entry p; `ones`: the depth-0 records of a scene without media hold the constant 1 implicitly
__device__ __forceinline__ S4 ld_throughput(const float4* arr, size_t p, bool ones) { return ones ? s4(1.0f) : ld4(&arr[p]); }
// r_u / r_l of generation entry p and the MIS weights of a shadow record, in either representation (DPathState::compact)
__device__ __forceinline__ S4 ld_ru(const DPathGen& g, size_t p, bool ones, bool compact) { return (ones || compact) ? s4(1.0f) : ld4(&g.r_u[p]); }
// (compact: r_l is one float and lives in the fourth word of the record's ray_d — the reference's ray.time, which this path never reads)
__device__ __forceinline__ S4 ld_rl(const DPathGen& g, size_t p, bool ones, bool compact) {
    if (ones) return s4(1.0f);
    if (compact) return s4(reinterpret_cast<const float*>(g.ray_d)[4 * p + 3]);
    return ld4(&g.r_l[p]);
}
// r_u / r_l of a record whose ray_d has ALREADY been stored with r_l.x in its fourth word when `compact` (the writers do that themselves)
__device__ __forceinline__ void st_ru_rl(const DPathGen& g, size_t p, S4 r_u, S4 r_l, bool compact) {
    if (!compact) {
        st4(&g.r_u[p], r_u);
        st4(&g.r_l[p], r_l);
    }
}
__device__ __forceinline__ void mul_rl(const DPathGen& g, size_t p, bool ones, float f, bool compact) {   // r_l[p] *= f
    if (compact) {
        float* w = reinterpret_cast<float*>(g.ray_d) + 4 * p + 3;
        *w = (ones ? 1.0f : *w) * f;
    } else
        st4(&g.r_l[p], ld_throughput(g.r_l, p, ones) * f);
}
__device__ __forceinline__ void st_shadow_weights(const DPathState& st, size_t rec, S4 ru, S4 rl) {
    if (st.compact)
        reinterpret_cast<float2*>(st.sh_ru)[rec] = make_float2(ru.x, rl.x);
    else {
        st4(&st.sh_ru[rec], ru);
        st4(&st.sh_rl[rec], rl);
    }
}
// COMPACT is a compile-time fact in the shadow kernels: k_shadow and k_shadow_walk<.., 0> only run in scenes without media
template <bool COMPACT>
__device__ __forceinline__ void ld_shadow_weights(const DPathState& st, size_t rec, S4& ru, S4& rl) {
    if (COMPACT) {
        const float2 w = reinterpret_cast<const float2*>(st.sh_ru)[rec];
        ru = s4(w.x);
        rl = s4(w.y);
    } else {
        ru = ld4(&st.sh_ru[rec]);
        rl = ld4(&st.sh_rl[rec]);
    }
}
// Streaming stores / loads of path and shadow records (written once, read once by a later kernel): marked non-temporal so that they
// do not push the register-spill lines of the resident waves out of the L2s (HK_NT=0 at build time: plain accesses)
#ifndef HK_NT
#define HK_NT 1
#endif
typedef uint32_t hk_u2v __attribute__((ext_vector_type(2)));
HKD void stream_st(float4* p, float4 v) {
#if HK_NT
    __builtin_nontemporal_store((hk_f4v){v.x, v.y, v.z, v.w}, (hk_f4v*)p);
#else
    *p = v;
#endif
}
HKD void stream_st(float4* p, S4 v) { stream_st(p, make_float4(v.x, v.y, v.z, v.w)); }
HKD void stream_st(uint2* p, uint2 v) {
#if HK_NT
    __builtin_nontemporal_store((hk_u2v){v.x, v.y}, (hk_u2v*)p);
#else
    *p = v;
#endif
}
HKD void stream_st(float* p, float v) {
#if HK_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
HKD void stream_st(uint32_t* p, uint32_t v) {
#if HK_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
HKD float4 stream_ld(const float4* p) {
#if HK_NT
    const hk_f4v v = __builtin_nontemporal_load((const hk_f4v*)p);
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
// The four wavelengths of a path never change after the camera drew them (TerminateSecondary is not part of the reference's path), so
// they are kept ONCE, by camera slot (lambda_s, which the film kernel needs anyway), instead of travelling with every generation
// record: 16 B less to write per continuing vertex and per camera ray, the same 16 B to read (slots of a queue ascend, so the reads
// stay nearly dense).  HK_LAMBDA_BY_SLOT=0 (hk_types.h) builds the round-2 layout (a copy in every generation) for A/B runs.
// Measured (round 3): films bit-identical; k_camera -5 %, k_shade unchanged (it is not bound by its bytes alone: DESIGN.md §5), 5 GB less
// path state at 164 M paths in flight.
__device__ __forceinline__ S4 ld_lambda(const DPathState& st, const DPathGen& g, size_t p, uint32_t pslot) {
#if HK_LAMBDA_BY_SLOT
    const float4 v = stream_ld(&st.lambda_s[pslot]);
#else
    const float4 v = stream_ld(&g.lambda[p]);
#endif
    return s4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_lambda(const DPathGen& g, size_t p, S4 lambda) {
#if !HK_LAMBDA_BY_SLOT
    stream_st(&g.lambda[p], lambda);
#endif
}
// lean generation records (DPathState::meta32 / const_origin): the record's meta word(s) and origin through one pair of accessors
__device__ __forceinline__ uint2 ld_meta(const DPathState& st, const DPathGen& g, size_t p, int depth) {
    if (st.meta32) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(g.meta)[p];
        return make_uint2((uint32_t)depth | (((w >> 30) & 1u) << 8) | ((w >> 31) << 9), w & 0x3fffffffu);
    }
    return g.meta[p];
}
__device__ __forceinline__ void st_meta(const DPathState& st, const DPathGen& g, size_t p, uint32_t flags, uint32_t slot) {
    if (st.meta32)
        stream_st(reinterpret_cast<uint32_t*>(g.meta) + p, slot | (((flags >> 8) & 1u) << 30) | (((flags >> 9) & 1u) << 31));
    else
        stream_st(&g.meta[p], make_uint2(flags, slot));
}
// const_origin: generation 0 keeps ONE origin per segment, at the segment's first entry `seg` (k_camera's lane with position 0 writes it),
// and every depth-0 reader of that segment loads that entry — one hot line instead of 16 B per path; no branch, no arithmetic repeated
__device__ __forceinline__ float4 ld_ray_o(const DPathState& st, const DPathGen& g, size_t p, int depth, size_t seg) {
    return stream_ld(&g.ray_o[(depth == 0 && st.const_origin) ? seg : p]);
}
// the generation the readers of bounce `depth` take their records from: the camera's for depth 0 (DPathState::gen_cam — gen[0] itself unless
// the state keeps the camera records across frames), else the ping-pong set that the shading of depth - 1 wrote
__device__ __forceinline__ DPathGen gen_at(const DPathState& st, int depth) { return depth == 0 ? st.gen_cam : st.gen[depth & 1]; }
// dense append of a whole record: the position the pushing lanes get inside the segment (count + rank among the pushing lanes)
struct WavePos {
    int count;  // wave-uniform: entries already in the segment
};
__device__ __forceinline__ int wp_push(WavePos& q, bool active) {   // returns this lane's position (valid where active)
    unsigned long long mask = __ballot(active);
    int pos = q.count + __popcll(mask & ((1ull << lane_id()) - 1ull));
    q.count += __popcll(mask);
    return pos;
}
__device__ __forceinline__ int* count_ptr(const DPathState& st, int depth, int q, int gw) { return st.counters + ((size_t)(depth * Q_COUNT + q) * st.n_waves + gw); }
__device__ __forceinline__ void wq_close(const WaveQ& q, int* cnt) {
    if (lane_id() == 0) *cnt = q.count;
}

#ifdef HK_DEBUG_UTIL
#define HK_DBG_DECL unsigned long long dbg_[32] = {0};
#define HK_DBG(i, active) do { dbg_[2 * (i)] += 64; dbg_[2 * (i) + 1] += __popcll(__ballot(active)); } while (0)
#define HK_DBG_FLUSH(stats) do { if (lane_id() == 0) for (int k_ = 0; k_ < 32; ++k_) (stats)->dbg[k_] += dbg_[k_]; } while (0)
#else
#define HK_DBG_DECL
#define HK_DBG(i, active) do { } while (0)
#define HK_DBG_FLUSH(stats) do { } while (0)
#endif
// per-wave statistics rows (summed on the host): plain read-modify-write, the row belongs to this wave
__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned v) {
    unsigned s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane_id() == 0 && s) *dst += (unsigned long long)s;
}

// Path slot of a pass -> (pixel slot, pass-sample k).  The samples of a pixel are ADJACENT slots (slot = pixel slot * S + k): a wave of
// camera rays is 64 samples of one pixel, the per-(pixel, dimension) sampler tables are read by neighbouring lanes, and k_film walks
// a contiguous run.  Division by the pass's sample count through a host-made reciprocal (DFrame::s_mul / s_shr, exact below 2^30).
__device__ __forceinline__ void split_slot(const DFrame& fr, uint32_t slot, int& pix, int& k) {
    const uint32_t q = (uint32_t)(((uint64_t)slot * fr.s_mul) >> fr.s_shr);
    pix = (int)q;
    k = (int)(slot - q * (uint32_t)fr.samples_in_pass);
}
__device__ __forceinline__ void slot_to_pixel(const DFrame& fr, int slot_in_sample, int& px, int& py, bool& inside) {
    int tile = slot_in_sample >> 6, l = slot_in_sample & 63;
    int tx = tile % fr.tiles_x, ty = tile / fr.tiles_x;
    px = fr.x0 + tx * 8 + (l & 7);
    py = fr.y0 + ty * 8 + (l >> 3);
    inside = px < fr.x1 && py < fr.y1;
}
