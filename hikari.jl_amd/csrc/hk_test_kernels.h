// hk_test_kernels.h — sub-kernel entry points of the parity tests and their launchers: device functions of the product kernels run over plain
// arrays.  Part of the hk_kernels.hip translation unit (included after hk_launch_impl.h); nothing on a render path calls into this file.
#pragma once

// ---------------------------------------------------------------------------------------------------
// sub-kernel entry points used by the parity tests
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HK_TRACE_BLOCK) k_test_trace(DScene sc, int n, const float* o3, const float* d3, const float* tmax, float* out_t, int* out_prim,
                                                               float* out_uv) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * HK_LDS_STACK * 64];
    int* stack = lds_stack + (threadIdx.x >> 6) * (HK_LDS_STACK * 64);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned a = 0, b = 0;
        bool dummy;
        HitRec h = traverse<0, false>(sc, mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]), tmax[i], stack, lane_id(), a, b,
                                      dummy);
        out_t[i] = h.prim >= 0 ? h.t : INF_F;
        out_prim[i] = h.prim;
        out_uv[2 * i] = h.prim >= 0 ? h.u : 0.0f;
        out_uv[2 * i + 1] = h.prim >= 0 ? h.v : 0.0f;
    }
}
// hk_test_tri_geo: the geometry table's rows as surface_at reads them, or the shared function on the positions the device holds
__global__ void __launch_bounds__(256) k_test_tri_geo(DScene sc, int recompute, float4* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < sc.n_tris; i += gridDim.x * blockDim.x) {
        if (recompute) {
            v3 a, b, c;
            tri_vertices(sc, i, a, b, c);
            out[i] = tri_geo_of(a, b, c);
        } else
            out[i] = tri_geo_row(sc, i);
    }
}
__global__ void k_test_sobol(DTables T, DSobol sob, int n, const int* px, const int* py, const int* sidx, const int* dim, float* o1, float* o2) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        SobolCtx c = sobol_ctx(sob, T.sobol, px[i], py[i], sidx[i]);
        o1[i] = sobol_1d(c, dim[i]);
        v2 v = sobol_2d(c, dim[i]);
        o2[2 * i] = v.x;
        o2[2 * i + 1] = v.y;
    }
}
__global__ void k_test_camera(DTables T, DFilter flt, DCamera cam, DSobol sob, int height, int n, const int* px, const int* py, const int* sidx, float* out15) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int x = px[i], y = py[i];
        SobolCtx sc = sobol_ctx(sob, T.sobol, x, y, sidx[i]);
        float wu = sobol_1d(sc, 1);
        v2 jit = sobol_2d(sc, 3);
        float tu = sobol_1d(sc, 4);
        v2 lens = sobol_2d(sc, 6);
        float fx, fy, fw;
        filter_sample(flt, jit, fx, fy, fw);
        S4 lambda, pdf;
        sample_wavelengths_visible(wu, lambda, pdf);
        v2 pfilm = mk2((float)x + 0.5f + fx, (float)height - (float)y + 1.0f + 0.5f + fy);
        v3 ro, rd;
        float time;
        generate_ray(cam, pfilm, lens, tu, ro, rd, time);
        float* o = out15 + 15 * (size_t)i;
        o[0] = lambda.x; o[1] = lambda.y; o[2] = lambda.z; o[3] = lambda.w;
        o[4] = pdf.x; o[5] = pdf.y; o[6] = pdf.z; o[7] = pdf.w;
        o[8] = fw;
        o[9] = ro.x; o[10] = ro.y; o[11] = ro.z;
        o[12] = rd.x; o[13] = rd.y; o[14] = rd.z;
    }
}
__global__ void k_test_uplift(DTables T, int mode, int n, const float* rgb, const float* lam, float* out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        S4 l = s4(lam[4 * i], lam[4 * i + 1], lam[4 * i + 2], lam[4 * i + 3]);
        float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        S4 s = mode == 0 ? eval_bounded(coef_bounded(T, r, g, b), l) : (mode == 1 ? eval_scaled(coef_unbounded(T, r, g, b), l) : eval_illuminant(coef_illuminant(T, r, g, b), l));
        out[4 * i] = s.x;
        out[4 * i + 1] = s.y;
        out[4 * i + 2] = s.z;
        out[4 * i + 3] = s.w;
    }
}
__global__ void k_test_light_bvh(DScene sc, int n, const float* p3, const float* n3, const float* u, int* out_light, float* out_pmf, const int* query, float* out_qpmf) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        v3 p = mk3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]), nn = mk3(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]);
        float pmf;
        unsigned vis = 0;
        out_light[i] = bvh_sample_light(sc, p, nn, u[i], pmf, vis);
        out_pmf[i] = pmf;
        if (query) out_qpmf[i] = bvh_pmf(sc, p, nn, query[i], vis);
    }
}

// resolve_mix_material (mix-material.jl:222-238) for n hit points: out = index of the material a MixMaterial resolves to
__global__ void k_test_mix(DScene sc, int mat_idx, int n, const float* p3, const float* wo3, const float* uv2, int* out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = resolve_mix_material(sc, mat_idx, mk3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]), mk3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]), mk2(uv2[2 * i], uv2[2 * i + 1]));
}
// media: mode 0 = sample_point (media.jl:1327-1370, 1527-1575; nanovdb.jl:400-469) -> out[13] = sigma_a4, sigma_s4, Le4, g;
//        mode 1 = majorant iterator along a ray (media.jl:229-340, 625-729) -> out[1 + 3*HK_TEST_MAJ_SEGS] = segment count, then
//                 (t_min, t_max, sigma_maj[0]) of the first HK_TEST_MAJ_SEGS segments.  Same MM instantiation as the tracking kernels.
//        mode 2 = the same walk with majorant_skip_zero in front of every majorant_next (what the tracking kernels do): total
//                 segment count incl. the skipped ones, then the first HK_TEST_MAJ_SEGS segments that were NOT skipped.
#define HK_TEST_MAJ_SEGS 16
template <int MM>
__global__ void k_test_medium(DScene sc, DTables T, int mode, int medium_idx, int n, const float* a3, const float* b3, const float* tmax, const float* lambda, float* out) {
    const DMedium& med = sc.media[medium_idx];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const S4 l = s4(lambda[4 * i], lambda[4 * i + 1], lambda[4 * i + 2], lambda[4 * i + 3]);
        const v3 a = mk3(a3[3 * i], a3[3 * i + 1], a3[3 * i + 2]);
        const S4 base_a = eval_scaled(med.sigma_a, l), base_s = eval_scaled(med.sigma_s, l), base_Le = eval_scaled(med.Le, l);
        if (mode == 0) {
            MediumProps mp = sample_point<MM>(T, l, med, base_a, base_s, base_Le, a);
            float* r = out + 13 * (size_t)i;
            r[0] = mp.sigma_a.x, r[1] = mp.sigma_a.y, r[2] = mp.sigma_a.z, r[3] = mp.sigma_a.w;
            r[4] = mp.sigma_s.x, r[5] = mp.sigma_s.y, r[6] = mp.sigma_s.z, r[7] = mp.sigma_s.w;
            r[8] = mp.Le.x, r[9] = mp.Le.y, r[10] = mp.Le.z, r[11] = mp.Le.w;
            r[12] = mp.g;
        } else {
            const v3 d = mk3(b3[3 * i], b3[3 * i + 1], b3[3 * i + 2]);
            float* r = out + (1 + 3 * HK_TEST_MAJ_SEGS) * (size_t)i;
            for (int k = 0; k < 1 + 3 * HK_TEST_MAJ_SEGS; ++k) r[k] = 0.0f;
            MajorantIter it = create_majorant_iterator<MM>(med, a, d, tmax[i]);
            int count = 0, kept = 0;
            float t0, t1;
            S4 sm;
            for (;;) {
                if (mode == 2) majorant_skip_zero<MM>(it, med, count);   // fast-forward over zero cells (measured and not used by the kernels: DESIGN §5)
                if (count >= 256 || !majorant_next<MM>(it, med, base_a + base_s, t0, t1, sm)) break;
                // mode 1 records every segment, mode 2 the segments that survive the fast-forward (zero cells excluded)
                if (kept < HK_TEST_MAJ_SEGS) r[1 + 3 * kept] = t0, r[2 + 3 * kept] = t1, r[3 + 3 * kept] = sm.x;
                ++kept;
                ++count;
            }
            r[0] = (float)count;
        }
    }
}
// The traversal of the surfaces-only bench path: lane_ray_round (while-while rounds, straggler exit, LDS stack of STACK entries)
// driven by the same per-lane refill as k_trace_lean / k_shadow, over a plain ray array.  Every wave owns a contiguous range of
// rays.  ANYHIT = the shadow kernel's first-accepted-hit mode (out_prim >= 0 <=> occluded).
template <bool ANYHIT, int STACK, bool QN = false>
__global__ void __launch_bounds__(HK_TRACE_BLOCK) k_test_trace_lean(DScene sc, int n, const float* o3, const float* d3, const float* tmax, float* out_t, int* out_prim, float* out_uv) {
    __shared__ int lds_stack[(HK_TRACE_BLOCK / 64) * STACK * 64];
    int* stack = lds_stack + (threadIdx.x >> 6) * (STACK * 64);
    const int lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int DONE = (int)0x80000000;
    const int waves = physical_waves();
    const int per_wave = (n + waves - 1) / waves;
    const int first = global_wave() * per_wave;
    const int count = first >= n ? 0 : (n - first < per_wave ? n - first : per_wave);
    unsigned n_nodes = 0, n_tris = 0;
    int cursor = 0;
    bool have = false;
    int idx = 0;
    LaneRay r;
    r.cur = r.pend = DONE;
    for (;;) {
        const unsigned long long run_m = __ballot(have && r.cur != DONE);
        if (run_m == 0ull || (64 - __popcll(run_m) >= HK_TRACE_MIN_IDLE && cursor < count)) {
            if (have && r.cur == DONE) {
                out_t[idx] = r.best.prim >= 0 ? r.best.t : INF_F;
                out_prim[idx] = r.best.prim;
                out_uv[2 * idx] = r.best.prim >= 0 ? r.best.u : 0.0f;
                out_uv[2 * idx + 1] = r.best.prim >= 0 ? r.best.v : 0.0f;
                have = false;
            }
            const unsigned long long want = __ballot(!have);
            const int avail = count - cursor;
            const int rank = __popcll(want & lt_mask);
            if (!have && rank < avail) {
                idx = first + cursor + rank;
                lane_ray_start<QN>(r, sc, mk3(o3[3 * idx], o3[3 * idx + 1], o3[3 * idx + 2]), mk3(d3[3 * idx], d3[3 * idx + 1], d3[3 * idx + 2]), tmax[idx]);
                have = true;
            }
            const int want_n = __popcll(want);
            cursor += want_n < avail ? want_n : (avail > 0 ? avail : 0);
            if (__ballot(have) == 0ull) break;
        }
        lane_ray_round<ANYHIT, false, 0, (ANYHIT ? HK_POSTPONE_ANYHIT != 0 : HK_POSTPONE_CLOSEST != 0), false, QN>(r, have && r.cur != DONE, sc, stack, lane, n_nodes, n_tris);
    }
}

namespace hk {

template <int KIND>
__device__ void test_bsdf_one(const DScene& sc, const DTables& T, const DMaterial& m, int mode, bool regularize, v3 wo, v3 wi, v3 ns, S4 lambda, v2 u, float uc, float* r) {
    if (mode == 0) {
        BSDFSample b = sample_bsdf<KIND>(sc, T, m, wo, ns, mk2(0.0f, 0.0f), lambda, u, uc, regularize);
        r[0] = b.wi.x, r[1] = b.wi.y, r[2] = b.wi.z;
        r[3] = b.f.x, r[4] = b.f.y, r[5] = b.f.z, r[6] = b.f.w;
        r[7] = b.pdf, r[8] = b.is_specular ? 1.0f : 0.0f, r[9] = b.eta_scale;
    } else {
        float pdf;
        S4 f = eval_bsdf<KIND>(sc, T, m, wo, wi, ns, mk2(0.0f, 0.0f), lambda, pdf);
        r[0] = f.x, r[1] = f.y, r[2] = f.z, r[3] = f.w, r[4] = pdf;
        r[5] = r[6] = r[7] = r[8] = r[9] = 0.0f;
    }
}
__global__ void k_test_bsdf(DScene sc, DTables T, int mode, int mat_idx, int regularize, int n, const float* wo, const float* wi, const float* ns, const float* lambda,
                            const float* u, const float* uc, float* out) {
    const DMaterial& m = sc.materials[mat_idx];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    v3 o = mk3(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]), d = mk3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), nn = mk3(ns[3 * i], ns[3 * i + 1], ns[3 * i + 2]);
    S4 l = s4(lambda[4 * i], lambda[4 * i + 1], lambda[4 * i + 2], lambda[4 * i + 3]);
    v2 uu = mk2(u[2 * i], u[2 * i + 1]);
    float* r = out + 10 * (size_t)i;
#define HK_TB_CASE(K) \
    case K: test_bsdf_one<K>(sc, T, m, mode, regularize != 0, o, d, nn, l, uu, uc[i], r); break;
    switch (m.kind) {
        HK_TB_CASE(HK_MAT_MATTE)
        HK_TB_CASE(HK_MAT_MIRROR)
        HK_TB_CASE(HK_MAT_GLASS)
        HK_TB_CASE(HK_MAT_CONDUCTOR)
        HK_TB_CASE(HK_MAT_COATED_DIFFUSE)
        HK_TB_CASE(HK_MAT_THIN_DIELECTRIC)
        HK_TB_CASE(HK_MAT_DIFFUSE_TRANSMISSION)
        HK_TB_CASE(HK_MAT_COATED_DIFFUSE_TRANSMISSION)
        HK_TB_CASE(HK_MAT_COATED_CONDUCTOR)
        default: test_bsdf_one<HK_MAT_FALLBACK>(sc, T, m, mode, regularize != 0, o, d, nn, l, uu, uc[i], r); break;
    }
    }
#undef HK_TB_CASE
}
__global__ void k_test_light(DScene sc, DTables T, int mode, int light_idx, int n, const float* p3, const float* in3, const float* lambda, float* out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        S4 l = s4(lambda[4 * i], lambda[4 * i + 1], lambda[4 * i + 2], lambda[4 * i + 3]);
        v3 a = mk3(in3[3 * i], in3[3 * i + 1], in3[3 * i + 2]);
        float* r = out + 12 * (size_t)i;
        for (int k = 0; k < 12; ++k) r[k] = 0.0f;
        if (mode == 0) {
            LightSample ls = sample_light(sc, T, sc.lights[light_idx - 1], mk3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]), l, mk2(a.x, a.y));
            r[0] = ls.wi.x, r[1] = ls.wi.y, r[2] = ls.wi.z, r[3] = ls.pdf;
            r[4] = ls.Li.x, r[5] = ls.Li.y, r[6] = ls.Li.z, r[7] = ls.Li.w;
            r[8] = ls.p_light.x, r[9] = ls.p_light.y, r[10] = ls.p_light.z, r[11] = ls.is_delta ? 1.0f : 0.0f;
        } else {
            S4 Le = s4(0.0f);
            float pdf = 0.0f;
            for (int li = 0; li < sc.n_lights; ++li) {
                const DLight& L = sc.lights[li];
                if (L.kind == HK_LIGHT_AMBIENT) Le = Le + L.scale * light_spectrum(L, l);
                if (L.kind == HK_LIGHT_ENVIRONMENT) {
                    float4 t = env_eval(sc.envmaps[L.Le_tex], a);
                    Le = Le + eval_illuminant(coef_illuminant(T, t.x * L.Le_rgba[0], t.y * L.Le_rgba[1], t.z * L.Le_rgba[2]), l);
                    pdf = pdf + env_pdf_li(sc.envmaps[L.Le_tex], a);
                }
            }
            r[0] = Le.x, r[1] = Le.y, r[2] = Le.z, r[3] = Le.w, r[4] = pdf;
        }
    }
}
void launch_test_mix(hipStream_t s, const DScene& sc, int mat_idx, int n, const float* p3, const float* wo3, const float* uv2, int* out) {
    hipLaunchKernelGGL(k_test_mix, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, sc, mat_idx, n, p3, wo3, uv2, out);
}
void launch_test_medium(hipStream_t s, const DScene& sc, const DTables& T, int mode, int medium_idx, int n, const float* a3, const float* b3, const float* tmax, const float* lambda,
                        float* out) {
    with_int<1, 2, 4, 8, 15>(media_mask_class(sc), [&](auto MM) {   // the instantiation of the tracking kernels for this scene
        hipLaunchKernelGGL(k_test_medium<decltype(MM)::value>, dim3(grid_for(n, 64, 4096)), dim3(64), 0, s, sc, T, mode, medium_idx, n, a3, b3, tmax, lambda, out);
    });
}
int test_majorant_stride() { return 1 + 3 * HK_TEST_MAJ_SEGS; }
void launch_test_trace_lean(hipStream_t s, int n_cu, const DScene& sc, int anyhit, int n, const float* o, const float* d, const float* tmax, float* t, int* prim, float* uv) {
    const int blocks = n_cu * 2;
    with_bool(anyhit != 0, [&](auto A) {
        constexpr bool a = decltype(A)::value;
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(HK_TRACE_BLOCK), 0, s, sc, n, o, d, tmax, t, prim, uv); };
        if (sc.bvh_depth <= 16) launch(k_test_trace_lean<a, 16>);
        else if (sc.qnodes != nullptr) launch(k_test_trace_lean<a, HK_LDS_STACK, true>);   // the kernels' own choice for a deep tree: its quantised nodes
        else launch(k_test_trace_lean<a, HK_LDS_STACK>);
    });
}
void launch_test_tri_geo(hipStream_t s, const DScene& sc, int recompute, float4* out) {
    if (sc.n_tris > 0) hipLaunchKernelGGL(k_test_tri_geo, dim3(grid_for(sc.n_tris, 256, 8192)), dim3(256), 0, s, sc, recompute, out);
}
void launch_test_trace(hipStream_t s, const DScene& sc, int n, const float* o, const float* d, const float* tmax, float* t, int* prim, float* uv) {
    hipLaunchKernelGGL(k_test_trace, dim3(grid_for(n, HK_TRACE_BLOCK, 1280)), dim3(HK_TRACE_BLOCK), 0, s, sc, n, o, d, tmax, t, prim, uv);
}
void launch_test_sobol(hipStream_t s, const DTables& T, const DSobol& sob, int n, const int* px, const int* py, const int* si, const int* dim, float* o1, float* o2) {
    hipLaunchKernelGGL(k_test_sobol, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, T, sob, n, px, py, si, dim, o1, o2);
}
void launch_test_camera(hipStream_t s, const DTables& T, const DFilter& f, const DCamera& c, const DSobol& sob, int height, int n, const int* px, const int* py, const int* si,
                        float* out) {
    hipLaunchKernelGGL(k_test_camera, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, T, f, c, sob, height, n, px, py, si, out);
}
void launch_test_uplift(hipStream_t s, const DTables& T, int mode, int n, const float* rgb, const float* lam, float* out) {
    hipLaunchKernelGGL(k_test_uplift, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, T, mode, n, rgb, lam, out);
}
void launch_test_light_bvh(hipStream_t s, const DScene& sc, int n, const float* p, const float* nn, const float* u, int* ol, float* op, const int* q, float* oq) {
    hipLaunchKernelGGL(k_test_light_bvh, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, sc, n, p, nn, u, ol, op, q, oq);
}
void launch_test_bsdf(hipStream_t s, const DScene& sc, const DTables& T, int mode, int mat_idx, int regularize, int n, const float* wo, const float* wi, const float* ns,
                      const float* lambda, const float* u, const float* uc, float* out) {
    hipLaunchKernelGGL(k_test_bsdf, dim3(grid_for(n, 64, 4096)), dim3(64), 0, s, sc, T, mode, mat_idx, regularize, n, wo, wi, ns, lambda, u, uc, out);
}
void launch_test_light(hipStream_t s, const DScene& sc, const DTables& T, int mode, int light_idx, int n, const float* p3, const float* in3, const float* lambda, float* out) {
    hipLaunchKernelGGL(k_test_light, dim3(grid_for(n, 64, 4096)), dim3(64), 0, s, sc, T, mode, light_idx, n, p3, in3, lambda, out);
}

}  // namespace hk
