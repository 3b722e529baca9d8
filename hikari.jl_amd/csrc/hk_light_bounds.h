// hk_light_bounds.h — the arithmetic of a light-BVH REFIT (hk_scene_refit_lights): the union of two light bounds (light-bounds.jl:24-158,
// as light_bvh.cpp's cone_union / lb_union state it) and the record the device walks derived from a node (DLightNode, hk_types.h),
// shared by the device kernels (k_light_refit_leaves / k_light_refit_level, hk_edit_kernels.h) and their host twin
// (hk::refit_light_bvh, light_bvh.cpp; tests/native/light_refit_check.cpp builds it with g++, plain and under the sanitizers).
// Plain C++, no device library.
//
// The builder takes asin, acos, sin and cos from libm; the device has no function that returns libm's bits.  So the four functions the
// union needs are written HERE from binary32 + - * / sqrt alone: no libm, no ocml call (sqrtf is the correctly rounded instruction /
// expansion on both sides).  With -ffp-contract=off and correctly rounded division and square root — the flags of the Makefile —
// the gfx950 code, the host pass of hipcc and a plain g++ build give the same bits (the product library, that is: the Makefile's `fast`
// target contracts and takes the hardware's divide and square root in the device code, and its refit no longer equals the host twin).  What they do NOT give is the bits of a libm-built
// inner node: a refit cone differs from the built one in its last places (tests/golden/light_refit_bounds.json holds the measured
// distance and the functions' worst error against binary64).  Boxes, phi, cos_e and the two-sided bit involve no such function and
// are the builder's bits.
//   asin, acos   the rational approximation of fdlibm's e_asinf.c / e_acosf.c on [0, 0.5] and, above, through sqrt((1 - x) / 2)
//   sin, cos     an angle in [0, pi]: folded ONCE to [-pi / 4, pi / 4] (t, t - pi / 2 or pi - t, with pi and pi / 2 as two binary32 words
//                each), then the polynomials of fdlibm's k_sinf / k_cosf
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HK_LB_HD __host__ __device__
#else
#define HK_LB_HD
#endif

// a node as the builder holds it and hk_scene_light_bvh_copy hands it out: the layout of hk::LightBVHNodeH (bvh_build.h), 64 bytes
struct HkLightRaw {
    float bmin[3], bmax[3], w[3];
    float phi, cos_o, cos_e;
    uint32_t bits;              // bit0 two_sided, bit1 leaf
    uint32_t child1_or_light;   // leaf: the light, 1-based; inner node: not read by the refit
    uint32_t pad[2];
};
// the record the device walks: the layout of DLightNode / hk::LightNodeRec
struct HkLightWalk {
    float centre[3];
    float half_diag;
    float r2;
    float w[3];
    float phi, cos_o, cos_e, sin_o;
    uint32_t bits;
    uint32_t child1_or_light;
    uint32_t pad[2];
};

#define HK_LB_PI 3.14159265358979323846f
#define HK_LB_PI_LO (-8.74227766e-8f)        // pi - (double)HK_LB_PI
#define HK_LB_PIO2 1.57079632679489661923f
#define HK_LB_PIO2_LO (-4.37113883e-8f)      // pi / 2 - (double)HK_LB_PIO2

HK_LB_HD inline float hk_lb_min(float a, float b) { return a < b ? a : b; }
HK_LB_HD inline float hk_lb_max(float a, float b) { return a > b ? a : b; }
HK_LB_HD inline float hk_lb_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// R(z) of asin(x) = x + x R(x^2), |x| <= 0.5
HK_LB_HD inline float hk_lb_asin_r(float z) {
    const float p = z * (1.6666586697e-01f + z * (-4.2743422091e-02f + z * -8.6563630030e-03f));
    const float q = 1.0f + z * -7.0662963390e-01f;
    return p / q;
}
// asin of x in [0, 1] (the union calls it on half a chord of two unit vectors)
HK_LB_HD inline float hk_lb_asin(float x) {
    if (x <= 0.5f) return x + x * hk_lb_asin_r(x * x);
    const float z = (1.0f - x) * 0.5f;
    const float s = sqrtf(z);
    return (HK_LB_PIO2 - 2.0f * (s + s * hk_lb_asin_r(z))) + HK_LB_PIO2_LO;
}
// acos of x in [-1, 1]
HK_LB_HD inline float hk_lb_acos(float x) {
    if (x > 0.5f) {
        const float z = (1.0f - x) * 0.5f;
        const float s = sqrtf(z);
        return 2.0f * (s + s * hk_lb_asin_r(z));
    }
    if (x < -0.5f) {
        const float z = (1.0f + x) * 0.5f;
        const float s = sqrtf(z);
        return (HK_LB_PI - 2.0f * (s + s * hk_lb_asin_r(z))) + HK_LB_PI_LO;
    }
    return (HK_LB_PIO2 - (x + x * hk_lb_asin_r(x * x))) + HK_LB_PIO2_LO;
}
HK_LB_HD inline float hk_lb_ksin(float x) {   // |x| <= pi / 4
    const float z = x * x;
    return x + x * (z * (-1.6666667163e-01f + z * (8.3333337680e-03f + z * (-1.9841270114e-04f + z * (2.7557314297e-06f + z * -2.5050759689e-08f)))));
}
HK_LB_HD inline float hk_lb_kcos(float x) {   // |x| <= pi / 4
    const float z = x * x;
    return (1.0f - 0.5f * z) + z * (z * (4.1666667908e-02f + z * (-1.3888889225e-03f + z * (2.4801587642e-05f + z * (-2.7557314297e-07f + z * 2.0875723372e-09f)))));
}
// sin and cos of t in [0, pi] (a little outside does no harm: the fold is continuous)
HK_LB_HD inline void hk_lb_sincos(float t, float& s, float& c) {
    if (t <= 0.5f * HK_LB_PIO2) {
        s = hk_lb_ksin(t), c = hk_lb_kcos(t);
    } else if (t <= 1.5f * HK_LB_PIO2) {   // v = t - pi / 2 in [-pi / 4, pi / 4]: the difference of the leading words is exact
        const float v = (t - HK_LB_PIO2) - HK_LB_PIO2_LO;
        s = hk_lb_kcos(v), c = -hk_lb_ksin(v);
    } else {                               // v = pi - t
        const float v = (HK_LB_PI - t) + HK_LB_PI_LO;
        s = hk_lb_ksin(v), c = -hk_lb_kcos(v);
    }
}
HK_LB_HD inline float hk_lb_sin(float t) {
    float s, c;
    hk_lb_sincos(t, s, c);
    return s;
}
HK_LB_HD inline float hk_lb_cos(float t) {
    float s, c;
    hk_lb_sincos(t, s, c);
    return c;
}

struct HkLbVec {
    float x, y, z;
};
HK_LB_HD inline HkLbVec hk_lb_v(float x, float y, float z) {
    HkLbVec r;
    r.x = x, r.y = y, r.z = z;
    return r;
}
HK_LB_HD inline HkLbVec hk_lb_add(HkLbVec a, HkLbVec b) { return hk_lb_v(a.x + b.x, a.y + b.y, a.z + b.z); }
HK_LB_HD inline HkLbVec hk_lb_sub(HkLbVec a, HkLbVec b) { return hk_lb_v(a.x - b.x, a.y - b.y, a.z - b.z); }
HK_LB_HD inline HkLbVec hk_lb_mul(HkLbVec a, float s) { return hk_lb_v(a.x * s, a.y * s, a.z * s); }
HK_LB_HD inline float hk_lb_dot(HkLbVec a, HkLbVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
HK_LB_HD inline HkLbVec hk_lb_cross(HkLbVec a, HkLbVec b) { return hk_lb_v(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
HK_LB_HD inline float hk_lb_len(HkLbVec a) { return sqrtf(hk_lb_dot(a, a)); }
HK_LB_HD inline HkLbVec hk_lb_nrm(HkLbVec a) { return hk_lb_mul(a, 1.0f / hk_lb_len(a)); }

struct HkLbCone {
    HkLbVec w;
    float c;
};
// light_bvh.cpp's angle_between and cone_union over the functions above, statement for statement but for the axis (below)
HK_LB_HD inline float hk_lb_angle_between(HkLbVec a, HkLbVec b) {
    if (hk_lb_dot(a, b) < 0.0f) return HK_LB_PI - 2.0f * hk_lb_asin(hk_lb_clamp(hk_lb_len(hk_lb_add(a, b)) * 0.5f, 0.0f, 1.0f));
    return 2.0f * hk_lb_asin(hk_lb_clamp(hk_lb_len(hk_lb_sub(b, a)) * 0.5f, 0.0f, 1.0f));
}
HK_LB_HD inline HkLbCone hk_lb_cone_union(HkLbCone a, HkLbCone b) {
    if (a.c == INFINITY) return b;
    if (b.c == INFINITY) return a;
    const float ta = hk_lb_acos(hk_lb_clamp(a.c, -1.0f, 1.0f)), tb = hk_lb_acos(hk_lb_clamp(b.c, -1.0f, 1.0f));
    const float td = hk_lb_angle_between(a.w, b.w);
    if (hk_lb_min(td + tb, HK_LB_PI) <= ta) return a;
    if (hk_lb_min(td + ta, HK_LB_PI) <= tb) return b;
    const float to = (ta + td + tb) * 0.5f;
    HkLbCone sphere;
    sphere.w = hk_lb_v(0.0f, 0.0f, 1.0f), sphere.c = -1.0f;
    if (to >= HK_LB_PI) return sphere;
    const float tr = to - ta;
    const HkLbVec wr = hk_lb_cross(a.w, b.w);
    if (hk_lb_dot(wr, wr) == 0.0f) return sphere;
    // ONE statement more than the builder: the axis is made perpendicular to a.w again.  For nearly opposite axes a.w x b.w is rounding
    // noise and its direction anything — harmless only while the turn still happens in a plane through a.w: then the new axis is tr
    // from a.w and, b.w being nearly -a.w, pi - tr from b.w whatever the plane.  A kept topology pairs such lights (a face of an
    // emitter turned over next to its neighbour); a builder rarely does, it splits them apart.
    HkLbVec axis = hk_lb_nrm(wr);
    axis = hk_lb_sub(axis, hk_lb_mul(a.w, hk_lb_dot(axis, a.w)));
    if (hk_lb_dot(axis, axis) == 0.0f) return sphere;
    axis = hk_lb_nrm(axis);
    float s, c;
    hk_lb_sincos(tr, s, c);
    const HkLbVec w = hk_lb_add(hk_lb_add(hk_lb_mul(a.w, c), hk_lb_mul(hk_lb_cross(axis, a.w), s)), hk_lb_mul(hk_lb_mul(axis, hk_lb_dot(axis, a.w)), 1.0f - c));
    HkLbCone r;
    // and the cosine is stepped one to two ulps towards -1 (the cone a little wider): rounded to nearest, cos(to) may give the smaller
    // cone, and next to -1 one ulp of the cosine is 3.4e-4 rad of the angle — a bound should err to the outside
    const float ct = hk_lb_cos(to);
    const float wide = ct > 0.0f ? ct * (1.0f - 1.1920929e-7f) : (ct < 0.0f ? ct * (1.0f + 1.1920929e-7f) : -1.0e-30f);
    r.w = hk_lb_nrm(w), r.c = hk_lb_max(wide, -1.0f);
    return r;
}
// lb_union of two nodes; the result is an inner node (bit1 clear), its child1_or_light and pad words are zero
HK_LB_HD inline HkLightRaw hk_lb_union(const HkLightRaw& a, const HkLightRaw& b) {
    HkLightRaw r;
    if (a.phi == 0.0f) r = b;
    else if (b.phi == 0.0f) r = a;
    else {
        HkLbCone ca, cb;
        ca.w = hk_lb_v(a.w[0], a.w[1], a.w[2]), ca.c = a.cos_o;
        cb.w = hk_lb_v(b.w[0], b.w[1], b.w[2]), cb.c = b.cos_o;
        const HkLbCone c = hk_lb_cone_union(ca, cb);
        for (int k = 0; k < 3; ++k) r.bmin[k] = hk_lb_min(a.bmin[k], b.bmin[k]), r.bmax[k] = hk_lb_max(a.bmax[k], b.bmax[k]);
        r.w[0] = c.w.x, r.w[1] = c.w.y, r.w[2] = c.w.z;
        r.phi = a.phi + b.phi;
        r.cos_o = c.c;
        r.cos_e = hk_lb_min(a.cos_e, b.cos_e);
        r.bits = (a.bits | b.bits) & 1u;
    }
    r.bits &= 1u;
    r.child1_or_light = 0u;
    r.pad[0] = r.pad[1] = 0u;
    return r;
}
// the walked record of a node (light_bvh.cpp's light_node_record: the same binary32 operations in the same order); `child` is the
// light of a leaf, the entry of child 0 of an inner node
HK_LB_HD inline HkLightWalk hk_lb_walk_record(const HkLightRaw& n, uint32_t child) {
    HkLightWalk o;
    float c[3], dg[3], r[3];
    for (int k = 0; k < 3; ++k) {
        const float sum = n.bmin[k] + n.bmax[k];
        c[k] = sum * 0.5f;
        dg[k] = n.bmax[k] - n.bmin[k];
    }
    for (int k = 0; k < 3; ++k) r[k] = n.bmax[k] - c[k];
    for (int k = 0; k < 3; ++k) o.centre[k] = c[k];
    o.half_diag = sqrtf((dg[0] * dg[0] + dg[1] * dg[1]) + dg[2] * dg[2]) * 0.5f;
    o.r2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    for (int k = 0; k < 3; ++k) o.w[k] = n.w[k];
    o.phi = n.phi, o.cos_o = n.cos_o, o.cos_e = n.cos_e;
    const float om = 1.0f - n.cos_o * n.cos_o;
    o.sin_o = sqrtf(om > 0.0f ? om : 0.0f);
    o.bits = n.bits;
    o.child1_or_light = child;
    o.pad[0] = o.pad[1] = 0u;
    return o;
}
