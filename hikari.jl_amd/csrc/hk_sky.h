// hk_sky.h — one texel of a Hosek-Wilkie sky baked into an equal-area environment map: the arithmetic of hk_scene_update_envmap_sky
// (the header states it), shared by the device kernel (k_sky_texels, hk_sky_kernels.h) and a stand-alone host check
// (tests/native/sky_texel_check.cpp builds it alone with g++, plain and under the sanitizers).  Plain C++, no device library.
//
// It follows sunsky.py (sky_texels), which follows lights/sun_sky.jl:87-190, 319-434: binary32 where the mirror computes in Float32 (the
// direction of the texel centre, cos gamma, the two arc cosines, the XYZ -> sRGB matrix), binary64 where it computes in Float64 (the
// model, the spectrum -> XYZ sum), nothing contracted (the library and the check are built with -ffp-contract=off).
//   - theta and gamma are BINARY32 values widened to double, as in the mirror (np.arccos of a Float32 array, then astype(float64)):
//     acos in double, rounded — the same number on host and device.  cos and sin of phi are taken the same way.
//   - x^1.5 is x * sqrt(x): sqrt is correctly rounded, so the product is within 1 ulp of binary64 of the power, and it costs a pow less.
// How far this is from the NumPy bake, and why: LAB_NOTEBOOK.md (the sky bake), tests/golden/sky_bake_bounds.json.
// Every band is evaluated once per texel; a wavelength between two bands interpolates their values.
#pragma once
#include <math.h>

#include "hikari_mi355x.h"

#if defined(__HIPCC__)
#define HK_SKY_HD __host__ __device__
#else
#define HK_SKY_HD
#endif

typedef hk_sky_params SkyConsts;   // the record of the entry point, passed to the kernel by value (wave-uniform)
struct SkyTexel {
    float r, g, b, a;
};

HK_SKY_HD inline float hk_sky_clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// centre of texel k (0-based) of `res` along one axis of the unit square
HK_SKY_HD inline float hk_sky_centre(int k, int res) { return ((float)(k + 1) - 0.5f) / (float)res; }

// equal_area_square_to_sphere of hk_device.h (textures/environment_map.jl:131-160) in binary32
HK_SKY_HD inline void hk_sky_direction(float pu, float pv, float w[3]) {
    const float u = 2.0f * pu - 1.0f, v = 2.0f * pv - 1.0f;
    const float up = fabsf(u), vp = fabsf(v);
    const float sd = 1.0f - (up + vp);
    const float r = 1.0f - fabsf(sd);
    const float phi = (r == 0.0f ? 1.0f : (vp - up) / r + 1.0f) * 3.14159265358979323846f / 4.0f;
    const float z = copysignf(1.0f - r * r, sd);
    const float cphi = (float)cos((double)phi), sphi = (float)sin((double)phi);
    const float rc = r * sqrtf(2.0f - r * r);
    w[0] = copysignf(cphi, u) * rc;
    w[1] = copysignf(sphi, v) * rc;
    w[2] = z;
}

// hosek_radiance (sun_sky.jl:127-140) of one band; ct = max(cos theta, 0), cg = cos gamma
HK_SKY_HD inline double hk_sky_band(const double* c, double ct, double cg, double gamma) {
    const double expM = exp(c[4] * gamma);
    const double rayM = cg * cg;
    const double den = 1.0 + c[8] * c[8] - 2.0 * c[8] * cg;
    const double mieM = (1.0 + cg * cg) / (den * sqrt(den));
    const double zenith = sqrt(ct);
    return (1.0 + c[0] * exp(c[1] / (ct + 0.01))) * (c[2] + c[3] * expM + c[5] * rayM + c[6] * mieM + c[7] * zenith);
}

HK_SKY_HD inline SkyTexel hk_sky_texel(const SkyConsts& S, int v_idx, int u_idx, int res) {
    float w[3];
    hk_sky_direction(hk_sky_centre(u_idx, res), hk_sky_centre(v_idx, res), w);
    SkyTexel out;
    out.a = 1.0f;
    if (S.ground_enabled && w[2] <= 0.0f) {   // +0 included: texel centres fall on the horizon at even res
        out.r = S.ground_rgb[0], out.g = S.ground_rgb[1], out.b = S.ground_rgb[2];
        return out;
    }
    const double theta = (double)(float)acos((double)hk_sky_clampf(w[2], 0.0f, 1.0f));
    const float cos_gamma = hk_sky_clampf((w[0] * S.sun_dir[0] + w[1] * S.sun_dir[1]) + w[2] * S.sun_dir[2], -1.0f, 1.0f);
    const double gamma = (double)(float)acos((double)cos_gamma);
    const double cg = cos(gamma), ct = fmax(cos(theta), 0.0);
    double F[11];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < 11; ++b) F[b] = hk_sky_band(S.config[b], ct, cg, gamma);
    double X = 0.0, Y = 0.0, Z = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 13; ++k) {   // 320 .. 720 nm; the band index and the weight are constants of k
        const double lambda = 320.0 + (double)k * (720.0 - 320.0) / 12.0;
        const double x = (lambda - 320.0) / 40.0;
        const int low = (int)floor(x);
        const double t = x - floor(x);
        double L = F[low] * S.radiance[low];
        if (!(t < 1e-6)) {
            L = (1.0 - t) * L;
            if (low + 1 < 11) L = L + t * F[low + 1] * S.radiance[low + 1];
        }
        X = X + L * S.xyz_weight[0][k];
        Y = Y + L * S.xyz_weight[1][k];
        Z = Z + L * S.xyz_weight[2][k];
    }
    const float Xf = (float)X, Yf = (float)Y, Zf = (float)Z;
    const float r = 3.2404542f * Xf - 1.5371385f * Yf - 0.4985314f * Zf;
    const float g = -0.9692660f * Xf + 1.8760108f * Yf + 0.0415560f * Zf;
    const float b = 0.0556434f * Xf - 0.2040259f * Yf + 1.0572252f * Zf;
    out.r = fmaxf(0.0f, r), out.g = fmaxf(0.0f, g), out.b = fmaxf(0.0f, b);
    return out;
}
