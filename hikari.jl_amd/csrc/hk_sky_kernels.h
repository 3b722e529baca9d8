// hk_sky_kernels.h — k_sky_texels: the texels of a Hosek-Wilkie sky baked into an environment map on the device
// (hk_scene_update_envmap_sky).  Part of the hk_kernels.hip translation unit; the arithmetic is hk_sky.h's, shared with the host check.
#pragma once

// ---------------------------------------------------------------------------------------------------
// One thread per texel, a pure function of (record, v_idx, u_idx): no LDS, no atomics, no wait.  Thread t takes v_idx = t % res,
// u_idx = t / res, so consecutive lanes run along the fastest index of DEnvMap::data ([y + height * x]) and a wave stores whole lines of
// float4.  The record (1224 bytes) is a kernel argument: wave-uniform, read through the scalar cache.  Per texel: 11 bands of two exp, a
// division, two sqrt in binary64, three acos / cos before them — FP64 VALU work, 16 bytes stored.  launch_envmap_tables follows on the
// same stream and reads what this wrote.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sky_texels(const SkyConsts S, int res, float4* __restrict__ data) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (unsigned)res * (unsigned)res) return;
    const int u_idx = (int)(t / (unsigned)res), v_idx = (int)(t - (unsigned)u_idx * (unsigned)res);
    const SkyTexel x = hk_sky_texel(S, v_idx, u_idx, res);
    data[t] = make_float4(x.r, x.g, x.b, x.a);
}
