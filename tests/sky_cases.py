"""Shared by test_sky_edit_host.py (CPU) and test_sky_edit.py (GPU): the parameter set of the sky bake, the host reference of every
case (sunsky.sky_texels, computed once per session and never written to), the agreement metric, and the recorded bounds.

THE METRIC.  e = max over sky texels and channels of |got - reference| / (largest channel of the reference texel); ground texels and
alpha must be EQUAL.  A count of equal texels proves nothing (10 - 45 % differ in the last place) and is not tested.

WHAT IS HELD (LAB_NOTEBOOK.md, the sky bake, has the measurements behind it):
  * outside the dark family (104 cases): e against the NumPy bake within 4 x the recorded `host_lit` / `device_lit`, which must be <= 2e-5;
  * in the dark family (turbidity 10 under a sun at elevation <= 0.02, 16 cases): e against the NumPy bake within 4 x the recorded
    `host` / `device`.  That figure is the FLOOR of the metric there, not a property of hk_sky.h: it is what NumPy's Float32 arccos,
    which is not correctly rounded, turns into in nearly black texels.  It depends on the NumPy build that bakes the reference (an
    SVML arccos and glibc's acosf differ in the last place); with a correctly rounded arccos it would be about 2e-6.  A defect of that
    size would pass, so the family is ALSO held to <= 2e-5 against the texels hk_sky.h gave when built with g++
    (tests/golden/sky_dark_family_host_build.npz, ground off; the ground texels of the ground-on cases are the record's)."""
import functools
import itertools
import json
import os

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_FILE = os.path.join(ROOT, "tests", "golden", "sky_bake_bounds.json")
DARK_FILE = os.path.join(ROOT, "tests", "golden", "sky_dark_family_host_build.npz")
LIMIT = 2e-5                         # what the design asks of the device figure

RESOLUTIONS = (8, 33, 96)            # a single block; odd, no multiple of a wave or a block; 36 blocks, even (texel centres on the horizon)
SUNS = {
    "zenith": (0.0, 0.0, 1.0),
    "elevation_0.02": (float(np.cos(0.02) * np.cos(0.7)), float(np.cos(0.02) * np.sin(0.7)), float(np.sin(0.02))),
    "below_horizon": (0.6, 0.3, -0.4),           # the model's solar elevation is clipped to 0
    "oblique_a": (1.0, 2.0, 9.0),
    "oblique_b": (-0.7, 0.4, 0.35),
}
TURBIDITIES = (1.0, 2.5, 3.3, 10.0)  # 10: the `it < 10` branch is skipped; 2.5 and 3.3: fractional parts
GROUNDS = (True, False)
CASES = [dict(res=r, sun=s, turbidity=t, ground=g) for r, s, t, g in itertools.product(RESOLUTIONS, SUNS, TURBIDITIES, GROUNDS)]


def dark_family(c):
    """turbidity 10 under a sun at elevation <= 0.02: a nearly black, out-of-gamut sky (see the module docstring)"""
    return c["turbidity"] == 10.0 and c["sun"] in ("elevation_0.02", "below_horizon")


def worst_of(results):
    """results: [(case, e)] -> {"dark": (e, id), "lit": (e, id)}: the largest e inside and outside the dark family"""
    out = {}
    for key, keep in (("dark", dark_family), ("lit", lambda c: not dark_family(c))):
        out[key] = max(((e, case_id(c)) for c, e in results if keep(c)), default=(0.0, None))
    return out


def case_id(c):
    return "%d-%s-T%g-%s" % (c["res"], c["sun"], c["turbidity"], "ground" if c["ground"] else "sky")


def sky_kwargs(hk, c):
    return dict(direction=SUNS[c["sun"]], turbidity=c["turbidity"], ground_albedo=hk.RGBSpectrum(0.3, 0.25, 0.1), ground_enabled=c["ground"])


@functools.lru_cache(maxsize=None)
def _host(res, sun, turbidity, ground):
    import hikari_jl_amd as hk
    from hikari_jl_amd import sunsky
    c = dict(res=res, sun=sun, turbidity=turbidity, ground=ground)
    data = sunsky.sky_texels(resolution=res, **sky_kwargs(hk, c))
    cc = ((np.arange(1, res + 1, dtype=f32) - f32(0.5)) / f32(res)).astype(f32)
    wz = sunsky._equal_area_square_to_sphere_f32(*np.meshgrid(cc, cc))[2]
    is_ground = (wz <= 0) & bool(ground)
    data.setflags(write=False)
    is_ground.setflags(write=False)
    return data, is_ground


def host_texels(c):
    """-> (texels [res, res, 3] Float32 as data[v, u], mask of the ground texels): the host bake, shared and read-only."""
    return _host(c["res"], c["sun"], c["turbidity"], c["ground"])


def from_device_layout(flat, res):
    """res * res * 4 floats with texel (v, u) at [v + res * u] -> [v, u, 4]"""
    return np.asarray(flat, f32).reshape(res, res, 4).transpose(1, 0, 2)


def _agreement(got, ref, is_ground, c):
    assert got.shape == ref.shape[:2] + (4,)
    assert np.array_equal(got[..., 3], np.ones(ref.shape[:2], f32)), "alpha"
    assert np.array_equal(got[is_ground][:, :3], ref[is_ground]), "ground texels"
    if c["ground"] and c["res"] % 2 == 0:
        assert is_ground.sum() > ref.shape[0] * ref.shape[1] // 2        # the horizon's texels (w.z == +0) are ground
    g, h = got[~is_ground][:, :3].astype(np.float64), ref[~is_ground].astype(np.float64)
    assert np.isfinite(g).all() and len(g) > 0
    top = h.max(axis=1, keepdims=True)
    black = top[:, 0] == 0
    assert np.array_equal(g[black], h[black])                         # nothing to scale a black texel by
    return float((np.abs(g - h)[~black] / top[~black]).max()) if (~black).any() else 0.0


def agreement(got, c):
    """got: [res, res, 4] as data[v, u].  Asserts what must be equal; -> e of the metric against the NumPy bake."""
    host, is_ground = host_texels(c)
    return _agreement(got, host, is_ground, c)


@functools.lru_cache(maxsize=None)
def _dark_golden():
    with np.load(DARK_FILE) as z:
        return {k: z[k] for k in z.files}


def agreement_with_host_build(got, c):
    """The same for a case of the dark family against the recorded g++ build of hk_sky.h."""
    assert dark_family(c)
    host, is_ground = host_texels(c)
    ref = _dark_golden()["%d-%s" % (c["res"], c["sun"])].copy()
    ref[is_ground] = host[is_ground]
    return _agreement(got, ref, is_ground, c)


def check(results, dark_results, who):
    """results: [(case, e against NumPy)] of every case; dark_results: [(case, e against the recorded g++ build)] of the dark family.
    who: "host" or "device".  Prints the figures, then asserts what the module docstring says."""
    worst, recorded = worst_of(results), bounds()
    dark = max(((e, case_id(c)) for c, e in dark_results), default=(0.0, None))
    print("sky bake, %s: outside the dark family e = %.4g at %s (recorded %.4g); dark family %.4g at %s against NumPy (recorded floor %.4g), %.4g at %s against the g++ build"
          % ((who,) + worst["lit"] + (recorded[who + "_lit"],) + worst["dark"] + (recorded[who],) + dark))
    assert 0 < recorded[who + "_lit"] <= LIMIT and worst["lit"][0] <= 4 * recorded[who + "_lit"], worst
    assert recorded[who] > 0 and worst["dark"][0] <= 4 * recorded[who], worst
    assert dark[0] <= LIMIT, dark


def bounds():
    with open(BOUNDS_FILE) as f:
        return json.load(f)
