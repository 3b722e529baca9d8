"""The light BVH refit on the device when lights are edited in place (hk_scene_refit_lights).  The contract: the topology of the tree
stays; the leaves of the edited lights are the builder's own leaves of the new records; every inner node on a path from an edited leaf
to the root is the union of its two children by the arithmetic of csrc/hk_light_bounds.h, which the host twin
(hk_test_light_refit_host) runs over the same arrays — so device and twin agree byte for byte; every other node keeps its bytes.
A refit tree is NOT the tree a fresh scene builds: both sample the same lights with another pmf, so films are compared byte for byte
only between routes to the same refit, and statistically against a fresh scene.

The figures the tests print — the worst cone residual over the libm-built trees of this file's scenes and over the refit trees, the
relMSE of the converged frame against a fresh scene and between two fresh renders — are recorded, as measured on one MI355X, in
tests/golden/light_refit_bounds.json; the bounds themselves are derived from the measurements of the run, not read from that file."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_volpath_np as R
import test_light_edits as E
import xform_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = E.W, E.H
PU = C.POINTER(C.c_uint32)
TREES = [1, 2, 3, 65, 300, 4096]
EDIT_SETS = ["one", "third", "all", "reversed"]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _emissive(hk, rng, two_sided):
    return hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)),
                              emission=hk.Emissive(Le=hk.RGBSpectrum(*(0.5 + 2.0 * rng.random(3))), scale=1.0 + float(rng.random()), two_sided=two_sided))


def _mixed(hk, n_tree, seed=7):
    """A Cornell room with n_tree lights in the tree — point, spot, one- and two-sided area lights, among them pairs with equal and with
    opposite axes (faces of normal -y and +y) — and, from 3 lights on, directional, ambient and zero-power lights scattered between."""
    from hikari_jl_amd.geometry import Mesh

    def build():
        rng = np.random.default_rng(seed)
        s = E._cornell(hk, "none", tess=6)()
        for i in range(n_tree):
            pos = rng.uniform((-0.8, 0.3, -0.8), (0.8, 1.8, 0.8))
            k = i % 6
            if k == 0:
                s.push(hk.PointLight(tuple(pos), hk.RGBSpectrum(*(1.0 + 4.0 * rng.random(3)))))
            elif k == 1:
                s.push(hk.SpotLight(tuple(pos), tuple(rng.uniform(-0.5, 0.5, 3) + (0, 0.8, 0)), hk.RGBSpectrum(*(5.0 + 10.0 * rng.random(3))), 20.0 + 40.0 * rng.random(), 10.0))
            else:
                a = 0.03 + 0.05 * rng.random()
                if k in (2, 3):      # axis-aligned faces: normals exactly -y (k = 2) and +y (k = 3)
                    tri = np.array([pos, pos + (a, 0, 0), pos + (0, 0, a if k == 2 else -a)], f32)
                else:
                    tri = np.array([pos, pos + a * rng.normal(size=3), pos + a * rng.normal(size=3)], f32)
                s.push(Mesh(tri[None], None, None), _emissive(hk, rng, two_sided=(k == 5)))
            if n_tree >= 3 and i % 4 == 2:   # lights outside the tree, scattered in the push order
                j = (i // 4) % 3
                if j == 0:
                    s.push(hk.DirectionalLight(hk.RGBSpectrum(0.3), tuple(rng.normal(size=3))))
                elif j == 1:
                    s.push(hk.AmbientLight(hk.RGBSpectrum(0.05)))
                else:
                    s.push(hk.PointLight(tuple(pos + 0.1), hk.RGBSpectrum(0.0)))
        s.sync()
        return s
    return build


def _emitter(hk, nu=64, nv=32):
    """A tessellated emitter under the ceiling: nu x nv x 2 = 4 096 area lights on a shallow dome (normals that differ from face to face)."""
    from hikari_jl_amd.geometry import Mesh

    def build():
        u, v = np.meshgrid(np.linspace(-0.8, 0.8, nu + 1), np.linspace(-0.8, 0.8, nv + 1), indexing="ij")
        P = np.stack([u, 1.9 - 0.4 * (u * u + v * v), v], axis=-1).astype(f32)
        a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
        tris = np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])
        s = E._cornell(hk, "none", tess=6)()
        s.push(hk.PointLight((0.1, 0.4, 0.2), hk.RGBSpectrum(2.0)))
        s.push(Mesh(np.ascontiguousarray(tris), None, None), _emissive(hk, np.random.default_rng(1), two_sided=False))
        s.sync()
        return s
    return build


def _build(hk, n_tree):
    return _emitter(hk)() if n_tree == 4096 else _mixed(hk, n_tree)()


# ---- records and trees ----------------------------------------------------------------------------------------------------------------
def _records(hk, s):
    d = s.desc
    return [hk._abi.hk_light.from_buffer_copy(d.lights[i]) for i in range(d.n_lights)]


def _edit_record(hk, rec, rng):
    """Another record of the same kind and the same membership in the tree: moved, re-coloured, turned."""
    A = hk._abi
    r = A.hk_light.from_buffer_copy(rec)
    gain = f32(0.5 + rng.random())
    for k in range(3):
        r.i_rgb[k] = float(f32(r.i_rgb[k]) * gain)
    if r.kind in (A.HK_LIGHT_POINT, A.HK_LIGHT_SPOT):
        for k in range(3):
            r.position[k] = float(f32(r.position[k] + rng.uniform(-0.2, 0.2)))
    if r.kind == A.HK_LIGHT_SPOT:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        r.light_to_world[2], r.light_to_world[6], r.light_to_world[10] = (float(f32(x)) for x in d)
    if r.kind == A.HK_LIGHT_DIFFUSE_AREA:
        shift = rng.uniform(-0.2, 0.2, 3)
        for k in range(9):
            r.v[k] = float(f32(r.v[k] + shift[k % 3]))
        if rng.random() < 0.4:                               # turned over: the cone's axis becomes the opposite one
            for k in range(3):
                r.normal[k] = -r.normal[k]
        if rng.random() < 0.3:
            r.two_sided = 1 - r.two_sided
        for k in range(3):
            r.Le.c[k] = float(f32(r.Le.c[k]) * gain)
    return r


def _edit_set(hk, recs, which, seed=5):
    """(flat indices, records): one light of the tree, a scattered third, all lights, all lights in reversed order."""
    rng = np.random.default_rng(seed)
    n = len(recs)
    if which == "one":
        in_tree = [i for i in range(n) if _in_tree(hk, recs[i])]
        idx = [in_tree[len(in_tree) // 2]]
    elif which == "third":
        idx = [i for i in range(n) if rng.random() < 1 / 3] or [0]
        idx = [int(i) for i in rng.permutation(idx)]
    else:
        idx = list(range(n))
        if which == "reversed":
            idx.reverse()
    new = {i: _edit_record(hk, recs[i], np.random.default_rng(1000 + i)) for i in idx}     # the record depends on the light alone, not on the set
    return idx, [new[i] for i in idx]


def _in_tree(hk, r):
    A = hk._abi
    if r.kind in (A.HK_LIGHT_POINT, A.HK_LIGHT_SPOT):
        return max(r.i_rgb[:3]) > 0 and r.scale > 0
    return r.kind == A.HK_LIGHT_DIFFUSE_AREA and r.area > 0 and max(r.Le.c[:3]) > 0


def _arr(hk, recs):
    return (hk._abi.hk_light * len(recs))(*recs)


def _refit(hk, sh, idx, recs):
    return hk._lib.lib().hk_scene_refit_lights(sh, len(idx), (C.c_int32 * len(idx))(*idx), _arr(hk, recs))


def _host(hk, lights, calls=()):
    """hk_test_light_refit_host: the tree built from `lights` after the refits `calls` = [(indices, records)] -> (nodes [n, 16], trails, table)."""
    L = hk._lib.lib()
    n = len(lights)
    call_n = (C.c_int32 * max(len(calls), 1))(*[len(i) for i, _ in calls])
    idx = [i for ii, _ in calls for i in ii]
    rec = [r for _, rr in calls for r in rr]
    nn = C.c_int32()
    nodes = np.zeros((2 * n, 16), f32)
    trails = np.zeros(n, np.uint32)
    table = np.zeros((2 * n, 16), np.uint32)
    hk._lib.check(L.hk_test_light_refit_host(_arr(hk, lights), n, len(calls), call_n, (C.c_int32 * max(len(idx), 1))(*idx), _arr(hk, rec) if rec else None, C.byref(nn),
                                             E._pf(hk, nodes), trails.ctypes.data_as(PU), table.ctypes.data_as(PU)), "hk_test_light_refit_host")
    return nodes[:nn.value].copy(), trails, table


def _device_tree(hk, ctx, s):
    n, nodes, trails = E._tree(hk, ctx, s)
    return np.frombuffer(nodes, f32).reshape(-1, 16)[:n].copy(), np.frombuffer(trails, np.uint32).copy()


def _device_table(hk, ctx, s):
    table = np.zeros((2 * max(s.desc.n_lights, 1), 16), np.uint32)
    hk._lib.check(hk._lib.lib().hk_test_light_table_copy(hk.scene_handle(ctx, s), table.ctypes.data_as(PU)), "hk_test_light_table_copy")
    return table


def _children(nodes):
    inner = nodes[:, 14] == 0
    i = np.nonzero(inner)[0]
    return i, i + 1, nodes[i, 13].astype(np.int64) - 1


def _dirty(nodes, lights_1based):
    """The nodes (host order) on the paths from the leaves of the given lights to the root."""
    n = len(nodes)
    parent = np.full(n, -1, np.int64)
    i, c0, c1 = _children(nodes)
    parent[c0], parent[c1] = i, i
    dirty = np.zeros(n, bool)
    want = set(int(x) for x in lights_1based)
    for leaf in np.nonzero(nodes[:, 14] > 0)[0]:
        if int(nodes[leaf, 13]) in want:
            k = leaf
            while k >= 0 and not dirty[k]:
                dirty[k] = True
                k = parent[k]
    return dirty


def _cone_residual(nodes):
    """Worst angle(w, w_c) + theta_c - theta over the inner nodes and both children, in float64 from the stored binary32 (0: all hold)."""
    i, c0, c1 = _children(nodes)
    i_keep = nodes[i, 10] > -1.0                             # the whole sphere holds everything
    worst = 0.0
    nd = nodes.astype(np.float64)
    theta = lambda c: np.arccos(np.clip(c, -1.0, 1.0))
    for c in (c0, c1):
        a, b = nd[i, 6:9], nd[c, 6:9]
        ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))
        r = ang + theta(nd[c, 10]) - theta(nd[i, 10])
        if i_keep.any():
            worst = max(worst, float(r[i_keep].max()))
    return worst


def _check_exact_invariants(nodes):
    i, c0, c1 = _children(nodes)
    assert np.array_equal(nodes[i, 0:3], np.minimum(nodes[c0, 0:3], nodes[c1, 0:3])) and np.array_equal(nodes[i, 3:6], np.maximum(nodes[c0, 3:6], nodes[c1, 3:6]))
    assert np.array_equal(nodes[i, 9], (nodes[c0, 9] + nodes[c1, 9]).astype(f32))
    assert np.array_equal(nodes[i, 11], np.minimum(nodes[c0, 11], nodes[c1, 11]))
    assert np.array_equal(nodes[i, 12] > 0, (nodes[c0, 12] > 0) | (nodes[c1, 12] > 0))
    assert np.allclose(np.linalg.norm(nodes[i, 6:9].astype(np.float64), axis=1), 1.0, atol=1e-5)


@pytest.fixture(scope="module")
def slack(hk):
    """The MEASURED slack of the cone test: the worst residual over the libm-built trees of this file's scenes — as pushed, and built
    from each edit set's records (host builds: hk_scene_create's code path, no device).  A refit tree may reach 4 x that (the issue's
    bar), plus 1e-6 rad where the built tree of the same lights has none."""
    worst, per = 0.0, {}
    for n in TREES:
        recs = _records(hk, _build(hk, n))
        per[(n, None)] = _cone_residual(_host(hk, recs)[0])
        for which in EDIT_SETS:
            idx, new = _edit_set(hk, recs, which)
            edited = list(recs)
            for i, r in zip(idx, new):
                edited[i] = r
            per[(n, which)] = _cone_residual(_host(hk, edited)[0])
    worst = max(per.values())
    print("libm-built trees: worst cone residual %.6g rad" % worst)
    return worst, per


# ---- twin, walked records, invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", EDIT_SETS)
@pytest.mark.parametrize("n_tree", TREES)
def test_refit_tree_equals_the_host_twin_and_holds_the_invariants(hk, gpu_ctx, slack, n_tree, which):
    s = _build(hk, n_tree)
    sh = hk.scene_handle(gpu_ctx, s)
    recs = _records(hk, s)
    built, trails0 = _device_tree(hk, gpu_ctx, s)
    assert (trails0 != 0xFFFFFFFF).sum() == (n_tree if n_tree != 4096 else 4097) and len(built) == 2 * (trails0 != 0xFFFFFFFF).sum() - 1
    if n_tree == 1:
        assert built[0, 14] == 1                             # the root is a leaf
    h_nodes, h_trails, h_table = _host(hk, recs)
    assert np.array_equal(built.view(np.uint32), h_nodes.view(np.uint32)) and np.array_equal(_device_table(hk, gpu_ctx, s), h_table)   # the starting point is common
    idx, new = _edit_set(hk, recs, which)
    assert _refit(hk, sh, idx, new) == 0, hk._lib.lib().hk_last_error()
    got, trails1 = _device_tree(hk, gpu_ctx, s)
    want, _, want_table = _host(hk, recs, [(idx, new)])
    # twin: tree and walked table byte for byte, trails untouched
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_device_table(hk, gpu_ctx, s), want_table)
    assert np.array_equal(trails1, trails0)
    assert np.array_equal(got[:, 13:15], built[:, 13:15])    # topology
    # off the dirty paths nothing moved
    dirty = _dirty(built, [i + 1 for i in idx])
    assert np.array_equal(got[~dirty].view(np.uint32), built[~dirty].view(np.uint32))
    assert dirty.any() == any(trails0[i] != 0xFFFFFFFF for i in idx) and (which != "one" or n_tree < 65 or 0 < dirty.sum() < len(built) // 4)
    # edited leaves are the leaves of a tree built from the edited description
    edited = list(recs)
    for i, r in zip(idx, new):
        edited[i] = r
    fresh = _host(hk, edited)[0]
    leaf_of = lambda t: {int(r[13]): r.view(np.uint32)[:13].tobytes() for r in t[t[:, 14] > 0]}
    mine, theirs = leaf_of(got), leaf_of(fresh)
    assert set(mine) == set(theirs)
    for i in idx:
        if i + 1 in mine:
            assert mine[i + 1] == theirs[i + 1], i
    # invariants, in float64 from the copied tree
    _check_exact_invariants(got)
    worst, per = slack
    r = _cone_residual(got)
    own = per[(n_tree, which)]
    print("tree %d, edit %s: cone residual refit %.6g, built from the same records %.6g, bound %.6g" % (n_tree, which, r, own, 4 * worst + (0 if own > 0 else 1e-6)))
    assert r <= 4 * worst + (0.0 if own > 0 else 1e-6)
    # walked records: the device's selections on the refit table against the NumPy walk of the copied tree (test_light_bvh_parity's bar)
    li, pmf, qp = E._select(hk, gpu_ctx, s)
    ref = R.LightBVH.__new__(R.LightBVH)
    ref.inf = np.array([i + 1 for i in range(len(recs)) if recs[i].kind not in (hk._abi.HK_LIGHT_POINT, hk._abi.HK_LIGHT_SPOT, hk._abi.HK_LIGHT_DIFFUSE_AREA)], np.int64)
    ref.n = int((trails1 != 0xFFFFFFFF).sum())
    ref.adopt(got, trails1)
    rng = np.random.default_rng(2)                           # _select's points
    n = 300
    p = rng.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3)).astype(f32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[::4] = 0
    u = rng.random(n).astype(f32)
    rl, rpmf = ref.sample(p, nrm, u)
    same = li == rl
    assert same.mean() > 0.999
    assert np.allclose(pmf[same], rpmf[same], rtol=2e-5, atol=0)
    query = (1 + np.arange(n) % len(recs)).astype(np.int64)
    bounded = trails1[query - 1] != 0xFFFFFFFF
    assert np.allclose(qp[bounded], ref.pmf(p[bounded], nrm[bounded], query[bounded]), rtol=2e-5, atol=1e-12)


def test_host_built_tree_is_the_tree_of_a_fresh_scene(hk, gpu_ctx):
    """What the tests above take as "the tree a fresh scene has": hk_test_light_refit_host without a refit is hk_scene_create's tree."""
    s = _build(hk, 65)
    recs = _records(hk, s)
    idx, new = _edit_set(hk, recs, "all")
    for i, r in zip(idx, new):
        s.desc.lights[i] = r
        recs[i] = r
    nodes, trails = _device_tree(hk, gpu_ctx, s)             # created here, from the edited description
    h_nodes, h_trails, h_table = _host(hk, recs)
    assert np.array_equal(nodes.view(np.uint32), h_nodes.view(np.uint32)) and np.array_equal(trails, h_trails) and np.array_equal(_device_table(hk, gpu_ctx, s), h_table)


# ---- routes ---------------------------------------------------------------------------------------------------------------------------
def _state(hk, ctx, s):
    nodes, trails = _device_tree(hk, ctx, s)
    return nodes.tobytes(), trails.tobytes(), _device_table(hk, ctx, s).tobytes(), E._film(hk, s).tobytes()


@pytest.mark.parametrize("n_tree", [3, 65])
def test_one_call_many_calls_and_another_order_give_the_same_scene(hk, gpu_ctx, n_tree):
    states = []
    for route in ("one call", "one light per call", "shuffled", "twice"):
        s = _build(hk, n_tree)
        sh = hk.scene_handle(gpu_ctx, s)
        recs = _records(hk, s)
        idx, new = _edit_set(hk, recs, "third")
        if route == "one call":
            assert _refit(hk, sh, idx, new) == 0
        elif route == "one light per call":
            for i, r in zip(idx, new):
                assert _refit(hk, sh, [i], [r]) == 0
        elif route == "shuffled":
            order = np.random.default_rng(9).permutation(len(idx))
            assert _refit(hk, sh, [idx[k] for k in order], [new[k] for k in order]) == 0
        else:                                                # other records first, then the final ones: the last record of a light counts
            other = [_edit_record(hk, recs[i], np.random.default_rng(77 + i)) for i in idx]
            assert _refit(hk, sh, idx, other) == 0 and _refit(hk, sh, idx, new) == 0
        states.append(_state(hk, gpu_ctx, s))
    assert all(st == states[0] for st in states[1:])


def test_rebuild_after_a_refit_is_a_fresh_scene(hk, gpu_ctx):
    s = _build(hk, 65)
    sh = hk.scene_handle(gpu_ctx, s)
    recs = _records(hk, s)
    idx, new = _edit_set(hk, recs, "third")
    assert _refit(hk, sh, idx, new) == 0
    refit_tree = _device_tree(hk, gpu_ctx, s)[0]
    for i, r in zip(idx, new):
        recs[i] = r
    assert hk._lib.lib().hk_scene_update_lights(sh, 0, 1, C.byref(recs[0])) == 0    # one unchanged record: the rebuild reads the scene's records
    f = _build(hk, 65)
    for i, r in enumerate(recs):
        f.desc.lights[i] = r
    for i, r in zip(idx, new):
        s.desc.lights[i] = r                                 # (the mirror's description of s, for _select's light count only)
    E._same_scene(hk, gpu_ctx, s, f)
    assert np.array_equal(_device_table(hk, gpu_ctx, s), _device_table(hk, gpu_ctx, f))
    assert not np.array_equal(refit_tree.view(np.uint32), _device_tree(hk, gpu_ctx, s)[0].view(np.uint32))   # the refit cones were not libm's
    # and the scene can be refit again, from the rebuilt tree
    idx2, new2 = _edit_set(hk, recs, "one")
    assert _refit(hk, sh, idx2, new2) == 0
    assert np.array_equal(_device_tree(hk, gpu_ctx, s)[0].view(np.uint32), _host(hk, recs, [(idx2, new2)])[0].view(np.uint32))


# ---- the mirror on the device -------------------------------------------------------------------------------------------------------
def _lamp_room(hk):
    """A small Cornell room with a tessellated emitter of 32 area lights in three instances and a point light."""
    from hikari_jl_amd.geometry import Mesh
    s = E._cornell(hk, "none", tess=8)()
    s.push(hk.PointLight((0.5, 1.5, -0.4), hk.RGBSpectrum(3.0, 2.5, 1.5)))
    y, insts = 1.9, []
    xs = np.linspace(-0.4, 0.4, 17)
    quads = []
    for a, b in zip(xs[:-1], xs[1:]):
        quads += [[(a, y, -0.2), (b, y, -0.2), (b, y, 0.2)], [(a, y, -0.2), (b, y, 0.2), (a, y, 0.2)]]
    tris = np.array(quads, f32)
    em = lambda: hk.MediumInterface(hk.MatteMaterial(Kd=hk.RGBSpectrum(0.0)), emission=hk.Emissive(Le=hk.RGBSpectrum(4.0), scale=1.0, two_sided=False))
    for part in (tris[:11], tris[11:22], tris[22:]):
        insts.append(s.push_instance(Mesh(np.ascontiguousarray(part), None, None), em()))
    s.sync()
    assert s.desc.n_lights == 33
    return s, insts


def _lamp_edits(hk, s, insts, tree, move):
    from hikari_jl_amd import lights as LT
    M = X.affine(rot_deg=35, axis=(0.2, 0.1, 1), scale=1.0, translate=(-0.1, -0.5, 0.2))
    s.set_transform(insts[0], M, move_lights=move)                                                    # a third of the emitter moved and turned, its lights with it
    pairs = [(0, hk.PointLight((-0.5, 1.2, 0.3), hk.RGBSpectrum(1.0, 2.0, 3.5)))]
    for i in range(12, 33, 3):                                                                        # re-coloured
        l = s.lights[i]
        pairs.append((i, LT.DiffuseAreaLight(l.vertices, l.normal, l.area, l.uv, hk.RGBSpectrum(6.0, 3.0, 1.0), 0.7, False)))
    s.update_lights(pairs, tree=tree)


def _film_seeded(hk, s, spp, seed):
    """E._film with the integrator's sampler_seed set."""
    film = hk.Film((W, H))
    cam = E._camera(hk, film)
    vp = hk.VolPath(max_depth=5, samples=spp)
    vp.params.sampler_seed = seed
    vp._ensure(film)
    vp.clear()
    vp.render_samples(s, film, cam, spp, first=1, readback=False)
    acc = vp.read_accumulators(film).copy()
    vp.close()
    return acc


def _rel_mse(a, b):
    n = 3 * W * H
    a, b = a[:n].astype(np.float64), b[:n].astype(np.float64)
    return float(np.mean((a - b) ** 2 / (b * b + 1e-2 * np.mean(b) ** 2)))


def test_converged_frame_of_a_refit_scene_equals_a_fresh_scene_up_to_noise(hk, gpu_ctx):
    """Both trees are unbiased: at 256 spp only noise separates the refit scene from a fresh scene of the edited description.  The bar
    is 2 x the relMSE of two fresh renders that differ in sampler_seed."""
    s, insts = _lamp_room(hk)
    hk.scene_handle(gpu_ctx, s)
    _lamp_edits(hk, s, insts, "refit", "refit")
    f, finsts = _lamp_room(hk)
    _lamp_edits(hk, f, finsts, "rebuild", True)              # before its device scene exists: created from the edited description
    assert [bytes(s.desc.lights[i]) for i in range(33)] == [bytes(f.desc.lights[i]) for i in range(33)]
    refit, fresh, fresh2 = _film_seeded(hk, s, 256, 0), _film_seeded(hk, f, 256, 0), _film_seeded(hk, f, 256, 1)
    assert not np.array_equal(fresh, fresh2)                 # the seed reached the integrator
    assert not np.array_equal(_device_tree(hk, gpu_ctx, s)[0].view(np.uint32), _device_tree(hk, gpu_ctx, f)[0].view(np.uint32))
    got, noise = _rel_mse(refit, fresh), _rel_mse(fresh2, fresh)
    print("relMSE at 256 spp: refit against fresh %.6g, fresh against fresh of another seed %.6g" % (got, noise))
    assert fresh[:3 * W * H].max() > 0 and noise > 0
    assert got <= 2 * noise


def test_refit_is_ordered_after_noted_calls(hk, gpu_ctx):
    """A noted one-sample call renders the lights as they were when the call was made; the next one sees the refit ones."""
    old = [w for _, w in E.POINTS]
    new_light = lambda: hk.PointLight((0.2, 1.7, 0.4), hk.RGBSpectrum(0.0, 12.0, 2.0))

    def refit_scene():
        t = E._three_points(hk, old)()
        hk.scene_handle(gpu_ctx, t)
        t.update_light(1, new_light(), tree="refit")
        return t

    s, s_old, s_new = E._three_points(hk, old)(), E._three_points(hk, old)(), refit_scene()
    hk.scene_handle(gpu_ctx, s)

    def run(first, then, edit):
        film = hk.Film((W, H))
        cam = E._camera(hk, film)
        vp = hk.VolPath(**E.KW)
        vp._ensure(film)
        vp.clear()
        vp.render_samples(first, film, cam, 1, first=1, readback=False)      # noted, not yet rendered
        if edit:
            s.update_light(1, new_light(), tree="refit")
        vp.render_samples(then, film, cam, 1, first=2, readback=False)
        acc = vp.read_accumulators(film).copy()
        vp.close()
        return acc

    got = run(s, s, True)
    assert np.array_equal(got, run(s_old, s_new, False))
    assert not np.array_equal(got, run(s_new, s_new, False)) and not np.array_equal(got, run(s_old, s_old, False))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_refits_leave_the_scene_untouched(hk, gpu_ctx):
    A = hk._abi
    L = hk._lib.lib()
    s = _build(hk, 65)
    sh = hk.scene_handle(gpu_ctx, s)
    recs = _records(hk, s)
    n = len(recs)
    point = next(i for i in range(n) if recs[i].kind == A.HK_LIGHT_POINT and _in_tree(hk, recs[i]))
    dark = next(i for i in range(n) if recs[i].kind == A.HK_LIGHT_POINT and not _in_tree(hk, recs[i]))
    area = next(i for i in range(n) if recs[i].kind == A.HK_LIGHT_DIFFUSE_AREA)
    ambient = next(i for i in range(n) if recs[i].kind == A.HK_LIGHT_AMBIENT)
    assert _refit(hk, sh, [point, dark, ambient], [recs[point], recs[dark], recs[ambient]]) == 0      # the refit arrays exist from here on
    state = lambda: (_state(hk, gpu_ctx, s), [x.tobytes() for x in E._select(hk, gpu_ctx, s)], E._light(hk, gpu_ctx, s, 0, point + 1).tobytes())
    before = state()
    copy = lambda i: A.hk_light.from_buffer_copy(recs[i])

    def refused(idx, new, text):
        assert _refit(hk, sh, idx, new) == A.HK_ERR_INVALID
        assert text in L.hk_last_error(), L.hk_last_error()

    r = copy(point)
    r.kind = A.HK_LIGHT_SPOT
    refused([point], [r], b"kind differs")
    refused([point, area, point], [recs[point], recs[area], recs[point]], b"given twice")
    refused([n], [recs[point]], b"outside the scene")
    refused([-1], [recs[point]], b"outside the scene")
    r = copy(area)
    r.v[4] = float("nan")
    refused([area], [r], b"non-finite")
    r = copy(point)
    r.position[0] = float("inf")
    refused([point], [r], b"non-finite")
    r = copy(dark)
    r.i_rgb[0] = r.i_rgb[1] = r.i_rgb[2] = 2.0                # phi 0 -> positive
    refused([dark], [r], b"hk_scene_update_lights")
    assert b"enter the light tree" in L.hk_last_error()
    r = copy(point)
    r.i_rgb[0] = r.i_rgb[1] = r.i_rgb[2] = 0.0                # phi positive -> 0
    refused([area, point], [recs[area], r], b"hk_scene_update_lights")
    assert b"leave the light tree" in L.hk_last_error()
    assert L.hk_scene_refit_lights(sh, 1, None, _arr(hk, [recs[point]])) == A.HK_ERR_INVALID
    assert L.hk_scene_refit_lights(sh, 0, (C.c_int32 * 1)(0), _arr(hk, [recs[point]])) == A.HK_ERR_INVALID
    assert state() == before
    # h_lights-derived copies: a rebuild from the scene's records gives the scene as created
    assert L.hk_scene_update_lights(sh, point, 1, C.byref(recs[point])) == 0
    E._same_scene(hk, gpu_ctx, s, _build(hk, 65))
