"""Host-side mirror of Hikari.Scene (src/scene.jl:17-161, src/scene-mesh.jl:9-179): incremental `push`, then
`sync` flattens everything into the POD arrays of hk_scene_desc (the job the Julia shim does by walking
`scene.accel` / `scene.materials` / `scene.lights`)."""
import ctypes as C
import inspect

import numpy as np

from . import _abi as A
from . import geometry as G
from . import lights as L
from . import materials as M
from . import media as MD

f32 = np.float32


class SceneInstance:
    """A mesh pushed by Scene.push_instance: its medium-interface index and its triangle range in the flattened soup."""

    __slots__ = ("mi_idx", "first_tri", "n_tris")

    def __init__(self, mi_idx, first_tri, n_tris):
        self.mi_idx, self.first_tri, self.n_tris = mi_idx, first_tri, n_tris

    def __repr__(self):
        return "SceneInstance(mi_idx=%d, first_tri=%d, n_tris=%d)" % (self.mi_idx, self.first_tri, self.n_tris)


def _move_lights_tree(move_lights):
    """move_lights of set_transform / set_vertices -> the `tree` of update_lights: False / True keep their meaning (True rebuilds the
    light BVH), "refit" refits it on the device."""
    if isinstance(move_lights, str):
        if move_lights != "refit":
            raise ValueError("move_lights must be False, True or 'refit', got %r" % (move_lights,))
        return "refit"
    return "rebuild"


def _affine_3x4(m4x4):
    """The 3x4 row-major affine part of a 4x4 transform; refuses what hk_scene_set_transform would refuse (ValueError)."""
    m = np.asarray(m4x4, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError("transform must be a 4x4 matrix, got shape %s" % (m.shape,))
    if not np.isfinite(m).all():
        raise ValueError("transform has non-finite entries")
    if not (m[3] == (0.0, 0.0, 0.0, 1.0)).all():
        raise ValueError("transform is not affine: its last row must be [0, 0, 0, 1]")
    m34 = np.ascontiguousarray(m[:3], dtype=f32)
    if not np.isfinite(m34).all():
        raise ValueError("transform entries overflow binary32")
    A3 = m34[:, :3].astype(np.float64)
    c0 = A3[1, 1] * A3[2, 2] - A3[1, 2] * A3[2, 1]
    c1 = A3[1, 2] * A3[2, 0] - A3[1, 0] * A3[2, 2]
    c2 = A3[1, 0] * A3[2, 1] - A3[1, 1] * A3[2, 0]
    det = (A3[0, 0] * c0 + A3[0, 1] * c1) + A3[0, 2] * c2
    if not (det != 0.0 and np.isfinite(det)):
        raise ValueError("transform is singular")
    return m34


def _transform_points(m34, p):
    """hk_scene_set_transform's point formula in binary32: p'[k] = ((m[k][0]*x + m[k][1]*y) + m[k][2]*z) + m[k][3]; [I | 0] copies."""
    m, p = np.asarray(m34, dtype=f32), np.asarray(p, dtype=f32)
    if (m == np.eye(3, 4, dtype=f32)).all():
        return p.copy()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = np.empty_like(p)
    for k in range(3):
        out[..., k] = ((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]
    return out


def _face_light_geometry(vs):
    """(normal, area) of a face's DiffuseAreaLight (scene-mesh.jl:98-131): edge cross product, its length `twice`, normal = cp / twice,
    area = twice / 2; None under the 1e-10 cut-off (no light is registered for such a face)."""
    e1, e2 = (vs[1] - vs[0]).astype(f32), (vs[2] - vs[0]).astype(f32)
    cp = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=f32)
    twice = np.sqrt(f32(f32(cp[0] * cp[0]) + f32(cp[1] * cp[1])) + f32(cp[2] * cp[2]), dtype=f32)
    if twice < 1e-10:
        return None
    return (cp / twice).astype(f32), f32(0.5) * twice


def _luminance(c):
    return float(f32(0.212671) * f32(c[0]) + f32(0.715160) * f32(c[1]) + f32(0.072169) * f32(c[2]))


class Scene:
    def __init__(self):
        self.lights = []            # in push order; flattened by type slot in sync()
        self._light_types = []      # type-slot order (MultiTypeSet: first-seen type order)
        self.materials = []         # BSDF materials in push order
        self._material_types = []
        self._material_keys = []    # SetKey (type_idx, vec_idx) per material, 1-based like the reference
        self.media = []
        self.media_interfaces = []  # (material, inside, outside) 0-based, -1 = vacuum
        self._meshes = []           # (Mesh world-space, per-face metas)
        self.textures = []
        self.spectra = []
        self._envmaps = []
        self._desc = None
        self._keep = None
        self._device = {}           # id(ctx) -> hk_scene handle (owned: released by close() / the next sync())
        self._transforms = {}       # (first_tri, n_tris) -> 3x4 float32: applied to every device scene after hk_scene_create
        self._stale_media = set()   # media edited by update_medium whose kept record still waits for its host majorant
        self._media_keep = {}
        self.bounds = None

    # ---- push! ---------------------------------------------------------------------------------
    def push_light(self, light):
        if type(light) not in self._light_types:
            self._light_types.append(type(light))
        self.lights.append(light)
        return len(self.lights)

    def _push_material_record(self, mat):
        if type(mat) not in self._material_types:
            self._material_types.append(type(mat))
        t = self._material_types.index(type(mat)) + 1
        v = sum(1 for m in self.materials if type(m) is type(mat)) + 1
        if isinstance(mat, M.MixMaterial):
            mat._idx1 = self._push_material_record(mat.material1)
            mat._idx2 = self._push_material_record(mat.material2)
            v = sum(1 for m in self.materials if type(m) is type(mat)) + 1
        self.materials.append(mat)
        self._material_keys.append((t, v))
        return len(self.materials) - 1

    def _push_medium(self, medium):
        if medium is None:
            return -1
        for i, m in enumerate(self.media):
            if m is medium:
                return i
        self.media.append(medium)
        return len(self.media) - 1

    def push_material(self, material):
        """push!(scene, material) -> index into media_interfaces (scene.jl:80-100)."""
        mi = material if isinstance(material, M.MediumInterface) else M.MediumInterface(material)
        mat_idx = self._push_material_record(mi.material)
        triple = (mat_idx, self._push_medium(mi.inside), self._push_medium(mi.outside))
        if triple not in self.media_interfaces:
            self.media_interfaces.append(triple)
        return self.media_interfaces.index(triple)

    def push(self, obj, material=None, transform=None):
        if isinstance(obj, L.Light):
            return self.push_light(obj)
        mesh = obj
        mi_idx = self.push_material(material)
        n = mesh.n_faces
        metas = np.zeros((n, 3), dtype=np.uint32)
        metas[:, 0] = mi_idx
        metas[:, 1] = np.arange(1, n + 1)
        emission = self._emission_info(material)
        if emission is not None:
            self._register_face_area_lights(mesh, metas, emission)
        world = mesh if transform is None else mesh.transformed(transform)
        self._meshes.append((world, metas))
        self._desc = None
        return mi_idx

    # ---- instances and in-place edits (update_transform!, update_material!) -------------------------------------------------
    def n_triangles(self):
        return sum(m.n_faces for m, _ in self._meshes)

    def push_instance(self, mesh, material, transform=None):
        """push! of a mesh that can be moved later: the description carries the mesh UN-transformed and the library applies
        `transform` (4x4 affine) after hk_scene_create.  Returns a SceneInstance for set_transform."""
        m34 = None if transform is None else _affine_3x4(transform)
        first = self.n_triangles()
        mi_idx = self.push(mesh, material)
        inst = SceneInstance(mi_idx, first, mesh.n_faces)
        if m34 is not None and inst.n_tris > 0:
            self._transforms[(first, inst.n_tris)] = m34
        return inst

    def set_transform(self, instance, m4x4, move_lights=False):
        """update_transform!: the instance's triangles become m4x4 applied to the mesh as pushed, in every device scene already
        created from this Scene and in those created later.

        move_lights=False (the default, the reference's behaviour, Q18): the area lights of an emissive instance stay where the mesh
        was pushed.  move_lights=True: they follow — every face's light is recomputed here from the moved vertices (the header's
        point formula, then _face_light_geometry as at push time) and sent with hk_scene_update_lights, one call per contiguous run
        of flat light indices; the light BVH is rebuilt.  A face whose moved edge cross product falls under the 1e-10 cut-off (a
        push would not have registered it) keeps its record with area = 0: zero power, so it leaves the tree, and comes back with
        the next transform that gives it an area.  move_lights="refit": the moved records go in ONE hk_scene_refit_lights call per
        device scene and the light BVH is refit on the device (update_light's tree="refit"); a face that degenerates or comes back
        would leave or enter the tree, which a refit refuses: ValueError before anything is moved — use True for such a move."""
        if not isinstance(instance, SceneInstance):
            raise TypeError("set_transform takes the SceneInstance push_instance returned")
        m34 = _affine_3x4(m4x4)
        if instance.n_tris < 1 or instance.first_tri < 0 or instance.first_tri + instance.n_tris > self.n_triangles():
            raise ValueError("instance %r is not a triangle range of this scene" % (instance,))
        moved = self._moved_area_lights(instance, m34) if move_lights else []
        tree = _move_lights_tree(move_lights)
        self._check_refit_moves(moved, tree)                # before anything changes: geometry and lights move together or not at all
        self._transforms[(instance.first_tri, instance.n_tris)] = m34
        from . import _lib
        for h in (getattr(self, "_device", None) or {}).values():
            _lib.check(_lib.lib().hk_scene_set_transform(h, instance.first_tri, instance.n_tris, m34.ctypes.data_as(A.PF)), "hk_scene_set_transform")
        if moved:
            self._replace_lights(moved, tree)

    def _check_refit_moves(self, moved, tree):
        """A refit keeps every light's membership in the light tree; of a moved face light only its area decides it (Le and scale are
        kept).  ValueError for a face that degenerates (area -> 0) or comes back, which hk_scene_refit_lights would refuse AFTER the
        geometry had moved."""
        if tree != "refit":
            return
        for index, light in moved:
            if (light.area > 0) != (self.lights[index].area > 0):
                raise ValueError("move_lights='refit': the area light of light %d would %s the light tree (its face %s); use move_lights=True for this move"
                                 % (index, "leave" if self.lights[index].area > 0 else "enter", "degenerates" if self.lights[index].area > 0 else "gets an area again"))

    def _mesh_index(self, instance):
        """Position in self._meshes of the mesh `instance` was pushed as."""
        first = 0
        for k, (mesh, _) in enumerate(self._meshes):
            if first == instance.first_tri and mesh.n_faces == instance.n_tris:
                return k
            first += mesh.n_faces
        raise ValueError("instance %r is not a mesh of this scene" % (instance,))

    def _moved_area_lights(self, instance, m34, positions=None, uvs=None):
        """[(index into self.lights, DiffuseAreaLight)] of the instance's faces that carry a light, from the kept mesh (or `positions` /
        `uvs` in its place) moved by m34."""
        mesh, metas = self._meshes[self._mesh_index(instance)]
        faces = np.nonzero(metas[:, 2])[0]
        P = _transform_points(m34, (mesh.positions if positions is None else positions)[faces])
        out = []
        for face, vs, idx1 in zip(faces, P, metas[faces, 2]):
            old = self.lights[int(idx1) - 1]
            geo = _face_light_geometry(vs)
            normal, area = geo if geo is not None else (np.asarray(old.normal, dtype=f32), 0.0)
            uv = np.array(old.uv if uvs is None else uvs[face], dtype=f32)
            out.append((int(idx1) - 1, L.DiffuseAreaLight(vs.copy(), normal, float(area), uv, old.Le, old.scale, old.two_sided)))
        return out

    def set_vertices(self, instance, positions, normals=None, uvs=None, move_lights=False):
        """New vertices for the mesh of `instance` (the SceneInstance of push_instance): positions [n_tris, 3, 3] and, optionally,
        normals [n_tris, 3, 3] and uvs [n_tris, 3, 2] replace the kept UN-transformed mesh — device scenes created later are built
        from it — the kept description, and, through hk_scene_set_vertices, the base geometry of every device scene already created.
        The instance keeps its transform.  An attribute left None keeps its values.

        move_lights=False (the default): area lights stay as they are, as with set_transform (Q18).  move_lights=True: every face
        light of the instance is recomputed from the new vertices under the instance's current transform (_face_light_geometry, a
        degenerate face keeping its record with area = 0, as set_transform(move_lights=True) does) and, with `uvs`, carries the new
        uvs; its Le is kept (a textured emission is not sampled again).  Which faces emit does not change.  move_lights="refit": as
        set_transform's — one hk_scene_refit_lights call per device scene, the light BVH refit on the device.

        ValueError for what the library would refuse: a wrong shape, a non-finite position, normals / uvs for a mesh pushed without."""
        if not isinstance(instance, SceneInstance):
            raise TypeError("set_vertices takes the SceneInstance push_instance returned")
        k = self._mesh_index(instance)
        mesh, metas = self._meshes[k]
        n = instance.n_tris

        def take(a, shape, what):
            a = np.asarray(a)
            if a.shape != shape:
                raise ValueError("set_vertices: %s must have shape %s, got %s" % (what, shape, a.shape))
            with np.errstate(over="ignore"):
                return np.ascontiguousarray(a, dtype=f32)

        if n < 1:
            raise ValueError("instance %r has no triangles" % (instance,))
        P = take(positions, (n, 3, 3), "positions")
        if not np.isfinite(P).all():
            raise ValueError("set_vertices: positions have non-finite entries")
        N = U = None
        if normals is not None:
            if mesh.normals is None:
                raise ValueError("set_vertices: normals for a mesh pushed without normals")
            N = take(normals, (n, 3, 3), "normals")
        if uvs is not None:
            if mesh.uvs is None:
                raise ValueError("set_vertices: uvs for a mesh pushed without uvs")
            U = take(uvs, (n, 3, 2), "uvs")
        moved = []
        tree = _move_lights_tree(move_lights)
        if move_lights:
            m34 = self._transforms.get((instance.first_tri, n), np.eye(3, 4, dtype=f32))
            moved = self._moved_area_lights(instance, m34, P, U)
        self._check_refit_moves(moved, tree)                # before anything changes
        self._meshes[k] = (G.Mesh(P.copy(), mesh.normals if N is None else N.copy(), mesh.uvs if U is None else U.copy()), metas)
        a, e = instance.first_tri, instance.first_tri + n
        if self._desc is not None:              # the arrays the kept description points into, rewritten in place
            kept_p, kept_n, kept_uv = self._keep[:3]
            kept_p[a:e] = P
            if N is not None:
                kept_n[a:e] = N
            if U is not None:
                kept_uv[a:e] = U
            lo, hi = kept_p.reshape(-1, 3).min(axis=0), kept_p.reshape(-1, 3).max(axis=0)
            c = (lo + hi) * f32(0.5)
            self.bounds = (lo, hi, c, float(np.linalg.norm(hi - c)))
        from . import _lib
        ptr = lambda arr: None if arr is None else arr.ctypes.data_as(A.PF)
        for h in (getattr(self, "_device", None) or {}).values():
            _lib.check(_lib.lib().hk_scene_set_vertices(h, a, n, ptr(P), ptr(N), None, ptr(U)), "hk_scene_set_vertices")
        if moved:
            self._replace_lights(moved, tree)

    def bvh_cost(self, ctx):
        """(now, created) of hk_scene_bvh_cost for this scene on `ctx`: the cost of the BVH as the device holds it after the refits
        of set_transform / set_vertices, and of the tree as hk_scene_create built it.  now / created is the quantity to watch when
        deciding whether to build the scene anew (sync())."""
        from . import _lib, volpath
        now, created = C.c_double(), C.c_double()
        _lib.check(_lib.lib().hk_scene_bvh_cost(volpath.scene_handle(ctx, self), C.byref(now), C.byref(created)), "hk_scene_bvh_cost")
        return now.value, created.value

    def rebuild_bvh(self, ctx=None, costs=True):
        """hk_scene_rebuild_bvh for every device scene created from this Scene (ctx=None), or for that context's alone: the BVH is
        built anew on the device from the world positions it holds, the tree hk_scene_create would build from them; everything else
        of the scene stays.  -> [(cost_before, cost_after)] per device scene touched (one pair for a given ctx): the tree cost
        (bvh_cost) the refits had left, and the cost of the new tree — the baseline of bvh_cost from now on.

        The library call waits for the device once.  The two cost read-outs around it wait too (one reduction and one wait each):
        costs=False skips them and returns [None] per device scene — the call an interactive loop wants."""
        from . import _lib, volpath
        if ctx is not None:
            handles = [volpath.scene_handle(ctx, self)]
        else:
            handles = list((getattr(self, "_device", None) or {}).values())
        out = []
        for h in handles:
            before, after = C.c_double(), C.c_double()
            if costs:
                _lib.check(_lib.lib().hk_scene_bvh_cost(h, C.byref(before), None), "hk_scene_bvh_cost")
            _lib.check(_lib.lib().hk_scene_rebuild_bvh(h), "hk_scene_rebuild_bvh")
            if costs:
                _lib.check(_lib.lib().hk_scene_bvh_cost(h, None, C.byref(after)), "hk_scene_bvh_cost")
            out.append((before.value, after.value) if costs else None)
        return out

    def bvh_leaves(self, ctx):
        """The triangle index of every leaf slot of this scene's BVH on `ctx` (hk_scene_bvh_leaves), int32 [n_triangles]: what the
        leaf references of hk_scene_bvh_copy (~ref = first slot << 3 | count - 1) index."""
        from . import _lib, volpath
        h = volpath.scene_handle(ctx, self)
        n = C.c_int32()
        _lib.check(_lib.lib().hk_scene_bvh_leaves(h, C.byref(n), None), "hk_scene_bvh_leaves")
        prims = np.empty(n.value, np.int32)
        if n.value:
            _lib.check(_lib.lib().hk_scene_bvh_leaves(h, C.byref(n), prims.ctypes.data_as(C.POINTER(C.c_int32))), "hk_scene_bvh_leaves")
        return prims

    # ---- lights and environment maps in place (hk_scene_update_lights, hk_scene_update_envmap) --------------------------------
    def _flat_index(self, index):
        light = self.lights[index]
        for i, l in enumerate(self.flat_lights()):
            if l is light:
                return i
        raise ValueError("light %d is not in the flat order" % index)

    def _replace_lights(self, pairs, tree="rebuild"):
        """pairs: [(index into self.lights, new light of the same class)].  Rewrites self.lights, the kept description and every
        device scene.  tree="rebuild": contiguous runs of FLAT indices (flat_lights() order, what hk_scene_desc::lights holds) in one
        hk_scene_update_lights call each.  tree="refit": the whole set in ONE hk_scene_refit_lights call per device scene."""
        if tree not in ("rebuild", "refit"):
            raise ValueError("tree must be 'rebuild' or 'refit', got %r" % (tree,))
        for index, light in pairs:
            if not 0 <= index < len(self.lights):
                raise IndexError("light index %d out of range" % index)
            if type(light) is not type(self.lights[index]):
                raise TypeError("update_light: %s cannot replace %s (the class must match)" % (type(light).__name__, type(self.lights[index]).__name__))
        flat = [self._flat_index(index) for index, _ in pairs]
        if tree == "refit" and len(set(flat)) != len(flat):
            raise ValueError("update_lights(tree='refit'): a light is given twice")
        recs = None
        if self._desc is not None:      # (before the first sync there is no description: the next one flattens the new lights)
            n_tex, n_env = len(self.textures), len(self._envmaps)
            try:
                recs = [self._light_record(light, None) for _, light in pairs]
                added = len(self.textures) != n_tex or len(self._envmaps) != n_env
            finally:
                del self.textures[n_tex:], self._envmaps[n_env:]
            if added:
                raise ValueError("update_light: the new light references a texture or an environment map that is not in the scene")
        from . import _lib
        if tree == "refit" and recs is not None and pairs:
            # the device scenes first: a refit the library refuses (a light entering or leaving the tree) leaves everything as it was
            idx = (C.c_int32 * len(flat))(*flat)
            arr = (A.hk_light * len(recs))(*recs)
            for h in (getattr(self, "_device", None) or {}).values():
                _lib.check(_lib.lib().hk_scene_refit_lights(h, len(flat), idx, arr), "hk_scene_refit_lights")
            for k, rec in zip(flat, recs):
                self._desc.lights[k] = rec
        for index, light in pairs:
            self.lights[index] = light
        if recs is None or tree == "refit":
            return
        order = sorted(range(len(flat)), key=lambda k: flat[k])
        k = 0
        while k < len(order):
            e = k + 1
            while e < len(order) and flat[order[e]] == flat[order[e - 1]] + 1:
                e += 1
            run = (A.hk_light * (e - k))(*[recs[order[j]] for j in range(k, e)])
            for j in range(k, e):
                self._desc.lights[flat[order[j]]] = recs[order[j]]
            for h in (getattr(self, "_device", None) or {}).values():
                _lib.check(_lib.lib().hk_scene_update_lights(h, flat[order[k]], e - k, run), "hk_scene_update_lights")
            k = e

    def update_light(self, index, light, tree="rebuild"):
        """The light self.lights[index] (0-based position in push order: push_light's return value minus one) is replaced by
        `light`, an object of the same class: dim a lamp, move a point light, turn the sun, re-colour an emitter (a
        DiffuseAreaLight: its Le, scale, two_sided, geometry).  The description holds the lights in flat_lights() order; the index
        is mapped through it.

        tree="rebuild" (the default): every device scene rebuilds its light BVH on the host (hk_scene_update_lights) and is, bit for
        bit, the scene a fresh hk_scene_create makes of the edited description.  tree="refit": the tree keeps its topology and is
        refit on the device (hk_scene_refit_lights) — interactive on many lights, the same expected image with another pmf; a light
        may not enter or leave the tree (a power going to or from zero), which the library refuses with nothing changed.  The kept
        description is rewritten either way, so a device scene created LATER from it has the fresh tree."""
        self._replace_lights([(index, light)], tree)

    def update_lights(self, pairs, tree="rebuild"):
        """update_light for a set: pairs = [(index, light)].  tree="refit" sends the whole set in one call per device scene."""
        self._replace_lights(list(pairs), tree)

    def update_envmap(self, env_map, data=None, rotation=None):
        """New texels (same size, [height, width, 3 or 4]) and / or a new 3x3 rotation for an EnvironmentMap of this scene, in the
        kept description and in every device scene (which builds the sampling tables from the texels itself)."""
        env_map.update(data=data, rotation=rotation)        # refuses what the library would refuse (ValueError)
        if self._desc is None:
            return
        for idx, e in enumerate(self._envmaps):
            if e is env_map:
                break
        else:
            raise ValueError("update_envmap: the map belongs to no EnvironmentLight of this scene")
        rec = self._desc.envmaps[idx]
        rec.rotation[:] = [float(x) for x in env_map.rotation.reshape(-1)]
        if env_map._sky is None:                            # (a sky the host has not baked: _bake_skies refreshes the value)
            rec.marginal_func_int = float(env_map.distribution.marginal_func_int)
        rot = np.ascontiguousarray(env_map.rotation, dtype=f32) if rotation is not None else None
        from . import _lib
        for h in (getattr(self, "_device", None) or {}).values():
            _lib.check(_lib.lib().hk_scene_update_envmap(h, idx, env_map._jl.ctypes.data_as(A.PF) if data is not None else None,
                                                        rot.ctypes.data_as(A.PF) if rot is not None else None), "hk_scene_update_envmap")

    def update_sky(self, env_light, direction, turbidity=2.5, intensity=None, ground_albedo=None, ground_enabled=True, sun=None, build="device"):
        """The map of `env_light` (an EnvironmentLight of this scene, as sunsky_to_envlight returns it) becomes the Hosek-Wilkie sky of a
        new sun `direction` (pointing TO the sun, z up), `turbidity` and ground; its size and rotation stay.
        build="device": every device scene bakes the texels itself from a parameter record of 1224 bytes (hk_scene_update_envmap_sky)
        and builds its tables from them.  The map keeps the parameters; its host texels and tables (env_map.data, .distribution) are
        baked only when something asks for them — reading either, record(), or creating a device scene from the kept description.
        build="host": the texels are baked here (sunsky.sky_texels) and go through update_envmap.
        `intensity`: the light's scale becomes the one sunsky_to_envlight gives that intensity.  `sun`: that SunLight of the scene is
        turned to the new direction as well (with `intensity`, it also gets the spectrum and scale sunsky_to_envlight gives it); both
        records go through update_light.
        LATER SCENES.  A device scene created afterwards from the kept description holds the HOST bake.  That is the same sky within
        the bound recorded in tests/golden/sky_bake_bounds.json (the device and NumPy differ in the last places of cos, acos and exp),
        not bit for bit the sky of the scene that was edited.  Use build="host" where every scene must hold the same bits.
        Raises ValueError for what the library would refuse."""
        from . import sunsky
        from .envmap import EnvironmentLight
        from .lights import SunLight
        if build not in ("device", "host"):
            raise ValueError("update_sky: build is 'device' or 'host', not %r" % (build,))
        if not isinstance(env_light, EnvironmentLight) or not any(l is env_light for l in self.lights):
            raise ValueError("update_sky: env_light is not an EnvironmentLight of this scene")
        if sun is not None and (not isinstance(sun, SunLight) or not any(l is sun for l in self.lights)):
            raise ValueError("update_sky: sun is not a SunLight of this scene")
        env_map = env_light.env_map
        if env_map.height != env_map.width:
            raise ValueError("update_sky: the map is %dx%d (a sky is baked into a square map)" % (env_map.width, env_map.height))
        d = np.asarray(direction, dtype=np.float64).reshape(-1)
        if d.shape != (3,) or not np.isfinite(d).all() or not (d * d).sum() > 0:
            raise ValueError("update_sky: the direction is not a finite, non-zero 3-vector")
        if not np.isfinite(float(turbidity)) or (intensity is not None and not np.isfinite(float(intensity))):
            raise ValueError("update_sky: non-finite turbidity or intensity")
        if ground_albedo is not None and not np.isfinite(np.asarray(ground_albedo.c, dtype=np.float64)).all():
            raise ValueError("update_sky: non-finite ground albedo")
        sky = dict(direction=tuple(float(x) for x in d), turbidity=float(turbidity), ground_albedo=ground_albedo, ground_enabled=bool(ground_enabled))
        params = sunsky.sky_params(**sky)
        if not all(np.isfinite(np.ctypeslib.as_array(getattr(params, name))).all() for name in ("sun_dir", "ground_rgb", "config", "radiance", "xyz_weight")):
            raise ValueError("update_sky: the cooked coefficients are not finite (turbidity %r)" % (turbidity,))
        idx = None
        if self._desc is not None:
            for idx, e in enumerate(self._envmaps):
                if e is env_map:
                    break
            else:
                raise ValueError("update_sky: the map belongs to no EnvironmentLight of this scene")
        if build == "host":
            self.update_envmap(env_map, data=sunsky.sky_texels(resolution=env_map.height, **sky))
        else:
            env_map.set_sky(**sky)
            if idx is not None:
                from . import _lib
                for h in (getattr(self, "_device", None) or {}).values():
                    _lib.check(_lib.lib().hk_scene_update_envmap_sky(h, idx, C.byref(params)), "hk_scene_update_envmap_sky")
        pairs = []
        if intensity is not None:
            env_light.scale_rgb = env_light.i = sunsky.sky_scale(intensity)
            pairs.append((next(k for k, l in enumerate(self.lights) if l is env_light), env_light))
        if sun is not None:
            new = sunsky.sun_light(sky["direction"], 1.0 if intensity is None else intensity)
            sun.direction = new.direction
            if intensity is not None:
                sun.i, sun.scale = new.i, new.scale
            pairs.append((next(k for k, l in enumerate(self.lights) if l is sun), sun))
        if pairs:
            self._replace_lights(pairs)

    def _bake_skies(self):
        """The host bakes update_sky(build="device") left pending, into the arrays the kept description points to."""
        for idx, e in enumerate(self._envmaps):
            if e._sky is not None:
                e.bake()
                self._desc.envmaps[idx].marginal_func_int = float(e.distribution.marginal_func_int)

    def update_medium(self, medium, **changes):
        """New volume data, coefficients, bounds or transform for a medium of this scene (the keywords of the medium's own update()),
        in the kept description and in every device scene — which builds the majorant grid, its zero-cell mask and the NanoVDB bricks
        from the data itself (hk_scene_update_medium); the host majorant of `medium` is rebuilt only when a scene is created again.
        A NanoVDBMedium's data=..., build="device" (a numpy array, or a torch tensor on the device of the scene's context) lets the
        device scenes build the tree as well (hk_scene_update_medium_dense); the medium keeps the field and builds its host tree late.
        A tensor is read in place by the scenes of a context (Context.get) on the tensor's device — which is waited for, so the device
        has read the tensor when this returns — and goes from host memory to every other scene.  The medium keeps the field BY
        REFERENCE for its late host tree (media.NanoVDBMedium.update): hand over a copy if the array is written again."""
        for idx, m in enumerate(self.media):
            if m is medium:
                break
        else:
            raise ValueError("update_medium: the medium belongs to no medium interface of this scene")
        unknown = set(changes) - set(inspect.signature(medium.update).parameters)
        if unknown:
            raise ValueError("update_medium: a %s has no %s to change" % (type(medium).__name__, ", ".join(sorted(unknown))))
        if len(self.media) == 1 and medium.kind in (A.HK_MEDIUM_GRID, A.HK_MEDIUM_NANOVDB):
            # a scene of ONE medium with flat sigma_a and sigma_s runs the grey kernels: that class cannot change in place
            after = all(MD.flat_spectrum(changes.get(k) or getattr(medium, k)) for k in ("sigma_a", "sigma_s"))
            if after != MD.is_grey(medium):
                raise ValueError("update_medium: a grey medium (flat sigma_a and sigma_s) cannot turn coloured in place, nor a coloured one grey")
        medium.update(**changes)               # refuses what the library would refuse of the object alone (ValueError)
        if self._desc is None:
            return
        self._stale_media.add(idx)             # the kept record is refilled, with the host majorant, when a scene is created from it
        keep = []
        rec = A.hk_medium()
        from . import _lib
        handles = list((getattr(self, "_device", None) or {}).values())
        field = medium.dense_field(keep) if changes.get("build") == "device" else None
        if field is not None:
            # the device builds the tree from the field (hk_scene_update_medium_dense); the host tree waits until something asks for it
            medium.fill_record(rec, keep, majorant=False, tree=False)
            from_host = field
            if field.on_device:
                # A tensor is read in place only by a scene whose context is on the tensor's device; every other scene gets the field
                # from host memory.  The tensor's producer is ordered before the library's stream here, and the context is waited for
                # after the call, so the build kernels have read the tensor when this returns: the caller may write into it again.
                import torch
                from .volpath import Context
                tensor = keep[0]
                torch.cuda.current_stream(tensor.device).synchronize()
                ctx_of = {id(c): c for c in Context._by_device.values()}
                local = {cid for cid in self._device if cid in ctx_of and int(ctx_of[cid].device) == int(tensor.device.index or 0)}
                if len(local) < len(self._device):
                    host = np.ascontiguousarray(tensor.cpu().numpy())
                    keep.append(host)
                    from_host = A.hk_dense_field.from_buffer_copy(field)
                    from_host.data, from_host.on_device = host.ctypes.data_as(A.PF), 0
            for cid, h in (getattr(self, "_device", None) or {}).items():
                in_place = field.on_device and cid in local
                _lib.check(_lib.lib().hk_scene_update_medium_dense(h, idx, C.byref(rec), C.byref(field if in_place else from_host)), "hk_scene_update_medium_dense")
                if in_place:
                    _lib.check(_lib.lib().hk_sync(ctx_of[cid].h), "hk_sync")
            return
        medium.fill_record(rec, keep, majorant=False)
        for h in handles:
            _lib.check(_lib.lib().hk_scene_update_medium(h, idx, C.byref(rec)), "hk_scene_update_medium")

    def _refresh_media(self):
        for idx in sorted(self._stale_media):
            keep = []
            rec = A.hk_medium()
            self.media[idx].fill_record(rec, keep)
            self._media_keep[idx] = keep
            self._desc.media[idx] = rec
        self._stale_media.clear()

    def _apply_transforms(self, handle):
        from . import _lib
        for (first, n), m34 in self._transforms.items():
            _lib.check(_lib.lib().hk_scene_set_transform(handle, first, n, m34.ctypes.data_as(A.PF)), "hk_scene_set_transform")

    def update_material(self, mi_idx, new_material):
        """update_material!(scene, idx, material) (scene.jl:104-112): the BSDF material of medium interface `mi_idx` (what push
        returned) is replaced by one of the same type.  Textures must be constants or Texture objects already in the scene."""
        if not 0 <= mi_idx < len(self.media_interfaces):
            raise IndexError("medium interface index %d out of range" % mi_idx)
        flat = self.media_interfaces[mi_idx][0]
        plan = []                               # (flat index, material) in record order
        self._plan_material_update(flat, new_material, plan)
        n_tex, n_spec = len(self.textures), len(self.spectra)
        try:
            recs = [(idx, self._material_record(m, self._material_keys[idx], None)) for idx, m in plan]
            added = len(self.textures) != n_tex or len(self.spectra) != n_spec
        finally:
            del self.textures[n_tex:], self.spectra[n_spec:]
        if added:
            raise ValueError("update_material: the new material references a texture or spectrum that is not in the scene")
        for idx, r in recs:
            if _alpha_tested(r) != _alpha_tested(self._material_record(self.materials[idx], self._material_keys[idx], None)):
                raise ValueError("update_material: a Matte material cannot change between opaque and alpha-tested")
        for idx, m in plan:
            self.materials[idx] = m
        kept = self._desc.materials if self._desc is not None else None
        from . import _lib
        for idx, r in recs:
            if kept is not None:
                kept[idx] = r
            for h in (getattr(self, "_device", None) or {}).values():
                _lib.check(_lib.lib().hk_scene_update_materials(h, idx, 1, C.byref(r)), "hk_scene_update_materials")

    def _plan_material_update(self, flat, new, plan):
        old = self.materials[flat]
        # (Emissive stays refused here: an emitter's colour is a property of its area lights — update_light changes it)
        if isinstance(new, (M.MediumInterface, M.Emissive)) or type(new) is not type(old):
            raise TypeError("update_material: %s cannot replace %s (the type must match; emission is not editable)" % (type(new).__name__, type(old).__name__))
        if isinstance(new, M.MixMaterial):
            new._idx1, new._idx2 = old._idx1, old._idx2
            self._plan_material_update(old._idx1, new.material1, plan)
            self._plan_material_update(old._idx2, new.material2, plan)
        plan.append((flat, new))

    @staticmethod
    def _emission_info(material):
        if isinstance(material, M.MediumInterface):
            if material.emission is not None:
                return material.emission
            return Scene._emission_info(material.material)
        if isinstance(material, M.Emissive):
            return material
        return None

    def _register_face_area_lights(self, mesh, metas, em):
        """scene-mesh.jl:98-131 — uses the UN-transformed mesh vertices (quirk Q18)."""
        for i in range(mesh.n_faces):
            vs = mesh.positions[i]
            uv = mesh.uvs[i] if mesh.uvs is not None else np.array([[0, 0], [1, 0], [1, 1]], dtype=f32)
            Le = em.Le
            if isinstance(Le, M.Texture):
                # evaluate_face_emission (scene-mesh.jl:49): the texture is point-sampled ONCE at the face's centroid uv
                # (evaluate_texture -> _sample_texture_data: nearest texel, (1-v, u) flip); the light carries that constant
                cu = f32(f32(f32(uv[0][0] + uv[1][0]) + uv[2][0]) / f32(3))
                cv = f32(f32(f32(uv[0][1] + uv[1][1]) + uv[2][1]) / f32(3))
                d = Le.data
                th, tw = d.shape[:2]
                ti = min(max(int(f32(1) + f32(th - 1) * f32(f32(1) - cv)), 1), th)
                tj = min(max(int(f32(1) + f32(tw - 1) * cu), 1), tw)
                texel = d[ti - 1, tj - 1]
                Le = M.RGBSpectrum(*[float(x) for x in np.atleast_1d(texel)[:4]]) if np.ndim(texel) else M.RGBSpectrum(float(texel))
            if _luminance(Le.c) < 1e-4:
                continue
            geo = _face_light_geometry(vs)
            if geo is None:
                continue
            normal, area = geo
            self.push_light(L.DiffuseAreaLight(vs.copy(), normal, float(area), uv.copy(), Le, em.scale, em.two_sided))
            metas[i, 2] = len(self.lights)  # flat index = length(scene.lights) at push time

    # ---- sync! / flatten -------------------------------------------------------------------------
    def flat_lights(self):
        """flat_to_light_index order: type slots in first-seen order (lights/light-sampler.jl:289-329)."""
        out = []
        for t in self._light_types:
            out.extend(l for l in self.lights if type(l) is t)
        return out

    def _tex_rgba(self, v, keep):
        r = A.hk_tex_rgba()
        if isinstance(v, M.Texture):
            r.tex = self._texture_index(v, keep)
            r.c[:] = (0, 0, 0, 1)
        else:
            r.tex = -1
            r.c[:] = v.c
        return r

    def _tex_f32(self, v, keep):
        r = A.hk_tex_f32()
        if isinstance(v, M.Texture):
            r.tex = self._texture_index(v, keep)
            r.v = 0.0
        else:
            r.tex = -1
            r.v = float(f32(v))
        return r

    def _texture_index(self, tex, keep):
        for i, t in enumerate(self.textures):
            if t is tex:
                return i
        self.textures.append(tex)
        return len(self.textures) - 1

    def _envmap_index(self, env):
        for i, e in enumerate(self._envmaps):
            if e is env:
                return i
        self._envmaps.append(env)
        return len(self._envmaps) - 1

    def _spectrum_index(self, sp):
        for i, s in enumerate(self.spectra):
            if s is sp:
                return i
        self.spectra.append(sp)
        return len(self.spectra) - 1

    def _material_record(self, m, key, keep):
        r = A.hk_material()
        r.kind = m.kind
        r.flags = 0
        for k in range(4):
            r.rgb[k].tex = -1
            r.rgb[k].c[:] = (0, 0, 0, 1)
        for k in range(8):
            r.f[k].tex = -1
        r.spectrum[0] = r.spectrum[1] = -1
        T, F = self._tex_rgba, self._tex_f32
        if isinstance(m, M.MatteMaterial):
            r.rgb[0], r.f[0] = T(m.Kd, keep), F(m.sigma, keep)
        elif isinstance(m, M.MirrorMaterial):
            r.rgb[0] = T(m.Kr, keep)
        elif isinstance(m, M.GlassMaterial):
            r.rgb[0], r.rgb[1], r.f[0] = T(m.Kr, keep), T(m.Kt, keep), F(m.index, keep)
        elif isinstance(m, M.ConductorMaterial):
            for slot, v in ((0, m.eta), (1, m.k)):
                if isinstance(v, M.PiecewiseLinearSpectrum):
                    r.spectrum[slot] = self._spectrum_index(v)
                else:
                    r.rgb[slot] = T(v, keep)
            r.f[0] = F(m.roughness, keep)
            r.flags = A.HK_MATF_REMAP_ROUGHNESS if m.remap_roughness else 0
        elif isinstance(m, M.CoatedDiffuseMaterial):
            r.rgb[0], r.rgb[1] = T(m.reflectance, keep), T(m.albedo, keep)
            for k, v in enumerate((m.u_roughness, m.v_roughness, m.thickness, m.eta, m.g)):
                r.f[k] = F(v, keep)
            r.i[0], r.i[1] = m.max_depth, m.n_samples
            r.flags = A.HK_MATF_REMAP_ROUGHNESS if m.remap_roughness else 0
        elif isinstance(m, M.ThinDielectricMaterial):
            r.f[0] = F(m.eta, keep)
        elif isinstance(m, M.DiffuseTransmissionMaterial):
            r.rgb[0], r.rgb[1], r.f[0] = T(m.reflectance, keep), T(m.transmittance, keep), F(m.scale, keep)
        elif isinstance(m, M.CoatedDiffuseTransmissionMaterial):
            r.rgb[0], r.rgb[1], r.rgb[2] = T(m.reflectance, keep), T(m.transmittance, keep), T(m.albedo, keep)
            for k, v in enumerate((m.u_roughness, m.v_roughness, m.thickness, m.eta, m.g)):
                r.f[k] = F(v, keep)
            r.i[0], r.i[1] = m.max_depth, m.n_samples
            r.flags = A.HK_MATF_REMAP_ROUGHNESS if m.remap_roughness else 0
        elif isinstance(m, M.CoatedConductorMaterial):
            for slot, v in ((0, m.conductor_eta), (1, m.conductor_k)):
                if isinstance(v, M.PiecewiseLinearSpectrum):
                    r.spectrum[slot] = self._spectrum_index(v)
                else:
                    r.rgb[slot] = T(M._rgb(v), keep)
            r.rgb[2], r.rgb[3] = T(m.reflectance, keep), T(m.albedo, keep)
            for k, v in enumerate((m.interface_u_roughness, m.interface_v_roughness, m.interface_eta,
                                   m.conductor_u_roughness, m.conductor_v_roughness, m.thickness, m.g)):
                r.f[k] = F(v, keep)
            r.i[0], r.i[1] = m.max_depth, m.n_samples
            r.flags = (A.HK_MATF_REMAP_ROUGHNESS if m.remap_roughness else 0) | (A.HK_MATF_USE_ETA_K if m.use_eta_k else 0)
        elif isinstance(m, M.MixMaterial):
            r.f[0] = F(m.amount, keep)
            r.i[0], r.i[1] = m._idx1, m._idx2
            k1, k2 = self._material_keys[m._idx1], self._material_keys[m._idx2]
            r.mix_key[:] = (k1[0], k1[1], k2[0], k2[1])
        return r

    def _light_record(self, l, keep):
        r = A.hk_light()
        r.kind = l.kind
        r.envmap = -1
        r.Le.tex = -1
        if isinstance(l, L.DiffuseAreaLight):
            r.spectrum_kind = A.HK_SPEC_RGB
            r.scale = l.scale
            r.v[:] = [float(x) for x in np.asarray(l.vertices, dtype=f32).reshape(-1)]
            r.normal[:] = [float(x) for x in l.normal]
            r.area = l.area
            r.uv[:] = [float(x) for x in np.asarray(l.uv, dtype=f32).reshape(-1)]
            r.Le = self._tex_rgba(l.Le, keep)
            r.two_sided = 1 if l.two_sided else 0
            return r
        if l.kind == A.HK_LIGHT_ENVIRONMENT:
            r.spectrum_kind = A.HK_SPEC_RGB
            r.i_rgb[:] = l.scale_rgb.c
            r.scale = 1.0
            r.envmap = self._envmap_index(l.env_map)
            return r
        sf = L._spec_fields(l.i)
        r.spectrum_kind = sf["spectrum_kind"]
        r.i_rgb[:] = sf["i_rgb"]
        r.poly[:] = sf["poly"]
        r.illum_scale = sf["illum_scale"]
        r.scale = l.scale
        if hasattr(l, "position"):
            r.position[:] = l.position
        if hasattr(l, "direction"):
            r.direction[:] = l.direction
        if isinstance(l, L.SpotLight):
            r.world_to_light[:] = [float(x) for x in l.world_to_light.reshape(-1)]
            r.light_to_world[:] = [float(x) for x in l.light_to_world.reshape(-1)]
            r.cos_total_width, r.cos_falloff_start = l.cos_total_width, l.cos_falloff_start
        return r

    def sync(self):
        """sync!(scene): flatten to hk_scene_desc (kept alive on self) and compute world bounds."""
        self.close()                # device scenes built from the previous description are released, not leaked
        keep = []
        P = np.concatenate([m.positions for m, _ in self._meshes], axis=0) if self._meshes else np.zeros((0, 3, 3), f32)
        T = P.shape[0]
        any_n = any(m.normals is not None for m, _ in self._meshes)
        any_uv = any(m.uvs is not None for m, _ in self._meshes)
        Nn = Uv = None
        if any_n:
            Nn = np.concatenate([m.normals if m.normals is not None else np.full(m.positions.shape, np.nan, f32) for m, _ in self._meshes], axis=0)
        if any_uv:
            default_uv = np.array([[0, 0], [1, 0], [1, 1]], dtype=f32)
            Uv = np.concatenate([m.uvs if m.uvs is not None else np.broadcast_to(default_uv, (m.n_faces, 3, 2)) for m, _ in self._meshes], axis=0)
        metas = np.concatenate([mt for _, mt in self._meshes], axis=0) if self._meshes else np.zeros((0, 3), np.uint32)
        P = np.ascontiguousarray(P, dtype=f32)
        metas = np.ascontiguousarray(metas, dtype=np.uint32)
        mats = (A.hk_material * max(1, len(self.materials)))()
        for i, m in enumerate(self.materials):
            mats[i] = self._material_record(m, self._material_keys[i], keep)
        mis = (A.hk_medium_interface * max(1, len(self.media_interfaces)))()
        for i, (a, b, c) in enumerate(self.media_interfaces):
            mis[i].material, mis[i].inside, mis[i].outside = a, b, c
        fl = self.flat_lights()
        self._envmaps = []
        lts = (A.hk_light * max(1, len(fl)))()
        for i, l in enumerate(fl):
            lts[i] = self._light_record(l, keep)
        texs = (A.hk_texture * max(1, len(self.textures)))()
        for i, t in enumerate(self.textures):
            d = t.data
            if isinstance(t, M.VertexColorTexture):      # Julia face_colors[3, n_faces]: a face's 3 colours are adjacent
                keep.append(d)
                texs[i].width, texs[i].height, texs[i].channels, texs[i].kind = t.n_faces, 3, 4, 1
                texs[i].data = d.ctypes.data_as(A.PF)
                continue
            h, w = d.shape[:2]
            ch = 1 if d.ndim == 2 else d.shape[2]
            jl = np.ascontiguousarray(np.transpose(d.reshape(h, w, ch), (1, 0, 2)))  # [w][h][c] == Julia [h,w] column-major
            keep.append(jl)
            texs[i].width, texs[i].height, texs[i].channels = w, h, ch
            texs[i].data = jl.ctypes.data_as(A.PF)
        specs = (A.hk_pl_spectrum * max(1, len(self.spectra)))()
        for i, s in enumerate(self.spectra):
            specs[i].n = s.lambdas.size
            specs[i].lambdas = s.lambdas.ctypes.data_as(A.PF)
            specs[i].values = s.values.ctypes.data_as(A.PF)
        media_recs, media_keep = _media_records(self.media)
        keep.append(media_keep)
        d = A.hk_scene_desc()
        d.n_triangles, d.n_materials, d.n_textures = T, len(self.materials), len(self.textures)
        envs = (A.hk_envmap * max(1, len(self._envmaps)))()
        for i, e in enumerate(self._envmaps):
            envs[i] = e.record()
        d.n_media_interfaces, d.n_lights, d.n_envmaps, d.n_media, d.n_spectra = len(self.media_interfaces), len(fl), len(self._envmaps), len(self.media), len(self.spectra)
        d.positions = P.ctypes.data_as(A.PF)
        d.normals = Nn.ctypes.data_as(A.PF) if Nn is not None else None
        d.uvs = np.ascontiguousarray(Uv, dtype=f32).ctypes.data_as(A.PF) if Uv is not None else None
        if Uv is not None:
            Uv = np.ascontiguousarray(Uv, dtype=f32)
            d.uvs = Uv.ctypes.data_as(A.PF)
        if Nn is not None:
            Nn = np.ascontiguousarray(Nn, dtype=f32)
            d.normals = Nn.ctypes.data_as(A.PF)
        d.tangents = None
        d.meta = metas.ctypes.data_as(C.POINTER(A.hk_tri_meta))
        d.materials, d.textures, d.media_interfaces, d.lights = mats, texs, mis, lts
        d.envmaps, d.media, d.spectra = envs, media_recs, specs
        self._keep = (P, Nn, Uv, metas, mats, mis, lts, texs, specs, keep, media_recs, envs, list(self._envmaps))
        self._desc = d
        if T:
            lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
            c = (lo + hi) * f32(0.5)
            self.bounds = (lo, hi, c, float(np.linalg.norm(hi - c)))
        self._device = {}
        self._stale_media, self._media_keep = set(), {}
        return self

    def close(self):
        """Release every device scene (BVH, leaf triangles, textures, env maps, media) created from this Scene."""
        dev, self._device = getattr(self, "_device", None) or {}, {}
        if dev:
            from . import _lib
            L = _lib.lib()
            for h in dev.values():
                L.hk_scene_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _description(self, bake_skies=True):
        """The kept description, complete: stale media records refilled, pending sky bakes run.  bake_skies=False is for a reader that
        follows no environment-map pointer (volpath.scene_handle with a device scene in hand)."""
        if self._desc is None:
            self.sync()
        if self._stale_media:
            self._refresh_media()
        if bake_skies:
            self._bake_skies()
        return self._desc

    @property
    def desc(self):
        return self._description()

    def world_radius(self):
        self.desc
        return self.bounds[3]


def _alpha_tested(rec):
    """The opacity class hk_scene_create derives from a record (Matte with an alpha texture or alpha < 1)."""
    return rec.kind == A.HK_MAT_MATTE and (rec.rgb[0].tex >= 0 or rec.rgb[0].c[3] < 1.0)


def _media_records(media):
    recs = (A.hk_medium * max(1, len(media)))()
    keep = []
    for i, m in enumerate(media):
        m.fill_record(recs[i], keep)
    return recs, keep
