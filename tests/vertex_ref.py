"""Deformations for the vertex-edit tests (tests/test_vertex_edits.py, tests/test_vertex_edits_host.py): plain NumPy in binary32, so the
edited scene and the scene built fresh from the deformed mesh are handed the same bits."""
import numpy as np

f32 = np.float32


def face_normals(P):
    """[T, 3, 3]: the unit face normal of every triangle at its three vertices (a degenerate face keeps (0, 0, 1))."""
    P = np.asarray(P, f32)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).astype(f32)
    ln = np.linalg.norm(n, axis=1, keepdims=True).astype(f32)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), np.array([0, 0, 1], f32)).astype(f32)
    return np.ascontiguousarray(np.repeat(n[:, None, :], 3, axis=1))


def ripple(P, N, amplitude=0.1, freq=9.0, phase=0.0):
    """Vertices pushed along their normals by amplitude * sin(freq * (x + 2y + 3z) + phase) — a function of the position, so vertices
    shared between triangles stay together — and the face normals of the result.  -> (positions, normals) float32 [T, 3, 3]."""
    P, N = np.asarray(P, f32), np.asarray(N, f32)
    s = np.sin(f32(freq) * (P[..., 0] + f32(2) * P[..., 1] + f32(3) * P[..., 2]) + f32(phase)).astype(f32)
    Q = np.ascontiguousarray((P + f32(amplitude) * s[..., None] * N).astype(f32))
    return Q, face_normals(Q)


def swirl_uvs(uvs, shift=0.25):
    """Other texture coordinates for the same faces: (u, v) -> (v + shift, u) wrapped into [0, 1)."""
    uvs = np.asarray(uvs, f32)
    out = np.stack([np.mod(uvs[..., 1] + f32(shift), f32(1)), uvs[..., 0]], axis=-1)
    return np.ascontiguousarray(out.astype(f32))
