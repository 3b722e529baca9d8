"""NumPy reference of hk_scene_set_transform's arithmetic (include/hikari_mi355x.h, "Editing a scene in place"): binary32, one
rounding per operation, in the header's order.  The GPU tests build the "fresh" scene from geometry moved by this module and compare
it bit for bit with the scene the device moved."""
import numpy as np

f32 = np.float32

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)


def is_identity(m34):
    return bool((np.asarray(m34, f32) == IDENTITY).all())


def normal_matrix(m34):
    """N[i][j] = (float)(C[i][j] / det): cofactors and determinant of the linear part in double."""
    A = np.asarray(m34, f32)[:, :3].astype(np.float64)
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i, j] = A[i1, j1] * A[i2, j2] - A[i1, j2] * A[i2, j1]
    det = (A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1]) + A[0, 2] * C[0, 2]
    if not (det != 0.0 and np.isfinite(det)):
        raise ValueError("singular transform")
    return (C / det).astype(f32)


def transform_points(m34, p):
    """p'[k] = ((m[k][0]*x + m[k][1]*y) + m[k][2]*z) + m[k][3] for points p[..., 3] (float32)."""
    m = np.asarray(m34, f32)
    p = np.asarray(p, f32)
    if is_identity(m):
        return p.copy()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = np.empty_like(p)
    for k in range(3):
        out[..., k] = ((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]
    return out


def transform_dirs(M3, v):
    """n' = (M[k][0]*x + M[k][1]*y) + M[k][2]*z, then n' / sqrt((x*x + y*y) + z*z); a vector with a NaN component is kept."""
    M = np.asarray(M3, f32)
    v = np.asarray(v, f32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    r = np.empty_like(v)
    for k in range(3):
        r[..., k] = (M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
        out = r / ln[..., None]
    keep = np.isnan(v).any(axis=-1)
    out[keep] = v[keep]
    return out


def transform_mesh(m34, positions, normals=None, tangents=None):
    """(positions, normals, tangents) of triangles [T, 3, 3] moved by m34, as the device moves them."""
    m = np.asarray(m34, f32)
    if is_identity(m):
        return tuple(None if a is None else np.array(a, f32) for a in (positions, normals, tangents))
    P = transform_points(m, positions)
    N = None if normals is None else transform_dirs(normal_matrix(m), normals)
    Tg = None if tangents is None else transform_dirs(m[:, :3], tangents)
    return P, N, Tg


def affine(rot_deg=0.0, axis=(0, 1, 0), scale=1.0, translate=(0, 0, 0)):
    """A 4x4 float32 affine transform: uniform scale, then a rotation about `axis`, then a translation."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(rot_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = R * scale
    m[:3, 3] = translate
    return m.astype(f32)
