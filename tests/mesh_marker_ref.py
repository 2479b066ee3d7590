"""CPU restatement of vgx_mesh_fill_marker (include/voxgraph_amd.h, "Mesh markers"): voxblox_ros fillMarkerWithMesh
[recalled] over a triangle soup -- marker.points [3T][3] f64 and marker.colors [3T][4] f32 in voxblox's ColorMode,
vectorised numpy.  voxblox_ros is not vendored: everything about it here is [recalled].

Rules: marker point j = 3 t + c is soup vertex j; points are the f32 coordinates widened; alpha = opacity everywhere; a
vertex's colour is its triangle's (or constant_rgba); c8(k) = (float)((double)k / 255.0); GRAY 0.5f; COLOR c8 per
channel; NORMALS (float)((double)n * 0.5 + 0.5); LAMBERT_COLOR in f32 without contraction, two lights normalised by
sqrtf((x*x + y*y) + z*z), d_i = max0((n.x*L.x + n.y*L.y) + n.z*L.z), v = (d1*c + d2*c) + 0.2f clamped at 1; LAMBERT the
same with (127, 127, 127); HEIGHT per vertex from its own z: t = (float)(((double)z + 1.0) / 11.0) clamped to [0, 1], the
bytes of rainbowColorMap((double)t) through c8 (a z that is not a number takes the map's default case, 255 127 127)."""
import numpy as np

F = np.float32

COLOR, HEIGHT, NORMALS, GRAY, LAMBERT, LAMBERT_COLOR = 0, 1, 2, 3, 4, 5
MODES = (COLOR, HEIGHT, NORMALS, GRAY, LAMBERT, LAMBERT_COLOR)
TRIANGLE_LIST = 11

C8 = (np.arange(256, dtype=np.float64) / 255.0).astype(F)


def _normalised(x, y, z):
    x, y, z = F(x), F(y), F(z)
    length = np.sqrt(F(F(x * x + y * y) + z * z))
    return np.array([x / length, y / length, z / length], F)


L1 = _normalised(0.8, -0.2, 0.7)
L2 = _normalised(-0.5, 0.2, 0.2)


def height_ratio(z):
    """t of a vertex at height z [..] f32: (float)(((double)z + 1.0) / 11.0) clamped to [0, 1]"""
    t = ((np.asarray(z, F).astype(np.float64) + 1.0) / 11.0).astype(F)
    t = np.where(t < 0, F(0), t)
    return np.where(F(1) < t, F(1), t).astype(F)


def rainbow_sector(t):
    """the sector i = floor(6 (h - floor(h))) of rainbowColorMap((double)t)"""
    h = np.asarray(t, F).astype(np.float64)
    h = h - np.floor(h)
    return np.floor(h * 6.0).astype(np.int64)


def rainbow_bytes(t):
    """voxblox rainbowColorMap((double)t) for t [..] f32, vectorised: [.., 3] uint8 (r, g, b)"""
    h = np.asarray(t, F).astype(np.float64)
    h = h - np.floor(h)
    h = h * 6.0
    nan = np.isnan(h)                                            # a z that is not a number: the map's default case
    h = np.where(nan, 0.0, h)
    i = np.where(nan, -1, np.floor(h).astype(np.int64))
    f = h - i
    f = np.where(i % 2 == 0, 1.0 - f, f)
    mid = np.where(nan, 0, (255.0 * (1.0 - f)).astype(np.int64))
    hi, lo = np.full_like(mid, 255), np.zeros_like(mid)
    r = np.select([(i == 0) | (i == 6), i == 1, i == 2, i == 3, i == 4, i == 5], [hi, mid, lo, lo, mid, hi], 255)
    g = np.select([(i == 0) | (i == 6), i == 1, i == 2, i == 3, i == 4, i == 5], [mid, hi, hi, mid, lo, lo], 127)
    b = np.select([(i == 0) | (i == 6), i == 1, i == 2, i == 3, i == 4, i == 5], [lo, lo, mid, hi, hi, mid], 127)
    return np.stack([r, g, b], -1).astype(np.uint8)


def _light(n, L):
    d = (n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2]      # f32 arrays: every product and sum rounds to f32
    return np.where(d < 0, F(0), d).astype(F)


def triangle_rgb(normals, rgba, mode):
    """[T][3] f32: the colour every mode but HEIGHT gives the three vertices of a triangle"""
    n = np.ascontiguousarray(normals, F).reshape(-1, 3)
    T = len(n)
    if mode == GRAY:
        return np.full((T, 3), 0.5, F)
    if mode == NORMALS:
        return (n.astype(np.float64) * 0.5 + 0.5).astype(F)
    if mode == LAMBERT:
        rgba = np.tile(np.array([127, 127, 127, 255], np.uint8), (T, 1))
    if rgba is None:
        raise ValueError("the mesh has no colours")              # voxblox CHECKs hasColors()
    c = C8[np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)[:, :3]]
    if mode == COLOR:
        return c
    if mode not in (LAMBERT, LAMBERT_COLOR):
        raise ValueError("unknown color mode")
    d1, d2 = _light(n, L1)[:, None], _light(n, L2)[:, None]
    v = (d1 * c + d2 * c) + F(0.2)
    return np.where(F(1) < v, F(1), v).astype(F)


def fill_marker(vertices, normals, rgba, mode, opacity=1.0, constant_rgba=None):
    """vertices [T][3][3] f32, normals [T][3] f32, rgba [T][4] uint8 or None (a mesh without colours); constant_rgba
    [4]: the colour of every triangle instead.  Returns (points [3T][3] f64, colors [3T][4] f32)."""
    if mode not in MODES:
        raise ValueError("unknown color mode")
    if not np.isfinite(opacity):
        raise ValueError("opacity not finite")
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3, 3)
    T = len(v)
    if constant_rgba is not None:
        rgba = np.tile(np.asarray(constant_rgba, np.uint8).reshape(1, 4), (T, 1))
    points = v.reshape(-1, 3).astype(np.float64)
    colors = np.empty((3 * T, 4), F)
    colors[:, 3] = F(opacity)
    if mode == HEIGHT:
        colors[:, :3] = C8[rainbow_bytes(height_ratio(v.reshape(-1, 3)[:, 2]))]
    else:
        colors[:, :3] = np.repeat(triangle_rgb(normals, rgba, mode), 3, axis=0)
    return points, colors


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
