"""The connected mesh restated in numpy: the rules of vgx_mesh_connect (include/voxgraph_amd.h) -- voxblox
createConnectedMesh [recalled] over a triangle soup in vgx_mesh_download's order.  The device is compared with this bit
for bit (tests/test_connected_mesh_gpu.py); tests/test_connected_mesh_cpu.py checks it by properties that do not trust it."""
import numpy as np

F = np.float32
DEFAULT_THRESHOLD = F(1e-10)          # voxblox's approximate_vertex_proximity_threshold default


def round_half_away(x):
    """std::round on f64: halves away from zero (np.round is half-to-even).  floor(|x|) and |x| - floor(|x|) are exact
    in f64, so is the comparison with 0.5; the sign is restored (-0.0 stays -0.0 and casts to 0)."""
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + ((a - f) >= 0.5), x)


def keys(points, threshold):
    """[N][3] int64: round((double)v * inv), inv = 1.0 / (double)(f32 threshold).  Raises where the library refuses."""
    t = F(threshold)
    if not np.isfinite(t) or not t > 0:
        raise ValueError("threshold not finite or not > 0")
    inv = np.float64(1.0) / np.float64(t)
    p = np.asarray(points, F).reshape(-1, 3).astype(np.float64) * inv
    if not np.all(np.abs(p) < 2.0 ** 62):           # (NaN and the infinities fail the comparison)
        raise OverflowError("a coordinate is not finite or |v * inv| >= 2^62")
    return round_half_away(p).astype(np.int64)


def connect(vertices, normals, colors=None, threshold=DEFAULT_THRESHOLD):
    """vertices [T][3][3] f32, normals [T][3] f32, colors [T][4] u8 or None ->
    (vertices [V][3] f32, normals [V][3] f32, rgba [V][4] u8 or None, indices [T][3] u32)"""
    soup = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    if len(soup) == 0:
        return (np.zeros((0, 3), F), np.zeros((0, 3), F), None if colors is None else np.zeros((0, 4), np.uint8),
                np.zeros((0, 3), np.uint32))
    k = keys(soup, threshold)
    _, first, inverse = np.unique(k, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")        # unique keys by first occurrence
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    rep = first[order]                              # the first soup vertex of each key, ascending
    rgba = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)[rep // 3]
    return soup[rep], normals[rep // 3], rgba, rank[np.asarray(inverse).ravel()].reshape(-1, 3).astype(np.uint32)
