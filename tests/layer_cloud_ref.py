"""numpy restatement of the layer point clouds (include/voxgraph_amd.h, "Layer point clouds"), written from the header's
rules: one voxel at a time in meaning, whole arrays in form.  Every operation is f32 (numpy keeps f32 op f32 in f32).

    layer_cloud(voxel_size, vps, block_index [n][3], distance [n][vps^3], seen [n][vps^3], kind, ...)
        -> xyz [m][3] f32, intensity [m] f32, rgba [m][4] u8 or None, per_block [n] (points each block contributed)

`seen` is the ESDF's observed (u8; esdf=True) or the TSDF's weight (f32; esdf=False)."""
import numpy as np

F = np.float32
DISTANCE, SURFACE_DISTANCE, SURFACE_COLOR = 0, 1, 2
MIN_WEIGHT = F(1e-3)              # ptcloud_vis.h kMinWeight [recalled]
SLICE_TOLERANCE = F(1e-6)         # voxblox kFloatingPointTolerance [recalled]


def voxel_centres(voxel_size, vps, block_index):
    """[n][vps^3][3] f32: origin + (idx + 0.5) * voxel_size, origin = (float)block_index * ((float)vps * voxel_size);
    linear index x fastest"""
    vs = F(voxel_size)
    block_size = F(vps) * vs
    origin = np.asarray(block_index, np.int32).astype(F) * block_size          # [n][3]
    lin = np.arange(vps ** 3)
    idx = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], -1).astype(F)
    return origin[:, None, :] + (idx[None] + F(0.5)) * vs


def layer_cloud(voxel_size, vps, block_index, distance, seen, kind=DISTANCE, surface_distance=0.6, min_weight=MIN_WEIGHT,
                slice_axis=-1, slice_value=0.0, esdf=True, rgba=None):
    n = len(block_index)
    nv = vps ** 3
    d = np.asarray(distance, F).reshape(n, nv)
    if esdf:
        keep = np.asarray(seen, np.uint8).reshape(n, nv) != 0
    else:
        with np.errstate(invalid="ignore"):
            keep = np.asarray(seen, F).reshape(n, nv) > F(min_weight)           # strictly; NaN is not observed
    if kind != DISTANCE:
        with np.errstate(invalid="ignore"):
            keep = keep & (np.abs(d) < F(surface_distance))                      # strictly; NaN and inf fail
    c = voxel_centres(voxel_size, vps, block_index)
    if slice_axis >= 0:
        reach = F(0.5) * F(voxel_size) + SLICE_TOLERANCE
        keep = keep & (np.abs(c[:, :, slice_axis] - F(slice_value)) <= reach)    # not strictly
    # blocks in slot order, voxels in linear-index order: the row-major order of `keep`
    xyz = c[keep]
    inten = d[keep]
    col = None
    if kind == SURFACE_COLOR:
        col = np.asarray(rgba, np.uint8).reshape(n, nv, 4)[keep]
    return xyz.astype(F), inten, col, keep.sum(1)


def bits(a):
    """the array's bytes, for exact comparison (NaN payloads and signed zeros included)"""
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
