"""numpy restatement of the elevation map (include/voxgraph_amd.h, "Elevation map"), written from the header's rules: one
cell at a time in meaning, whole grids in form.  Every float operation is f32 (numpy keeps f32 op f32 in f32); counts,
the run of free voxels, the support and the distance passes are integers.  Cell, grid order, box, observed, band and the
distance are the planar map's rules, and their restatement is that of tests/planar_map_ref.py.

    elevation_map(voxel_size, vps, block_index [n][3], distance [n][vps^3], seen [n][vps^3], esdf, z_min, z_max, ...)
        -> x0, y0, W, H, state / height / headroom / crossings / support / step / grad / slope / slope_valid / cls /
           distance [H][W] (grad [H][W][2]), state_counts, class_counts, R, and for the scenes' census: n_free, n_solid,
           n_cross (unsaturated), t and z_row (of the chosen crossing: t is NaN where there is none; z_row the global row of
           its solid voxel), obstacle

`seen` is the ESDF's observed (u8; esdf=True) or the TSDF's weight (f32; esdf=False).  Block indices are distinct."""
from types import SimpleNamespace

import numpy as np

from tests.planar_map_ref import MAX_CELLS, MAX_R, MIN_WEIGHT, brute_force_distance, planar_distance, radius, row_centres  # noqa: F401

F = np.float32
FIELDS = ("state", "height", "headroom", "crossings", "support", "step", "grad", "slope", "slope_valid", "cls", "distance")
MAX_RADIUS = 64


def _shift(a, dy, dx, fill):
    """b[y][x] = a[y + dy][x + dx] where that cell is inside the grid, else fill"""
    H, W = a.shape
    out = np.full_like(a, fill)
    ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ya < yb and xa < xb:
        out[ya:yb, xa:xb] = a[ya + dy:yb + dy, xa + dx:xb + dx]
    return out


def step_and_support(surface, height, r):
    """the separable window: a row pass, then a column pass; exact min, max (f32) and count (int)"""
    lo = np.where(surface, height, F(np.inf)).astype(F)
    hi = np.where(surface, height, F(-np.inf)).astype(F)
    n = surface.astype(np.int32)
    for axis in (1, 0):
        lo2, hi2, n2 = lo.copy(), hi.copy(), n.copy()
        for k in range(1, r + 1):
            for s in (-k, k):
                d = (0, s) if axis == 1 else (s, 0)
                lo2 = np.minimum(lo2, _shift(lo, *d, F(np.inf)))
                hi2 = np.maximum(hi2, _shift(hi, *d, F(-np.inf)))
                n2 = n2 + _shift(n, *d, 0)
        lo, hi, n = lo2, hi2, n2
    with np.errstate(invalid="ignore"):
        step = np.where(surface, hi - lo, F(0)).astype(F)
    return step, np.where(surface, n, 0).astype(np.uint16)


def _axis(surface, height, vs, dy, dx):
    """one axis of the gradient: (defined, g)"""
    right, left = _shift(surface, dy, dx, False), _shift(surface, -dy, -dx, False)
    h_r, h_l = _shift(height, dy, dx, F(0)), _shift(height, -dy, -dx, F(0))
    both = (h_r - h_l) / (F(2.0) * vs)
    only_r = (h_r - height) / vs
    only_l = (height - h_l) / vs
    g = np.where(right & left, both, np.where(right, only_r, only_l)).astype(F)
    defined = surface & (right | left)
    return defined, np.where(defined, g, F(0)).astype(F)


def brute_force_step(surface, height, r):
    """max - min and the count over the whole window at once, cell by cell"""
    H, W = surface.shape
    step, support = np.zeros((H, W), F), np.zeros((H, W), np.uint16)
    for y, x in zip(*np.nonzero(surface)):
        win = (slice(max(0, y - r), y + r + 1), slice(max(0, x - r), x + r + 1))
        hs = height[win][surface[win]]
        step[y, x], support[y, x] = hs.max() - hs.min(), len(hs)
    return step, support


def elevation_map(voxel_size, vps, block_index, distance, seen, esdf, z_min, z_max, min_weight=MIN_WEIGHT, min_free_voxels=1, pick=0,
                  step_radius_cells=1, min_support=1, max_slope=1.0, max_step_m=0.2, min_headroom_voxels=1, hole_is_obstacle=1,
                  unknown_is_obstacle=0, max_distance_m=2.0, use_box=0, cell_min=(0, 0), cell_dim=(0, 0)):
    assert pick in (0, 1) and 0 <= step_radius_cells <= MAX_RADIUS and min_support >= 1 and min_headroom_voxels >= 1
    vs = F(voxel_size)
    bi = np.asarray(block_index, np.int32).reshape(-1, 3)
    n = len(bi)
    d = np.asarray(distance, F).reshape(n, vps, vps, vps)                        # [b][z][y][x]
    if esdf:
        observed = np.asarray(seen, np.uint8).reshape(n, vps, vps, vps) != 0
    else:
        with np.errstate(invalid="ignore"):
            observed = np.asarray(seen, F).reshape(n, vps, vps, vps) > F(min_weight)   # strictly; NaN is not observed
    cz = row_centres(voxel_size, vps, bi[:, 2])                                  # [b][lz]
    in_band = (F(z_min) <= cz) & (cz <= F(z_max))
    has_row = in_band.any(1)
    if use_box:
        x0, y0, W, H = int(cell_min[0]), int(cell_min[1]), int(cell_dim[0]), int(cell_dim[1])
    elif has_row.any():
        lo, hi = bi[has_row, :2].min(0).astype(np.int64), bi[has_row, :2].max(0).astype(np.int64)
        x0, y0 = int(lo[0]) * vps, int(lo[1]) * vps
        W, H = int(hi[0] - lo[0] + 1) * vps, int(hi[1] - lo[1] + 1) * vps
    else:
        x0 = y0 = W = H = 0
    assert W >= 0 and H >= 0 and W * H <= MAX_CELLS

    run = np.zeros((H, W), np.int32)
    d_u = np.zeros((H, W), F)
    n_free, n_solid, n_cross = (np.zeros((H, W), np.int32) for _ in range(3))
    height = np.zeros((H, W), F)
    headroom = np.zeros((H, W), np.int32)
    t_pick = np.full((H, W), np.nan, F)
    z_row = np.zeros((H, W), np.int64)                                           # global row of the chosen crossing's solid voxel
    if n and W * H:
        # every row of every z block from the highest block to the lowest, downwards: a block that is missing under a cell
        # leaves its rows unclassified there (so they reset the run), and so does a row out of the band
        zs = range(int(bi[:, 2].max()), int(bi[:, 2].min()) - 1, -1)
        centres = row_centres(voxel_size, vps, list(zs))                         # the same centres, from the z index alone
        for k, bz in enumerate(zs):
            members = []
            for b in np.flatnonzero(bi[:, 2] == bz):
                bx0, by0 = int(bi[b, 0]) * vps - x0, int(bi[b, 1]) * vps - y0    # the block's corner in cells
                xa, xb, ya, yb = max(bx0, 0), min(bx0 + vps, W), max(by0, 0), min(by0 + vps, H)
                if xa < xb and ya < yb:
                    members.append((b, (slice(ya, yb), slice(xa, xb)), (slice(ya - by0, yb - by0), slice(xa - bx0, xb - bx0))))
            for lz in range(vps - 1, -1, -1):
                c = centres[k, lz]
                if not (F(z_min) <= c <= F(z_max)):
                    run[:] = 0
                    continue
                dd = np.full((H, W), np.nan, F)
                classified = np.zeros((H, W), bool)
                for b, cell, vox in members:
                    dd[cell] = d[b, lz][vox]
                    classified[cell] = observed[b, lz][vox] & ~np.isnan(d[b, lz][vox])
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    free = classified & (dd > F(0))
                    solid = classified & ~free
                    cross = solid & (run >= 1)
                    t = (-dd) / (d_u - dd)
                    t = np.where((t >= F(0)) & (t <= F(1)), t, F(0.5)).astype(F)
                    h = (c + t * vs).astype(F)
                take = cross & ((n_cross == 0) | (pick == 1))
                height = np.where(take, h, height)
                headroom = np.where(take, run, headroom)
                t_pick = np.where(take, t, t_pick)
                z_row = np.where(take, bz * vps + lz, z_row)
                n_cross += cross
                n_free += free
                n_solid += solid
                d_u = np.where(free, dd, d_u)
                run = np.where(free, run + 1, 0).astype(np.int32)
    state = np.where(n_cross >= 1, 1, np.where(n_solid >= 1, 3, np.where(n_free >= int(min_free_voxels), 2, 0))).astype(np.uint8)
    surface = state == 1
    height = np.where(surface, height, F(0)).astype(F)
    headroom = np.where(surface, headroom, 0).astype(np.int32)
    crossings = np.minimum(n_cross, 255).astype(np.uint8)

    step, support = step_and_support(surface, height, int(step_radius_cells))
    with np.errstate(over="ignore", invalid="ignore"):
        has_x, gx = _axis(surface, height, vs, 0, 1)
        has_y, gy = _axis(surface, height, vs, 1, 0)
        valid = has_x & has_y
        gx, gy = np.where(valid, gx, F(0)).astype(F), np.where(valid, gy, F(0)).astype(F)
        slope = np.where(valid, np.sqrt(gx * gx + gy * gy), F(0)).astype(F)
    grad = np.stack([gx, gy], -1).astype(F)

    cls = np.zeros((H, W), np.uint8)                                             # 1. state 0
    cls[state == 3] = 2                                                          # 2.
    cls[state == 2] = 2 if hole_is_obstacle else 0                               # 3.
    low = surface & (headroom < int(min_headroom_voxels))                        # 4., in its order
    unsure = surface & ~low & (~valid | (support < int(min_support)))
    with np.errstate(invalid="ignore"):
        bad = surface & ~low & ~unsure & ((slope > F(max_slope)) | (step > F(max_step_m)))
    cls[low] = 2
    cls[unsure] = 0
    cls[bad] = 2
    cls[surface & ~low & ~unsure & ~bad] = 1

    obstacle = (cls == 2) | ((cls == 0) if unknown_is_obstacle else np.zeros((H, W), bool))
    R = radius(max_distance_m, voxel_size)
    assert 1 <= R <= MAX_R
    dist = planar_distance(obstacle, R, voxel_size, max_distance_m)
    return SimpleNamespace(x0=x0, y0=y0, W=W, H=H, state=state, height=height, headroom=headroom, crossings=crossings, support=support,
                           step=step, grad=grad, slope=slope, slope_valid=valid.astype(np.uint8), cls=cls, distance=dist,
                           state_counts=tuple(int((state == k).sum()) for k in range(4)),
                           class_counts=tuple(int((cls == k).sum()) for k in range(3)), R=R, n_free=n_free, n_solid=n_solid,
                           n_cross=n_cross, t=t_pick, z_row=z_row, obstacle=obstacle)


def bits(a):
    """the array's bytes, for exact comparison (NaN payloads and signed zeros included)"""
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
