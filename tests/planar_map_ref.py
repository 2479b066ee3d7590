"""numpy restatement of the planar map (include/voxgraph_amd.h, "Planar map"), written from the header's rules: one voxel
at a time in meaning, whole arrays in form.  Every float operation is f32 (numpy keeps f32 op f32 in f32); counts, the
row pass and the column pass are integers.

    planar_map(voxel_size, vps, block_index [n][3], distance [n][vps^3], seen [n][vps^3], esdf, z_min, z_max, ...)
        -> PlanarMap: x0, y0, W, H, state / occupancy / clearance / height / distance [H][W], n_occ / n_free [H][W],
           counts (unknown, free, occupied), R, z_blocks [H][W] (z blocks that gave a cell a classified voxel)

`seen` is the ESDF's observed (u8; esdf=True) or the TSDF's weight (f32; esdf=False).  Block indices are distinct."""
import math
from types import SimpleNamespace

import numpy as np

F = np.float32
MIN_WEIGHT = F(1e-3)
NONE = np.int64(1) << 40          # "no obstacle within R" of the integer passes
MAX_R = 2048
MAX_CELLS = 1 << 28


def row_centres(voxel_size, vps, bz):
    """[len(bz)][vps] f32: cz = (float)bz * ((float)vps * voxel_size) + ((float)lz + 0.5) * voxel_size"""
    vs = F(voxel_size)
    origin = np.asarray(bz, np.int32).astype(F) * (F(vps) * vs)
    return origin[:, None] + (np.arange(vps).astype(F)[None] + F(0.5)) * vs


def radius(max_distance_m, voxel_size):
    return int(math.ceil(float(F(max_distance_m)) / float(F(voxel_size))))


def planar_distance(obstacle, R, voxel_size, max_distance_m):
    """the row pass, the column pass and the clip over obstacle [H][W] bool -> f32 [H][W]"""
    H, W = obstacle.shape
    out = np.full((H, W), F(max_distance_m), F)
    if H == 0 or W == 0:
        return out
    xs = np.arange(W, dtype=np.int64)
    # row pass: the nearest obstacle at or left of x, and at or right of x, by running maxima / minima
    left = np.maximum.accumulate(np.where(obstacle, xs[None], -NONE), axis=1)
    right = np.minimum.accumulate(np.where(obstacle, xs[None], NONE)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(xs[None] - left, right - xs[None])
    g = np.where(g <= R, g, NONE)                                                # [y][x]
    # column pass: every row offset dy that stays inside the grid
    g2 = np.where(g != NONE, g, 0) ** 2
    d2 = np.full((H, W), NONE, np.int64)
    for dy in range(max(-R, -(H - 1)), min(R, H - 1) + 1):
        ya, yb = max(0, -dy), min(H, H - dy)                                     # rows y with y + dy in the grid
        cand = np.where(g[ya + dy:yb + dy] != NONE, dy * dy + g2[ya + dy:yb + dy], NONE)
        d2[ya:yb] = np.minimum(d2[ya:yb], cand)
    found = d2 != NONE
    m = np.sqrt(np.where(found, d2, 0).astype(F)) * F(voxel_size)
    return np.where(found & (m < F(max_distance_m)), m, F(max_distance_m)).astype(F)


def brute_force_distance(obstacle, voxel_size, max_distance_m):
    """the exact Euclidean transform over ALL cell pairs (no window), integer d2, then the same f32 tail"""
    H, W = obstacle.shape
    out = np.full((H, W), F(max_distance_m), F)
    oy, ox = np.nonzero(obstacle)
    if len(oy) == 0 or H * W == 0:
        return out
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = ((yy[:, :, None] - oy) ** 2 + (xx[:, :, None] - ox) ** 2).min(2)
    m = np.sqrt(d2.astype(F)) * F(voxel_size)
    return np.where(m < F(max_distance_m), m, F(max_distance_m)).astype(F)


def planar_map(voxel_size, vps, block_index, distance, seen, esdf, z_min, z_max, occupied_distance=0.0, min_weight=MIN_WEIGHT,
               min_free_voxels=1, unknown_is_obstacle=0, max_distance_m=2.0, use_box=0, cell_min=(0, 0), cell_dim=(0, 0)):
    bi = np.asarray(block_index, np.int32).reshape(-1, 3)
    n, nv = len(bi), vps ** 3
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
    with np.errstate(invalid="ignore"):
        occupied_v = observed & in_band[:, :, None, None] & (d <= F(occupied_distance))
        free_v = observed & in_band[:, :, None, None] & (d > F(occupied_distance))
    n_occ = np.zeros((H, W), np.int32)
    n_free = np.zeros((H, W), np.int32)
    z_blocks = np.zeros((H, W), np.int32)
    any_v = np.zeros((H, W), bool)
    clearance = np.zeros((H, W), F)
    height = np.zeros((H, W), F)
    # ascending global z: blocks by their z index (one block per (x, y, z): no tie matters), rows inside a block upwards
    for b in np.argsort(bi[:, 2], kind="stable"):
        if not has_row[b] or W * H == 0:
            continue
        bx0, by0 = int(bi[b, 0]) * vps - x0, int(bi[b, 1]) * vps - y0            # the block's corner in cells
        xa, xb, ya, yb = max(bx0, 0), min(bx0 + vps, W), max(by0, 0), min(by0 + vps, H)
        if xa >= xb or ya >= yb:
            continue
        cell = (slice(ya, yb), slice(xa, xb))
        vox = (slice(ya - by0, yb - by0), slice(xa - bx0, xb - bx0))
        gave = np.zeros((yb - ya, xb - xa), bool)
        for lz in range(vps):
            if not in_band[b, lz]:
                continue
            occ, fre, dd = occupied_v[b, lz][vox], free_v[b, lz][vox], d[b, lz][vox]
            cls = occ | fre
            with np.errstate(invalid="ignore"):
                take = cls & (~any_v[cell] | (dd < clearance[cell]))             # strictly: the first of a tie stays
            clearance[cell] = np.where(take, dd, clearance[cell])
            any_v[cell] |= cls
            n_occ[cell] += occ
            n_free[cell] += fre
            height[cell] = np.where(occ, cz[b, lz], height[cell])
            gave |= cls
        z_blocks[cell] += gave
    state = np.where(n_occ >= 1, 2, np.where(n_free >= int(min_free_voxels), 1, 0)).astype(np.uint8)
    clearance = np.where(state != 0, clearance, F(0)).astype(F)
    height = np.where(state == 2, height, F(0)).astype(F)
    occupancy = np.array([-1, 0, 100], np.int8)[state]
    obstacle = (state == 2) | ((state == 0) if unknown_is_obstacle else np.zeros((H, W), bool))
    R = radius(max_distance_m, voxel_size)
    assert 1 <= R <= MAX_R
    dist = planar_distance(obstacle, R, voxel_size, max_distance_m)
    counts = tuple(int((state == k).sum()) for k in range(3))
    return SimpleNamespace(x0=x0, y0=y0, W=W, H=H, state=state, occupancy=occupancy, clearance=clearance, height=height,
                           distance=dist, n_occ=n_occ, n_free=n_free, counts=counts, R=R, z_blocks=z_blocks, obstacle=obstacle)


def bits(a):
    """the array's bytes, for exact comparison (NaN payloads and signed zeros included)"""
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
