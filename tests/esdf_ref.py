"""Device-free numpy restatement of the device ESDF (voxgraph_amd/csrc/vgx_esdf.hip): esdf_init_kernel, then the recurrence of
esdf_relax_kernel iterated as whole-grid Jacobi sweeps in f32 until nothing changes.

The recurrence lowers |d(v)| to the smallest |d(n)| + step over the 26 neighbours n of the same strict sign with
|d(n)| < max_distance_m.  f32 addition is monotone (a <= b gives a + s <= b + s after rounding), values only ever fall and a
lower value is never a worse source, so every fair order of relaxations -- the device's block-parallel in-LDS sweeps, these
Jacobi sweeps -- ends in the same greatest fixed point: each value is the smallest left-to-right f32 sum along any path from a
source.  The device layer therefore equals this one BIT FOR BIT; the tests compare with np.array_equal on the bits.

Every operation below is a single f32 operation on f32 arrays (numpy does not contract a multiply and an add), as the kernel is
compiled with fp contract off."""
import numpy as np

F = np.float32


def _grid(bi, vps, rows, fill):
    """[n][vps^3] block rows (x fastest) -> dense [Z][Y][X] over the blocks' bounding box with a one-voxel rim of `fill`"""
    lo = bi.min(0)
    dims = (bi.max(0) - lo + 1) * vps
    out = np.full((dims[2] + 2, dims[1] + 2, dims[0] + 2), fill, rows.dtype)
    for b in range(len(bi)):
        ox, oy, oz = (bi[b] - lo) * vps + 1
        out[oz:oz + vps, oy:oy + vps, ox:ox + vps] = rows[b].reshape(vps, vps, vps)
    return out


def _rows(bi, vps, grid):
    lo = bi.min(0)
    out = np.empty((len(bi), vps ** 3), grid.dtype)
    for b in range(len(bi)):
        ox, oy, oz = (bi[b] - lo) * vps + 1
        out[b] = grid[oz:oz + vps, oy:oy + vps, ox:ox + vps].reshape(-1)
    return out


def esdf_from_tsdf(voxel_size, vps, block_index, tsdf_distance, tsdf_weight, max_distance_m=2.0, min_distance_m=0.2,
                   default_distance_m=2.0, min_weight=1e-6, return_sweeps=False):
    """-> (esdf_distance [n][vps^3] f32, esdf_observed [n][vps^3] u8) in the submap's block order and voxel order (x fastest);
    with return_sweeps also the number of Jacobi sweeps that changed something"""
    bi = np.ascontiguousarray(block_index, np.int64).reshape(-1, 3)
    n, nv = len(bi), vps ** 3
    td = np.ascontiguousarray(tsdf_distance, F).reshape(n, nv)
    tw = np.ascontiguousarray(tsdf_weight, F).reshape(n, nv)
    max_d, min_d, default, min_w, vs = F(max_distance_m), F(min_distance_m), F(default_distance_m), F(min_weight), F(voxel_size)
    if n == 0:
        out = np.zeros((0, nv), F), np.zeros((0, nv), np.uint8)
        return out + (0,) if return_sweeps else out
    with np.errstate(invalid="ignore"):
        # esdf_init_kernel: unobserved iff w < min_weight (a NaN weight is observed); |d| < min fixed; else sgn(d) * default
        unobserved = tw < min_w
        fixed = ~unobserved & (np.abs(td) < min_d)
        sgn = (td > 0).astype(F) - (td < 0).astype(F)
        init = np.where(fixed, td, sgn * default).astype(F)
    # esdf_relax_kernel stages unobserved voxels and missing blocks as NaN: never a source, never updated
    D = _grid(bi, vps, np.where(unobserved, F(np.nan), init).astype(F), F(np.nan))
    free = _grid(bi, vps, ~unobserved & ~fixed, False)[1:-1, 1:-1, 1:-1]
    steps = {1: vs, 2: F(np.sqrt(F(2.0))) * vs, 3: F(np.sqrt(F(3.0))) * vs}
    assert all(s.dtype == F for s in steps.values())
    Z, Y, X = (s - 2 for s in D.shape)
    sweeps = 0
    while True:
        C = D[1:-1, 1:-1, 1:-1]
        pos, neg = C > 0, C < 0
        mag = np.abs(C)
        best = mag.copy()
        with np.errstate(invalid="ignore"):
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        k = (dx != 0) + (dy != 0) + (dz != 0)
                        if k == 0:
                            continue
                        N = D[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
                        a = np.abs(N)
                        cand = a + steps[k]
                        ok = ((pos & (N > 0)) | (neg & (N < 0))) & (a < max_d) & (cand < best)
                        best = np.where(ok, cand, best)
            moved = free & (best < mag)
        if not moved.any():
            break
        sweeps += 1
        new = D.copy()
        new[1:-1, 1:-1, 1:-1] = np.where(moved, np.where(pos, best, -best), C)
        D = new
    ed = _rows(bi, vps, D)
    ed[unobserved] = F(0.0)
    eo = (~unobserved).astype(np.uint8)
    return (ed, eo, sweeps) if return_sweeps else (ed, eo)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
