"""The scene of the hand-stated special-value tests of the three layer readers (tests/test_view_render_gpu.py,
tests/test_scan_registration_gpu.py, tests/test_scan_localization_gpu.py): a 2 x 2 x 2-block layer (vps 8, 0.1 m voxels,
blocks -1 .. 0 on every axis) of the linear field D = Z0 - z -- free space below the plane z = Z0, weight 1 everywhere -- and
ONE cube of 8 neighbouring voxels, CELL, into which a special value is planted.  The expectations in those tests come from
IEEE arithmetic and the header's comparisons ("all 8 weights > 0", "not (D > 0)", "|D| < max_abs_distance_m"), not from
the restatements.

CELL: the voxels x 1..2, y 2..3 of block 0 and z 6..7 of block -1, centres x 0.15 / 0.25, y 0.25 / 0.35, z -0.15 / -0.05.
Every position with x = 0.17, y = 0.27 and -0.15 < z < -0.05 interpolates over exactly these 8, at dl = (0.2, 0.2, > 0).
Neighbour 7 (x 2, y 3, z 7: the high one on every axis) is the only one whose coefficient in the trilinear form is
multiplied by dl0 dl1 dl2 alone, so a +-inf planted THERE reaches D as +-inf (any other neighbour's inf meets its own
negation in the coefficients: NaN).  The cube below (z 5..6) does not hold neighbour 7; the cube above (z 7 and z 0 of
block 0) does.

What IEEE gives for a weight w under `w > 0`: true for 1e-40 (a denormal is a positive number unless the device flushes it)
and +inf; false for NaN (every comparison with a NaN is false), -0.0 and 0.0 (equal to zero) and -1."""
import numpy as np

from oracle import synth

F = np.float32
VPS, VOXEL_SIZE, Z0 = 8, 0.1, -0.09
X, Y = 0.17, 0.27
Z_BELOW, Z_IN = -0.2, -0.1175            # a position in the cube below CELL (D = 0.11), one in CELL (D = 0.0275)
NEIGHBOUR_7 = ((0, 0, -1), (2, 3, 7))    # (block, voxel x y z)
CELL = [((0, 0, -1), (1 + ((k >> 2) & 1), 2 + ((k >> 1) & 1), 6 + (k & 1))) for k in range(8)]
WEIGHTS_OBSERVED = (1e-40, np.inf)
WEIGHTS_UNOBSERVED = (np.nan, -0.0, 0.0, -1.0)


def layer():
    """(block_index [8][3] i32, distance [8][512] f32, weight [8][512] f32), fresh arrays"""
    bi = synth.dense_block_index((-1, -1, -1), (2, 2, 2)).astype(np.int32)
    z = synth.voxel_centres(VOXEL_SIZE, VPS, bi)[..., 2]
    d = (F(Z0) - z).astype(F)
    return bi, d, np.ones_like(d)


def plant(bi, a, where, value):
    """a copy of the voxel array `a` with `value` at every (block, voxel) of `where`"""
    out = a.copy()
    for block, (x, y, z) in where:
        slot = int(np.flatnonzero((bi == np.array(block)).all(1))[0])
        out[slot, x + VPS * (y + VPS * z)] = F(value)
    return out
