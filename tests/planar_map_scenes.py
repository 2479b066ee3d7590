"""The synthetic scenes of tests/test_planar_map_gpu.py, kept apart so that tests/test_planar_map_cpu.py can check on the
CPU that none of them passes on nothing.  A scene is one block set with an ESDF (distance, observed) and a TSDF (distance,
weight) over it, and the planar-map configurations it is viewed with; every source kind views the same arrays.

A scene's `means` says what its configurations are meant to show, and census() measures it:
    "states"   some configuration has all three states present, in every source kind
    "zblocks"  some cell takes classified voxels from at least two z blocks
    "between"  some cell's distance is strictly between 0 and the limit
A scene that cannot show one of these by construction (a band that holds no row; a scene without obstacles) says so by
leaving it out, and the CPU test then asserts the opposite."""
import numpy as np

from tests import planar_map_ref as R

F = np.float32
SOURCES = ("esdf", "tsdf", "layer")


class Scene:
    def __init__(self, voxel_size, vps, bi, d, o, w, configs, means=("states", "zblocks", "between")):
        self.voxel_size, self.vps, self.bi, self.d, self.o, self.w = voxel_size, vps, np.ascontiguousarray(bi, np.int32), d, o, w
        self.configs, self.means = configs, set(means)


def reference(sc, cfg, source):
    """the restatement for one source kind: "esdf", "tsdf" (a finished submap's layers) or "layer" (a vgx_tsdf_layer)"""
    esdf = source == "esdf"
    return R.planar_map(sc.voxel_size, sc.vps, sc.bi, sc.d, sc.o if esdf else sc.w, esdf, **cfg)


def census(sc):
    """over the configurations: (some config shows all three states in every source, most z blocks feeding one cell,
    some cell strictly between 0 and the limit in every source)"""
    states, zblocks, between = False, 0, False
    for cfg in sc.configs:
        maps = [reference(sc, cfg, s) for s in SOURCES[:2]]
        states |= all(min(m.counts) > 0 for m in maps)
        zblocks = max(zblocks, min(int(m.z_blocks.max()) if m.z_blocks.size else 0 for m in maps))
        limit = F(cfg.get("max_distance_m", 2.0))
        between |= all(bool(((m.distance > 0) & (m.distance < limit)).any()) for m in maps)
    return states, zblocks, between


def _dense(lo, dims):
    xs, ys, zs = (np.arange(lo[a], lo[a] + dims[a]) for a in range(3))
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def _world(rng, voxel_size, vps, bi, dropout=0.1, hole=0.2):
    """Columns that mean something: the distance is a function of (x, y) plus a little noise along z, negative (occupied)
    in bands and positive (free) between them; whole columns unobserved where a 2D mask says so, so that unknown cells
    exist; single voxels dropped at random."""
    n = len(bi)
    lin = np.arange(vps ** 3)
    lx, ly = lin % vps, (lin // vps) % vps
    gx = bi[:, 0:1] * vps + lx[None]
    gy = bi[:, 1:2] * vps + ly[None]
    d = (0.6 * np.sin(0.37 * gx + 0.21 * gy) + 0.25 + 0.05 * rng.standard_normal((n, vps ** 3))).astype(F)
    known = (np.sin(0.9 * gx - 0.5 * gy) + np.sin(0.23 * gy)) > (2.0 * hole - 1.0) * 1.2
    drop = rng.random((n, vps ** 3)) < dropout
    o = (known & ~drop).astype(np.uint8)
    o[(o != 0) & (rng.random(o.shape) < 0.05)] = 200                             # observed is "!= 0", not "== 1"
    w = np.where(known & ~drop, rng.uniform(0.5, 5.0, (n, vps ** 3)), 0.0).astype(F)
    return d, o, w


def _holes(rng, bi, keep):
    return np.ascontiguousarray(bi[np.sort(rng.permutation(len(bi))[:keep])])


def _slot(sc_bi, block):
    return int(np.flatnonzero((sc_bi == np.asarray(block)).all(1))[0])


def _lin(vps, x, y, z):
    return x + vps * (y + vps * z)


def _band_scene(vps):
    """voxel_size 0.125: row centres are exact in f32, so a band edge can sit exactly on one"""
    vs, rng = 0.125, np.random.default_rng(10 + vps)
    bi = _holes(rng, _dense((-2, -1, -1), (4, 3, 3)), 30)
    d, o, w = _world(rng, vs, vps, bi)
    bs = vps * vs
    c = lambda bz, lz: float(bz * bs + (lz + 0.5) * vs)                            # noqa: E731 (exact)
    configs = [
        dict(z_min=c(0, 2) - 0.01, z_max=c(0, vps - 3) + 0.01),                  # cuts block 0 in the middle
        dict(z_min=c(0, 1), z_max=c(0, vps - 2)),                                # both edges exactly on row centres: included
        dict(z_min=c(-1, vps - 1), z_max=c(1, 0), max_distance_m=1.0),           # ... across three z blocks, edges on centres
        dict(z_min=c(0, 3), z_max=c(0, 3)),                                      # one row, z_min == z_max == its centre
        dict(z_min=c(0, 1) + 0.01, z_max=c(0, 2) - 0.01),                        # narrower than a voxel, between two rows
        dict(z_min=c(0, 1) + 0.01, z_max=c(0, 2) - 0.01, use_box=1, cell_min=(-3, 2), cell_dim=(9, 5)),
    ]
    return Scene(vs, vps, bi, d, o, w, configs)


def _narrow_scene():
    """nothing but bands that hold no row: the default box is empty, a given box is all unknown"""
    vs, vps, rng = 0.1, 8, np.random.default_rng(3)
    bi = _dense((0, 0, 0), (2, 2, 2))
    d, o, w = _world(rng, vs, vps, bi)
    configs = [dict(z_min=0.16, z_max=0.24), dict(z_min=0.16, z_max=0.24, use_box=1, cell_min=(3, 3), cell_dim=(7, 6)),
               dict(z_min=100.0, z_max=101.0), dict(z_min=0.16, z_max=0.24, use_box=1, cell_min=(0, 0), cell_dim=(5, 5),
                                                    unknown_is_obstacle=1)]
    return Scene(vs, vps, bi, d, o, w, configs, means=())


def _gap_scene():
    """a column of three z blocks with the middle one missing, at negative indices; voxel_size 0.1 (nothing exact)"""
    vs, vps, rng = 0.1, 16, np.random.default_rng(5)
    bi = _dense((-3, -2, -2), (2, 2, 3))
    bi = bi[~((bi[:, 0] == -3) & (bi[:, 1] == -2) & (bi[:, 2] == -1))]           # the middle block of one column
    bi = np.ascontiguousarray(bi[rng.permutation(len(bi))])
    d, o, w = _world(rng, vs, vps, bi)
    configs = [dict(z_min=-2.5, z_max=0.9), dict(z_min=-1.75, z_max=-1.4, min_free_voxels=3),
               dict(z_min=-3.0, z_max=2.0, occupied_distance=0.1, max_distance_m=0.75)]
    return Scene(vs, vps, bi, d, o, w, configs)


def _special_scene(vps):
    """planted NaN / +-inf / +-0 distances, NaN weights and weights at the threshold, in known columns of block (0, 0, 0)
    and (0, 0, 1); an occupied voxel just outside the band under free ones inside it"""
    vs, rng = 0.125, np.random.default_rng(20 + vps)
    bi = _holes(rng, _dense((-1, -1, 0), (3, 3, 2)), 16)
    if not ((bi == (0, 0, 0)).all(1).any() and (bi == (0, 0, 1)).all(1).any()):
        bi = np.concatenate([bi[~(((bi[:, :2] == 0).all(1)))], np.array([[0, 0, 0], [0, 0, 1]], np.int32)])
    d, o, w = _world(rng, vs, vps, bi, dropout=0.0, hole=0.1)
    lo, hi = _slot(bi, (0, 0, 0)), _slot(bi, (0, 0, 1))

    def column(x, y, values, weights=None, observed=None):
        """the column's voxels from row 1 of the lower block upwards (row 0 stays below the band)"""
        for k, v in enumerate(values):
            z = 1 + k
            b, lz = (lo, z) if z < vps else (hi, z - vps)
            at = _lin(vps, x, y, lz)
            d[b, at] = v
            w[b, at] = 2.0 if weights is None else weights[k]
            o[b, at] = 1 if observed is None else observed[k]

    inf, nan = F(np.inf), F(np.nan)
    rows = 2 * vps - 2                                                             # rows 1 .. 2 vps - 2 are in the band
    free = [F(0.5)] * rows
    column(0, 0, [inf, F(-0.0), F(0.0)] + free[3:])          # clearance -0.0: +0.0 is not < -0.0
    column(1, 0, [inf, F(0.0), F(-0.0)] + free[3:])          # clearance +0.0: the first of the tie stays
    column(2, 0, [nan] * rows)                               # nothing classifies: unknown, however observed
    column(3, 0, [nan, F(0.25), nan] + [nan] * (rows - 3))   # one free voxel among NaNs
    column(4, 0, [-inf] + free[1:])                          # occupied, clearance -inf
    column(5, 0, [inf] * rows)                               # free, clearance +inf
    column(6, 0, [F(-0.5)] * rows, weights=[nan] * rows, observed=[0] * rows)           # NaN weight: not observed
    column(7, 0, [F(-0.5)] * rows, weights=[R.MIN_WEIGHT] * rows, observed=[0] * rows)  # weight == min_weight: not observed
    column(0, 1, [F(-0.5)] * rows, weights=[np.nextafter(R.MIN_WEIGHT, F(1))] * rows)   # just above: observed
    column(1, 1, [F(-0.5)] * rows, weights=[F(0.5)] * rows)                             # observed unless min_weight = 0.5
    column(2, 1, free)                                       # free in the band ...
    for b, lz in ((lo, 0), (hi, vps - 1)):                   # ... over and under occupied voxels just outside it
        d[b, _lin(vps, 2, 1, lz)], w[b, _lin(vps, 2, 1, lz)], o[b, _lin(vps, 2, 1, lz)] = F(-0.5), F(2.0), 1
    column(3, 1, [F(0.5), F(-0.25), F(0.5), F(-0.125)] + free[4:])   # height: the HIGHEST occupied row, not the nearest
    bs = vps * vs
    band = dict(z_min=float(1.5 * vs), z_max=float(2 * bs - 1.5 * vs))           # rows 1 .. 2 vps - 2, edges on centres
    configs = [dict(band), dict(band, min_weight=0.5), dict(band, min_free_voxels=3),
               dict(band, occupied_distance=0.25), dict(band, unknown_is_obstacle=1, max_distance_m=0.5)]
    return Scene(vs, vps, bi, d, o, w, configs)


def _free_count_scene():
    """a three-row band with many voxels dropped: n_free runs over 0 .. 3, so min_free_voxels 1 and 3 differ"""
    vs, vps, rng = 0.1, 8, np.random.default_rng(7)
    bi = _holes(rng, _dense((-2, 0, 0), (4, 3, 2)), 20)
    d, o, w = _world(rng, vs, vps, bi, dropout=0.45)
    band = dict(z_min=0.62, z_max=0.9)                                           # rows 6, 7 of block 0 and row 0 of block 1
    return Scene(vs, vps, bi, d, o, w, [dict(band, min_free_voxels=1), dict(band, min_free_voxels=3),
                                       dict(band, min_free_voxels=4)])


def _box_scene(vps):
    vs, rng = 0.1, np.random.default_rng(30 + vps)
    nx, ny = (4, 3) if vps == 8 else (3, 2)                                      # (grids of at most 64 x 64 cells)
    bi = _holes(rng, _dense((-2, -1, 0), (nx, ny, 2)), 2 * nx * ny - 3)
    d, o, w = _world(rng, vs, vps, bi)
    band = dict(z_min=0.3, z_max=vps * vs + 0.3, max_distance_m=0.6)
    x0, y0, W, H = -2 * vps, -1 * vps, nx * vps, ny * vps
    configs = [
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(W - 8, H - 7)),          # cuts blocks on all four sides
        dict(band, use_box=1, cell_min=(x0 - 5, y0 - 3), cell_dim=(W + 9, H + 7)),          # larger than the layer
        dict(band, use_box=1, cell_min=(x0 + W + 3, y0), cell_dim=(11, 9)),                 # disjoint: all unknown
        dict(band, use_box=1, cell_min=(x0 + W + 3, y0), cell_dim=(11, 9), unknown_is_obstacle=1),
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(0, 7)),                  # cell_dim 0
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(0, 0)),
        dict(band, use_box=1, cell_min=(-1, -1), cell_dim=(1, 1)),                          # one cell
        dict(band),                                                                          # the default box, for comparison
    ]
    return Scene(vs, vps, bi, d, o, w, configs)


def _distance_scene(obstacles, configs, means):
    """48 x 40 cells (wider and taller than the 16 x 16 gather tile and the 32 x 8 tile of the distance passes), two z
    blocks, every voxel observed and free but the columns listed"""
    vs, vps = 0.125, 8
    bi = _dense((0, 0, 0), (6, 5, 2))
    n = len(bi)
    d = np.full((n, vps ** 3), 0.5, F)
    o = np.ones((n, vps ** 3), np.uint8)
    w = np.full((n, vps ** 3), 2.0, F)
    for x, y in obstacles:
        for bz in range(2):
            b = _slot(bi, (x // vps, y // vps, bz))
            for lz in range(vps):
                d[b, _lin(vps, x % vps, y % vps, lz)] = F(-0.1)
    band = dict(z_min=0.4, z_max=1.6)
    return Scene(vs, vps, bi, d, o, w, [dict(band, **c) for c in configs], means=means)


_LIMITS = [dict(max_distance_m=5.0),                    # R = 40: beyond the 32-cell tile, and the grid's 40 rows
           dict(max_distance_m=0.125),                  # R = 1
           dict(max_distance_m=0.1),                    # R = 1, the limit below one cell
           dict(max_distance_m=1.3)]                    # R = 11, not a multiple of the voxel size

SCENES = {
    "band_vps8": lambda: _band_scene(8),
    "band_vps16": lambda: _band_scene(16),
    "narrow": _narrow_scene,
    "gap_vps16": _gap_scene,
    "special_vps8": lambda: _special_scene(8),
    "special_vps16": lambda: _special_scene(16),
    "free_count": _free_count_scene,
    "box_vps8": lambda: _box_scene(8),
    "box_vps16": lambda: _box_scene(16),
    "corner": lambda: _distance_scene([(0, 0)], _LIMITS, ("zblocks", "between")),
    "ties": lambda: _distance_scene([(10, 20), (30, 20), (20, 10), (20, 30), (47, 39)], _LIMITS, ("zblocks", "between")),
    "outside_box": lambda: _distance_scene([(0, 0), (47, 39)], [dict(c, use_box=1, cell_min=(2, 2), cell_dim=(40, 36)) for c in _LIMITS],
                                           ("zblocks",)),
    "no_obstacle": lambda: _distance_scene([], _LIMITS + [dict(max_distance_m=5.0, unknown_is_obstacle=1)], ("zblocks",)),
}


def fuzz_draw(rng):
    """one draw of the fuzzer: (scene with ONE configuration, source kind) -- a random sparse layer with planted special
    values, a random band, box and limit"""
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.1, 0.125, 0.2, 0.05]))
    lo = rng.integers(-40, 40, 3)
    dims = (int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))) if vps == 8 else \
        (int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 4)))
    pool = _dense(lo, dims)
    bi = np.ascontiguousarray(pool[rng.permutation(len(pool))[:max(1, int(rng.integers(1, len(pool) + 1)))]])
    d, o, w = _world(rng, vs, vps, bi, dropout=float(rng.uniform(0.0, 0.6)), hole=float(rng.uniform(0.05, 0.5)))
    for value in (F(np.nan), F(np.inf), F(-np.inf), F(0.0), F(-0.0)):
        d[rng.random(d.shape) < 0.01] = value
    w[rng.random(w.shape) < 0.02] = R.MIN_WEIGHT
    w[rng.random(w.shape) < 0.01] = F(np.nan)
    bs = vps * vs
    z_lo = float(lo[2]) * bs + float(rng.uniform(-0.5, dims[2])) * bs
    cfg = dict(z_min=z_lo, z_max=z_lo + float(rng.choice([0.0, 0.3 * vs, 2.5 * vs, bs, 3 * bs])),
               occupied_distance=float(rng.choice([0.0, 0.1, -0.1])), min_free_voxels=int(rng.integers(1, 4)),
               unknown_is_obstacle=int(rng.integers(0, 2)), max_distance_m=float(rng.choice([0.5 * vs, vs, 3.3 * vs, 1.0, 40 * vs])))
    if rng.random() < 0.3:                                                       # an edge exactly on a row centre
        cfg["z_min"] = float(R.row_centres(vs, vps, [int(lo[2])])[0, int(rng.integers(0, vps))])
        cfg["z_max"] = max(cfg["z_max"], cfg["z_min"])
    if rng.random() < 0.5:
        cfg.update(use_box=1, cell_min=(int(lo[0]) * vps + int(rng.integers(-12, 20)), int(lo[1]) * vps + int(rng.integers(-12, 20))),
                   cell_dim=(int(rng.integers(0, 50)), int(rng.integers(0, 50))))
    return Scene(vs, vps, bi, d, o, w, [cfg], means=()), SOURCES[int(rng.integers(0, 3))]
