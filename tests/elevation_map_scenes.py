"""The synthetic scenes of tests/test_elevation_map_gpu.py, kept apart so that tests/test_elevation_map_cpu.py can check on
the CPU that none of them passes on nothing.  A scene is one block set with an ESDF (distance, observed) and a TSDF
(distance, weight) over it, and the elevation-map configurations it is viewed with; every source kind views the same arrays.

A scene's `means` says what its configurations are meant to show, and census() measures it over the configurations:
    "states"    some configuration has all four states present, in every source kind
    "classes"   ... all three classes
    "multi"     some cell has two or more crossings
    "inside"    some chosen crossing has t strictly inside (0, 1)
    "straddle"  some chosen crossing has its solid voxel in the top row of a z block (the free one is in the block above)
    "between"   some cell's distance is strictly between 0 and the limit
A scene that cannot show one of these by construction says so by leaving it out, and the CPU test then asserts the
opposite."""
import numpy as np

from tests import elevation_map_ref as R

F = np.float32
SOURCES = ("esdf", "tsdf", "layer")
ALL = ("states", "classes", "multi", "inside", "straddle", "between")


class Scene:
    def __init__(self, voxel_size, vps, bi, d, o, w, configs, means=ALL):
        self.voxel_size, self.vps, self.bi, self.d, self.o, self.w = voxel_size, vps, np.ascontiguousarray(bi, np.int32), d, o, w
        self.configs, self.means = configs, set(means)


def reference(sc, cfg, source):
    """the restatement for one source kind: "esdf", "tsdf" (a finished submap's layers) or "layer" (a vgx_tsdf_layer)"""
    esdf = source == "esdf"
    return R.elevation_map(sc.voxel_size, sc.vps, sc.bi, sc.d, sc.o if esdf else sc.w, esdf, **cfg)


def census(sc):
    out = dict.fromkeys(ALL, False)
    for cfg in sc.configs:
        maps = [reference(sc, cfg, s) for s in SOURCES[:2]]
        limit = F(cfg.get("max_distance_m", 2.0))
        out["states"] |= all(min(m.state_counts) > 0 for m in maps)
        out["classes"] |= all(min(m.class_counts) > 0 for m in maps)
        out["multi"] |= all(bool((m.n_cross >= 2).any()) for m in maps)
        with np.errstate(invalid="ignore"):
            out["inside"] |= all(bool(((m.t > 0) & (m.t < 1)).any()) for m in maps)
        out["straddle"] |= all(bool(((m.state == 1) & (m.z_row % sc.vps == sc.vps - 1)).any()) for m in maps)
        out["between"] |= all(bool(((m.distance > 0) & (m.distance < limit)).any()) for m in maps)
    return out


def _dense(lo, dims):
    xs, ys, zs = (np.arange(lo[a], lo[a] + dims[a]) for a in range(3))
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def _coords(vps, bi):
    """global voxel indices gx, gy, gz [n][vps^3] (linear index x fastest)"""
    lin = np.arange(vps ** 3)
    return (bi[:, 0:1] * vps + (lin % vps)[None], bi[:, 1:2] * vps + ((lin // vps) % vps)[None],
            bi[:, 2:3] * vps + (lin // (vps * vps))[None])


def _terrain(vs, vps, bi, surf, seen=None, rng=None, noise=0.0):
    """d = (the voxel centre's z) - surf(gx, gy): free above the surface, solid below it.  `seen`: a mask over (gx, gy, gz);
    unobserved voxels get observed 0 / weight 0."""
    gx, gy, gz = _coords(vps, bi)
    d = ((gz + 0.5) * vs - surf(gx, gy)).astype(F)
    if rng is not None and noise:
        d = (d + noise * rng.standard_normal(d.shape)).astype(F)
    known = np.ones(d.shape, bool) if seen is None else seen(gx, gy, gz)
    o = known.astype(np.uint8)
    o[(o != 0) & ((gx + gy + gz) % 7 == 0)] = 200                                # observed is "!= 0", not "== 1"
    w = np.where(known, 2.0, 0.0).astype(F)
    return d, o, w


def _slab(zc, floor, lo, hi):
    """the distance in a column with a slab [lo, hi] over a floor: free above the slab, solid inside it, free under it down
    to half way to the floor (measured to the slab there), and the floor's own distance below that"""
    return np.select([zc > hi, zc >= lo, zc > 0.5 * (floor + lo)], [zc - hi, -np.minimum(zc - lo, hi - zc), lo - zc], zc - floor)


def _slot(bi, block):
    return int(np.flatnonzero((bi == np.asarray(block)).all(1))[0])


def _lin(vps, x, y, z):
    return x + vps * (y + vps * z)


def _set_column(sc_arrays, vps, bi, x, y, z_lo, values, weights=None, observed=None):
    """the voxels of global column (x, y) from global row z_lo upwards"""
    d, o, w = sc_arrays
    for k, v in enumerate(values):
        z = z_lo + k
        b = _slot(bi, (x // vps, y // vps, z // vps))
        at = _lin(vps, x % vps, y % vps, z % vps)
        d[b, at] = v
        w[b, at] = 2.0 if weights is None else weights[k]
        o[b, at] = 1 if observed is None else observed[k]


def _tilted_scene(vps):
    """a tilted plane through two (vps 8) or three (vps 16) z blocks at negative indices, with a patch never seen, a
    patch seen only above the surface (holes) and one seen only below it (blocked); the step windows 0, 1, 3 and 9"""
    vs = 0.125 if vps == 8 else 0.1
    nx, ny, nz = (6, 5, 2) if vps == 8 else (3, 3, 3)
    lo = (-4, -2, -1)
    bi = _dense(lo, (nx, ny, nz))
    bi = np.ascontiguousarray(bi[np.random.default_rng(vps).permutation(len(bi))])
    z0 = lo[2] * vps * vs
    top = nz * vps * vs
    sx, sy, base = (0.2, 0.08, 0.15) if vps == 8 else (0.31, 0.12, 0.35)                                  # (the plane stays inside the blocks)
    surf = lambda gx, gy: z0 + base * top + sx * vs * (gx - lo[0] * vps) + sy * vs * (gy - lo[1] * vps)   # noqa: E731

    def seen(gx, gy, gz):
        ux, uy = gx - lo[0] * vps, gy - lo[1] * vps
        above = (gz + 0.5) * vs > surf(gx, gy)
        never = (ux >= 5) & (ux < 9) & (uy >= 20) & (uy < 26)
        only_above = (ux >= 20) & (ux < 24) & (uy >= 3) & (uy < 8)
        only_below = (ux >= 30) & (ux < 33) & (uy >= 10) & (uy < 15)
        return ~never & ~(only_above & ~above) & ~(only_below & above)

    d, o, w = _terrain(vs, vps, bi, surf, seen)
    band = dict(z_min=z0 - 1.0, z_max=z0 + top + 1.0)
    W, H = nx * vps, ny * vps
    configs = [dict(band), dict(band, step_radius_cells=0, max_slope=0.5 * sx), dict(band, step_radius_cells=3, max_step_m=6.5 * sx * vs, min_support=30),
               dict(band, step_radius_cells=9, max_step_m=20 * sx * vs, max_slope=1.2 * sx, hole_is_obstacle=0, unknown_is_obstacle=1),
               dict(band, step_radius_cells=9, use_box=1, cell_min=(lo[0] * vps + 3, lo[1] * vps + 5), cell_dim=(W - 8, H - 7)),
               dict(band, max_slope=1.1 * sx, max_step_m=10.0, max_distance_m=0.7)]
    return Scene(vs, vps, bi, d, o, w, configs, means=("states", "classes", "inside", "straddle", "between"))


def _gap_scene():
    """three z blocks with the surface inside the middle one; in one block column the middle block is missing, exactly
    between the free voxels of the top block and the solid ones of the bottom block, so no crossing results there"""
    vs, vps = 0.1, 8
    bi = _dense((-2, -1, -2), (3, 2, 3))
    bi = bi[~((bi[:, 0] == -1) & (bi[:, 1] == -1) & (bi[:, 2] == -1))]
    bi = np.ascontiguousarray(bi[np.random.default_rng(4).permutation(len(bi))])
    d, o, w = _terrain(vs, vps, bi, lambda gx, gy: -1.0 * vps * vs + 0.33 + 0.01 * gx)        # inside the middle block
    band = dict(z_min=-2.0, z_max=1.0)
    return Scene(vs, vps, bi, d, o, w, [dict(band), dict(band, pick=1), dict(band, unknown_is_obstacle=1, max_distance_m=0.55)],
                 means=("inside", "between"))


def _table_scene(vps):
    """a floor with a table over part of it: two crossings under the table, pick 0 against 1, and the lower crossing's
    headroom limited by the table"""
    vs = 0.125 if vps == 8 else 0.1
    nx, ny = (5, 4) if vps == 8 else (3, 2)
    bi = _dense((-1, -3, 0), (nx, ny, 3 if vps == 8 else 2))
    gx, gy, gz = _coords(vps, bi)
    zc = (gz + 0.5) * vs
    floor = 0.31 + 0.004 * (gx + gy)
    ux, uy = gx + vps, gy + 3 * vps
    table = (ux >= 6) & (ux < 22) & (uy >= 4) & (uy < 17)
    k_lo, k_hi = (3.2, 5.4) if vps == 8 else (10.5, 14.5)                        # the table's top lies about a z block boundary
    d = np.where(table, _slab(zc, floor, floor + k_lo * vs, floor + k_hi * vs), zc - floor).astype(F)
    o = np.ones(d.shape, np.uint8)
    w = np.full(d.shape, 2.0, F)
    band = dict(z_min=0.0, z_max=float(3 * vps * vs))
    room = int(k_lo)                                                             # free voxels under the table, at most
    configs = [dict(band), dict(band, pick=1), dict(band, pick=1, min_headroom_voxels=room + 2, max_distance_m=0.8),
               dict(band, pick=1, min_headroom_voxels=room - 1), dict(band, pick=0, step_radius_cells=3, max_step_m=0.5),
               dict(band, z_max=float(floor.min() + 4 * vs), pick=0)]                                  # the band ends under the table
    return Scene(vs, vps, bi, d, o, w, configs, means=("multi", "inside", "straddle", "between"))


def _special_scene(vps):
    """a flat floor with planted NaN / +-inf / +-0 distances, NaN weights and weights at the threshold in known columns of
    blocks (0, 0, 0) and (0, 0, 1); the floor's crossing is between global rows 3 (solid) and 4 (free)"""
    vs = 0.125
    bi = _dense((-1, -1, 0), (3, 3, 2))
    bi = np.ascontiguousarray(bi[np.random.default_rng(20 + vps).permutation(len(bi))])
    d, o, w = _terrain(vs, vps, bi, lambda gx, gy: 4 * vs + 0.0 * gx)           # d = (row - 3.5) vs: t = 0.5 everywhere, exactly
    inf, nan = F(np.inf), F(np.nan)
    a = (d, o, w)
    col = lambda x, y, values, **kw: _set_column(a, vps, bi, x, y, 2, values, **kw)   # noqa: E731  rows 2, 3, 4, 5, ...
    s, f = F(-0.3), F(0.2)
    col(0, 0, [s, -inf, f, f])                       # d_l = -inf: inf / inf, t = 0.5
    col(1, 0, [s, s, inf, f])                        # d_u = +inf: t = 0
    col(2, 0, [s, -inf, inf, f])                     # both: t = 0.5
    col(3, 0, [s, F(-0.0), f, f])                    # d_l = -0: solid, t = 0
    col(4, 0, [s, F(0.0), f, f])                     # d_l = +0: solid (not > 0), t = 0
    col(5, 0, [s, s, nan, f])                        # a NaN between: the run is reset, no crossing there -> blocked below, ...
    col(6, 0, [s, nan, f, f])                        # ... and a NaN solid side: no crossing at all in these rows
    col(7, 0, [s, s, f, f], weights=[2.0, 2.0, nan, 2.0], observed=[1, 1, 0, 1])              # NaN weight on the free voxel
    col(0, 1, [s, s, f, f], weights=[2.0, R.MIN_WEIGHT, 2.0, 2.0], observed=[1, 0, 1, 1])     # weight == min_weight: unobserved
    col(1, 1, [s, s, f, f], weights=[2.0, np.nextafter(R.MIN_WEIGHT, F(1)), 2.0, 2.0])       # just above: observed
    col(2, 1, [s, s, f, f], weights=[0.5] * 4)                                                # observed unless min_weight = 0.5
    col(3, 1, [s, F(-1e-30), F(1e-30), f])           # tiny operands: t = 0.5 by division, not by the fallback
    col(4, 1, [s, F(-3e38), F(3e38), f])             # d_u - d_l overflows to inf: t = 0
    col(5, 1, [f, s, f, s, f, s, f])                 # four crossings within seven rows
    band = dict(z_min=0.0, z_max=float(2 * vps * vs))
    configs = [dict(band), dict(band, pick=1), dict(band, min_weight=0.5), dict(band, unknown_is_obstacle=1, max_distance_m=0.5),
               dict(band, max_step_m=0.01, step_radius_cells=3)]
    return Scene(vs, vps, bi, d, o, w, configs, means=("multi", "inside", "between") + (("straddle",) if vps == 8 else ()))


def _band_scene():
    """the same flat floor (crossing between rows 3 and 4 of block 0, voxel_size 0.125: centres exact) under bands that keep
    it, cut its upper voxel, hold one row, and end exactly on the two centres"""
    vs, vps = 0.125, 8
    bi = _dense((0, 0, 0), (2, 2, 2))
    d, o, w = _terrain(vs, vps, bi, lambda gx, gy: 4 * vs + 0.02 * np.sin(gx + 2 * gy))
    c = lambda row: float((row + 0.5) * vs)                                      # noqa: E731 (exact)
    configs = [dict(z_min=c(3), z_max=c(4)),                                     # edges exactly on the two centres: a surface
               dict(z_min=c(3), z_max=c(4) - 0.01),                              # cuts the upper voxel: blocked
               dict(z_min=c(3) + 0.01, z_max=c(9)),                              # cuts the solid voxel: holes
               dict(z_min=c(3), z_max=c(3)), dict(z_min=c(4), z_max=c(4)),       # one row: no crossing can exist
               dict(z_min=c(1), z_max=c(12), max_distance_m=0.3),
               dict(z_min=5.0, z_max=6.0),                                       # no row: W = H = 0
               dict(z_min=5.0, z_max=6.0, use_box=1, cell_min=(3, 3), cell_dim=(7, 6), unknown_is_obstacle=1)]
    return Scene(vs, vps, bi, d, o, w, configs, means=("inside",))


def _sparse_scene():
    """surface cells planted one by one on an otherwise unseen grid (48 x 40 cells, vps 8): alone, in pairs, in row and
    column ends, in an L and in a plus: no, one and two valid neighbours on each axis, with heights that make a slope"""
    vs, vps = 0.1, 8
    bi = _dense((0, -5, 0), (6, 5, 1))
    gx, gy, gz = _coords(vps, bi)
    uy = gy + 5 * vps
    cells = set()
    for x, y in ((3, 3), (10, 3), (11, 3), (20, 3), (20, 4), (30, 3), (31, 3), (30, 4), (40, 10), (41, 10), (42, 10), (41, 9), (41, 11),
                 (0, 0), (1, 0), (0, 1), (47, 39), (46, 39), (47, 38), (15, 20), (16, 20), (17, 20), (31, 16), (32, 16), (31, 15), (31, 17),
                 (16, 8), (15, 8), (16, 7), (36, 24), (36, 25), (36, 26)):
        cells.add((x, y))
    mask = np.zeros(gx.shape, bool)
    for x, y in cells:
        mask |= (gx == x) & (uy == y)
    for x in range(5, 30):                                                      # a strip three cells wide: every neighbour count
        for y in range(28, 31):
            mask |= (gx == x) & (uy == y)
    d, o, w = _terrain(vs, vps, bi, lambda gx, gy: 0.33 + 0.07 * ((gx * 5 + gy * 3) % 4), lambda gx, gy, gz: mask)
    band = dict(z_min=0.0, z_max=0.8)
    configs = [dict(band, max_slope=5.0, max_step_m=1.0), dict(band, max_slope=1.0), dict(band, min_support=3, max_slope=5.0, max_step_m=1.0),
               dict(band, step_radius_cells=3, min_support=8, max_slope=5.0, max_step_m=0.1, max_distance_m=0.45),
               dict(band, use_box=1, cell_min=(10, -37), cell_dim=(22, 30), max_slope=5.0, max_step_m=1.0)]
    return Scene(vs, vps, bi, d, o, w, configs, means=("classes", "inside", "between"))


def _class_order_scene():
    """stairs under a low ceiling strip and next to an unseen strip: cells where two class branches disagree, so that the
    stated order decides -- low headroom with an undefined slope, an undefined slope with a large step, a large step with
    too little support"""
    vs, vps = 0.125, 8
    bi = _dense((-3, 0, 0), (6, 5, 2))
    gx, gy, gz = _coords(vps, bi)
    ux = gx + 3 * vps
    zc = (gz + 0.5) * vs
    floor = 0.3 + 0.375 * (ux // 12) + 0.003 * gy                                # stairs along x, a tread every 12 cells
    ceiling = (gy >= 30) & (gy < 36)                                             # a slab two voxels above the floor there
    d = np.where(ceiling, _slab(zc, floor, floor + 2.3 * vs, floor + 4.4 * vs), zc - floor).astype(F)
    known = ~((ux >= 17) & (ux < 19)) & ~(((gy == 12) | (gy == 13) | (gy == 32)) & (ux % 2 == 0))   # an unseen strip, and combs of unseen cells
    o = known.astype(np.uint8)
    w = np.where(known, 2.0, 0.0).astype(F)
    band = dict(z_min=0.0, z_max=2.0)
    configs = [dict(band, min_headroom_voxels=3), dict(band, min_headroom_voxels=3, pick=1, step_radius_cells=3, max_step_m=0.3),
               dict(band, min_headroom_voxels=3, pick=1, min_support=9), dict(band, pick=1, max_slope=0.0, max_step_m=0.0),
               dict(band, pick=1, max_slope=float("inf"), max_step_m=float("inf"), unknown_is_obstacle=1, max_distance_m=1.3)]
    return Scene(vs, vps, bi, d, o, w, configs, means=("classes", "multi", "inside", "straddle", "between"))


def _box_scene(vps):
    vs = 0.1
    nx, ny = (4, 3) if vps == 8 else (3, 2)
    rng = np.random.default_rng(30 + vps)
    pool = _dense((-2, -1, 0), (nx, ny, 2))
    bi = np.ascontiguousarray(pool[np.sort(rng.permutation(len(pool))[:len(pool) - 3])])
    d, o, w = _terrain(vs, vps, bi, lambda gx, gy: vps * vs + 0.15 * np.sin(0.3 * gx + 0.2 * gy), rng=rng, noise=0.01)   # about the z block boundary
    band = dict(z_min=0.0, z_max=2 * vps * vs, max_distance_m=0.6, step_radius_cells=3)
    x0, y0, W, H = -2 * vps, -1 * vps, nx * vps, ny * vps
    configs = [
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(W - 8, H - 7)),          # cuts blocks on all four sides
        dict(band, use_box=1, cell_min=(x0 - 5, y0 - 3), cell_dim=(W + 9, H + 7)),          # larger than the layer
        dict(band, use_box=1, cell_min=(x0 + W + 3, y0), cell_dim=(11, 9)),                 # disjoint: all unknown
        dict(band, use_box=1, cell_min=(x0 + W + 3, y0), cell_dim=(11, 9), unknown_is_obstacle=1),
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(0, 7)),                  # cell_dim 0
        dict(band, use_box=1, cell_min=(x0 + 3, y0 + 5), cell_dim=(0, 0)),
        dict(band, use_box=1, cell_min=(-1, -1), cell_dim=(1, 1)),                          # one cell
        dict(band, use_box=1, cell_min=(x0 + 2, y0 + 1), cell_dim=(W - 3, 1), step_radius_cells=9),   # one row of cells
        dict(band),                                                                          # the default box, for comparison
    ]
    return Scene(vs, vps, bi, d, o, w, configs, means=("states", "classes", "inside", "straddle", "between"))


SCENES = {
    "tilted_vps8": lambda: _tilted_scene(8),
    "tilted_vps16": lambda: _tilted_scene(16),
    "gap": _gap_scene,
    "table_vps8": lambda: _table_scene(8),
    "table_vps16": lambda: _table_scene(16),
    "special_vps8": lambda: _special_scene(8),
    "special_vps16": lambda: _special_scene(16),
    "band": _band_scene,
    "sparse": _sparse_scene,
    "class_order": _class_order_scene,
    "box_vps8": lambda: _box_scene(8),
    "box_vps16": lambda: _box_scene(16),
}


def fuzz_draw(rng):
    """one draw of the fuzzer: (scene with ONE configuration, source kind) -- a random sparse layer holding a wavy surface
    under a wavy ceiling, dropped voxels and planted special values, a random band, box, window and limits"""
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.1, 0.125, 0.2, 0.05]))
    lo = rng.integers(-40, 40, 3)
    dims = (int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))) if vps == 8 else \
        (int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 4)))
    pool = _dense(lo, dims)
    bi = np.ascontiguousarray(pool[rng.permutation(len(pool))[:max(1, int(rng.integers(1, len(pool) + 1)))]])
    bs = vps * vs
    z0, zt = float(lo[2]) * bs, dims[2] * bs
    a, b, ph = rng.uniform(0.02, 0.2, 2), rng.uniform(0.05, 0.6, 2), rng.uniform(0, 6, 2)
    base, amp, gap = rng.uniform(0.2, 0.6), rng.uniform(0.0, 0.12), rng.uniform(0.1, 0.5)
    gx, gy, gz = _coords(vps, bi)
    zc = (gz + 0.5) * vs
    floor = z0 + zt * (base + amp * np.sin(a[0] * gx + ph[0]) * np.sin(a[1] * gy + ph[1]))
    slab_lo = floor + zt * gap
    slab_hi = slab_lo + 1.7 * vs
    roofed = np.sin(b[0] * gx + b[1] * gy + ph[0]) > 0.3
    d = np.where(roofed, _slab(zc, floor, slab_lo, slab_hi), zc - floor)
    d = (d + 0.02 * vs * rng.standard_normal(d.shape)).astype(F)
    known = (np.sin(0.9 * gx - 0.5 * gy) + np.sin(0.23 * gy)) > -1.2 * (1.0 - 2.0 * rng.uniform(0.05, 0.4))
    known &= rng.random(d.shape) >= rng.uniform(0.0, 0.15)
    o = known.astype(np.uint8)
    w = np.where(known, rng.uniform(0.5, 5.0, d.shape), 0.0).astype(F)
    for value in (F(np.nan), F(np.inf), F(-np.inf), F(0.0), F(-0.0)):
        d[rng.random(d.shape) < 0.005] = value
    w[rng.random(w.shape) < 0.01] = R.MIN_WEIGHT
    w[rng.random(w.shape) < 0.005] = F(np.nan)
    z_lo = z0 + float(rng.uniform(-0.3, 0.3)) * bs
    cfg = dict(z_min=z_lo, z_max=z_lo + float(rng.choice([0.0, 2.5 * vs, bs, 3 * bs, 4 * bs, 4 * bs])), min_free_voxels=int(rng.integers(1, 4)),
               pick=int(rng.integers(0, 2)), step_radius_cells=int(rng.choice([0, 1, 2, 3, 5, 9, 17, 64])), min_support=int(rng.choice([1, 2, 5, 20])),
               max_slope=float(rng.choice([0.0, 0.5, 1.0, 3.0])), max_step_m=float(rng.choice([0.0, 2 * vs, 5 * vs, 1.0])),
               min_headroom_voxels=int(rng.choice([1, 2, 4])), hole_is_obstacle=int(rng.integers(0, 2)),
               unknown_is_obstacle=int(rng.integers(0, 2)), max_distance_m=float(rng.choice([0.5 * vs, vs, 3.3 * vs, 1.0, 40 * vs])))
    if rng.random() < 0.3:                                                       # an edge exactly on a row centre
        cfg["z_min"] = float(R.row_centres(vs, vps, [int(lo[2])])[0, int(rng.integers(0, vps))])
        cfg["z_max"] = max(cfg["z_max"], cfg["z_min"])
    if rng.random() < 0.5:
        cfg.update(use_box=1, cell_min=(int(lo[0]) * vps + int(rng.integers(-12, 20)), int(lo[1]) * vps + int(rng.integers(-12, 20))),
                   cell_dim=(int(rng.integers(0, 50)), int(rng.integers(0, 50))))
    return Scene(vs, vps, bi, d, o, w, [cfg], means=()), SOURCES[int(rng.integers(0, 3))]
