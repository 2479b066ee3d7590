"""Device-free TSDF scenes for the ESDF tests (tests/test_esdf_cpu.py, tests/test_esdf_gpu.py, profiles/fuzz_esdf.py).

oracle/synth.make_submap marks a voxel observed only within 2 * trunc of the surface, so the ESDF front never runs more than about
six voxels there.  These scenes are CARVED, as an integrated layer is: weight > 0 and d = +-trunc through all the free space, so
the front runs max_distance_m / voxel_size voxels across several blocks.  Every scene is a Scene(vs, vps, bi, td, tw); SCENES maps
a name to (builder, configurations); scene(name) and reference(name, cfg) build each scene and each restatement once per process
(the arrays are read-only: copy before planting anything)."""
import collections
import functools

import numpy as np

from oracle import synth
from tests import esdf_ref

F = np.float32
Scene = collections.namedtuple("Scene", ["vs", "vps", "bi", "td", "tw"])
# (max_distance_m, min_distance_m, default_distance_m): voxblox's defaults
DEFAULT = (2.0, 0.2, 2.0)
INF = float("inf")


def voxel_index(bi, vps):
    """[n][vps^3][3] global integer voxel coordinates, x fastest"""
    i = np.arange(vps)
    lz, ly, lx = np.meshgrid(i, i, i, indexing="ij")
    local = np.stack([lx.ravel(), ly.ravel(), lz.ravel()], -1)
    return np.asarray(bi, np.int64)[:, None, :] * vps + local[None]


def _scene(vs, vps, bi, td, tw):
    bi = np.ascontiguousarray(bi, np.int32).reshape(-1, 3)
    td, tw = np.ascontiguousarray(td, F), np.ascontiguousarray(tw, F)
    assert td.shape == tw.shape == (len(bi), vps ** 3)
    return Scene(float(F(vs)), int(vps), bi, td, tw)


def carved_box(vps, vs, block_min, dims, seed, holes=0.05, shuffle=True):
    """sphere + ground in a box carved everywhere: d clipped to +-trunc (3 voxels), weight 10 apart from `holes` random
    weight-0 voxels; the block rows shuffled so that slot order is not spatial order"""
    rng = np.random.default_rng(seed)
    bi = synth.dense_block_index(block_min, dims)
    if shuffle:
        bi = bi[rng.permutation(len(bi))]
    lo, ext = np.array(block_min) * vps * vs, np.array(dims) * vps * vs
    centre = lo + rng.uniform(0.3, 0.7, 3) * ext
    sdf = synth.sphere_ground_sdf(tuple(centre), float(rng.uniform(0.15, 0.3) * ext.min()), float(lo[2] + rng.uniform(0.05, 0.2) * ext[2]))
    d = sdf(synth.voxel_centres(vs, vps, bi).reshape(-1, 3)).reshape(len(bi), vps ** 3)
    td = np.clip(d, -F(3 * vs), F(3 * vs)).astype(F)
    tw = np.where(rng.uniform(size=td.shape) < holes, 0, 10).astype(F)
    return _scene(vs, vps, bi, td, tw)


def point_sources(vps, vs, bi, sources, unobserved=()):
    """every voxel of the blocks `bi` carved (d = +trunc, weight 10) around small spheres at the centres of the blocks `sources`
    (radius (1 + k / 4) voxels for the k-th: two sources never look alike); the blocks `unobserved` have weight 0 throughout"""
    bi = np.asarray(bi, np.int64).reshape(-1, 3)
    p = synth.voxel_centres(vs, vps, bi).reshape(-1, 3)
    d = np.full(len(p), np.inf, F)
    for k, s in enumerate(sources):
        c = ((np.asarray(s, F) + F(0.5)) * F(vps) * F(vs)).astype(F)
        d = np.minimum(d, np.sqrt(((p - c) ** 2).sum(-1, dtype=F)).astype(F) - F((1 + 0.25 * k) * vs))
    td = np.clip(d, -F(3 * vs), F(3 * vs)).astype(F).reshape(len(bi), vps ** 3)
    tw = np.full(td.shape, 10, F)
    for u in unobserved:
        tw[(bi == np.asarray(u)).all(1)] = 0
    return _scene(vs, vps, bi, td, tw)


# the 12 block offsets that share only an edge and the 8 that share only a corner
EDGES = [d for d in np.ndindex(3, 3, 3) if sum(x != 1 for x in d) == 2]
EDGES = [tuple(int(x) - 1 for x in d) for d in EDGES]
CORNERS = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]


def two_blocks(vps, offset, base=(-1, 2, -3), vs=0.1):
    """a block with a source and one other block at `offset` from it: whatever reaches the second came through the halo"""
    a = np.array(base)
    return point_sources(vps, vs, [a + np.array(offset), a], [a])       # (the source's block in the second slot)


def lut_corners(vps, centre, base=(-2, -1, -3), vs=0.1):
    """blocks at the eight extreme corners of a 3 x 3 x 3 block box, every face and edge neighbour of each missing: with `centre`
    a ninth block in the middle holds the only source and feeds each corner through one diagonal halo voxel; without it every
    corner has a source of its own and nothing may pass from one to another (a block index that wraps in the table would)"""
    b = np.array(base)
    corners = [b + 2 * np.array(c) for c in np.ndindex(2, 2, 2)]
    if centre:
        return point_sources(vps, vs, corners[:4] + [b + 1] + corners[4:], [b + 1])
    return point_sources(vps, vs, corners, corners)


def unobserved_neighbour(vps, vs=0.1):
    """3 x 2 x 1 blocks, the source in (0,0,0), block (1,0,0) present but wholly unobserved: the front stops at it and reaches
    (2,0,0) the long way round through the second row"""
    bi = [(2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0)]
    return point_sources(vps, vs, bi, [(0, 0, 0)], unobserved=[(1, 0, 0)])


def corridor(n_blocks=40, vps=8, vs=0.1):
    """one carved row of blocks along x with the surface at the x = 0 end only; the slots run against the front's direction"""
    bi = np.array([(x, 0, 0) for x in range(n_blocks - 1, -1, -1)])
    ix = voxel_index(bi, vps)[..., 0]
    td = np.clip((ix.astype(F) + F(0.5)) * F(vs) - F(0.12), -F(3 * vs), F(3 * vs)).astype(F)
    return _scene(vs, vps, bi, td, np.full(td.shape, 10, F))


def labyrinth(vps, vs=0.1):
    """a carved 3 x 3 x 1-block slab with the surface at x = 0 and one-voxel walls of weight-0 voxels every vps / 2 voxels in x,
    open at alternating ends: the only way on is a serpentine, far longer than the straight line"""
    bi = synth.dense_block_index((-1, -2, 3), (3, 3, 1))[::-1]
    v = voxel_index(bi, vps)
    ix, iy = v[..., 0] + vps, v[..., 1] + 2 * vps                       # from 0 to 3 * vps - 1
    td = np.clip((ix.astype(F) + F(0.5)) * F(vs) - F(0.02), -F(3 * vs), F(3 * vs)).astype(F)
    half, n = vps // 2, 3 * vps
    wall = (ix % half == 0) & (ix > 0)
    lane = ix // half
    gap = np.where(lane % 2 == 1, iy >= n - half, iy < half)
    tw = np.where(wall & ~gap, 0, 10).astype(F)
    return _scene(vs, vps, bi, td, tw)


def thin_wall(vps, diagonal3, vs=0.1):
    """2 x 2 x 2 blocks around the origin cut by a one-voxel fixed band on the staircase x + y (+ z) == -1, which passes through
    the blocks' common edge (corner): negative on one side, positive on the other, the band's own voxels alternately +-0.02 so that
    both sides have sources.  Voxels of opposite sides are diagonal neighbours across the staircase, also across block borders."""
    bi = synth.dense_block_index((-1, -1, -1), (2, 2, 2))[[5, 2, 7, 0, 3, 6, 1, 4]]
    v = voxel_index(bi, vps)
    s = v[..., 0] + v[..., 1] + (v[..., 2] if diagonal3 else 0)
    band = np.where((v[..., 2] + v[..., 0]) % 2 == 0, F(0.02), F(-0.02))
    td = np.where(s == -1, band, np.where(s < -1, -F(3 * vs), F(3 * vs))).astype(F)
    return _scene(vs, vps, bi, td, np.full(td.shape, 10, F))


def plane_box(vps, axis, vs=0.1):
    """a fully carved 4 x 4 x 4-block box (3 blocks at vps 16) holding one plane normal to `axis` just off the middle: along
    the normal the ESDF is the last fixed value plus k steps, added one at a time in f32"""
    n = 4 if vps == 8 else 3
    bi = synth.dense_block_index((-2, -1, 0), (n, n, n))
    i = voxel_index(bi, vps)[..., axis] - (-2, -1, 0)[axis] * vps
    td = np.clip((i.astype(F) + F(0.5)) * F(vs) - F(n * vps * vs / 2 + 0.03), -F(3 * vs), F(3 * vs)).astype(F)
    return _scene(vs, vps, bi, td, np.full(td.shape, 10, F))


def arith_zeros(vps=8):
    """a carved box with +0.0 and -0.0 planted in the free space (min_distance_m = 0 leaves them outside the band)"""
    sc = carved_box(vps, 0.1, (-1, -1, -1), (2, 2, 2), 11)
    td = sc.td.copy()
    td[:, 5::17] = F(0.0)
    td[:, 9::23] = -F(0.0)
    return sc._replace(td=td)


def arith_nans(vps=8):
    """a carved box with NaN weights, NaN distances under a positive weight, and both at once"""
    sc = carved_box(vps, 0.1, (-1, -1, -1), (2, 2, 2), 12)
    td, tw = sc.td.copy(), sc.tw.copy()
    tw[:, 3::29] = np.nan
    td[:, 7::31] = np.nan
    tw[:, 7::62] = np.nan
    return sc._replace(td=td, tw=tw)


def room_scans(n=3):
    """n small LiDAR-like scans of a 4.2 x 3.3 x 2 m room from poses 0.3 m apart: [(T_G_C [7], points [k][3])]"""
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 192, endpoint=False) + (2 * np.pi / 192) / 3.0, np.linspace(-0.5, 0.5, 16) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    out = []
    for k in range(n):
        pos = np.array([0.1 + 0.3 * k, -0.05 - 0.2 * k, 0.02])
        lo, hi = np.array([-2.0, -1.5, -0.8]) - pos, np.array([2.2, 1.8, 1.2]) - pos
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
        out.append((np.array([1, 0, 0, 0, *pos], F), (d * t[:, None]).astype(F)))
    return out


# name -> (builder, [(max_distance_m, min_distance_m, default_distance_m), ...])
SCENES = {
    # carved boxes: 3 to 5 blocks a side, negative and positive block indices, the default configuration and one with default > max
    "box_vps8": (lambda: carved_box(8, 0.1, (-3, -2, -1), (5, 4, 3), 1), [DEFAULT, (1.6, 0.2, 2.0)]),
    "box_vps16": (lambda: carved_box(16, 0.1, (1, -4, 2), (3, 3, 3), 2), [DEFAULT, (1.6, 0.2, 2.0)]),
    "box_vps8_5cm": (lambda: carved_box(8, 0.05, (-2, 0, -4), (4, 3, 5), 3), [(2.0, 0.1, 2.0), (1.0, 0.1, 2.0)]),
    # (the uncapped configurations: max_distance_m / voxel_size fits no int)
    "corridor": (corridor, [DEFAULT, (INF, 0.2, INF), (1e10, 0.2, 1e10)]),
    "labyrinth_vps8": (lambda: labyrinth(8), [(30.0, 0.2, 30.0), (INF, 0.2, INF)]),
    "labyrinth_vps16": (lambda: labyrinth(16), [(30.0, 0.2, 30.0)]),
    "wall2_vps8": (lambda: thin_wall(8, False), [(2.0, 0.05, 2.0)]),
    "wall3_vps8": (lambda: thin_wall(8, True), [(2.0, 0.05, 2.0)]),
    "wall2_vps16": (lambda: thin_wall(16, False), [(2.0, 0.05, 2.0)]),
    "wall3_vps16": (lambda: thin_wall(16, True), [(2.0, 0.05, 2.0)]),
    "lut_corners_fed_vps8": (lambda: lut_corners(8, True), [DEFAULT]),
    "lut_corners_fed_vps16": (lambda: lut_corners(16, True), [(4.0, 0.2, 4.0)]),
    "lut_corners_alone_vps8": (lambda: lut_corners(8, False), [DEFAULT]),
    "lut_corners_alone_vps16": (lambda: lut_corners(16, False), [DEFAULT]),
    "unobserved_vps8": (lambda: unobserved_neighbour(8), [(4.0, 0.2, 4.0)]),
    "unobserved_vps16": (lambda: unobserved_neighbour(16), [(6.0, 0.2, 6.0)]),
    # arithmetic edges: min_distance_m = 0 (with planted zeros), NaNs, max_distance_m below one voxel step (default at and beyond
    # it), default_distance_m < max_distance_m
    "zeros": (arith_zeros, [(2.0, 0.0, 2.0), DEFAULT]),
    "nans": (arith_nans, [DEFAULT, (1.0, 0.25, 2.0)]),
    # (without holes, for the sampling grid: every voxel point has its eight interpolation corners)
    "box_whole": (lambda: carved_box(8, 0.1, (-1, -1, -1), (2, 2, 2), 13, holes=0.0), [(2.0, 0.1, 2.0), (1.0, 0.3, 1.5)]),
    "box_small": (lambda: carved_box(8, 0.1, (-1, -1, -1), (2, 2, 2), 13), [(0.05, 0.04, 0.05), (0.05, 0.04, 2.0), (0.25, 0.2, 2.0),
                                                                           (2.0, 0.2, 1.0), (2.0, 0.3, 0.7)]),
}
for _vps in (8, 16):
    for _k, _o in enumerate(EDGES + CORNERS):
        if _vps == 8 or _k % 5 == 0:                                    # vps 16: four of the twenty (edges 0, 5, 10, corner 3)
            SCENES["halo_vps%d_%+d%+d%+d" % ((_vps,) + _o)] = (functools.partial(two_blocks, _vps, _o), [DEFAULT if _vps == 8 else (3.0, 0.2, 3.0)])
    for _a in range(3):
        SCENES["plane_vps%d_%s" % (_vps, "xyz"[_a])] = (functools.partial(plane_box, _vps, _a), [DEFAULT, (1.0, 0.1, 1.5)])
# the scenes whose front travels far: the ones the queue's slack is measured on
DEEP = ("box_vps8", "box_vps16", "box_vps8_5cm", "labyrinth_vps8", "labyrinth_vps16", "unobserved_vps16", "lut_corners_fed_vps16")


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = SCENES[name][0]()
    for a in (sc.bi, sc.td, sc.tw):
        a.setflags(write=False)
    return sc


def configs(name):
    return SCENES[name][1]


def cases(names=None):
    """[(name, cfg)] over the registry"""
    return [(n, c) for n in (names or SCENES) for c in SCENES[n][1]]


@functools.lru_cache(maxsize=None)
def reference(name, cfg):
    """the restatement of scene `name` under cfg = (max, min, default): (esdf_distance, esdf_observed, Jacobi sweeps), read-only"""
    sc = scene(name)
    out = esdf_ref.esdf_from_tsdf(sc.vs, sc.vps, sc.bi, sc.td, sc.tw, cfg[0], cfg[1], cfg[2], return_sweeps=True)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def front_travel(sc, cfg, ed, eo):
    """-> (observed voxels outside the band, how many of them ended below the default, the farthest any of those ended from the
    band in voxels: (|d| - min_distance_m) / voxel_size)"""
    with np.errstate(invalid="ignore"):
        free = eo.astype(bool) & ~(np.abs(sc.td) < F(cfg[1]))
        moved = free & (np.abs(ed) < F(cfg[2]))
    far = float(((np.abs(ed[moved]) - F(cfg[1])) / F(sc.vs)).max()) if moved.any() else 0.0
    return int(free.sum()), int(moved.sum()), far
