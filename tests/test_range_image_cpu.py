"""LiDAR range images without a device: the angle rule's error against f64 atan2 and its host form against the numpy
restatement (tests/range_image_ref.py) bit for bit, the pixel rule on hand-worked directions, hand-worked voxels on a beam,
vgx_tsdf_range_image_box (host only) against the restatement's box and that box against every voxel the rules update,
the new symbols and their refusals, and that the scenes of tests/test_range_image_gpu.py reach every branch of the rules.
At sensor sizes (S.SENSOR_MODELS, up to 4096 x 256): the host pixel rule against the restatement on random directions and on
the rule's own row and column boundaries, every pixel-centre ray back into its own pixel, the box against every voxel the
rules update, and that those scenes pass on something."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import range_image_ref as R
from tests import range_image_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ["vgx_atan2_rule", "vgx_range_image_check", "vgx_range_image_pixel", "vgx_range_image_create", "vgx_range_image_destroy",
       "vgx_range_image_build", "vgx_range_image_build_device", "vgx_range_image_stats", "vgx_range_image_download",
       "vgx_tsdf_integrate_range_image", "vgx_tsdf_range_image_box"]
BAR = 2 * np.pi / 4096 / 64            # 1 / 64 of the finest pixel pitch vgx_range_image_check accepts: 2.4e-5 rad


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


def _directions():
    """(y, x) f32: 4e6 directions on the circle, radii over 20 octaves, the axes, the octant seams and their f32 neighbours"""
    rng = np.random.default_rng(7)
    th = np.concatenate([np.linspace(-np.pi, np.pi, 3_000_001), rng.uniform(-np.pi, np.pi, 1_000_000)])
    rad = np.concatenate([np.ones(3_000_001), np.exp2(rng.uniform(-10, 10, 1_000_000))])
    y, x = (rad * np.sin(th)).astype(F), (rad * np.cos(th)).astype(F)
    seams = np.arange(-4, 5) * np.pi / 4
    sy, sx = np.sin(seams).astype(F), np.cos(seams).astype(F)
    near_y = np.concatenate([sy, np.nextafter(sy, F(2)), np.nextafter(sy, F(-2)), sy, sy])
    near_x = np.concatenate([sx, sx, sx, np.nextafter(sx, F(2)), np.nextafter(sx, F(-2))])
    axes_y = np.array([0, 0, 1, -1, 0.0, -0.0, 1e-30, -1e-30, 3e38, 1e-38], F)
    axes_x = np.array([1, -1, 0, 0, 1e-38, -1.0, -1, -1, 3e38, 1e-38], F)
    return np.concatenate([y, near_y, axes_y]), np.concatenate([x, near_x, axes_x])


def test_the_angle_rule_against_f64_atan2(capi):
    y, x = _directions()
    assert len(y) >= 4_000_000
    got = R.atan2_rule(y, x).astype(np.float64)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err = np.abs(got - want)
    err = np.minimum(err, 2 * np.pi - err)                 # (-pi and pi are one direction)
    worst = float(err.max())
    print(f"largest error of the angle rule: {worst:.3e} rad over {len(y)} directions (bar {BAR:.3e})")
    assert worst <= R.MAX_ERROR <= BAR
    assert np.abs(got).max() <= float(R.PI)
    assert R.atan2_rule(F(0), F(0)) == 0 and R.atan2_rule(F(-0.0), F(0)) == 0
    # the axes: exact multiples of the stated constants
    assert R.atan2_rule(F(0), F(1)) == 0 and R.atan2_rule(F(1), F(0)) == R.PI_2 and R.atan2_rule(F(-1), F(0)) == -R.PI_2
    assert R.atan2_rule(F(0), F(-1)) == R.PI and R.atan2_rule(F(-1e-30), F(-1)) == -R.PI
    # the header's constants are the restatement's, and the host form of the kernels' rule gives the same bits
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    for name, value in [(f"C{k}", c) for k, c in enumerate(R.C)] + [("PI_2", R.PI_2), ("PI", R.PI)]:
        text = re.search(rf"#define VGX_ATAN2_{name} (\S+)f\n", header).group(1)
        assert F(float.fromhex(text)) == value and float(F(float.fromhex(text))) == float.fromhex(text), name
    assert F(float(re.search(r"#define VGX_ATAN2_RULE_MAX_ERROR (\S+)f\n", header).group(1))) == F(R.MAX_ERROR)
    pick = np.concatenate([np.arange(0, len(y), 41), np.arange(len(y) - 60, len(y))])
    assert np.array_equal(capi.atan2_rule(y[pick], x[pick]).view(np.uint32), R.atan2_rule(y[pick], x[pick]).view(np.uint32))


def test_the_pixel_rule_on_hand_worked_directions(capi):
    """64 columns of 2 pi / 64, 9 rows of 0.1 rad from -0.4 (row 0) to 0.4 (row 8)"""
    ccw = R.Model(64, 9, 0.0, 0, -0.4, 0.4)            # column 0 looks along +x, columns advance towards +y
    cw = R.Model(64, 9, 0.0, 1, -0.4, 0.4)             # ... towards -y
    back = R.Model(64, 9, float(R.PI), 1, 0.4, -0.4)   # column 0 looks along -x, clockwise, the top row first
    t = np.tan(0.1 * np.arange(-5, 6))                  # z of unit-rho directions at elevations -0.5 .. 0.5
    cases = [
        # the axes
        (ccw, (1, 0, 0), (0, 4)), (ccw, (0, 1, 0), (16, 4)), (ccw, (-1, 0, 0), (32, 4)), (ccw, (0, -1, 0), (48, 4)),
        (cw, (1, 0, 0), (0, 4)), (cw, (0, 1, 0), (48, 4)), (cw, (-1, 0, 0), (32, 4)), (cw, (0, -1, 0), (16, 4)),
        # the +-pi seam, both column directions: just above and just below the -x axis
        (ccw, (-1, 1e-6, 0), (32, 4)), (ccw, (-1, -1e-6, 0), (32, 4)), (cw, (-1, 1e-6, 0), (32, 4)), (cw, (-1, -1e-6, 0), (32, 4)),
        (back, (-1, 1e-6, 0), (0, 4)), (back, (-1, -1e-6, 0), (0, 4)), (back, (-1, 0, 0), (0, 4)), (back, (1, 0, 0), (32, 4)),
        # half a column either side of column 0's edge (pitch 0.098: the edge is at 0.049 rad)
        (ccw, (1, np.tan(0.048), 0), (0, 4)), (ccw, (1, np.tan(0.050), 0), (1, 4)),
        (ccw, (1, -np.tan(0.048), 0), (0, 4)), (ccw, (1, -np.tan(0.050), 0), (63, 4)),
        (back, (-1, np.tan(0.050), 0), (1, 4)), (back, (-1, -np.tan(0.050), 0), (63, 4)),
        # the z axis: rho = 0, az = 0, el = +-pi/2: outside the rows, the column is column 0's
        (ccw, (0, 0, 1), (0, -1)), (ccw, (0, 0, -1), (0, -1)),
        # the row edges: the rows end half a pitch beyond their first and last centres, at +-0.45
        (ccw, (1, 0, np.tan(0.449)), (0, 8)), (ccw, (1, 0, np.tan(0.451)), (0, -1)),
        (ccw, (1, 0, -np.tan(0.449)), (0, 0)), (ccw, (1, 0, -np.tan(0.451)), (0, -1)),
        (back, (1, 0, np.tan(0.449)), (32, 0)), (back, (1, 0, -np.tan(0.449)), (32, 8)), (back, (1, 0, np.tan(0.451)), (32, -1)),
        (ccw, (1, 0, t[6]), (0, 5)), (ccw, (1, 0, t[1]), (0, 0)), (ccw, (3, 0, 3 * t[9]), (0, 8)),
    ]
    for m, d, (u, v) in cases:
        ui, vi, ok = R.pixel(m, *[F(c) for c in d])
        assert (int(ui), int(vi), bool(ok)) == (u, v, v >= 0), (d, int(ui), int(vi))
        assert capi.range_image_pixel(m.capi(capi), *d) == (capi.OK, u, v), d
    assert capi.range_image_pixel(ccw.capi(capi), 0, 0, 0)[0] == capi.ERR_INVALID
    assert capi.range_image_pixel(ccw.capi(capi), float("inf"), 0, 0)[0] == capi.ERR_INVALID
    assert capi.range_image_pixel(None, 1, 0, 0)[0] == capi.ERR_INVALID
    # a random cloud: the host form of the kernels' rule and the restatement agree pixel for pixel
    rng = np.random.default_rng(2)
    p = (rng.normal(size=(3000, 3)) * np.exp2(rng.uniform(-6, 6, (3000, 1)))).astype(F)
    for m in (ccw, back, S.MODELS["128x16"]):
        ui, vi, ok = R.pixel(m, p[:, 0], p[:, 1], p[:, 2])
        got = np.array([capi.range_image_pixel(m.capi(capi), *q)[1:] for q in p.tolist()])
        assert np.array_equal(got[:, 0], ui) and np.array_equal(got[:, 1], vi) and ok.sum() > 100 and (~ok).sum() > 100


def test_hand_worked_voxels_on_a_beam_in_front_of_a_wall():
    """One return at (1, 0, 0) -- a wall at 1 m on the beam of pixel (0, 4) --, identity orientation, voxel 0.1 m, 8 voxels a
    side, truncation 0.3 m.  The sensor sits at (0, 0.05, 0.05): on the axis of the voxel row (vx, 0, 0), whose centres
    ((vx + 0.5) 0.1, 0.05, 0.05) are then on the beam: y = z = 0, r_v = x, sdf = 1 - x, weight 1 / 1^2 = 1."""
    m = R.Model(64, 9, 0.0, 0, -0.4, 0.4)
    red = 0xff0000ff
    img = R.build(m, np.array([[1, 0, 0]], F), np.array([red], np.uint32))
    assert img.range[4, 0] == 1 and img.rgba[4, 0] == red and img.index[4, 0] == 0 and img.counts["n_filled"] == 1
    cfg = R.Config(default_truncation_distance=0.3, max_ray_length_m=5.0, min_ray_length_m=0.1)
    T = np.array([1, 0, 0, 0, 0, F(0.5) * F(0.1), F(0.5) * F(0.1)], F)
    L = R.Layer(0.1, 8)
    fr = R.integrate(L, T, img, cfg)
    row = {}
    for bi, branch in zip(fr.voxel, fr.branch):
        for k in np.nonzero((bi[:, 1] == 0) & (bi[:, 2] == 0))[0]:
            vx = int(bi[k, 0])
            slot = L.index.get((vx // 8, 0, 0), -1)
            held = (L.distance[slot, vx % 8], L.weight[slot, vx % 8], L.rgba[slot, vx % 8]) if slot >= 0 else None
            row[vx] = (int(branch[k]), held)
    # vx = 9: x = 0.95, sdf = 0.05 inside the band: the voxel becomes (sdf, 1, the cell's colour)
    assert row[9] == (R.UPDATED, (F(1) - F(9.5) * F(0.1), F(1), red)) and abs(row[9][1][0] - 0.05) < 1e-6
    # vx = 10: sdf = -0.05: behind the surface but not below -voxel_size: full weight
    assert row[10] == (R.UPDATED, (F(1) - F(10.5) * F(0.1), F(1), red)) and abs(row[10][1][0] + 0.05) < 1e-6
    # vx = 11: sdf = -0.15 < -0.1: the drop-off, w = 1 (0.3 - 0.15) / (0.3 - 0.1) = 0.75
    d, w, c = row[11][1]
    sdf = F(1) - F(11.5) * F(0.1)
    assert row[11][0] == R.UPDATED and abs(d + 0.15) < 1e-6 and abs(w - 0.75) < 1e-6 and c == red
    assert w == (F(1) * (F(0.3) + sdf)) / (F(0.3) - F(0.1)) and d == sdf
    # vx = 12: sdf = -0.25: w = 0.05 / 0.2 = 0.25;  vx = 13: sdf = -0.35 < -truncation: behind, untouched
    assert row[12][0] == R.UPDATED and abs(row[12][1][1] - 0.25) < 1e-6 and abs(row[12][1][0] + 0.25) < 1e-6
    assert row[13] == (R.BEHIND, (F(0), F(0), 0))
    # vx = 5: sdf = 0.45 > truncation: carved -- the distance is clamped, the colour is NOT blended;  vx = 0 alike
    assert row[5] == (R.CARVED, (F(0.3), F(1), 0)) and row[0] == (R.CARVED, (F(0.3), F(1), 0))
    # vx = -1: x = -0.05 looks backwards, into pixel (32, 4): an empty cell
    assert row[-1][0] == R.EMPTY_CELL
    assert fr.dropped_off.sum() > 0 and fr.counts["n_cleared"] == 0 and fr.counts["n_carved"] > 0
    # a voxel of the same pixel off the beam (a coarser model: 8 columns, 3 rows 0.8 rad apart): the sdf is the difference of
    # the RANGES, not of the x
    coarse = R.Model(8, 3, 0.0, 0, -0.8, 0.8)
    fc = R.integrate(R.Layer(0.1, 8), T, R.build(coarse, np.array([[1, 0, 0]], F), np.array([red], np.uint32)), cfg)
    k = np.nonzero((fc.voxel[..., 0] == 9) & (fc.voxel[..., 1] == 0) & (fc.voxel[..., 2] == 1))
    x, z = F(9.5) * F(0.1), F(1.5) * F(0.1) - T[6]
    assert fc.branch[k] == R.UPDATED and fc.sdf[k] == F(1) - np.sqrt((x * x + F(0)) + z * z) and fc.sdf[k] < F(1) - x
    # a second scan: weights add, the distance is the weighted mean (here: the same), the carved voxel stays uncoloured
    R.integrate(L, T, img, cfg)
    s1, s0 = L.index[(1, 0, 0)], L.index[(0, 0, 0)]
    assert L.weight[s1, 1] == F(2) and L.distance[s1, 1] == F(1) - F(9.5) * F(0.1) and L.rgba[s1, 1] == red
    assert L.weight[s0, 5] == F(2) and L.rgba[s0, 5] == 0
    # a return beyond max_ray_length_m: clearing, sdf = max_ray_length_m - r_v wherever r_v + truncation <= max_ray_length_m
    far = R.build(m, np.array([[6, 0, 0]], F), np.array([red], np.uint32))
    L2 = R.Layer(0.1, 8)
    fr2 = R.integrate(L2, T, far, cfg)
    on_beam = (fr2.voxel[..., 1] == 0) & (fr2.voxel[..., 2] == 0)
    vx = fr2.voxel[..., 0]
    assert (fr2.branch[on_beam & (vx >= 0) & (vx <= 46)] == R.CLEARED).all()              # x <= 4.65: 4.65 + 0.3 <= 5
    assert (fr2.branch[on_beam & (vx >= 47) & (vx <= 52)] == R.CLEAR_REFUSED).all()       # x >= 4.75
    assert (vx[on_beam].max() >= 52) and fr2.counts["n_cleared"] == fr2.counts["n_updates"] > 0 and fr2.counts["n_carved"] == 0
    assert L2.distance[L2.index[(5, 0, 0)], 0] == F(0.3) and L2.weight[L2.index[(5, 0, 0)], 0] == F(1) / (F(6) * F(6))


def test_the_image_keeps_the_nearest_return_and_of_equal_ranges_the_lowest_index():
    m = S.MODELS["64x8"]
    pts, rgba = S.scan(m)
    img = R.build(m, pts, rgba)
    c = img.counts
    assert c["n_rejected_range"] == 1 and c["n_rejected_rows"] == 1 and c["n_collided"] >= 5 and c["n_filled"] < m.width * m.height
    assert c["n_kept"] == c["n_points"] - 2 and c["n_filled"] + c["n_collided"] == c["n_kept"]
    n = len(pts)
    planted = np.arange(n - 10, n)          # zero, near, far, equal, short, above, seam x 3, the duplicate of point 7
    near, far_, equal, dup = planted[1], planted[2], planted[3], planted[9]
    cell = img.pixel_of_point[near]
    assert cell == img.pixel_of_point[far_] == img.pixel_of_point[equal] and img.index.reshape(-1)[cell] == near
    assert img.range.reshape(-1)[cell] == F(0.7) and img.rgba.reshape(-1)[cell] == rgba[near] != rgba[equal]
    assert img.pixel_of_point[dup] == img.pixel_of_point[7] and img.index.reshape(-1)[img.pixel_of_point[7]] == 7
    assert img.pixel_of_point[planted[0]] == -1 and img.pixel_of_point[planted[5]] == -1
    # the seam points land in column 0 of the Ouster-like model (it looks backwards) and in one column of the other
    assert set((img.pixel_of_point[planted[6:9]] % m.width).tolist()) == {0}
    other = S.MODELS["128x16"]
    cols = R.build(other, pts, rgba).pixel_of_point[planted[6:8]] % other.width
    assert cols[0] == cols[1]
    # every filled cell holds the smallest range of the points of its pixel
    r = R.norm3(pts[:, 0], pts[:, 1], pts[:, 2])
    for cell in np.unique(img.pixel_of_point[img.pixel_of_point >= 0]):
        assert img.range.reshape(-1)[cell] == r[img.pixel_of_point == cell].min()


def _poses():
    rng = np.random.default_rng(12)
    yaw = lambda a: S.quat([0, 0, 1], a)
    out = [S.IDENTITY, S.pose(yaw(np.pi / 2), [0.3, -0.2, 0.1]), S.pose(yaw(np.pi), [1.0, 2.0, -0.5]),
           S.pose(yaw(-np.pi / 2), [0, 0, 0]), S.TILTED, S.far_from_origin(S.TILTED),
           S.pose(S.quat([1, 0, 0], np.pi / 2), [-40 * 0.8 - 0.3, -40 * 0.8 - 0.1, -40 * 0.8 - 0.7]),
           S.pose(S.quat([0, 1, 0], np.pi), [-32.0, -32.0, -32.0])]
    for _ in range(6):
        q = rng.normal(size=4)
        out.append(S.pose(q / np.linalg.norm(q), rng.uniform(-60, 60, 3)))
    return out


def test_the_box_equals_the_restatement(capi):
    cfgs = [S.config(0.1), S.config(0.05, max_ray_length_m=2.5), S.config(0.1, max_ray_length_m=float("inf"))]
    n = 0
    for name, m in S.MODELS.items():
        img = R.build(m, *S.scan(m))
        empty = R.build(m, np.zeros((0, 3), F))
        for T in _poses():
            for cfg in cfgs:
                for vs, vps in ((0.1, 8), (0.05, 16)):
                    for counts in (img.counts, empty.counts):
                        rc, lo, hi = capi.range_image_box(m.capi(capi), counts, cfg.capi(capi), T, vs, vps)
                        code, rlo, rhi = R.box(m, counts, cfg, T, vs, vps)
                        assert rc == code == capi.OK and np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (T, lo, rlo, hi, rhi)
                        assert (hi - lo >= 2).all()
                        n += 1
    assert n >= 14 * 12
    # the sensor 40 blocks from the origin in negative coordinates: its box lies there
    m = S.MODELS["64x8"]
    rc, lo, hi = capi.range_image_box(m.capi(capi), R.build(m, *S.scan(m)).counts, cfgs[0].capi(capi), _poses()[6], 0.1, 8)
    assert rc == capi.OK and (hi < -30).all() and (lo > -50).all()


def test_the_box_holds_every_voxel_the_rules_update():
    """the check of the header's derivation: with the candidate walk widened by two blocks on every side, a changed
    voxel's block is never outside the box nor on its outermost layer -- on every scene of the GPU test, and a scan of the
    room from 14 poses"""
    def held(m, pts, rgba, cfg, T, vs, vps, what):
        img = R.build(m, pts, rgba)
        _, lo, hi = R.box(m, img.counts, cfg, T, vs, vps)
        fr = R.integrate(R.Layer(vs, vps), T, img, cfg, lo_hi=(lo - 2, hi + 2))
        blocks = fr.voxel[fr.branch >= R.UPDATED] // vps
        assert len(blocks) > 1000 and (blocks > lo).all() and (blocks < hi).all(), what

    for name in S.CASES:
        held(*S.case(name), name)
    m = S.MODELS["64x8"]
    pts, rgba = S.scan(m, S.TILTED)
    for k, T in enumerate(_poses()):      # (the room moves with the sensor: the scan is the same, the layer frame is not)
        held(m, pts, rgba, S.config(0.2), T, 0.2, 8, k)


# ---- sensor sizes (S.SENSOR_MODELS: up to 4096 x 256, pitches down to 1.5 mrad)

def host_pixels(fn, cm, p):
    """the library's host pixel rule `fn` (vgx_range_image_pixel or its _beams form) on directions p [n][3] -> [n][2] (u, v)"""
    u, v = C.c_int32(), C.c_int32()
    pu, pv, ref, out = C.byref(u), C.byref(v), C.byref(cm), np.empty((len(p), 2), np.int64)
    for k, (x, y, z) in enumerate(p.tolist()):
        assert fn(ref, x, y, z, pu, pv) == 0
        out[k] = u.value, v.value
    return out


def random_directions(seed, el_lo, el_hi, n=100_000):
    """f32 [n][3]: half of them anywhere, half within and just beyond the elevations the rows cover; ranges over 12 octaves"""
    rng = np.random.default_rng(seed)
    anywhere = rng.normal(size=(n // 2, 3))
    anywhere /= np.linalg.norm(anywhere, axis=1)[:, None]
    pad = 0.2 * (el_hi - el_lo) + min(0.01, el_hi - el_lo)
    el, az = rng.uniform(el_lo - pad, min(el_hi + pad, 1.57), n - n // 2), rng.uniform(-np.pi, np.pi, n - n // 2)
    rows = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    return (np.concatenate([anywhere, rows]) * np.exp2(rng.uniform(-6, 6, (n, 1)))).astype(F)


def directions_at_elevations(targets, az=0.0):
    """-> (f32 [3 len(targets)][3], how many exact hits): for every f32 elevation in `targets` a direction at azimuth `az`
    whose elevation BY THE ANGLE RULE is bit-equal to it (where the 81 f32 neighbours of z tried hold one), the one with the
    largest elevation below it and the one with the smallest above"""
    b = np.asarray(targets, F).astype(np.float64)
    ca, sa = np.cos(az), np.sin(az)
    g = b.copy()                          # the geometric elevation the rule gives `b` for: two steps against its smooth error
    for _ in range(2):
        g -= R.atan2_rule(np.sin(g).astype(F), np.cos(g).astype(F)).astype(np.float64) - b
    x, y = (np.cos(g) * ca).astype(F)[:, None], (np.cos(g) * sa).astype(F)[:, None]
    z0 = np.sin(g).astype(F)
    z = (z0.astype(np.float64)[:, None] + np.arange(-40, 41)[None, :] * np.spacing(np.abs(z0)).astype(np.float64)[:, None]).astype(F)
    x, y = np.broadcast_to(x, z.shape), np.broadcast_to(y, z.shape)
    el = R.atan2_rule(z, np.sqrt(x * x + y * y)).astype(np.float64)
    t = b[:, None]
    rows = np.arange(len(b))
    on = np.abs(el - t).argmin(1)
    below = np.where(el < t, el, -np.inf).argmax(1)
    above = np.where(el > t, el, np.inf).argmin(1)
    assert (el[rows, below] < b).all() and (el[rows, above] > b).all()
    pick = np.concatenate([on, below, above])
    rows3 = np.concatenate([rows, rows, rows])
    return np.stack([x[rows3, pick], y[rows3, pick], z[rows3, pick]], 1), int((el[rows, on] == b).sum())


def column_and_seam_directions(m, offsets, elevations, pixel):
    """-> (f32 [n][3], the column boundaries straddled): for every given (azimuth offset, elevation) row and every column
    boundary of it, the four neighbouring directions, of 129 spaced 5e-8 rad around the boundary's f64 azimuth, between which
    `pixel` (the restated rule) changes the column -- the rule's OWN boundary, two directions either side; and directions
    either side of the +-pi seam"""
    out, straddled = [], 0
    u = np.arange(m.width)
    for off, e in zip(offsets, elevations):
        az = (float(m.azimuth_first_rad) + float(off) + (u - 0.5) / float(m.su))[:, None] + np.arange(-64, 65)[None, :] * 5e-8
        d = np.stack([np.cos(az) * np.cos(e), np.sin(az) * np.cos(e), np.sin(e) + 0 * az], -1).astype(F)
        ui = pixel(m, d[..., 0], d[..., 1], d[..., 2])[0]
        change = ui[:, 1:] != ui[:, :-1]
        straddled += int(change.any(1).sum())
        j = change.argmax(1)[:, None] + np.arange(-1, 3)[None, :]
        out.append(d[u[:, None], np.clip(j, 0, 128)].reshape(-1, 3))
        tiny = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3], F)
        for r in (1.0, 3.7):
            out.append(np.stack([np.full(10, -r, F), tiny * F(r), np.full(10, r * np.tan(e), F)], 1))
    return np.concatenate(out).astype(F), straddled


def _row_edges(m):
    """the f64 elevations of the uniform rows' boundaries, half a pitch beyond the first and the last centre included"""
    return float(m.elevation_first_rad) + (np.arange(m.height + 1) - 0.5) / float(m.sv)


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_host_pixel_rule_equals_the_restatement_at_sensor_sizes(capi, name):
    """bit for bit (pixels are integers): 1e5 random directions, directions on every row boundary by the angle rule's own
    elevation and its f32 neighbours, on every column boundary, and either side of the seam"""
    m = S.SENSOR_MODELS[name]
    assert m.check() == R.OK
    edges = _row_edges(m)
    rows = np.unique(np.linspace(0, m.height - 1, 5).astype(int))
    centres = float(m.elevation_first_rad) + rows / float(m.sv)
    near, exact = directions_at_elevations(edges.astype(F), az=0.3)
    columns, straddled = column_and_seam_directions(m, np.zeros(len(rows)), centres, R.pixel)
    p = np.concatenate([random_directions(5, edges.min(), edges.max()), near, columns])
    assert len(p) >= 100_000 + 3 * (m.height + 1) + 4 * len(rows) * m.width
    ui, vi, ok = R.pixel(m, p[:, 0], p[:, 1], p[:, 2])
    got = host_pixels(capi.load().vgx_range_image_pixel, m.capi(capi), p)
    assert np.array_equal(got[:, 0], ui) and np.array_equal(got[:, 1], vi), name
    # nothing passed on nothing: rows and no rows, every column and every row met, every column boundary straddled
    assert ok.sum() > 10_000 and (~ok).sum() > 10_000 and (vi[~ok] == -1).all()
    assert len(np.unique(ui)) == m.width and len(np.unique(vi[ok])) == m.height and straddled == len(rows) * m.width
    print(f"{name}: {len(p)} directions, {exact} of {m.height + 1} row boundaries met bit-equal")


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_every_pixel_centre_ray_maps_back_to_its_own_pixel_at_sensor_sizes(capi, name):
    """the ray through a pixel's centre, formed in f64 from the model's angles and rounded once: the f32 rule gives that
    pixel, for all pixels -- exact by construction (a centre is half a pitch from every boundary, the rule's error is
    VGX_ATAN2_RULE_MAX_ERROR and a few f32 roundings of the pixel coordinate), and held to the geometry, not to a restatement"""
    m = S.SENSOR_MODELS[name]
    v, u = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    d = m.centre(u, v).reshape(-1, 3).astype(F)
    ui, vi, ok = R.pixel(m, d[:, 0], d[:, 1], d[:, 2])
    misses = int(((ui != u.ravel()) | (vi != v.ravel()) | ~ok).sum())
    print(f"{name}: {misses} misses over {len(d)} pixel-centre rays")
    assert misses == 0
    # ... and so says the library's host form, on every 61st pixel, the first and the last column of every row
    pick = np.unique(np.concatenate([np.arange(0, len(d), 61), np.arange(m.height) * m.width, np.arange(1, m.height + 1) * m.width - 1]))
    got = host_pixels(capi.load().vgx_range_image_pixel, m.capi(capi), d[pick])
    assert np.array_equal(got[:, 0], u.ravel()[pick]) and np.array_equal(got[:, 1], v.ravel()[pick])


# the first scan of the 512 x 4 sensor: its field of view of 0.027 rad (four rows of 6.7 mrad) is a disc through the room of
# about 10 m^2 x 0.027 rad x 1.3 m mean range = 0.35 m^3: 350 voxel centres of 0.1 m, more where it runs on through the
# opening and behind the walls -- a thousand updates do not fit into it.  Every other integration updates more than 1000.
LEAST_UPDATES = {"512x4": 300}


@pytest.fixture(scope="module")
def sensor_images():
    """name -> (Model, points, rgba, Image) of the scan at TILTED, computed once and left unchanged"""
    out = {}
    for name, m in S.SENSOR_MODELS.items():
        pts, rgba = S.scan(m, S.TILTED)
        out[name] = (m, pts, rgba, R.build(m, pts, rgba))
    return out


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_the_box_holds_every_voxel_the_rules_update_at_sensor_sizes(capi, sensor_images, name):
    """the method of test_the_box_holds_every_voxel_the_rules_update at pitches down to 1.5 mrad, where the box's widening
    (reach times the pitches) is a fraction of a voxel: near the origin and far from it, with the LIBRARY's box (host only),
    which is the restatement's"""
    m, pts, rgba, img = sensor_images[name]
    cfg, vs, vps = S.config(0.1), 0.1, 8
    for T in (S.TILTED, S.far_from_origin(S.TILTED)):
        T = np.asarray(T, F)
        rc, lo, hi = capi.range_image_box(m.capi(capi), img.counts, cfg.capi(capi), T, vs, vps)
        code, rlo, rhi = R.box(m, img.counts, cfg, T, vs, vps)
        assert rc == code == capi.OK and np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (name, T, lo, rlo, hi, rhi)
        fr = R.integrate(R.Layer(vs, vps), T, img, cfg, lo_hi=(lo - 2, hi + 2))
        blocks = fr.voxel[fr.branch >= R.UPDATED] // vps
        assert len(blocks) > LEAST_UPDATES.get(name, 1000) and (blocks > lo).all() and (blocks < hi).all(), (name, T)


def test_the_sensor_sized_gpu_scenes_pass_on_something():
    """what the sensor-sized tests of tests/test_range_image_gpu.py build and integrate, in the restatement alone"""
    seen = set()
    for name in S.SENSOR_CASES:
        m, scans, cfg, vs, vps = S.sensor_case(name)
        L = R.Layer(vs, vps)
        for k, (pts, rgba, T) in enumerate(scans):
            img = R.build(m, pts, rgba)
            c = img.counts
            # an image of many workgroups, nearly full, with the planted collisions and rejections
            assert c["n_filled"] > 0.9 * m.width * m.height and c["n_collided"] >= 4 and c["n_rejected_range"] == 1 and c["n_rejected_rows"] >= 1
            fr = R.integrate(L, T, img, cfg)
            seen |= set(np.unique(fr.branch).tolist())
            least = LEAST_UPDATES.get(S.SENSOR_CASES[name][0], 1000) if k == 0 else 1000
            assert fr.counts["n_updates"] > least and fr.counts["n_candidate_blocks"] > 200, (name, k, fr.counts)
            assert fr.new_blocks > 10 if k == 0 else fr.held_blocks > 10
    assert {R.UPDATED, R.CARVED, R.CLEARED, R.BEHIND, R.EMPTY_CELL, R.OUTSIDE_ROWS, R.TOO_SHORT, R.CLEAR_REFUSED} <= seen
    big = S.SENSOR_MODELS["4096x256"]
    assert big.width * big.height == 1024 * 4 * 256                  # 1024 workgroups of the resolve, four cells a lane


def test_refusals_of_the_host_only_calls(capi):
    ok = dict(width=64, height=8, azimuth_first_rad=0.5, azimuth_clockwise=1, elevation_first_rad=0.3, elevation_last_rad=-0.3)
    check = lambda **kw: capi.range_image_check(capi.lidar_model(**{**ok, **kw}))
    ref = lambda **kw: R.Model(**{**ok, **kw}).check()
    assert check() == ref() == capi.OK and capi.range_image_check(None) == capi.ERR_INVALID
    for kw, code in [(dict(azimuth_first_rad=float("nan")), capi.ERR_INVALID), (dict(elevation_first_rad=float("inf")), capi.ERR_INVALID),
                     (dict(elevation_last_rad=float("nan")), capi.ERR_INVALID), (dict(elevation_last_rad=0.3), capi.ERR_INVALID),
                     (dict(elevation_first_rad=1.58), capi.ERR_INVALID), (dict(elevation_last_rad=-1.5707964), capi.ERR_INVALID),
                     (dict(azimuth_first_rad=3.2), capi.ERR_INVALID), (dict(width=0), capi.ERR_INVALID), (dict(height=0), capi.ERR_INVALID),
                     (dict(width=4097), capi.ERR_UNSUPPORTED), (dict(height=257), capi.ERR_UNSUPPORTED), (dict(width=3), capi.ERR_UNSUPPORTED),
                     (dict(height=1), capi.ERR_UNSUPPORTED), (dict(height=1, elevation_last_rad=0.3), capi.ERR_UNSUPPORTED)]:
        assert check(**kw) == ref(**kw) == code, kw
    assert check(width=4096, height=256) == check(width=4, height=2) == check(azimuth_first_rad=float(R.PI)) == capi.OK
    m = S.MODELS["64x8"]
    counts, cfg = R.build(m, *S.scan(m)).counts, S.config(0.1)
    box = lambda *a: capi.range_image_box(*a)[0]
    assert box(m.capi(capi), counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    assert box(None, counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi), None, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi), counts, None, S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi, width=5000), counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_UNSUPPORTED
    bad = S.IDENTITY.copy()
    bad[5] = np.nan
    assert box(m.capi(capi), counts, cfg.capi(capi), bad, 0.1, 8) == R.box(m, counts, cfg, bad, 0.1, 8)[0] == capi.ERR_INVALID
    assert box(m.capi(capi), counts, cfg.capi(capi), S.IDENTITY, 0.0, 8) == R.box(m, counts, cfg, S.IDENTITY, 0.0, 8)[0] == capi.ERR_INVALID
    assert box(m.capi(capi), counts, cfg.capi(capi), S.IDENTITY, 0.1, 12) == R.box(m, counts, cfg, S.IDENTITY, 0.1, 12)[0] == capi.ERR_INVALID
    # an unbounded max_ray_length_m is bounded by the image's largest range; an unbounded range by max_ray_length_m; both: refused
    unbounded = S.config(0.1, max_ray_length_m=float("inf"))
    assert box(m.capi(capi), counts, unbounded.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    endless = dict(counts, max_range=F(np.inf))
    assert box(m.capi(capi), endless, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    assert box(m.capi(capi), endless, unbounded.capi(capi), S.IDENTITY, 0.1, 8) == R.box(m, endless, unbounded, S.IDENTITY, 0.1, 8)[0] \
        == capi.ERR_UNSUPPORTED
    far = S.IDENTITY.copy()
    far[4] = 1e12
    assert box(m.capi(capi), counts, cfg.capi(capi), far, 0.1, 8) == R.box(m, counts, cfg, far, 0.1, 8)[0] == capi.ERR_UNSUPPORTED


def test_new_symbols_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    declared = set(re.findall(r"VGX_API\s+[\w\s\*]+?\b(vgx_\w+)\s*\(", header))
    lib = os.path.join(ROOT, "voxgraph_amd", "lib", "libvoxgraph_amd.so")
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines() if line}
    for name in NEW:
        assert name in declared and name in exported and name in capi.SIGNATURES, name
        assert getattr(capi.load(), name).argtypes == capi.SIGNATURES[name][1]
    assert "typedef struct vgx_lidar_model" in header and C.sizeof(capi.LidarModel) == 24
    assert "typedef struct vgx_range_image_counts" in header and C.sizeof(capi.RangeImageCounts) == 104
    assert hasattr(capi, "RangeImage") and hasattr(capi.FastTsdfIntegrator, "integrate_range_image")
    lib = capi.load()
    T = S.IDENTITY.copy()
    assert lib.vgx_tsdf_integrate_range_image(None, T.ctypes.data_as(capi.f32p), None, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_build(None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_build_device(None, None, None, None, 0, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_stats(None, None, None) == lib.vgx_range_image_download(None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_destroy(None) == capi.ERR_INVALID


def test_the_gpu_scenes_reach_every_branch():
    """what tests/test_range_image_gpu.py integrates, in the restatement alone: no GPU test passes on nothing"""
    seen, dropped_off, new, held, collided = set(), 0, 0, 0, 0
    for name in S.CASES:
        m, pts, rgba, cfg, T, vs, vps = S.case(name)
        img = R.build(m, pts, rgba)
        L = R.Layer(vs, vps)
        first, second = R.integrate(L, T, img, cfg), R.integrate(L, T, img, cfg)
        for fr in (first, second):
            seen |= set(np.unique(fr.branch).tolist())
            dropped_off += int(fr.dropped_off.sum())
        new, held, collided = new + first.new_blocks, held + second.held_blocks, collided + img.counts["n_collided"]
        assert first.counts["n_updates"] == int((first.branch >= R.UPDATED).sum()) > 1000
        assert len(L.block_index) == first.new_blocks and second.new_blocks == 0 and second.held_blocks == first.new_blocks
        # the collided pixel and the too-short return are looked up by voxels
        cell = img.pixel_of_point[len(pts) - 9]
        assert (first.pixel == cell).sum() > 0 and (first.branch[first.pixel == img.pixel_of_point[len(pts) - 6]] == R.TOO_SHORT).any()
    # updated, carved, cleared, behind the surface, dropped off, an empty cell, outside the rows, too short -- and the
    # refusals of carving and clearing
    assert {R.UPDATED, R.CARVED, R.CLEARED, R.BEHIND, R.EMPTY_CELL, R.OUTSIDE_ROWS, R.TOO_SHORT, R.CARVE_REFUSED, R.CLEAR_REFUSED} <= seen
    assert dropped_off > 1000 and new > 100 and held > 100 and collided >= 5 * len(S.CASES)
