"""Beam-table range images without a device: the derived row boundaries on hand-worked values, the host pixel rule
(vgx_range_image_pixel_beams) against the numpy restatement (tests/beam_table_ref.py) and on hand-worked directions, the
round trip of vgx_view_rays_lidar_beams, vgx_tsdf_range_image_box_beams against the restatement's box and that box against
every voxel the rules update, every refusal, the new symbols, and that the scenes of tests/test_beam_table_gpu.py reach every
branch of the rules -- a direction and a voxel in a hole between two rows included.  At sensor sizes (S.SENSOR_MODELS, up to
256 rows): that the tables reach every arm of the row walk, two trips round its loop, a table entry above 127 and the clamped
scale; the host pixel rule on every lo_k and hi_k and the rule's own column boundaries; every pixel-centre ray; the box."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import beam_table_ref as B
from tests import beam_table_scenes as S
from tests.test_range_image_cpu import _poses, column_and_seam_directions, directions_at_elevations, host_pixels, random_directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ["vgx_range_image_check_beams", "vgx_range_image_pixel_beams", "vgx_range_image_build_beams",
       "vgx_range_image_build_beams_device", "vgx_range_image_beams", "vgx_tsdf_range_image_box_beams", "vgx_view_rays_lidar_beams"]


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


def _host_pixels(capi, m, p):
    cm = m.capi(capi)
    return np.array([capi.range_image_pixel_beams(cm, *q)[1:] for q in p.tolist()])


def test_derived_boundaries_on_hand_worked_values():
    """the table {-0.3, 0, 0.1} rad: mid = -0.15, 0.05; the outer rows reach as far out as in"""
    def f32(v):
        return np.array(v, np.float64).astype(F)
    e = f32([-0.3, 0.0, 0.1]).astype(np.float64)           # (the f32 inputs, as the rule reads them)
    for table in (e, e[::-1]):
        m = B.BeamModel(64, table)
        assert np.array_equal(m.lo, f32([e[0] - ((e[0] + e[1]) * 0.5 - e[0]), (e[0] + e[1]) * 0.5, (e[1] + e[2]) * 0.5]))
        assert np.array_equal(m.hi, f32([(e[0] + e[1]) * 0.5, (e[1] + e[2]) * 0.5, e[2] + (e[2] - (e[1] + e[2]) * 0.5)]))
        assert np.allclose(m.lo, [-0.45, -0.15, 0.05], atol=1e-7) and np.allclose(m.hi, [-0.15, 0.05, 0.15], atol=1e-7)
        assert np.array_equal(m.hi[:-1], m.lo[1:]) and m.check() == B.OK              # no gap, no overlap
        L = float(F(0.04))
        c = B.BeamModel(64, table, row_half_extent_max_rad=0.04)
        assert np.array_equal(c.lo, f32([e[0] - L, e[1] - L, e[2] - L])) and np.array_equal(c.hi, f32([e[0] + L, e[1] + L, e[2] + L]))
        assert np.allclose(c.lo, [-0.34, -0.04, 0.06], atol=1e-7) and np.allclose(c.hi, [-0.26, 0.04, 0.14], atol=1e-7)
        assert c.check() == B.OK and abs(c.ext_max - 0.08) < 1e-7 and abs(m.ext_max - 0.3) < 1e-7
    # a limit between the half gaps clips the wide gap only; a single row; the clamp to +-PI_2
    c = B.BeamModel(64, e, row_half_extent_max_rad=0.1)
    assert np.allclose(c.lo, [-0.4, -0.1, 0.05], atol=1e-7) and np.allclose(c.hi, [-0.2, 0.05, 0.15], atol=1e-7)
    one = B.BeamModel(64, [0.2], row_half_extent_max_rad=0.05)
    assert np.array_equal(one.lo, f32([float(F(0.2)) - float(F(0.05))])) and np.array_equal(one.hi, f32([float(F(0.2)) + float(F(0.05))]))
    wide = B.BeamModel(64, [-1.5, 1.5])
    assert wide.lo[0] == -B.PI_2 and wide.hi[1] == B.PI_2 and wide.check() == B.OK


def test_host_pixel_rule_equals_the_restatement_on_random_directions(capi):
    rng = np.random.default_rng(2)
    n = 0
    models = list(S.MODELS.values()) + [S.OTHER_64x8, B.uniform_as_table(B.Model(1024, 64, -3.0, 1, 0.3, -0.4))]
    for m in models:
        p = (rng.normal(size=(17000, 3)) * np.exp2(rng.uniform(-6, 6, (17000, 1)))).astype(F)
        p[::3, 2] *= F(0.2)                                    # (a third of them near the horizon, where the rows are)
        ui, vi, ok = B.beam_pixel(m, p[:, 0], p[:, 1], p[:, 2])
        got = _host_pixels(capi, m, p)
        assert np.array_equal(got[:, 0], ui) and np.array_equal(got[:, 1], vi), m.height
        assert ok.sum() > 1000 and (~ok).sum() > 1000 and ((ui < 0) == (vi < 0)).all()
        n += len(p)
    assert n >= 100_000


def test_the_pixel_rule_on_hand_worked_directions(capi):
    # 64 columns of 0.098 rad; rows at -0.2, 0, 0.3 with offsets 0.2, 0, -0.2
    ccw = B.BeamModel(64, [-0.2, 0.0, 0.3], [0.2, 0.0, -0.2], 0.0, 0)
    cw = B.BeamModel(64, [-0.2, 0.0, 0.3], [0.2, 0.0, -0.2], 0.0, 1)
    back = B.BeamModel(64, [0.3, 0.0, -0.2], [-0.2, 0.0, 0.2], float(B.PI), 1)      # column 0 backwards, the top row first
    holes = B.BeamModel(64, [-0.2, 0.0, 0.3], None, 0.0, 0, row_half_extent_max_rad=0.05)
    t = np.tan
    cases = [
        # row 1 has no offset: the axes as in the uniform model
        (ccw, (1, 0, 0), (0, 1)), (ccw, (0, 1, 0), (16, 1)), (ccw, (-1, 0, 0), (32, 1)), (cw, (0, 1, 0), (48, 1)),
        # row 0's column 0 looks along azimuth 0.2: +x is 0.2 / 0.098 = 2.04 columns back
        (ccw, (1, 0, t(-0.2)), (62, 0)), (cw, (1, 0, t(-0.2)), (2, 0)), (ccw, (np.cos(0.2), np.sin(0.2), t(-0.2)), (0, 0)),
        (ccw, (1, 0, t(0.3)), (2, 2)), (cw, (1, 0, t(0.3)), (62, 2)),
        # the +-pi seam with a non-zero offset, both spin directions: either side of -x lands in one column
        (ccw, (-1, 1e-6, t(-0.2)), (30, 0)), (ccw, (-1, -1e-6, t(-0.2)), (30, 0)), (cw, (-1, 1e-6, t(-0.2)), (34, 0)),
        (cw, (-1, -1e-6, t(-0.2)), (34, 0)), (back, (-1, 1e-6, t(-0.2)), (2, 2)), (back, (-1, -1e-6, t(-0.2)), (2, 2)),
        (back, (-1, 1e-6, t(0.3)), (62, 0)), (back, (-1, -1e-6, t(0.3)), (62, 0)), (back, (1, 0, 0), (32, 1)),
        # the z axis: rho = 0, el = +-PI_2: outside the rows, no column
        (ccw, (0, 0, 1), (-1, -1)), (ccw, (0, 0, -1), (-1, -1)),
        # the row boundaries: -0.3 | -0.1 | 0.15 | 0.45
        (ccw, (1, 0, t(-0.299)), (62, 0)), (ccw, (1, 0, t(-0.301)), (-1, -1)), (ccw, (1, 0, t(-0.101)), (62, 0)),
        (ccw, (1, 0, t(-0.099)), (0, 1)), (ccw, (1, 0, t(0.149)), (0, 1)), (ccw, (1, 0, t(0.151)), (2, 2)),
        (ccw, (1, 0, t(0.449)), (2, 2)), (ccw, (1, 0, t(0.451)), (-1, -1)), (back, (1, 0, t(0.151)), (30, 0)),
        # in a hole between two clipped rows, and back inside
        (holes, (1, 0, t(0.1)), (-1, -1)), (holes, (1, 0, t(-0.1)), (-1, -1)), (holes, (1, 0, t(0.049)), (0, 1)),
        (holes, (1, 0, t(0.051)), (-1, -1)), (holes, (1, 0, t(0.251)), (0, 2)), (holes, (1, 0, t(-0.249)), (0, 0)),
        (holes, (1, 0, t(-0.251)), (-1, -1)),
    ]
    for m, d, (u, v) in cases:
        ui, vi, ok = B.beam_pixel(m, *[F(c) for c in d])
        assert (int(ui), int(vi), bool(ok)) == (u, v, v >= 0), (d, int(ui), int(vi))
        assert capi.range_image_pixel_beams(m.capi(capi), *d) == (capi.OK, u, v), d
    # a boundary planted bit-equal to a direction's elevation: the direction belongs to the UPPER row ...
    x, y, z = F(0.8), F(-0.3), F(0.31)
    el0 = B.atan2_rule(z, np.sqrt(x * x + y * y))
    step = F(2.0 ** -6)
    # (el0 = 0.348: el0 -+ 2^-6 lie in its binade and are exact, so the midpoint is el0 itself)
    two = B.BeamModel(64, [el0 - step, el0 + step])
    assert two.hi[0] == two.lo[1] == el0
    assert int(B.beam_pixel(two, x, y, z)[1]) == 1 and capi.range_image_pixel_beams(two.capi(capi), x, y, z)[2] == 1
    flipped = B.BeamModel(64, [el0 + step, el0 - step])
    assert int(B.beam_pixel(flipped, x, y, z)[1]) == 0 and capi.range_image_pixel_beams(flipped.capi(capi), x, y, z)[2] == 0
    # ... and a direction bit-equal to hi of the top row is outside
    top = B.BeamModel(64, [el0 - 3 * step, el0 - step])
    assert top.hi[1] == el0 and not B.beam_pixel(top, x, y, z)[2]
    assert capi.range_image_pixel_beams(top.capi(capi), x, y, z) == (capi.OK, -1, -1)
    assert capi.range_image_pixel_beams(ccw.capi(capi), 0, 0, 0)[0] == capi.ERR_INVALID
    assert capi.range_image_pixel_beams(ccw.capi(capi), float("inf"), 0, 0)[0] == capi.ERR_INVALID
    assert capi.range_image_pixel_beams(None, 1, 0, 0)[0] == capi.ERR_INVALID


def _round_trip_tables():
    rng = np.random.default_rng(5)
    # 32 rows: 0.33 deg apart near the horizon, up to 9 deg apart at the edges; offsets up to 4.2 deg
    gaps = np.radians(np.concatenate([[9, 7, 5, 3, 2, 1], np.full(20, 0.33), [1, 2, 3, 5, 9]]))
    el = np.radians(-30.0) + np.concatenate([[0.0], np.cumsum(gaps)])
    off = np.radians(rng.uniform(-4.2, 4.2, 32))
    off[[0, 31]] = np.radians([4.2, -4.2])
    return [(el, off), (el[::-1], off[::-1]), (el[12:20], off[12:20]), (np.array([-0.3, 0.0, 0.4]), np.array([np.pi / 2, 0.0, -np.pi / 2]))]


def test_every_pixel_centre_ray_maps_back_to_its_own_pixel(capi):
    """vgx_view_rays_lidar_beams through the pixel rule: 0 misses -- a condition, not a tolerance"""
    misses = n = 0
    for el, off in _round_trip_tables():
        for limit in (np.inf, np.radians(0.5), np.radians(0.1)):
            for width in (4, 7, 64, 1024, 4096):
                for cw in (0, 1):
                    for first in (-float(B.PI), -1.0, 0.0, 2.5, float(B.PI)):
                        m = B.BeamModel(width, el, off, first, cw, limit)
                        assert m.check() == B.OK
                        d = m.rays()
                        ui, vi, ok = B.beam_pixel(m, d[:, 0], d[:, 1], d[:, 2])
                        v, u = np.meshgrid(np.arange(m.height), np.arange(width), indexing="ij")
                        misses += int(((ui != u.ravel()) | (vi != v.ravel())).sum())
                        n += len(d)
    print(f"round trip: {misses} misses over {n} rays")
    assert misses == 0 and n > 10_000_000
    # the library's rays are the restatement's (numpy's and libm's cos and sin may round the f64 differently: one f32 ulp),
    # and its own pixel rule maps them back
    for el, off in _round_trip_tables():
        m = B.BeamModel(64, el, off, 2.5, 1, np.radians(0.5))
        got = capi.view_rays_lidar_beams(m.capi(capi))
        assert got.shape == (m.height * 64, 3) and np.abs(got - m.rays()).max() <= 2.0 ** -23
        px = _host_pixels(capi, m, got)
        v, u = np.meshgrid(np.arange(m.height), np.arange(64), indexing="ij")
        assert np.array_equal(px[:, 0], u.ravel()) and np.array_equal(px[:, 1], v.ravel())


def test_the_box_equals_the_restatement(capi):
    cfgs = [S.config(0.1), S.config(0.05, max_ray_length_m=2.5), S.config(0.1, max_ray_length_m=float("inf"))]
    n = 0
    for name, m in S.MODELS.items():
        img = B.build(m, *S.scan(m))
        empty = B.build(m, np.zeros((0, 3), F))
        for T in _poses():
            for cfg in cfgs:
                for vs, vps in ((0.1, 8), (0.05, 16)):
                    for counts in (img.counts, empty.counts):
                        rc, lo, hi = capi.range_image_box_beams(m.capi(capi), counts, cfg.capi(capi), T, vs, vps)
                        code, rlo, rhi = B.box(m, counts, cfg, T, vs, vps)
                        assert rc == code == capi.OK and np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (name, T, lo, rlo, hi, rhi)
                        assert (hi - lo >= 2).all()
                        n += 1
    assert n >= 14 * 12 * 4
    # the widest row sets the widening: a table of the uniform centres gives the uniform box
    u = B.Model(64, 8, 0.3, 0, -0.35, 0.35)
    t = B.uniform_as_table(u)
    counts = B.build(u, *S.S.scan(u)).counts
    a = capi.range_image_box(u.capi(capi), counts, cfgs[0].capi(capi), S.TILTED, 0.1, 8)
    b = capi.range_image_box_beams(t.capi(capi), counts, cfgs[0].capi(capi), S.TILTED, 0.1, 8)
    assert a[0] == b[0] == capi.OK and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_the_box_holds_every_voxel_the_rules_update():
    """the containment argument checked: with the candidate walk widened by two blocks on every side, a changed voxel's
    block is never outside the box nor on its outermost layer -- on every scene of the GPU test, the single row and the
    4 x 2 model, and a scan of the room from 7 poses"""
    def held(m, pts, rgba, cfg, T, vs, vps, what, least=1000):
        img = B.build(m, pts, rgba)
        _, lo, hi = B.box(m, img.counts, cfg, T, vs, vps)
        fr = B.integrate(B.Layer(vs, vps), T, img, cfg, lo_hi=(lo - 2, hi + 2))
        blocks = fr.voxel[fr.branch >= B.UPDATED] // vps
        assert len(blocks) > least and (blocks > lo).all() and (blocks < hi).all(), what

    for name in S.CASES:
        held(*S.case(name), name)
    for name in ("64x1", "4x2"):
        m = S.MODELS[name]
        held(m, *S.scan(m, S.TILTED), S.config(0.1), S.TILTED, 0.1, 8, name, least=100)
    m = S.MODELS["64x8"]
    pts, rgba = S.scan(m, S.TILTED)
    for k, T in enumerate(_poses()[::2]):      # (the room moves with the sensor: the scan is the same, the layer frame is not)
        held(m, pts, rgba, S.config(0.2), T, 0.2, 8, k)


# ---- sensor sizes (S.SENSOR_MODELS: up to 256 rows, gaps down to 1 mrad; and the uniform 2048 x 128 sensor as a table)

SENSOR_TABLES = {**S.SENSOR_MODELS, "uniform_2048x128": S.UNIFORM_2048x128}
# The fields of view of these tables hold too few voxel centres for a thousand updates: 17 m^3 of room are 17 000 voxels of
# 0.1 m, of which a band of d rad around a cone holds about d / 2 (the room spans some 2 rad of elevation seen from inside
# it): 2e-3 rad (64 x 2, rows 1e-3 rad apart) some tens, 2e-5 rad (256 x 1 at a limit of 1e-5) none.  The frame is compared
# on the device all the same: its candidates, its cones and its counts.  Every other integration updates more than 1000.
LEAST_UPDATES = {"256x1_thin": -1, "64x2_close": 20}


def _elevations(pts):
    """the angle rule's elevation of every point with a range"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return B.atan2_rule(z, np.sqrt(x * x + y * y))[B.norm3(x, y, z) > 0]


def test_the_sensor_tables_reach_the_whole_row_search():
    """no scene passes on nothing: the scan directions of the sensor tables take the row walk behind the coarse table through
    no step, each of its three arms and two trips round its loop; a table entry above 127; the clamped scale"""
    met = {}
    for name, m in S.SENSOR_MODELS.items():
        assert m.check() == B.OK, name
        el = _elevations(S.scan(m, S.TILTED)[0])
        k, entry = B.walk_length(m, el[el >= m.lo[0]])
        assert (k >= entry).all()                                       # (an entry never overshoots)
        met[name] = sorted(set((k - entry).tolist()))
    print("answer row - table entry, per sensor table:", met)
    every = set().union(*met.values())
    assert {0, 1, 2, 3} <= every and max(every) >= 6
    assert max(met["512x256_descending"]) >= 2                         # (beyond the first arm with first[] entries above 127)
    # the tables of tests/beam_table_scenes.py MODELS end in the first arm or without a step: what these scenes add
    for m in S.MODELS.values():
        k, entry = B.walk_length(m, np.linspace(float(m.lo[0]), float(m.hi[-1]), 100_001).astype(F)[1:])
        assert (k - entry).max() <= 1
    assert B.coarse_table(S.SENSOR_MODELS["512x256_descending"])[1].max() > 127
    thin = S.SENSOR_MODELS["256x1_thin"]
    span = float(thin.hi[-1]) - float(thin.lo[0])
    assert B.BINS / span > 1e6 and B.coarse_table(thin)[0] == F(1e6)
    pts, rgba = S.scan(thin, S.TILTED)
    img = B.build(thin, pts, rgba)
    t = (_elevations(pts)[img.pixel_of_point[B.norm3(*pts.T) > 0] >= 0] - thin.lo[0]) * F(1e6)
    # (the row is bins 0 .. 20 of the 256; the scan's returns, 0.3 half extents around its centre, fall into several of them)
    assert img.counts["n_filled"] > 200 and 0 <= t.min() and t.max() <= 20 and len(np.unique(t.astype(int))) >= 5


@pytest.mark.parametrize("name", list(SENSOR_TABLES))
def test_host_pixel_rule_equals_the_restatement_at_sensor_sizes(capi, name):
    """bit for bit (pixels are integers): 1e5 random directions, directions whose elevation by the angle rule is every lo_k
    and hi_k and its f32 neighbours, the rule's own column boundaries in five rows, and either side of the seam"""
    m = SENSOR_TABLES[name]
    assert m.check() == B.OK
    near, exact = directions_at_elevations(np.concatenate([m.lo, m.hi]), az=0.3)
    rows = np.unique(np.linspace(0, m.height - 1, 5).astype(int))
    columns, straddled = column_and_seam_directions(m, m.offsets[rows], m.row_elevation_rad[rows].astype(np.float64), B.beam_pixel)
    p = np.concatenate([random_directions(6, float(m.lo[0]), float(m.hi[-1])), near, columns])
    ui, vi, ok = B.beam_pixel(m, p[:, 0], p[:, 1], p[:, 2])
    got = host_pixels(capi.load().vgx_range_image_pixel_beams, m.capi(capi), p)
    assert np.array_equal(got[:, 0], ui) and np.array_equal(got[:, 1], vi), name
    assert ok.sum() > 10_000 and (~ok).sum() > 10_000 and ((ui < 0) == (vi < 0)).all()
    assert len(np.unique(vi[ok])) == m.height and len(np.unique(ui[ok])) == m.width and straddled == len(rows) * m.width
    # a boundary met bit-equal belongs to the row above it (or, the top row's hi and the upper edge of a hole: to none)
    on = B.atan2_rule(near[:, 2], np.sqrt(near[:, 0] * near[:, 0] + near[:, 1] * near[:, 1]))[:2 * m.height]
    hit = on == np.concatenate([m.lo, m.hi])
    assert exact == hit.sum() > m.height // 4
    k = np.arange(m.height)
    row_of = (m.height - 1 - k) if m.descending else k
    v_on = vi[100_000:100_000 + 2 * m.height]
    assert np.array_equal(v_on[:m.height][hit[:m.height]], row_of[hit[:m.height]])
    meets = np.append(m.hi[:-1] == m.lo[1:], False)                   # hi_k is lo_{k+1}: the row above; else no row
    want_hi = np.where(meets, np.roll(row_of, -1), -1)
    assert np.array_equal(v_on[m.height:][hit[m.height:]], want_hi[hit[m.height:]])
    print(f"{name}: {len(p)} directions, {exact} of {2 * m.height} row boundaries met bit-equal")


@pytest.mark.parametrize("name", list(SENSOR_TABLES))
def test_every_pixel_centre_ray_maps_back_to_its_own_pixel_at_sensor_sizes(capi, name):
    """every ray of vgx_view_rays_lidar_beams, formed in f64 and rounded once, through the f32 rule: its own pixel, for all
    pixels -- exact by construction, as in the uniform test"""
    m = SENSOR_TABLES[name]
    d = m.rays()
    v, u = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    ui, vi, ok = B.beam_pixel(m, d[:, 0], d[:, 1], d[:, 2])
    misses = int(((ui != u.ravel()) | (vi != v.ravel())).sum())
    print(f"{name}: {misses} misses over {len(d)} pixel-centre rays")
    assert misses == 0
    got = capi.view_rays_lidar_beams(m.capi(capi))                       # the library's own rays through its own host rule
    pick =np.unique(np.concatenate([np.arange(0, len(d), 61), np.arange(m.height) * m.width, np.arange(1, m.height + 1) * m.width - 1]))
    px = host_pixels(capi.load().vgx_range_image_pixel_beams, m.capi(capi), got[pick])
    assert np.array_equal(px[:, 0], u.ravel()[pick]) and np.array_equal(px[:, 1], v.ravel()[pick])


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_the_box_holds_every_voxel_the_rules_update_at_sensor_sizes(capi, name):
    """the method of test_the_box_holds_every_voxel_the_rules_update where the widest row is a few mrad and the box's widening
    a fraction of a voxel: near the origin and far from it, with the LIBRARY's box (host only), which is the restatement's"""
    m = S.SENSOR_MODELS[name]
    pts, rgba = S.scan(m, S.TILTED)
    img, cfg, vs, vps = B.build(m, pts, rgba), S.config(0.1), 0.1, 8
    for T in (S.TILTED, S.far_from_origin(S.TILTED)):
        T = np.asarray(T, F)
        rc, lo, hi = capi.range_image_box_beams(m.capi(capi), img.counts, cfg.capi(capi), T, vs, vps)
        code, rlo, rhi = B.box(m, img.counts, cfg, T, vs, vps)
        assert rc == code == capi.OK and np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (name, T, lo, rlo, hi, rhi)
        fr = B.integrate(B.Layer(vs, vps), T, img, cfg, lo_hi=(lo - 2, hi + 2))
        blocks = fr.voxel[fr.branch >= B.UPDATED] // vps
        assert len(blocks) > LEAST_UPDATES.get(name, 1000) and (blocks > lo).all() and (blocks < hi).all(), (name, T)


def test_the_sensor_sized_gpu_scenes_pass_on_something():
    """what the sensor-sized tests of tests/test_beam_table_gpu.py build and integrate, in the restatement alone"""
    seen = set()
    for name, (model, _, _) in S.SENSOR_CASES.items():
        m, scans, cfg, vs, vps = S.sensor_case(name)
        L = B.Layer(vs, vps)
        for k, (pts, rgba, T) in enumerate(scans):
            img = B.build(m, pts, rgba)
            c = img.counts
            assert c["n_filled"] > 0.9 * m.width * m.height and c["n_collided"] >= 4 and c["n_rejected_range"] == 1 and c["n_rejected_rows"] >= 1
            fr = B.integrate(L, T, img, cfg)
            seen |= set(np.unique(fr.branch).tolist())
            assert fr.counts["n_updates"] > LEAST_UPDATES.get(model, 1000) and fr.counts["n_candidate_blocks"] > 200, (name, k, fr.counts)
            if model not in LEAST_UPDATES:
                assert fr.new_blocks > 10 if k == 0 else fr.held_blocks > 10
        if S.hole(m) is not None:                          # voxels in the holes between the clusters, rejected by rows
            assert (fr.branch == B.OUTSIDE_ROWS).sum() > 1000
    assert {B.UPDATED, B.CARVED, B.CLEARED, B.BEHIND, B.EMPTY_CELL, B.OUTSIDE_ROWS, B.TOO_SHORT, B.CLEAR_REFUSED} <= seen


def test_refusals_of_the_host_only_calls(capi):
    el, off = [-0.2, 0.0, 0.3], [0.1, 0.0, -0.1]
    ok = dict(width=64, row_elevation_rad=el, row_azimuth_offset_rad=off, azimuth_first_rad=0.5, azimuth_clockwise=1,
              row_half_extent_max_rad=np.inf)
    check = lambda **kw: capi.range_image_check_beams(capi.lidar_beam_model(**{**ok, **kw}))
    ref = lambda **kw: B.BeamModel(**{**ok, **kw}).check()
    nan, inf = float("nan"), float("inf")
    assert check() == ref() == capi.OK and capi.range_image_check_beams(None) == capi.ERR_INVALID
    null = capi.lidar_beam_model(**ok)
    null.row_elevation_rad = None
    assert capi.range_image_check_beams(null) == capi.ERR_INVALID
    I, U = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    for kw, code in [(dict(azimuth_first_rad=nan), I), (dict(azimuth_first_rad=inf), I), (dict(azimuth_first_rad=3.2), I),
                     (dict(row_elevation_rad=[-0.2, nan, 0.3]), I), (dict(row_elevation_rad=[-0.2, 0.0, inf]), I),
                     (dict(row_azimuth_offset_rad=[0.1, nan, 0.0]), I), (dict(row_azimuth_offset_rad=[0.1, -inf, 0.0]), I),
                     (dict(row_elevation_rad=[-1.58, 0.0, 0.3]), I), (dict(row_elevation_rad=[-0.2, 0.0, 1.5707964]), I),
                     (dict(row_elevation_rad=[-0.2, 0.0, 0.0]), I), (dict(row_elevation_rad=[-0.2, 0.3, 0.0]), I),
                     (dict(row_elevation_rad=[0.3, 0.0, 0.1]), I),
                     (dict(row_half_extent_max_rad=0.0), I), (dict(row_half_extent_max_rad=-0.1), I), (dict(row_half_extent_max_rad=nan), I),
                     (dict(row_azimuth_offset_rad=[0.1, 1.58, 0.0]), I), (dict(row_azimuth_offset_rad=[-1.58, 0.0, 0.0]), I),
                     (dict(width=0), I), (dict(row_elevation_rad=[], row_azimuth_offset_rad=None), I),
                     (dict(row_elevation_rad=[0.1], row_azimuth_offset_rad=None), I),                       # one row, the limit inf
                     (dict(row_elevation_rad=[0.1, 0.1 + 1e-7], row_azimuth_offset_rad=None, row_half_extent_max_rad=1e-12), I),
                     (dict(width=4097), U), (dict(width=3), U),
                     (dict(row_elevation_rad=np.linspace(-0.5, 0.5, 257), row_azimuth_offset_rad=None), U)]:
        assert check(**kw) == ref(**kw) == code, kw
    # (the last INVALID case: boundaries 1e-12 either side of 0.1 round to 0.1 itself, so a row is left no extent)
    assert check(width=4096) == check(width=4) == check(azimuth_first_rad=float(B.PI)) == check(row_azimuth_offset_rad=None) == capi.OK
    assert check(row_elevation_rad=np.linspace(-0.5, 0.5, 256), row_azimuth_offset_rad=None) == capi.OK
    assert check(row_elevation_rad=[0.1], row_azimuth_offset_rad=[float(B.PI_2)], row_half_extent_max_rad=0.2) == capi.OK   # a single row
    m = S.MODELS["64x8"]
    counts, cfg = B.build(m, *S.scan(m)).counts, S.config(0.1)
    box = lambda *a: capi.range_image_box_beams(*a)[0]
    assert box(m.capi(capi), counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    assert box(None, counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi), None, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi), counts, None, S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(m.capi(capi, width=5000), counts, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_UNSUPPORTED
    bad = S.IDENTITY.copy()
    bad[5] = np.nan
    assert box(m.capi(capi), counts, cfg.capi(capi), bad, 0.1, 8) == B.box(m, counts, cfg, bad, 0.1, 8)[0] == capi.ERR_INVALID
    assert box(m.capi(capi), counts, cfg.capi(capi), S.IDENTITY, 0.1, 12) == capi.ERR_INVALID
    unbounded, endless = S.config(0.1, max_ray_length_m=inf), dict(counts, max_range=F(np.inf))
    assert box(m.capi(capi), counts, unbounded.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    assert box(m.capi(capi), endless, unbounded.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.VgxError):
        capi.view_rays_lidar_beams(capi.lidar_beam_model(**{**ok, "width": 3}))
    assert capi.load().vgx_view_rays_lidar_beams(C.byref(capi.lidar_beam_model(**ok)), None) == capi.ERR_INVALID


def test_new_symbols_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    declared = set(re.findall(r"VGX_API\s+[\w\s\*]+?\b(vgx_\w+)\s*\(", header))
    lib = os.path.join(ROOT, "voxgraph_amd", "lib", "libvoxgraph_amd.so")
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines() if line}
    for name in NEW:
        assert name in declared and name in exported and name in capi.SIGNATURES, name
        assert getattr(capi.load(), name).argtypes == capi.SIGNATURES[name][1]
    assert "typedef struct vgx_lidar_beam_model" in header and C.sizeof(capi.LidarBeamModel) == 40
    assert "is not supported" not in header[header.index("LiDAR range images"):header.index("typedef struct vgx_lidar_model")]
    assert hasattr(capi.RangeImage, "beams") and callable(capi.lidar_beam_model)
    lib = capi.load()
    assert lib.vgx_range_image_build_beams(None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_build_beams_device(None, None, None, None, 0, None) == capi.ERR_INVALID
    assert lib.vgx_range_image_beams(None, None, None, None, None) == capi.ERR_INVALID
    # lidar_beam_model keeps its arrays alive: the structure's pointers are those of the arrays it holds
    m = capi.lidar_beam_model(64, [0.1, 0.2], [0.0, 0.01])
    assert C.addressof(m.row_elevation_rad.contents) == m._keep[0].ctypes.data and m.height == 2
    assert C.addressof(m.row_azimuth_offset_rad.contents) == m._keep[1].ctypes.data


def test_the_gpu_scenes_reach_every_branch():
    """what tests/test_beam_table_gpu.py integrates, in the restatement alone: no GPU test passes on nothing"""
    seen, dropped_off, new, held, collided, gap_voxels = set(), 0, 0, 0, 0, 0
    for name in S.CASES:
        m, pts, rgba, cfg, T, vs, vps = S.case(name)
        img = B.build(m, pts, rgba)
        L = B.Layer(vs, vps)
        first, second = B.integrate(L, T, img, cfg), B.integrate(L, T, img, cfg)
        for fr in (first, second):
            seen |= set(np.unique(fr.branch).tolist())
            dropped_off += int(fr.dropped_off.sum())
        new, held, collided = new + first.new_blocks, held + second.held_blocks, collided + img.counts["n_collided"]
        assert first.counts["n_updates"] == int((first.branch >= B.UPDATED).sum()) > 1000
        assert len(L.block_index) == first.new_blocks and second.new_blocks == 0 and second.held_blocks == first.new_blocks
        h = S.hole(m)
        n = len(pts) - (1 if h is not None else 0)
        cell = img.pixel_of_point[n - 9]                      # the collided pixel and the too-short return are looked up
        assert (first.pixel == cell).sum() > 0 and (first.branch[first.pixel == img.pixel_of_point[n - 6]] == B.TOO_SHORT).any()
        assert img.pixel_of_point[n - 5] == -1 and img.counts["n_rejected_range"] == 1
        if h is not None:
            # the planted direction in a hole is rejected by rows, and so are voxels between the lowest and the highest row
            assert img.pixel_of_point[n] == -1 and img.counts["n_rejected_rows"] == 2 and float(m.lo[0]) < h < float(m.hi[-1])
            out = first.branch == B.OUTSIDE_ROWS
            p = (first.voxel[out].astype(np.float64) + 0.5) * vs - T[4:].astype(np.float64)
            p = S.S.rotate(T[:4].astype(np.float64) * np.array([1, -1, -1, -1]), p)
            el = np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]))
            k = np.searchsorted(m.lo.astype(np.float64), el) - 1
            inside = (k >= 0) & (k < m.height - 1)
            above, below = m.hi.astype(np.float64)[np.clip(k, 0, None)], m.lo.astype(np.float64)[np.clip(k + 1, None, m.height - 1)]
            deep = inside & (el > above + 1e-3) & (el < below - 1e-3)
            gap_voxels += int(deep.sum())
        else:
            assert img.counts["n_rejected_rows"] == 1
    assert {B.UPDATED, B.CARVED, B.CLEARED, B.BEHIND, B.EMPTY_CELL, B.OUTSIDE_ROWS, B.TOO_SHORT, B.CARVE_REFUSED, B.CLEAR_REFUSED} <= seen
    assert dropped_off > 1000 and new > 100 and held > 100 and collided >= 5 * len(S.CASES) and gap_voxels > 1000
