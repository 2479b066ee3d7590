"""The beam-table range image and its projective integration on the device (vgx_range_image_build_beams and its device
form, vgx_tsdf_integrate_range_image on a table image; voxgraph_amd/csrc/vgx_range_image.hip) against the numpy restatement
(tests/beam_table_ref.py), bit for bit: the image's ranges, colours, winning indices and counts; the layer's distance,
weight, colour, block index in slot order and all five counts of a frame.  The same at sensor sizes, up to 256 rows and
rows 1.2 mrad apart: build, full coverage, the uniform 2048 x 128 sensor as a table, two scans a layer, a rendered view."""
import numpy as np
import pytest

from profiles import fuzz_beam_table as Z
from profiles.fuzz_range_image import on_device
from tests import beam_table_ref as B
from tests import beam_table_scenes as S
from tests import range_image_scenes as U

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """every scene's restated image, computed once and left unchanged: name -> (case tuple, Image)"""
    out = {}
    for name in S.CASES:
        c = S.case(name)
        out[name] = (c, B.build(c[0], c[1], c[2]))
    return out


class Rig:
    """a layer with its integrator and a range image, destroyed together"""

    def __init__(self, capi, ctx, cfg, vs, vps, **layer_kw):
        self.capi, self.ctx = capi, ctx
        self.layer = capi.TsdfLayer(ctx, vs, vps, **layer_kw)
        self.integ = capi.FastTsdfIntegrator(ctx, cfg if not isinstance(cfg, B.Config) else cfg.capi(capi), self.layer)
        self.image = capi.RangeImage(ctx)

    def build(self, m, pts, rgba, through_scan=True, count=True):
        return Z.build(self.capi, self.ctx, self.image, m, pts, rgba, through_scan, count)

    def integrate(self, T, count=True):
        return self.integ.integrate_range_image(T, self.image, count)

    def close(self):
        self.image.destroy()
        self.integ.destroy()
        self.layer.destroy()


@pytest.fixture()
def rigs(capi, ctx):
    made = []

    def make(cfg, vs, vps, **kw):
        made.append(Rig(capi, ctx, cfg, vs, vps, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


def _equal(layer, ref):
    assert Z.same_layer(layer.download(), ref.download()) is None


def _same_image(image, want):
    assert Z.same_image(image.download(), want) is None
    assert B.same_counts(image.stats(), want.counts), (image.stats(), want.counts)
    m = want.model
    if isinstance(m, B.BeamModel):
        el, off, limit = image.beams()
        assert np.array_equal(el, m.row_elevation_rad) and np.array_equal(off, m.offsets) and F(limit) == m.row_half_extent_max_rad
        s = image.model()
        assert (s.width, s.height) == (m.width, m.height)              # (a summary: the table's first and last elevation)
        assert (s.elevation_first_rad, s.elevation_last_rad) == (m.row_elevation_rad[0], m.row_elevation_rad[-1])
    else:
        assert image.beams() is None


# ---- the image

@pytest.mark.parametrize("name", list(S.MODELS))
def test_image_equals_the_restatement_in_every_form(rigs, name):
    """from a decoded scan counted, from device arrays queued, and rebuilt into the same handle from a scan, queued"""
    m = S.MODELS[name]
    pts, rgba = S.scan(m, S.TILTED)
    want = B.build(m, pts, rgba)
    c = want.counts
    assert c["n_collided"] >= 5 and c["n_rejected_range"] == 1 and c["n_rejected_rows"] >= 1 and 0 < c["n_filled"] <= m.width * m.height
    r = rigs(S.config(0.1), 0.1, 8)
    assert B.same_counts(r.build(m, pts, rgba), c)
    _same_image(r.image, want)
    assert r.build(m, pts, rgba, through_scan=False, count=False) is None
    _same_image(r.image, want)
    other = B.build(m, pts[::-1], rgba[::-1])
    assert r.build(m, pts[::-1], rgba[::-1], count=False) is None
    _same_image(r.image, other)
    assert B.same_counts(r.build(m, pts, rgba, through_scan=False), c)
    _same_image(r.image, want)


def test_a_different_table_of_the_same_height_and_uniform_between_tables(rigs):
    """a rebuild with ANOTHER table of the same height must not meet the table held; uniform, table, uniform in one handle"""
    a, b, u = S.MODELS["64x8"], S.OTHER_64x8, U.MODELS["64x8"]
    pts, rgba = S.scan(a, S.TILTED)
    want_a, want_b, want_u = B.build(a, pts, rgba), B.build(b, pts, rgba), B.build(u, pts, rgba)
    assert not np.array_equal(want_a.index, want_b.index) and not np.array_equal(want_a.index, want_u.index)
    r = rigs(S.config(0.1), 0.1, 8)
    for m, want, queued in ((u, want_u, False), (a, want_a, True), (b, want_b, True), (a, want_a, False), (u, want_u, True), (b, want_b, False)):
        r.build(m, pts, rgba, through_scan=queued, count=not queued)
        _same_image(r.image, want)
    # ... and the frames follow the image held: a table frame, a uniform frame, the other table's frame on one layer
    cfg, ref = S.config(0.1), B.Layer(0.1, 8)
    for m, want in ((a, want_a), (u, want_u), (b, want_b)):
        r.build(m, pts, rgba, count=False)
        assert r.integrate(S.TILTED) == B.integrate(ref, S.TILTED, want, cfg).counts
    _equal(r.layer, ref)


def test_two_points_in_one_pixel_the_seam_and_a_zero_length_point(rigs):
    m = B.BeamModel(64, [-0.4, -0.25, 0.0, 0.05, 0.3], [0.1, -0.1, 0.05, 0.0, -0.05], 0.0, 0, row_half_extent_max_rad=0.1)
    r = rigs(S.config(0.1), 0.1, 8)
    d = m.direction(7, 3)
    gap = np.array([np.cos(0.17), 0.0, np.sin(0.17)])               # between rows 3 (up to 0.15) and 4 (from 0.2)
    pts = np.array([d * 2.0, d * 1.5, d * 1.5, d * 3.0, [0, 0, 0], [-1, 1e-7, 0], [-2, -1e-7, 0], [-1, 0, 0], [0, 0, 5], gap], F)
    rgba = np.arange(1, len(pts) + 1, dtype=np.uint32) * np.uint32(0x01010101)
    want = B.build(m, pts, rgba)
    # different ranges: the nearest wins; bit-equal ranges: the lower index wins; both seam sides and the axis: one column
    seam = want.pixel_of_point[5]
    assert want.index[3, 7] == 1 and want.range[3, 7] == B.norm3(*pts[1]) == B.norm3(*pts[2])
    assert seam == want.pixel_of_point[6] == want.pixel_of_point[7] and want.index.reshape(-1)[seam] == 5 and seam // 64 == 2
    assert want.counts["n_filled"] == 2 and want.counts["n_collided"] == 5 and want.counts["n_rejected_range"] == 1 \
        and want.counts["n_rejected_rows"] == 2
    for through_scan in (True, False):
        assert B.same_counts(r.build(m, pts, rgba, through_scan), want.counts)
        _same_image(r.image, want)
    back = B.build(m, pts[::-1], rgba[::-1])
    assert back.index[3, 7] == 7 and back.index.reshape(-1)[seam] == 2
    r.build(m, pts[::-1], rgba[::-1], through_scan=False)
    _same_image(r.image, back)
    kp, pp = on_device(pts)
    r.image.build_device(m.capi(r.capi), pp, None, len(pts))           # no colours given: opaque white
    assert (r.image.download()[1][3, 7] == 255).all() and (r.image.download()[1][0, 0] == 0).all()


def test_a_scan_of_no_points_and_refused_models(capi, ctx, rigs):
    m = S.MODELS["64x8"]
    r = rigs(S.config(0.1), 0.1, 8)
    empty = B.build(m, np.zeros((0, 3), F))
    for through_scan in (True, False):
        got = r.build(m, np.zeros((0, 3), F), np.zeros(0, np.uint32), through_scan)
        assert B.same_counts(got, empty.counts) and got["n_points"] == got["n_filled"] == 0 and got["max_range"] == 0
        _same_image(r.image, empty)
        got = r.integrate(S.TILTED)
        assert got == B.integrate(B.Layer(0.1, 8), S.TILTED, empty, S.config(0.1)).counts
        assert got["n_updates"] == got["n_new_blocks"] == 0 and got["n_candidate_blocks"] == 27 and r.layer.stats() == (0, 0)
    for bad, code in ((capi.lidar_beam_model(64, [0.1]), capi.ERR_INVALID), (capi.lidar_beam_model(64, [0.1, 0.3, 0.2]), capi.ERR_INVALID),
                      (capi.lidar_beam_model(3, [0.1, 0.2]), capi.ERR_UNSUPPORTED)):
        with pytest.raises(capi.VgxError) as e:
            r.image.build_device(bad, None, None, 0)
        assert e.value.code == code
        _same_image(r.image, empty)                               # (a refused build leaves the image as it was)


def test_image_from_an_undistorted_and_from_a_depth_decoded_scan(capi, ctx, rigs):
    """whatever decode filled the scan handle, the image is the restatement's image of the points the scan holds"""
    from tests import projective_scenes as D
    m = S.MODELS["128x16"]
    r = rigs(S.config(0.1), 0.1, 8)
    pts, rgba = S.scan(m)
    data, layout = S.message(pts, rgba)
    scan = capi.Scan(ctx)
    try:
        knots = [S.pose(S.quat([0, 0, 1], -0.05), [0.0, 0.0, 0.0]), S.pose(S.quat([0, 0, 1], 0.06), [0.1, 0.02, 0.0])]
        n, _ = scan.decode_undistorted(capi.scan_layout(**layout), data, capi.scan_time_field(capi.SCAN_TIME_FLOAT32, 0, 0.01), [-1.0, 1.0], knots)
        assert n == len(pts)
        moved, colours = scan.download()
        assert not np.array_equal(moved, pts)
        want = B.build(m, moved, np.ascontiguousarray(colours).view(np.uint32)[:, 0])
        assert B.same_counts(r.image.build(m.capi(capi), scan), want.counts) and want.counts["n_filled"] > 1000
        _same_image(r.image, want)
        # a depth camera's frame decoded into the same handle: a cloud around +z, seen by rows that look upwards
        up = B.BeamModel(128, 0.6 + np.cumsum([0.0, 0.02, 0.1, 0.03, 0.2, 0.05, 0.15, 0.3]), 0.05 * np.cos(np.arange(8)), 0.0, 0,
                         row_half_extent_max_rad=0.06)
        img, cam = D.frame(1, D.IDENTITY, 1)
        n, _ = scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color)
        cloud, colours = scan.download()
        want = B.build(up, cloud, np.ascontiguousarray(colours).view(np.uint32)[:, 0])
        assert r.image.build(up.capi(capi), scan, count=False) is None
        assert want.counts["n_filled"] > 100 and want.counts["n_collided"] > 100 and want.counts["n_rejected_rows"] > 100
        _same_image(r.image, want)
    finally:
        scan.destroy()


# ---- the integration

@pytest.mark.parametrize("name", list(S.CASES))
def test_scene_equals_the_restatement(capi, ctx, rigs, cases, name):
    """one scan into an empty layer, counted; the same fully queued into a second layer (build, frame, download); and the
    scan again onto the blocks that now exist"""
    (m, pts, rgba, cfg, T, vs, vps), img = cases[name]
    ref = B.Layer(vs, vps)
    want = B.integrate(ref, T, img, cfg).counts
    assert want["n_updates"] > 1000 and want["n_new_blocks"] > 10
    a, b = rigs(cfg, vs, vps), rigs(cfg, vs, vps)
    a.build(m, pts, rgba)
    assert a.integrate(T) == want
    _equal(a.layer, ref)
    data, layout = S.message(pts, rgba)
    scan = capi.Scan(ctx)
    try:
        scan.decode_msg(capi.scan_layout(**layout), data)
        assert b.image.build(m.capi(capi), scan, count=False) is None and b.integrate(T, count=False) is None
        _equal(b.layer, ref)
    finally:
        scan.destroy()
    again = B.integrate(ref, T, img, cfg)
    assert again.counts["n_new_blocks"] == 0 and again.held_blocks == want["n_new_blocks"]
    assert a.integrate(T) == again.counts
    _equal(a.layer, ref)


@pytest.mark.parametrize("name", ["64x1", "4x2"])
def test_single_row_and_smallest_model_integrate(rigs, name):
    m, cfg = S.MODELS[name], S.config(0.1)
    pts, rgba = S.scan(m, S.TILTED)
    img, ref, r = B.build(m, pts, rgba), B.Layer(0.1, 8), rigs(S.config(0.1), 0.1, 8)
    want = B.integrate(ref, S.TILTED, img, cfg).counts
    assert want["n_updates"] > 100
    r.build(m, pts, rgba)
    assert r.integrate(S.TILTED) == want
    _equal(r.layer, ref)


def test_five_scans_along_a_track_twice(rigs):
    """... and two runs of the same sequence give identical bytes, block order included"""
    m, vs, vps, cfg = S.MODELS["64x8"], 0.1, 8, S.config(0.1)
    ref, runs = B.Layer(vs, vps), [rigs(cfg, vs, vps), rigs(cfg, vs, vps)]
    new = []
    for k, T in enumerate(S.track()):
        pts, rgba = S.scan(m, T, seed=10 + k)
        want = B.integrate(ref, T, B.build(m, pts, rgba), cfg)
        new.append((want.new_blocks, want.held_blocks))
        runs[0].build(m, pts, rgba, through_scan=k % 2 == 0)
        assert runs[0].integrate(T) == want.counts
        runs[1].build(m, pts, rgba, through_scan=k % 2 == 1, count=False)
        assert runs[1].integrate(T, count=False) is None
    _equal(runs[0].layer, ref)
    assert Z.same_layer(runs[0].layer.download(), runs[1].layer.download()) is None
    # (new blocks in the first scan and in later ones, held blocks from the second scan on)
    assert new[0][0] > 100 and sum(n for n, _ in new[1:]) > 10 and all(h > 100 for _, h in new[1:])


def test_layer_grows_its_box_and_its_pool_during_the_call(rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["ouster_tilted"]
    ref = B.Layer(vs, vps)
    want = B.integrate(ref, T, img, cfg).counts
    r = rigs(cfg, vs, vps, lut_min=[0, 0, 0], lut_dim=[1, 1, 1], max_blocks=1)
    r.build(m, pts, rgba)
    assert r.integrate(T) == want and r.layer.growths() >= 2
    assert r.layer.stats() == (want["n_new_blocks"], 0)
    _equal(r.layer, ref)


def test_max_weight_is_reached_by_repeating_a_scan(rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["const_weight"]
    cfg = S.config(vs, use_const_weight=1, max_weight=3.0)
    ref, r = B.Layer(vs, vps), rigs(cfg, vs, vps)
    r.build(m, pts, rgba)
    for k in range(5):
        assert r.integrate(T) == B.integrate(ref, T, img, cfg).counts
    _equal(r.layer, ref)
    assert ref.weight.max() == F(3.0) and (ref.weight == F(3.0)).sum() > 1000


def test_table_image_then_ray_cast_then_uniform_image(capi, ctx, rigs):
    """a table image, a ray-cast scan in the reproducible mode, a uniform image, on ONE layer: old blocks keep their slots,
    new ones follow in candidate order; the whole layer is compared after every step the restatement covers"""
    m, u, vs, vps, cfg = S.MODELS["64x8"], U.MODELS["64x8"], 0.1, 8, S.config(0.1)
    poses = S.track(3)
    r = rigs(cfg.capi(capi, deterministic=1), vs, vps)
    ref = B.Layer(vs, vps)
    pts, rgba = S.scan(m, poses[0], seed=20)
    r.build(m, pts, rgba)
    assert r.integrate(poses[0]) == B.integrate(ref, poses[0], B.build(m, pts, rgba), cfg).counts
    _equal(r.layer, ref)
    pts, rgba = S.scan(m, poses[1], seed=21, planted=False)
    data, layout = S.message(pts, rgba)
    scan = capi.Scan(ctx)
    try:
        scan.decode_msg(capi.scan_layout(**layout), data)
        assert r.integ.integrate_scan(poses[1], scan) > 1000
    finally:
        scan.destroy()
    before = r.layer.download()
    assert np.array_equal(before[0][:len(ref.block_index)], ref.block_index)
    ref = B.Layer.of(vs, vps, *before)
    pts, rgba = U.scan(u, poses[2], seed=22)
    want = B.integrate(ref, poses[2], B.build(u, pts, rgba), cfg)
    r.build(u, pts, rgba, through_scan=False)
    assert r.integrate(poses[2]) == want.counts and want.held_blocks > 10
    _equal(r.layer, ref)
    assert np.array_equal(r.layer.download()[0][:len(before[0])], before[0])


def test_a_view_rendered_with_the_models_rays_fills_its_own_pixels(capi, ctx, rigs):
    """a layer rendered along vgx_view_rays_lidar_beams, the hits built into a table image of the same sensor: every pixel
    whose ray returned is filled by its own ray's point, and no two returns share a pixel"""
    m, cfg = S.MODELS["128x16"], S.config(0.1)
    r = rigs(cfg, 0.1, 8)
    for k, T in enumerate(S.track(3)):
        r.build(m, *S.scan(m, T, seed=40 + k, planted=False), count=False)
        r.integrate(T, count=False)
    dirs = capi.view_rays_lidar_beams(m.capi(capi))
    view = capi.View(ctx, capi.view_config(flags=0, s_max=6.0, min_step=0.025, unknown_step=0.1, max_bracket=0.3))
    try:
        got = r.layer.render_view(view, S.track(3)[1], dirs).download()
    finally:
        view.destroy()
    hit = got.status == capi.VIEW_HIT
    assert hit.sum() > 0.3 * len(dirs)
    pts = np.where(hit[:, None], dirs * got.range[:, None], F(0)).astype(F)       # (a ray without a return: a zero-length point)
    counts = r.build(m, pts, np.zeros(len(pts), np.uint32), through_scan=False)
    assert counts["n_collided"] == 0 and counts["n_filled"] == int(hit.sum()) and counts["n_rejected_rows"] == 0
    index = r.image.download()[2].reshape(-1)
    assert np.array_equal(index, np.where(hit, np.arange(len(dirs)), -1))


def test_refusals_leave_the_layer_untouched(capi, ctx, rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["ouster"]
    ref, r = B.Layer(vs, vps), rigs(cfg, vs, vps)
    r.build(m, pts, rgba)
    assert r.integrate(T) == B.integrate(ref, T, img, cfg).counts

    def refused(code, T):
        with pytest.raises(capi.VgxError) as e:
            r.integrate(T)
        assert e.value.code == code, (e.value.code, code)
        _equal(r.layer, ref)

    bad = T.copy()
    bad[2] = np.inf
    refused(capi.ERR_INVALID, bad)
    far = T.copy()
    far[4] = 3e12
    refused(capi.ERR_UNSUPPORTED, far)
    open_cfg = S.config(vs, max_ray_length_m=float("inf"))                 # bounded by the image's largest range
    o, oref = rigs(open_cfg, vs, vps), B.Layer(vs, vps)
    o.build(m, pts, rgba)
    want = B.integrate(oref, T, img, open_cfg).counts
    assert o.integrate(T) == want and want["n_cleared"] == 0
    _equal(o.layer, oref)
    assert r.integrate(T) == B.integrate(ref, T, img, cfg).counts          # and the integrator works on
    _equal(r.layer, ref)


# ---- sensor sizes (S.SENSOR_MODELS: up to 256 rows, clusters of rows a third of a coarse bin apart -- every arm of the row
# walk and its loop --, a clamped bin scale; tests/test_beam_table_cpu.py holds that these scenes reach all of that)

@pytest.fixture(scope="module")
def sensors():
    """(table name, scan 0 or 1) -> (BeamModel, points, rgba, the restated Image): computed when first asked for, left unchanged"""
    made = {}

    def get(name, k=0):
        if (name, k) not in made:
            m = S.SENSOR_MODELS[name]
            pts, rgba = S.sensor_scan(m, k)
            made[name, k] = (m, pts, rgba, B.build(m, pts, rgba))
        return made[name, k]
    return get


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_sensor_sized_image_equals_the_restatement(rigs, sensors, name):
    """from a decoded scan counted and from device arrays queued: cells, colours, indices, all counts and the extremes"""
    m, pts, rgba, want = sensors(name)
    r = rigs(S.config(0.1), 0.1, 8)
    assert B.same_counts(r.build(m, pts, rgba), want.counts)
    _same_image(r.image, want)
    assert r.build(m, pts[::-1], rgba[::-1], through_scan=False, count=False) is None
    _same_image(r.image, B.build(m, pts[::-1], rgba[::-1]))


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_one_return_per_pixel_centre_fills_every_pixel(capi, rigs, name):
    m = S.SENSOR_MODELS[name]
    n = m.width * m.height
    order = np.random.default_rng(9).permutation(n)
    pts = (capi.view_rays_lidar_beams(m.capi(capi)) * (1.5 + np.sin(0.01 * np.arange(n))).astype(F)[:, None])[order]
    r = rigs(S.config(0.1), 0.1, 8)
    c = r.build(m, pts, np.arange(n, dtype=np.uint32), through_scan=False)
    assert c["n_filled"] == c["n_kept"] == c["n_points"] == n and c["n_collided"] == c["n_rejected_rows"] == c["n_rejected_range"] == 0
    rng, rgba, index = r.image.download()
    index = index.reshape(-1)
    assert np.array_equal(index[order], np.arange(n))              # every pixel holds its own centre's point: a permutation
    assert np.array_equal(np.ascontiguousarray(rgba).view(np.uint32).reshape(-1), index.astype(np.uint32))
    assert np.array_equal(rng.reshape(-1)[order], B.norm3(pts[:, 0], pts[:, 1], pts[:, 2]))


def test_the_uniform_2048x128_sensor_given_as_a_table_builds_the_uniform_image(rigs):
    u, t = U.SENSOR_MODELS["2048x128"], S.UNIFORM_2048x128
    pts, rgba = U.scan(u, S.TILTED)
    want = B.build(u, pts, rgba)
    as_table = B.build(t, pts, rgba)
    assert Z.same_image((as_table.range, as_table.rgba.view(np.uint8).reshape(u.height, u.width, 4), as_table.index), want) is None
    r = rigs(S.config(0.1), 0.1, 8)
    for m, through_scan in ((t, True), (u, False), (t, False)):
        assert B.same_counts(r.build(m, pts, rgba, through_scan), want.counts)
        assert Z.same_image(r.image.download(), want) is None
        assert (r.image.beams() is None) == (m is u)


@pytest.mark.parametrize("name", list(S.SENSOR_CASES))
def test_sensor_sized_scans_equal_the_restatement(rigs, sensors, name):
    """a scan at TILTED and a second from a moved pose of track() into the same layer: the block index in slot order,
    distance, weight, colour and the five counts of each frame"""
    model, far, vps = S.SENSOR_CASES[name]
    cfg, vs = S.config(0.1), 0.1
    ref, r = B.Layer(vs, vps), rigs(cfg, vs, vps)
    for k, (_, T) in enumerate(S.sensor_poses(far)):
        m, pts, rgba, img = sensors(model, k)
        want = B.integrate(ref, T, img, cfg).counts
        r.build(m, pts, rgba, through_scan=k == 1, count=False)
        assert r.integrate(T) == want
        _equal(r.layer, ref)
    assert len(ref.block_index) > 20 or model in S.THIN


def test_a_view_rendered_with_the_clustered_tables_rays_fills_its_own_pixels(capi, ctx, rigs, sensors):
    """test_a_view_rendered_with_the_models_rays_fills_its_own_pixels at 1024 x 128 with rows 1.2 mrad apart"""
    cfg = S.config(0.1)
    r = rigs(cfg, 0.1, 8)
    for k, (_, T) in enumerate(S.sensor_poses()):
        m, pts, rgba, _ = sensors("1024x128_clustered", k)
        r.build(m, pts, rgba, count=False)
        r.integrate(T, count=False)
    dirs = capi.view_rays_lidar_beams(m.capi(capi))
    view = capi.View(ctx, capi.view_config(flags=0, s_max=6.0, min_step=0.025, unknown_step=0.1, max_bracket=0.3))
    try:
        got = r.layer.render_view(view, S.track(3)[1], dirs).download()
    finally:
        view.destroy()
    hit = got.status == capi.VIEW_HIT
    assert hit.sum() > 0.3 * len(dirs)
    pts = np.where(hit[:, None], dirs * got.range[:, None], F(0)).astype(F)       # (a ray without a return: a zero-length point)
    counts = r.build(m, pts, np.zeros(len(pts), np.uint32), through_scan=False)
    assert counts["n_collided"] == 0 and counts["n_filled"] == int(hit.sum()) and counts["n_rejected_rows"] == 0
    assert np.array_equal(r.image.download()[2].reshape(-1), np.where(hit, np.arange(len(dirs)), -1))


@pytest.mark.parametrize("seed", range(100))
def test_fuzz(capi, ctx, seed):
    bad, counts = Z.run(capi, ctx, seed)
    assert bad is None, bad
    assert sum(c["n_candidate_blocks"] for c in counts) > 0
