"""The LiDAR range image and its projective integration on the device (vgx_range_image_build and its device form,
vgx_tsdf_integrate_range_image; voxgraph_amd/csrc/vgx_range_image.hip) against the numpy restatement
(tests/range_image_ref.py), bit for bit: the image's ranges, colours, winning indices and counts; the layer's distance,
weight, colour, block index in slot order and all five counts of a frame; and the surface against the ray-cast routes'.
The same at sensor sizes, up to 4096 x 256: build, full coverage, two scans a layer, an organised message, a rendered view."""
import numpy as np
import pytest

from profiles import fuzz_range_image as Z
from tests import range_image_ref as R
from tests import range_image_scenes as S

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
        out[name] = (c, R.build(c[0], c[1], c[2]))
    return out


class Rig:
    """a layer with its integrator and a range image, destroyed together"""

    def __init__(self, capi, ctx, cfg, vs, vps, **layer_kw):
        self.capi, self.ctx = capi, ctx
        self.layer = capi.TsdfLayer(ctx, vs, vps, **layer_kw)
        self.integ = capi.FastTsdfIntegrator(ctx, cfg if not isinstance(cfg, R.Config) else cfg.capi(capi), self.layer)
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
    assert R.same_counts(image.stats(), want.counts), (image.stats(), want.counts)


# ---- the image

@pytest.mark.parametrize("name", ["ouster", "ouster_tilted", "ccw_vps16", "ccw_yaw180"])
def test_image_equals_the_restatement_in_every_form(rigs, cases, name):
    """from a decoded scan counted, from device arrays queued, and rebuilt into the same handle from a scan, queued"""
    (m, pts, rgba, cfg, T, vs, vps), want = cases[name]
    c = want.counts
    assert c["n_collided"] >= 5 and c["n_rejected_range"] == 1 and c["n_rejected_rows"] == 1 and 0 < c["n_filled"] < m.width * m.height
    r = rigs(cfg, vs, vps)
    assert R.same_counts(r.build(m, pts, rgba), c)
    _same_image(r.image, want)
    assert r.build(m, pts, rgba, through_scan=False, count=False) is None
    _same_image(r.image, want)
    # another scan into the same handle, the first again after it
    other = R.build(m, pts[::-1], rgba[::-1])
    assert r.build(m, pts[::-1], rgba[::-1], count=False) is None
    _same_image(r.image, other)
    assert R.same_counts(r.build(m, pts, rgba, through_scan=False), c)
    _same_image(r.image, want)


def test_two_points_in_one_pixel_the_seam_and_a_zero_length_point(rigs):
    m = R.Model(64, 9, 0.0, 0, -0.4, 0.4)
    r = rigs(S.config(0.1), 0.1, 8)
    d = m.centre(7, 3)
    pts = np.array([d * 2.0, d * 1.5, d * 1.5, d * 3.0, [0, 0, 0], [-1, 1e-7, 0], [-2, -1e-7, 0], [-1, 0, 0], [0, 0, 5]], F)
    rgba = np.arange(1, len(pts) + 1, dtype=np.uint32) * np.uint32(0x01010101)
    want = R.build(m, pts, rgba)
    # different ranges: the nearest wins; bit-equal ranges: the lower index wins; both seam sides and the axis: one column
    assert want.index[3, 7] == 1 and want.range[3, 7] == R.norm3(*pts[1]) == R.norm3(*pts[2]) and want.index[4, 32] == 5
    assert want.counts["n_filled"] == 2 and want.counts["n_collided"] == 5 and want.counts["n_rejected_range"] == 1 \
        and want.counts["n_rejected_rows"] == 1
    for through_scan in (True, False):
        assert R.same_counts(r.build(m, pts, rgba, through_scan), want.counts)
        _same_image(r.image, want)
    # the same with the points in the opposite order: now index 6 and 7 hold the equal ranges, 6 wins
    back = R.build(m, pts[::-1], rgba[::-1])
    assert back.index[3, 7] == 6 and back.index[4, 32] == 1
    r.build(m, pts[::-1], rgba[::-1], through_scan=False)
    _same_image(r.image, back)
    # no colours given: opaque white
    kp, pp = Z.on_device(pts)
    r.image.build_device(m.capi(r.capi), pp, None, len(pts))
    assert (r.image.download()[1][3, 7] == 255).all() and (r.image.download()[1][0, 0] == 0).all()
    # the smallest model the check accepts
    tiny = R.Model(4, 2, 0.5, 1, -0.3, 0.3)
    r.build(tiny, *S.scan(S.MODELS["64x8"]))
    _same_image(r.image, R.build(tiny, *S.scan(S.MODELS["64x8"])))


def test_a_scan_of_no_points_and_an_image_never_built(capi, ctx, rigs):
    m = S.MODELS["64x8"]
    r = rigs(S.config(0.1), 0.1, 8)
    with pytest.raises(capi.VgxError) as e:
        r.integrate(S.IDENTITY)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.VgxError):
        r.image.stats()
    empty = R.build(m, np.zeros((0, 3), F))
    for through_scan in (True, False):
        got = r.build(m, np.zeros((0, 3), F), np.zeros(0, np.uint32), through_scan)
        assert R.same_counts(got, empty.counts) and got["n_points"] == got["n_filled"] == 0 and got["max_range"] == 0
        _same_image(r.image, empty)
        got = r.integrate(S.TILTED)
        assert got == R.integrate(R.Layer(0.1, 8), S.TILTED, empty, S.config(0.1)).counts
        assert got["n_updates"] == got["n_new_blocks"] == 0 and got["n_candidate_blocks"] == 27 and r.layer.stats() == (0, 0)
    with pytest.raises(capi.VgxError) as e:
        r.image.build_device(capi.lidar_model(width=64, height=1, elevation_first_rad=0.1, elevation_last_rad=0.2), None, None, 0)
    assert e.value.code == capi.ERR_UNSUPPORTED
    _same_image(r.image, empty)                                   # (a refused build leaves the image as it was)


def test_image_from_an_undistorted_and_from_a_depth_decoded_scan(capi, ctx, rigs):
    """whatever decode filled the scan handle, the image is the restatement's image of the points the scan holds"""
    from tests import projective_scenes as D
    m = S.MODELS["128x16"]
    r = rigs(S.config(0.1), 0.1, 8)
    pts, rgba = S.scan(m)
    data, layout = S.message(pts, rgba)
    scan = capi.Scan(ctx)
    try:
        # the x coordinate doubles as the time field: t = x / 100, a track of two knots around it
        knots = [S.pose(S.quat([0, 0, 1], -0.05), [0.0, 0.0, 0.0]), S.pose(S.quat([0, 0, 1], 0.06), [0.1, 0.02, 0.0])]
        n, _ = scan.decode_undistorted(capi.scan_layout(**layout), data, capi.scan_time_field(capi.SCAN_TIME_FLOAT32, 0, 0.01), [-1.0, 1.0], knots)
        assert n == len(pts)
        moved, colours = scan.download()
        assert not np.array_equal(moved, pts)
        want = R.build(m, moved, np.ascontiguousarray(colours).view(np.uint32)[:, 0])
        assert R.same_counts(r.image.build(m.capi(capi), scan), want.counts) and want.counts["n_filled"] > 1000
        _same_image(r.image, want)
        # a depth camera's frame decoded into the same handle: a cloud around the optical axis (+z), seen by a model whose
        # rows look upwards (elevations 0.6 to 1.5 rad); the pixels next to the axis lie above the last row
        up = R.Model(128, 16, 0.0, 0, 0.6, 1.5)
        img, cam = D.frame(1, D.IDENTITY, 1)
        n, _ = scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color)
        cloud, colours = scan.download()
        want = R.build(up, cloud, np.ascontiguousarray(colours).view(np.uint32)[:, 0])
        assert r.image.build(up.capi(capi), scan, count=False) is None
        assert want.counts["n_filled"] > 500 and want.counts["n_collided"] > 500 and want.counts["n_rejected_rows"] > 0
        _same_image(r.image, want)
    finally:
        scan.destroy()


# ---- the integration

@pytest.mark.parametrize("name", list(S.CASES))
def test_scene_equals_the_restatement(capi, ctx, rigs, cases, name):
    """one scan into an empty layer, counted; the same queued into a second layer (image and frame both queued: the
    download is ordered behind them); and the scan again onto the blocks that now exist"""
    (m, pts, rgba, cfg, T, vs, vps), img = cases[name]
    ref = R.Layer(vs, vps)
    want = R.integrate(ref, T, img, cfg).counts
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
    again = R.integrate(ref, T, img, cfg)
    assert again.counts["n_new_blocks"] == 0 and again.held_blocks == want["n_new_blocks"]
    assert a.integrate(T) == again.counts
    _equal(a.layer, ref)


def test_five_scans_along_a_track_twice(rigs):
    """... and two runs of the same sequence give identical bytes"""
    m, vs, vps, cfg = S.MODELS["64x8"], 0.1, 8, S.config(0.1)
    ref, runs = R.Layer(vs, vps), [rigs(cfg, vs, vps), rigs(cfg, vs, vps)]
    new = []
    for k, T in enumerate(S.track()):
        pts, rgba = S.scan(m, T, seed=10 + k)
        want = R.integrate(ref, T, R.build(m, pts, rgba), cfg)
        new.append((want.new_blocks, want.held_blocks))
        runs[0].build(m, pts, rgba, through_scan=k % 2 == 0)
        assert runs[0].integrate(T) == want.counts
        runs[1].build(m, pts, rgba, through_scan=k % 2 == 1, count=False)
        assert runs[1].integrate(T, count=False) is None
    _equal(runs[0].layer, ref)
    assert Z.same_layer(runs[0].layer.download(), runs[1].layer.download()) is None
    assert all(n > 0 for n, _ in new) and all(h > 10 for _, h in new[1:])


def test_layer_grows_its_box_and_its_pool_during_the_call(rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["ouster_tilted"]
    ref = R.Layer(vs, vps)
    want = R.integrate(ref, T, img, cfg).counts
    r = rigs(cfg, vs, vps, lut_min=[0, 0, 0], lut_dim=[1, 1, 1], max_blocks=1)
    r.build(m, pts, rgba)
    assert r.integrate(T) == want and r.layer.growths() >= 2
    assert r.layer.stats() == (want["n_new_blocks"], 0)
    _equal(r.layer, ref)


def test_max_weight_is_reached_by_repeating_a_scan(rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["const_weight"]
    cfg = S.config(vs, use_const_weight=1, max_weight=3.0)
    ref, r = R.Layer(vs, vps), rigs(cfg, vs, vps)
    r.build(m, pts, rgba)
    for k in range(5):
        assert r.integrate(T) == R.integrate(ref, T, img, cfg).counts
    _equal(r.layer, ref)
    assert ref.weight.max() == F(3.0) and (ref.weight == F(3.0)).sum() > 1000


def test_range_image_then_ray_cast_then_range_image(capi, ctx, rigs):
    """a range-image scan, a ray-cast scan in the reproducible mode, a range-image scan, on one layer: old blocks keep their
    slots, new ones follow in candidate order; the whole layer is compared after every step the restatement covers"""
    m, vs, vps, cfg = S.MODELS["64x8"], 0.1, 8, S.config(0.1)
    poses = S.track(3)
    r = rigs(cfg.capi(capi, deterministic=1), vs, vps)
    ref = R.Layer(vs, vps)
    pts, rgba = S.scan(m, poses[0], seed=20)
    r.build(m, pts, rgba)
    assert r.integrate(poses[0]) == R.integrate(ref, poses[0], R.build(m, pts, rgba), cfg).counts
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
    ref = R.Layer.of(vs, vps, *before)
    pts, rgba = S.scan(m, poses[2], seed=22)
    want = R.integrate(ref, poses[2], R.build(m, pts, rgba), cfg)
    r.build(m, pts, rgba, through_scan=False)
    assert r.integrate(poses[2]) == want.counts and want.held_blocks > 10
    _equal(r.layer, ref)
    assert np.array_equal(r.layer.download()[0][:len(before[0])], before[0])


def test_refusals_leave_the_layer_untouched(capi, ctx, rigs, cases):
    (m, pts, rgba, cfg, T, vs, vps), img = cases["ouster"]
    ref, r = R.Layer(vs, vps), rigs(cfg, vs, vps)
    r.build(m, pts, rgba)
    assert r.integrate(T) == R.integrate(ref, T, img, cfg).counts

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
    # an unbounded max_ray_length_m is bounded by the image's largest range
    open_cfg = S.config(vs, max_ray_length_m=float("inf"))
    o, oref = rigs(open_cfg, vs, vps), R.Layer(vs, vps)
    o.build(m, pts, rgba)
    want = R.integrate(oref, T, img, open_cfg).counts
    assert o.integrate(T) == want and want["n_cleared"] == 0
    _equal(o.layer, oref)
    assert r.integrate(T) == R.integrate(ref, T, img, cfg).counts          # and the integrator works on
    _equal(r.layer, ref)


def _median_range_error(capi, ctx, layer, T, dirs, truth):
    view = capi.View(ctx, capi.view_config(flags=0, s_max=6.0, min_step=0.025, unknown_step=0.1, max_bracket=0.3))
    try:
        got = layer.render_view(view, T, dirs).download()
    finally:
        view.destroy()
    hit = got.status == capi.VIEW_HIT
    assert hit.sum() > 0.3 * len(dirs)
    return float(np.median(np.abs(got.range[hit].astype(np.float64) - truth[hit])))


def test_the_surface_is_consistent_with_the_ray_cast_routes(capi, ctx, rigs):
    """Five scans of the room along a track, integrated by this route, by the reproducible ray cast and by the racing ray
    cast; each layer rendered from a held-out pose and compared with the analytic room.  This route's median absolute range
    error is at most the reproducible ray cast's plus half a voxel (nearest-pixel lookup can displace a surface by a pitch
    times the range).  Measured on this scene (0.1 m voxels, 128 x 16 pixels): see DESIGN.md 31."""
    m, vs, vps, cfg = S.MODELS["128x16"], 0.1, 8, S.config(0.1)
    a, b, c = rigs(cfg, vs, vps), rigs(cfg.capi(capi, deterministic=1), vs, vps), rigs(cfg.capi(capi), vs, vps)
    scan = capi.Scan(ctx)
    try:
        for k, T in enumerate(S.track()):
            pts, rgba = S.scan(m, T, seed=30 + k, planted=False)
            data, layout = S.message(pts, rgba)
            scan.decode_msg(capi.scan_layout(**layout), data)
            a.image.build(m.capi(capi), scan, count=False)
            assert a.integrate(T)["n_updates"] > 1000
            assert b.integ.integrate_scan(T, scan) > 1000 and c.integ.integrate_scan(T, scan) > 1000
    finally:
        scan.destroy()
    held_out = S.pose(S.quat([0, 0, 1], 0.33), [0.22, -0.08, 0.05])
    v, u = np.meshgrid(np.arange(1, m.height - 1), np.arange(m.width), indexing="ij")
    dirs = m.centre(u + 0.37, v + 0.41).reshape(-1, 3)
    truth = S.ranges(dirs, held_out)
    errors = [_median_range_error(capi, ctx, r.layer, held_out, dirs.astype(F), truth) for r in (a, b, c)]
    print(f"median |range error|: range image {errors[0]:.5f} m, reproducible ray cast {errors[1]:.5f} m, racing ray cast {errors[2]:.5f} m")
    assert errors[0] <= errors[1] + 0.5 * vs, errors


# ---- sensor sizes (S.SENSOR_MODELS: up to 4096 x 256 -- 1024 workgroups of the resolve, a million keys --, pitches down to
# 1.5 mrad; tests/test_range_image_cpu.py holds that these scenes pass on something)

@pytest.fixture(scope="module")
def sensors():
    """(model name, scan 0 or 1) -> (Model, points, rgba, the restated Image): computed when first asked for, left unchanged"""
    made = {}

    def get(name, k=0):
        if (name, k) not in made:
            m = S.SENSOR_MODELS[name]
            pts, rgba = S.sensor_scan(m, k)
            made[name, k] = (m, pts, rgba, R.build(m, pts, rgba))
        return made[name, k]
    return get


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_sensor_sized_image_equals_the_restatement(rigs, sensors, name):
    """from a decoded scan counted and from device arrays queued: cells, colours, indices, all counts and the extremes"""
    m, pts, rgba, want = sensors(name)
    r = rigs(S.config(0.1), 0.1, 8)
    assert R.same_counts(r.build(m, pts, rgba), want.counts)
    _same_image(r.image, want)
    assert r.build(m, pts[::-1], rgba[::-1], through_scan=False, count=False) is None
    _same_image(r.image, R.build(m, pts[::-1], rgba[::-1]))


@pytest.mark.parametrize("name", list(S.SENSOR_MODELS))
def test_one_return_per_pixel_centre_fills_every_pixel(rigs, name):
    m = S.SENSOR_MODELS[name]
    n = m.width * m.height
    v, u = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    order = np.random.default_rng(9).permutation(n)
    pts = (m.centre(u, v).reshape(-1, 3) * (1.5 + np.sin(0.01 * np.arange(n)))[:, None]).astype(F)[order]
    r = rigs(S.config(0.1), 0.1, 8)
    c = r.build(m, pts, np.arange(n, dtype=np.uint32), through_scan=False)
    assert c["n_filled"] == c["n_kept"] == c["n_points"] == n and c["n_collided"] == c["n_rejected_rows"] == c["n_rejected_range"] == 0
    rng, rgba, index = r.image.download()
    index = index.reshape(-1)
    assert np.array_equal(index[order], np.arange(n))              # every pixel holds its own centre's point: a permutation
    assert np.array_equal(np.ascontiguousarray(rgba).view(np.uint32).reshape(-1), index.astype(np.uint32))
    assert np.array_equal(rng.reshape(-1)[order], R.norm3(pts[:, 0], pts[:, 1], pts[:, 2]))


@pytest.mark.parametrize("name", list(S.SENSOR_CASES))
def test_sensor_sized_scans_equal_the_restatement(rigs, sensors, name):
    """a scan at TILTED and a second from a moved pose of track() into the same layer: the block index in slot order,
    distance, weight, colour and the five counts of each frame"""
    model, far, vps = S.SENSOR_CASES[name]
    cfg, vs = S.config(0.1), 0.1
    ref, r = R.Layer(vs, vps), rigs(cfg, vs, vps)
    for k, (_, T) in enumerate(S.sensor_poses(far)):
        m, pts, rgba, img = sensors(model, k)
        want = R.integrate(ref, T, img, cfg).counts
        r.build(m, pts, rgba, through_scan=k == 1, count=False)
        assert r.integrate(T) == want
        _equal(r.layer, ref)
    assert len(ref.block_index) > 20


def test_sensor_sized_chain_from_an_organised_message_on_the_device(capi, ctx, rigs):
    """a 2048 x 128 organised PointCloud2 in device memory: decoded there, built into the image, integrated -- the image of
    the points the scan holds and the layer are the restatement's"""
    m, cfg, vs, vps = S.SENSOR_MODELS["2048x128"], S.config(0.1), 0.1, 8
    rng = np.random.default_rng(17)
    v, u = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    dirs = m.centre(u + rng.uniform(-0.3, 0.3, u.shape), v + rng.uniform(-0.3, 0.3, v.shape)).reshape(-1, 3)
    pts = (dirs * S.ranges(dirs, S.TILTED)[:, None]).astype(F)              # in pixel order: row after row of the sensor
    pts[rng.random(len(pts)) < 0.05] = np.nan                                # pixels without a return
    rgba = rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
    data, layout = S.message(pts, rgba)
    layout.update(width=m.width, height=m.height, row_step=16 * m.width)
    r = rigs(cfg, vs, vps)
    scan = capi.Scan(ctx)
    try:
        keep, address = Z.on_device(data)
        n, dropped = scan.decode_msg_device(capi.scan_layout(**layout), address, len(data))
        held = np.isfinite(pts).all(1)
        assert n == held.sum() > 0.9 * len(pts) and n + dropped == len(pts)
        assert r.image.build(m.capi(capi), scan, count=False) is None
        got = r.integrate(S.TILTED)
        cloud, colours = scan.download()
        assert np.array_equal(cloud.view(np.uint32), pts[held].view(np.uint32))
        want = R.build(m, cloud, np.ascontiguousarray(colours).view(np.uint32)[:, 0])
        assert want.counts["n_filled"] == n
        _same_image(r.image, want)
        ref = R.Layer(vs, vps)
        assert got == R.integrate(ref, S.TILTED, want, cfg).counts and got["n_updates"] > 1000
        _equal(r.layer, ref)
    finally:
        scan.destroy()


def test_a_view_rendered_with_the_sensor_sized_models_rays_fills_its_own_pixels(capi, ctx, rigs, sensors):
    """a layer rendered along the f64-formed pixel-centre rays of the 2048 x 128 model, the hits built into its image: every
    pixel whose ray returned is filled by its own ray's point, and no two returns share a pixel"""
    cfg = S.config(0.1)
    r = rigs(cfg, 0.1, 8)
    for k, (_, T) in enumerate(S.sensor_poses()):
        m, pts, rgba, _ = sensors("2048x128", k)
        r.build(m, pts, rgba, count=False)
        r.integrate(T, count=False)
    v, u = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    dirs = m.centre(u, v).reshape(-1, 3).astype(F)
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
