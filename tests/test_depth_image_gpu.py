"""The depth-image decode (vgx_scan_decode_depth_image and its device / undistorting forms, voxgraph_amd/csrc/vgx_scan.hip)
against its numpy restatement (tests/depth_image_ref.py), bit for bit: points as uint32, colours, order, every counter;
against the PointCloud2 decode of the same frame packed as a cloud; and what the scan's consumers make of a decoded
frame against what they make of the restatement's arrays."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_image_ref as D
from tests import scan_msg_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
ENCODINGS = [D.DEPTH_16UC1, D.DEPTH_32FC1]
GATE = dict(min_depth_m=D.MIN_DEPTH, max_depth_m=D.MAX_DEPTH)


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


@pytest.fixture()
def scan(capi, ctx):
    s = capi.Scan(ctx)
    yield s
    s.destroy()


def _same(got, want):
    (gp, gc), (wp, wc) = got, want[:2]
    return (gp.shape == wp.shape and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)) and gc.shape == wc.shape
            and np.array_equal(gc, wc))


def _counters(want):
    st = want[3]
    return ((len(want[0]), D.dropped(st)), (st["candidates"], st["invalid"], st["out_of_range"], st["overflowed"]),
            (st["bad_time"], st["track_overflowed"], st["clamped"]))


def _on_device(a, shift):
    """the bytes of `a` in device memory at an address that is `shift` past a multiple of 256 -> (tensor, address)"""
    import torch
    d = torch.zeros(len(a) + 16, dtype=torch.uint8, device="cuda")
    if len(a):
        d[shift:shift + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d, d.data_ptr() + shift


def _check(capi, scan, img, cam, shift=None, constant_rgba=None, row_time=None, knots=(None, None)):
    """decodes (host form, or the device form with the images `shift` bytes off alignment) and compares everything"""
    cfg = {} if constant_rgba is None else dict(constant_rgba=constant_rgba)
    want = D.decode(img, cam, row_time=row_time, knot_time=knots[0], knot_T=knots[1], **cfg)
    config = capi.scan_config(**cfg) if cfg else None
    rt = None if row_time is None else capi.depth_row_time(*row_time)
    if shift is None:
        got = scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color, config, rt, *knots)
    else:
        (kd, pd), (kc, pc) = _on_device(img.depth, shift), _on_device(img.color if img.color is not None else b"", shift)
        got = scan.decode_depth_image_device(img.layout(capi), cam.capi(capi), pd, len(img.depth), pc if img.color is not None else None,
                                             0 if img.color is None else len(img.color), config, rt, *knots)
    stats, dstats, ustats = _counters(want)
    assert got == stats and scan.stats() == stats and stats[0] + stats[1] == dstats[0]
    assert scan.depth_stats() == dstats and scan.undistort_stats() == ustats
    assert _same(scan.download(), want)
    return want


SHAPES = [(1, 1), (7, 5), (41, 25), (32, 32), (3077, 1)]     # one pixel; a thread's four straddle rows; a tile plus one; one tile; the chain


@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_shapes_equal_the_restatement(capi, scan, encoding, width, height):
    bpp = D.DEPTH_BPP[encoding]
    for seed, pad in enumerate((0, 2 * bpp, 3)):                             # tight rows, padded rows, an odd row_step
        img = D.planted_image(width, height, encoding, seed=10 * width + seed, row_pad=pad)
        assert img.row_step % 2 == (pad == 3) and len(img.depth) == height * img.row_step
        shut, opened = D.camera_for(width, height, **GATE), D.camera_for(width, height)
        want = _check(capi, scan, img, shut)
        wide = _check(capi, scan, img, opened, constant_rgba=(1, 2, 3, 254))
        for shift in (0, 1):                                                 # the device form, element loads and byte loads
            _check(capi, scan, img, shut, shift=shift)
            assert _same(scan.download(), want)
        if width * height >= 1024:
            st, so = want[3], wide[3]
            assert st["invalid"] > 20 and st["out_of_range"] > 20 and so["out_of_range"] == 0 and len(want[0]) > 500
            assert (so["overflowed"] > 0) == (encoding == D.DEPTH_32FC1)
            if encoding == D.DEPTH_32FC1:                                    # the gate's ends are included, a denormal is a depth
                assert (want[0][:, 2] == F(D.MIN_DEPTH)).any() and (want[0][:, 2] == F(D.MAX_DEPTH)).any()
                assert (wide[0][:, 2] == F(1e-40)).any()
            else:
                assert (wide[0][:, 2] == F(1) * F(0.001)).any() and (wide[0][:, 2] == F(65535) * F(0.001)).any()


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_strides(capi, scan, encoding):
    img = D.planted_image(41, 25, encoding, seed=3, row_pad=5)
    for su, sv in ((2, 3), (1, 2), (41, 1), (50, 50), (3, 1)):
        cam = D.camera_for(41, 25, stride_u=su, stride_v=sv, **GATE)
        want = _check(capi, scan, img, cam)
        assert want[3]["candidates"] == -(-41 // su) * -(-25 // sv)
        _check(capi, scan, img, cam, shift=1)
    big = D.planted_image(3077, 3, encoding, seed=4)
    _check(capi, scan, big, D.camera_for(3077, 3, stride_u=2, stride_v=2))   # (1539 candidates a row, two rows: three tiles)


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_all_invalid_and_empty_images(capi, scan, encoding):
    z = np.zeros((25, 41), np.uint16) if encoding == D.DEPTH_16UC1 else np.full((25, 41), np.nan, F)
    img = D.Image(41, 25, encoding, D.rows(z, 0, 0)[0])
    want = _check(capi, scan, img, D.camera_for(41, 25))
    assert want[3]["invalid"] == 1025 and scan.stats() == (0, 1025) and scan.device_pointers() == (None, None)
    for w, h in ((0, 0), (0, 5), (5, 0)):
        _check(capi, scan, D.planted_image(41, 25, encoding, seed=1), D.camera_for(41, 25))      # (something to forget)
        empty = D.planted_image(w, h, encoding, seed=0)
        assert scan.decode_depth_image(empty.layout(capi), D.camera_for(w, h).capi(capi), empty.depth) == (0, 0)
        assert scan.depth_stats() == (0, 0, 0, 0) and scan.download()[0].shape == (0, 3)
        assert scan.decode_depth_image_device(empty.layout(capi), D.camera_for(w, h).capi(capi), None, 0) == (0, 0)


@pytest.mark.parametrize("kind", [D.COLOR_NONE, D.COLOR_RGB8, D.COLOR_BGR8, D.COLOR_RGBA8, D.COLOR_BGRA8, D.COLOR_MONO8])
def test_colour_kinds(capi, scan, kind):
    for encoding, (w, h), pad in ((D.DEPTH_16UC1, (41, 25), 3), (D.DEPTH_32FC1, (7, 5), 1), (D.DEPTH_16UC1, (3077, 1), 0)):
        img = D.planted_image(w, h, encoding, seed=20 + kind, row_pad=2, color_kind=kind, color_pad=pad)
        cam = D.camera_for(w, h, stride_u=1 + (w == 41), **GATE)
        want = _check(capi, scan, img, cam, constant_rgba=(11, 22, 33, 44))
        _check(capi, scan, img, cam, shift=1, constant_rgba=(11, 22, 33, 44))
        if kind == D.COLOR_NONE:
            assert (want[1] == (11, 22, 33, 44)).all()
        elif w == 41:
            assert len(np.unique(want[1][:, 0])) > 50 and (want[1][:, 3] == 255).all() == (kind not in (D.COLOR_RGBA8, D.COLOR_BGRA8))


def test_host_form_over_two_staging_pieces_equals_the_device_form(capi, scan):
    """1024 x 600 16UC1 is 1.2 MB and its RGB8 image 1.8 MB: each goes up in two pieces of the pinned stage"""
    img, cam = D.room_frame(1024, 600, D.DEPTH_16UC1, seed=1)
    assert len(img.depth) > (1 << 20) and len(img.color) > (1 << 20)
    want = _check(capi, scan, img, cam)
    assert 400000 < len(want[0]) < 1024 * 600
    host = scan.download()
    _check(capi, scan, img, cam, shift=0)
    assert _same(scan.download(), host)
    _check(capi, scan, img, cam)                                             # (and again: the stage's halves in turn)


def _row_times(scale, offset_s, v):
    return np.float64(offset_s) + np.asarray(v, np.float64) * np.float64(scale)


def _turn(angle, t):
    return [np.cos(angle / 2), 0.02, -0.03, np.sin(angle / 2), *t]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_identity_track_equals_the_plain_decode_but_for_negative_zero(capi, scan, encoding):
    img = D.planted_image(41, 25, encoding, seed=5, color_kind=D.COLOR_BGR8)
    cam = D.Camera(-30.0, 31.0, 20.0, 12.0, **GATE)                          # (fx < 0: column 20's x is -0.0)
    plain = _check(capi, scan, img, cam)
    assert (plain[0].view(np.uint32) == 0x80000000).any()
    moved = _check(capi, scan, img, cam, row_time=(1e-3, 0.0), knots=([0.5], [[1, 0, 0, 0, 0, 0, 0]]))
    assert moved[3]["clamped"] == len(moved[0]) == len(plain[0]) and np.array_equal(moved[1], plain[1])
    assert np.array_equal(moved[0].view(np.uint32), (plain[0] + F(0)).view(np.uint32)) and not (moved[0].view(np.uint32) == 0x80000000).any()


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_three_knot_track(capi, scan, encoding):
    """rows before the track, inside either segment, on a knot, on the last knot and after it; the middle knot's translation
    (finite: legal) throws the 3e38 depth planted at the image's centre past the f32 range and nothing else"""
    img = D.planted_image(41, 25, encoding, seed=6, row_pad=1, color_kind=D.COLOR_RGB8, color_pad=2)
    if encoding == D.DEPTH_32FC1:
        z = img.depth.reshape(25, -1)[:, :164].copy().view(F)
        z[12, 20] = F(3e38)
        img = D.Image(41, 25, encoding, D.rows(z, 1, 0xAB)[0], img.row_step, img.color_kind, img.color, img.color_row_step)
    cam = D.camera_for(41, 25)
    scale, offset_s = 0.01, -0.03
    kt = _row_times(scale, offset_s, [3, 10, 20])
    kT = np.array([_turn(0.1, (0.1, 0, 0)), _turn(0.3, (0.2, -0.1, 3e38)), _turn(-0.2, (0.3, 0.1, 0))], F)
    want = _check(capi, scan, img, cam, row_time=(scale, offset_s), knots=(kt, kT))
    st = want[3]
    v = want[2] // 41
    assert st["clamped"] == int(((v < 3) | (v > 20)).sum()) > 50 and (v == 20).any() and (v == 10).any() and (v == 5).any()
    assert st["bad_time"] == 0 and (st["track_overflowed"] >= 1) == (encoding == D.DEPTH_32FC1)
    _check(capi, scan, img, cam, shift=1, row_time=(scale, offset_s), knots=(kt, kT))
    # a row time that overflows f64 from row 2 on: bad times, counted apart
    bad = _check(capi, scan, img, cam, row_time=(1e308, 0.0), knots=(kt, kT))
    assert bad[3]["bad_time"] > 500 and set(bad[2] // 41) == {0, 1}
    # strides: v is the row in the full image
    _check(capi, scan, img, D.camera_for(41, 25, stride_u=2, stride_v=3), row_time=(scale, offset_s), knots=(kt, kT))


def test_counters_and_the_zeros_rules_across_decode_kinds(capi, scan):
    from tests import scan_msg_scenes as S
    from tests import scan_undistort_ref as U
    from tests import scan_undistort_scenes as Z
    img = D.planted_image(41, 25, D.DEPTH_32FC1, seed=7)
    kt, kT = _row_times(0.01, 0.0, [2, 12]), np.array([_turn(0.1, (0, 0, 0)), _turn(0.2, (0.1, 0, 0))], F)
    m, f, _ = Z.message("driver48", 211, 3, seed=5)
    mkt, mkT = Z.knots(m, f, 5, seed=5)
    for k in range(2):
        want = _check(capi, scan, img, D.camera_for(41, 25), row_time=(0.01, 0.0), knots=(kt, kT))
        assert want[3]["clamped"] > 0 and want[3]["invalid"] > 0 and want[3]["overflowed"] > 0
        plain = _check(capi, scan, img, D.camera_for(41, 25, **GATE))        # no track: the undistort counters are zeros
        assert scan.undistort_stats() == (0, 0, 0) and plain[3]["out_of_range"] > 0
        cloud = U.decode(m, f, mkt, mkT)                                     # a PointCloud2: the depth counters are zeros
        scan.decode_undistorted(m.layout(capi), m.data, f.capi(capi), mkt, mkT)
        assert scan.depth_stats() == (0, 0, 0, 0) and _same(scan.download(), cloud)
        assert scan.undistort_stats() == (cloud[3]["bad_time"], cloud[3]["overflowed"], cloud[3]["clamped"])
        want = R.decode(m)
        assert scan.decode_msg(m.layout(capi), m.data) == (len(want[0]), m.n - len(want[0])) and scan.depth_stats() == (0, 0, 0, 0)
        assert scan.undistort_stats() == (0, 0, 0) and _same(scan.download(), want)
    lib = capi.load()
    assert lib.vgx_scan_depth_stats(None, None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_scan_depth_stats(scan.h, None, None, None, None) == capi.OK


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_cloud_route_gives_the_same_scan(capi, scan, encoding):
    """the frame unprojected by the restatement and packed as a PointCloud2 with NaN holes, through vgx_scan_decode_msg"""
    for (w, h), strides in (((41, 25), (1, 1)), ((41, 25), (2, 3)), ((3077, 1), (1, 1))):
        img = D.planted_image(w, h, encoding, seed=8, row_pad=2)
        cam = D.camera_for(w, h, stride_u=strides[0], stride_v=strides[1], **GATE)
        m = D.as_cloud(img, cam, D.unproject(img, cam)[0])
        cfg = capi.scan_config(constant_rgba=(5, 6, 7, 8))
        via_cloud = scan.decode_msg(m.layout(capi), m.data, cfg)
        cloud = scan.download()
        assert scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, None, cfg) == via_cloud
        assert via_cloud[0] > 0 and via_cloud[1] > 0 and _same(scan.download(), cloud) and (cloud[1] == (5, 6, 7, 8)).all()


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_integrating_a_decoded_frame_equals_integrating_the_restatements_arrays(capi, ctx, scan, encoding):
    cfg = capi.voxgraph_tsdf_config(deterministic=1)
    la, lb = capi.TsdfLayer(ctx, 0.2, 16), capi.TsdfLayer(ctx, 0.2, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    for k in range(2):
        img, cam = D.room_frame(160, 120, encoding, seed=k)
        pts, rgba, _, st = D.decode(img, cam)
        T = D.T_ROOM_OPTICAL + F(0.05 * k) * np.array([0, 0, 0, 0, 1, -1, 0], F)
        assert scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color) == (len(pts), D.dropped(st))
        na, nb = ia.integrate_scan(T, scan), ib.integratePointCloud(T, pts, rgba)
        assert na == nb > 0 and st["invalid"] > 1000 and len(pts) > 10000
    a, b = la.download(), lb.download()
    assert len(a[0]) > 5 and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    for o in (ia, ib, la, lb):
        o.destroy()


def test_registering_a_decoded_frame_equals_registering_the_restatements_arrays(capi, ctx, scan):
    from tests import scan_registration_ref as G
    layer = capi.TsdfLayer(ctx, G.VOXEL_SIZE, G.VPS)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    img, cam = D.room_frame(160, 120, D.DEPTH_16UC1, seed=3)
    pts = D.decode(img, cam)[0]
    integ.integratePointCloud(D.T_ROOM_OPTICAL, pts)
    scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color)
    ra = capi.ScanRegistration(ctx, capi.scan_registration_config(G.MAX_ABS_DISTANCE))
    rb = capi.ScanRegistration(ctx, capi.scan_registration_config(G.MAX_ABS_DISTANCE))
    ra.set_points(scan)
    rb.set_points(pts)
    prior = D.T_ROOM_OPTICAL + np.array([0, 0, 0, 0, 0.04, -0.03, 0.02], F)
    a, b = ra.evaluate(layer, prior, np.zeros(4)), rb.evaluate(layer, prior, np.zeros(4))
    flat = lambda r: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in r])
    assert np.array_equal(flat(a).view(np.uint64), flat(b).view(np.uint64)) and np.abs(flat(a)).max() > 0
    for o in (ra, rb, integ, layer):
        o.destroy()


def _refused(ctx, rc, code, text):
    msg = ctx.lib.vgx_last_error(ctx.h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_leave_the_scan_intact_and_name_their_cause(capi, ctx, scan):
    img = D.planted_image(41, 25, D.DEPTH_16UC1, seed=9, row_pad=2, color_kind=D.COLOR_RGB8, color_pad=1)
    cam = D.camera_for(41, 25, **GATE)
    kt, kT = [0.0, 0.3], np.array([_turn(0.1, (0, 0, 0)), _turn(0.2, (0.1, 0, 0))], F)
    want = _check(capi, scan, img, cam, row_time=(0.01, 0.0), knots=(kt, kT))
    stats, dstats, ustats = _counters(want)
    lib, inv = ctx.lib, capi.ERR_INVALID
    dp, cp = C.c_void_p(img.depth.ctypes.data), C.c_void_p(img.color.ctypes.data)
    nan, inf = float("nan"), float("inf")

    def decode(lay=None, camera=None, cfg=None, null=None, depth=dp, color=cp, depth_n=len(img.depth), color_n=len(img.color),
               track=False, device=False, rt=(0.01, 0.0), kt=kt, kT=kT, n_knots=None):
        layout, c = img.layout(capi, **(lay or {})), cam.capi(capi, **(camera or {}))
        a = [scan.h, None if null == "layout" else C.byref(layout), None if null == "camera" else C.byref(c),
             None if cfg is None else C.byref(cfg)]
        if track:
            view, keep = capi.scan_track_view(kt, kT)
            if n_knots is not None:
                view.n_knots = n_knots
            row_time = capi.depth_row_time(*rt)
            a += [None if null == "row_time" else C.byref(row_time), None if null == "track" else C.byref(view)]
        name = "vgx_scan_decode_depth_image" + ("_undistorted" if track else "") + ("_device" if device else "")
        return getattr(lib, name)(*a, depth, depth_n, color, color_n)

    bad_T = kT.copy()
    bad_T[1, 5] = inf
    cases = [
        (lambda: decode(null="layout"), "vgx_scan_decode_depth_image: NULL layout"),
        (lambda: decode(null="camera"), "vgx_scan_decode_depth_image: NULL camera"),
        (lambda: decode(depth=None), "vgx_scan_decode_depth_image: NULL depth image"),
        (lambda: decode(color=None), "vgx_scan_decode_depth_image: NULL colour image"),
        (lambda: decode(depth=None, device=True), "vgx_scan_decode_depth_image_device: NULL depth image"),
        (lambda: decode(color=None, device=True, track=True), "vgx_scan_decode_depth_image_undistorted_device: NULL colour image"),
        (lambda: decode(lay=dict(encoding=2)), "unknown depth encoding"),
        (lambda: decode(lay=dict(color_kind=6)), "unknown color_kind"),
        (lambda: decode(lay=dict(row_step=81)), "row_step is less than width * bytes per pixel"),
        (lambda: decode(lay=dict(color_row_step=122)), "color_row_step is less than width * bytes per pixel"),
        (lambda: decode(depth_n=len(img.depth) - 3), "depth_n_bytes is less than (height - 1) * row_step + width * bytes per pixel"),
        (lambda: decode(color_n=len(img.color) - 2), "color_n_bytes is less than (height - 1) * color_row_step + width * bytes per pixel"),
        (lambda: decode(depth_n=-1), "n_bytes is negative"),
        (lambda: decode(camera=dict(fx=0.0)), "fx or fy is zero or not finite"),
        (lambda: decode(camera=dict(fy=nan)), "fx or fy is zero or not finite"),
        (lambda: decode(camera=dict(cx=inf)), "cx or cy is not finite"),
        (lambda: decode(camera=dict(cy=nan)), "cx or cy is not finite"),
        (lambda: decode(camera=dict(depth_unit_m=0.0)), "depth_unit_m is not finite or not positive"),
        (lambda: decode(camera=dict(depth_unit_m=inf)), "depth_unit_m is not finite or not positive"),
        (lambda: decode(camera=dict(min_depth_m=nan)), "the depth bounds are NaN, negative or not min <= max"),
        (lambda: decode(camera=dict(min_depth_m=-0.5)), "the depth bounds are NaN, negative or not min <= max"),
        (lambda: decode(camera=dict(min_depth_m=9.0)), "the depth bounds are NaN, negative or not min <= max"),
        (lambda: decode(camera=dict(stride_u=0)), "a stride is less than 1"),
        (lambda: decode(camera=dict(stride_v=-2)), "a stride is less than 1"),
        (lambda: decode(cfg=capi.scan_config(intensity_max=nan)), "the intensity range is not finite or not max > min"),
        (lambda: decode(track=True, null="row_time"), "vgx_scan_decode_depth_image_undistorted: NULL row time"),
        (lambda: decode(track=True, null="track"), "vgx_scan_decode_depth_image_undistorted: NULL track"),
        (lambda: decode(track=True, rt=(nan, 0.0)), "the row time's scale or offset_s is not finite"),
        (lambda: decode(track=True, rt=(0.01, -inf)), "the row time's scale or offset_s is not finite"),
        (lambda: decode(track=True, n_knots=0), "n_knots is not in 1 .. 65536"),
        (lambda: decode(track=True, kt=[0.3, 0.3]), "the knot times are not finite and strictly ascending"),
        (lambda: decode(track=True, kT=bad_T), "a knot_T entry is not finite"),
        (lambda: decode(track=True, lay=dict(row_step=81)), "row_step is less than width * bytes per pixel"),
    ]
    for call, text in cases:
        _refused(ctx, call(), inv, text)
        assert scan.stats() == stats and scan.depth_stats() == dstats and scan.undistort_stats() == ustats, text
        assert _same(scan.download(), want), text
    _refused(ctx, decode(lay=dict(is_bigendian=1)), capi.ERR_UNSUPPORTED, "big-endian images are not supported")
    _refused(ctx, decode(lay=dict(is_bigendian=1), track=True, device=True), capi.ERR_UNSUPPORTED, "big-endian images are not supported")
    assert lib.vgx_scan_decode_depth_image(None, None, None, None, None, 0, None, 0) == inv
    assert scan.stats() == stats and scan.depth_stats() == dstats and _same(scan.download(), want)
    # the accepted neighbours: the least row steps' images, min == max, and a colour pointer that NONE does not read
    assert decode(camera=dict(min_depth_m=2.0, max_depth_m=2.0)) == capi.OK and scan.stats()[0] + scan.stats()[1] == 1025
    assert decode(lay=dict(color_kind=D.COLOR_NONE), color=None, color_n=-5) == capi.OK and scan.stats()[0] == stats[0] + ustats[0] + ustats[1]
